// barrier_selftest.cpp -- TEST INFRASTRUCTURE: two toy kernels for the simulator's own check of the workgroup barrier
// (wave_sim.hpp: syncthreads; tests/test_wave_sim_selftest.py).  Host only: nothing of iris_lama_amd is compiled in.
//
//   barrier_selftest in-step      every thread passes the same barriers; prints the sum and exits 0
//   barrier_selftest mis-stepped  thread 255 reads a shared word before the store that the others see, skips the first loop body and
//                                 its barriers, and is one loop trip ahead of the others from then on -- the shape of the fault that
//                                 k_brushfire_canon had.  While both are inside the loop they meet at the SAME two call sites, a trip
//                                 apart; when thread 255 leaves the loop it meets the other lanes of its wave from another
//                                 line.  The barrier counts match (the tail makes up the skipped trip), so a simulator that
//                                 only counts arrivals runs to the end and prints 1535; this one must abort with "divergent
//                                 barrier".
#include <hip/hip_runtime.h>

#include <cstring>

__global__ void k_levels(int* out, int misstep)
{
    __shared__ int hist[4];
    __shared__ int sum;
    const int tid = (int)threadIdx.x;
    if (tid == 0) { hist[0] = 0; hist[1] = 1; hist[2] = 1; hist[3] = 0; sum = 0; }
    __syncthreads();
    // the fault: thread 0's store of hist[0] has no barrier behind it.  The fiber that completes a barrier continues first: thread 255
    // reads the 0.  (In step, every thread takes the value the store will have.)
    if (tid == 0) hist[0] = 1;
    int skipped = 0;
    for (int lev = 0; lev < 3; ++lev) {
        if ((lev == 0 && !misstep ? 1 : hist[lev]) == 0) { ++skipped; continue; }
        __syncthreads();                                  // A
        atomicAdd(&sum, lev + 1);
        __syncthreads();                                  // B
    }
    for (int k = 0; k < skipped; ++k) { __syncthreads(); __syncthreads(); }      // (so that the counts match: see above)
    __syncthreads();
    if (tid == 0) *out = sum;
}

int main(int argc, char** argv)
{
    const int misstep = argc > 1 && std::strcmp(argv[1], "mis-stepped") == 0;
    int out = -1;
    int* d_out = &out;               // (device memory is host memory here; the launch copies its arguments)
    hipLaunchKernelGGL(k_levels, dim3(1), dim3(256), 0, nullptr, d_out, misstep);
    std::printf("sum %d\n", out);
    return 0;
}
