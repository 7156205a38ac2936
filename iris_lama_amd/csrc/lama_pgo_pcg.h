// lama_pgo_pcg.h -- the damped system of lama::SimplePGO's Levenberg-Marquardt try solved ON THE DEVICE by a block-Jacobi
// preconditioned conjugate gradient (opt-in: SimplePGO::linear_solver = DevicePCG; the default stays the host's sparse LDL^T).
//
//   (H + lambda D) dx = b      H: the lower block-CSR `blocks` of k_pgo_assemble (3x3 blocks, symmetric, only the lower half stored),
//                              D = diag(H) (`diag`), b = -J^T e -- all left on the device by lama_hip_pgo_linearize_system.
//
// Nothing is factorised, so nothing fills in: the solver needs the block sparse product, axpys and dot products only.  fp64, wave64,
// +, -, *, / and comparisons only, built with -ffp-contract=off like the rest: tests/_pgo_pcg.py restates every sum below in numpy in
// the same order and the tests ask for bit-equal dx, iteration count, r.r and model decrease.  No floating-point atomics.
//
// Launch shape: ordinary bounded launches.  No kernel waits for another workgroup; the scalars of the iteration (rho, the stop
// threshold, the iteration counter, the `done` word) live in PcgState on the device, every workgroup re-sums the partials it needs
// itself, and only thread 0 of workgroup 0 writes the state.  A word of the state that a kernel writes is never one whose value the
// other workgroups of the SAME kernel depend on: rho is double-buffered by the iteration's parity, and a workgroup that sees `done`
// set early only skips work whose result is no longer used.  The host enqueues the three kernels of an iteration in batches and reads
// the state once per batch; once `done` is set the remaining launches return at once, so the result does not depend on the batch.
//
//   k_pgo_pcg_setup : one thread per pose v.  M_v = (diagonal block of v) + lambda diag(diag_v), i.e. M[c][c] = B[4c] + lambda * d[c];
//                     its inverse in closed form (adjugate / determinant; positive definite iff the three leading minors are > 0
//                     and finite, else done = BREAKDOWN and a zero inverse); x = 0, r = b, z = M^-1 r, p = z; partials of r.z, b.b.
//   k_pgo_pcg_begin : one wave: rho = sum r.z, bb = sum b.b, threshold = tol^2 * bb; bb == 0 -> done = CONVERGED at 0 iterations.
//   k_pgo_pcg_spmv  : q = (H + lambda D) p.  PCG_GROUP = 8 consecutive lanes per row (a hub's row is spread over them).  The terms of
//                     row r in order: t = 0 the diagonal, M_r p_r; then the lower blocks of the row by ascending column, B p_c; then
//                     the transposed blocks by ascending row r' > r (the transpose index built at create), B^T p_r'.  A 3x3 product is
//                     y[a] = (B[a][0] p[0] + B[a][1] p[1]) + B[a][2] p[2] (B^T: B[0][a], B[1][a], B[2][a]).  Lane g of the group adds
//                     the terms t = g, g + 8, g + 16, ... to its accumulator (from 0) in that order; the 8 accumulators are combined
//                     by the xor-shuffle tree 4, 2, 1 (v += shfl_xor(v, o)).  Lane 0 of the group stores q_r and contributes
//                     (p[0] q[0] + p[1] q[1]) + p[2] q[2] to p.q, the other lanes 0.
//   k_pgo_pcg_step  : one thread per pose.  alpha = rho / p.q (p.q not in (0, DBL_MAX]: breakdown, nothing is written);
//                     x += alpha p, r -= alpha q, z = M^-1 r; partials of r.r and r.z, each (v[0]^2 + v[1]^2) + v[2]^2 per pose.
//   k_pgo_pcg_dir   : one thread per pose.  breakdown -> done = BREAKDOWN; r.r <= threshold -> done = CONVERGED; otherwise
//                     beta = r.z / rho, p = z + beta p, rho' = r.z.  Either way but breakdown the iteration counter advances.
//   k_pgo_pcg_model : per pose (dx[0] ((lambda d[0]) dx[0] + b[0]) + dx[1] (...)) + dx[2] (...); k_pgo_sum halves the sum: the
//                     denominator of minisam's gain ratio (LevenbergMarquardtOptimizer.cpp:219-236), so the loop downloads nothing.
//
// Every dot product: per-workgroup partials in the k_pgo_error style (xor-shuffle tree 32 .. 1 over the wave, then the 4 waves in
// order), and the partials summed as k_pgo_sum does (lane l adds the partials l, l + 64, ... in order, then the xor tree 32 .. 1).
// p.q has one partial per 32 rows, the others one per 256 poses.
#pragma once
#include "lama_pgo.h"

namespace lama_dev {

constexpr int PCG_GROUP = 8;                              // lanes per row of the product
constexpr int PCG_ROWS = PGO_BLOCK / PCG_GROUP;           // rows per workgroup of k_pgo_pcg_spmv
constexpr uint32_t PCG_CONVERGED = 1, PCG_BREAKDOWN = 2;  // PcgState::done (0: running)
constexpr double PCG_DBL_MAX = 1.7976931348623157e308;

struct PcgState {
    double rho[2];        // r.z, by the parity of the iteration that READS it
    double bb;            // b.b
    double thresh;        // tol^2 * b.b
    double rr;            // r.r after the last completed iteration (b.b before the first)
    double model;         // 0.5 sum dx (lambda D dx + b)
    uint32_t done;
    uint32_t iters;
};

struct PcgPtrs {
    const double* blocks;     // [nnzb][9]  (k_pgo_assemble)
    const double* diag;       // [N][3]
    const double* b;          // [N][3]
    const int32_t* row_ptr;   // [N+1] lower pattern: the diagonal block leads its row
    const int32_t* bcol;      // [nnzb]
    const int32_t* brow;      // [nnzb]
    const int32_t* tptr;      // [N+1] transpose index: the off-diagonal blocks with column r, ...
    const int32_t* tidx;      // ... their block indices, ascending in their row
    double* minv;             // [N][9]
    double* x;                // [N][3]
    double* r;
    double* z;
    double* p;
    double* q;
    double* part_pq;          // [ceil(N / PCG_ROWS)]
    double* part_rr;          // [ceil(N / PGO_BLOCK)]
    double* part_rz;          // [ceil(N / PGO_BLOCK)]
    PcgState* st;
};

__device__ inline bool pcg_positive_finite(double v) { return v > 0.0 && v <= PCG_DBL_MAX; }     // (false for a NaN)

// the partials of one dot product, summed by every wave for itself as k_pgo_sum does: all lanes return the same value
__device__ inline double pcg_sum(const double* part, uint32_t n)
{
    double t = 0.0;
    for (uint32_t q = threadIdx.x & 63u; q < n; q += 64) t += part[q];
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    return t;
}

// one partial per workgroup in the k_pgo_error style; every thread of the workgroup calls it
__device__ inline void pcg_block_partial(double v, double* red, double* out)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) { double t = 0; for (int w = 0; w < PGO_BLOCK / 64; ++w) t += red[w]; *out = t; }
    __syncthreads();
}

__global__ __launch_bounds__(PGO_BLOCK) void k_pgo_pcg_setup(PcgPtrs s, double lambda, uint32_t N)
{
    __shared__ double red[PGO_BLOCK / 64];
    const uint32_t v = blockIdx.x * PGO_BLOCK + threadIdx.x;
    double rz = 0.0, bb = 0.0;
    if (v < N) {
        const double* B = s.blocks + 9 * (size_t)s.row_ptr[v];
        const double m00 = B[0] + lambda * s.diag[3 * (size_t)v], m11 = B[4] + lambda * s.diag[3 * (size_t)v + 1],
                     m22 = B[8] + lambda * s.diag[3 * (size_t)v + 2];
        const double m10 = B[3], m20 = B[6], m21 = B[7];              // (the lower triangle: the block is symmetric)
        const double c00 = m11 * m22 - m21 * m21, c10 = m20 * m21 - m10 * m22, c20 = m10 * m21 - m20 * m11;
        const double c11 = m00 * m22 - m20 * m20, c21 = m10 * m20 - m00 * m21, c22 = m00 * m11 - m10 * m10;
        const double det = (m00 * c00 + m10 * c10) + m20 * c20;
        double I[6] = {0, 0, 0, 0, 0, 0};                             // i00, i10, i11, i20, i21, i22
        if (pcg_positive_finite(m00) && pcg_positive_finite(c22) && pcg_positive_finite(det)) {
            I[0] = c00 / det; I[1] = c10 / det; I[2] = c11 / det; I[3] = c20 / det; I[4] = c21 / det; I[5] = c22 / det;
        }
        bool fine = I[0] > 0.0;
        for (int t = 0; t < 6; ++t) fine = fine && I[t] >= -PCG_DBL_MAX && I[t] <= PCG_DBL_MAX;
        if (!fine) {
            for (int t = 0; t < 6; ++t) I[t] = 0.0;
            s.st->done = PCG_BREAKDOWN;                               // (every such thread stores the same word)
        }
        double* W = s.minv + 9 * (size_t)v;
        W[0] = I[0]; W[1] = I[1]; W[2] = I[3];
        W[3] = I[1]; W[4] = I[2]; W[5] = I[4];
        W[6] = I[3]; W[7] = I[4]; W[8] = I[5];
        const double b0 = s.b[3 * (size_t)v], b1 = s.b[3 * (size_t)v + 1], b2 = s.b[3 * (size_t)v + 2];
        const double z0 = (W[0] * b0 + W[1] * b1) + W[2] * b2, z1 = (W[3] * b0 + W[4] * b1) + W[5] * b2,
                     z2 = (W[6] * b0 + W[7] * b1) + W[8] * b2;
        const double bv[3] = {b0, b1, b2}, zv[3] = {z0, z1, z2};
        for (int t = 0; t < 3; ++t) {
            s.x[3 * (size_t)v + t] = 0.0;
            s.r[3 * (size_t)v + t] = bv[t];
            s.z[3 * (size_t)v + t] = zv[t];
            s.p[3 * (size_t)v + t] = zv[t];
        }
        rz = (b0 * z0 + b1 * z1) + b2 * z2;
        bb = (b0 * b0 + b1 * b1) + b2 * b2;
    }
    pcg_block_partial(rz, red, s.part_rz + blockIdx.x);
    pcg_block_partial(bb, red, s.part_rr + blockIdx.x);
}

__global__ __launch_bounds__(64) void k_pgo_pcg_begin(PcgPtrs s, double tol2, uint32_t nparts)
{
    const double rho = pcg_sum(s.part_rz, nparts), bb = pcg_sum(s.part_rr, nparts);
    if (threadIdx.x != 0) return;
    const uint32_t done = uload_u32(&s.st->done);                     // (k_pgo_pcg_setup's flag)
    s.st->rho[0] = rho; s.st->rho[1] = 0.0;
    s.st->bb = bb; s.st->thresh = tol2 * bb; s.st->rr = bb; s.st->model = 0.0;
    s.st->iters = 0;
    if (done == 0) {
        if (bb == 0.0) s.st->done = PCG_CONVERGED;                    // b = 0: dx = 0 after 0 iterations
        else if (!pcg_positive_finite(bb) || !pcg_positive_finite(rho)) s.st->done = PCG_BREAKDOWN;
    }
}

__global__ __launch_bounds__(PGO_BLOCK) void k_pgo_pcg_spmv(PcgPtrs s, double lambda, uint32_t N)
{
    __shared__ double red[PGO_BLOCK / 64];
    if (uload_u32(&s.st->done) != 0) return;                          // (uniform over the launch: nobody writes `done` in this kernel)
    const uint32_t row = blockIdx.x * PCG_ROWS + threadIdx.x / PCG_GROUP;
    const int32_t g = (int32_t)(threadIdx.x % PCG_GROUP);
    double acc[3] = {0.0, 0.0, 0.0}, pq = 0.0;
    if (row < N) {
        const int32_t q0 = s.row_ptr[row], nlow = s.row_ptr[row + 1] - q0 - 1;
        const int32_t t0 = s.tptr[row], terms = 1 + nlow + (s.tptr[row + 1] - t0);
        for (int32_t t = g; t < terms; t += PCG_GROUP) {
            double y[3];
            if (t == 0) {
                const double* B = s.blocks + 9 * (size_t)q0;
                const double* pv = s.p + 3 * (size_t)row;
                const double* d = s.diag + 3 * (size_t)row;
                y[0] = ((B[0] + lambda * d[0]) * pv[0] + B[1] * pv[1]) + B[2] * pv[2];
                y[1] = (B[3] * pv[0] + (B[4] + lambda * d[1]) * pv[1]) + B[5] * pv[2];
                y[2] = (B[6] * pv[0] + B[7] * pv[1]) + (B[8] + lambda * d[2]) * pv[2];
            } else if (t <= nlow) {
                const int32_t q = q0 + t;
                const double* B = s.blocks + 9 * (size_t)q;
                const double* pv = s.p + 3 * (size_t)s.bcol[q];
                for (int a = 0; a < 3; ++a) y[a] = (B[3 * a] * pv[0] + B[3 * a + 1] * pv[1]) + B[3 * a + 2] * pv[2];
            } else {
                const int32_t q = s.tidx[t0 + (t - 1 - nlow)];
                const double* B = s.blocks + 9 * (size_t)q;
                const double* pv = s.p + 3 * (size_t)s.brow[q];
                for (int a = 0; a < 3; ++a) y[a] = (B[a] * pv[0] + B[3 + a] * pv[1]) + B[6 + a] * pv[2];
            }
            for (int a = 0; a < 3; ++a) acc[a] += y[a];
        }
    }
    for (int a = 0; a < 3; ++a)
        for (int o = PCG_GROUP / 2; o > 0; o >>= 1) acc[a] += __shfl_xor(acc[a], o, 64);
    if (row < N && g == 0) {
        const double* pv = s.p + 3 * (size_t)row;
        for (int a = 0; a < 3; ++a) s.q[3 * (size_t)row + a] = acc[a];
        pq = (pv[0] * acc[0] + pv[1] * acc[1]) + pv[2] * acc[2];
    }
    pcg_block_partial(pq, red, s.part_pq + blockIdx.x);
}

__global__ __launch_bounds__(PGO_BLOCK) void k_pgo_pcg_step(PcgPtrs s, uint32_t parity, uint32_t nparts_pq, uint32_t N)
{
    __shared__ double red[PGO_BLOCK / 64];
    if (uload_u32(&s.st->done) != 0) return;                          // (nobody writes `done` in this kernel)
    const double pq = pcg_sum(s.part_pq, nparts_pq);
    if (!pcg_positive_finite(pq)) return;                             // breakdown: k_pgo_pcg_dir flags it, x stays as it is
    const double alpha = uload_f64(&s.st->rho[parity]) / pq;
    const uint32_t v = blockIdx.x * PGO_BLOCK + threadIdx.x;
    double rr = 0.0, rz = 0.0;
    if (v < N) {
        double rv[3], zv[3];
        for (int t = 0; t < 3; ++t) {
            const size_t k = 3 * (size_t)v + t;
            s.x[k] = s.x[k] + alpha * s.p[k];
            rv[t] = s.r[k] - alpha * s.q[k];
            s.r[k] = rv[t];
        }
        const double* W = s.minv + 9 * (size_t)v;
        for (int a = 0; a < 3; ++a) {
            zv[a] = (W[3 * a] * rv[0] + W[3 * a + 1] * rv[1]) + W[3 * a + 2] * rv[2];
            s.z[3 * (size_t)v + a] = zv[a];
        }
        rr = (rv[0] * rv[0] + rv[1] * rv[1]) + rv[2] * rv[2];
        rz = (rv[0] * zv[0] + rv[1] * zv[1]) + rv[2] * zv[2];
    }
    pcg_block_partial(rr, red, s.part_rr + blockIdx.x);
    pcg_block_partial(rz, red, s.part_rz + blockIdx.x);
}

__global__ __launch_bounds__(PGO_BLOCK) void k_pgo_pcg_dir(PcgPtrs s, uint32_t iteration, uint32_t nparts_pq, uint32_t nparts, uint32_t N)
{
    // `done` may be set by workgroup 0 of this very launch: a workgroup that sees it skips an update of p that nothing reads any more
    if (uload_u32(&s.st->done) != 0) return;
    const uint32_t parity = iteration & 1u;
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    const double pq = pcg_sum(s.part_pq, nparts_pq);
    if (!pcg_positive_finite(pq)) {
        if (writer) s.st->done = PCG_BREAKDOWN;
        return;
    }
    const double rr = pcg_sum(s.part_rr, nparts), rz = pcg_sum(s.part_rz, nparts);
    const double thresh = uload_f64(&s.st->thresh);
    if (rr <= thresh) {
        if (writer) { s.st->rr = rr; s.st->iters = iteration + 1; s.st->done = PCG_CONVERGED; }
        return;
    }
    const double beta = rz / uload_f64(&s.st->rho[parity]);           // (this launch writes the OTHER parity)
    const uint32_t v = blockIdx.x * PGO_BLOCK + threadIdx.x;
    if (v < N)
        for (int t = 0; t < 3; ++t) {
            const size_t k = 3 * (size_t)v + t;
            s.p[k] = s.z[k] + beta * s.p[k];
        }
    if (writer) { s.st->rho[parity ^ 1u] = rz; s.st->rr = rr; s.st->iters = iteration + 1; }
}

__global__ __launch_bounds__(PGO_BLOCK) void k_pgo_pcg_model(PcgPtrs s, double lambda, uint32_t N)
{
    __shared__ double red[PGO_BLOCK / 64];
    const uint32_t v = blockIdx.x * PGO_BLOCK + threadIdx.x;
    double m = 0.0;
    if (v < N) {
        double t[3];
        for (int a = 0; a < 3; ++a) {
            const size_t k = 3 * (size_t)v + a;
            t[a] = s.x[k] * ((lambda * s.diag[k]) * s.x[k] + s.b[k]);
        }
        m = (t[0] + t[1]) + t[2];
    }
    pcg_block_partial(m, red, s.part_rr + blockIdx.x);
}

} // namespace lama_dev
