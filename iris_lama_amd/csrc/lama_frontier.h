// lama_frontier.h -- the FRONTIERS of a particle's occupancy map (lama_hip_map_frontiers): where mapped free space ends and unknown
// space begins, grouped into 8-connected clusters with a size, a box and a centroid -- the candidate places an exploring robot drives
// to.  The input is the trinary grid k_raster<RASTER_TRINARY> (lama_raster.h) writes for the box widened by one pixel per side (the
// halo); everything here is integers and every result is independent of the order in which lanes, waves and workgroups run.
//
//   frontier pixel: value 0 (free) and at least one of the four EDGE neighbours -1 (unknown); a halo neighbour counts like any other,
//     a neighbour that would lie below cell 0 or above cell 2^32 - 1 does not exist (FrontierBox::ox / oy / has_right / has_down).
//   cluster: an 8-connected component of the frontier pixels of the box; its label is its smallest pixel index j * width + i.
//
// Union-find labelling in a fixed number of launches (no grid-wide barrier, no workgroup ever waits for another):
//   k_frontier_mark     L[idx] = idx at a frontier pixel, FRONTIER_NONE elsewhere; the statistics slots reset; the pixels counted.
//   k_frontier_merge    each frontier pixel unites with its frontier neighbours at W, NW, N and NE: both roots are found, the larger
//                       is linked to the smaller with atomicMin, and where the returned value shows that the larger was no root any
//                       more the union goes on from that value.  A link only ever points to a smaller index, so every chase ends
//                       and the root of a finished component is its smallest index -- the label, with no extra pass.  L is read
//                       through relaxed atomic loads here: other lanes' atomics change it during the launch.
//   k_frontier_reduce   L[idx] = root, and per root the pixel count, the index sums and the box.  Lanes of a wave are consecutive
//                       pixels of a row, so a frontier along a row puts the whole wave on one root: runs of equal roots are first
//                       reduced inside the wave (a segmented shuffle reduction over run numbers) and only a run's first lane issues
//                       the atomics -- one set per run instead of one per pixel (64 times fewer on such a row).
//   k_frontier_compact  the slots with pixels >= min_pixels, listed densely in arbitrary order (one atomic per wave).
//   k_frontier_gather   their records, 40 bytes each; the host sorts them.
//
// Statistics slots: two 8-connected frontier pixels cannot lie in the same 2 x 2 block of pixels without being one component, so a
// component's root owns the slot of ITS block, (root_j / 2) * ceil(width / 2) + root_i / 2, and 28 bytes per block suffice: count
// (uint32), the two sums (uint64) and the box packed into one uint64 {min_i, min_j, max_i, max_j: 16 bits each, sides are at most
// 32766} that is updated by compare-and-swap (skipped when the box already covers the run; a failed swap retries with the value it
// returned: lock-free).  Additions, minima and maxima commute: the result is exact whatever the order.
#pragma once
#include "lama_raster.h"

namespace lama_dev {

constexpr uint32_t FRONTIER_NONE = 0xFFFFFFFFu;
constexpr uint64_t FRONTIER_BOX_EMPTY = 0x00000000FFFFFFFFull;       // min_i = min_j = 0xFFFF, max_i = max_j = 0

// the box in pixels; the widened raster is [rh][rw] and holds pixel (i, j) of the box at (i + ox, j + oy): ox / oy are 1 where the
// halo column / row before the box exists, has_right / has_down say whether the ones after it do (they are always rasterised)
struct FrontierBox { uint32_t width, height, rw, rh, ox, oy, has_right, has_down, sw, nslots; };
// what the launches share: the compacted slots' number and all frontier pixels
struct FrontierHead { uint32_t n, r0; uint64_t pixels; };
struct FrontierSlots { unsigned long long* sum_i; unsigned long long* sum_j; unsigned long long* box; uint32_t* count; };
// lama_hip_frontier (include/lama_hip.h), field by field
struct FrontierRec { uint32_t label, pixels, min_i, min_j, max_i, max_j; uint64_t sum_i, sum_j; };

__device__ inline uint32_t frontier_load(const uint32_t* L, uint32_t k) { return __hip_atomic_load(L + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of k's tree: links point to smaller indices only, so this ends after at most k steps whatever other lanes do meanwhile
__device__ inline uint32_t frontier_find(const uint32_t* L, uint32_t k)
{
    for (;;) {
        const uint32_t p = frontier_load(L, k);
        if (p == k) return k;
        k = p;
    }
}

__device__ inline void frontier_unite(uint32_t* L, uint32_t a, uint32_t b)
{
    for (;;) {
        a = frontier_find(L, a);
        b = frontier_find(L, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }          // a is the larger root
        const uint32_t old = atomicMin(L + a, b);
        if (old == a) return;                                       // a was still a root: linked
        // a had been linked to `old` (< a) meanwhile.  L[a] is now min(old, b): whichever of the two it does not point to any more
        // is joined by uniting them
        a = old;
    }
}

__global__ __launch_bounds__(256) void k_frontier_mark(FrontierBox fb, const int8_t* __restrict__ ras, uint32_t* __restrict__ L, FrontierSlots st, FrontierHead* head)
{
    const uint32_t total = fb.width * fb.height, idx = blockIdx.x * 256u + threadIdx.x;
    bool f = false;
    if (idx < total) {
        const uint32_t i = idx % fb.width, j = idx / fb.width;
        const int8_t* const c = ras + (size_t)(j + fb.oy) * fb.rw + (i + fb.ox);
        if (*c == 0) {
            const bool w = (i > 0u || fb.ox) && c[-1] == -1, e = (i + 1u < fb.width || fb.has_right) && c[1] == -1;
            const bool n = (j > 0u || fb.oy) && *(c - fb.rw) == -1, s = (j + 1u < fb.height || fb.has_down) && c[fb.rw] == -1;
            f = w || e || n || s;
        }
        L[idx] = f ? idx : FRONTIER_NONE;
        if (!(i & 1u) && !(j & 1u)) {
            const uint32_t slot = (j >> 1) * fb.sw + (i >> 1);
            st.sum_i[slot] = 0ull; st.sum_j[slot] = 0ull; st.box[slot] = FRONTIER_BOX_EMPTY; st.count[slot] = 0u;
        }
    }
    const unsigned long long m = __ballot(f);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(reinterpret_cast<unsigned long long*>(&head->pixels), (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(256) void k_frontier_merge(FrontierBox fb, uint32_t* L)
{
    const uint32_t total = fb.width * fb.height, idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total || frontier_load(L, idx) == FRONTIER_NONE) return;
    const uint32_t i = idx % fb.width, j = idx / fb.width;
    if (i > 0u && frontier_load(L, idx - 1u) != FRONTIER_NONE) frontier_unite(L, idx, idx - 1u);
    if (j == 0u) return;
    const uint32_t up = idx - fb.width;
    if (i > 0u && frontier_load(L, up - 1u) != FRONTIER_NONE) frontier_unite(L, idx, up - 1u);
    if (frontier_load(L, up) != FRONTIER_NONE) frontier_unite(L, idx, up);
    if (i + 1u < fb.width && frontier_load(L, up + 1u) != FRONTIER_NONE) frontier_unite(L, idx, up + 1u);
}

__global__ __launch_bounds__(256) void k_frontier_reduce(FrontierBox fb, uint32_t* L, FrontierSlots st)
{
    const uint32_t total = fb.width * fb.height, idx = blockIdx.x * 256u + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    uint32_t root = FRONTIER_NONE, i = 0, j = 0;
    if (idx < total && frontier_load(L, idx) != FRONTIER_NONE) {
        root = frontier_find(L, idx);
        __hip_atomic_store(L + idx, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (other lanes may be walking through idx: still a path to the root)
        i = idx % fb.width; j = idx / fb.width;
    }
    // runs of equal roots among the wave's lanes: a run starts where the lane before holds another root
    const uint32_t before = (uint32_t)__shfl((int)root, lane > 0 ? lane - 1 : 0, 64);
    const bool first = lane == 0 || before != root;
    const unsigned long long heads = __ballot(first);
    const int run = __popcll(heads & (~0ull >> (63 - lane)));       // run numbers ascend with the lane: equal numbers at lane and lane + off mean one run in between
    uint32_t cnt = root != FRONTIER_NONE ? 1u : 0u, si = i, sj = j, lo_i = i, hi_i = i, lo_j = j, hi_j = j;
    for (int off = 1; off < 64; off <<= 1) {
        const int src = lane + off < 64 ? lane + off : lane;
        const int orun = __shfl(run, src, 64);
        const uint32_t oc = (uint32_t)__shfl((int)cnt, src, 64), osi = (uint32_t)__shfl((int)si, src, 64), osj = (uint32_t)__shfl((int)sj, src, 64);
        const uint32_t oli = (uint32_t)__shfl((int)lo_i, src, 64), ohi = (uint32_t)__shfl((int)hi_i, src, 64);
        const uint32_t olj = (uint32_t)__shfl((int)lo_j, src, 64), ohj = (uint32_t)__shfl((int)hi_j, src, 64);
        if (lane + off < 64 && orun == run) {
            cnt += oc; si += osi; sj += osj;                        // at most 64 * 32765: 32 bits
            lo_i = oli < lo_i ? oli : lo_i; hi_i = ohi > hi_i ? ohi : hi_i; lo_j = olj < lo_j ? olj : lo_j; hi_j = ohj > hi_j ? ohj : hi_j;
        }
    }
    if (!first || root == FRONTIER_NONE) return;
    const uint32_t slot = ((root / fb.width) >> 1) * fb.sw + ((root % fb.width) >> 1);
    atomicAdd(st.count + slot, cnt);
    atomicAdd(st.sum_i + slot, (unsigned long long)si);
    atomicAdd(st.sum_j + slot, (unsigned long long)sj);
    unsigned long long cur = __hip_atomic_load(st.box + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        const uint32_t a = (uint32_t)(cur & 0xFFFFull), b = (uint32_t)((cur >> 16) & 0xFFFFull), c = (uint32_t)((cur >> 32) & 0xFFFFull), d = (uint32_t)(cur >> 48);
        const unsigned long long nw = (unsigned long long)(lo_i < a ? lo_i : a) | (unsigned long long)(lo_j < b ? lo_j : b) << 16 |
                                      (unsigned long long)(hi_i > c ? hi_i : c) << 32 | (unsigned long long)(hi_j > d ? hi_j : d) << 48;
        if (nw == cur) break;                                       // the box covers this run already
        const unsigned long long old = atomicCAS(st.box + slot, cur, nw);
        if (old == cur) break;
        cur = old;                                                  // another run widened it in between: merge with what it left
    }
}

__global__ __launch_bounds__(256) void k_frontier_compact(FrontierBox fb, FrontierSlots st, uint32_t min_pixels, FrontierHead* head, uint32_t* __restrict__ ids)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    const bool keep = s < fb.nslots && st.count[s] >= min_pixels;    // min_pixels >= 1: an unused slot is never kept
    const unsigned long long m = __ballot(keep);
    uint32_t base = 0;
    if (lane == 0 && m) base = atomicAdd(&head->n, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, 0, 64);
    if (keep) ids[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = s;
}

__global__ __launch_bounds__(256) void k_frontier_gather(FrontierBox fb, const uint32_t* __restrict__ L, FrontierSlots st, const uint32_t* __restrict__ ids, uint32_t n,
                                                         FrontierRec* __restrict__ out)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const uint32_t s = ids[k], bi = (s % fb.sw) << 1, bj = (s / fb.sw) << 1;
    // the root is the one pixel of the slot's block that is its own label: the block's frontier pixels belong to one component, and
    // after the flattening only a root has L[p] == p
    uint32_t label = FRONTIER_NONE;
    for (uint32_t q = 0; q < 4u; ++q) {
        const uint32_t i = bi + (q & 1u), j = bj + (q >> 1);
        if (i < fb.width && j < fb.height && label == FRONTIER_NONE && L[j * fb.width + i] == j * fb.width + i) label = j * fb.width + i;
    }
    const unsigned long long b = st.box[s];
    FrontierRec r;
    r.label = label; r.pixels = st.count[s];
    r.min_i = (uint32_t)(b & 0xFFFFull); r.min_j = (uint32_t)((b >> 16) & 0xFFFFull); r.max_i = (uint32_t)((b >> 32) & 0xFFFFull); r.max_j = (uint32_t)(b >> 48);
    r.sum_i = st.sum_i[s]; r.sum_j = st.sum_j[s];
    out[k] = r;
}

} // namespace lama_dev
