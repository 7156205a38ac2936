// lama_travel.h -- ROUTES through a particle's device maps (lama_hip_map_travel): the travel-cost field from a set of source pixels
// over the box's traversable pixels, the best pixel near every goal and the path that leads there.  The inputs are the two grids
// k_raster (lama_raster.h) writes for the box: the trinary occupancy layer and the squared-distance layer.  Integers only; the field
// is the unique least fixed point of the move rules (include/lama_hip.h), so no result depends on the order in which lanes, waves,
// workgroups or rounds run.
//
//   k_travel_classify  one byte per pixel: TRAVEL_PASS (free, and sq >= clearance^2) | TRAVEL_NEAR (sq < prefer^2: entering costs
//                      near_factor times as much); the field starts at TRAVEL_INF.
//   k_travel_seed      F = 0 at every source pixel; the tiles that see it are marked active.
//   k_travel_compact   the marked tiles of this round, listed densely (one atomic per wave; the order is of no consequence); their
//                      marks are cleared for the round after next.
//   k_travel_relax     one workgroup per listed tile of 32 x 32 pixels (a workgroup takes several when the list is longer than the
//                      grid).  The tile's field and a ring of one pixel around it go into LDS, 34 x 34 dwords; every thread owns the
//                      pixels (column lane & 31, rows (thread >> 5) + 8k): a group of 32 lanes always touches 32 consecutive dwords of
//                      one LDS row, which no pitch can make conflict (ds_read_b32 banks by dword mod 32 within 32 lanes).  What makes
//                      a move into a pixel legal -- the pixel passable, for a diagonal both pixels beside it -- depends on classes
//                      only and is formed once into 8 bits per pixel; a sweep then is eight LDS reads, adds and minima per pixel, in
//                      place.  Sweeps repeat until one changes nothing (three rotating LDS flags, one barrier per sweep).  Values only
//                      ever fall and every value stored is the cost of a real path, so reading a neighbour tile's rim while its own
//                      workgroup rewrites it gives a valid, perhaps stale, bound: a workgroup that LOWERED a pixel on its rim marks
//                      the (up to three) tiles that see that pixel for the next round, and they look again.  No workgroup waits for
//                      another.  A tile whose sweeps exceed TRAVEL_MAX_SWEEPS (a bound no tile should reach: every sweep that changes
//                      anything makes one more pixel of the tile final) writes back what it has and marks itself.
//   k_travel_answer    a wave per goal: the smallest F in the reach window, ties to the smallest pixel index.
//   k_travel_trace     a wave per reached goal: from the answer pixel, lanes 0..7 test the eight neighbours in ascending pixel index,
//                      the first that fits (finite, legal move, F[n] + step == F[p]) is the next pixel.  The pixels go into a ring of
//                      path_cap entries, so that the LAST path_cap pixels of the descent -- the source end -- survive, and are then
//                      written out source first.  One chase, no second pass.
//
// The host (lama_hip.hip) launches compact + relax round after round and reads the rounds' list lengths back in batches.
#pragma once
#include "lama_raster.h"

namespace lama_dev {

constexpr uint32_t TRAVEL_INF = 0xFFFFFFFFu;
constexpr uint32_t TRAVEL_PITCH = 34u, TRAVEL_LDS = 34u * 34u;
constexpr uint32_t TRAVEL_MAX_SWEEPS = 2048u;
constexpr uint32_t TRAVEL_PASS = 1u, TRAVEL_NEAR = 2u;
constexpr uint32_t TRAVEL_REACHED = 0u, TRAVEL_UNREACHED = 1u, TRAVEL_OUTSIDE = 2u, TRAVEL_BROKEN = 0xFFu;

// the box in pixels, its tiles (tw x th of 32 x 32 pixels) and the multiplier of TRAVEL_NEAR pixels
struct TravelBox { uint32_t x0, y0, width, height, log2s, tw, th, ntiles, near_factor; };
// lama_hip_route (include/lama_hip.h), field by field
struct TravelRoute { uint32_t status, pixel, cost, steps; };

// the tiles that hold pixel (i, j) in their tile or in their ring, the pixel's own tile left out unless `own`
__device__ inline void travel_mark(const TravelBox& tb, uint32_t* flags, uint32_t i, uint32_t j, bool own)
{
    const int ti = (int)(i >> 5), tj = (int)(j >> 5);
    const int li = (int)(i & 31u), lj = (int)(j & 31u);
    for (int dy = -1; dy <= 1; ++dy) {
        if ((dy < 0 && lj != 0) || (dy > 0 && lj != 31)) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            if ((dx < 0 && li != 0) || (dx > 0 && li != 31) || (!own && dx == 0 && dy == 0)) continue;
            const int a = ti + dx, b = tj + dy;
            if (a >= 0 && b >= 0 && a < (int)tb.tw && b < (int)tb.th) flags[(uint32_t)b * tb.tw + (uint32_t)a] = 1u;
        }
    }
}

// occ == nullptr: the context has no occupancy map (only the distance rule applies); sq == nullptr: no distance patch (max_sqdist
// everywhere); nothing: neither map has a patch -- no pixel is passable
__global__ __launch_bounds__(256) void k_travel_classify(TravelBox tb, const int8_t* __restrict__ occ, const uint16_t* __restrict__ sq, uint32_t max_sqdist,
                                                         uint32_t clear2, uint32_t prefer2, int nothing, uint8_t* __restrict__ cls, uint32_t* __restrict__ F)
{
    const uint32_t total = tb.width * tb.height, idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const uint32_t d = sq ? (uint32_t)sq[idx] : max_sqdist;
    const bool pass = !nothing && (!occ || occ[idx] == 0) && d >= clear2;
    cls[idx] = (uint8_t)((pass ? TRAVEL_PASS : 0u) | (d < prefer2 ? TRAVEL_NEAR : 0u));
    F[idx] = TRAVEL_INF;
}

__global__ __launch_bounds__(256) void k_travel_seed(TravelBox tb, uint32_t ns, const uint32_t* __restrict__ src_xy, uint32_t* __restrict__ F, uint32_t* flags)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= ns) return;
    const uint32_t i = (src_xy[2u * k] - tb.x0) >> tb.log2s, j = (src_xy[2u * k + 1u] - tb.y0) >> tb.log2s;      // inside the box: the host has checked
    F[j * tb.width + i] = 0u;
    travel_mark(tb, flags, i, j, true);
}

__global__ __launch_bounds__(256) void k_travel_compact(uint32_t ntiles, uint32_t* flags, uint32_t* __restrict__ list, uint32_t* n)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    const bool on = t < ntiles && flags[t] != 0u;
    if (on) flags[t] = 0u;
    const unsigned long long m = __ballot(on);
    uint32_t base = 0;
    if (lane == 0 && m) base = atomicAdd(n, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, 0, 64);
    if (on) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = t;
}

__global__ __launch_bounds__(256) void k_travel_relax(TravelBox tb, const uint8_t* __restrict__ cls, uint32_t* F, const uint32_t* __restrict__ list,
                                                      const uint32_t* __restrict__ n_ptr, uint32_t* flags_next)
{
    __shared__ uint32_t f[TRAVEL_LDS];
    __shared__ uint8_t cl[TRAVEL_LDS];
    __shared__ uint32_t changed[3];
    __shared__ uint32_t rim;                                         // bit (dy + 1) * 3 + (dx + 1): a pixel that the tile at (dx, dy) sees was lowered
    const uint32_t tid = threadIdx.x, n = uload_u32(n_ptr);          // (uniform reads of what earlier launches wrote: never through the scalar cache)
    const int col = (int)(tid & 31u), row0 = (int)(tid >> 5);
    const int W = (int)tb.width, H = (int)tb.height;
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
        const uint32_t tile = uload_u32(list + k);
        const int ti = (int)(tile % tb.tw), tj = (int)(tile / tb.tw), bi = ti * 32 - 1, bj = tj * 32 - 1;
        for (uint32_t e = tid; e < TRAVEL_LDS; e += 256u) {
            const int gi = bi + (int)(e % TRAVEL_PITCH), gj = bj + (int)(e / TRAVEL_PITCH);
            const bool in = gi >= 0 && gj >= 0 && gi < W && gj < H;
            const size_t g = in ? (size_t)gj * tb.width + (size_t)gi : 0;
            f[e] = in ? F[g] : TRAVEL_INF;
            cl[e] = in ? cls[g] : (uint8_t)0;
        }
        if (tid < 3u) changed[tid] = 0u;
        if (tid == 0u) rim = 0u;
        __syncthreads();
        // the thread's four pixels: which of the eight moves INTO each are legal, and what they cost
        uint32_t cur[4], was[4], legal[4], c5[4], c7[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t e = (uint32_t)(row0 + 8 * q + 1) * TRAVEL_PITCH + (uint32_t)col + 1u;
            const uint32_t c = cl[e];
            uint32_t m = 0;
            if (c & TRAVEL_PASS) {
                const uint32_t w = cl[e - 1u] & TRAVEL_PASS, ea = cl[e + 1u] & TRAVEL_PASS, no = cl[e - TRAVEL_PITCH] & TRAVEL_PASS, so = cl[e + TRAVEL_PITCH] & TRAVEL_PASS;
                m = 0x5Au | (no & w) | (no & ea) << 2 | (so & w) << 5 | (so & ea) << 7;       // bits in ascending pixel index: NW N NE W E SW S SE
            }
            legal[q] = m;
            const uint32_t mult = (c & TRAVEL_NEAR) ? tb.near_factor : 1u;
            c5[q] = 5u * mult; c7[q] = 7u * mult;
            cur[q] = was[q] = f[e];
        }
        uint32_t sweep = 0;
        bool again = false;
        for (;;) {
            bool ch = false;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (!legal[q]) continue;
                const uint32_t e = (uint32_t)(row0 + 8 * q + 1) * TRAVEL_PITCH + (uint32_t)col + 1u;
                uint32_t best = cur[q];
                // a real cost plus a step never wraps (the host refuses boxes where it could), TRAVEL_INF plus a step always does
#define TRAVEL_TRY(bit, off, cost) if (legal[q] & (1u << (bit))) { const uint32_t v = f[(off)], t = v + (cost); if (t > v && t < best) best = t; }
                TRAVEL_TRY(0, e - TRAVEL_PITCH - 1u, c7[q]) TRAVEL_TRY(1, e - TRAVEL_PITCH, c5[q]) TRAVEL_TRY(2, e - TRAVEL_PITCH + 1u, c7[q])
                TRAVEL_TRY(3, e - 1u, c5[q]) TRAVEL_TRY(4, e + 1u, c5[q])
                TRAVEL_TRY(5, e + TRAVEL_PITCH - 1u, c7[q]) TRAVEL_TRY(6, e + TRAVEL_PITCH, c5[q]) TRAVEL_TRY(7, e + TRAVEL_PITCH + 1u, c7[q])
#undef TRAVEL_TRY
                if (best < cur[q]) { cur[q] = best; f[e] = best; ch = true; }
            }
            const uint32_t slot = sweep % 3u;
            if (ch) changed[slot] = 1u;
            __syncthreads();
            const bool any = changed[slot] != 0u;
            if (tid == 0u) changed[(sweep + 2u) % 3u] = 0u;          // read by everyone before the barrier just passed, set again two sweeps on
            if (!any) break;
            if (++sweep >= TRAVEL_MAX_SWEEPS) { again = true; break; }
        }
        uint32_t bits = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (cur[q] >= was[q]) continue;
            const int lj = row0 + 8 * q;
            F[(size_t)(bj + 1 + lj) * tb.width + (size_t)(bi + 1 + col)] = cur[q];
            const int dx0 = col == 0 ? -1 : 0, dx1 = col == 31 ? 1 : 0, dy0 = lj == 0 ? -1 : 0, dy1 = lj == 31 ? 1 : 0;
            for (int dy = dy0; dy <= dy1; ++dy)
                for (int dx = dx0; dx <= dx1; ++dx) bits |= 1u << ((dy + 1) * 3 + dx + 1);
        }
        bits &= ~(1u << 4);
        if (bits) atomicOr(&rim, bits);
        __syncthreads();
        if (tid < 9u) {
            const int a = ti + (int)(tid % 3u) - 1, b = tj + (int)(tid / 3u) - 1;
            const bool mark = tid == 4u ? again : ((rim >> tid) & 1u) != 0u;
            if (mark && a >= 0 && b >= 0 && a < (int)tb.tw && b < (int)tb.th) flags_next[(uint32_t)b * tb.tw + (uint32_t)a] = 1u;
        }
        __syncthreads();                                             // the LDS is the next tile's
    }
}

__global__ __launch_bounds__(64) void k_travel_answer(TravelBox tb, uint32_t ng, const uint32_t* __restrict__ goals_xy, uint32_t reach,
                                                      const uint32_t* __restrict__ F, TravelRoute* __restrict__ routes)
{
    const uint32_t g = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (g >= ng) return;
    const uint32_t gx = uload_u32(goals_xy + 2u * g), gy = uload_u32(goals_xy + 2u * g + 1u);
    const uint32_t i = (gx - tb.x0) >> tb.log2s, j = (gy - tb.y0) >> tb.log2s;
    if (gx < tb.x0 || gy < tb.y0 || i >= tb.width || j >= tb.height) {
        if (lane == 0) routes[g] = TravelRoute{TRAVEL_OUTSIDE, TRAVEL_INF, TRAVEL_INF, 0u};
        return;
    }
    const uint32_t i0 = i > reach ? i - reach : 0u, j0 = j > reach ? j - reach : 0u;
    const uint32_t i1 = i + reach < tb.width ? i + reach : tb.width - 1u, j1 = j + reach < tb.height ? j + reach : tb.height - 1u;
    const uint32_t ww = i1 - i0 + 1u, total = ww * (j1 - j0 + 1u);
    uint32_t best = TRAVEL_INF, at = TRAVEL_INF;
    for (uint32_t q = (uint32_t)lane; q < total; q += 64u) {         // ascending pixel index within a lane: `<` keeps the smallest
        const uint32_t idx = (j0 + q / ww) * tb.width + i0 + q % ww, v = F[idx];
        if (v < best) { best = v; at = idx; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t ob = (uint32_t)__shfl_xor((int)best, off, 64), oa = (uint32_t)__shfl_xor((int)at, off, 64);
        if (ob < best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
    if (lane == 0) routes[g] = best == TRAVEL_INF ? TravelRoute{TRAVEL_UNREACHED, TRAVEL_INF, TRAVEL_INF, 0u} : TravelRoute{TRAVEL_REACHED, at, best, 0u};
}

__global__ __launch_bounds__(64) void k_travel_trace(TravelBox tb, uint32_t ng, const uint8_t* __restrict__ cls, const uint32_t* __restrict__ F,
                                                     TravelRoute* routes, uint32_t cap, uint32_t* ring, uint32_t* __restrict__ out)
{
    const uint32_t g = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (g >= ng) return;
    if (uload_u32(&routes[g].status) != TRAVEL_REACHED) return;
    uint32_t p = uload_u32(&routes[g].pixel), fp = uload_u32(&routes[g].cost), steps = 0;
    uint32_t* const mine = ring + (size_t)g * cap;
    if (cap && lane == 0) mine[0] = p;
    // lanes 0 .. 7: the neighbours in ascending pixel index
    const int di = lane < 3 ? lane - 1 : (lane == 3 ? -1 : (lane == 4 ? 1 : lane - 6)), dj = lane < 3 ? -1 : (lane < 5 ? 0 : 1);
    const uint32_t guard = tb.width * tb.height;
    bool broken = false;
    while (fp != 0u) {
        const int pi = (int)(p % tb.width), pj = (int)(p / tb.width), ni = pi + di, nj = pj + dj;
        uint32_t nidx = 0, fn = TRAVEL_INF;
        bool ok = lane < 8 && ni >= 0 && nj >= 0 && ni < (int)tb.width && nj < (int)tb.height;
        if (ok) {
            const uint32_t cp = cls[p];
            nidx = (uint32_t)nj * tb.width + (uint32_t)ni;
            fn = F[nidx];
            const bool diag = di != 0 && dj != 0;
            const uint32_t cost = (diag ? 7u : 5u) * ((cp & TRAVEL_NEAR) ? tb.near_factor : 1u);
            bool legal = (cp & TRAVEL_PASS) != 0u;
            if (legal && diag) legal = ((uint32_t)cls[(uint32_t)pj * tb.width + (uint32_t)ni] & (uint32_t)cls[(uint32_t)nj * tb.width + (uint32_t)pi] & TRAVEL_PASS) != 0u;
            ok = legal && fn != TRAVEL_INF && fn + cost == fp;
        }
        const unsigned long long m = __ballot(ok);
        if (!m) { broken = true; break; }                            // cannot happen on a finished field: F[p] > 0 has a predecessor
        const int first = __ffsll((long long)m) - 1;
        p = (uint32_t)__shfl((int)nidx, first, 64);
        fp = (uint32_t)__shfl((int)fn, first, 64);
        ++steps;
        if (cap && lane == 0) mine[steps % cap] = p;
        if (steps > guard) { broken = true; break; }
    }
    if (lane == 0) { routes[g].steps = steps; if (broken) routes[g].status = TRAVEL_BROKEN; }
    if (!cap || broken) return;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");               // lane 0's ring entries, for the other lanes
    const uint32_t cnt = steps + 1u < cap ? steps + 1u : cap;
    for (uint32_t t = (uint32_t)lane; t < cnt; t += 64u) out[(size_t)g * cap + t] = mine[(steps - t) % cap];
}

} // namespace lama_dev
