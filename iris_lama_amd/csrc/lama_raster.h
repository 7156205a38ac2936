// lama_raster.h -- a particle's sparse device maps written out as DENSE grids (lama_hip_map_rasterize) and the box of its allocated
// patches (lama_hip_map_bounds, Map::bounds, src/sdm/map.cpp:139-157): what nav_msgs/OccupancyGrid carries and a planner's costmap
// eats, one byte (two for the squared distance) per `stride x stride` block of cells instead of the 4 .. 10 bytes per cell of the
// reference's records that lama_hip_pf_download_map brings down.
//
// k_raster: one workgroup per PATCH POSITION of the box (the patches the box touches, present or not).  One directory lookup; an
// absent patch -- outside the window, or no slot -- only fills its region with the layer's "unknown".  A present patch is read once
// with 16-byte loads (4 frequency / log-odds cells, 8 distance cells of the default build, 4 of the wide one per lane), every cell is
// classified into an LDS tile, blocks of stride x stride cells are reduced in LDS (rows first, then columns: at most 2 x 32 reads per
// thread), and the patch's rows of pixels go out in aligned chunks of 8 pixels (8 bytes / 16 bytes per store) with single pixels
// only at the two ragged ends of a row segment.  The box's origin is a multiple of the stride and a patch is 32 cells, so a block
// never straddles two patches and no two workgroups write the same pixel.
//
// Cell rules (exact, order-free, integers only):
//   frequency {uint16 occupied, uint16 visited}: visited == 0 unknown; 4 * occupied > visited occupied; 4 * occupied < visited free;
//     equality unknown.  This IS the reference's `(double)occupied / (double)visited > 0.25` (< 0.25) for every uint16 pair: 0.25 is a
//     double, division is correctly rounded and therefore monotone with fl(0.25) = 0.25, so the quotient can only land on the wrong
//     side by rounding ONTO 0.25 -- but |occupied / visited - 0.25| = |4 occupied - visited| / (4 visited) is either 0 or at least
//     1 / (4 * 65535) > 2^-19, thirty-odd binary orders above the spacing of doubles near 0.25.  (A mask bit adds nothing: a cell's
//     Container bit is "visited != 0" or a bit a counter wrap left behind, and visited == 0 is unknown either way.)
//     Probability: (200 * occupied + visited) / (2 * visited) = round-half-up(100 * occupied / visited), capped at 100 (occupied can
//     exceed visited only after visited wrapped).
//   log-odds float l (policy 1): mask bit on and l < 0 free, l > 0 occupied, otherwise unknown.
//   distance: mask bit on and valid_obstacle -> the stored sqdist, otherwise max_sqdist (DynamicDistanceMap::distance).
// Blocks: occupied (100) beats free (0) beats unknown (-1) and the largest probability wins -- both a signed maximum; the squared
// distance takes the minimum.
#pragma once
#include "lama_map_build.h"

namespace lama_dev {

constexpr int RASTER_TRINARY = 0, RASTER_PROBABILITY = 1, RASTER_SQDIST = 2;

struct RasterBox { uint32_t x0, y0, width, height, stride, log2s; };
// what k_map_bounds leaves: the box of the allocated patches in window patch coordinates and their number
struct MapBoundsRec { uint32_t x0, x1, y0, y1, n, r0; };

// a directory entry for the whole wave: the table is rewritten by the host (window moves, uploads, resamples), so the word that holds
// the int16 comes through the coherent uniform load
__device__ inline int dir_entry_uniform(const int16_t* dir, size_t idx)
{
    const uintptr_t a = (uintptr_t)(dir + idx);
    const uint32_t w = uload_u32(reinterpret_cast<const void*>(a & ~(uintptr_t)3));
    return (int)(int16_t)((a & 2u) ? (w >> 16) : (w & 0xFFFFu));
}

template <int LAYER> struct RasterOut { typedef int8_t type; };
template <> struct RasterOut<RASTER_SQDIST> { typedef uint16_t type; };

__device__ inline int8_t raster_freq_trinary(uint32_t v)
{
    const uint32_t o4 = 4u * (v & 0xFFFFu), vis = v >> 16;
    return vis == 0u || o4 == vis ? (int8_t)-1 : (o4 > vis ? (int8_t)100 : (int8_t)0);
}
__device__ inline int8_t raster_freq_probability(uint32_t v)
{
    const uint32_t o = v & 0xFFFFu, vis = v >> 16;
    if (vis == 0u) return (int8_t)-1;
    const uint32_t q = (200u * o + vis) / (2u * vis);
    return (int8_t)(q > 100u ? 100u : q);
}
__device__ inline int8_t raster_logodds_trinary(uint32_t v, bool masked)
{
    const float l = __uint_as_float(v);
    return masked && l < 0.0f ? (int8_t)0 : (masked && l > 0.0f ? (int8_t)100 : (int8_t)-1);
}

template <int LAYER>
__global__ __launch_bounds__(256) void k_raster(DevParams prm, int p, RasterBox box, typename RasterOut<LAYER>::type* __restrict__ out)
{
    typedef typename RasterOut<LAYER>::type T;
    typedef typename std::conditional<LAYER == RASTER_SQDIST, sv_t, uint32_t>::type Cell;
    constexpr int PER = 16 / (int)sizeof(Cell);                  // cells per 16-byte load
    __shared__ T tile[1024];                                      // the patch, one value per cell
    __shared__ T rowred[512];                                     // [32 rows][32 / stride]: blocks reduced along x
    __shared__ T pix[256];                                        // [32 / stride][32 / stride]: the patch's pixels (stride > 1)
    const int tid = threadIdx.x;
    const PV pv = pview(prm, p);
    const T unknown = LAYER == RASTER_SQDIST ? (T)prm.max_sqdist : (T)-1;
    // the patch of this workgroup: absolute cell coordinates of its anchor (64 bits: a box may reach past the last map cell)
    const uint64_t ax = (uint64_t)(box.x0 & ~31u) + 32ull * blockIdx.x, ay = (uint64_t)(box.y0 & ~31u) + 32ull * blockIdx.y;
    const uint64_t rx = ax - prm.wx0, ry = ay - prm.wy0;          // (below the window: wraps to a huge number)
    int slot = -1;
    if (rx < prm.WC && ry < prm.WC) slot = dir_entry_uniform(LAYER == RASTER_SQDIST ? pv.dm_dir : pv.occ_dir, (size_t)(ry >> 5) * prm.W + (size_t)(rx >> 5));
    const uint32_t s = box.stride, n = 32u >> box.log2s;          // pixels per patch side
    const T* res = pix;
    if (slot < 0) {
        if (s == 1u) { for (int k = 0; k < 4; ++k) tile[tid + 256 * k] = unknown; res = tile; }
        else pix[tid] = unknown;
    } else {
        if (tid < 1024 / PER) {
            const Cell* cells = (LAYER == RASTER_SQDIST ? (const Cell*)pv.dm_sv : (const Cell*)pv.occ) + (size_t)slot * 1024;
            const uint4 q = *reinterpret_cast<const uint4*>(cells + PER * tid);
            struct { Cell c[PER]; } u;
            __builtin_memcpy(&u, &q, 16);
            uint64_t mw = ~0ull;                                  // the Container mask word of these cells (PER divides 64)
            if (LAYER == RASTER_SQDIST) mw = pv.dm_mask[(size_t)slot * 16 + (PER * tid >> 6)];
            else if (LAYER == RASTER_TRINARY && prm.occ_policy != 0u) mw = pv.occ_mask[(size_t)slot * 16 + (PER * tid >> 6)];
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const bool masked = (mw >> ((PER * tid + k) & 63)) & 1ull;
                T v;
                if (LAYER == RASTER_SQDIST) v = masked && (u.c[k] & SV_VALID) ? (T)(u.c[k] & SV_SQMASK) : unknown;
                else if (LAYER == RASTER_PROBABILITY) v = (T)raster_freq_probability((uint32_t)u.c[k]);
                else v = (T)(prm.occ_policy != 0u ? raster_logodds_trinary((uint32_t)u.c[k], masked) : raster_freq_trinary((uint32_t)u.c[k]));
                tile[PER * tid + k] = v;
            }
        }
        __syncthreads();
        if (s == 1u) res = tile;
        else {
            for (uint32_t t = tid; t < 32u * n; t += 256u) {      // row r, block u: s cells along x
                const uint32_t r = t / n, u = t % n;
                T a = tile[r * 32u + u * s];
                for (uint32_t k = 1; k < s; ++k) { const T b = tile[r * 32u + u * s + k]; a = LAYER == RASTER_SQDIST ? (b < a ? b : a) : (b > a ? b : a); }
                rowred[t] = a;
            }
            __syncthreads();
            if ((uint32_t)tid < n * n) {                          // pixel (u, v): s rows
                const uint32_t v = tid / n, u = tid % n;
                T a = rowred[v * s * n + u];
                for (uint32_t k = 1; k < s; ++k) { const T b = rowred[(v * s + k) * n + u]; a = LAYER == RASTER_SQDIST ? (b < a ? b : a) : (b > a ? b : a); }
                pix[tid] = a;
            }
        }
    }
    __syncthreads();
    // res[v * n + u] is pixel (pi0 + u, pj0 + v) of the output, where (pi0, pj0) may be negative or past the box (first / last patch)
    const int64_t pi0 = ((int64_t)ax - (int64_t)box.x0) >> box.log2s, pj0 = ((int64_t)ay - (int64_t)box.y0) >> box.log2s;
    const int64_t ulo = pi0 < 0 ? -pi0 : 0, uhi = pi0 + (int64_t)n > (int64_t)box.width ? (int64_t)box.width - pi0 : (int64_t)n;
    const int64_t v = tid >> 3, k8 = tid & 7;                     // eight threads per pixel row, a chunk of 8 pixels each
    const int64_t j = pj0 + v;
    if (v >= (int64_t)n || j < 0 || j >= (int64_t)box.height || ulo >= uhi) return;
    const uint64_t e0 = (uint64_t)j * box.width + (uint64_t)(pi0 + ulo), e1 = e0 + (uint64_t)(uhi - ulo);      // the row segment [e0, e1) of `out`
    const uint64_t cb = (e0 & ~7ull) + 8ull * (uint64_t)k8;       // an unaligned run of at most 32 pixels spans at most 5 aligned chunks
    if (cb >= e1) return;
    const T* src = res + v * n + ulo;                             // src[e - e0]
    if (cb >= e0 && cb + 8u <= e1) {
        T t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = src[cb - e0 + k];
        if (sizeof(T) == 1) { uint2 d; __builtin_memcpy(&d, t, 8); *reinterpret_cast<uint2*>(out + cb) = d; }
        else { uint4 d; __builtin_memcpy(&d, t, 8 * sizeof(T)); *reinterpret_cast<uint4*>(out + cb) = d; }
    } else {
        const uint64_t a = cb > e0 ? cb : e0, b = cb + 8u < e1 ? cb + 8u : e1;
        for (uint64_t e = a; e < b; ++e) out[e] = src[e - e0];
    }
}

// Map::bounds of the particle's map of `kind` (0 distance, 1 occupancy) in WINDOW patch coordinates, and the number of patches: one
// workgroup over the directory (per-lane loads: the addresses depend on the thread index)
__global__ __launch_bounds__(MB_SCAN_BLOCK) void k_map_bounds(DevParams prm, int p, int kind, MapBoundsRec* out)
{
    __shared__ uint32_t red[5][MB_SCAN_BLOCK / 64];
    const PV pv = pview(prm, p);
    const int16_t* dir = kind == 0 ? pv.dm_dir : pv.occ_dir;
    const uint32_t W = prm.W, WW = W * W;
    uint32_t x0 = 0xFFFFFFFFu, x1 = 0, y0 = 0xFFFFFFFFu, y1 = 0, cnt = 0;
    for (uint32_t q = threadIdx.x; q < WW; q += MB_SCAN_BLOCK) {
        if (dir[q] < 0) continue;
        const uint32_t wx = q % W, wy = q / W;
        x0 = wx < x0 ? wx : x0; x1 = wx > x1 ? wx : x1; y0 = wy < y0 ? wy : y0; y1 = wy > y1 ? wy : y1; ++cnt;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t ox0 = (uint32_t)__shfl_xor((int)x0, off, 64), ox1 = (uint32_t)__shfl_xor((int)x1, off, 64);
        const uint32_t oy0 = (uint32_t)__shfl_xor((int)y0, off, 64), oy1 = (uint32_t)__shfl_xor((int)y1, off, 64);
        x0 = ox0 < x0 ? ox0 : x0; x1 = ox1 > x1 ? ox1 : x1; y0 = oy0 < y0 ? oy0 : y0; y1 = oy1 > y1 ? oy1 : y1;
        cnt += (uint32_t)__shfl_xor((int)cnt, off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = x0; red[1][wave] = x1; red[2][wave] = y0; red[3][wave] = y1; red[4][wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        MapBoundsRec r{0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0u, 0u};
        for (int w = 0; w < MB_SCAN_BLOCK / 64; ++w) {
            r.x0 = red[0][w] < r.x0 ? red[0][w] : r.x0; r.x1 = red[1][w] > r.x1 ? red[1][w] : r.x1;
            r.y0 = red[2][w] < r.y0 ? red[2][w] : r.y0; r.y1 = red[3][w] > r.y1 ? red[3][w] : r.y1; r.n += red[4][w];
        }
        *out = r;
    }
}

} // namespace lama_dev
