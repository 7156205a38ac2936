// lama_map_build.h -- K posed key scans integrated into ONE frequency occupancy map in a single, order-free pass
// (GraphSlam2D::generateOccupancyMap, src/graph_slam2d.cpp:131-164: per key pose setOccupied at every hit and, in the full variant,
// computeRay + setFree along every beam, then prune(); src/sdm/map.cpp:198-227, src/sdm/frequency_occupancy_map.cpp:65-91,149-158),
// and the list of the occupied cells of such a map (isOccupied, :132-138) in visit_all_cells order.
//
// A rebuild needs none of what makes the per-scan map update (lama_raycast_par.h) ordered: no threshold events, no distance map.
// The {uint16 occupied, uint16 visited} counters commute modulo 2^16 per field, and so do the Container mask bits and the set of
// allocated patches, so all K x n rays go in parallel and the result is what the reference's sequential loop leaves.  Following
// lama_raycast_patch.h (scattered atomics on the cells are bound by the L2's atomic rate), a workgroup OWNS a patch; with K scans
// from K origins the per-scan cone pruning of k_ray_patches has nothing to hold on to, so the rays are BINNED by patch instead:
//
//   k_mb_geom     thread / point : beam geometry (beam_geometry, no truncation: the reference applies none here) -> ray record + hit
//                                  cell, the box of all start and hit cells in patches (the host places / grows the window from it)
//   k_mb_bin      thread / point : COUNT pass -- the ray is walked patch by patch (the walk of k_ray_alloc_walk), one count per
//                                  (ray, patch) crossing and one for the hit, in a table over the box of the call;
//   k_mb_scan     one workgroup  : exclusive scan of the table -> bin offsets, the list of touched patches, how many of them the
//                                  particle does not have yet (the host makes room BEFORE anything is allocated or modified);
//   k_mb_alloc    thread / touched patch : dir_get_or_alloc;
//   k_mb_bin      again, FILL pass: ray indices into the bins;
//   k_mb_patches  workgroup / touched patch : two LDS counter arrays (hits, misses) over the patch's bin -- the exact step range of
//                                  a ray inside the patch is ray_axis_range's, the cells ray_cell's closed form -- then every cell is
//                                  read, both 16-bit fields are advanced SEPARATELY (each wraps on its own; no packed add whose low
//                                  half could carry into the high one) and written once.  No global atomic touches a cell;
//   k_mb_prune    FrequencyOccupancyMap::prune over all patches of the particle.
//
// The inputs (points, offsets, transforms) are host-written buffers copied on the context's own stream and read with per-lane
// vector loads (their addresses depend on the thread index); the few wave-uniform reads go through uload_* (DESIGN.md section 8).
#pragma once
#include "lama_raycast_patch.h"

namespace lama_dev {

struct MbRay {
    RayRec r;                // valid bit (1 << 18): the ray has free cells to visit (full variant, at least two cells long)
    uint32_t mhx, mhy;       // hit cell, map coordinates
};
static_assert(sizeof(MbRay) == 32, "MbRay is four quadwords");

// what k_mb_geom leaves for the host: the patch box of all start / hit cells, problem flags, cell visits of the call
struct MbBounds { uint32_t x0, x1, y0, y1, flags, r0; unsigned long long visits; };
constexpr uint32_t MB_NONFINITE = 1u, MB_TOO_LONG = 2u;
// what k_mb_scan leaves: touched patches, those of them without a slot, bin entries in all
struct MbMeta { uint32_t touched, need, items, r0; };
constexpr uint32_t MB_HIT = 0x80000000u;      // bin entry: the ray's hit (else: its free cells inside the patch)
constexpr int MB_SCAN_BLOCK = 1024;

// exclusive prefix of `v` over the MB_SCAN_BLOCK threads of the workgroup (tmp: 17 words of LDS); total = the sum
__device__ inline uint32_t mb_block_exscan(uint32_t v, uint32_t* tmp, uint32_t& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int off = 1; off < 64; off <<= 1) { const uint32_t o = (uint32_t)__shfl((int)inc, lane >= off ? lane - off : lane, 64); if (lane >= off) inc += o; }
    __syncthreads();                                              // (tmp may still be read from the previous round)
    if (lane == 63) tmp[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t s = 0; for (int w = 0; w < MB_SCAN_BLOCK / 64; ++w) { const uint32_t t = tmp[w]; tmp[w] = s; s += t; } tmp[16] = s; }
    __syncthreads();
    total = tmp[16];
    return tmp[wave] + inc - v;
}

__global__ __launch_bounds__(256) void k_mb_geom(DevParams prm, const double* pts, const uint32_t* offsets, const double* tfs, uint32_t num_scans,
                                                 uint32_t total, int full, MbRay* __restrict__ rays, MbBounds* bounds)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool live = i < total;
    uint32_t x0 = 0xFFFFFFFFu, x1 = 0, y0 = 0xFFFFFFFFu, y1 = 0, flags = 0, steps = 0;
    if (live) {
        uint32_t lo = 0, hi = num_scans;                          // the scan of point i: offsets[lo] <= i < offsets[lo + 1]
        while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (offsets[mid] <= i) lo = mid; else hi = mid; }
        double T[12];
        for (int k = 0; k < 12; ++k) T[k] = tfs[12 * (size_t)lo + k];
        const double px = pts[3 * (size_t)i], py = pts[3 * (size_t)i + 1], pz = pts[3 * (size_t)i + 2];
        const BeamGeom g = beam_geometry(prm, T, px, py, pz);
        MbRay m;
        m.r = ray_rec(g);
        m.mhx = g.mhx; m.mhy = g.mhy;
        const bool finite = fabs(px) <= 1.7976931348623157e308 && fabs(py) <= 1.7976931348623157e308 && fabs(pz) <= 1.7976931348623157e308;   // (false for NaN and +-inf)
        if (!finite) flags |= MB_NONFINITE;
        if (!full || !finite || g.steps < 0) m.r.nnf &= ~(1u << 18);
        if (full && finite && g.steps < 0) flags |= MB_TOO_LONG;
        rays[i] = m;
        if (finite) {
            x0 = x1 = g.mhx >> 5; y0 = y1 = g.mhy >> 5;
            if (m.r.nnf & (1u << 18)) {
                steps = (uint32_t)g.steps;
                const uint32_t sx = g.msx >> 5, sy = g.msy >> 5;
                x0 = sx < x0 ? sx : x0; x1 = sx > x1 ? sx : x1; y0 = sy < y0 ? sy : y0; y1 = sy > y1 ? sy : y1;
            }
            steps += 1u;                                          // the hit
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t ox0 = (uint32_t)__shfl_xor((int)x0, off, 64), ox1 = (uint32_t)__shfl_xor((int)x1, off, 64);
        const uint32_t oy0 = (uint32_t)__shfl_xor((int)y0, off, 64), oy1 = (uint32_t)__shfl_xor((int)y1, off, 64);
        x0 = ox0 < x0 ? ox0 : x0; x1 = ox1 > x1 ? ox1 : x1; y0 = oy0 < y0 ? oy0 : y0; y1 = oy1 > y1 ? oy1 : y1;
        flags |= (uint32_t)__shfl_xor((int)flags, off, 64);
        steps += (uint32_t)__shfl_xor((int)steps, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (x0 <= x1) { atomicMin(&bounds->x0, x0); atomicMax(&bounds->x1, x1); atomicMin(&bounds->y0, y0); atomicMax(&bounds->y1, y1); }
        if (flags) atomicOr(&bounds->flags, flags);
        if (steps) atomicAdd(&bounds->visits, (unsigned long long)steps);
    }
}

// The patches a ray's free cells (steps 1 .. nn - 1) lie in, in step order: f(X, Y), window-relative patch coordinates.  Both
// coordinates of Map::computeRay's closed form are monotone in t and move by at most one cell per step, so the patch changes exactly
// where an axis makes a move that takes it across a multiple of 32 (the derivation is k_ray_alloc_walk's, lama_raycast_patch.h).
template <class F>
__device__ inline void mb_walk_patches(const DevParams& prm, const RayRec& r, F&& f)
{
    const uint32_t a0 = r.a01 & 0xFFFFu, a1 = r.a01 >> 16, nn = r.nnf & 0xFFFFu, t1 = nn - 1u;
    const uint32_t k0 = (uint32_t)(((uint64_t)(2u * a0 + nn) * r.magic) >> 42), k1 = (uint32_t)(((uint64_t)(2u * a1 + nn) * r.magic) >> 42);
    const bool neg0 = (r.nnf >> 16) & 1u, neg1 = (r.nnf >> 17) & 1u;
    const uint32_t bx = r.msx - prm.wx0, by = r.msy - prm.wy0;
    const uint32_t rx = neg0 ? bx - k0 : bx + k0, ry = neg1 ? by - k1 : by + k1;          // the cell of step 1
    uint32_t X = rx >> 5, Y = ry >> 5;
    uint32_t kx = neg0 ? k0 + (rx & 31u) + 1u : k0 + 32u - (rx & 31u), ky = neg1 ? k1 + (ry & 31u) + 1u : k1 + 32u - (ry & 31u);
    auto step_of = [nn](uint32_t k, uint32_t a) { return k > a ? 0xFFFFFFFFu : (2u * nn * k - nn + 2u * a - 1u) / (2u * a); };
    uint32_t tx = step_of(kx, a0), ty = step_of(ky, a1);
    f(X, Y);
    for (;;) {
        const uint32_t t = tx < ty ? tx : ty;
        if (t > t1) break;
        if (tx == t) { X = neg0 ? X - 1u : X + 1u; kx += 32u; tx = step_of(kx, a0); }
        if (ty == t) { Y = neg1 ? Y - 1u : Y + 1u; ky += 32u; ty = step_of(ky, a1); }
        f(X, Y);
    }
}

// One more entry for bin `b` from every lane that is active here.  The rays of a wave are consecutive beams of (mostly) one scan:
// they start in one patch, so the lanes whose bin is the first active lane's share ONE atomic (the others -- a scan boundary inside
// the wave -- add their own).  Returns the lane's position inside the bin's new entries.
__device__ inline uint32_t mb_bin_add(uint32_t* table, uint32_t b)
{
#ifdef LAMA_WAVE_SIM
    return atomicAdd(table + b, 1u);
#else
    const unsigned long long act = __ballot(true);
    const int lane = (int)(threadIdx.x & 63u), leader = __ffsll((long long)act) - 1;
    const uint32_t lb = (uint32_t)__builtin_amdgcn_readlane((int)b, leader);
    const unsigned long long same = __ballot(b == lb);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(table + lb, (uint32_t)__popcll(same));
    base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
    if (b == lb) return base + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    return atomicAdd(table + b, 1u);
#endif
}

// count pass (bins == nullptr): table[b] += entries of bin b; fill pass: table = the bins' cursors, entries go to bins[off[b] + cursor]
__global__ __launch_bounds__(256) void k_mb_bin(DevParams prm, const MbRay* __restrict__ rays, uint32_t total, uint32_t bx0, uint32_t by0, uint32_t bw,
                                                uint32_t bh, uint32_t* table, const uint32_t* __restrict__ off, uint32_t* __restrict__ bins)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const MbRay m = rays[i];
    const uint32_t hx = ((m.mhx - prm.wx0) >> 5) - bx0, hy = ((m.mhy - prm.wy0) >> 5) - by0;
    if (hx < bw && hy < bh) {                                     // (a point the geometry pass refused lies outside: the call fails before this runs)
        const uint32_t b = hy * bw + hx, k = mb_bin_add(table, b);
        if (bins) bins[off[b] + k] = i | MB_HIT;
    }
    if (!(m.r.nnf & (1u << 18))) return;
    bool first = true;
    mb_walk_patches(prm, m.r, [&](uint32_t X, uint32_t Y) {
        const uint32_t x = X - bx0, y = Y - by0;
        if (x >= bw || y >= bh) return;
        const uint32_t b = y * bw + x;
        // (only the first patch is reached by all lanes of the wave together)
        const uint32_t k = first ? mb_bin_add(table, b) : atomicAdd(table + b, 1u);
        first = false;
        if (bins) bins[off[b] + k] = i;
    });
}

// table[nb] -> off[nb + 1] (exclusive scan), the touched bins in ascending order, how many of them have no patch yet; the table is
// cleared for the fill pass.  One workgroup.
__global__ __launch_bounds__(MB_SCAN_BLOCK) void k_mb_scan(DevParams prm, int p, uint32_t bx0, uint32_t by0, uint32_t bw, uint32_t nb, uint32_t* table,
                                                           uint32_t* __restrict__ off, uint32_t* __restrict__ tlist, MbMeta* meta)
{
    __shared__ uint32_t tmp[17];
    const PV pv = pview(prm, p);
    uint32_t items = 0, touched = 0, need = 0;
    for (uint32_t base = 0; base < nb; base += MB_SCAN_BLOCK) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < nb ? table[b] : 0u;
        uint32_t tot = 0;
        const uint32_t e = mb_block_exscan(v, tmp, tot);
        if (b < nb) { off[b] = items + e; table[b] = 0; }
        items += tot;
        const uint32_t et = mb_block_exscan(v ? 1u : 0u, tmp, tot);
        if (v) {
            tlist[touched + et] = b;
            if (pv.occ_dir[(size_t)(by0 + b / bw) * prm.W + bx0 + b % bw] < 0) ++need;
        }
        touched += tot;
    }
    uint32_t tot = 0;
    (void)mb_block_exscan(need, tmp, tot);
    if (threadIdx.x == 0) { off[nb] = items; meta->touched = touched; meta->need = tot; meta->items = items; }
}

__global__ __launch_bounds__(256) void k_mb_alloc(DevParams prm, int p, uint32_t bx0, uint32_t by0, uint32_t bw, const uint32_t* __restrict__ tlist,
                                                  uint32_t touched, int32_t* __restrict__ tslot)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const PV pv = pview(prm, p);
    if (i >= touched) return;
    const uint32_t b = tlist[i];
    tslot[i] = dir_get_or_alloc(pv.occ_dir, (by0 + b / bw) * prm.W + bx0 + b % bw, prm.counts + 2 * p + 1, (int)pv.occ_cap, ERR_OCC_CAP, prm.err);
}

__global__ __launch_bounds__(256) void k_mb_patches(DevParams prm, int p, uint32_t bx0, uint32_t by0, uint32_t bw, const uint32_t* __restrict__ tlist,
                                                    const int32_t* __restrict__ tslot, const uint32_t* __restrict__ off, const uint32_t* __restrict__ bins,
                                                    const MbRay* __restrict__ rays)
{
    __shared__ uint32_t hits[1024], miss[1024];
    if (map_update_aborted(prm)) return;                          // an allocation failed: no cell changes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PVOcc pv = pview_occ_w(prm, p);
    const uint32_t b = uload_u32(tlist + blockIdx.x);          // (wave-uniform reads: coherent loads, lama_dev.h)
    const int slot = uload_i32(tslot + blockIdx.x);
    if (slot < 0) return;
    const int px = (int)((bx0 + b % bw) * 32u), py = (int)((by0 + b / bw) * 32u);      // window-relative origin of the patch
    for (int j = 0; j < 4; ++j) { hits[tid + 256 * j] = 0; miss[tid + 256 * j] = 0; }
    __syncthreads();
    const uint32_t e1 = uload_u32(off + b + 1);
    for (uint32_t e = uload_u32(off + b) + (uint32_t)tid; e < e1; e += 256u) {
        const uint32_t ent = bins[e];
        const MbRay m = rays[ent & ~MB_HIT];
        if (ent & MB_HIT) {
            const uint32_t rx = m.mhx - prm.wx0, ry = m.mhy - prm.wy0;
            atomicAdd(&hits[(rx & 31u) | ((ry & 31u) << 5)], 1u);
            continue;
        }
        const uint32_t nn = m.r.nnf & 0xFFFFu, steps = nn - 1u;
        uint32_t xl = 0, xh = 0, yl = 0, yh = 0;
        if (!ray_axis_range((int)(m.r.msx - prm.wx0), (m.r.nnf >> 16) & 1u, m.r.a01 & 0xFFFFu, nn, px, steps, xl, xh)) continue;
        if (!ray_axis_range((int)(m.r.msy - prm.wy0), (m.r.nnf >> 17) & 1u, m.r.a01 >> 16, nn, py, steps, yl, yh)) continue;
        const uint32_t tl = xl > yl ? xl : yl, th = xh < yh ? xh : yh;
        for (uint32_t t = tl; t <= th; ++t) {
            uint32_t rx, ry;
            ray_cell(m.r, prm.wx0, prm.wy0, t, rx, ry);
            if ((int)(rx & ~31u) == px && (int)(ry & ~31u) == py) atomicAdd(&miss[(rx & 31u) | ((ry & 31u) << 5)], 1u);      // (always: the range is exact)
        }
    }
    __syncthreads();
    for (int j = 0; j < 4; ++j) {
        const int ci = tid + 256 * j;
        const uint32_t h = hits[ci], f = miss[ci];
        bool wrap = false;
        if (h | f) {
            uint32_t* cell = pv.occ + (size_t)slot * 1024 + ci;
            const uint32_t v = *cell;
            const uint32_t o = ((v & 0xFFFFu) + h) & 0xFFFFu;                        // setOccupied: occupied++ and visited++; setFree: visited++
            const uint64_t vis = (uint64_t)(v >> 16) + h + f;
            wrap = vis > 0xFFFFu;                                                    // the counter passed 0: the Container mask bit outlives it
            *cell = o | ((uint32_t)(vis & 0xFFFFu) << 16);
        }
        const unsigned long long wm = __ballot(wrap);                                // cells 256 j + 64 wave .. + 63 = mask word 4 j + wave
        if (lane == 0 && wm) atomicOr((unsigned long long*)(pv.occ_mask + (size_t)slot * 16 + 4 * j + wave), wm);
    }
}

// FrequencyOccupancyMap::prune (src/sdm/frequency_occupancy_map.cpp:149-158): visited == 1 and occupied <= 1 -> {0, 0}; the cell
// stays in the Container mask (a mask bit is "visited != 0" or the plane's bit: the plane gets it here)
__global__ __launch_bounds__(256) void k_mb_prune(DevParams prm, int p)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PVOcc pv = pview_occ_w(prm, p);
    const int count = uload_i32(prm.counts + 2 * p + 1);
    for (int slot = blockIdx.x; slot < count; slot += gridDim.x)
        for (int j = 0; j < 4; ++j) {
            uint32_t* cell = pv.occ + (size_t)slot * 1024 + tid + 256 * j;
            const uint32_t v = *cell;
            const bool cut = (v >> 16) == 1u && (v & 0xFFFFu) <= 1u;
            if (cut) *cell = 0;
            const unsigned long long cm = __ballot(cut);
            if (lane == 0 && cm) atomicOr((unsigned long long*)(pv.occ_mask + (size_t)slot * 16 + 4 * j + wave), cm);
        }
}

// ---- the occupied cells of a particle's occupancy map, in visit_all_cells order --------------------------------------------------
// k_mb_order: the particle's patches by ascending reference patch index (Map::m2p: x-major, include/lama/sdm/map.h:153-161) -- a scan
// over the window directory read column by column; one workgroup.
__global__ __launch_bounds__(MB_SCAN_BLOCK) void k_mb_order(DevParams prm, int p, int32_t* __restrict__ slots, uint32_t* __restrict__ pos)
{
    __shared__ uint32_t tmp[17];
    const PV pv = pview(prm, p);
    const uint32_t W = prm.W, WW = W * W;
    uint32_t n = 0;
    for (uint32_t base = 0; base < WW; base += MB_SCAN_BLOCK) {
        const uint32_t q = base + threadIdx.x;                    // q = wx * W + wy
        const uint32_t pidx = q < WW ? (q % W) * W + q / W : 0u;
        const int slot = q < WW ? (int)pv.occ_dir[pidx] : -1;
        uint32_t tot = 0;
        const uint32_t e = mb_block_exscan(slot >= 0 ? 1u : 0u, tmp, tot);
        if (slot >= 0) { slots[n + e] = slot; pos[n + e] = pidx; }
        n += tot;
    }
}

__device__ inline bool mb_is_occupied(uint32_t v)              // prob(cell) > occ_thresh, in double as the reference evaluates it (:38-45)
{
    const uint32_t o = v & 0xFFFFu, vis = v >> 16;
    return vis != 0u && (double)o / (double)vis > 0.25;
}

// count pass (out == nullptr): cnt[j] = occupied cells of the j-th patch; emit pass: their map coordinates from position off[j] on,
// ascending cell index
__global__ __launch_bounds__(256) void k_mb_occupied(DevParams prm, int p, const int32_t* __restrict__ slots, const uint32_t* __restrict__ pos,
                                                     uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off, uint32_t cap, uint32_t* __restrict__ out)
{
    __shared__ uint32_t wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PVOcc pv = pview_occ_w(prm, p);
    const int slot = uload_i32(slots + blockIdx.x);
    const uint32_t pidx = uload_u32(pos + blockIdx.x);
    unsigned long long m[4];
    for (int j = 0; j < 4; ++j) m[j] = __ballot(mb_is_occupied(pv.occ[(size_t)slot * 1024 + tid + 256 * j]));     // cells 256 j + 64 wave ..
    if (lane == 0) for (int j = 0; j < 4; ++j) wsum[4 * j + wave] = (uint32_t)__popcll(m[j]);
    __syncthreads();
    if (!out) {
        if (tid == 0) { uint32_t s = 0; for (int k = 0; k < 16; ++k) s += wsum[k]; cnt[blockIdx.x] = s; }
        return;
    }
    const uint32_t x0 = prm.wx0 + (pidx % prm.W) * 32u, y0 = prm.wy0 + (pidx / prm.W) * 32u;
    for (int j = 0; j < 4; ++j) {
        if (!((m[j] >> lane) & 1ull)) continue;
        uint32_t k = uload_u32(off + blockIdx.x) + (uint32_t)__popcll(m[j] & ((1ull << lane) - 1ull));
        for (int w = 0; w < 4 * j + wave; ++w) k += wsum[w];
        const uint32_t ci = (uint32_t)(tid + 256 * j);
        if (k < cap) { out[2 * (size_t)k] = x0 + (ci & 31u); out[2 * (size_t)k + 1] = y0 + (ci >> 5); }
    }
}

// off[n + 1] = exclusive scan of cnt[n]; one workgroup
__global__ __launch_bounds__(MB_SCAN_BLOCK) void k_mb_exscan(const uint32_t* __restrict__ cnt, uint32_t n, uint32_t* __restrict__ off)
{
    __shared__ uint32_t tmp[17];
    uint32_t sum = 0;
    for (uint32_t base = 0; base < n; base += MB_SCAN_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        uint32_t tot = 0;
        const uint32_t e = mb_block_exscan(i < n ? cnt[i] : 0u, tmp, tot);
        if (i < n) off[i] = sum + e;
        sum += tot;
    }
    if (threadIdx.x == 0) off[n] = sum;
}

} // namespace lama_dev
