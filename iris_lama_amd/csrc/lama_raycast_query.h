// lama_raycast_query.h -- what a sensor at a given pose WOULD see in a particle's device map (lama_hip_map_cast_rays): the first cell
// of every beam that stops the ray.  Read-only: no map, pose or counter changes.
//
// k_cast_rays: one lane per (pose, beam); beams along x in blocks of 256, poses along y (a grid-stride loop: more poses than a grid has
// rows), so a wave holds 64 neighbouring beams of one pose and their loads stay in the same few patches.
//
// The cell sequence of a beam is the map update's, not new geometry: start and hit cell from beam_geometry (lama_raycast_par.h; the
// transform composed on the host by host_scan_tf, no truncation -- a query asks about the whole beam, as the map rebuild does), then
// the cells of Map::computeRay(start, hit) in order through k_raycast's closed form floor((2 t a + nn) / (2 nn)), t = 1 .. nn - 1,
// then the hit cell: nn entries, none for start == hit, the start cell never among them.  The host has checked nn <= 8191 for every
// beam before the launch, the loop runs at most nn times, and nothing that a map holds can prolong it.
//
// Stop rules (exact, integers only): an occupancy cell by lama_raster.h's trinary rules (raster_freq_trinary / raster_logodds_trinary:
// 100 stops the ray; -1 is "unknown" and stops it with RAY_STOP_UNKNOWN, as does a cell in an absent patch or outside the window); a
// distance cell where dm_cell_sv's record says valid_obstacle with a squared distance of 0 (an off-bit cell is all-zero and reads as
// not valid).  A lane keeps its patch slot while the walk stays inside one patch: one directory lookup per patch crossed.
//
// The directories are rewritten by the host (window moves, uploads, resamples): a lane's entry comes through an agent-scope load of
// the word that holds the int16, the per-lane form of lama_raster.h's dir_entry_uniform; the pose transforms through uload_f64_w.
#pragma once
#include "lama_raster.h"

namespace lama_dev {

constexpr uint32_t RAY_STOP_UNKNOWN = 1u;                          // LAMA_HIP_RAY_STOP_UNKNOWN
constexpr int RAY_NONE = 0, RAY_OCCUPIED = 1, RAY_UNKNOWN = 2;     // status
constexpr int RAY_AGREES = 0, RAY_BLOCKED = 1, RAY_NOVEL = 2;      // label

// [num_poses][n] each; every one but status may be null
struct CastOut { uint8_t* status; int32_t* step; uint32_t* nn; uint32_t* cell_xy; uint32_t* end_sqdist; uint8_t* label; };

// a directory entry for ONE lane (the address depends on the beam): coherent at the L2, never the scalar cache
__device__ inline int dir_entry_lane(const int16_t* dir, size_t idx)
{
    const uintptr_t a = (uintptr_t)(dir + idx);
    const uint32_t w = __hip_atomic_load(reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (int)(int16_t)((a & 2u) ? (w >> 16) : (w & 0xFFFFu));
}

// DM = true: the particle's distance map, else its occupancy map
template <bool DM>
__global__ __launch_bounds__(256) void k_cast_rays(DevParams prm, int p, const double* pts, uint32_t n, const double* tfs, uint32_t num_poses,
                                                   uint32_t flags, int32_t tolerance, CastOut out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool live = i < n;
    const uint32_t ic = live ? i : n - 1u;
    const PV pv = pview(prm, p);
    const int16_t* const dir = DM ? pv.dm_dir : pv.occ_dir;
    const double px = pts[3 * (size_t)ic], py = pts[3 * (size_t)ic + 1], pz = pts[3 * (size_t)ic + 2];
    const bool stop_unknown = !DM && (flags & RAY_STOP_UNKNOWN);
    for (uint32_t pose = blockIdx.y; pose < num_poses; pose += gridDim.y) {
        double T[12];
        uload_f64_w<12>(tfs + 12 * (size_t)pose, T);              // (every lane of the wave is here: `live` masks the stores only)
        const BeamGeom g = beam_geometry(prm, T, px, py, pz);
        const uint32_t nn = g.nn;
        int status = RAY_NONE, step = -1;
        uint32_t sx = g.mhx, sy = g.mhy;                          // the stopping cell; the hit cell when nothing stops the ray
        uint32_t cur = 0xFFFFFFFFu;                               // the window patch the lane holds the slot of (none yet)
        int slot = -1;
        for (uint32_t k = 0; k < nn; ++k) {
            uint32_t cx = g.mhx, cy = g.mhy;                      // entry nn - 1: the hit cell
            if (k + 1u < nn) {
                const uint32_t t = k + 1u;
                const uint32_t st0 = (uint32_t)(((uint64_t)(2u * t * g.a0 + nn) * g.magic) >> 42);
                const uint32_t st1 = (uint32_t)(((uint64_t)(2u * t * g.a1 + nn) * g.magic) >> 42);
                cx = g.msx + (uint32_t)(g.s0 * (int)st0); cy = g.msy + (uint32_t)(g.s1 * (int)st1);
            }
            const uint32_t rx = cx - prm.wx0, ry = cy - prm.wy0;
            int cls = RAY_UNKNOWN;                                // outside the window, or in an absent patch
            if (rx < prm.WC && ry < prm.WC) {
                const uint32_t pidx = (ry >> 5) * prm.W + (rx >> 5);
                if (pidx != cur) { cur = pidx; slot = dir_entry_lane(dir, pidx); }
                if (slot >= 0) {
                    const uint32_t ci = (rx & 31u) | ((ry & 31u) << 5);
                    if (DM) {
                        const sv_t v = pv.dm_sv[(size_t)slot * 1024 + ci];
                        cls = (v & SV_VALID) && (v & SV_SQMASK) == 0 ? RAY_OCCUPIED : RAY_NONE;
                    } else {
                        const uint32_t v = pv.occ[(size_t)slot * 1024 + ci];
                        int8_t tri;
                        if (prm.occ_policy != 0u) tri = raster_logodds_trinary(v, (pv.occ_mask[(size_t)slot * 16 + (ci >> 6)] >> (ci & 63u)) & 1ull);
                        else tri = raster_freq_trinary(v);
                        cls = tri == (int8_t)100 ? RAY_OCCUPIED : (tri == (int8_t)0 ? RAY_NONE : RAY_UNKNOWN);
                    }
                }
            }
            if (cls == RAY_OCCUPIED || (cls == RAY_UNKNOWN && stop_unknown)) { status = cls; step = (int)k; sx = cx; sy = cy; break; }
        }
        if (!live) continue;
        const uint32_t end = dm_sqdist_cell(prm, pv.dm_dir, pv.dm_sv, g.mhx, g.mhy);
        const size_t o = (size_t)pose * n + i;
        out.status[o] = (uint8_t)status;
        if (out.step) out.step[o] = step;
        if (out.nn) out.nn[o] = nn;
        if (out.cell_xy) { out.cell_xy[2 * o] = sx; out.cell_xy[2 * o + 1] = sy; }
        if (out.end_sqdist) out.end_sqdist[o] = end;
        if (out.label) {
            const int64_t tol = tolerance;
            const bool blocked = status == RAY_OCCUPIED && (int64_t)nn - 1 - (int64_t)step > tol;
            out.label[o] = (uint8_t)(blocked ? RAY_BLOCKED : ((int64_t)end <= tol * tol ? RAY_AGREES : RAY_NOVEL));
        }
    }
}

} // namespace lama_dev
