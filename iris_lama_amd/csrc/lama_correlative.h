// lama_correlative.h -- k_search_lattice: the score of EVERY pose of a regular lattice (headings x cell-aligned translations) against
// one distance map, and the best node of every tile of it (lama_hip_match_search_lattice, include/lama_hip.h) -- correlative scan
// matching (Olson 2009) as the stage that produces the pose guess which k_match_solve_batch then refines.
//
// A translation by whole cells moves every point's cell by the same whole cells, so a heading's points are turned into cells ONCE
// (the transform of the heading comes from the host, 12 doubles: no trigonometry here) and a node's score is a sum of the squared
// distances the map stores -- integer additions, exact in any order, which is what lets the waves of a workgroup split the point list
// freely and the tests compare bit for bit.
//
// One workgroup of CS_BLOCK threads per (tile, heading): every thread turns points into cells in LDS (CS_CHUNK at a time, a scan of
// any length), then lane = node of the tile in each of the four waves, wave w takes the w-th quarter of the staged cells: the cell
// is a broadcast LDS read, the gather's addresses differ by cell_step cells along a tile row, i.e. neighbouring lanes read the same
// rows of the same few patches.  The waves' partial sums meet in LDS, wave 0 forms the keys and reduces their minimum.
#pragma once
#include "lama_kernels.h"

namespace lama_dev {

constexpr int CS_BLOCK = 256;
constexpr int CS_WAVES = CS_BLOCK / 64;
constexpr int CS_NODES = 64;               // nodes of a tile at most: one per lane
constexpr int CS_CHUNK = 1024;             // rotated cells staged per pass (8 KiB)

// tfs [H][12]: fixed_tf({c_h, s_h, wx0, wy0}) * moving_tf per heading, rows of R then t (host_scan_tf); point i of the call is
// pts[point_step * i], i < n_used.  best_out [H][tiles_y][tiles_x], scores_out [H][ny][nx] or nullptr.
__global__ __launch_bounds__(CS_BLOCK) void k_search_lattice(DevParams prm, int particle, const double* __restrict__ pts, uint32_t n_used,
                                                              uint32_t point_step, const double* __restrict__ tfs, uint32_t cell_step,
                                                              uint32_t nx, uint32_t ny, uint32_t tile, uint32_t tiles_x, uint32_t tiles_y,
                                                              uint64_t total, uint64_t* __restrict__ best_out, uint32_t* __restrict__ scores_out)
{
    __shared__ uint2 cells[CS_CHUNK];
    __shared__ uint32_t part[CS_WAVES][64];
    const PV pv_ = pview_w(prm, particle);
    const int16_t* dir = pv_.dm_dir;
    const sv_t* sv = pv_.dm_sv;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t lx = lane % tile, ly = lane / tile;
    for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {         // (workgroup-uniform: the barriers below are reached by all)
        const uint32_t tx = (uint32_t)(w % tiles_x), ty = (uint32_t)((w / tiles_x) % tiles_y), h = (uint32_t)(w / ((uint64_t)tiles_x * tiles_y));
        // (what the host wrote for this call is read with agent-scope loads, never through the scalar cache: lama_dev.h)
        double t12[12];
        uload_f64_w<12>(tfs + 12 * (size_t)h, t12);
        Affine tf;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) tf.R[i][j] = t12[3 * i + j];
            tf.t[i] = t12[9 + i];
        }
        const uint32_t ix = tx * tile + lx, iy = ty * tile + ly;
        const bool live = ly < tile && ix < nx && iy < ny;             // (edge tiles are partial; lanes beyond tile * tile idle)
        const uint32_t dx = cell_step * ix, dy = cell_step * iy;
        uint32_t sum = 0;
        for (uint32_t base = 0; base < n_used; base += CS_CHUNK) {
            const uint32_t cnt = n_used - base < (uint32_t)CS_CHUNK ? n_used - base : (uint32_t)CS_CHUNK;
            for (uint32_t j = threadIdx.x; j < cnt; j += CS_BLOCK) {
                const double* q = pts + 3 * ((size_t)(base + j) * point_step);
                const double px = cload_f64(q), py = cload_f64(q + 1), pz = cload_f64(q + 2);
                double hx, hy;
                hit_xy(tf, px, py, pz, hx, hy);
                cells[j] = make_uint2(w2m(prm, hx), w2m(prm, hy));
            }
            __syncthreads();
            const uint32_t per = (cnt + CS_WAVES - 1) / CS_WAVES;
            const uint32_t j0 = wave * per < cnt ? wave * per : cnt, j1 = j0 + per < cnt ? j0 + per : cnt;
            if (live)
                for (uint32_t j = j0; j < j1; ++j) {
                    const uint2 c = cells[j];
                    sum += dm_sqdist_cell(prm, dir, sv, c.x + dx, c.y + dy);
                }
            __syncthreads();
        }
        part[wave][lane] = sum;
        __syncthreads();
        if (wave == 0) {
            uint32_t s = part[0][lane];
#pragma unroll
            for (int k = 1; k < CS_WAVES; ++k) s += part[k][lane];
            const uint32_t index = (h * ny + iy) * nx + ix;
            unsigned long long key = live ? (((unsigned long long)s << 32) | index) : ~0ull;
            if (live && scores_out) scores_out[index] = s;
            // keys are unique, so the minimum is one node whatever the order of the exchange
            for (int m = 32; m >= 1; m >>= 1) {
                const unsigned long long o = __shfl_xor(key, m);
                key = o < key ? o : key;
            }
            if (lane == 0) best_out[w] = key;
        }
        __syncthreads();                                               // (part and cells are the next tile's too)
    }
}

} // namespace lama_dev
