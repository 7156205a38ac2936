// lama_match_batch.h -- k_match_solve_batch: B independent scan-to-map registrations in one launch, with the robust cost the
// caller names (lama_hip_match_solve_batch, include/lama_hip.h).  The single-problem entry points (lama_hip_match_solve,
// lama_hip_match_solve_with: Solve(options, MatchSurface2D(dm, scan, pose), &cov) as Loc2D::update uses it, src/loc2d.cpp:168-180)
// run it on a batch of one with the compile-time CauchyWeight(0.15) of lama_kernels.h.
//
// One workgroup of SM_BLOCK threads per problem, the workgroup of k_scan_match: the same beams per thread, the same
// block_sum tree, the same single-lane step (gn_solve, lama_kernels.h).  A problem is a latency chain -- evaluate, reduce, step,
// evaluate -- of a few microseconds per link; nothing is gained by tiling one problem wider, everything by running many chains
// side by side.  What differs per problem comes from memory: whose distance map, which slice of the
// concatenated points, the sensor mount, the start pose, the iteration limit.  What differs per call is compiled in: the weight
// policy (five instantiations per BIGSQ) and, through DevParams, the strategy.
#pragma once
#include "lama_kernels.h"

namespace lama_dev {

// RobustCost::value of the reference's five classes (src/nlls/robust_cost.cpp:36-82), the parameter as the class stores it
struct WUnit {
    double p;                                                       // (unused: every policy travels as one double)
    __device__ inline double operator()(double) const { return 1.0; }
};
struct WTukey {
    double bb;                                                      // bb_ = b * b
    __device__ inline double operator()(double x) const
    {
        const double xx = x * x;
        if (xx <= bb) { const double w = 1.0 - xx / bb; return w * w; }
        return 0.0;
    }
};
struct WTDist {
    double dof;
    __device__ inline double operator()(double x) const { return ((dof + 1.0) / (dof + (x * x))); }      // (dof_ + 1.0f: the float literal is exact)
};
struct WCauchy {
    double c;                                                       // c_ = 1 / (param * param), computed on the host
    __device__ inline double operator()(double x) const { return (1.0 / (1.0 + x * x * c)); }
};
struct WHuber {
    double k;
    __device__ inline double operator()(double x) const { return (x < k) ? 1.0 : (k / fabs(x)); }        // the reference tests x, not |x|
};

// one problem of a batch (two quadwords: read with uload_rec)
struct MsbProblem {
    uint32_t particle;      // whose distance map
    uint32_t off, n;        // its points: [off, off + n) of the concatenated array
    uint32_t max_iter;      // 0: evaluate only
};
static_assert(sizeof(MsbProblem) == 16, "MsbProblem is read as two quadwords");

// poses_io [B][4] {c, s, tx, ty}; mtfs [B][12] = the sensor mount of every problem (Translation(origin) * q, rows of R then t);
// out8 [B][8]: [0..5] lower triangle of J^T J with the weighted J at the returned pose (Solver::solve cov branch,
// src/nlls/solver.cpp:109-116), [6] sum of squared UNWEIGHTED residuals (RMSE, src/loc2d.cpp:178-180), [7] sum of squared CELL
// distances (MatchSurface2D::error's terms, src/match_surface_2d.cpp:92-116); status [B]: 1 = a step produced a zero-norm unit complex (the reference throws SophusException).
template <bool BIGSQ, class WT>
__global__ __launch_bounds__(SM_BLOCK) __attribute__((amdgpu_num_vgpr(128))) void k_match_solve_batch(
    DevParams prm, const MsbProblem* __restrict__ problems, const double* __restrict__ pts_all,
    const double* __restrict__ mtfs, double* __restrict__ poses_io, double* __restrict__ out8, int32_t* __restrict__ iters_out,
    uint32_t* __restrict__ status_out, WT wt)
{
    __shared__ SMShared sh;
    __shared__ int numeric;
    // (everything the host wrote for this call is read with agent-scope loads, never through the scalar cache: lama_dev.h)
    const uint32_t b = blockIdx.x;
    const MsbProblem pb = uload_rec(problems + b);
    double m12[12];
    uload_f64_w<12>(mtfs + 12 * (size_t)b, m12);
    Affine mtf;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) mtf.R[i][j] = m12[3 * i + j];
        mtf.t[i] = m12[9 + i];
    }
    const PV pv_ = pview_w(prm, (int)pb.particle);
    const int16_t* dir = pv_.dm_dir;
    const sv_t* sv = pv_.dm_sv;
    const double* __restrict__ pts = pts_all + 3 * (size_t)pb.off;
    const int n = (int)pb.n;
    double* const pose_io = poses_io + 4 * (size_t)b;
    if (threadIdx.x == 0) {
        sh.state = load_pose(pose_io);
        sh.tf = scan_tf(sh.state, mtf);
        sh.ctl[0] = 0; sh.ctl[1] = 0;
        numeric = 0;
    }
    sm_build_lut(prm, sh.lut);
    __syncthreads();
    DevParams lp = prm;
    lp.max_iter = pb.max_iter;
    uint32_t evals = 0;
    const uint32_t iter = gn_solve<BIGSQ, WT>(lp, dir, sv, pts, n, mtf, sh, evals, wt, &numeric);
    // what the covariance, the RMSE and MatchSurface2D::error need at the solution
    double acc[10];
    const Affine tf = sh.tf;
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < n; i += SM_BLOCK) {
        const double px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
        double hx, hy;
        hit_xy(tf, px, py, pz, hx, hy);
        double gx, gy;
        const double r = dm_distance(prm, dir, sv, hx, hy, &gx, &gy);
        const double w = sqrt(wt(r));
        const double j0 = gx * w, j1 = gy * w, j2 = (gy * hx - gx * hy) * w;
        acc[0] += j0 * j0; acc[1] += j1 * j0; acc[2] += j1 * j1;
        acc[3] += j2 * j0; acc[4] += j2 * j1; acc[5] += j2 * j2;
        acc[6] += r * r;
        const double dc = dm_distance_cell(prm, dir, sv, w2m(prm, hx), w2m(prm, hy));
        acc[7] += dc * dc;
    }
    block_sum<10>(acc, sh.red, sh.tot);
    if (threadIdx.x == 0) {
        pose_io[0] = sh.state.c; pose_io[1] = sh.state.s; pose_io[2] = sh.state.tx; pose_io[3] = sh.state.ty;
        for (int k = 0; k < 8; ++k) out8[8 * (size_t)b + k] = sh.tot[k];
        iters_out[b] = (int32_t)iter;
        status_out[b] = (uint32_t)numeric;
    }
}

} // namespace lama_dev
