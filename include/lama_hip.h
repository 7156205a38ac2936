/* =====================================================================================
 * lama_hip.h -- C-ABI of the MI355X (gfx950) particle-filter scan-matching path.
 *
 * This is the drop-in boundary.  The reference has no FFI layer: its seam
 * is the C++ class API of include/lama/ (static library `iris_lama`).  The entry points below
 * are what a host-side `lama::PFSlam2D` calls INSTEAD of the bodies of the reference's two
 * per-particle parallel regions and of resample():
 *
 *   reference (file:line, relative to /root/reference)            entry point here
 *   -----------------------------------------------------------   --------------------------
 *   PFSlam2D::update first-scan block   src/pf_slam2d.cpp:185-228  lama_hip_pf_init
 *   region 1: scanMatch per particle    src/pf_slam2d.cpp:254-266  lama_hip_pf_scan_match
 *     = MatchSurface2D::eval            src/match_surface_2d.cpp:42-90
 *     + Solver::solve / GaussNewton     src/nlls/solver.cpp:53-107, src/nlls/gauss_newton.cpp:53-86
 *     + CauchyWeight                    src/nlls/robust_cost.cpp:66-73
 *     + calculateLikelihood             src/pf_slam2d.cpp:393-414
 *   resample(): particle-set copy       src/pf_slam2d.cpp:558-574  lama_hip_pf_resample
 *   region 2: updateParticleMaps        src/pf_slam2d.cpp:292-302  lama_hip_pf_update_maps
 *     = Map::computeRay                 src/sdm/map.cpp:198-227
 *     + FrequencyOccupancyMap::set*     src/sdm/frequency_occupancy_map.cpp:65-91
 *     + DynamicDistanceMap add/remove/update  src/sdm/dynamic_distance_map.cpp:160-330
 *   getOccupancyMap()/getDistanceMap()  include/lama/pf_slam2d.h:211-225  lama_hip_pf_download_map
 *   Particle::pose read/write           include/lama/pf_slam2d.h:77      lama_hip_pf_set_poses / _get_poses
 *
 * Host-side pieces that stay on the host (RNG order is part of the result): drawFromMotion
 * (:365-391), normalize (:511-535), systematic-resampling index generation (:537-556).
 *
 * Conventions
 *   - plain C, POD arguments only; no exceptions, STL, Eigen or torch types cross this boundary;
 *   - every function returns int32_t status: LAMA_HIP_OK (0) or a negative LAMA_HIP_E_* code;
 *     lama_hip_last_error() gives a human-readable message for the last failure on that context;
 *   - host buffers are borrowed for the duration of the call; outputs go to caller-provided arrays;
 *   - calls on one context must be serialised by the caller (same contract as PFSlam2D::update);
 *   - a pose is the reference's SE2 state: 4 doubles {c, s, tx, ty} (unit complex + translation,
 *     include/lama/sophus/se2.hpp); the scan is PointCloudXYZ (include/lama/types.h:111-120):
 *     n x 3 doubles + sensor_origin_[3] + sensor_orientation_ quaternion {w,x,y,z}.
 * ===================================================================================== */
#ifndef LAMA_HIP_H
#define LAMA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LAMA_HIP_OK 0
#define LAMA_HIP_E_INVALID (-1)    /* bad argument / unsupported option                         */
#define LAMA_HIP_E_HIP (-2)        /* a HIP runtime call failed                                 */
#define LAMA_HIP_E_WINDOW (-3)     /* a cell fell outside the device map window                 */
#define LAMA_HIP_E_CAPACITY (-4)   /* patch arena / brushfire queue capacity exceeded           */
#define LAMA_HIP_E_STATE (-5)      /* call sequence error (e.g. scan_match before init)         */
#define LAMA_HIP_E_NUMERIC (-6)    /* zero-norm unit complex (the reference throws SophusException) */

typedef struct lama_hip_ctx lama_hip_ctx;

/* Subset of PFSlam2D::Options (include/lama/pf_slam2d.h:132-185) the device path needs, plus
 * device-side capacities (0 = default). */
typedef struct lama_hip_cfg {
    uint32_t particles;          /* particles owned by THIS context (one shard of the pool)       */
    double resolution;           /* Options::resolution (0.05)                                    */
    uint32_t patch_size;         /* Options::patch_size; only 32 is supported on the device       */
    double l2_max;               /* Options::l2_max -> DynamicDistanceMap::setMaxDistance.  ceil(l2_max / resolution) <= 127 cells in
                                    liblama_hip.so; liblama_hip_wide.so -- the same sources and the same C-ABI, built with a 4-byte
                                    distance plane -- takes up to 255 cells, which is all the reference's own record can hold
                                    (distance_t::sqdist is a uint16_t).  The host classes and iris_lama_amd.ffi bind the library
                                    that the reach of the map asks for; a C caller links the one it needs.               */
    double meas_sigma;           /* Options::meas_sigma (likelihood divisor, pf_slam2d.cpp:411)   */
    uint32_t max_iter;           /* Options::max_iter                                             */
    double truncated_ray;        /* Options::truncated_ray                                        */
    double truncated_range;      /* Options::truncated_range                                      */
    int32_t device;              /* HIP device ordinal                                            */
    uint32_t window_patches;     /* INITIAL side of the square map window in patches (default 128 = 204.8 m; a multiple of 8).  The window
                                    follows the robot and GROWS (re-allocated at least half as large again) when the mapped area
                                    outgrows it, up to 1016 patches = 1.6 km at 0.05 m; only a wider map is LAMA_HIP_E_WINDOW */
    uint32_t dm_patch_capacity;  /* smallest DM region a particle gets, in patches (default 128: 10 m x 10 m of map; regions grow on demand).  The reference's maps are unbounded; here
                                    every particle owns one contiguous region per map kind inside pooled planes: the region grows with
                                    ITS particle's map (moved to a larger one, that particle alone, when it runs short), the pools grow
                                    chunk by chunk.  A map update that needs more patches than are free reports that BEFORE it modifies
                                    any cell (its allocation phase comes first), upon which the particles that ran short get what they
                                    asked for and the update is run again.  LAMA_HIP_E_CAPACITY remains for the hard limit of 32767
                                    patches per particle and map, and for a device that has no memory left for another pool chunk */
    uint32_t occ_patch_capacity; /* smallest occupancy region a particle gets (default 128)      */
    uint32_t queue_capacity;     /* brushfire queue entries per particle (default 32768, at least 8192; brushfire_mode = 1: see there) */
    uint32_t profile;            /* !=0: bracket every kernel with hipEvents (lama_hip_get_counters) */
    uint32_t active_capacity;    /* parallel ray-cast: max. order-sensitive cell visits per particle and scan (default 8192) */
    uint32_t sequential_raycast; /* ray-cast kernels: 0 / 2 = parallel form (default), 1 = beam-sequential form; bit-identical */
    uint32_t brushfire_mode;     /* 0 = exact (default): bit-identical to the reference incl. libstdc++'s tie order;
                                    1 = level-synchronous with a canonical tie rule (parallel; identical sqdist/valid/masks on
                                        the measured logs, obstacle offsets of tie cells -- and, once in millions of cells, a
                                        distance -- may differ).  NOT bit-identical: only a caller that sets
                                        this field gets it (no environment variable selects it) and lama_hip_get_counters
                                        reports the mode that ran.  Other values are rejected.
                                        Limits of mode 1 (lama_brushfire_canon.h).  A particle's update is left, untouched, to
                                        the exact kernels -- the result is then the exact one -- when the map's reach is above
                                        32 cells (max_sqdist > 1024; always in liblama_hip_wide.so) or when one scan removes or
                                        adds more obstacle cells than queue_capacity / 2.  Its LDS table of 4096 cells does NOT
                                        limit the cells of a level or of a raise round: larger ones are worked in passes.
                                        queue_capacity bounds the cells ONE update lowers (the pending list is append-only; for
                                        the exact kernels it bounds the front at its widest): beyond it, and in the unlikely
                                        case that one pass's class of 8 x 8 blocks alone holds more than 4096 distinct cells,
                                        the update ends with LAMA_HIP_E_CAPACITY after cells have been modified, as a full
                                        queue of the exact kernels does. */
    uint32_t brushfire_waves;    /* exact brushfire: 0 / 2 = a helper wave per particle owns the heap (default), 1 = one wave per
                                    particle; bit-identical */
    uint32_t occupancy_policy;   /* cell policy of the occupancy map: 0 = FrequencyOccupancyMap {uint16 occupied, uint16 visited}
                                    (PFSlam2D, Slam2D); 1 = ProbabilisticOccupancyMap {float log-odds}
                                    (src/sdm/probabilistic_occupancy_map.cpp:53-107; LidarOdometry2D) -- beam-sequential ray-cast */
    uint32_t ray_rule;           /* where a ray starts: 0 = PFSlam2D/Slam2D (truncated_ray / truncated_range options),
                                    1 = LidarOdometry2D::updateMaps (src/lidar_odometry_2d.cpp:108-114: the last metre before the hit) */
    uint32_t solver_strategy;    /* nlls strategy of the scan matcher: 0 = GaussNewton (src/nlls/gauss_newton.cpp; PFSlam2D always),
                                    1 = LevenbergMarquard (src/nlls/levenberg_marquardt.cpp; Slam2D / Loc2D with strategy "lm") */
} lama_hip_cfg;

void lama_hip_default_cfg(lama_hip_cfg* cfg);

int32_t lama_hip_device_count(int32_t* count);

int32_t lama_hip_ctx_create(const lama_hip_cfg* cfg, lama_hip_ctx** out);
void lama_hip_ctx_destroy(lama_hip_ctx* ctx);
const char* lama_hip_last_error(const lama_hip_ctx* ctx);

/* First scan (src/pf_slam2d.cpp:185-228): every particle's pose = pose0; particle 0 builds its maps
 * from the scan (updateParticleMaps), all others become copies of particle 0. */
int32_t lama_hip_pf_init(lama_hip_ctx* ctx, const double* pts_xyz, uint32_t n,
                         const double* sensor_origin3, const double* sensor_quat_wxyz,
                         const double* pose0);

/* Particle poses, P x 4 doubles {c,s,tx,ty}. */
int32_t lama_hip_pf_set_poses(lama_hip_ctx* ctx, const double* poses);
int32_t lama_hip_pf_get_poses(lama_hip_ctx* ctx, double* poses);

/* Region 1 (scanMatch): per particle, Gauss-Newton + Cauchy(0.15) on the particle's own distance map
 * starting from its current pose; the refined pose replaces the particle's pose.
 * Outputs (any may be NULL): poses_out P x 4, loglik_out P (calculateLikelihood),
 * iters_out P (Solver iterations = applied + reverted steps). */
int32_t lama_hip_pf_scan_match(lama_hip_ctx* ctx, const double* pts_xyz, uint32_t n,
                               const double* sensor_origin3, const double* sensor_quat_wxyz,
                               double* poses_out, double* loglik_out, int32_t* iters_out);

/* resample(): new particle i := copy of old particle sample_idx[i] (pose + both maps). */
int32_t lama_hip_pf_resample(lama_hip_ctx* ctx, const int32_t* sample_idx);

/* Region 2 (updateParticleMaps): per particle ray-cast of the scan from the particle's pose into its
 * FrequencyOccupancyMap, add/remove obstacle events into its DynamicDistanceMap, then dm->update().
 * pts_xyz may be NULL to reuse the scan (same n) uploaded by the preceding lama_hip_pf_scan_match call. */
int32_t lama_hip_pf_update_maps(lama_hip_ctx* ctx, const double* pts_xyz, uint32_t n,
                                const double* sensor_origin3, const double* sensor_quat_wxyz);

/* Map download in the REFERENCE's record formats, so a host lama::Map can be rebuilt byte for byte:
 *   kind LAMA_HIP_MAP_DISTANCE : cells are DynamicDistanceMap::distance_t (10 B:
 *        int16 obstacle[3], uint16 sqdist, bool valid_obstacle, bool is_queued), 10240 B / patch
 *   kind LAMA_HIP_MAP_OCCUPANCY: cells are FrequencyOccupancyMap::frequency (4 B: uint16 occupied,
 *        uint16 visited), 4096 B / patch
 *   patch_ids: the reference's 64-bit patch index (Map::m2p, include/lama/sdm/map.h:153-161), ascending
 *   masks    : 16 x uint64 per patch (Container::mask, include/lama/sdm/container.h:57-65)
 * lama_hip_pf_map_patches returns the number of patches; download fills up to `cap` patches. */
#define LAMA_HIP_MAP_DISTANCE 0
#define LAMA_HIP_MAP_OCCUPANCY 1
int32_t lama_hip_pf_map_patches(lama_hip_ctx* ctx, uint32_t particle, int32_t kind, uint32_t* num_patches);
int32_t lama_hip_pf_download_map(lama_hip_ctx* ctx, uint32_t particle, int32_t kind, uint32_t cap,
                                 uint64_t* patch_ids, uint8_t* cells, uint64_t* masks, uint32_t* num_patches);

/* The inverse of lama_hip_pf_download_map -- Map::read (src/sdm/map.cpp:533-575) for a map that lives on the device: particle
 * `particle`'s map of `kind` is REPLACED by the given patches (the reference's record formats, as download returns them and as a
 * `.sdm` file stores them: lama::sdm::read).  A distance map built elsewhere -- by the reference, by an earlier run, by another
 * context -- is put in place without replaying addObstacle() + update(): Loc2D's static map of a building is one serial brushfire
 * chain of millions of pops when it is built on the device (bench.py: next_rows.loc2d_map_load), a file read when it is loaded.
 * patch_ids need not be sorted; a patch outside the largest window is LAMA_HIP_E_WINDOW.  On a context that has not seen
 * lama_hip_pf_init it also places the map window (like lama_hip_map_add_obstacles). */
int32_t lama_hip_pf_upload_map(lama_hip_ctx* ctx, uint32_t particle, int32_t kind, uint32_t num_patches,
                               const uint64_t* patch_ids, const uint8_t* cells, const uint64_t* masks);

/* The same map update split in two, so that the host work of the NEXT scan (odometry prediction, motion sampling) overlaps
 * with the kernels: _begin queues the work on the context's stream and returns; its status (window / capacity errors) and
 * counters are collected by lama_hip_sync, or implicitly at the start of the next call on the context, whichever comes
 * first -- a deferred error is then returned by THAT call (message prefixed "deferred from ...").
 * lama_hip_pf_update_maps == _begin followed by lama_hip_sync. */
int32_t lama_hip_pf_update_maps_begin(lama_hip_ctx* ctx, const double* pts_xyz, uint32_t n,
                                      const double* sensor_origin3, const double* sensor_quat_wxyz);
int32_t lama_hip_sync(lama_hip_ctx* ctx);
/* One whole device step of a filter: lama_hip_pf_set_poses(poses_in) + lama_hip_pf_scan_match + lama_hip_pf_update_maps_begin of the
 * MATCHED poses, i.e. a step in which the resample, if one is due, follows the map update instead of preceding it.  That order gives
 * the same poses and maps bit for bit (a resample copies a particle's pose and both maps and touches nothing else; a particle's map
 * update is a function of its own pose, its own maps and the scan), and it lets a pool below the routing threshold (64 particles)
 * run as contiguous particle groups (three by default), each on a stream of its own: a group goes on to its ray-cast and brushfire as soon
 * as ITS scan match is back, and the call returns, with all results, while every group's map update is still queued or running.
 * Nothing in it waits for a map update: the status of a group's update travels with the results of the group's next scan match, so
 * a deferred error is returned by the next call on the context, as with _begin.  Every other entry point first waits for all groups.
 * A lama_hip_pf_resample that follows while the groups are still running is likewise only recorded and carried out by the next call
 * on the context (its error, if any, is that call's), so that the caller's host work of the next step runs beside the map kernels.
 * Larger pools, and scans or configurations that need more than the plain parallel map update, run the three calls above as they
 * are.  poses_out [P][4] / loglik_out [P] / iters_out [P] may be NULL.  LAMA_HIP_STEP_GROUPS=n in the environment at context
 * creation overrides the number of groups (1 .. 4; 1 = the single-stream schedule). */
int32_t lama_hip_pf_match_and_map(lama_hip_ctx* ctx, const double* pts_xyz, uint32_t n, const double* sensor_origin3,
                                  const double* sensor_quat_wxyz, const double* poses_in, double* poses_out, double* loglik_out,
                                  int32_t* iters_out);
/* After an error return of lama_hip_pf_match_and_map the step is LOST and must not be repeated: the groups taken before the failing one
 * have queued their map update of this scan already (a second call with the same scan would integrate it twice there), and the
 * context's poses are a mix of matched and predicted ones.  The context itself takes further calls as after any other failed call.
 *
 * *ran: how many particle groups the last lama_hip_pf_match_and_map of the context really ran (empty groups of a pool with fewer
 * particles than groups do not count; 1: the single-stream schedule; 0: none yet) -- waits for the device like every other entry
 * point.  *configured: into how many groups a step of this context is split when it can be (0: never -- a pool of 64 particles or
 * more, or an override of 1: every step is the three calls above), fixed at creation; asking
 * for it alone (ran == NULL) waits for nothing.  Either pointer may be NULL.  (These two figures are not members of
 * lama_hip_counters.) */
int32_t lama_hip_pf_step_groups(lama_hip_ctx* ctx, uint32_t* ran, uint32_t* configured);
/* HIP device ordinal the context lives on (cfg.device); < 0 for a null context.  Lets a caller of a multi-GPU object check
 * that its shards really sit on distinct devices. */
int32_t lama_hip_ctx_device(const lama_hip_ctx* ctx);

/* Patch bookkeeping for transient maps (LidarOdometry2D::updateMaps, src/lidar_odometry_2d.cpp:128-199):
 *   lama_hip_pf_patch_ids     : Map::visit_all_patches -- the reference patch indices (Map::m2p) of the allocated patches;
 *   lama_hip_pf_delete_patches: Map::deletePatchAt (src/sdm/map.cpp:465-488) on BOTH maps of the particle for every listed patch
 *                               index (absent patches, duplicates and indices outside the window are skipped); the arenas stay dense.
 *                               *deleted = distance-map patches removed.  Cells of the surviving patches keep their obstacle offsets
 *                               into a deleted patch, as the reference's do; from the first removed distance-map patch on, the
 *                               context's brushfire re-creates such a patch when it reads the obstacle cell ("What a
 *                               deletion leaves behind"). */
int32_t lama_hip_pf_patch_ids(lama_hip_ctx* ctx, uint32_t particle, int32_t kind, uint32_t cap, uint64_t* patch_ids, uint32_t* num_patches);
/* One 64-bit checksum per particle of its distance / occupancy map, computed on the device: order-independent sum over the
 * allocated patches (reference patch indices, Map::m2p) and their cells of a hash of what the reference stores per cell
 * (distance_t / frequency, include/lama/sdm/dynamic_distance_map.h:48-53, frequency_occupancy_map.h:43-46) and of the
 * Container mask bit (include/lama/sdm/container.h:167-183).  Two maps with equal patch sets, cells and masks have equal
 * checksums; used to compare ALL particles of a large filter with a checker without downloading the maps.  out: P values. */
int32_t lama_hip_pf_map_checksums(lama_hip_ctx* ctx, int32_t kind, uint64_t* out);
int32_t lama_hip_pf_delete_patches(lama_hip_ctx* ctx, uint32_t particle, const uint64_t* patch_ids, uint32_t n, uint32_t* deleted);

/* Batched evaluation on ONE particle's distance map (Loc2D::globalLocalization-style):
 * B poses -> B log-likelihoods (calculateLikelihood) without changing any state. */
int32_t lama_hip_match_batch(lama_hip_ctx* ctx, uint32_t particle, const double* pts_xyz, uint32_t n,
                             const double* sensor_origin3, const double* sensor_quat_wxyz,
                             const double* poses, uint32_t num_poses, double* loglik_out);

/* Loc2D::globalLocalization's candidate evaluation (src/loc2d.cpp:249-286, the loop body :271-284): for each of the
 * B poses {c, s, tx, ty} the squared norm of MatchSurface2D's residuals (bilinear distance per point, no robust
 * weight; src/match_surface_2d.cpp:58-101) on `particle`'s distance map, and/or the particle filter's log-likelihood
 * (either output may be NULL).  No state changes.  The candidates themselves are drawn on the host (random::uniform). */
int32_t lama_hip_eval_batch(lama_hip_ctx* ctx, uint32_t particle, const double* pts_xyz, uint32_t n,
                            const double* sensor_origin3, const double* sensor_quat_wxyz,
                            const double* poses, uint32_t num_poses, double* sqnorm_out, double* loglik_out);

/* Loc2D::addSamplingCovariance's likelihood samples (src/loc2d.cpp:199-234): for each of the K world positions
 * xy[k] the scan is placed there with heading `yaw`; every `point_step`-th point (0, step, 2 step, ...; at most
 * LAMA_HIP_SAMPLE_MAX_TERMS of them, which covers Loc2D's step = max(n / 100, 1) for every n; more is refused with
 * LAMA_HIP_E_INVALID) looks up the NON-interpolated distance d and l_out[k] = sum exp(-d^2 / 0.01)^3, summed in point order. */
#define LAMA_HIP_SAMPLE_MAX_TERMS 256
int32_t lama_hip_map_sample_likelihood(lama_hip_ctx* ctx, uint32_t particle, const double* pts_xyz, uint32_t n,
                                       const double* sensor_origin3, const double* sensor_quat_wxyz, double yaw,
                                       const double* xy, uint32_t num_samples, uint32_t point_step, double* l_out);

/* Static-map localisation support (Loc2D, src/loc2d.cpp:61-192) on a one-particle context:
 *  lama_hip_map_add_obstacles: DynamicDistanceMap::addObstacle for every cell of the list (map coordinates as
 *      returned by Map::w2m, x then y, in the given order) followed by dm->update().  On a context that has not seen
 *      lama_hip_pf_init it also places the map window (centred on the first cell).
 *  lama_hip_match_solve: Solve(GaussNewton + Cauchy(0.15), MatchSurface2D(dm, scan, pose), &cov): pose_inout {c,s,tx,ty};
 *      out7 = lower triangle of J^T J (weighted J at the solution: 00,10,11,20,21,22) and the sum of squared unweighted
 *      residuals; iters_out = solver iterations.  do_solve == 0 only evaluates at the given pose.  (One problem of
 *      lama_hip_match_solve_batch's kernel, below, with the weight compiled in.) */
int32_t lama_hip_map_add_obstacles(lama_hip_ctx* ctx, uint32_t particle, const uint32_t* cells_xy, uint32_t n);
int32_t lama_hip_match_solve(lama_hip_ctx* ctx, uint32_t particle, const double* pts_xyz, uint32_t n,
                             const double* sensor_origin3, const double* sensor_quat_wxyz, double* pose_inout,
                             double* out7, int32_t* iters_out, int32_t do_solve);
/* The same with the strategy chosen per call (0 = GaussNewton, 1 = LevenbergMarquard) instead of cfg.solver_strategy:
 * and its own iteration limit: Solve(options, MatchSurface2D&, &cov) of a caller that builds its own Solver::Options
 * (include/lama/nlls/solver.h:52-67). */
int32_t lama_hip_match_solve_with(lama_hip_ctx* ctx, uint32_t particle, const double* pts_xyz, uint32_t n,
                                  const double* sensor_origin3, const double* sensor_quat_wxyz, double* pose_inout,
                                  double* out7, int32_t* iters_out, int32_t strategy, uint32_t max_iterations /* 0: cfg.max_iter */);
/* MatchSurface2D::eval (src/match_surface_2d.cpp:42-90; the reference's nlls::Problem interface, include/lama/nlls/problem.h:
 * 40-57) against particle `particle`'s distance map at pose {c,s,tx,ty}: residuals[n] = interpolated distance at every beam's
 * end point (no robust weight), jacobian (may be NULL) = n x 3 COLUMN-major [gx | gy | gy*hx - gx*hy]. */
int32_t lama_hip_match_eval(lama_hip_ctx* ctx, uint32_t particle, const double* pts_xyz, uint32_t n,
                            const double* sensor_origin3, const double* sensor_quat_wxyz, const double* pose,
                            double* residuals, double* jacobian);
/* The per-beam terms of MatchSurface2D::error (src/match_surface_2d.cpp:92-116): distances[i] = DynamicDistanceMap::distance
 * of the CELL w2m(tf * p_i) (no interpolation); the caller takes sqrt(sum of squares / n). */
int32_t lama_hip_match_cell_distances(lama_hip_ctx* ctx, uint32_t particle, const double* pts_xyz, uint32_t n,
                                      const double* sensor_origin3, const double* sensor_quat_wxyz, const double* pose,
                                      double* distances);

/* num_problems independent scan-to-map registrations in ONE launch, one workgroup each (csrc/lama_match_batch.h): what
 * lama_hip_match_solve_with does for one problem, for many, with the robust cost the caller names -- the matching stage of loop
 * closure (GraphSlam2D::correlateCandidateScan, src/graph_slam2d.cpp:315-355: HuberWeight(0.15), 1 then 100 iterations, then
 * error()), the refinement of many global-localisation candidates, a fleet on one map.  Problem b:
 *   particles[b]                     whose distance map it is matched against (no map is changed);
 *   pts_xyz, scan_offsets [B + 1]    its points scan_offsets[b] .. scan_offsets[b + 1] - 1 of the concatenated array (not empty);
 *   sensor_origin3_per_problem [B][3] / sensor_quat_wxyz_per_problem [B][4]   its sensor mount (NULL: zero / identity);
 *   poses_inout [B][4] {c,s,tx,ty}   start pose in, solution out;
 *   max_iterations [B]               its iteration limit; 0 evaluates out8 at the start pose, which is returned bit for bit.
 * Per call: strategy (0 = GaussNewton, 1 = LevenbergMarquard, default thresholds) and the weight RobustCost::value
 * (src/nlls/robust_cost.cpp:36-82) of robust_kind with robust_param: UnitWeight (parameter ignored, must be finite), TukeyWeight(b),
 * TDistributionWeight(dof), CauchyWeight(param), HuberWeight(k) -- the reference's formulas literally, Huber's test `x < k` included.
 * Out: out8 [B][8] = lower triangle of J^T J (weighted J at the solution: 00,10,11,20,21,22), the sum of squared unweighted
 * residuals, and the sum of squared CELL distances -- MatchSurface2D::error() is sqrt(out8[7] / n) --; iters_out [B];
 * status_out [B] (may be NULL): 0, or 1 where a step met a zero-norm unit complex (the reference throws SophusException).  Such a
 * problem makes the call return LAMA_HIP_E_NUMERIC with the problem named in lama_hip_last_error; every array is still written and
 * the other problems' results stand.  A CauchyWeight(0.15) problem returns bit for bit what lama_hip_match_solve_with returns.
 * LAMA_HIP_E_INVALID, found before anything is uploaded and with every array untouched: an empty slice, a particle out of range, a
 * non-finite point, pose, mount or parameter, an unknown kind or strategy, a parameter for which the reference's formula divides by
 * zero or weighs negatively (b == 0, param == 0, dof <= 0, k <= 0).  num_problems == 0 does nothing.  Workgroup b takes problem b:
 * the problems start in the order given.  Whether a ragged batch gains from starting its long scans first is NOT measured (DESIGN.md
 * section 4f); a caller who wants that order lists the problems so. */
#define LAMA_HIP_ROBUST_UNIT 0
#define LAMA_HIP_ROBUST_TUKEY 1
#define LAMA_HIP_ROBUST_TDIST 2
#define LAMA_HIP_ROBUST_CAUCHY 3
#define LAMA_HIP_ROBUST_HUBER 4
/* or-ed into robust_kind: robust_param is the constant as the reference's class STORES it -- TukeyWeight::bb_ = b * b, CauchyWeight::c_
 * = 1 / (param * param); the other classes store their argument -- so that a caller who holds the object need not undo its
 * constructor (lama::SolveBatch).  The same refusals apply to the stored constant. */
#define LAMA_HIP_ROBUST_STORED 0x100
int32_t lama_hip_match_solve_batch(lama_hip_ctx* ctx, uint32_t num_problems, const uint32_t* particles, const double* pts_xyz,
                                   const uint32_t* scan_offsets, const double* sensor_origin3_per_problem,
                                   const double* sensor_quat_wxyz_per_problem, double* poses_inout, const uint32_t* max_iterations,
                                   int32_t strategy, int32_t robust_kind, double robust_param, double* out8, int32_t* iters_out,
                                   uint32_t* status_out);

/* Exhaustive search of a regular pose lattice against `particle`'s distance map (csrc/lama_correlative.h): correlative scan matching
 * (Olson 2009), the stage that PRODUCES the start pose lama_hip_match_solve_batch refines -- what the reference approaches with 3000
 * random poses (Loc2D::globalLocalization, src/loc2d.cpp:249-286) and a coarse retry (GraphSlam2D::coarseSearchAndCorrelateCandidateScan).
 * The lattice: num_headings headings, given as headings_cs [H][2] = {cos, sin} COMPUTED BY THE CALLER, times nx x ny translations;
 * node (0, 0) is the world position (wx0, wy0), node (ix, iy) is node (0, 0) shifted by cell_step * (ix, iy) whole CELLS.  Of the
 * scan, points 0, point_step, 2 point_step, ... are used.  Definition:
 *   for heading h the pose is {c_h, s_h, wx0, wy0}; every used point i has the cell cell_i = w2m(hit_i), with hit_i formed as
 *   lama_hip_match_cell_distances forms it -- except that the pose's transform is composed on the host (libm): the device does no
 *   trigonometry, so the cells are the reference's bit for bit at every heading;
 *   score(h, ix, iy) = sum over i of q(cell_i + cell_step * (ix, iy)) in uint32 arithmetic, where q is the SQUARED distance in cells
 *   that the map stores for a cell with a valid obstacle, and the map's maximum squared distance (ceil(l2_max / resolution)^2) for a
 *   cell outside the window, in an absent patch, or without a valid obstacle -- DynamicDistanceMap::distance of the cell, before the
 *   square root and the resolution;
 *   best_out [H][ceil(ny / tile)][ceil(nx / tile)]: per tile of tile x tile nodes (partial at the upper edges) the smallest key
 *   ((uint64) score << 32) | index, index = (h * ny + iy) * nx + ix.  Keys are unique: equal scores go to the smaller index, and the
 *   result depends on no scheduling;
 *   scores_out [H][ny][nx] (may be NULL): every score.
 * No map, pose or counter of the context changes (the scan becomes the resident one, as with lama_hip_match_eval).
 * LAMA_HIP_E_INVALID, found before anything is uploaded and with every array untouched: n, point_step, num_headings, nx, ny,
 * cell_step or tile of 0; tile > 8 (a workgroup holds the 64 nodes of a tile, one per lane); a non-finite point, mount, heading entry
 * or origin; a particle out of range; num_headings * nx * ny >= 2^32; ceil(n / point_step) * max squared distance >= 2^32 (a score
 * must fit 32 bits: raise point_step); a lattice whose far corner, with the scan's reach around it, would leave the 32-bit range of map
 * cell coordinates. */
int32_t lama_hip_match_search_lattice(lama_hip_ctx* ctx, uint32_t particle, const double* pts_xyz, uint32_t n,
                                      const double* sensor_origin3, const double* sensor_quat_wxyz, uint32_t point_step,
                                      const double* headings_cs, uint32_t num_headings, double wx0, double wy0,
                                      uint32_t cell_step, uint32_t nx, uint32_t ny, uint32_t tile,
                                      uint64_t* best_out, uint32_t* scores_out);

/* Map rebuild from posed key scans (GraphSlam2D::generateOccupancyMap, src/graph_slam2d.cpp:131-164) on `particle`'s FREQUENCY
 * occupancy map, all scans in one order-free pass (csrc/lama_map_build.h).  Per scan k and point p, the reference's loop:
 * tf = T(pose_k) * T(sensor_origin_k) * R(sensor_quat_k); hit = tf * p; setOccupied(w2m(hit)); with flags bit 0 ("full") also
 * computeRay(w2m(tf.translation()), w2m(hit)) -- end points excluded -- with setFree on every cell.  No truncated_ray /
 * truncated_range (the reference applies none here).  The call ADDS to the map that is there: scans [0, a) then [a, K) in two calls
 * equal one call (the reference's mapping_keyid increment), and so does any order of the scans -- the uint16 counters commute, each
 * field modulo 2^16 on its own.  flags bit 1 ("prune") runs FrequencyOccupancyMap::prune afterwards
 * (src/sdm/frequency_occupancy_map.cpp:149-158: visited == 1 and occupied <= 1 becomes {0, 0}; masks and patches stay).  The
 * particle's distance map is not touched.
 *   poses4 [K][4] {c, s, tx, ty};  pts_xyz: the points of all scans, scan k = points scan_offsets[k] .. scan_offsets[k + 1] - 1
 *   (K + 1 non-decreasing offsets);  sensor_origin3_per_scan [K][3] / sensor_quat_wxyz_per_scan [K][4] (NULL: zero / identity).
 * Everything that can refuse the call -- LAMA_HIP_E_WINDOW (the scans, together with the map so far, are wider than the largest
 * window, or a ray is longer than 8191 cells), LAMA_HIP_E_CAPACITY, LAMA_HIP_E_INVALID (a non-finite point or pose) -- is found
 * BEFORE a patch is allocated or a cell changes.  On a context that has not seen lama_hip_pf_init the call also places the map
 * window (like lama_hip_map_add_obstacles).  num_scans == 0, or scans without any point, change nothing (prune included). */
#define LAMA_HIP_MAP_BUILD_FULL 1u
#define LAMA_HIP_MAP_BUILD_PRUNE 2u
int32_t lama_hip_map_integrate_scans(lama_hip_ctx* ctx, uint32_t particle, uint32_t num_scans, const double* poses4,
                                     const double* pts_xyz, const uint32_t* scan_offsets, const double* sensor_origin3_per_scan,
                                     const double* sensor_quat_wxyz_per_scan, uint32_t flags);
/* The map coordinates {x, y} of every cell of `particle`'s frequency occupancy map with isOccupied (visited != 0 and
 * occupied / visited > 0.25 evaluated in double, src/sdm/frequency_occupancy_map.cpp:38-45,132-138), compacted on the device, in
 * Map::visit_all_cells order: ascending reference patch index (Map::m2p), then the cell index inside the patch.  *n = their number;
 * up to `cap` of them are written to cells_xy (NULL: only the number is wanted). */
int32_t lama_hip_map_occupied_cells(lama_hip_ctx* ctx, uint32_t particle, uint32_t cap, uint32_t* cells_xy, uint32_t* n);

/* Map::bounds (src/sdm/map.cpp:139-157) of `particle`'s device map of `kind` (LAMA_HIP_MAP_*): min over the allocated patches'
 * anchors, max + 32, in map cells; one small reduction over the window directory on the device.  A map without patches:
 * *num_patches = 0, min = 0xFFFFFFFF, max = 32 (what lama::Map::bounds of its snapshot gives).  Any output pointer may be NULL. */
int32_t lama_hip_map_bounds(lama_hip_ctx* ctx, uint32_t particle, int32_t kind, uint32_t min_xy[2], uint32_t max_xy[2], uint32_t* num_patches);

/* `particle`'s map written out DENSE on the device (csrc/lama_raster.h), one element per `stride x stride` block of cells -- what a
 * nav_msgs/OccupancyGrid, a costmap or a viewer takes -- instead of the sparse reference records of lama_hip_pf_download_map.
 * Pixel (i, j), stored at out[j * width + i] (row-major, x fastest), covers the map cells [x0 + i * stride, x0 + (i + 1) * stride) x
 * [y0 + j * stride, y0 + (j + 1) * stride).  stride is 1, 2, 4, 8, 16 or 32; x0 and y0 are multiples of it (a block never straddles a
 * patch); width and height are 1 .. 32768 pixels; out_bytes == width * height * element size.  Anything else is LAMA_HIP_E_INVALID,
 * found before `out` is written.  The box may lie partly or wholly outside the allocated patches or the map window: those cells are
 * "absent", not an error.  Cell rules, exact and in integers:
 *   frequency cells (cfg.occupancy_policy 0): visited == 0 or absent -> unknown; 4 * occupied > visited -> occupied; 4 * occupied <
 *     visited -> free; equality -> unknown (identical to the reference's double comparison of occupied / visited with 0.25 for every
 *     uint16 pair, see csrc/lama_raster.h); probability = (200 * occupied + visited) / (2 * visited), at most 100;
 *   log-odds cells (policy 1): l < 0 free, l > 0 occupied, otherwise unknown (no probability layer: exp is not exact);
 *   distance cells: the stored sqdist where the cell is present and valid_obstacle is set, otherwise the context's max_sqdist.
 * Blocks (stride > 1): occupied if any cell is, else free if any cell is, else unknown; the largest probability of the visited cells,
 * else -1; the smallest squared distance.  Like every entry point the call first waits for queued map updates. */
#define LAMA_HIP_RASTER_TRINARY     0   /* int8:  0 free, 100 occupied, -1 otherwise  (isFree / else isOccupied / else, as the ROS nodes do) */
#define LAMA_HIP_RASTER_PROBABILITY 1   /* int8:  0..100 = round-half-up(100 * occupied / visited), -1 where visited == 0 or absent; policy 0 only */
#define LAMA_HIP_RASTER_SQDIST      2   /* uint16: squared distance in cells; max_sqdist where the cell is absent or has no valid obstacle */
int32_t lama_hip_map_rasterize(lama_hip_ctx* ctx, uint32_t particle, int32_t layer, uint32_t x0, uint32_t y0,
                               uint32_t width, uint32_t height, uint32_t stride, void* out, uint64_t out_bytes);

/* The FRONTIERS of `particle`'s occupancy map inside a box: where mapped free space ends and unknown space begins, grouped into
 * connected clusters with a size, a box and the sums a centroid needs (csrc/lama_frontier.h) -- the candidate places an exploring robot
 * drives to, and the seeds lama_hip_map_cast_rays(LAMA_HIP_RAY_STOP_UNKNOWN) takes.  Only the cluster list comes down, not the grid.
 * The definition is exact, in integers, and independent of how the device schedules the work:
 *   grid      the pixels of lama_hip_map_rasterize(LAMA_HIP_RASTER_TRINARY, x0, y0, width, height, stride), either occupancy policy;
 *             the same rules for x0, y0 and stride; pixel (i, j) has the index j * width + i;
 *   frontier  a pixel of the box with value 0 (free) of whose four EDGE neighbours at least one is -1 (unknown).  A diagonal unknown
 *             neighbour alone does not count, an occupied neighbour does not count.  Neighbours outside the box are classified from the
 *             map as well, as the raster of the box widened by one pixel per side gives them (absent patches and cells outside the map
 *             window are unknown) -- except that a neighbour whose cells would lie below coordinate 0 or above 2^32 - 1 does not exist
 *             and is not unknown.  The free cells on the rim of Map::bounds are therefore frontiers;
 *   cluster   an 8-connected component of the frontier pixels of the box (pixels outside the box never belong to one, nor do they
 *             join two); its label is the smallest pixel index among its pixels.
 * Outputs: *n = the number of clusters with pixels >= min_pixels (0 is taken as 1); *frontier_pixels (may be NULL) = ALL frontier
 * pixels, those of smaller clusters included; out[0 .. min(cap, *n)) = the records ordered by pixels descending, then label ascending
 * (out may be NULL with cap == 0; entries past *n are left alone); labels_out (may be NULL) [height][width] = the cluster's label at
 * every frontier pixel, small clusters included, 0xFFFFFFFF elsewhere; kernel_ms (may be NULL) = the device time of the call's
 * launches, from events (two brackets: the launches before and the one after the read-back of the count).
 * LAMA_HIP_E_INVALID, found before anything is written: the stride and origin rules of lama_hip_map_rasterize; width or height 0 or
 * above 32766 (room for the halo within the raster's 32768); width * height > 2^28; a particle out of range; n == NULL; out == NULL
 * with cap != 0.  A map without any occupancy patch: *n = 0, *frontier_pixels = 0, labels_out all 0xFFFFFFFF, no launch.
 * No map, pose or counter of the context changes; like every entry point the call first waits for queued map updates.  Temporary
 * device memory is grow-only and the context's: below 12 bytes per pixel of the widened box (the raster's buffer) plus 40 bytes per
 * reported cluster. */
typedef struct lama_hip_frontier {          /* 40 bytes */
    uint32_t label;                         /* smallest pixel index j * width + i of the cluster: itself a frontier pixel (free) */
    uint32_t pixels;                        /* number of frontier pixels in the cluster */
    uint32_t min_i, min_j, max_i, max_j;    /* bounding box in pixels of the box */
    uint64_t sum_i, sum_j;                  /* sums of the pixel indices: centroid = sum / pixels */
} lama_hip_frontier;
int32_t lama_hip_map_frontiers(lama_hip_ctx* ctx, uint32_t particle, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
                               uint32_t stride, uint32_t min_pixels, uint32_t cap, lama_hip_frontier* out, uint32_t* n,
                               uint64_t* frontier_pixels, uint32_t* labels_out, double* kernel_ms);

/* ROUTES through `particle`'s device maps inside a box: can the robot get from where it is to each of a list of goals, how far is it,
 * and along which pixels (csrc/lama_travel.h) -- a travel-cost field from the source pixels over the traversable pixels, the best pixel
 * near every goal, and the path to it.  Only the routes come down, not the grids.  The definition is exact, in integers, and
 * independent of how the device schedules the work:
 *   pixels       those of lama_hip_map_rasterize for the same x0, y0, width, height and stride (the same rules for them); pixel (i, j)
 *                has the index j * width + i.  occ = the TRINARY layer, sq = the SQDIST layer (the smallest squared distance of the
 *                block; max_sqdist where the cell is absent).  A context whose occupancy map has no patch while its distance map has
 *                some (lama::Loc2D's) has no occ layer;
 *   traversable  occ == 0 (free) and sq >= clearance_cells^2; without an occ layer the sq condition alone (that map knows no
 *                "unknown").  Pixels outside the box do not exist: there is no halo;
 *   entering     m(q) = near_factor where sq(q) < prefer_cells^2, else 1.  A step from p to an EDGE neighbour q costs 5 * m(q), to a
 *                DIAGONAL neighbour 7 * m(q);
 *   moves        a step may only enter a traversable pixel; a diagonal step needs in addition BOTH pixels that share an edge with p
 *                and q to be traversable (no corner is cut), so reachability is 4-connected while paths are 8-connected;
 *   sources      sources_xy [num_sources][2] in map CELL coordinates; every source pixel has cost 0 whatever its class (the robot is
 *                where it is) and may be left by any legal move; a non-traversable source blocks diagonals like any such pixel;
 *   field        F[q] = the least total cost of a move sequence from any source to q, 0xFFFFFFFF where there is none.  F is unique;
 *   goal         goals_xy [num_goals][2] in map cell coordinates.  Among the goal's pixel and every pixel within Chebyshev distance
 *                goal_reach of it, clipped to the box, the answer is the one with the smallest F, ties to the smallest index:
 *                routes[g] = {status, pixel, cost = F[pixel], steps}.  LAMA_HIP_ROUTE_REACHED; LAMA_HIP_ROUTE_UNREACHED when none of
 *                them has a finite F, LAMA_HIP_ROUTE_OUTSIDE when the goal's cell is not in the box (pixel = cost = 0xFFFFFFFF,
 *                steps = 0 in both);
 *   path         from the answer pixel p, until F[p] == 0: of p's 8 neighbours n in ascending pixel index the first with F[n]
 *                finite, the move n -> p legal and F[n] + (5 or 7) * m(p) == F[p] is the next p.  steps = the number of moves, in
 *                full.  paths[g][0 .. min(path_cap, steps + 1)) = the pixels counted FROM THE SOURCE END (the source first): the
 *                moves to drive next are what a caller needs when the cap cuts the list.  Entries past that and the rows of goals
 *                not reached are left alone.
 * field_out (may be NULL) [height][width] = F.  rounds (may be NULL) = the relaxation rounds that ran a tile; a diagnostic that may
 * differ from run to run.  kernel_ms (may be NULL) = the device time between the first and the last launch of the call, from events
 * (the host's batched read-backs of the rounds' tile counts lie inside it).
 * LAMA_HIP_E_INVALID, found before anything is written: the stride and origin rules of lama_hip_map_rasterize; width or height 0 or
 * above 32768; width * height * 7 * near_factor >= 2^32 (a shortest path enters a pixel at most once, so below this no cost wraps);
 * a particle out of range; num_sources == 0; sources_xy, goals_xy, routes or paths NULL where their count is not 0; a source outside
 * the box; clearance_cells^2 > max_sqdist; prefer_cells < clearance_cells or above 65535; near_factor outside 1 .. 64; goal_reach
 * above 16; num_goals * path_cap above 2^28.
 * Neither map has a patch: no pixel is traversable, so the field is 0 at the sources and 0xFFFFFFFF elsewhere, a goal is REACHED only
 * where its window holds a source, and nothing is rasterised or relaxed.
 * No map, pose or counter of the context changes; like every entry point the call first waits for queued map updates.  Temporary
 * device memory is grow-only and the context's: 8 bytes per pixel (the two rasters 3, the class 1, the field 4), 12 bytes per tile
 * of 32 x 32 pixels, 8 bytes per source and per goal, 16 per goal and 8 per goal and path entry. */
#define LAMA_HIP_ROUTE_REACHED   0u
#define LAMA_HIP_ROUTE_UNREACHED 1u
#define LAMA_HIP_ROUTE_OUTSIDE   2u
#define LAMA_HIP_ROUTE_NONE 0xFFFFFFFFu     /* F of an unreached pixel; pixel and cost of a route that is not REACHED */
typedef struct lama_hip_route {             /* 16 bytes */
    uint32_t status;                        /* LAMA_HIP_ROUTE_* */
    uint32_t pixel;                         /* the answer pixel j * width + i */
    uint32_t cost;                          /* F[pixel]: 5 per edge step, 7 per diagonal step, near_factor times that close to obstacles */
    uint32_t steps;                         /* moves from the source to the answer pixel; the path has steps + 1 pixels */
} lama_hip_route;
int32_t lama_hip_map_travel(lama_hip_ctx* ctx, uint32_t particle, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, uint32_t stride,
                            uint32_t clearance_cells, uint32_t prefer_cells, uint32_t near_factor, uint32_t num_sources, const uint32_t* sources_xy,
                            uint32_t num_goals, const uint32_t* goals_xy, uint32_t goal_reach, lama_hip_route* routes, uint32_t path_cap,
                            uint32_t* paths, uint32_t* field_out, uint32_t* rounds, double* kernel_ms);
/* Diagnostics of the context's last lama_hip_map_travel (each may be NULL): the rounds, the tiles run over all rounds, the most tiles
 * any round ran, and the blocking read-backs of the host loop. */
int32_t lama_hip_map_travel_stats(lama_hip_ctx* ctx, uint32_t* rounds, uint64_t* tiles_run, uint32_t* max_tiles, uint32_t* readbacks);

/* What a sensor at each of num_poses poses WOULD see in `particle`'s device map of `kind` (LAMA_HIP_MAP_*): per (pose, beam) the first
 * cell that stops the ray (csrc/lama_raycast_query.h), one lane each -- the expected ranges of a beam model, a scan check (which beams
 * of a real scan agree with the map, which pass through a mapped obstacle, which end in mapped free space), visibility gating of many
 * candidate poses at once.  Inputs as for lama_hip_map_integrate_scans: poses4 [num_poses][4] {c, s, tx, ty}; pts_xyz [n][3], the
 * SAME n points for every pose (a fan of max_range, or a real scan); one sensor mount (NULL: zero / identity).
 * A beam's cells are the map update's: tf = T(pose) * T(sensor origin) * R(sensor orientation) composed on the host, start cell
 * w2m(tf.translation()), hit cell w2m(tf * p) (PFSlam2D::updateParticleMaps, src/pf_slam2d.cpp:458-493, with no truncated_ray /
 * truncated_range, as in the map rebuild: the question is about the whole beam), then the SEQUENCE Map::computeRay(start, hit) in
 * order followed by the hit cell: nn entries, nn = the largest cell delta over the three axes, none when start == hit.  The start
 * cell is never tested.  The ray stops at the first entry that is
 *   occupancy map, frequency cells (cfg.occupancy_policy 0): visited != 0 and 4 * occupied > visited;  log-odds cells (policy 1): mask
 *     bit on and l > 0;  with LAMA_HIP_RAY_STOP_UNKNOWN in `flags` also at an unknown cell: visited == 0, 4 * occupied == visited,
 *     mask bit off or l == 0, a cell in an absent patch, a cell outside the map window;
 *   distance map: the cell is present, valid_obstacle is set and the stored squared distance is 0 -- an obstacle cell (the only device
 *     map of lama::Loc2D).  LAMA_HIP_RAY_STOP_UNKNOWN has no meaning there and is refused.
 * The same exact integer rules as lama_hip_map_rasterize.  Outputs, [num_poses][n] each, every one but `status` may be NULL:
 *   status uint8       LAMA_HIP_RAY_NONE / _OCCUPIED / _UNKNOWN;
 *   step int32         0-based index into the sequence, -1 for NONE;             nn uint32: the beam's step count;
 *   cell_xy uint32[2]  the stopping cell; the hit cell where nothing stopped the ray;
 *   end_sqdist uint32  the distance map's squared distance in cells at the HIT cell, the context's max_sqdist where that cell is
 *                      absent or has no valid obstacle (always, on a context without a distance map);
 *   label uint8        written when tolerance_cells >= 0: LAMA_HIP_RAY_BLOCKED where status is OCCUPIED and nn - 1 - step >
 *                      tolerance_cells (the map has an obstacle in front of the measured end point); else LAMA_HIP_RAY_AGREES where
 *                      end_sqdist <= tolerance_cells^2; else LAMA_HIP_RAY_NOVEL (the beam ends where the map has nothing).
 * No range is formed in floating point on the device: start_xy [num_poses][2] (may be NULL) is the start cell of each pose's beams, and
 * a caller takes resolution * sqrt(dx * dx + dy * dy) of the stopping cell's integer offset from it.  kernel_ms (may be NULL): device
 * time of the launch.  No map, pose or counter of the context changes; like every entry point the call first waits for queued
 * map updates.  LAMA_HIP_E_INVALID, found before anything is uploaded and with every output untouched: n == 0 or num_poses == 0, a
 * NULL status, a non-finite point, pose or mount, a particle out of range, an unknown kind or flag, LAMA_HIP_RAY_STOP_UNKNOWN on the
 * distance map, num_poses * n >= 2^31, a start or hit cell outside the 32-bit range of map cell coordinates.  LAMA_HIP_E_WINDOW, in
 * the same way: a beam of more than 8191 steps (the map update's own limit).  Scans of any n are accepted. */
#define LAMA_HIP_RAY_STOP_UNKNOWN 1u
#define LAMA_HIP_RAY_NONE     0
#define LAMA_HIP_RAY_OCCUPIED 1
#define LAMA_HIP_RAY_UNKNOWN  2
#define LAMA_HIP_RAY_AGREES   0
#define LAMA_HIP_RAY_BLOCKED  1
#define LAMA_HIP_RAY_NOVEL    2
int32_t lama_hip_map_cast_rays(lama_hip_ctx* ctx, uint32_t particle, int32_t kind, uint32_t num_poses, const double* poses4,
                               const double* pts_xyz, uint32_t n, const double* sensor_origin3, const double* sensor_quat_wxyz,
                               uint32_t flags, int32_t tolerance_cells, uint8_t* status, int32_t* step, uint32_t* nn,
                               uint32_t* cell_xy, uint32_t* end_sqdist, uint8_t* label, uint32_t* start_xy, double* kernel_ms);

/* Particle shipping for multi-GPU resampling (one context per GPU): serialise one particle (pose + both
 * maps, used patches only) into a DEVICE buffer / restore it into slot `particle` of this context.
 * export returns the number of bytes needed in *bytes when buf == NULL. */
int32_t lama_hip_pf_export_particle(lama_hip_ctx* ctx, uint32_t particle, void* device_buf, uint64_t cap, uint64_t* bytes);
int32_t lama_hip_pf_import_particle(lama_hip_ctx* ctx, uint32_t particle, const void* device_buf, uint64_t bytes);
/* The same for ALL outgoing / incoming particles of a resample at once: one kernel launch and one synchronisation per batch instead
 * of a dozen copies per particle (a 3000-particle filter on 8 GPUs ships hundreds of particles per resample).  export: device_bufs ==
 * NULL only reports the sizes in bytes_out[n]; import: a slot may appear once per batch. */
int32_t lama_hip_pf_export_particles(lama_hip_ctx* ctx, uint32_t n, const uint32_t* particles, void* const* device_bufs, const uint64_t* caps,
                                     uint64_t* bytes_out);
int32_t lama_hip_pf_import_particles(lama_hip_ctx* ctx, uint32_t n, const uint32_t* particles, const void* const* device_bufs, const uint64_t* bytes);

/* (Peer access: the first lama_hip_blob_copy between two devices queries hipDeviceCanAccessPeer and enables access in both
 * directions, once per pair and process; when the platform refuses it the copy still works -- the runtime stages it through host
 * memory -- and lama_hip_counters::peer_access says 0.)
 * Device staging buffers for particle shipping when ONE process drives several contexts (lama::PFSlam2D with Options::gpus > 1: a
 * host thread per GPU, src/pf_slam2d.cpp:254-302's two parallel regions become G device streams): allocate / free a buffer on the
 * context's device, and copy between buffers of two contexts -- hipMemcpyPeerAsync when they live on different GPUs (xGMI), a
 * plain device copy otherwise.  The copy is complete when the call returns. */
int32_t lama_hip_blob_alloc(lama_hip_ctx* ctx, uint64_t bytes, void** device_buf);
int32_t lama_hip_blob_free(lama_hip_ctx* ctx, void* device_buf);
int32_t lama_hip_blob_copy(lama_hip_ctx* dst_ctx, void* dst_device_buf, lama_hip_ctx* src_ctx, const void* src_device_buf, uint64_t bytes);

/* SE2 pose-graph linearisation: the per-factor body and the accumulation of minisam's
 * linearzationLowerHessian (vendor/minisam/minisam/nonlinear/linearization.cpp:150-272,290-341) for PriorFactor<SE2d> /
 * BetweenFactor<SE2d> with DiagonalLoss, as built by SimplePGO::optimize (src/simple_pgo.cpp:48-105) and -- with the robust
 * losses of lama_hip_pgo_create_robust below -- GraphSlam2D::optimizePoseGraph (src/graph_slam2d.cpp:394-430).  The graph structure and measurements are uploaded once
 * (create), every Levenberg-Marquardt iteration calls linearize with the current poses {c, s, tx, ty}.  Outputs, dense 3x3
 * blocks row-major (the caller scatters them into its sparse lower Hessian and runs the Cholesky on the host):
 *   err   [F][3]  whitened error           Hoff [F][9]  J_i^T J_j of factor f (zero for a prior, fj = -1)
 *   Hdiag [N][9]  sum of J_v^T J_v over the factors of v, in factor order     b [N][3]  Atb = -sum J_v^T err
 * Any output may be NULL.  kernel_ms: device time of the two kernels (hipEvents on the graph's stream). */
typedef struct lama_hip_pgo lama_hip_pgo;
int32_t lama_hip_pgo_create(int32_t device, uint32_t num_poses, const int32_t* fi, const int32_t* fj, const double* meas4,
                            const double* sqrt_info3, uint32_t num_factors, lama_hip_pgo** out);
void lama_hip_pgo_destroy(lama_hip_pgo* g);
const char* lama_hip_pgo_last_error(const lama_hip_pgo* g);
int32_t lama_hip_pgo_linearize(lama_hip_pgo* g, const double* poses4, double* err, double* Hdiag, double* Hoff, double* b,
                               double* chi2, double* kernel_ms);

/* The device-resident Levenberg-Marquardt loop of lama::SimplePGO (include/lama/simple_pgo.h).  The graph holds two pose buffers on the
 * device, the current state and a candidate; lama_hip_pgo_linearize above also sets the current state.
 *   pattern          : the lower block-CSR pattern of the Hessian, fixed at create: row r holds its diagonal block first, then the
 *                      distinct columns c < r that share a factor with r, ascending.  row_ptr [N+1], cols [nnzb]; either may be NULL
 *                      (ask for nnzb first).
 *   set_poses / get_poses : the current state {c, s, tx, ty} [N][4].
 *   linearize_system : at the current state: blocks [nnzb][9] (row-major 3x3, the order of `cols`; the factors on one pair add up in
 *                      factor order), b [N][3] = -J^T e, diag [N][3] = the undamped Hessian diagonal, half_chi2 = 0.5 sum ||e||^2.
 *                      Outputs may be NULL.  (Bit for bit: blocks are the scatter of lama_hip_pgo_linearize's Hdiag / Hoff.)
 *   try_step         : candidate = current * exp(dx) per pose (dx [N][3], the right-multiplicative retract of minisam's Sophus
 *                      traits) and its 0.5 sum ||e||^2; only dx goes up and one scalar comes back.
 *   accept           : the candidate becomes the current state (no copy).  A candidate is pending from a successful try_step until
 *                      the next accept, set_poses or lama_hip_pgo_linearize; with none pending accept returns LAMA_HIP_E_STATE
 *                      (lama_hip_pgo_last_error says so) and leaves the current state as it is.
 * kernel_ms: device time of the call's kernels (may be NULL). */
int32_t lama_hip_pgo_pattern(const lama_hip_pgo* g, int32_t* row_ptr, int32_t* cols, uint32_t* nnzb);
int32_t lama_hip_pgo_set_poses(lama_hip_pgo* g, const double* poses4);
int32_t lama_hip_pgo_get_poses(lama_hip_pgo* g, double* poses4);
int32_t lama_hip_pgo_linearize_system(lama_hip_pgo* g, double* blocks, double* b, double* diag, double* half_chi2, double* kernel_ms);
int32_t lama_hip_pgo_try_step(lama_hip_pgo* g, const double* dx, double* half_chi2, double* kernel_ms);
int32_t lama_hip_pgo_accept(lama_hip_pgo* g);

/* The damped system of one Levenberg-Marquardt try, (H + lambda diag(H)) dx = b, solved on the device by a conjugate gradient
 * preconditioned with the inverse of the damped 3x3 diagonal blocks (iris_lama_amd/csrc/lama_pgo_pcg.h): no factorisation, no fill.
 * Opt-in (lama::SimplePGO::linear_solver); the calls above are unchanged.
 *   solve_pcg       : needs a lama_hip_pgo_linearize_system since the last set_poses / accept / lama_hip_pgo_linearize, otherwise
 *                     LAMA_HIP_E_STATE (lama_hip_pgo_last_error says so).  Stops when r.r <= rel_tol^2 b.b (outcome CONVERGED; b = 0
 *                     gives dx = 0 after 0 iterations), after max_iterations (CAP), or when a damped diagonal block is not positive
 *                     definite or p.(H + lambda D)p is not a positive finite number (BREAKDOWN; nothing non-finite is stored).  The
 *                     solution stays on the device; dx [N][3] may be NULL.  rel_residual_sq = r.r / b.b of the recurrence;
 *                     model_decrease = 0.5 sum dx (lambda diag dx + b), the denominator of minisam's gain ratio.  The iterations are
 *                     enqueued `batch` at a time (0: LAMA_HIP_PCG_DEFAULT_BATCH) and the device's stop word is read once per batch;
 *                     the result does not depend on the batch.  LAMA_HIP_E_INVALID with nothing touched: lambda negative or not
 *                     finite, rel_tol outside (0, 1), max_iterations == 0.  The system (blocks, b, diag) is only read.
 *   try_solved_step : lama_hip_pgo_try_step with the solution the device holds (after CONVERGED or CAP); LAMA_HIP_E_STATE when there
 *                     is none or the state or the system changed since the solve.  accept works after it as after try_step. */
#define LAMA_HIP_PCG_CONVERGED 0
#define LAMA_HIP_PCG_CAP 1
#define LAMA_HIP_PCG_BREAKDOWN 2
#define LAMA_HIP_PCG_DEFAULT_BATCH 32
int32_t lama_hip_pgo_solve_pcg(lama_hip_pgo* g, double lambda, double rel_tol, uint32_t max_iterations, uint32_t batch, double* dx,
                               uint32_t* iterations, double* rel_residual_sq, int32_t* outcome, double* model_decrease, double* kernel_ms);
int32_t lama_hip_pgo_try_solved_step(lama_hip_pgo* g, double* half_chi2, double* kernel_ms);

/* Per-factor robust losses, applied AFTER the diagonal whitening: minisam's ComposedLoss(DiagonalLoss, robust), and with
 * sqrt_info = 1 the bare HuberLoss GraphSlam2D::optimizePoseGraph puts on its loop closures (src/graph_slam2d.cpp:266).  With e the
 * whitened error and n = sqrt((e0 e0 + e1 e1) + e2 e2) (vendor/minisam/minisam/core/LossFunction.h:173,200-202,230-238):
 *   HUBER  (param k): w = n < k ? 1 : k / |n|        CAUCHY (param k): w = k^2 / (k^2 + n^2)
 *   DCS    (param c): w = n^2 > c ? (2 c / (c + n^2))^2 : 1
 * The error and both whitened Jacobians are multiplied by sqrt(w) before any product is formed, so err, chi2 / half_chi2, Hdiag,
 * Hoff, b and the assembled system of every call above are those of the robustly weighted error (Factor::weightedError), and
 * try_step / try_solved_step return the error under the same weight.
 *   create_robust  : lama_hip_pgo_create with loss_kind [F] (LAMA_HIP_PGO_LOSS_*) and loss_param [F]; loss_param is not read for a
 *                    factor of kind NONE, and may be NULL when every kind is NONE.  loss_kind NULL is lama_hip_pgo_create.  A graph
 *                    without a robust factor runs exactly the kernels lama_hip_pgo_create's runs.  LAMA_HIP_E_INVALID with nothing
 *                    created: an unknown kind, or a robust factor whose parameter is not finite and > 0 --
 *                    lama_hip_pgo_last_error(NULL) then names the factor (per thread, until the next create_robust).
 *   factor_weights : w [F] (w, not its root) of every factor in the last linearize / linearize_system, 1 for a loss-free factor;
 *                    LAMA_HIP_E_STATE before the first linearisation. */
#define LAMA_HIP_PGO_LOSS_NONE 0
#define LAMA_HIP_PGO_LOSS_HUBER 1
#define LAMA_HIP_PGO_LOSS_CAUCHY 2
#define LAMA_HIP_PGO_LOSS_DCS 3
int32_t lama_hip_pgo_create_robust(int32_t device, uint32_t num_poses, const int32_t* fi, const int32_t* fj, const double* meas4,
                                   const double* sqrt_info3, const int32_t* loss_kind, const double* loss_param, uint32_t num_factors,
                                   lama_hip_pgo** out);
int32_t lama_hip_pgo_factor_weights(lama_hip_pgo* g, double* w);

/* Accumulated per-kernel device time (hipEvent elapsed, on the stream the kernels run on) and work
 * counters since the last reset; valid when cfg.profile != 0. */
typedef struct lama_hip_counters {
    double ms_scan_match;  uint64_t launches_scan_match;
    double ms_update_maps; uint64_t launches_update_maps;   /* = raycast + brushfire */
    double ms_raycast;     uint64_t launches_raycast;
    double ms_brushfire;   uint64_t launches_brushfire;
    double ms_resample;    uint64_t launches_resample;
    uint64_t gn_iterations;     /* sum over particles and calls                                    */
    uint64_t gn_evals;          /* residual evaluations (with or without Jacobian) + likelihood     */
    uint64_t ray_cells;         /* Bresenham cells visited                                          */
    uint64_t bf_cells;          /* brushfire cells processed (DynamicDistanceMap::update return)     */
    uint64_t dm_patches;        /* sum of allocated DM patches over particles (current)             */
    uint64_t occ_patches;       /* sum of allocated occupancy patches over particles (current)      */
    double ms_eval_batch;  uint64_t launches_eval_batch;     /* lama_hip_eval_batch                   */
    uint64_t arena_growths;     /* batches of particles moved to larger regions (maps grow on demand)  */
    uint64_t window_shifts;     /* times the map window was re-centred (the window follows the robot)  */
    uint64_t wrap_guard_scans;  /* scans ray-cast beam by beam because a uint16 `visited` counter could wrap inside them */
    /* what actually ran (set by every map update; not cleared by lama_hip_reset_counters' zeroing of the sums above): */
    uint32_t brushfire_mode;    /* cfg.brushfire_mode of the last map update: 0 = exact, 1 = canonical tie rule (not bit-identical) */
    uint32_t brushfire_waves;   /* exact brushfire of the last map update: 2 = wave pair per particle, 1 = one wave per particle */
    uint64_t sequential_raycast_scans;  /* map updates whose ray-cast ran beam by beam (k_raycast)                           */
    uint64_t parallel_raycast_scans;    /* map updates whose ray-cast ran in the parallel, patch-centric form                */
    uint32_t brushfire_handovers;       /* particle updates whose brushfire queue outgrew the first stage's LDS window (lower queue: 1020 entries at entry,
                                           1276 in the lower phase, wave pair and one wave alike; raise queue: 252) and
                                           were finished by the resume stage (sum since the last reset).  Such an update is one long
                                           serial chain: at 3000 particles one of them (13.9 ms) is what made the resume kernel's MEAN
                                           1.2 ms in the round-3 profile while its median is 5 us (profiles/r04_timeline_3000_before.txt) */
    uint32_t replay_handovers;          /* the same for the ordered replay of the parallel ray-cast (more than 2048 order-sensitive visits) */
    uint32_t window_patches;            /* current side of the map window in patches (it grows with the mapped area, up to 1016)            */
    uint32_t window_growths;            /* times the window directories were re-allocated with a larger side                                */
    uint64_t bf_longest_chain_sum;      /* sum over map updates of the LARGEST brushfire cell count of a single particle: a particle's exact
                                           brushfire is one serial chain, so a map update lasts as long as its longest chain --
                                           bf_longest_chain_sum / map updates against bf_cells / (particles x map updates) is the spread   */
    uint64_t bf_longest_chain_last;     /* the largest per-particle count of the last map update                                           */
    uint64_t brushfire_early;           /* ... of which: particles the PREVIOUS update had routed and that therefore ran their ray-cast and their
                                           brushfire in the early lane, ahead of everybody else's ray-cast (counted in brushfire_routed too)   */
    uint64_t brushfire_routed;          /* particle updates whose brushfire ran in the big-queue stage from the start, beside the first stage:
                                           their obstacle-event count (known before the brushfire starts) marked them as the long chains   */
    /* round 5: memory that follows the maps (one particle set, in-place resampling, per-particle regions in pooled planes) */
    uint64_t pool_growths;              /* times a patch pool was re-allocated larger (geometric)                                          */
    uint64_t resample_clones;           /* particles a resample / the first scan really COPIED: a particle that survives keeps its home and
                                           regions, only the second and further copies of a multiply drawn particle are written           */
    uint64_t resample_bytes;            /* bytes those copies read (= wrote): directories + used slots of every plane                       */
    uint64_t hbm_bytes_allocated;       /* device memory the context holds for the maps now: patch pools + directories                     */
    uint64_t hbm_bytes_used;            /* ... of which used: the allocated patches of all particles (all planes) + directories            */
    uint64_t hbm_bytes_total;           /* everything the context has allocated on the device (maps, queues, scratch)                      */
    uint32_t peer_access;               /* lama_hip_blob_copy between two devices: 1 = the last such copy went GPU to GPU directly (peer access
                                           enabled both ways), 0 = it was staged by the runtime (peer access refused) or none was made      */
    uint32_t struct_bytes;              /* sizeof(lama_hip_counters) of the library that filled the struct (see lama_hip_get_counters_sized) */
    double peer_copy_ms;                /* device time (hipEvents on the destination's stream) of the cross-device lama_hip_blob_copy calls ... */
    uint64_t peer_copy_bytes;           /* ... and the bytes they moved INTO this context: bytes / ms = the achieved xGMI rate               */
} lama_hip_counters;      /* (the group count of the grouped step schedule: lama_hip_pf_step_groups, not a member here) */
int32_t lama_hip_get_counters(lama_hip_ctx* ctx, lama_hip_counters* out);
/* The same for a caller compiled against another version of this header: at most `bytes` bytes are written (the struct
 * grows at its END only, a consumer built against an older header passes its own sizeof and is never written past). */
int32_t lama_hip_get_counters_sized(lama_hip_ctx* ctx, void* out, uint32_t bytes);
uint32_t lama_hip_counters_bytes(void);     /* sizeof(lama_hip_counters) in the library (a binding checks its own mirror against it) */
int32_t lama_hip_reset_counters(lama_hip_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* LAMA_HIP_H */
