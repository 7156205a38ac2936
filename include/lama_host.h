/* =====================================================================================
 * lama_host.h -- C surface of liblama_host.so: the host-side mirror of the reference interface
 * (lama::PFSlam2D of include/lama/pf_slam2d.h) flattened for FFI users (Python ctypes in this repo:
 * tests, bench.py, iris_lama_amd/distributed.py), plus the synthetic workload generator.
 *
 * C++ consumers (iris_lama_ros) use the classes in include/lama/ directly; this header exists because the
 * measuring/test harness is Python.  All functions catch C++ exceptions; a negative return is an error and
 * lama_pf_last_error() holds the message.
 * ===================================================================================== */
#ifndef LAMA_HOST_H
#define LAMA_HOST_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Seeded synthetic corridor log.  pts: (steps+1) x beams x 3 doubles (sensor frame),
 * odom_xyr / truth_xyr: (steps+1) x 3 doubles (x, y, yaw).  truth_xyr may be NULL.  Returns 0. */
int lama_corridor_generate(int steps, int beams, double* pts, double* odom_xyr, double* truth_xyr);

/* PFSlam2D::Options (include/lama/pf_slam2d.h) as a POD. */
typedef struct lama_pf_options {
    uint32_t particles;
    double srr, str, stt, srt;
    double meas_sigma, meas_sigma_gain;
    double trans_thresh, rot_thresh;
    double l2_max, truncated_ray, truncated_range, resolution;
    uint32_t patch_size, max_iter;
    uint32_t seed;
    int32_t create_summary;
    int32_t gpu_device;
    uint32_t shard_rank, shard_world;
    int32_t profile;
    uint32_t brushfire_mode;
    uint32_t window_patches, dm_patch_capacity, occ_patch_capacity, queue_capacity;   /* device map storage, 0 = defaults */
    int32_t gpus;                 /* PFSlam2D::Options::gpus: > 1 = one object drives that many shards / devices from C++ (0 / 1: one) */
} lama_pf_options;

typedef struct lama_pf lama_pf;

void lama_pf_default_options(lama_pf_options* o);

#ifdef LAMA_TESTING
/* ONLY in a host library compiled with -DLAMA_TESTING (the test-suite builds its own copy, tests/cpu_engine/Makefile); the
 * shipped liblama_host.so neither declares nor exports it (tests/test_cabi.py asserts that) and always binds liblama_hip.so
 * next to itself.  Device library used by the objects created afterwards (NULL = liblama_hip.so): the test-suite points it at
 * an oracle-backed test double to exercise the host / multi-rank logic on machines without a GPU. */
int lama_host_set_engine_library(const char* path);
#endif
/* Path of the device library bound to `pf` (so callers can assert that the HIP library is the one in use). */
const char* lama_pf_engine_origin(const lama_pf* pf);

/* err (optional, errcap bytes) receives the failure message when NULL is returned. */
lama_pf* lama_pf_create(const lama_pf_options* o, char* err, int errcap);
void lama_pf_destroy(lama_pf* pf);
const char* lama_pf_last_error(const lama_pf* pf);

void lama_pf_set_prior(lama_pf* pf, double x, double y, double yaw);

/* PFSlam2D::update: 1 = update done, 0 = motion gate closed, <0 = error. */
int lama_pf_update(lama_pf* pf, const double* pts_xyz, uint32_t n, const double* origin3, const double* quat_wxyz,
                   const double* odom_xyr, double timestamp);

/* step-wise API (sharded operation), see include/lama/pf_slam2d.h */
int lama_pf_update_begin(lama_pf* pf, const double* pts_xyz, uint32_t n, const double* origin3, const double* quat_wxyz,
                         const double* odom_xyr, double timestamp);   /* 0 no update, 1 first scan, 2 matched */
int lama_pf_local_range(const lama_pf* pf, uint32_t* lo, uint32_t* hi);
int lama_pf_local_loglik(const lama_pf* pf, double* out /* hi-lo */);
int lama_pf_plan_resample(lama_pf* pf, const double* all_loglik /* P */, int32_t* sample_idx_out /* P */); /* 1 = resample */
int lama_pf_apply_resample(lama_pf* pf, const int32_t* sample_idx /* P */);
int lama_pf_update_maps(lama_pf* pf);
void* lama_pf_device_context(const lama_pf* pf);   /* lama_hip_ctx* of the local shard */

/* state queries; poses are {c,s,tx,ty} for all P particles (valid for locally owned ones) */
int lama_pf_get_poses(const lama_pf* pf, double* poses_P4);
int lama_pf_set_pose(lama_pf* pf, uint32_t i, const double* pose4);
int lama_pf_get_weights(const lama_pf* pf, double* weight, double* normalized_weight, double* weight_sum);
int lama_pf_set_weights(lama_pf* pf, const double* weight, const double* weight_sum);
double lama_pf_neff(const lama_pf* pf);
int lama_pf_best(const lama_pf* pf);
int lama_pf_best_pose_xyr(const lama_pf* pf, double* xyr);
uint32_t lama_pf_num_resamples(const lama_pf* pf);
/* Options::gpus > 1: seconds the last update spent gathering log-likelihoods / shipping (export + peer copy) / importing particles,
 * particles and bytes shipped between shards by it.  out8 = {gather_s, ship_s, import_s, particles, bytes, local_copies_s (resample copies
 * inside a shard), phase_begin_s (motion + scan match on all shards), phase_maps_s (map-update launch + state mirror)}.  Returns the number of shards. */
int lama_pf_exchange_times(const lama_pf* pf, double* out8);
/* lama_hip_ctx* of shard r of a gpus > 1 object (NULL when out of range) */
void* lama_pf_shard_context(const lama_pf* pf, uint32_t r);
uint64_t lama_pf_memory_usage(const lama_pf* pf);
/* Summary::report() into buf; returns the length needed */
int lama_pf_summary(const lama_pf* pf, char* buf, int cap);
/* Summary buckets of the last `update` (seconds): total, solving, normalizing, resampling, mapping */
int lama_pf_last_times(const lama_pf* pf, double* out5);

/* host-logic hooks (RNG replay tests): same formulas as src/pf_slam2d.cpp:365-391, 511-556 */
int lama_pf_draw_from_motion(lama_pf* pf, const double* delta4, double* pose4_inout);
double lama_pf_normalize(lama_pf* pf);
int lama_pf_resample_indices(const lama_pf* pf, double u01, int32_t* out_P);
/* pose algebra: out = a^-1 * b (Pose2D::operator-), {c,s,tx,ty} */
void lama_pose_minus(const double* a4, const double* b4, double* out4);
void lama_pose_from_xyr(double x, double y, double yaw, double* out4);

/* ---- lama::Slam2D (include/lama/slam2d.h), flattened ---- */
typedef struct lama_slam lama_slam;
typedef struct lama_slam_options {
    double trans_thresh, rot_thresh, l2_max, truncated_ray, truncated_range, resolution;
    uint32_t patch_size, max_iter;
    int32_t gpu_device;
    int32_t transient_map;      /* Slam2D::Options::transient_map (src/slam2d.cpp:322-379) */
    int32_t lm;                 /* Slam2D::Options::strategy == "lm" (Levenberg-Marquardt instead of Gauss-Newton) */
} lama_slam_options;
void lama_slam_default_options(lama_slam_options* o);
lama_slam* lama_slam_create(const lama_slam_options* o, char* err, int errcap);
void lama_slam_destroy(lama_slam* s);
const char* lama_slam_last_error(const lama_slam* s);
void lama_slam_set_pose(lama_slam* s, double x, double y, double yaw);
int lama_slam_get_pose(const lama_slam* s, double* pose4);
/* Slam2D::update: 1 = update done, 0 = not enough motion, <0 = error */
int lama_slam_update(lama_slam* s, const double* pts_xyz, uint32_t n, const double* origin3, const double* quat_wxyz,
                     const double* odom_xyr, double timestamp);
int lama_slam_enough_motion(lama_slam* s, const double* odom_xyr);
uint32_t lama_slam_processed_cells(const lama_slam* s);
uint32_t lama_slam_iterations(const lama_slam* s);
uint32_t lama_slam_deleted_patches(const lama_slam* s);
void* lama_slam_device_context(const lama_slam* s);
/* Queries on the snapshots returned by Slam2D::getOccupancyMap() / getDistanceMap() (include/lama/sdm_maps.h: the const
 * query API of the reference's map classes).  which: 0 = occupancy, 1 = distance.  All return < 0 when no map is available. */
int lama_slam_view_bounds(lama_slam* s, int which, uint32_t* min3, uint32_t* max3, double* wmin3, double* wmax3);
int64_t lama_slam_view_cells(lama_slam* s, int which, uint32_t* xy_out, uint64_t cap);      /* visit_all_cells; returns the count */
int lama_slam_view_occupancy(lama_slam* s, uint64_t n, const uint32_t* xy, uint8_t* is_free, uint8_t* is_occupied,
                             uint8_t* is_unknown, double* probability);
int lama_slam_view_distance_cells(lama_slam* s, uint64_t n, const uint32_t* xy, double* distance);
int lama_slam_view_distance_points(lama_slam* s, uint64_t n, const double* xy, double* dist_gx_gy);   /* n x 3 out */
/* lama::MatchSurface2D / lama::Solve (include/lama/match_surface_2d.h, include/lama/nlls/solver.h) on the distance map
 * Slam2D::getDistanceMap() returns -- the scan-matching problem a caller of the reference builds by hand:
 *   match_eval : MatchSurface2D::eval at pose4 {c,s,tx,ty}: residuals[n], jacobian n x 3 column-major (may be NULL), rmse_out =
 *                MatchSurface2D::error() (may be NULL);
 *   match_solve: Solve(options, problem, &cov): strategy "gn" | "lm", weight "cauchy" | "unit" | "tukey" | "huber" with its
 *                parameter; pose4 in/out, cov9 row-major (may be NULL).  Returns 0, or -3 when the configuration has no device
 *                kernel (message through lama_slam_last_error). */
int lama_slam_match_eval(lama_slam* s, const double* pts_xyz, uint32_t n, const double* origin3, const double* quat_wxyz,
                         const double* pose4, double* residuals, double* jacobian, double* rmse_out);
int lama_slam_match_solve(lama_slam* s, const double* pts_xyz, uint32_t n, const double* origin3, const double* quat_wxyz,
                          double* pose4, const char* strategy, const char* weight, double weight_param, uint32_t max_iterations,
                          double* cov9, uint32_t* iterations);
/* The same solve through lama::Solver's GENERIC host loop (a Problem that forwards to the MatchSurface2D: per-beam evaluation on the
 * device, weights / normal equations / steps on the host).  weight: "unit", "tukey", "tdist", "cauchy", "huber"; any parameter. */
int lama_slam_match_solve_generic(lama_slam* s, const double* pts_xyz, uint32_t n, const double* origin3, const double* quat_wxyz,
                                  double* pose4, const char* strategy, const char* weight, double weight_param, uint32_t max_iterations,
                                  double* cov9, uint32_t* iterations);
/* lama::SolveBatch (lama/nlls/solver.h) over num_problems MatchSurface2D on this object's distance map -- the odd-numbered ones on
 * `other`'s when that is not NULL --: points concatenated with num_problems + 1 offsets, origins [B][3] / quats [B][4] (NULL: zero /
 * identity), poses4 [B][4] in / out, max_iterations [B] (NULL: 100 each), eps1 > 0 replaces the strategy's first threshold, cov9
 * [B][9], iterations [B], errors [B] = MatchSurface2D::error() at the solution.  -3: SolveBatch threw std::invalid_argument. */
int lama_slam_solve_batch(lama_slam* s, lama_slam* other, uint32_t num_problems, const double* pts_xyz, const uint32_t* offsets,
                          const double* origins3, const double* quats_wxyz, double* poses4, const uint32_t* max_iterations,
                          const char* strategy, double eps1, const char* weight, double weight_param, double* cov9, uint32_t* iterations,
                          double* errors);
/* lama::CorrelativeSearch2D::search (lama/correlative_search_2d.h) on this object's distance map over the box box4 = {min x, min y, max
 * x, max y}; the options are the class's (point_step 0: max(n / 256, 1)).  *num_out = candidates found; the first min(cap, *num_out),
 * sorted by rmse, are written: coarse4 [cap][4] / poses4 [cap][4] {c, s, tx, ty}, scores, rmse, iterations.  lattice6 (may be NULL) =
 * cell_step, nx, ny, headings, point_step, tile of the lattice that was searched.  -1: no map yet, -3: std::invalid_argument, -2: any
 * other failure (the device library lacks the entry, ...). */
int lama_slam_correlative_search(lama_slam* s, const double* pts_xyz, uint32_t n, const double* origin3, const double* quat_wxyz, const double* box4,
                                 double linear_step, double angular_step, uint32_t point_step, uint32_t tile, uint32_t max_candidates, int refine,
                                 uint32_t refine_iterations, uint32_t cap, double* coarse4, uint32_t* scores, double* poses4, double* rmse,
                                 uint32_t* iterations, uint32_t* lattice6, uint32_t* num_out);
const char* lama_slam_engine_origin(const lama_slam* s);

/* ---- lama::Loc2D (include/lama/loc2d.h), flattened ---- */
typedef struct lama_loc lama_loc;
lama_loc* lama_loc_create(double trans_thresh, double rot_thresh, double l2_max, double resolution, uint32_t max_iter,
                          int32_t gpu_device, char* err, int errcap);
void lama_loc_destroy(lama_loc* l);
const char* lama_loc_last_error(const lama_loc* l);
const char* lama_loc_engine_origin(const lama_loc* l);
/* distance_map->addObstacle(w2m(x, y)) for every world point, then distance_map->update() */
int lama_loc_set_obstacles_world(lama_loc* l, const double* xy, uint32_t n);
/* distance_map->write(file) / distance_map->read(file): the reference's .sdm format (Map::write / Map::read, src/sdm/map.cpp:489-575).
 * read REPLACES the device map by the file's patches (lama_hip_pf_upload_map): a static map is loaded instead of rebuilt. */
int lama_loc_write_distance_map(lama_loc* l, const char* filename);
int lama_loc_read_distance_map(lama_loc* l, const char* filename);
void* lama_loc_device_context(const lama_loc* l);      /* the lama_hip_ctx behind the object (NULL before the first map / update) */
void lama_loc_set_pose(lama_loc* l, double x, double y, double yaw);
int lama_loc_get_pose(const lama_loc* l, double* pose4);
int lama_loc_update(lama_loc* l, const double* pts_xyz, uint32_t n, const double* origin3, const double* quat_wxyz,
                    const double* odom_xyr, double timestamp, int force_update);   /* 1 / 0 / <0 */
int lama_loc_covar(const lama_loc* l, double* out9);
double lama_loc_rmse(const lama_loc* l);
uint32_t lama_loc_iterations(const lama_loc* l);
/* global localisation / sampling covariance (src/loc2d.cpp:194-286) */
lama_loc* lama_loc_create2(double trans_thresh, double rot_thresh, double l2_max, double resolution, uint32_t max_iter,
                           uint32_t gloc_particles, uint32_t gloc_iters, double gloc_thresh, double cov_blend,
                           int32_t gpu_device, char* err, int errcap);
lama_loc* lama_loc_create3(double trans_thresh, double rot_thresh, double l2_max, double resolution, uint32_t max_iter,
                           uint32_t gloc_particles, uint32_t gloc_iters, double gloc_thresh, double cov_blend,
                           const char* strategy /* "gn" | "lm" */, int32_t gpu_device, char* err, int errcap);
/* occupancy_map->setFree / setUnknown / setOccupied on map cells (x, y pairs); state -1 / 0 / 1 */
int lama_loc_occ_set_cells(lama_loc* l, const uint32_t* cells_xy, uint32_t n, int state);
int lama_loc_occ_bounds(const lama_loc* l, double* out6);
void lama_loc_trigger_global_localization(lama_loc* l);
int lama_loc_global_localization_active(const lama_loc* l);
uint32_t lama_loc_gloc_candidates(const lama_loc* l, double* poses4, double* errors, uint32_t cap);
uint32_t lama_loc_sampling_likelihoods(const lama_loc* l, double* out, uint32_t cap);
/* Loc2D::relocalize with the given CorrelativeSearch2D options: 1 = a candidate's rmse was below gloc_thresh and the pose was set, 0 =
 * none was (nothing changed), -1 = failure.  lama_loc_relocalize_candidates: the candidates of the last call, best first (returns their
 * number; the first min(cap, number) are written, arrays as lama_slam_correlative_search's). */
int lama_loc_relocalize(lama_loc* l, const double* pts_xyz, uint32_t n, const double* origin3, const double* quat_wxyz, double linear_step,
                        double angular_step, uint32_t point_step, uint32_t tile, uint32_t max_candidates, uint32_t refine_iterations);
uint32_t lama_loc_relocalize_candidates(const lama_loc* l, uint32_t cap, double* coarse4, uint32_t* scores, double* poses4, double* rmse,
                                        uint32_t* iterations);
/* ---- lama::LidarOdometry2D (include/lama/lidar_odometry_2d.h), flattened ---- */
typedef struct lama_lo lama_lo;
lama_lo* lama_lo_create(double resolution, uint32_t max_iter, int32_t gpu_device, char* err, int errcap);
void lama_lo_destroy(lama_lo* l);
const char* lama_lo_last_error(const lama_lo* l);
const char* lama_lo_engine_origin(const lama_lo* l);
int lama_lo_update(lama_lo* l, const double* pts_xyz, uint32_t n, const double* origin3, const double* quat_wxyz, double timestamp);   /* 1 / <0 */
int lama_lo_get_odom(const lama_lo* l, double* pose4);
uint32_t lama_lo_iterations(const lama_lo* l);
uint32_t lama_lo_deleted_patches(const lama_lo* l);
void* lama_lo_device_context(const lama_lo* l);

/* ---- lama::sdm map formats (include/lama/sdm_io.h): the reference's `.sdm` file (Map::write/read, src/sdm/map.cpp:489-575)
 * and the export images of src/sdm/export.cpp:46-110 for maps downloaded from the device.
 * kind: 0 DynamicDistanceMap (10 B cells), 1 FrequencyOccupancyMap (4 B), 2 SimpleOccupancyMap (1 B). */
int lama_sdm_write(const char* file, int kind, double resolution, uint32_t max_sqdist, uint32_t n,
                   const uint64_t* ids, const uint8_t* cells, const uint64_t* masks);
int lama_sdm_read(const char* file, int* kind, double* resolution, uint32_t* max_sqdist, uint32_t cap,
                  uint64_t* ids, uint8_t* cells, uint64_t* masks, uint32_t* n);       /* cap = 0: query n */
int lama_sdm_image(int kind, double resolution, uint32_t max_sqdist, uint32_t n, const uint64_t* ids, const uint8_t* cells,
                   const uint64_t* masks, uint32_t* width, uint32_t* height, uint8_t* out, uint64_t cap);
int lama_sdm_export_png(int kind, double resolution, uint32_t max_sqdist, uint32_t n, const uint64_t* ids, const uint8_t* cells,
                        const uint64_t* masks, const char* file);
/* The FIRST build of lama::Loc2D's distance map on the host (iris_lama_amd/host/dm_builder.hpp: addObstacle for n cells of an empty
 * map in the given order + one update(), /root/reference/src/loc2d.cpp:61-108, src/sdm/dynamic_distance_map.cpp:160-226,281-330) --
 * what lama::DynamicDistanceMap::update() of a Loc2D runs before it uploads the result to the device.  Exposed so that the harness can
 * compare it with the checker and time it.  lama_dm_build returns the number of patches (kept until the next call on this thread;
 * -1: not buildable on the host, e.g. max_sqdist beyond the device's 14 bits) and update()'s return value in *processed;
 * lama_dm_build_fetch copies the records out (ids n, cells n x 10240 B, masks n x 16 words). */
int64_t lama_dm_build(const uint32_t* cells_xy, uint64_t n, uint32_t max_sqdist, uint32_t* processed);
int lama_dm_build_fetch(uint64_t* ids, uint8_t* cells, uint64_t* masks);
/* ---- lama::SimplePGO (include/lama/simple_pgo.h) flattened: poses {c, s, tx, ty}.  nodes4 [n][4] = node_list; loop closures
 * k < ne: edge_from[k] -> edge_to[k] with measurement edge4[k] (edge_list); fixed nodes k < nf: fixed_idx[k] at fixed4[k] (fixed_list).
 * Returns 1 when optimize() returned true (out4 [n][4] = the optimised node_list), 0 when it returned false (out4 = nodes4), -1 on an
 * error (no device library / HIP device: the message goes to err).  report and trace (one entry per LM try: 1 accepted, 0 rejected,
 * 2 rank deficient; at most trace_cap written) may be NULL. */
typedef struct lama_pgo_report {
    int32_t status;                 /* minisam NonlinearOptimizationStatus: 0 SUCCESS, 1 MAX_ITERATION, 2 ERROR_INCREASE, 3 RANK_DEFICIENCY */
    uint32_t iterations, tries;
    double initial_error, final_error;   /* 0.5 * sum of squared whitened errors */
    uint64_t nnz_L;
    double ms_device_linearize, ms_device_try, ms_analyze, ms_factorize, ms_total;
} lama_pgo_report;
int lama_pgo_optimize(const double* nodes4, uint32_t n, const int32_t* edge_from, const int32_t* edge_to, const double* edge4, uint32_t ne,
                      const int32_t* fixed_idx, const double* fixed4, uint32_t nf, int32_t device, double* out4, lama_pgo_report* report,
                      int8_t* trace, uint32_t trace_cap, char* err, int errcap);
/* The same with the choice of the linear solver (lama::SimplePGO::linear_solver and its pcg_* members).  Both structs begin with their
 * own size as the CALLER compiled it: the library reads and writes at most that many bytes, so either may grow at its end.
 * lama_pgo_report2 is lama_pgo_report behind struct_bytes, then the counters of the device solver (all zero with the host LDL^T). */
typedef struct lama_pgo_options {
    uint32_t struct_bytes;          /* sizeof(lama_pgo_options) */
    int32_t device;
    int32_t linear_solver;          /* 0: sparse LDL^T on the host (what lama_pgo_optimize runs), 1: block-Jacobi PCG on the device */
    uint32_t pcg_max_iterations;    /* 0: max(100, 6 n) */
    double pcg_rel_tol;             /* ||r|| <= pcg_rel_tol ||b||; 1e-10 in lama::SimplePGO */
} lama_pgo_options;
typedef struct lama_pgo_report2 {
    uint32_t struct_bytes;          /* sizeof(lama_pgo_report2), set by the caller */
    int32_t status;
    uint32_t iterations, tries;
    double initial_error, final_error;
    uint64_t nnz_L;                 /* 0 when no try needed the host factorisation */
    double ms_device_linearize, ms_device_try, ms_analyze, ms_factorize, ms_total;
    uint64_t pcg_iterations;        /* summed over the tries */
    uint32_t pcg_max_iterations_seen;    /* the longest solve */
    uint32_t pcg_fallbacks;         /* tries that reached the iteration cap and were solved by the host LDL^T instead */
    double ms_device_solve;         /* device time of the solves, summed */
} lama_pgo_report2;
int lama_pgo_optimize_with(const double* nodes4, uint32_t n, const int32_t* edge_from, const int32_t* edge_to, const double* edge4,
                           uint32_t ne, const int32_t* fixed_idx, const double* fixed4, uint32_t nf, const lama_pgo_options* options,
                           double* out4, lama_pgo_report2* report, int8_t* trace, uint32_t trace_cap, char* err, int errcap);
/* ---- lama::PoseGraph2D (include/lama/pose_graph_2d.h) flattened: nodes4 [n][4]; factor k < nf on nodes fi[k], fj[k] (fj = -1: a prior on
 * fi[k]) with measurement meas4[k], sigmas3[k] and the loss loss_kind[k] (LAMA_HIP_PGO_LOSS_* of include/lama_hip.h: 0 none, 1 Huber,
 * 2 Cauchy, 3 DCS) with parameter loss_param[k]; both loss arrays NULL: no losses.  Any other negative fj is an invalid index.  options NULL: the defaults.  Returns as
 * lama_pgo_optimize_with; weights [nf] (may be NULL) receives lama::PoseGraph2D::weights when optimize() ran (1 or 0 returned with
 * report.status != -1) and is left untouched otherwise. */
int lama_pose_graph_optimize(const double* nodes4, uint32_t n, const int32_t* fi, const int32_t* fj, const double* meas4,
                             const double* sigmas3, const int32_t* loss_kind, const double* loss_param, uint32_t nf,
                             const lama_pgo_options* options, double* out4, double* weights, lama_pgo_report2* report, int8_t* trace,
                             uint32_t trace_cap, char* err, int errcap);
/* ---- lama::MapBuilder2D (include/lama/map_builder_2d.h), flattened: a map rebuilt from posed key scans ---- */
typedef struct lama_mapbuilder lama_mapbuilder;
typedef struct lama_mapbuilder_options {
    double resolution, l2_max;          /* l2_max 0: no distance map */
    uint32_t patch_size;
    int32_t full, prune, gpu_device;
    uint32_t window_patches, occ_patch_capacity, dm_patch_capacity;
} lama_mapbuilder_options;
void lama_mapbuilder_default_options(lama_mapbuilder_options* o);
lama_mapbuilder* lama_mapbuilder_create(const lama_mapbuilder_options* o, char* err, int errcap);
void lama_mapbuilder_destroy(lama_mapbuilder* b);
const char* lama_mapbuilder_last_error(const lama_mapbuilder* b);
const char* lama_mapbuilder_engine_origin(const lama_mapbuilder* b);
void* lama_mapbuilder_device_context(const lama_mapbuilder* b);
/* add: returns the key id (< 0: error); pose4 {c, s, tx, ty}.  set_poses: one pose per key.  build / reset: 0 or < 0. */
int64_t lama_mapbuilder_add(lama_mapbuilder* b, const double* pts_xyz, uint32_t n, const double* origin3, const double* quat_wxyz, const double* pose4);
int lama_mapbuilder_set_pose(lama_mapbuilder* b, uint64_t key, const double* pose4);
int lama_mapbuilder_set_poses(lama_mapbuilder* b, const double* poses4, uint64_t n);
int lama_mapbuilder_build(lama_mapbuilder* b);
int lama_mapbuilder_reset(lama_mapbuilder* b);
/* the occupied cells the last build found (returns their number; up to cap {x, y} pairs written), and its wall-clock
 * milliseconds by stage: integrate, occupied list, distance map */
int64_t lama_mapbuilder_occupied_cells(const lama_mapbuilder* b, uint32_t* xy_out, uint64_t cap);
int lama_mapbuilder_timing(const lama_mapbuilder* b, double* ms3);
/* visit_all_cells of getOccupancyMap() (which 0) / getDistanceMap() (which 1): returns the count, < 0 when there is no map */
int64_t lama_mapbuilder_view_cells(lama_mapbuilder* b, int which, uint32_t* xy_out, uint64_t cap);
/* lama::Solve(GaussNewton + Cauchy(0.15), MatchSurface2D(getDistanceMap(), scan, pose)): pose4 in / out */
int lama_mapbuilder_match_solve(lama_mapbuilder* b, const double* pts_xyz, uint32_t n, const double* origin3, const double* quat_wxyz,
                                double* pose4, uint32_t max_iterations, uint32_t* iterations);
/* ---- dense grids (include/lama/sdm/grid.h): getOccupancyGrid / getDistanceGrid of the classes above, made on the device.
 * options NULL: the defaults (whole map, stride 1, trinary).  Each call returns 1 when the grid was made -- its header in *out, its
 * pixels (row-major, x fastest; int8 occupancy, uint16 squared cell distances) kept on the calling thread until its next grid call --,
 * 0 when the object has no such map (before the first scan / build, a particle of another process), -2 on a failure (message through
 * the object's last_error: a device library without lama_hip_map_rasterize, an invalid stride, ...).  lama_grid_fetch copies the kept
 * pixels when cap_bytes suffices and returns their size in bytes.  lama_pf_*: particle < 0 is the best particle. */
typedef struct lama_grid_options {
    uint32_t stride;
    int32_t probability, whole_map;
    double world_min[2], world_max[2];
} lama_grid_options;
typedef struct lama_grid {
    uint32_t x0, y0, width, height, stride, element_bytes;
    double resolution, cell_size, max_distance;      /* max_distance: distance grids, metres */
    double origin[3];                                /* Map::m2w of cell (x0, y0), z = 0 */
} lama_grid;
void lama_grid_default_options(lama_grid_options* o);
int64_t lama_grid_fetch(void* out, uint64_t cap_bytes);
int lama_slam_occupancy_grid(lama_slam* s, const lama_grid_options* options, lama_grid* out);
int lama_slam_distance_grid(lama_slam* s, const lama_grid_options* options, lama_grid* out);
int lama_pf_occupancy_grid(lama_pf* pf, int64_t particle, const lama_grid_options* options, lama_grid* out);
int lama_pf_distance_grid(lama_pf* pf, int64_t particle, const lama_grid_options* options, lama_grid* out);
int lama_mapbuilder_occupancy_grid(lama_mapbuilder* b, const lama_grid_options* options, lama_grid* out);
int lama_mapbuilder_distance_grid(lama_mapbuilder* b, const lama_grid_options* options, lama_grid* out);
int lama_lo_occupancy_grid(lama_lo* l, const lama_grid_options* options, lama_grid* out);
int lama_lo_distance_grid(lama_lo* l, const lama_grid_options* options, lama_grid* out);
int lama_loc_distance_grid(lama_loc* l, const lama_grid_options* options, lama_grid* out);
/* ---- ray casts (include/lama/sdm/ray_cast.h): castRays of the classes above -- what a sensor at each of num_poses poses {c, s, tx, ty}
 * would see in the object's device map, per pose and point of the scan the first cell that stops the beam.  options NULL: the defaults
 * (occupancy map -- lama_loc_*: the distance map, the only one it has on the device --, unknown cells do not stop a beam, no labels).
 * Every array of *out may be NULL; the others hold num_poses * n elements (cell_xy twice as many, start_xy 2 * num_poses), label is
 * written with tolerance_cells >= 0 only, range is in metres (+inf where nothing stopped the beam).  Returns 1 when the rays were cast,
 * 0 when the object has no such map (before the first scan / build, a particle of another process), -2 on a failure (message through
 * the object's last_error: a device library without lama_hip_map_cast_rays, a beam of more than 8191 cells, ...).  lama_pf_*:
 * particle < 0 is the best particle.  lama_loc_check_scan: Loc2D::checkScan -- one label per point (0 agrees, 1 blocked, 2 novel) at the
 * current pose; returns their number, 0 while there is no device map, -2 on a failure. */
typedef struct lama_ray_options {
    int32_t map;                 /* 0 distance map, 1 occupancy map (LAMA_HIP_MAP_*) */
    int32_t stop_at_unknown;     /* occupancy map only */
    int32_t tolerance_cells;     /* >= 0: label the beams */
} lama_ray_options;
typedef struct lama_ray_result {
    uint8_t* status; int32_t* step; uint32_t* nn; uint32_t* cell_xy; uint32_t* end_sqdist; uint8_t* label; uint32_t* start_xy; double* range;
} lama_ray_result;
void lama_ray_default_options(lama_ray_options* o);
/* the host loop a caller had before castRays, for comparison (tools/raycast_query_bench.py): getOccupancyMap()'s snapshot walked per
 * pose and point from the sensor's cell to the point's, isOccupied per cell; step_out [num_poses][n]: the index of the first occupied
 * cell, -1 for none.  Returns 0, -1 before the first scan, -2 on a failure. */
int lama_slam_view_cast_rays(lama_slam* s, const double* poses4, uint32_t num_poses, const double* pts_xyz, uint32_t n, int32_t* step_out);
int lama_slam_cast_rays(lama_slam* s, const double* poses4, uint32_t num_poses, const double* pts_xyz, uint32_t n, const double* origin3,
                        const double* quat_wxyz, const lama_ray_options* options, lama_ray_result* out);
int lama_pf_cast_rays(lama_pf* pf, int64_t particle, const double* poses4, uint32_t num_poses, const double* pts_xyz, uint32_t n, const double* origin3,
                      const double* quat_wxyz, const lama_ray_options* options, lama_ray_result* out);
int lama_mapbuilder_cast_rays(lama_mapbuilder* b, const double* poses4, uint32_t num_poses, const double* pts_xyz, uint32_t n, const double* origin3,
                              const double* quat_wxyz, const lama_ray_options* options, lama_ray_result* out);
int lama_lo_cast_rays(lama_lo* l, const double* poses4, uint32_t num_poses, const double* pts_xyz, uint32_t n, const double* origin3,
                      const double* quat_wxyz, const lama_ray_options* options, lama_ray_result* out);
int lama_loc_cast_rays(lama_loc* l, const double* poses4, uint32_t num_poses, const double* pts_xyz, uint32_t n, const double* origin3,
                       const double* quat_wxyz, const lama_ray_options* options, lama_ray_result* out);
int64_t lama_loc_check_scan(lama_loc* l, const double* pts_xyz, uint32_t n, const double* origin3, const double* quat_wxyz, int32_t tolerance_cells,
                            uint8_t* labels_out);
/* ---- frontiers (include/lama/sdm/frontier.h): getFrontiers of the classes above -- the clusters of free pixels that border unknown
 * space in the object's device occupancy map, labelled on the device.  options NULL: the defaults (whole map, stride 1, every cluster,
 * no label grid).  Each call returns 1 when the frontiers were made -- the box and the counts in *out, the records (by pixels
 * descending, then label ascending) and the label grid ([height][width] uint32, 0xFFFFFFFF where the pixel is no frontier; with
 * options->labels only) kept on the calling thread until its next frontier call --, 0 when the object has no map (before the first scan
 * / build, a particle of another process), -2 on a failure (message through the object's last_error: a device library without
 * lama_hip_map_frontiers, an invalid stride, ...).  lama_frontiers_fetch copies the kept records and labels, each when its pointer is
 * not NULL and its capacity (in elements) suffices, and returns the number of records.  lama_pf_*: particle < 0 is the best particle.
 * (lama_loc has none: its occupancy map is a host map.) */
typedef struct lama_frontier_options {
    uint32_t stride;
    int32_t whole_map;
    double world_min[2], world_max[2];
    uint32_t min_pixels, max_frontiers;      /* max_frontiers 0: all */
    int32_t labels;
} lama_frontier_options;
typedef struct lama_frontier {
    uint32_t label, pixels, min_i, min_j, max_i, max_j;
    uint64_t sum_i, sum_j;
    double centroid[2], seed[2];             /* world metres */
} lama_frontier;
typedef struct lama_frontier_set {
    uint32_t x0, y0, width, height, stride, count;   /* count: the records kept (clusters, or max_frontiers if that is smaller) */
    double resolution, cell_size;
    double origin[3];                                /* Map::m2w of cell (x0, y0), z = 0 */
    uint64_t frontier_pixels, clusters;
} lama_frontier_set;
void lama_frontier_default_options(lama_frontier_options* o);
int64_t lama_frontiers_fetch(lama_frontier* records, uint64_t cap_records, uint32_t* labels, uint64_t cap_labels);
int lama_slam_frontiers(lama_slam* s, const lama_frontier_options* options, lama_frontier_set* out);
int lama_pf_frontiers(lama_pf* pf, int64_t particle, const lama_frontier_options* options, lama_frontier_set* out);
int lama_mapbuilder_frontiers(lama_mapbuilder* b, const lama_frontier_options* options, lama_frontier_set* out);
int lama_lo_frontiers(lama_lo* l, const lama_frontier_options* options, lama_frontier_set* out);
/* ---- routes (include/lama/sdm/travel.h): planRoutes of the classes above -- from the world points from_xy [n_from][2] to each of
 * goals_xy [n_goals][2] (metres) through the object's device maps: reachability, cost and path, relaxed on the device.  options NULL:
 * the defaults (whole map, stride 1, a point robot, paths of up to 1024 points, no field).  Each call returns 1 when the routes were
 * made -- the box and the counts in *out; the routes, the path points (world metres, source first, route after route) and the field
 * ([height][width] uint32, 0xFFFFFFFF where no route leads; with options->field only) kept on the calling thread until its next route
 * call --, 0 when the object has no map (before the first scan / build, a particle of another process), -2 on a failure (message
 * through the object's last_error: a device library without lama_hip_map_travel, a start point outside the box, ...).
 * lama_routes_fetch copies what was kept, each array when its pointer is not NULL and its capacity (in elements; path points count
 * two doubles each) suffices, and returns the number of routes.  lama_pf_*: particle < 0 is the best particle.  lama_loc_*: the
 * distance map alone decides what is traversable (its occupancy map is a host map). */
typedef struct lama_travel_options {
    uint32_t stride;
    int32_t whole_map;
    double world_min[2], world_max[2];
    double robot_radius, preferred_clearance;        /* metres */
    uint32_t near_factor, goal_reach, max_path_points;
    int32_t field;
} lama_travel_options;
typedef struct lama_route {
    uint32_t status, pixel, cost, steps;             /* status: 0 reached, 1 unreached, 2 the goal lies outside the box */
    double length_m;                                 /* cost * cell_size / 5 */
    uint64_t path_first;                             /* the route's first point among the kept path points */
    uint32_t path_points, reserved;                  /* min(max_path_points, steps + 1); 0 unless reached */
} lama_route;
typedef struct lama_route_set {
    uint32_t x0, y0, width, height, stride, count;   /* count: the routes, one per goal */
    double resolution, cell_size;
    double origin[3];                                /* Map::m2w of cell (x0, y0), z = 0 */
    uint64_t path_points;                            /* of all routes together */
    uint32_t rounds, has_field;
} lama_route_set;
void lama_travel_default_options(lama_travel_options* o);
int64_t lama_routes_fetch(lama_route* routes, uint64_t cap_routes, double* path_xy, uint64_t cap_points, uint32_t* field, uint64_t cap_field);
int lama_slam_plan_routes(lama_slam* s, const double* from_xy, uint32_t n_from, const double* goals_xy, uint32_t n_goals, const lama_travel_options* options, lama_route_set* out);
int lama_pf_plan_routes(lama_pf* pf, int64_t particle, const double* from_xy, uint32_t n_from, const double* goals_xy, uint32_t n_goals, const lama_travel_options* options,
                        lama_route_set* out);
int lama_mapbuilder_plan_routes(lama_mapbuilder* b, const double* from_xy, uint32_t n_from, const double* goals_xy, uint32_t n_goals, const lama_travel_options* options,
                                lama_route_set* out);
int lama_lo_plan_routes(lama_lo* l, const double* from_xy, uint32_t n_from, const double* goals_xy, uint32_t n_goals, const lama_travel_options* options, lama_route_set* out);
int lama_loc_plan_routes(lama_loc* l, const double* from_xy, uint32_t n_from, const double* goals_xy, uint32_t n_goals, const lama_travel_options* options, lama_route_set* out);
/* lama::random (include/lama/random.h) */
void lama_random_set_seed(uint32_t seed);
double lama_random_uniform(void);

#ifdef __cplusplus
}
#endif
#endif
