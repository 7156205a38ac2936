// host_capi.cpp -- extern "C" flattening of lama::PFSlam2D (include/lama_host.h).
#include "lama_host.h"
#include "lama/match_surface_2d.h"
#include "lama/nlls/solver.h"

#include <algorithm>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

#include "hip_engine.hpp"
#include "lama/pf_slam2d.h"
#include "lama/lidar_odometry_2d.h"
#include "lama/loc2d.h"
#include "lama/random.h"
#include "lama/sdm_io.h"
#include "dm_builder.hpp"
#include "lama/slam2d.h"
#include "lama/pose_graph_2d.h"
#include "lama/simple_pgo.h"
#include "lama/map_builder_2d.h"
#include "lama/correlative_search_2d.h"

using namespace lama;

struct lama_pf {
    std::unique_ptr<PFSlam2D> pf;
    std::string error;
    std::string origin;
    double times[5] = {0, 0, 0, 0, 0};
};

namespace {

PointCloudXYZ::Ptr make_cloud(const double* pts, uint32_t n, const double* origin3, const double* quat)
{
    auto c = std::make_shared<PointCloudXYZ>();
    c->points.resize(n);
    for (uint32_t i = 0; i < n; ++i) c->points[i] = Vector3d(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    if (origin3) c->sensor_origin_ = Vector3d(origin3[0], origin3[1], origin3[2]);
    if (quat) c->sensor_orientation_ = Quaterniond(quat[0], quat[1], quat[2], quat[3]);
    return c;
}

template <class F>
int guarded(lama_pf* pf, F&& f)
{
    try {
        return f();
    } catch (const std::exception& e) {
        pf->error = e.what();
        return -1;
    } catch (...) {
        pf->error = "unknown exception";
        return -1;
    }
}

void collect_times(lama_pf* h, size_t before[5])
{
    const PFSlam2D::Summary* s = h->pf->summary;
    if (!s) return;
    const DynamicArray<double>* v[5] = {&s->time, &s->time_solving, &s->time_normalizing, &s->time_resampling, &s->time_mapping};
    for (int k = 0; k < 5; ++k) h->times[k] = v[k]->size() > before[k] ? v[k]->back() : 0.0;
}

void sizes(const lama_pf* h, size_t out[5])
{
    const PFSlam2D::Summary* s = h->pf->summary;
    for (int k = 0; k < 5; ++k) out[k] = 0;
    if (!s) return;
    out[0] = s->time.size(); out[1] = s->time_solving.size(); out[2] = s->time_normalizing.size();
    out[3] = s->time_resampling.size(); out[4] = s->time_mapping.size();
}

} // namespace

extern "C" {

void lama_pf_default_options(lama_pf_options* o)
{
    PFSlam2D::Options d;
    std::memset(o, 0, sizeof(*o));
    o->particles = d.particles; o->srr = d.srr; o->str = d.str; o->stt = d.stt; o->srt = d.srt;
    o->meas_sigma = d.meas_sigma; o->meas_sigma_gain = d.meas_sigma_gain;
    o->trans_thresh = d.trans_thresh; o->rot_thresh = d.rot_thresh; o->l2_max = d.l2_max;
    o->truncated_ray = d.truncated_ray; o->truncated_range = d.truncated_range; o->resolution = d.resolution;
    o->patch_size = d.patch_size; o->max_iter = d.max_iter; o->seed = d.seed;
    o->create_summary = 1; o->gpu_device = 0; o->shard_rank = 0; o->shard_world = 1; o->profile = 0;
}

#ifdef LAMA_TESTING      // test builds of the host library only; the shipped liblama_host.so does not export this
int lama_host_set_engine_library(const char* path)
{
    try {
        if (!path || !*path) { setEngineOverride(nullptr); return 0; }
        setEngineOverride(loadHipEngine(path));
        return 0;
    } catch (...) {
        return -1;
    }
}
#endif

lama_pf* lama_pf_create(const lama_pf_options* o, char* err, int errcap)
{
    auto* h = new lama_pf;
    try {
        PFSlam2D::Options p;
        p.particles = o->particles; p.srr = o->srr; p.str = o->str; p.stt = o->stt; p.srt = o->srt;
        p.meas_sigma = o->meas_sigma; p.meas_sigma_gain = o->meas_sigma_gain;
        p.trans_thresh = o->trans_thresh; p.rot_thresh = o->rot_thresh; p.l2_max = o->l2_max;
        p.truncated_ray = o->truncated_ray; p.truncated_range = o->truncated_range; p.resolution = o->resolution;
        p.patch_size = o->patch_size; p.max_iter = o->max_iter; p.seed = o->seed;
        p.create_summary = o->create_summary != 0; p.gpu_device = o->gpu_device;
        p.shard_rank = o->shard_rank; p.shard_world = o->shard_world; p.profile = o->profile != 0;
        p.brushfire_mode = o->brushfire_mode;
        p.window_patches = o->window_patches; p.dm_patch_capacity = o->dm_patch_capacity;
        p.occ_patch_capacity = o->occ_patch_capacity; p.queue_capacity = o->queue_capacity;
        p.gpus = o->gpus > 1 ? o->gpus : 1;
        h->pf.reset(new PFSlam2D(p));
        h->origin = h->pf->engine()->origin;
        return h;
    } catch (const std::exception& e) {
        if (err && errcap > 0) { std::strncpy(err, e.what(), (size_t)errcap - 1); err[errcap - 1] = 0; }
        delete h;
        return nullptr;
    }
}

void lama_pf_destroy(lama_pf* pf) { delete pf; }
int lama_pf_exchange_times(const lama_pf* h, double* out8)
{
    const PFSlam2D::ExchangeTimes& x = h->pf->exchangeTimes();
    out8[0] = x.gather; out8[1] = x.ship; out8[2] = x.import_; out8[3] = (double)x.shipped_particles; out8[4] = (double)x.shipped_bytes;
    out8[5] = x.local_copies; out8[6] = x.phase_begin; out8[7] = x.phase_maps;
    return (int)h->pf->numShards();
}
void* lama_pf_shard_context(const lama_pf* h, uint32_t r)
{
    const PFSlam2D* s = h->pf->shard(r);
    return s ? (void*)s->deviceContext() : nullptr;
}
const char* lama_pf_last_error(const lama_pf* pf) { return pf ? pf->error.c_str() : "null handle"; }
const char* lama_pf_engine_origin(const lama_pf* pf) { return pf ? pf->origin.c_str() : ""; }

void lama_pf_set_prior(lama_pf* pf, double x, double y, double yaw) { pf->pf->setPrior(Pose2D(x, y, yaw)); }

int lama_pf_update(lama_pf* h, const double* pts, uint32_t n, const double* origin3, const double* quat,
                   const double* odom_xyr, double ts)
{
    return guarded(h, [&] {
        size_t before[5]; sizes(h, before);
        bool r = h->pf->update(make_cloud(pts, n, origin3, quat), Pose2D(odom_xyr[0], odom_xyr[1], odom_xyr[2]), ts);
        collect_times(h, before);
        return r ? 1 : 0;
    });
}

int lama_pf_update_begin(lama_pf* h, const double* pts, uint32_t n, const double* origin3, const double* quat,
                         const double* odom_xyr, double ts)
{
    return guarded(h, [&] { return (int)h->pf->updateBegin(make_cloud(pts, n, origin3, quat), Pose2D(odom_xyr[0], odom_xyr[1], odom_xyr[2]), ts); });
}

int lama_pf_local_range(const lama_pf* h, uint32_t* lo, uint32_t* hi)
{
    *lo = h->pf->localBegin(); *hi = h->pf->localEnd();
    return 0;
}

int lama_pf_local_loglik(const lama_pf* h, double* out)
{
    const auto& v = h->pf->localLogLik();
    std::memcpy(out, v.data(), sizeof(double) * v.size());
    return (int)v.size();
}

int lama_pf_plan_resample(lama_pf* h, const double* all_loglik, int32_t* idx_out)
{
    return guarded(h, [&] {
        std::vector<int32_t> idx;
        const bool r = h->pf->planResample(all_loglik, idx);
        if (r) std::memcpy(idx_out, idx.data(), sizeof(int32_t) * idx.size());
        return r ? 1 : 0;
    });
}

int lama_pf_apply_resample(lama_pf* h, const int32_t* idx)
{
    return guarded(h, [&] {
        std::vector<int32_t> v(idx, idx + h->pf->getOptions().particles);
        h->pf->applyResample(v);
        return 0;
    });
}

int lama_pf_update_maps(lama_pf* h) { return guarded(h, [&] { h->pf->updateMaps(); return 0; }); }
void* lama_pf_device_context(const lama_pf* h) { return (void*)h->pf->deviceContext(); }

int lama_pf_get_poses(const lama_pf* h, double* out)
{
    const auto& ps = h->pf->getParticles();
    for (size_t i = 0; i < ps.size(); ++i) ps[i].pose.state.toArray(out + 4 * i);
    return (int)ps.size();
}

int lama_pf_set_pose(lama_pf* h, uint32_t i, const double* pose4)
{
    auto& ps = const_cast<std::vector<PFSlam2D::Particle>&>(h->pf->getParticles());
    if (i >= ps.size()) return -1;
    ps[i].pose.state = SE2d::fromArray(pose4);
    return 0;
}

int lama_pf_get_weights(const lama_pf* h, double* w, double* nw, double* ws)
{
    const auto& ps = h->pf->getParticles();
    for (size_t i = 0; i < ps.size(); ++i) {
        if (w) w[i] = ps[i].weight;
        if (nw) nw[i] = ps[i].normalized_weight;
        if (ws) ws[i] = ps[i].weight_sum;
    }
    return (int)ps.size();
}

int lama_pf_set_weights(lama_pf* h, const double* w, const double* ws)
{
    auto& ps = const_cast<std::vector<PFSlam2D::Particle>&>(h->pf->getParticles());
    for (size_t i = 0; i < ps.size(); ++i) {
        if (w) ps[i].weight = w[i];
        if (ws) ps[i].weight_sum = ws[i];
    }
    return 0;
}

double lama_pf_neff(const lama_pf* h) { return h->pf->getNeff(); }
int lama_pf_best(const lama_pf* h) { return (int)h->pf->getBestParticleIdx(); }
int lama_pf_best_pose_xyr(const lama_pf* h, double* xyr)
{
    const Pose2D p = h->pf->getPose();
    xyr[0] = p.x(); xyr[1] = p.y(); xyr[2] = p.rotation();
    return 0;
}
uint32_t lama_pf_num_resamples(const lama_pf* h) { return h->pf->numResamples(); }
uint64_t lama_pf_memory_usage(const lama_pf* h) { return h->pf->getMemoryUsage(); }

int lama_pf_summary(const lama_pf* h, char* buf, int cap)
{
    if (!h->pf->summary) return 0;
    const std::string r = h->pf->summary->report();
    if (buf && cap > 0) { std::strncpy(buf, r.c_str(), (size_t)cap - 1); buf[cap - 1] = 0; }
    return (int)r.size() + 1;
}

int lama_pf_last_times(const lama_pf* h, double* out5)
{
    std::memcpy(out5, h->times, sizeof(h->times));
    return 0;
}

int lama_pf_draw_from_motion(lama_pf* h, const double* delta4, double* pose4)
{
    return guarded(h, [&] {
        Pose2D pose(SE2d::fromArray(pose4));
        h->pf->drawFromMotion(Pose2D(SE2d::fromArray(delta4)), pose);
        pose.state.toArray(pose4);
        return 0;
    });
}

double lama_pf_normalize(lama_pf* h) { h->pf->normalize(); return h->pf->getNeff(); }

int lama_pf_resample_indices(const lama_pf* h, double u01, int32_t* out)
{
    const std::vector<int32_t> v = h->pf->resampleIndices(u01);
    std::memcpy(out, v.data(), sizeof(int32_t) * v.size());
    return (int)v.size();
}

void lama_pose_minus(const double* a4, const double* b4, double* out4)
{
    (Pose2D(SE2d::fromArray(a4)) - Pose2D(SE2d::fromArray(b4))).state.toArray(out4);
}

void lama_pose_from_xyr(double x, double y, double yaw, double* out4) { Pose2D(x, y, yaw).state.toArray(out4); }

// ------------------------------------------------------------------ Slam2D
struct lama_slam {
    std::unique_ptr<Slam2D> s;
    std::string error, origin;
};

void lama_slam_default_options(lama_slam_options* o)
{
    Slam2D::Options d;
    o->trans_thresh = d.trans_thresh; o->rot_thresh = d.rot_thresh; o->l2_max = d.l2_max; o->truncated_ray = d.truncated_ray;
    o->truncated_range = d.truncated_range; o->resolution = d.resolution; o->patch_size = d.patch_size; o->max_iter = d.max_iter;
    o->gpu_device = 0;
    o->transient_map = d.transient_map ? 1 : 0;
    o->lm = 0;
}

lama_slam* lama_slam_create(const lama_slam_options* o, char* err, int errcap)
{
    auto* h = new lama_slam;
    try {
        Slam2D::Options p;
        p.trans_thresh = o->trans_thresh; p.rot_thresh = o->rot_thresh; p.l2_max = o->l2_max; p.truncated_ray = o->truncated_ray;
        p.truncated_range = o->truncated_range; p.resolution = o->resolution; p.patch_size = o->patch_size; p.max_iter = o->max_iter;
        p.gpu_device = o->gpu_device;
        p.transient_map = o->transient_map != 0;
        if (o->lm) p.strategy = "lm";
        h->s.reset(new Slam2D(p));
        h->origin = h->s->engine()->origin;
        return h;
    } catch (const std::exception& e) {
        if (err && errcap > 0) { std::strncpy(err, e.what(), (size_t)errcap - 1); err[errcap - 1] = 0; }
        delete h;
        return nullptr;
    }
}
void lama_slam_destroy(lama_slam* s) { delete s; }
const char* lama_slam_last_error(const lama_slam* s) { return s ? s->error.c_str() : "null handle"; }
const char* lama_slam_engine_origin(const lama_slam* s) { return s ? s->origin.c_str() : ""; }
void lama_slam_set_pose(lama_slam* s, double x, double y, double yaw) { s->s->setPose(Pose2D(x, y, yaw)); }
int lama_slam_get_pose(const lama_slam* s, double* pose4) { s->s->getPose().state.toArray(pose4); return 0; }
int lama_slam_update(lama_slam* h, const double* pts, uint32_t n, const double* origin3, const double* quat, const double* odom_xyr, double ts)
{
    try {
        return h->s->update(make_cloud(pts, n, origin3, quat), Pose2D(odom_xyr[0], odom_xyr[1], odom_xyr[2]), ts) ? 1 : 0;
    } catch (const std::exception& e) { h->error = e.what(); return -1; }
}
int lama_slam_enough_motion(lama_slam* h, const double* odom_xyr) { return h->s->enoughMotion(Pose2D(odom_xyr[0], odom_xyr[1], odom_xyr[2])) ? 1 : 0; }
uint32_t lama_slam_processed_cells(const lama_slam* h) { return h->s->getNumberOfProcessedCells(); }
uint32_t lama_slam_deleted_patches(const lama_slam* h) { return h->s->getLastDeletedPatches(); }
uint32_t lama_slam_iterations(const lama_slam* h) { return h->s->getLastIterations(); }
void* lama_slam_device_context(const lama_slam* h) { return (void*)h->s->deviceContext(); }

}   // extern "C"
namespace {
template <class M>
int view_bounds(const M* m, uint32_t* min3, uint32_t* max3, double* wmin3, double* wmax3)
{
    if (!m) return -1;
    Vector3ui a, b;
    Vector3d wa, wb;
    m->bounds(a, b);
    m->bounds(wa, wb);
    for (int k = 0; k < 3; ++k) { min3[k] = a(k); max3[k] = b(k); wmin3[k] = wa[k]; wmax3[k] = wb[k]; }
    return 0;
}
template <class M>
int64_t view_cells(const M* m, uint32_t* xy_out, uint64_t cap)
{
    if (!m) return -1;
    uint64_t n = 0;
    m->visit_all_cells([&](const Vector3ui& c) {
        if (n < cap) { xy_out[2 * n] = c(0); xy_out[2 * n + 1] = c(1); }
        ++n;
    });
    return (int64_t)n;
}
}
extern "C" {

int lama_slam_view_bounds(lama_slam* h, int which, uint32_t* min3, uint32_t* max3, double* wmin3, double* wmax3)
{
    try {
        return which == 0 ? view_bounds(h->s->getOccupancyMap(), min3, max3, wmin3, wmax3) : view_bounds(h->s->getDistanceMap(), min3, max3, wmin3, wmax3);
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}
int64_t lama_slam_view_cells(lama_slam* h, int which, uint32_t* xy_out, uint64_t cap)
{
    try {
        return which == 0 ? view_cells(h->s->getOccupancyMap(), xy_out, cap) : view_cells(h->s->getDistanceMap(), xy_out, cap);
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}
int lama_slam_view_occupancy(lama_slam* h, uint64_t n, const uint32_t* xy, uint8_t* is_free, uint8_t* is_occupied, uint8_t* is_unknown, double* probability)
{
    try {
        const FrequencyOccupancyMap* m = h->s->getOccupancyMap();
        if (!m) return -1;
        for (uint64_t i = 0; i < n; ++i) {
            const Vector3ui c(xy[2 * i], xy[2 * i + 1], 0);
            is_free[i] = m->isFree(c); is_occupied[i] = m->isOccupied(c); is_unknown[i] = m->isUnknown(c); probability[i] = m->getProbability(c);
        }
        return 0;
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}
// the host loop a caller had before castRays (tools/raycast_query_bench.py measures it): per pose and point the cells from the sensor's
// cell to the point's over getOccupancyMap()'s snapshot -- Map::computeRay's cells in the closed form floor((2 t a + nn) / (2 nn)) of the
// map update, then the point's cell -- with isOccupied per cell; step_out: the index of the first occupied one, -1 for none
int lama_slam_view_cast_rays(lama_slam* h, const double* poses4, uint32_t num_poses, const double* pts, uint32_t n, int32_t* step_out)
{
    try {
        const FrequencyOccupancyMap* m = h->s->getOccupancyMap();
        if (!m) return -1;
        for (uint32_t k = 0; k < num_poses; ++k) {
            const double c = poses4[4 * (size_t)k], s = poses4[4 * (size_t)k + 1], tx = poses4[4 * (size_t)k + 2], ty = poses4[4 * (size_t)k + 3];
            const Vector3ui ms = m->w2m(Vector3d(tx, ty, 0.0));
            for (uint32_t i = 0; i < n; ++i) {
                const double px = pts[3 * (size_t)i], py = pts[3 * (size_t)i + 1];
                const Vector3ui mh = m->w2m(Vector3d((c * px - s * py) + tx, (s * px + c * py) + ty, pts[3 * (size_t)i + 2]));
                const int64_t d0 = (int64_t)mh(0) - (int64_t)ms(0), d1 = (int64_t)mh(1) - (int64_t)ms(1), d2 = (int64_t)mh(2) - (int64_t)ms(2);
                const int64_t a0 = d0 < 0 ? -d0 : d0, a1 = d1 < 0 ? -d1 : d1, a2 = d2 < 0 ? -d2 : d2, nn = std::max(a0, std::max(a1, a2));
                int32_t step = -1;
                for (int64_t t = 1; t <= nn && step < 0; ++t) {
                    const int64_t x = (int64_t)ms(0) + (d0 < 0 ? -1 : 1) * ((2 * t * a0 + nn) / (2 * nn)), y = (int64_t)ms(1) + (d1 < 0 ? -1 : 1) * ((2 * t * a1 + nn) / (2 * nn));
                    if (m->isOccupied(Vector3ui((uint32_t)x, (uint32_t)y, 0))) step = (int32_t)(t - 1);
                }
                step_out[(size_t)k * n + i] = step;
            }
        }
        return 0;
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}
int lama_slam_view_distance_cells(lama_slam* h, uint64_t n, const uint32_t* xy, double* distance)
{
    try {
        const DynamicDistanceMap* m = h->s->getDistanceMap();
        if (!m) return -1;
        for (uint64_t i = 0; i < n; ++i) distance[i] = m->distance(Vector3ui(xy[2 * i], xy[2 * i + 1], 0));
        return 0;
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}
static PointCloudXYZ::Ptr cloud_of(const double* pts, uint32_t n, const double* o, const double* q)
{
    PointCloudXYZ::Ptr c(new PointCloudXYZ);
    c->points.reserve(n);
    for (uint32_t i = 0; i < n; ++i) c->points.push_back(Vector3d(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
    if (o) c->sensor_origin_ = Vector3d(o[0], o[1], o[2]);
    if (q) c->sensor_orientation_ = Quaterniond(q[0], q[1], q[2], q[3]);
    return c;
}

int lama_slam_match_eval(lama_slam* h, const double* pts, uint32_t n, const double* o, const double* q, const double* pose4,
                         double* residuals, double* jacobian, double* rmse_out)
{
    try {
        const DynamicDistanceMap* dm = h->s->getDistanceMap();
        if (!dm) return -1;
        MatchSurface2D problem(dm, cloud_of(pts, n, o, q), SE2d::fromArray(pose4));
        VectorXd r;
        MatrixXd J;
        problem.eval(r, jacobian ? &J : nullptr);
        for (uint32_t i = 0; i < n; ++i) residuals[i] = r[i];
        if (jacobian) for (uint32_t c = 0; c < 3; ++c) for (uint32_t i = 0; i < n; ++i) jacobian[(size_t)c * n + i] = J(i, c);
        if (rmse_out) *rmse_out = problem.error();
        return 0;
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}

int lama_slam_match_solve(lama_slam* h, const double* pts, uint32_t n, const double* o, const double* q, double* pose4, const char* strategy,
                          const char* weight, double weight_param, uint32_t max_iterations, double* cov9, uint32_t* iterations)
{
    try {
        const DynamicDistanceMap* dm = h->s->getDistanceMap();
        if (!dm) return -1;
        MatchSurface2D problem(dm, cloud_of(pts, n, o, q), SE2d::fromArray(pose4));
        Solver::Options so;
        so.max_iterations = max_iterations;
        const std::string st(strategy ? strategy : "gn"), w(weight ? weight : "cauchy");
        if (st == "lm") so.strategy.reset(new LevenbergMarquard); else so.strategy.reset(new GaussNewton);
        if (w == "cauchy") so.robust_cost.reset(new CauchyWeight(weight_param));
        else if (w == "tukey") so.robust_cost.reset(new TukeyWeight(weight_param));
        else if (w == "huber") so.robust_cost.reset(new HuberWeight(weight_param));
        else so.robust_cost.reset(new UnitWeight);
        Solver solver(so);
        MatrixXd cov;
        try {
            solver.solve(problem, cov9 ? &cov : nullptr);
        } catch (const std::invalid_argument& e) { h->error = e.what(); return -3; }
        problem.getState().toArray(pose4);
        if (cov9) for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) cov9[3 * r + c] = cov(r, c);
        if (iterations) *iterations = solver.lastIterations();
        return 0;
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}

namespace {
bool solver_options_of(const char* strategy, const char* weight, double weight_param, double eps1, uint32_t max_iterations, Solver::Options* so)
{
    so->max_iterations = max_iterations;
    const std::string st(strategy ? strategy : "gn"), w(weight ? weight : "cauchy");
    if (st == "lm") { LevenbergMarquard::Options o; if (eps1 > 0) o.eps1 = eps1; so->strategy.reset(new LevenbergMarquard(o)); }
    else if (st == "gn") { GaussNewton::Options o; if (eps1 > 0) o.eps1 = eps1; so->strategy.reset(new GaussNewton(o)); }
    else return false;
    if (w == "cauchy") so->robust_cost.reset(new CauchyWeight(weight_param));
    else if (w == "tukey") so->robust_cost.reset(new TukeyWeight(weight_param));
    else if (w == "huber") so->robust_cost.reset(new HuberWeight(weight_param));
    else if (w == "tdist") so->robust_cost.reset(new TDistributionWeight(weight_param));
    else if (w == "unit") so->robust_cost.reset(new UnitWeight);
    else return false;
    return true;
}

// a Problem that forwards to a MatchSurface2D without being one: Solver::solve then runs its generic host loop around the device's
// per-beam evaluation (lama_hip_match_eval) instead of the fused kernel
struct ForwardingProblem : public Problem {
    explicit ForwardingProblem(MatchSurface2D* m) : m_(m) {}
    void eval(VectorXd& residuals, MatrixXd* J) override { m_->eval(residuals, J); }
    void update(const VectorXd& h) override { m_->update(h); }
    MatchSurface2D* m_;
};
}

int lama_slam_match_solve_generic(lama_slam* h, const double* pts, uint32_t n, const double* o, const double* q, double* pose4, const char* strategy,
                                  const char* weight, double weight_param, uint32_t max_iterations, double* cov9, uint32_t* iterations)
{
    try {
        const DynamicDistanceMap* dm = h->s->getDistanceMap();
        if (!dm) return -1;
        MatchSurface2D problem(dm, cloud_of(pts, n, o, q), SE2d::fromArray(pose4));
        ForwardingProblem fwd(&problem);
        Solver::Options so;
        if (!solver_options_of(strategy, weight, weight_param, 0.0, max_iterations, &so)) { h->error = "unknown strategy or weight"; return -3; }
        Solver solver(so);
        MatrixXd cov;
        solver.solve(fwd, cov9 ? &cov : nullptr);
        problem.getState().toArray(pose4);
        if (cov9) for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) cov9[3 * r + c] = cov(r, c);
        if (iterations) *iterations = solver.lastIterations();
        return 0;
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}

int lama_slam_solve_batch(lama_slam* h, lama_slam* other, uint32_t num_problems, const double* pts, const uint32_t* offs, const double* origins,
                          const double* quats, double* poses4, const uint32_t* max_iterations, const char* strategy, double eps1, const char* weight,
                          double weight_param, double* cov9, uint32_t* iterations, double* errors)
{
    try {
        const DynamicDistanceMap* dm = h->s->getDistanceMap();
        const DynamicDistanceMap* dm2 = other ? other->s->getDistanceMap() : dm;
        if (!dm || !dm2) return -1;
        std::vector<std::unique_ptr<MatchSurface2D>> owned;
        std::vector<MatchSurface2D*> problems;
        for (uint32_t b = 0; b < num_problems; ++b) {
            owned.emplace_back(new MatchSurface2D((b & 1u) ? dm2 : dm, cloud_of(pts + 3 * (size_t)offs[b], offs[b + 1] - offs[b], origins ? origins + 3 * (size_t)b : nullptr,
                                                                                quats ? quats + 4 * (size_t)b : nullptr), SE2d::fromArray(poses4 + 4 * (size_t)b)));
            problems.push_back(owned.back().get());
        }
        Solver::Options so;
        if (!solver_options_of(strategy, weight, weight_param, eps1, 100, &so)) { h->error = "unknown strategy or weight"; return -3; }
        std::vector<MatrixXd> covs;
        std::vector<uint32_t> its;
        std::vector<double> errs;
        try {
            if (max_iterations) SolveBatch(so, problems, std::vector<uint32_t>(max_iterations, max_iterations + num_problems), &covs, &its, &errs);
            else SolveBatch(so, problems, &covs, &its, &errs);
        } catch (const std::invalid_argument& e) { h->error = e.what(); return -3; }
        for (uint32_t b = 0; b < num_problems; ++b) {
            problems[b]->getState().toArray(poses4 + 4 * (size_t)b);
            if (cov9) for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) cov9[9 * (size_t)b + 3 * r + c] = covs[b](r, c);
            if (iterations) iterations[b] = its[b];
            if (errors) errors[b] = errs[b];
        }
        return 0;
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}

namespace {
CorrelativeSearch2D::Options correlative_options(double linear_step, double angular_step, uint32_t point_step, uint32_t tile, uint32_t max_candidates,
                                                 bool refine, uint32_t refine_iterations)
{
    CorrelativeSearch2D::Options o;
    o.linear_step = linear_step; o.angular_step = angular_step; o.point_step = point_step; o.tile = tile; o.max_candidates = max_candidates;
    o.refine = refine; o.refine_iterations = refine_iterations;
    return o;
}
uint32_t write_candidates(const std::vector<CorrelativeSearch2D::Candidate>& c, uint32_t cap, double* coarse4, uint32_t* scores, double* poses4, double* rmse,
                          uint32_t* iterations)
{
    for (uint32_t i = 0; i < c.size() && i < cap; ++i) {
        if (coarse4) c[i].coarse.state.toArray(coarse4 + 4 * (size_t)i);
        if (poses4) c[i].pose.state.toArray(poses4 + 4 * (size_t)i);
        if (scores) scores[i] = c[i].score;
        if (rmse) rmse[i] = c[i].rmse;
        if (iterations) iterations[i] = c[i].iterations;
    }
    return (uint32_t)c.size();
}
}

int lama_slam_correlative_search(lama_slam* h, const double* pts, uint32_t n, const double* o, const double* q, const double* box4, double linear_step,
                                 double angular_step, uint32_t point_step, uint32_t tile, uint32_t max_candidates, int refine, uint32_t refine_iterations,
                                 uint32_t cap, double* coarse4, uint32_t* scores, double* poses4, double* rmse, uint32_t* iterations, uint32_t* lattice6,
                                 uint32_t* num_out)
{
    try {
        const DynamicDistanceMap* dm = h->s->getDistanceMap();
        if (!dm) return -1;
        const CorrelativeSearch2D cs(correlative_options(linear_step, angular_step, point_step, tile, max_candidates, refine != 0, refine_iterations));
        const Vector2d bmin(box4[0], box4[1]), bmax(box4[2], box4[3]);
        std::vector<CorrelativeSearch2D::Candidate> c;
        try {
            if (lattice6) {
                const CorrelativeSearch2D::Lattice L = cs.lattice(dm->resolution, n, bmin, bmax);
                lattice6[0] = L.cell_step; lattice6[1] = L.nx; lattice6[2] = L.ny; lattice6[3] = L.num_headings; lattice6[4] = L.point_step; lattice6[5] = L.tile;
            }
            c = cs.search(dm, cloud_of(pts, n, o, q), bmin, bmax);
        } catch (const std::invalid_argument& e) { h->error = e.what(); return -3; }
        const uint32_t count = write_candidates(c, cap, coarse4, scores, poses4, rmse, iterations);
        if (num_out) *num_out = count;
        return 0;
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}

int lama_slam_view_distance_points(lama_slam* h, uint64_t n, const double* xy, double* out)
{
    try {
        const DynamicDistanceMap* m = h->s->getDistanceMap();
        if (!m) return -1;
        for (uint64_t i = 0; i < n; ++i) {
            Vector3d g;
            out[3 * i] = m->distance(Vector3d(xy[2 * i], xy[2 * i + 1], 0.0), &g);
            out[3 * i + 1] = g[0]; out[3 * i + 2] = g[1];
        }
        return 0;
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}


// ------------------------------------------------------------------ Loc2D
struct lama_loc {
    Loc2D l;
    std::string error;
};

lama_loc* lama_loc_create(double trans_thresh, double rot_thresh, double l2_max, double resolution, uint32_t max_iter,
                          int32_t gpu_device, char* err, int errcap)
{
    auto* h = new lama_loc;
    try {
        Loc2D::Options o;
        o.trans_thresh = trans_thresh; o.rot_thresh = rot_thresh; o.l2_max = l2_max; o.resolution = resolution; o.max_iter = max_iter;
        o.gpu_device = gpu_device;
        h->l.Init(o);
        return h;
    } catch (const std::exception& e) {
        if (err && errcap > 0) { std::strncpy(err, e.what(), (size_t)errcap - 1); err[errcap - 1] = 0; }
        delete h;
        return nullptr;
    }
}
void lama_loc_destroy(lama_loc* l) { delete l; }
const char* lama_loc_last_error(const lama_loc* l) { return l ? l->error.c_str() : "null handle"; }
const char* lama_loc_engine_origin(const lama_loc* l) { return (l && l->l.engine()) ? l->l.engine()->origin.c_str() : ""; }
int lama_loc_set_obstacles_world(lama_loc* h, const double* xy, uint32_t n)
{
    try {
        for (uint32_t i = 0; i < n; ++i) {
            const Vector3ui c = h->l.distance_map->w2m(Vector3d(xy[2 * i], xy[2 * i + 1], 0.0));
            h->l.occupancy_map->setOccupied(c);
            h->l.distance_map->addObstacle(c);
        }
        h->l.distance_map->update();
        return 0;
    } catch (const std::exception& e) { h->error = e.what(); return -1; }
}
void* lama_loc_device_context(const lama_loc* h) { return h ? (void*)h->l.deviceContext() : nullptr; }
int lama_loc_write_distance_map(lama_loc* h, const char* filename)
{
    try { return h->l.distance_map->write(filename) ? 0 : -1; } catch (const std::exception& e) { h->error = e.what(); return -1; }
}
int lama_loc_read_distance_map(lama_loc* h, const char* filename)
{
    try {
        if (!h->l.distance_map->read(filename)) { h->error = std::string("cannot read ") + filename; return -1; }
        return 0;
    } catch (const std::exception& e) { h->error = e.what(); return -1; }
}
void lama_loc_set_pose(lama_loc* h, double x, double y, double yaw) { h->l.setPose(Pose2D(x, y, yaw)); }
int lama_loc_get_pose(const lama_loc* h, double* pose4) { h->l.getPose().state.toArray(pose4); return 0; }
int lama_loc_update(lama_loc* h, const double* pts, uint32_t n, const double* origin3, const double* quat, const double* odom_xyr, double ts, int force)
{
    try {
        return h->l.update(make_cloud(pts, n, origin3, quat), Pose2D(odom_xyr[0], odom_xyr[1], odom_xyr[2]), ts, force != 0) ? 1 : 0;
    } catch (const std::exception& e) { h->error = e.what(); return -1; }
}
int lama_loc_covar(const lama_loc* h, double* out9)      // row-major, whatever lama::Matrix3d is (Eigen's is column-major)
{
    const lama::Matrix3d& c = h->l.getCovar();
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) out9[3 * r + k] = c(r, k);
    return 0;
}
double lama_loc_rmse(const lama_loc* h) { return h->l.getRMSE(); }
uint32_t lama_loc_iterations(const lama_loc* h) { return h->l.getLastIterations(); }

lama_loc* lama_loc_create2(double trans_thresh, double rot_thresh, double l2_max, double resolution, uint32_t max_iter,
                           uint32_t gloc_particles, uint32_t gloc_iters, double gloc_thresh, double cov_blend,
                           int32_t gpu_device, char* err, int errcap)
{
    auto* h = new lama_loc;
    try {
        Loc2D::Options o;
        o.trans_thresh = trans_thresh; o.rot_thresh = rot_thresh; o.l2_max = l2_max; o.resolution = resolution; o.max_iter = max_iter;
        o.gloc_particles = gloc_particles; o.gloc_iters = gloc_iters; o.gloc_thresh = gloc_thresh; o.cov_blend = cov_blend;
        o.gpu_device = gpu_device;
        h->l.Init(o);
        return h;
    } catch (const std::exception& e) {
        if (err && errcap > 0) { std::strncpy(err, e.what(), (size_t)errcap - 1); err[errcap - 1] = 0; }
        delete h;
        return nullptr;
    }
}
lama_loc* lama_loc_create3(double trans_thresh, double rot_thresh, double l2_max, double resolution, uint32_t max_iter,
                           uint32_t gloc_particles, uint32_t gloc_iters, double gloc_thresh, double cov_blend,
                           const char* strategy, int32_t gpu_device, char* err, int errcap)
{
    auto* h = new lama_loc;
    try {
        Loc2D::Options o;
        o.trans_thresh = trans_thresh; o.rot_thresh = rot_thresh; o.l2_max = l2_max; o.resolution = resolution; o.max_iter = max_iter;
        o.gloc_particles = gloc_particles; o.gloc_iters = gloc_iters; o.gloc_thresh = gloc_thresh; o.cov_blend = cov_blend;
        o.strategy = strategy ? strategy : "gn";
        o.gpu_device = gpu_device;
        h->l.Init(o);
        return h;
    } catch (const std::exception& e) {
        if (err && errcap > 0) { std::strncpy(err, e.what(), (size_t)errcap - 1); err[errcap - 1] = 0; }
        delete h;
        return nullptr;
    }
}
int lama_loc_occ_set_cells(lama_loc* h, const uint32_t* cells_xy, uint32_t n, int state)
{
    for (uint32_t i = 0; i < n; ++i) {
        const Vector3ui c(cells_xy[2 * i], cells_xy[2 * i + 1], 0);
        if (state < 0) h->l.occupancy_map->setFree(c); else if (state > 0) h->l.occupancy_map->setOccupied(c); else h->l.occupancy_map->setUnknown(c);
    }
    return 0;
}
int lama_loc_occ_bounds(const lama_loc* h, double* out6)
{
    Vector3d a, b;
    h->l.occupancy_map->bounds(a, b);
    for (int i = 0; i < 3; ++i) { out6[i] = a[i]; out6[3 + i] = b[i]; }
    return 0;
}
void lama_loc_trigger_global_localization(lama_loc* h) { h->l.triggerGlobalLocalization(); }
int lama_loc_global_localization_active(const lama_loc* h) { return h->l.globalLocalizationIsActive() ? 1 : 0; }
uint32_t lama_loc_gloc_candidates(const lama_loc* h, double* poses4, double* errors, uint32_t cap)
{
    const uint32_t n = (uint32_t)h->l.lastGlocErrors().size();
    for (uint32_t i = 0; i < n && i < cap; ++i) {
        for (int k = 0; k < 4; ++k) poses4[4 * i + k] = h->l.lastGlocPoses()[4 * i + k];
        errors[i] = h->l.lastGlocErrors()[i];
    }
    return n;
}
uint32_t lama_loc_sampling_likelihoods(const lama_loc* h, double* out, uint32_t cap)
{
    const uint32_t n = (uint32_t)h->l.lastSamplingLikelihoods().size();
    for (uint32_t i = 0; i < n && i < cap; ++i) out[i] = h->l.lastSamplingLikelihoods()[i];
    return n;
}
int lama_loc_relocalize(lama_loc* h, const double* pts, uint32_t n, const double* origin3, const double* quat, double linear_step, double angular_step,
                        uint32_t point_step, uint32_t tile, uint32_t max_candidates, uint32_t refine_iterations)
{
    try {
        return h->l.relocalize(make_cloud(pts, n, origin3, quat), correlative_options(linear_step, angular_step, point_step, tile, max_candidates, true, refine_iterations)) ? 1 : 0;
    } catch (const std::exception& e) { h->error = e.what(); return -1; }
}
uint32_t lama_loc_relocalize_candidates(const lama_loc* h, uint32_t cap, double* coarse4, uint32_t* scores, double* poses4, double* rmse, uint32_t* iterations)
{
    return write_candidates(h->l.lastRelocalizeCandidates(), cap, coarse4, scores, poses4, rmse, iterations);
}
// ------------------------------------------------------------------ LidarOdometry2D
struct lama_lo {
    std::unique_ptr<LidarOdometry2D> l;
    std::string error;
};
lama_lo* lama_lo_create(double resolution, uint32_t max_iter, int32_t gpu_device, char* err, int errcap)
{
    auto* h = new lama_lo;
    try {
        LidarOdometry2D::Options o;
        o.resolution = resolution; o.max_iter = max_iter; o.gpu_device = gpu_device;
        h->l.reset(new LidarOdometry2D(o));
        return h;
    } catch (const std::exception& e) {
        if (err && errcap > 0) { std::strncpy(err, e.what(), (size_t)errcap - 1); err[errcap - 1] = 0; }
        delete h;
        return nullptr;
    }
}
void lama_lo_destroy(lama_lo* h) { delete h; }
const char* lama_lo_last_error(const lama_lo* h) { return h ? h->error.c_str() : "null handle"; }
const char* lama_lo_engine_origin(const lama_lo* h) { return (h && h->l->engine()) ? h->l->engine()->origin.c_str() : ""; }
int lama_lo_update(lama_lo* h, const double* pts, uint32_t n, const double* origin3, const double* quat, double ts)
{
    try {
        return h->l->update(make_cloud(pts, n, origin3, quat), ts) ? 1 : 0;
    } catch (const std::exception& e) { h->error = e.what(); return -1; }
}
int lama_lo_get_odom(const lama_lo* h, double* pose4) { h->l->odom.state.toArray(pose4); return 0; }
uint32_t lama_lo_iterations(const lama_lo* h) { return h->l->getLastIterations(); }
uint32_t lama_lo_deleted_patches(const lama_lo* h) { return h->l->getLastDeletedPatches(); }
void* lama_lo_device_context(const lama_lo* h) { return h->l->deviceContext(); }

static lama::sdm::HostMap host_map(int kind, double resolution, uint32_t max_sqdist, uint32_t n, const uint64_t* ids, const uint8_t* cells,
                                    const uint64_t* masks)
{
    lama::sdm::HostMap m;
    m.kind = (lama::sdm::MapKind)kind; m.resolution = resolution; m.max_sqdist = max_sqdist;
    const size_t pb = (size_t)1024 * m.cellSize();
    m.ids.assign(ids, ids + n);
    m.cells.assign(cells, cells + (size_t)n * pb);
    m.masks.assign(masks, masks + (size_t)n * 16);
    return m;
}
int lama_sdm_write(const char* file, int kind, double resolution, uint32_t max_sqdist, uint32_t n, const uint64_t* ids, const uint8_t* cells,
                   const uint64_t* masks)
{
    return lama::sdm::write(host_map(kind, resolution, max_sqdist, n, ids, cells, masks), file) ? 0 : -1;
}
int lama_sdm_read(const char* file, int* kind, double* resolution, uint32_t* max_sqdist, uint32_t cap, uint64_t* ids, uint8_t* cells,
                  uint64_t* masks, uint32_t* n)
{
    lama::sdm::HostMap m;
    if (!lama::sdm::read(m, file)) return -1;
    if (kind) *kind = (int)m.kind;
    if (resolution) *resolution = m.resolution;
    if (max_sqdist) *max_sqdist = m.max_sqdist;
    if (n) *n = (uint32_t)m.numPatches();
    if (cap >= m.numPatches() && ids && cells && masks) {
        std::memcpy(ids, m.ids.data(), m.ids.size() * 8);
        std::memcpy(cells, m.cells.data(), m.cells.size());
        std::memcpy(masks, m.masks.data(), m.masks.size() * 8);
    }
    return 0;
}
int lama_sdm_image(int kind, double resolution, uint32_t max_sqdist, uint32_t n, const uint64_t* ids, const uint8_t* cells,
                   const uint64_t* masks, uint32_t* width, uint32_t* height, uint8_t* out, uint64_t cap)
{
    lama::sdm::Image im;
    lama::sdm::build_image(host_map(kind, resolution, max_sqdist, n, ids, cells, masks), im);
    if (width) *width = im.width;
    if (height) *height = im.height;
    if (out && cap >= im.data.size()) std::memcpy(out, im.data.data(), im.data.size());
    return 0;
}
int lama_sdm_export_png(int kind, double resolution, uint32_t max_sqdist, uint32_t n, const uint64_t* ids, const uint8_t* cells,
                        const uint64_t* masks, const char* file)
{
    return lama::sdm::export_to_png(host_map(kind, resolution, max_sqdist, n, ids, cells, masks), file) ? 0 : -1;
}
static thread_local lama::sdm::HostMap g_dm_build;
int64_t lama_dm_build(const uint32_t* cells_xy, uint64_t n, uint32_t max_sqdist, uint32_t* processed)
{
    uint32_t done = 0;
    g_dm_build = lama::sdm::HostMap();
    g_dm_build.kind = lama::sdm::kDistanceMap; g_dm_build.max_sqdist = max_sqdist;
    try {
        if (!cells_xy || !lama::detail::build_distance_map(cells_xy, (size_t)n, max_sqdist, g_dm_build, done)) return -1;
    } catch (...) { return -1; }
    if (processed) *processed = done;
    return (int64_t)g_dm_build.numPatches();
}
int lama_dm_build_fetch(uint64_t* ids, uint8_t* cells, uint64_t* masks)
{
    if (!ids || !cells || !masks) return -1;
    std::memcpy(ids, g_dm_build.ids.data(), g_dm_build.ids.size() * 8);
    std::memcpy(cells, g_dm_build.cells.data(), g_dm_build.cells.size());
    std::memcpy(masks, g_dm_build.masks.data(), g_dm_build.masks.size() * 8);
    return 0;
}
void lama_random_set_seed(uint32_t seed) { lama::random::setSeed(seed); }
double lama_random_uniform(void) { return lama::random::uniform(); }

int lama_pgo_optimize(const double* nodes4, uint32_t n, const int32_t* edge_from, const int32_t* edge_to, const double* edge4, uint32_t ne,
                      const int32_t* fixed_idx, const double* fixed4, uint32_t nf, int32_t device, double* out4, lama_pgo_report* report,
                      int8_t* trace, uint32_t trace_cap, char* err, int errcap)
{
    try {
        SimplePGO p;
        p.device = device;
        for (uint32_t i = 0; i < n; ++i) p.node_list.push_back(Pose2D(SE2d::fromArray(nodes4 + 4 * i)));
        for (uint32_t k = 0; k < ne; ++k) p.edge_list.push_back({edge_from[k], {edge_to[k], Pose2D(SE2d::fromArray(edge4 + 4 * k))}});
        for (uint32_t k = 0; k < nf; ++k) p.fixed_list.push_back({fixed_idx[k], Pose2D(SE2d::fromArray(fixed4 + 4 * k))});
        const bool ok = p.optimize();
        if (out4) for (uint32_t i = 0; i < n; ++i) p.node_list[i].state.toArray(out4 + 4 * i);
        if (report) {
            const SimplePGO::Report& r = p.report;
            report->status = r.status; report->iterations = r.iterations; report->tries = r.tries;
            report->initial_error = r.initial_error; report->final_error = r.final_error; report->nnz_L = r.nnz_L;
            report->ms_device_linearize = r.ms_device_linearize; report->ms_device_try = r.ms_device_try;
            report->ms_analyze = r.ms_analyze; report->ms_factorize = r.ms_factorize; report->ms_total = r.ms_total;
        }
        if (trace) for (size_t q = 0; q < p.report.trace.size() && q < trace_cap; ++q) trace[q] = p.report.trace[q];
        return ok ? 1 : 0;
    } catch (const std::exception& e) {
        if (err && errcap > 0) { std::strncpy(err, e.what(), (size_t)errcap - 1); err[errcap - 1] = 0; }
        return -1;
    }
}

// lama_pgo_report2 from the class's report: at most the bytes the caller's struct has
static void fill_report2(const SimplePGO::Report& r, lama_pgo_report2* report)
{
    lama_pgo_report2 f;
    std::memset(&f, 0, sizeof(f));
    f.struct_bytes = report->struct_bytes;
    f.status = r.status; f.iterations = r.iterations; f.tries = r.tries;
    f.initial_error = r.initial_error; f.final_error = r.final_error; f.nnz_L = r.nnz_L;
    f.ms_device_linearize = r.ms_device_linearize; f.ms_device_try = r.ms_device_try;
    f.ms_analyze = r.ms_analyze; f.ms_factorize = r.ms_factorize; f.ms_total = r.ms_total;
    f.pcg_iterations = r.pcg_iterations; f.pcg_max_iterations_seen = r.pcg_max_iterations_seen;
    f.pcg_fallbacks = r.pcg_fallbacks; f.ms_device_solve = r.ms_device_solve;
    std::memcpy(report, &f, std::min<size_t>(report->struct_bytes, sizeof(f)));
}

int lama_pgo_optimize_with(const double* nodes4, uint32_t n, const int32_t* edge_from, const int32_t* edge_to, const double* edge4,
                           uint32_t ne, const int32_t* fixed_idx, const double* fixed4, uint32_t nf, const lama_pgo_options* options,
                           double* out4, lama_pgo_report2* report, int8_t* trace, uint32_t trace_cap, char* err, int errcap)
{
    try {
        lama_pgo_options o;
        std::memset(&o, 0, sizeof(o));
        o.pcg_rel_tol = SimplePGO().pcg_rel_tol;
        if (options) std::memcpy(&o, options, std::min<size_t>(options->struct_bytes, sizeof(o)));
        SimplePGO p;
        p.device = o.device;
        if (o.linear_solver != SimplePGO::HostLDLT && o.linear_solver != SimplePGO::DevicePCG)
            throw std::invalid_argument("lama_pgo_optimize_with: linear_solver must be 0 (host LDL^T) or 1 (device PCG)");
        p.linear_solver = (SimplePGO::LinearSolver)o.linear_solver;
        p.pcg_rel_tol = o.pcg_rel_tol;
        p.pcg_max_iterations = o.pcg_max_iterations;
        for (uint32_t i = 0; i < n; ++i) p.node_list.push_back(Pose2D(SE2d::fromArray(nodes4 + 4 * i)));
        for (uint32_t k = 0; k < ne; ++k) p.edge_list.push_back({edge_from[k], {edge_to[k], Pose2D(SE2d::fromArray(edge4 + 4 * k))}});
        for (uint32_t k = 0; k < nf; ++k) p.fixed_list.push_back({fixed_idx[k], Pose2D(SE2d::fromArray(fixed4 + 4 * k))});
        const bool ok = p.optimize();
        if (out4) for (uint32_t i = 0; i < n; ++i) p.node_list[i].state.toArray(out4 + 4 * i);
        if (report) {
            fill_report2(p.report, report);
        }
        if (trace) for (size_t q = 0; q < p.report.trace.size() && q < trace_cap; ++q) trace[q] = p.report.trace[q];
        return ok ? 1 : 0;
    } catch (const std::exception& e) {
        if (err && errcap > 0) { std::strncpy(err, e.what(), (size_t)errcap - 1); err[errcap - 1] = 0; }
        return -1;
    }
}

int lama_pose_graph_optimize(const double* nodes4, uint32_t n, const int32_t* fi, const int32_t* fj, const double* meas4,
                             const double* sigmas3, const int32_t* loss_kind, const double* loss_param, uint32_t nf,
                             const lama_pgo_options* options, double* out4, double* weights, lama_pgo_report2* report, int8_t* trace,
                             uint32_t trace_cap, char* err, int errcap)
{
    try {
        lama_pgo_options o;
        std::memset(&o, 0, sizeof(o));
        o.pcg_rel_tol = PoseGraph2D().pcg_rel_tol;
        if (options) std::memcpy(&o, options, std::min<size_t>(options->struct_bytes, sizeof(o)));
        if (o.linear_solver != PoseGraph2D::HostLDLT && o.linear_solver != PoseGraph2D::DevicePCG)
            throw std::invalid_argument("lama_pose_graph_optimize: linear_solver must be 0 (host LDL^T) or 1 (device PCG)");
        PoseGraph2D p;
        p.device = o.device;
        p.linear_solver = (PoseGraph2D::LinearSolver)o.linear_solver;
        p.pcg_rel_tol = o.pcg_rel_tol;
        p.pcg_max_iterations = o.pcg_max_iterations;
        for (uint32_t i = 0; i < n; ++i) p.addNode(Pose2D(SE2d::fromArray(nodes4 + 4 * i)));
        for (uint32_t k = 0; k < nf; ++k) {
            PoseGraph2D::Loss loss;
            if (loss_kind) { loss.kind = loss_kind[k]; loss.param = loss_param ? loss_param[k] : 0.0; }
            const Vector3d sig(sigmas3[3 * k], sigmas3[3 * k + 1], sigmas3[3 * k + 2]);
            if (fj[k] == -1) p.addPrior(fi[k], Pose2D(SE2d::fromArray(meas4 + 4 * k)), sig, loss);
            else p.addBetween(fi[k], fj[k], Pose2D(SE2d::fromArray(meas4 + 4 * k)), sig, loss);
        }
        const bool ok = p.optimize();
        if (out4) for (uint32_t i = 0; i < n; ++i) p.nodes[i].state.toArray(out4 + 4 * i);
        if (weights) std::copy(p.weights.begin(), p.weights.end(), weights);
        if (report) fill_report2(p.report, report);
        if (trace) for (size_t q = 0; q < p.report.trace.size() && q < trace_cap; ++q) trace[q] = p.report.trace[q];
        return ok ? 1 : 0;
    } catch (const std::exception& e) {
        if (err && errcap > 0) { std::strncpy(err, e.what(), (size_t)errcap - 1); err[errcap - 1] = 0; }
        return -1;
    }
}

// ---- lama::MapBuilder2D ----
struct lama_mapbuilder {
    std::unique_ptr<MapBuilder2D> b;
    std::string error, origin;
};

void lama_mapbuilder_default_options(lama_mapbuilder_options* o)
{
    MapBuilder2D::Options d;
    o->resolution = d.resolution; o->l2_max = d.l2_max; o->patch_size = d.patch_size; o->full = d.full ? 1 : 0; o->prune = d.prune ? 1 : 0;
    o->gpu_device = d.gpu_device; o->window_patches = 0; o->occ_patch_capacity = 0; o->dm_patch_capacity = 0;
}

lama_mapbuilder* lama_mapbuilder_create(const lama_mapbuilder_options* o, char* err, int errcap)
{
    auto* h = new lama_mapbuilder;
    try {
        MapBuilder2D::Options p;
        p.resolution = o->resolution; p.l2_max = o->l2_max; p.patch_size = o->patch_size; p.full = o->full != 0; p.prune = o->prune != 0;
        p.gpu_device = o->gpu_device; p.window_patches = o->window_patches; p.occ_patch_capacity = o->occ_patch_capacity; p.dm_patch_capacity = o->dm_patch_capacity;
        h->b.reset(new MapBuilder2D(p));
        h->origin = h->b->engine()->origin;
        return h;
    } catch (const std::exception& e) {
        if (err && errcap > 0) { std::strncpy(err, e.what(), (size_t)errcap - 1); err[errcap - 1] = 0; }
        delete h;
        return nullptr;
    }
}
void lama_mapbuilder_destroy(lama_mapbuilder* b) { delete b; }
const char* lama_mapbuilder_last_error(const lama_mapbuilder* b) { return b ? b->error.c_str() : "null handle"; }
const char* lama_mapbuilder_engine_origin(const lama_mapbuilder* b) { return b ? b->origin.c_str() : ""; }
void* lama_mapbuilder_device_context(const lama_mapbuilder* b) { return (void*)b->b->deviceContext(); }
int64_t lama_mapbuilder_add(lama_mapbuilder* h, const double* pts, uint32_t n, const double* o, const double* q, const double* pose4)
{
    try {
        return (int64_t)h->b->add(cloud_of(pts, n, o, q), Pose2D(SE2d::fromArray(pose4)));
    } catch (const std::exception& e) { h->error = e.what(); return -1; }
}
int lama_mapbuilder_set_pose(lama_mapbuilder* h, uint64_t key, const double* pose4)
{
    try { h->b->setPose((size_t)key, Pose2D(SE2d::fromArray(pose4))); return 0; } catch (const std::exception& e) { h->error = e.what(); return -1; }
}
int lama_mapbuilder_set_poses(lama_mapbuilder* h, const double* poses4, uint64_t n)
{
    try {
        std::vector<Pose2D> v;
        for (uint64_t i = 0; i < n; ++i) v.push_back(Pose2D(SE2d::fromArray(poses4 + 4 * i)));
        h->b->setPoses(v);
        return 0;
    } catch (const std::exception& e) { h->error = e.what(); return -1; }
}
int lama_mapbuilder_build(lama_mapbuilder* h) { try { h->b->build(); return 0; } catch (const std::exception& e) { h->error = e.what(); return -1; } }
int lama_mapbuilder_reset(lama_mapbuilder* h) { try { h->b->reset(); return 0; } catch (const std::exception& e) { h->error = e.what(); return -1; } }
int64_t lama_mapbuilder_occupied_cells(const lama_mapbuilder* h, uint32_t* xy_out, uint64_t cap)
{
    const std::vector<uint32_t>& c = h->b->occupiedCells();
    const uint64_t n = c.size() / 2;
    if (xy_out) std::memcpy(xy_out, c.data(), sizeof(uint32_t) * 2 * (size_t)(n < cap ? n : cap));
    return (int64_t)n;
}
int lama_mapbuilder_timing(const lama_mapbuilder* h, double* ms3)
{
    const MapBuilder2D::Timing t = h->b->lastTiming();
    ms3[0] = t.integrate_ms; ms3[1] = t.occupied_ms; ms3[2] = t.distance_ms;
    return 0;
}
int64_t lama_mapbuilder_view_cells(lama_mapbuilder* h, int which, uint32_t* xy_out, uint64_t cap)
{
    try {
        return which == 0 ? view_cells(h->b->getOccupancyMap(), xy_out, cap) : view_cells(h->b->getDistanceMap(), xy_out, cap);
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}
int lama_mapbuilder_match_solve(lama_mapbuilder* h, const double* pts, uint32_t n, const double* o, const double* q, double* pose4,
                                uint32_t max_iterations, uint32_t* iterations)
{
    try {
        const DynamicDistanceMap* dm = h->b->getDistanceMap();
        if (!dm) return -1;
        MatchSurface2D problem(dm, cloud_of(pts, n, o, q), SE2d::fromArray(pose4));
        Solver::Options so;
        so.max_iterations = max_iterations;
        so.strategy.reset(new GaussNewton);
        so.robust_cost.reset(new CauchyWeight(0.15));
        Solver solver(so);
        solver.solve(problem, nullptr);
        problem.getState().toArray(pose4);
        if (iterations) *iterations = solver.lastIterations();
        return 0;
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}

}   // extern "C"
// ---- dense grids (include/lama/sdm/grid.h) of the classes above ----
namespace {
thread_local std::vector<uint8_t> g_grid_data;              // the pixels of the last grid made on this thread (lama_grid_fetch)
lama::sdm::GridOptions grid_options(const lama_grid_options* o)
{
    lama::sdm::GridOptions g;
    if (o) {
        g.stride = o->stride; g.probability = o->probability != 0; g.whole_map = o->whole_map != 0;
        g.world_min = Vector2d(o->world_min[0], o->world_min[1]); g.world_max = Vector2d(o->world_max[0], o->world_max[1]);
    }
    return g;
}
template <class T>
void grid_keep(const lama::sdm::GridHeader& g, double max_distance, const std::vector<T>& pixels, lama_grid* out)
{
    out->x0 = g.x0; out->y0 = g.y0; out->width = g.width; out->height = g.height; out->stride = g.stride; out->element_bytes = (uint32_t)sizeof(T);
    out->resolution = g.resolution; out->cell_size = g.cell_size; out->max_distance = max_distance;
    for (int k = 0; k < 3; ++k) out->origin[k] = g.origin[k];
    g_grid_data.resize(pixels.size() * sizeof(T));
    if (!pixels.empty()) std::memcpy(g_grid_data.data(), pixels.data(), g_grid_data.size());
}
// 1: the grid was made (header in *out, pixels kept for lama_grid_fetch), 0: the object has no such map (yet / here), -2: failure
template <class H, class F>
int occupancy_grid_of(H* h, const lama_grid_options* o, lama_grid* out, F&& get)
{
    try {
        lama::sdm::OccupancyGrid g;
        if (!get(g, grid_options(o))) return 0;
        grid_keep(g, 0.0, g.data, out);
        return 1;
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}
template <class H, class F>
int distance_grid_of(H* h, const lama_grid_options* o, lama_grid* out, F&& get)
{
    try {
        lama::sdm::DistanceGrid g;
        if (!get(g, grid_options(o))) return 0;
        grid_keep(g, g.max_distance, g.sqdist, out);
        return 1;
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}
}
extern "C" {
void lama_grid_default_options(lama_grid_options* o)
{
    const lama::sdm::GridOptions d;
    o->stride = d.stride; o->probability = d.probability ? 1 : 0; o->whole_map = d.whole_map ? 1 : 0;
    o->world_min[0] = o->world_min[1] = o->world_max[0] = o->world_max[1] = 0.0;
}
int64_t lama_grid_fetch(void* out, uint64_t cap_bytes)
{
    if (out && cap_bytes >= g_grid_data.size() && !g_grid_data.empty()) std::memcpy(out, g_grid_data.data(), g_grid_data.size());
    return (int64_t)g_grid_data.size();
}
int lama_slam_occupancy_grid(lama_slam* h, const lama_grid_options* o, lama_grid* out)
{ return occupancy_grid_of(h, o, out, [h](lama::sdm::OccupancyGrid& g, const lama::sdm::GridOptions& go) { return h->s->getOccupancyGrid(g, go); }); }
int lama_slam_distance_grid(lama_slam* h, const lama_grid_options* o, lama_grid* out)
{ return distance_grid_of(h, o, out, [h](lama::sdm::DistanceGrid& g, const lama::sdm::GridOptions& go) { return h->s->getDistanceGrid(g, go); }); }
int lama_pf_occupancy_grid(lama_pf* h, int64_t particle, const lama_grid_options* o, lama_grid* out)
{
    return occupancy_grid_of(h, o, out, [h, particle](lama::sdm::OccupancyGrid& g, const lama::sdm::GridOptions& go) {
        return particle < 0 ? h->pf->getOccupancyGrid(g, go) : h->pf->getParticleOccupancyGrid((size_t)particle, g, go); });
}
int lama_pf_distance_grid(lama_pf* h, int64_t particle, const lama_grid_options* o, lama_grid* out)
{
    return distance_grid_of(h, o, out, [h, particle](lama::sdm::DistanceGrid& g, const lama::sdm::GridOptions& go) {
        return particle < 0 ? h->pf->getDistanceGrid(g, go) : h->pf->getParticleDistanceGrid((size_t)particle, g, go); });
}
int lama_mapbuilder_occupancy_grid(lama_mapbuilder* h, const lama_grid_options* o, lama_grid* out)
{ return occupancy_grid_of(h, o, out, [h](lama::sdm::OccupancyGrid& g, const lama::sdm::GridOptions& go) { return h->b->getOccupancyGrid(g, go); }); }
int lama_mapbuilder_distance_grid(lama_mapbuilder* h, const lama_grid_options* o, lama_grid* out)
{ return distance_grid_of(h, o, out, [h](lama::sdm::DistanceGrid& g, const lama::sdm::GridOptions& go) { return h->b->getDistanceGrid(g, go); }); }
int lama_lo_occupancy_grid(lama_lo* h, const lama_grid_options* o, lama_grid* out)
{ return occupancy_grid_of(h, o, out, [h](lama::sdm::OccupancyGrid& g, const lama::sdm::GridOptions& go) { return h->l->getOccupancyGrid(g, go); }); }
int lama_lo_distance_grid(lama_lo* h, const lama_grid_options* o, lama_grid* out)
{ return distance_grid_of(h, o, out, [h](lama::sdm::DistanceGrid& g, const lama::sdm::GridOptions& go) { return h->l->getDistanceGrid(g, go); }); }
int lama_loc_distance_grid(lama_loc* h, const lama_grid_options* o, lama_grid* out)
{ return distance_grid_of(h, o, out, [h](lama::sdm::DistanceGrid& g, const lama::sdm::GridOptions& go) { return h->l.getDistanceGrid(g, go); }); }
}   // extern "C"
// ---- frontiers (include/lama/sdm/frontier.h) of the classes above ----
namespace {
thread_local std::vector<lama_frontier> g_frontier_records;  // the result of the last frontier call on this thread (lama_frontiers_fetch)
thread_local std::vector<uint32_t> g_frontier_labels;
// 1: made (box and counts in *out, records and labels kept), 0: the object has no map (yet / here), -2: failure
template <class H, class F>
int frontiers_of(H* h, const lama_frontier_options* o, lama_frontier_set* out, F&& get)
{
    try {
        lama::sdm::FrontierOptions fo;
        if (o) {
            fo.stride = o->stride; fo.whole_map = o->whole_map != 0; fo.min_pixels = o->min_pixels; fo.max_frontiers = o->max_frontiers; fo.labels = o->labels != 0;
            fo.world_min = Vector2d(o->world_min[0], o->world_min[1]); fo.world_max = Vector2d(o->world_max[0], o->world_max[1]);
        }
        lama::sdm::FrontierSet s;
        if (!get(s, fo)) return 0;
        out->x0 = s.x0; out->y0 = s.y0; out->width = s.width; out->height = s.height; out->stride = s.stride; out->count = (uint32_t)s.frontiers.size();
        out->resolution = s.resolution; out->cell_size = s.cell_size;
        for (int k = 0; k < 3; ++k) out->origin[k] = s.origin[k];
        out->frontier_pixels = s.frontier_pixels; out->clusters = s.clusters;
        g_frontier_records.resize(s.frontiers.size());
        for (size_t k = 0; k < s.frontiers.size(); ++k) {
            const lama::sdm::Frontier& f = s.frontiers[k];
            g_frontier_records[k] = lama_frontier{f.label, f.pixels, f.min_i, f.min_j, f.max_i, f.max_j, f.sum_i, f.sum_j,
                                                  {f.centroid[0], f.centroid[1]}, {f.seed[0], f.seed[1]}};
        }
        g_frontier_labels.swap(s.labels);
        return 1;
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}
}
extern "C" {
void lama_frontier_default_options(lama_frontier_options* o)
{
    const lama::sdm::FrontierOptions d;
    o->stride = d.stride; o->whole_map = d.whole_map ? 1 : 0; o->min_pixels = d.min_pixels; o->max_frontiers = d.max_frontiers; o->labels = d.labels ? 1 : 0;
    o->world_min[0] = o->world_min[1] = o->world_max[0] = o->world_max[1] = 0.0;
}
int64_t lama_frontiers_fetch(lama_frontier* records, uint64_t cap_records, uint32_t* labels, uint64_t cap_labels)
{
    if (records && cap_records >= g_frontier_records.size() && !g_frontier_records.empty())
        std::memcpy(records, g_frontier_records.data(), g_frontier_records.size() * sizeof(lama_frontier));
    if (labels && cap_labels >= g_frontier_labels.size() && !g_frontier_labels.empty())
        std::memcpy(labels, g_frontier_labels.data(), g_frontier_labels.size() * sizeof(uint32_t));
    return (int64_t)g_frontier_records.size();
}
int lama_slam_frontiers(lama_slam* h, const lama_frontier_options* o, lama_frontier_set* out)
{ return frontiers_of(h, o, out, [h](lama::sdm::FrontierSet& s, const lama::sdm::FrontierOptions& fo) { return h->s->getFrontiers(s, fo); }); }
int lama_pf_frontiers(lama_pf* h, int64_t particle, const lama_frontier_options* o, lama_frontier_set* out)
{
    return frontiers_of(h, o, out, [h, particle](lama::sdm::FrontierSet& s, const lama::sdm::FrontierOptions& fo) {
        return particle < 0 ? h->pf->getFrontiers(s, fo) : h->pf->getParticleFrontiers((size_t)particle, s, fo); });
}
int lama_mapbuilder_frontiers(lama_mapbuilder* h, const lama_frontier_options* o, lama_frontier_set* out)
{ return frontiers_of(h, o, out, [h](lama::sdm::FrontierSet& s, const lama::sdm::FrontierOptions& fo) { return h->b->getFrontiers(s, fo); }); }
int lama_lo_frontiers(lama_lo* h, const lama_frontier_options* o, lama_frontier_set* out)
{ return frontiers_of(h, o, out, [h](lama::sdm::FrontierSet& s, const lama::sdm::FrontierOptions& fo) { return h->l->getFrontiers(s, fo); }); }
}   // extern "C"
// ---- routes (include/lama/sdm/travel.h) of the classes above ----
namespace {
thread_local std::vector<lama_route> g_routes;               // the result of the last route call on this thread (lama_routes_fetch)
thread_local std::vector<double> g_route_points;
thread_local std::vector<uint32_t> g_route_field;
// 1: made (box and counts in *out, routes, points and field kept), 0: the object has no map (yet / here), -2: failure
template <class H, class F>
int routes_of(H* h, const double* from_xy, uint32_t n_from, const double* goals_xy, uint32_t n_goals, const lama_travel_options* o, lama_route_set* out, F&& plan)
{
    try {
        lama::sdm::TravelOptions to;
        if (o) {
            to.stride = o->stride; to.whole_map = o->whole_map != 0; to.robot_radius = o->robot_radius; to.preferred_clearance = o->preferred_clearance;
            to.near_factor = o->near_factor; to.goal_reach = o->goal_reach; to.max_path_points = o->max_path_points; to.field = o->field != 0;
            to.world_min = Vector2d(o->world_min[0], o->world_min[1]); to.world_max = Vector2d(o->world_max[0], o->world_max[1]);
        }
        std::vector<Vector2d> from(n_from), goals(n_goals);
        for (uint32_t k = 0; k < n_from; ++k) from[k] = Vector2d(from_xy[2 * k], from_xy[2 * k + 1]);
        for (uint32_t k = 0; k < n_goals; ++k) goals[k] = Vector2d(goals_xy[2 * k], goals_xy[2 * k + 1]);
        lama::sdm::RouteSet s;
        if (!plan(from, goals, s, to)) return 0;
        out->x0 = s.x0; out->y0 = s.y0; out->width = s.width; out->height = s.height; out->stride = s.stride; out->count = (uint32_t)s.routes.size();
        out->resolution = s.resolution; out->cell_size = s.cell_size;
        for (int k = 0; k < 3; ++k) out->origin[k] = s.origin[k];
        out->rounds = s.rounds; out->has_field = s.field.empty() ? 0u : 1u;
        g_routes.resize(s.routes.size());
        g_route_points.clear();
        for (size_t k = 0; k < s.routes.size(); ++k) {
            const lama::sdm::Route& r = s.routes[k];
            g_routes[k] = lama_route{r.status, r.pixel, r.cost, r.steps, r.length_m, (uint64_t)(g_route_points.size() / 2), (uint32_t)r.path.size(), 0u};
            for (const Vector2d& p : r.path) { g_route_points.push_back(p[0]); g_route_points.push_back(p[1]); }
        }
        out->path_points = (uint64_t)(g_route_points.size() / 2);
        g_route_field.swap(s.field);
        return 1;
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}
}
extern "C" {
void lama_travel_default_options(lama_travel_options* o)
{
    const lama::sdm::TravelOptions d;
    o->stride = d.stride; o->whole_map = d.whole_map ? 1 : 0; o->robot_radius = d.robot_radius; o->preferred_clearance = d.preferred_clearance;
    o->near_factor = d.near_factor; o->goal_reach = d.goal_reach; o->max_path_points = d.max_path_points; o->field = d.field ? 1 : 0;
    o->world_min[0] = o->world_min[1] = o->world_max[0] = o->world_max[1] = 0.0;
}
int64_t lama_routes_fetch(lama_route* routes, uint64_t cap_routes, double* path_xy, uint64_t cap_points, uint32_t* field, uint64_t cap_field)
{
    if (routes && cap_routes >= g_routes.size() && !g_routes.empty()) std::memcpy(routes, g_routes.data(), g_routes.size() * sizeof(lama_route));
    if (path_xy && 2 * cap_points >= g_route_points.size() && !g_route_points.empty()) std::memcpy(path_xy, g_route_points.data(), g_route_points.size() * sizeof(double));
    if (field && cap_field >= g_route_field.size() && !g_route_field.empty()) std::memcpy(field, g_route_field.data(), g_route_field.size() * sizeof(uint32_t));
    return (int64_t)g_routes.size();
}
#define LAMA_PLAN_ARGS const std::vector<Vector2d>& f, const std::vector<Vector2d>& g, lama::sdm::RouteSet& s, const lama::sdm::TravelOptions& to
int lama_slam_plan_routes(lama_slam* h, const double* from_xy, uint32_t n_from, const double* goals_xy, uint32_t n_goals, const lama_travel_options* o, lama_route_set* out)
{ return routes_of(h, from_xy, n_from, goals_xy, n_goals, o, out, [h](LAMA_PLAN_ARGS) { return h->s->planRoutes(f, g, s, to); }); }
int lama_pf_plan_routes(lama_pf* h, int64_t particle, const double* from_xy, uint32_t n_from, const double* goals_xy, uint32_t n_goals, const lama_travel_options* o,
                        lama_route_set* out)
{
    return routes_of(h, from_xy, n_from, goals_xy, n_goals, o, out, [h, particle](LAMA_PLAN_ARGS) {
        return particle < 0 ? h->pf->planRoutes(f, g, s, to) : h->pf->planParticleRoutes((size_t)particle, f, g, s, to); });
}
int lama_mapbuilder_plan_routes(lama_mapbuilder* h, const double* from_xy, uint32_t n_from, const double* goals_xy, uint32_t n_goals, const lama_travel_options* o,
                                lama_route_set* out)
{ return routes_of(h, from_xy, n_from, goals_xy, n_goals, o, out, [h](LAMA_PLAN_ARGS) { return h->b->planRoutes(f, g, s, to); }); }
int lama_lo_plan_routes(lama_lo* h, const double* from_xy, uint32_t n_from, const double* goals_xy, uint32_t n_goals, const lama_travel_options* o, lama_route_set* out)
{ return routes_of(h, from_xy, n_from, goals_xy, n_goals, o, out, [h](LAMA_PLAN_ARGS) { return h->l->planRoutes(f, g, s, to); }); }
int lama_loc_plan_routes(lama_loc* h, const double* from_xy, uint32_t n_from, const double* goals_xy, uint32_t n_goals, const lama_travel_options* o, lama_route_set* out)
{ return routes_of(h, from_xy, n_from, goals_xy, n_goals, o, out, [h](LAMA_PLAN_ARGS) { return h->l.planRoutes(f, g, s, to); }); }
#undef LAMA_PLAN_ARGS
}   // extern "C"
// ---- ray casts (include/lama/sdm/ray_cast.h) of the classes above ----
namespace {
// 1: cast (the arrays of *out that are not NULL are filled), 0: the object has no such map (yet / here), -2: failure
template <class H, class F>
int cast_rays_of(H* h, const double* poses4, uint32_t num_poses, const double* pts, uint32_t n, const double* o, const double* q, const lama_ray_options* opt,
                 lama_ray_result* out, F&& cast)
{
    try {
        lama::sdm::RayCastOptions ro;
        if (opt) { ro.map = opt->map == 0 ? lama::sdm::kRayDistanceMap : lama::sdm::kRayOccupancyMap; ro.stop_at_unknown = opt->stop_at_unknown != 0; ro.tolerance_cells = opt->tolerance_cells; }
        if (opt && opt->map != 0 && opt->map != 1) throw std::invalid_argument("lama_ray_options: map is 0 (distance) or 1 (occupancy)");
        std::vector<Pose2D> poses;
        poses.reserve(num_poses);
        for (uint32_t k = 0; k < num_poses; ++k) poses.push_back(Pose2D(SE2d::fromArray(poses4 + 4 * (size_t)k)));
        lama::sdm::RayCastResult r;
        if (!cast(poses, cloud_of(pts, n, o, q), r, ro)) return 0;
        auto copy = [](auto* dst, const auto& src) { if (dst && !src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(src[0])); };
        if (out) {
            copy(out->status, r.status); copy(out->step, r.step); copy(out->nn, r.nn); copy(out->cell_xy, r.cell_xy); copy(out->end_sqdist, r.end_sqdist);
            copy(out->label, r.label); copy(out->start_xy, r.start_xy); copy(out->range, r.range);
        }
        return 1;
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}
using lama::sdm::RayCastOptions;
using lama::sdm::RayCastResult;
}
extern "C" {
void lama_ray_default_options(lama_ray_options* o)
{
    const RayCastOptions d;
    o->map = (int32_t)d.map; o->stop_at_unknown = d.stop_at_unknown ? 1 : 0; o->tolerance_cells = d.tolerance_cells;
}
int lama_slam_cast_rays(lama_slam* h, const double* poses4, uint32_t num_poses, const double* pts, uint32_t n, const double* o, const double* q,
                        const lama_ray_options* opt, lama_ray_result* out)
{
    return cast_rays_of(h, poses4, num_poses, pts, n, o, q, opt, out, [h](const std::vector<Pose2D>& p, const PointCloudXYZ::Ptr& s, RayCastResult& r, const RayCastOptions& ro) {
        return h->s->castRays(p, s, r, ro); });
}
int lama_pf_cast_rays(lama_pf* h, int64_t particle, const double* poses4, uint32_t num_poses, const double* pts, uint32_t n, const double* o, const double* q,
                      const lama_ray_options* opt, lama_ray_result* out)
{
    return cast_rays_of(h, poses4, num_poses, pts, n, o, q, opt, out, [h, particle](const std::vector<Pose2D>& p, const PointCloudXYZ::Ptr& s, RayCastResult& r, const RayCastOptions& ro) {
        return particle < 0 ? h->pf->castRays(p, s, r, ro) : h->pf->castParticleRays((size_t)particle, p, s, r, ro); });
}
int lama_mapbuilder_cast_rays(lama_mapbuilder* h, const double* poses4, uint32_t num_poses, const double* pts, uint32_t n, const double* o, const double* q,
                              const lama_ray_options* opt, lama_ray_result* out)
{
    return cast_rays_of(h, poses4, num_poses, pts, n, o, q, opt, out, [h](const std::vector<Pose2D>& p, const PointCloudXYZ::Ptr& s, RayCastResult& r, const RayCastOptions& ro) {
        return h->b->castRays(p, s, r, ro); });
}
int lama_lo_cast_rays(lama_lo* h, const double* poses4, uint32_t num_poses, const double* pts, uint32_t n, const double* o, const double* q,
                      const lama_ray_options* opt, lama_ray_result* out)
{
    return cast_rays_of(h, poses4, num_poses, pts, n, o, q, opt, out, [h](const std::vector<Pose2D>& p, const PointCloudXYZ::Ptr& s, RayCastResult& r, const RayCastOptions& ro) {
        return h->l->castRays(p, s, r, ro); });
}
int lama_loc_cast_rays(lama_loc* h, const double* poses4, uint32_t num_poses, const double* pts, uint32_t n, const double* o, const double* q,
                       const lama_ray_options* opt, lama_ray_result* out)
{
    lama_ray_options dm;
    if (!opt) { lama_ray_default_options(&dm); dm.map = 0; opt = &dm; }      // Loc2D's only device map
    return cast_rays_of(h, poses4, num_poses, pts, n, o, q, opt, out, [h](const std::vector<Pose2D>& p, const PointCloudXYZ::Ptr& s, RayCastResult& r, const RayCastOptions& ro) {
        return h->l.castRays(p, s, r, ro); });
}
int64_t lama_loc_check_scan(lama_loc* h, const double* pts, uint32_t n, const double* o, const double* q, int32_t tolerance_cells, uint8_t* labels_out)
{
    try {
        const std::vector<uint8_t> labels = h->l.checkScan(cloud_of(pts, n, o, q), tolerance_cells);
        if (labels_out && !labels.empty()) std::memcpy(labels_out, labels.data(), labels.size());
        return (int64_t)labels.size();
    } catch (const std::exception& e) { h->error = e.what(); return -2; }
}

} // extern "C"
