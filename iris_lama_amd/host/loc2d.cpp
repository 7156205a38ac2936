// loc2d.cpp -- host-side lama::Loc2D (include/lama/loc2d.h); orchestration of src/loc2d.cpp:61-192.
#include "lama/loc2d.h"

#include <cmath>
#include <algorithm>
#include <limits>
#include <stdexcept>

#include "correlative_impl.hpp"
#include "covariance3.hpp"
#include "dm_builder.hpp"
#include "hip_engine.hpp"
#include "scan_arrays.hpp"
#include "lama/random.h"

namespace lama {

Loc2D::Options::Options()                      // src/loc2d.cpp:46-58
{
    trans_thresh = 0.5; rot_thresh = 0.5; l2_max = 1.0; resolution = 0.05; patch_size = 32;
    gloc_particles = 3000; gloc_iters = 10; gloc_thresh = 0.15; max_iter = 100; cov_blend = 0.0;
}

void Loc2D::Init(const Options& o)
{
    opt_ = o;
    // a second Init() (new map, resolution, l2_max or strategy) starts from fresh maps like the reference's (src/loc2d.cpp:61-78):
    // the device context is rebuilt from the new options by the next ensureContext()
    dev_.reset();
    delete occupancy_map; delete distance_map;
    occupancy_map = new SimpleOccupancyMap(o.resolution, o.patch_size);                // src/loc2d.cpp:63-66
    distance_map = new DynamicDistanceMap(o.resolution, o.patch_size);
    distance_map->setMaxDistance(o.l2_max);
    DynamicDistanceMap::Writer w;
    w.apply = [this](std::vector<uint32_t>& cells_xy, double max_distance) -> uint32_t {
        (void)max_distance;                                 // part of the context's configuration (ensureContext)
        ensureContext();
        // an empty map is built on the host and uploaded, a map that exists is updated on the device (dm_builder.hpp)
        bool host_built = false; uint32_t processed = 0; const char* what = "";
        const int32_t rc = detail::add_obstacles_to_map(*dev_.engine(), dev_.get(), cells_xy.data(), cells_xy.size() / 2, distance_map->resolution,
                                                        distance_map->patch_length, distance_map->maxSqDist(), host_built, processed, what);
        dev_.check(rc, what);
        if (host_built) host_built_ = true;
        return processed;
    };
    w.download = [this](sdm::HostMap& m) -> bool {
        m.kind = sdm::kDistanceMap; m.max_sqdist = distance_map->maxSqDist();
        return dev_.download(0, LAMA_HIP_MAP_DISTANCE, m.ids, m.cells, m.masks);         // false while there is no context
    };
    w.upload = [this](const sdm::HostMap& m) {
        ensureContext();
        dev_.check(dev_->pf_upload_map(dev_.get(), 0, LAMA_HIP_MAP_DISTANCE, (uint32_t)m.ids.size(), m.ids.data(), m.cells.data(), m.masks.data()),
                   "lama_hip_pf_upload_map");
    };
    distance_map->bindWriter(std::move(w));
    rmse_ = 0.0;
    host_built_ = false;
    cov_ = Matrix3d::Identity();
    has_first_scan = false;
    do_global_localization_ = false;                                   // :80-90
    gloc_cur_iter_ = 0;
    cov_blend_ = std::max(std::min(o.cov_blend, 1.0), 0.0);
    if (!sampling_steps_.empty()) return;                              // :93-107
    const double sstep = distance_map->resolution;
    sampling_steps_.push_back(Vector2d(0.0, 0.0));
    for (int i = 1; i <= 20; ++i) {
        sampling_steps_.push_back(Vector2d(i * sstep, 0.0));   sampling_steps_.push_back(Vector2d(0.0, i * sstep));
        sampling_steps_.push_back(Vector2d(-i * sstep, 0.0));  sampling_steps_.push_back(Vector2d(0.0, -i * sstep));
        sampling_steps_.push_back(Vector2d(i * sstep, i * sstep));   sampling_steps_.push_back(Vector2d(-i * sstep, i * sstep));
        sampling_steps_.push_back(Vector2d(i * sstep, -i * sstep));  sampling_steps_.push_back(Vector2d(-i * sstep, -i * sstep));
    }
}

Loc2D::~Loc2D()
{
    delete occupancy_map;
    delete distance_map;
}

void Loc2D::ensureContext()
{
    if (dev_) return;
    if (!distance_map) throw std::runtime_error("lama::Loc2D: Init() must be called first");
    std::shared_ptr<HipEngine> eng = defaultEngine(distance_map->maxDistanceOption(), opt_.resolution);
    lama_hip_cfg cfg;
    eng->default_cfg(&cfg);
    cfg.particles = 1;
    cfg.resolution = opt_.resolution; cfg.patch_size = opt_.patch_size; cfg.l2_max = distance_map->maxDistanceOption(); cfg.max_iter = opt_.max_iter;
    cfg.device = opt_.gpu_device;
    cfg.solver_strategy = opt_.strategy == "lm" ? 1u : 0u;       // makeStrategy, src/loc2d.cpp:288-294
    cfg.dm_patch_capacity = 4096;            // a static building-scale map; occupancy is not kept on the device
    cfg.occ_patch_capacity = 8;
    cfg.queue_capacity = 1u << 20;
    dev_.create(std::move(eng), cfg);
}

bool Loc2D::enoughMotion(const Pose2D& odometry)               // src/loc2d.cpp:113-124
{
    if (!has_first_scan) return true;
    Pose2D odelta = odom_ - odometry;
    if (odelta.xy().norm() <= opt_.trans_thresh && std::abs(odelta.rotation()) <= opt_.rot_thresh) return false;
    return true;
}

void Loc2D::solve(const PointCloudXYZ& s, bool do_solve)
{
    ensureContext();
    const detail::ScanArrays a(s);
    double p[4], out7[7];
    int32_t iters = 0;
    pose_.state.toArray(p);
    dev_.check(dev_->match_solve(dev_.get(), 0, a.pts.data(), (uint32_t)s.points.size(), a.o, a.q, p, out7, &iters, do_solve ? 1 : 0), "lama_hip_match_solve");
    if (do_solve) {
        pose_.state = SE2d::fromArray(p);
        last_iterations_ = (uint32_t)iters;
        double c9[9];
        detail::covariance_from_normal3(out7, c9);
        for (int k = 0; k < 9; ++k) cov_(k / 3, k % 3) = c9[k];
        if (cov_blend_ > 0.0) addSamplingCovariance(s);                                 // :175-176
    }
    rmse_ = std::sqrt(out7[6] / ((double)(s.points.size() - 1)));                       // :178-180
}

bool Loc2D::update(const PointCloudXYZ::Ptr& surface, const Pose2D& odometry, double, bool force_update)
{
    if (!surface || surface->points.size() < 2) throw std::runtime_error("lama::Loc2D::update: empty scan");
    if (distance_map && distance_map->hasPending()) distance_map->update();
    if (!has_first_scan) {                                      // :128-143
        odom_ = odometry;
        has_first_scan = true;
        if (!force_update) return true;
        solve(*surface, false);
    }
    Pose2D odelta = odom_ - odometry;                           // :146-147
    Pose2D ppose = pose_ + odelta;
    if (!force_update && !enoughMotion(odometry)) return false; // :151-152
    pose_ = ppose;
    odom_ = odometry;
    if (do_global_localization_) {                              // :157-168
        if (gloc_cur_iter_ < opt_.gloc_iters) {
            ++gloc_cur_iter_;
            globalLocalization(*surface);
        } else {
            do_global_localization_ = false;
            gloc_cur_iter_ = 0;
        }
    }
    solve(*surface, true);                                      // :170-180 (cov, optional sampling covariance, rmse)
    if (do_global_localization_ && rmse_ < opt_.gloc_thresh) {  // :182-189
        do_global_localization_ = false;
        gloc_cur_iter_ = 0;
    }
    return true;
}

// Additions: ray casts through the device distance map (include/lama/sdm/ray_cast.h)
bool Loc2D::castRays(const std::vector<Pose2D>& poses, const PointCloudXYZ::Ptr& surface, sdm::RayCastResult& result, const sdm::RayCastOptions& options)
{
    if (options.map != sdm::kRayDistanceMap) throw std::invalid_argument("lama::Loc2D::castRays: only the distance map is on the device (RayCastOptions::map = kRayDistanceMap)");
    if (distance_map && distance_map->hasPending()) distance_map->update();
    return dev_ && surface && dev_.castRays(0, opt_.resolution, poses, *surface, result, options);
}

bool Loc2D::planRoutes(const std::vector<Vector2d>& from, const std::vector<Vector2d>& goals, sdm::RouteSet& set, const sdm::TravelOptions& options)
{
    if (distance_map && distance_map->hasPending()) distance_map->update();
    return dev_ && dev_.travel(0, opt_.resolution, true, from, goals, set, options);
}

std::vector<uint8_t> Loc2D::checkScan(const PointCloudXYZ::Ptr& surface, int32_t tolerance_cells)
{
    if (tolerance_cells < 0) throw std::invalid_argument("lama::Loc2D::checkScan: tolerance_cells must not be negative");
    sdm::RayCastOptions o = distanceRays();
    o.tolerance_cells = tolerance_cells;
    sdm::RayCastResult r;
    if (!castRays(std::vector<Pose2D>(1, pose_), surface, r, o)) return std::vector<uint8_t>();
    return std::move(r.label);
}

void Loc2D::triggerGlobalLocalization() { do_global_localization_ = true; }      // :194-197

// An addition: the lattice search of lama::CorrelativeSearch2D over the occupancy map's extent, on this object's context.
bool Loc2D::relocalize(const PointCloudXYZ::Ptr& surface, const CorrelativeSearch2D::Options& options)
{
    if (!surface || surface->points.empty()) throw std::runtime_error("lama::Loc2D::relocalize: empty scan");
    if (!distance_map || !occupancy_map) throw std::runtime_error("lama::Loc2D: Init() must be called first");
    if (distance_map->hasPending()) distance_map->update();
    ensureContext();
    Vector3d mn, mx;
    occupancy_map->bounds(mn, mx);
    detail::CorrelativeDevice dev;
    dev.engine = dev_.engine().get(); dev.ctx = dev_.get(); dev.particle = 0; dev.resolution = distance_map->resolution;
    const SimpleOccupancyMap* occ = occupancy_map;
    reloc_ = detail::correlative_search(CorrelativeSearch2D(options), dev, *surface, Vector2d(mn[0], mn[1]), Vector2d(mx[0], mx[1]),
                                        [occ](double x, double y) { return occ->isFree(Vector3d(x, y, 0.0)); });
    if (reloc_.empty() || !(reloc_[0].rmse < opt_.gloc_thresh)) return false;
    setPose(reloc_[0].pose);
    return true;
}

// :249-286.  The candidates are drawn exactly like the reference (x, y until the cell is free in the occupancy map,
// then the heading; lama::random's stream); their squared residual norms come from the device in one batch and the
// FIRST smallest one wins (the reference's strict `<`).
void Loc2D::globalLocalization(const PointCloudXYZ& surface)
{
    ensureContext();
    Vector3d mn, mx;
    occupancy_map->bounds(mn, mx);
    const double diff0 = mx[0] - mn[0], diff1 = mx[1] - mn[1];
    const uint32_t B = opt_.gloc_particles;
    if (B == 0) return;
    bool any_free = false;
    occupancy_map->visit_all_cells([&](const Vector3ui& c) { if (!any_free && occupancy_map->isFree(c)) any_free = true; });
    if (!any_free) throw std::runtime_error("lama::Loc2D::globalLocalization: the occupancy map has no free cell");
    gloc_poses_.assign((size_t)4 * B, 0.0);
    gloc_errors_.assign(B, 0.0);
    for (uint32_t i = 0; i < B; ++i) {
        double x, y, a;
        for (;;) {
            x = mn[0] + random::uniform() * diff0;
            y = mn[1] + random::uniform() * diff1;
            if (!occupancy_map->isFree(Vector3d(x, y, 0.0))) continue;
            a = random::uniform() * 2 * M_PI - M_PI;
            break;
        }
        Pose2D(x, y, a).state.toArray(&gloc_poses_[4 * i]);
    }
    const detail::ScanArrays a(surface);
    dev_.check(dev_->eval_batch(dev_.get(), 0, a.pts.data(), (uint32_t)surface.points.size(), a.o, a.q, gloc_poses_.data(), B, gloc_errors_.data(), nullptr),
               "lama_hip_eval_batch");
    double best_error = std::numeric_limits<double>::max();
    for (uint32_t i = 0; i < B; ++i)
        if (gloc_errors_[i] < best_error) { best_error = gloc_errors_[i]; pose_.state = SE2d::fromArray(&gloc_poses_[4 * i]); }
}

// :199-247 (Olson 2009).  The 161 likelihood samples come from the device, the 2x2 statistics are accumulated here in
// the reference's order.
void Loc2D::addSamplingCovariance(const PointCloudXYZ& surface)
{
    const size_t num_points = surface.points.size();
    const size_t step = std::max(num_points / 100, size_t(1));
    const size_t K = sampling_steps_.size();
    std::vector<double> xy(2 * K);
    for (size_t i = 0; i < K; ++i) { xy[2 * i] = pose_.x() + sampling_steps_[i].x(); xy[2 * i + 1] = pose_.y() + sampling_steps_[i].y(); }
    sampling_l_.assign(K, 0.0);
    const detail::ScanArrays a(surface);
    dev_.check(dev_->map_sample_likelihood(dev_.get(), 0, a.pts.data(), (uint32_t)num_points, a.o, a.q, pose_.rotation(), xy.data(), (uint32_t)K,
                                           (uint32_t)step, sampling_l_.data()), "lama_hip_map_sample_likelihood");
    double Km[2][2] = {{0, 0}, {0, 0}}, u[2] = {0, 0}, s = 0;
    for (size_t i = 0; i < K; ++i) {
        const double x = xy[2 * i], y = xy[2 * i + 1], l = sampling_l_[i];
        Km[0][0] = Km[0][0] + x * x * l; Km[0][1] = Km[0][1] + x * y * l;
        Km[1][0] = Km[1][0] + y * x * l; Km[1][1] = Km[1][1] + y * y * l;
        u[0] = u[0] + x * l; u[1] = u[1] + y * l;
        s = s + l;
    }
    const double a1 = 1.0 / s, a2 = 1.0 / (s * s);
    const double sc[2][2] = {{a1 * Km[0][0] - a2 * u[0] * u[0], a1 * Km[0][1] - a2 * u[0] * u[1]},
                             {a1 * Km[1][0] - a2 * u[1] * u[0], a1 * Km[1][1] - a2 * u[1] * u[1]}};
    const double alpha = cov_blend_;
    for (int r = 0; r < 2; ++r) for (int c = 0; c < 2; ++c) cov_(r, c) = alpha * sc[r][c] + (1.0 - alpha) * cov_(r, c);
}

} // namespace lama
