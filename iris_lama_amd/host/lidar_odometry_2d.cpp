// lidar_odometry_2d.cpp -- host-side lama::LidarOdometry2D (include/lama/lidar_odometry_2d.h); orchestration of
// src/lidar_odometry_2d.cpp:42-200 over a one-particle device context.
#include "lama/lidar_odometry_2d.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>

#include "hip_engine.hpp"
#include "scan_arrays.hpp"
#include "transient_map.hpp"

namespace lama {

LidarOdometry2D::LidarOdometry2D(const Options& o) : opt_(o)              // src/lidar_odometry_2d.cpp:42-52
{
    std::shared_ptr<HipEngine> eng = defaultEngine();
    lama_hip_cfg cfg;
    eng->default_cfg(&cfg);
    cfg.particles = 1;
    cfg.resolution = o.resolution; cfg.patch_size = 32; cfg.l2_max = 1.0; cfg.max_iter = o.max_iter;
    cfg.device = o.gpu_device;
    cfg.occupancy_policy = 1;                  // ProbabilisticOccupancyMap
    cfg.ray_rule = 1;                          // the last metre before the hit
    cfg.dm_patch_capacity = 1024; cfg.occ_patch_capacity = 1024;
    cfg.queue_capacity = 1u << 18;
    dev_.create(std::move(eng), cfg);
}

LidarOdometry2D::~LidarOdometry2D() = default;

bool LidarOdometry2D::update(const PointCloudXYZ::Ptr& surface, double)   // :60-83
{
    if (!surface || surface->points.empty()) throw std::runtime_error("lama::LidarOdometry2D::update: empty scan");
    if (!has_first_scan) {
        updateMaps(surface);
        has_first_scan = true;
        return true;
    }
    const detail::ScanArrays s(*surface);
    double p[4], out7[7];
    int32_t iters = 0;
    odom.state.toArray(p);
    dev_.check(dev_->match_solve(dev_.get(), 0, s.pts.data(), (uint32_t)surface->points.size(), s.o, s.q, p, out7, &iters, 1), "lama_hip_match_solve");
    odom.state = SE2d::fromArray(p);                                       // :72
    last_iterations_ = (uint32_t)iters;
    Pose2D odelta = map_update_odom - odom;                                // :75-80
    if (odelta.xy().norm() > 0.1 || std::abs(odelta.rotation()) > 0.5) {
        updateMaps(surface);
        map_update_odom = odom;
    }
    return true;
}

void LidarOdometry2D::updateMaps(const PointCloudXYZ::Ptr& surface)        // :85-200
{
    const PointCloudXYZ& s = *surface;
    const detail::ScanArrays a(s);
    double p[4];
    odom.state.toArray(p);
    const uint32_t n = (uint32_t)s.points.size();
    if (!device_initialised_) {
        dev_.check(dev_->pf_init(dev_.get(), a.pts.data(), n, a.o, a.q, p), "lama_hip_pf_init");
        device_initialised_ = true;
    } else {
        dev_.check(dev_->pf_set_poses(dev_.get(), p), "lama_hip_pf_set_poses");
        dev_.check(dev_->pf_update_maps(dev_.get(), a.pts.data(), n, a.o, a.q), "lama_hip_pf_update_maps");
    }
    // transient map (:128-199)
    dev_.check(transient::prune(dev_.engine().get(), dev_.get(), s, odom, opt_.resolution, 1.0, 0.0, 1.0, &last_deleted_),
               "lama_hip_pf_patch_ids / lama_hip_pf_delete_patches");
}

bool LidarOdometry2D::downloadDistanceMap(sdm::HostMap& m) const
{
    m.kind = sdm::kDistanceMap; m.resolution = opt_.resolution;
    const uint32_t r = (uint32_t)std::ceil(1.0 * (1.0 / opt_.resolution));
    m.max_sqdist = r * r;
    return dev_.download(0, LAMA_HIP_MAP_DISTANCE, m.ids, m.cells, m.masks);
}

bool LidarOdometry2D::downloadOccupancyMap(sdm::HostMap& m) const
{
    m.kind = sdm::kProbabilisticOccupancyMap;   // 4-byte cells: ProbabilisticOccupancyMap::prob_tag {float}
    m.resolution = opt_.resolution;
    return dev_.download(0, LAMA_HIP_MAP_OCCUPANCY, m.ids, m.cells, m.masks);
}

} // namespace lama
