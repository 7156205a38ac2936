// lama/lidar_odometry_2d.h -- host-side lama::LidarOdometry2D on the MI355X path.
//
// Same struct name, Options and methods as the reference's include/lama/lidar_odometry_2d.h:45-80; update() /
// updateMaps() follow src/lidar_odometry_2d.cpp:60-200: scan-to-map Gauss-Newton (lama_hip_match_solve), then -- after
// 0.1 m / 0.5 rad of motion -- the map update on the device with the ProbabilisticOccupancyMap cell policy
// (cfg.occupancy_policy = 1: float log-odds, src/sdm/probabilistic_occupancy_map.cpp:82-107) and LidarOdometry2D's ray rule
// (the last metre before the hit), the dynamic distance map (max distance 1 m), and the transient-map step that deletes
// every patch whose box does not meet the expanded box of the scan (lama_hip_pf_patch_ids / _delete_patches).
// Differences: `distance_map` / `occupancy_map` are not host objects -- use downloadDistanceMap / downloadOccupancyMap
// (sdm::HostMap, occupancy cells are 4-byte float log-odds); Options gains gpu_device.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "device_context.h"
#include "pose2d.h"
#include "sdm/grid.h"
#include "sdm/ray_cast.h"
#include "sdm/frontier.h"
#include "sdm/travel.h"
#include "sdm_io.h"

namespace lama {

struct LidarOdometry2D {
    bool has_first_scan = false;
    Pose2D odom;
    Pose2D map_update_odom;

    struct Options {
        Options() {}
        double resolution = 0.05;       // resolution of the maps
        uint32_t max_iter = 100;        // maximum number of optimiser iterations
        int32_t gpu_device = 0;         // addition
    };

    explicit LidarOdometry2D(const Options& options = Options());
    virtual ~LidarOdometry2D();
    LidarOdometry2D(const LidarOdometry2D&) = delete;
    LidarOdometry2D& operator=(const LidarOdometry2D&) = delete;

    bool update(const PointCloudXYZ::Ptr& surface, double timestamp);
    void updateMaps(const PointCloudXYZ::Ptr& surface);

    bool downloadDistanceMap(sdm::HostMap& m) const;
    bool downloadOccupancyMap(sdm::HostMap& m) const;      // kind = kProbabilisticOccupancyMap: 4-byte float log-odds cells
    // Dense grids of the device maps, made on the device (lama/sdm/grid.h); false before the first scan.  The occupancy map holds
    // log-odds: trinary only (GridOptions::probability is refused, exp is not exact).  The distance map reaches 1 m.
    bool getOccupancyGrid(sdm::OccupancyGrid& grid, const sdm::GridOptions& options = sdm::GridOptions()) const
    { return device_initialised_ && dev_.occupancyGrid(0, opt_.resolution, grid, options); }
    bool getDistanceGrid(sdm::DistanceGrid& grid, const sdm::GridOptions& options = sdm::GridOptions()) const
    { return device_initialised_ && dev_.distanceGrid(0, opt_.resolution, 1.0, grid, options); }
    // What a sensor at each of `poses` would see in the device map (lama/sdm/ray_cast.h): per pose and point of `surface` the first
    // cell that stops the beam, made on the device.  false before the first scan.  No snapshot is made or dropped.
    bool castRays(const std::vector<Pose2D>& poses, const PointCloudXYZ::Ptr& surface, sdm::RayCastResult& result,
                  const sdm::RayCastOptions& options = sdm::RayCastOptions()) const
    { return device_initialised_ && surface && dev_.castRays(0, opt_.resolution, poses, *surface, result, options); }
    // The frontier clusters of the device occupancy map (lama/sdm/frontier.h), labelled on the device.  false before the first scan.
    bool getFrontiers(sdm::FrontierSet& set, const sdm::FrontierOptions& options = sdm::FrontierOptions()) const
    { return device_initialised_ && dev_.frontiers(0, opt_.resolution, set, options); }
    // Routes through the device maps (lama/sdm/travel.h) from the world points `from` to each of `goals`: reachability, cost and path,
    // relaxed on the device; only the routes come down.  false where getFrontiers returns false.  No snapshot is made or dropped.
    bool planRoutes(const std::vector<Vector2d>& from, const std::vector<Vector2d>& goals, sdm::RouteSet& set, const sdm::TravelOptions& options = sdm::TravelOptions()) const
    { return device_initialised_ && dev_.travel(0, opt_.resolution, false, from, goals, set, options); }
    uint32_t getLastIterations() const { return last_iterations_; }
    uint32_t getLastDeletedPatches() const { return last_deleted_; }
    lama_hip_ctx* deviceContext() const { return dev_.get(); }
    const HipEngine* engine() const { return dev_.engine().get(); }

private:
    Options opt_;
    DeviceContext dev_{"lama::LidarOdometry2D"};
    bool device_initialised_ = false;
    uint32_t last_iterations_ = 0, last_deleted_ = 0;
};

} // namespace lama
