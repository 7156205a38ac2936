// lama/map_builder_2d.h -- lama::MapBuilder2D: a map rebuilt from posed key scans, on the MI355X path.
//
// The step every loop-closing user performs right after optimising a pose graph (lama::SimplePGO hands back corrected key poses):
// the reference does it in GraphSlam2D::generateOccupancyMap (src/graph_slam2d.cpp:131-164) -- for every key pose setOccupied at
// each hit and, in the full variant, computeRay + setFree along each beam, then prune().  The same routine serves anyone who wants
// a clean map from a finished trajectory (a particle's pose history, an offline log).  Here all key scans are integrated in one
// order-free pass on the device (lama_hip_map_integrate_scans, csrc/lama_map_build.h); the result is bit-identical to the
// reference's sequential loop.  With Options::l2_max > 0 build() also replaces the distance map by the one of the occupied cells
// (addObstacle for each + update(), the way Loc2D::Init builds its map), so the rebuilt map serves MatchSurface2D / lama::Solve and
// the lama_hip_match_* entry points without a round trip through a file.  There is no CPU fallback.
//
//   full = false with resolution = 0.1 is the reference's coarse variant (generateOccupancyMap(false)).
//   build() integrates the keys added since the last build (the reference's mapping_keyid increment); after setPose / setPoses
//   it rebuilds from all keys.  An empty cloud contributes nothing (the reference never inspects the cloud).
#pragma once

#include <cmath>
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
#include "sdm_maps.h"

namespace lama {

class MapBuilder2D {
public:
    struct Options {
        Options() {}
        double resolution = 0.05;
        uint32_t patch_size = 32;
        bool full = true;            // free cells along the rays (generateOccupancyMap(true)); false: hits only
        bool prune = true;           // FrequencyOccupancyMap::prune after every build
        double l2_max = 0.5;         // reach of the distance map; 0: no distance map
        int32_t gpu_device = 0;
        uint32_t window_patches = 0, occ_patch_capacity = 0, dm_patch_capacity = 0;      // device map storage, 0 = defaults
    };
    // wall-clock milliseconds of the last build(), by stage
    struct Timing { double integrate_ms = 0, occupied_ms = 0, distance_ms = 0; };

    explicit MapBuilder2D(const Options& options = Options());
    virtual ~MapBuilder2D();
    MapBuilder2D(const MapBuilder2D&) = delete;
    MapBuilder2D& operator=(const MapBuilder2D&) = delete;

    size_t add(const PointCloudXYZ::Ptr& cloud, const Pose2D& pose);      // returns the key id
    void setPose(size_t key, const Pose2D& pose);                         // e.g. from SimplePGO; marks the map stale
    void setPoses(const std::vector<Pose2D>& poses);
    Pose2D getPose(size_t key) const { return poses_.at(key); }
    size_t size() const { return poses_.size(); }
    void build();
    void reset();

    // the occupied cells the last build() found ({x, y} map coordinates, Map::visit_all_cells order); empty with l2_max == 0
    const std::vector<uint32_t>& occupiedCells() const { return occupied_; }
    Timing lastTiming() const { return timing_; }

    bool downloadOccupancyMap(sdm::HostMap& m) const;
    bool downloadDistanceMap(sdm::HostMap& m) const;
    // host snapshots with the reference's const query API (lama/sdm_maps.h), as in Slam2D: downloaded on first use after a build,
    // kept until the next one; nullptr before the first build.  The distance map is bound to the device (bindDevice): MatchSurface2D
    // and lama::Solve run their kernels on the map build() left there.
    const FrequencyOccupancyMap* getOccupancyMap() const;
    const DynamicDistanceMap* getDistanceMap() const;

    // Dense grids of the built maps, made on the device (lama/sdm/grid.h); false before the first build (the distance grid also with
    // l2_max == 0).  The snapshots above are neither made nor dropped.
    bool getOccupancyGrid(sdm::OccupancyGrid& grid, const sdm::GridOptions& options = sdm::GridOptions()) const
    { return has_map_ && dev_.occupancyGrid(0, opt_.resolution, grid, options); }
    bool getDistanceGrid(sdm::DistanceGrid& grid, const sdm::GridOptions& options = sdm::GridOptions()) const
    { return has_map_ && opt_.l2_max > 0.0 && dev_.distanceGrid(0, opt_.resolution, opt_.l2_max, grid, options); }
    // What a sensor at each of `poses` would see in the device map (lama/sdm/ray_cast.h): per pose and point of `surface` the first
    // cell that stops the beam, made on the device.  false before the first build.  No snapshot is made or dropped.
    bool castRays(const std::vector<Pose2D>& poses, const PointCloudXYZ::Ptr& surface, sdm::RayCastResult& result,
                  const sdm::RayCastOptions& options = sdm::RayCastOptions()) const
    { return has_map_ && surface && dev_.castRays(0, opt_.resolution, poses, *surface, result, options); }
    // The frontier clusters of the built occupancy map (lama/sdm/frontier.h), labelled on the device.  false before the first build.
    bool getFrontiers(sdm::FrontierSet& set, const sdm::FrontierOptions& options = sdm::FrontierOptions()) const
    { return has_map_ && dev_.frontiers(0, opt_.resolution, set, options); }
    // Routes through the device maps (lama/sdm/travel.h) from the world points `from` to each of `goals`: reachability, cost and path,
    // relaxed on the device; only the routes come down.  false where getFrontiers returns false.  No snapshot is made or dropped.
    bool planRoutes(const std::vector<Vector2d>& from, const std::vector<Vector2d>& goals, sdm::RouteSet& set, const sdm::TravelOptions& options = sdm::TravelOptions()) const
    { return has_map_ && dev_.travel(0, opt_.resolution, false, from, goals, set, options); }

    lama_hip_ctx* deviceContext() const { return dev_.get(); }
    const HipEngine* engine() const { return dev_.engine().get(); }

private:
    Options opt_;
    DeviceContext dev_{"lama::MapBuilder2D"};        // declared before dm_view_, which holds its raw handle: destroyed after it
    std::vector<Pose2D> poses_;
    std::vector<double> pts_, origins_, quats_;      // all key scans: points concatenated, per-scan sensor origin / orientation
    std::vector<uint32_t> offsets_{0u};
    size_t built_ = 0;                               // keys in the device map
    bool stale_ = false, has_map_ = false;
    std::vector<uint32_t> occupied_;
    Timing timing_;
    mutable std::unique_ptr<FrequencyOccupancyMap> occ_view_;
    mutable std::unique_ptr<DynamicDistanceMap> dm_view_;
};

} // namespace lama
