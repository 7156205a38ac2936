// lama/sdm/ray_cast.h -- what a sensor at a given pose WOULD see in a device map: per (pose, beam) the first map cell that stops the ray.
// An addition (the reference answers this with Map::computeRay + isOccupied per beam on a downloaded map): castRays() of the host
// classes walks all beams of all poses on the device (lama_hip_map_cast_rays, iris_lama_amd/csrc/lama_raycast_query.h) -- the expected
// ranges of a beam model, a check of a real scan against the map (Loc2D::checkScan), visibility gating of many candidate poses.
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>
#include <memory>
#include <vector>

#include "../types.h"

namespace lama { namespace sdm {

enum RayMap { kRayDistanceMap = 0, kRayOccupancyMap = 1 };          // LAMA_HIP_MAP_*
enum RayStatus { kRayNone = 0, kRayOccupied = 1, kRayUnknown = 2 };   // LAMA_HIP_RAY_NONE / _OCCUPIED / _UNKNOWN
enum RayLabel { kRayAgrees = 0, kRayBlocked = 1, kRayNovel = 2 };     // LAMA_HIP_RAY_AGREES / _BLOCKED / _NOVEL

struct RayCastOptions {
    RayMap map = kRayOccupancyMap;     // the occupancy map (occupied: probability above 0.25 / positive log-odds), or the distance map
                                       // (occupied: an obstacle cell, squared distance 0)
    bool stop_at_unknown = false;      // occupancy map only: an unvisited cell, a cell at exactly 0.25, a cell no patch holds also stops the ray
    int32_t tolerance_cells = -1;      // >= 0: also label every beam (RayLabel) with this many cells of slack
};

// Beam i of pose k is element k * n + i of every array.  A beam's cells are the map update's: from the cell of the sensor (start_xy of
// its pose; never tested) along Map::computeRay to the cell of the point, nn entries with the point's own cell last.
struct RayCastResult {
    uint32_t num_poses = 0, n = 0;
    double resolution = 0.0;
    std::vector<uint8_t> status;       // RayStatus
    std::vector<int32_t> step;         // index of the stopping cell in the beam's sequence, -1 where nothing stopped the ray
    std::vector<uint32_t> nn;          // cells in the beam's sequence (0: the point lies in the sensor's cell)
    std::vector<uint32_t> cell_xy;     // [2]: the stopping cell; the point's cell where nothing stopped the ray
    std::vector<uint32_t> end_sqdist;  // squared cell distance to the nearest obstacle at the point's cell (the map's largest: none in reach)
    std::vector<uint8_t> label;        // RayLabel; empty unless tolerance_cells >= 0
    std::vector<uint32_t> start_xy;    // [num_poses][2]: the sensor's cell
    std::vector<double> range;         // metres from the sensor's cell to the stopping cell, +inf where nothing stopped the ray
};

// resolution * sqrt(dx^2 + dy^2) of the stopping cell's offset from the start cell: one correctly rounded square root of an exact
// integer (an offset is below 2^14 cells), the same number wherever it is computed
inline double rayRange(double resolution, const uint32_t* start_xy, const uint32_t* cell_xy)
{
    const int64_t dx = (int64_t)cell_xy[0] - (int64_t)start_xy[0], dy = (int64_t)cell_xy[1] - (int64_t)start_xy[1];
    return resolution * std::sqrt((double)(dx * dx + dy * dy));
}
inline void fillRayRanges(RayCastResult& r)
{
    r.range.assign(r.status.size(), std::numeric_limits<double>::infinity());
    for (size_t e = 0; e < r.status.size(); ++e)
        if (r.status[e] != kRayNone) r.range[e] = rayRange(r.resolution, &r.start_xy[2 * (e / r.n)], &r.cell_xy[2 * e]);
}

// The points of a fan in the sensor frame: n beams, beam i at angle_min + i * angle_increment, each max_range long (z = 0) -- what a
// sensor_msgs/LaserScan describes.  cos and sin are taken here on the host, once per beam: the device does no trigonometry.
inline PointCloudXYZ::Ptr makeFan(uint32_t n, double angle_min, double angle_increment, double max_range)
{
    PointCloudXYZ::Ptr cloud(new PointCloudXYZ);
    cloud->points.reserve(n);
    for (uint32_t i = 0; i < n; ++i) {
        const double a = angle_min + (double)i * angle_increment;
        cloud->points.push_back(Vector3d(max_range * std::cos(a), max_range * std::sin(a), 0.0));
    }
    return cloud;
}

}} // namespace lama::sdm
