// device_context.cpp -- lama::DeviceContext (include/lama/device_context.h) and the text of a refused device call.
#include "lama/device_context.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

#include "hip_engine.hpp"
#include "lama/pose2d.h"
#include "lama/sdm/grid.h"
#include "lama/sdm/ray_cast.h"
#include "lama/sdm/frontier.h"
#include "lama/sdm/travel.h"
#include "scan_arrays.hpp"
#include "lama/sdm_maps.h"

namespace lama {

const char* lastDeviceError(const HipEngine& e, const lama_hip_ctx* ctx)
{
    const char* msg = e.last_error ? e.last_error(ctx) : "";
    return msg ? msg : "";
}

std::string deviceFailure(const HipEngine& e, const lama_hip_ctx* ctx, const char* who, const char* what, int32_t rc)
{
    return std::string(who) + ": " + what + " failed (status " + std::to_string(rc) + "): " + lastDeviceError(e, ctx);
}

void DeviceContext::create(std::shared_ptr<HipEngine> engine, const lama_hip_cfg& cfg)
{
    reset();
    eng_ = std::move(engine);
    const int32_t rc = eng_->ctx_create(&cfg, &ctx_);
    if (rc != 0 || !ctx_) {
        ctx_ = nullptr;
        throw std::runtime_error(std::string(owner_) + ": lama_hip_ctx_create failed (status " + std::to_string(rc) +
                                 "): no usable MI355X / HIP device; there is no CPU fallback");
    }
}

void DeviceContext::reset()
{
    if (ctx_) eng_->ctx_destroy(ctx_);
    ctx_ = nullptr;
}

void DeviceContext::check(int32_t rc, const char* what) const
{
    if (rc) throw std::runtime_error(deviceFailure(*eng_, ctx_, owner_, what, rc));
}

bool DeviceContext::download(uint32_t particle, int32_t kind, std::vector<uint64_t>& ids, std::vector<uint8_t>& cells, std::vector<uint64_t>& masks) const
{
    uint32_t n = 0, got = 0;
    if (!ctx_ || eng_->pf_map_patches(ctx_, particle, kind, &n) != 0) return false;
    ids.assign(n, 0);
    cells.assign((size_t)n * kCellsPerPatch * (kind == LAMA_HIP_MAP_DISTANCE ? kDistanceCellBytes : kOccupancyCellBytes), 0);
    masks.assign((size_t)n * kMaskWordsPerPatch, 0);
    if (n == 0) return true;
    return eng_->pf_download_map(ctx_, particle, kind, n, ids.data(), cells.data(), masks.data(), &got) == 0 && got == n;
}

// ---- dense grids (include/lama/sdm/grid.h) ------------------------------------------------------------------------------------
namespace {

constexpr uint32_t kMaxGridSide = 32768;            // pixels (lama_hip_map_rasterize)
constexpr uint32_t kMaxFrontierSide = 32766;        // pixels (lama_hip_map_frontiers: a pixel of halo on either side)

// the box of the grid: Map::bounds of the device map, or the world box in cells (Map::w2m) widened outwards to multiples of the
// stride; a side is clipped to max_side pixels.  false: the map has no patch (whole_map) -- nothing to rasterise.
bool grid_box(const HipEngine& e, lama_hip_ctx* ctx, const char* owner, uint32_t particle, int32_t kind, double resolution,
              const sdm::GridOptions& o, sdm::GridHeader& g, uint32_t max_side = kMaxGridSide)
{
    if (!e.map_bounds || !e.map_rasterize)
        throw std::runtime_error(std::string(owner) + ": the device library " + e.origin + " has no lama_hip_map_bounds / lama_hip_map_rasterize (dense grids)");
    if (o.stride == 0) throw std::invalid_argument(std::string(owner) + ": a grid stride of 0");
    const Map frame(resolution, sdm::kDistanceMap);                 // w2m / m2w of every map of this resolution
    uint64_t lo[2], hi[2];                                          // cells, hi exclusive
    if (o.whole_map) {
        uint32_t a[2], b[2], n = 0;
        const int32_t rc = e.map_bounds(ctx, particle, kind, a, b, &n);
        if (rc) throw std::runtime_error(deviceFailure(e, ctx, owner, "lama_hip_map_bounds", rc));
        if (n == 0) return false;
        for (int k = 0; k < 2; ++k) { lo[k] = a[k]; hi[k] = b[k]; }
    } else {
        if (!(o.world_min[0] <= o.world_max[0]) || !(o.world_min[1] <= o.world_max[1]))
            throw std::invalid_argument(std::string(owner) + ": the world box of a grid needs min <= max");
        const Vector3ui a = frame.w2m(Vector3d(o.world_min[0], o.world_min[1], 0.0)), b = frame.w2m(Vector3d(o.world_max[0], o.world_max[1], 0.0));
        for (int k = 0; k < 2; ++k) { lo[k] = a(k); hi[k] = (uint64_t)b(k) + 1u; }
    }
    const uint64_t s = o.stride;
    for (int k = 0; k < 2; ++k) { lo[k] = lo[k] / s * s; hi[k] = (hi[k] + s - 1u) / s * s; }
    g.x0 = (uint32_t)lo[0]; g.y0 = (uint32_t)lo[1]; g.stride = o.stride;
    g.width = (uint32_t)std::min<uint64_t>((hi[0] - lo[0]) / s, max_side);
    g.height = (uint32_t)std::min<uint64_t>((hi[1] - lo[1]) / s, max_side);
    g.resolution = resolution; g.cell_size = (double)o.stride * resolution;
    const Vector3d w = frame.m2w(Vector3ui(g.x0, g.y0, 0));
    g.origin = Vector3d(w[0], w[1], 0.0);
    return true;
}

template <class T>
void grid_raster(const HipEngine& e, lama_hip_ctx* ctx, const char* owner, uint32_t particle, int32_t layer, const sdm::GridHeader& g, std::vector<T>& out)
{
    out.assign((size_t)g.width * g.height, T(0));
    const int32_t rc = e.map_rasterize(ctx, particle, layer, g.x0, g.y0, g.width, g.height, g.stride, out.data(), (uint64_t)out.size() * sizeof(T));
    if (rc) throw std::runtime_error(deviceFailure(e, ctx, owner, "lama_hip_map_rasterize", rc));
}

} // namespace

bool DeviceContext::occupancyGrid(uint32_t particle, double resolution, sdm::OccupancyGrid& grid, const sdm::GridOptions& options) const
{
    if (!ctx_) return false;
    static_cast<sdm::GridHeader&>(grid) = sdm::GridHeader();
    grid.data.clear();
    if (!grid_box(*eng_, ctx_, owner_, particle, LAMA_HIP_MAP_OCCUPANCY, resolution, options, grid)) return true;     // a map without patches: an empty grid
    grid_raster(*eng_, ctx_, owner_, particle, options.probability ? LAMA_HIP_RASTER_PROBABILITY : LAMA_HIP_RASTER_TRINARY, grid, grid.data);
    return true;
}

bool DeviceContext::distanceGrid(uint32_t particle, double resolution, double l2_max, sdm::DistanceGrid& grid, const sdm::GridOptions& options) const
{
    if (!ctx_) return false;
    static_cast<sdm::GridHeader&>(grid) = sdm::GridHeader();
    grid.sqdist.clear();
    const uint32_t r = (uint32_t)std::ceil(l2_max * (1.0 / resolution));         // DynamicDistanceMap::setMaxDistance / maxDistance
    grid.max_distance = std::sqrt((double)(r * r)) * resolution;
    if (!grid_box(*eng_, ctx_, owner_, particle, LAMA_HIP_MAP_DISTANCE, resolution, options, grid)) return true;
    grid_raster(*eng_, ctx_, owner_, particle, LAMA_HIP_RASTER_SQDIST, grid, grid.sqdist);
    return true;
}

// ---- frontiers (include/lama/sdm/frontier.h) ------------------------------------------------------------------------------------
bool DeviceContext::frontiers(uint32_t particle, double resolution, sdm::FrontierSet& set, const sdm::FrontierOptions& o) const
{
    if (!ctx_) return false;
    if (!eng_->map_frontiers)
        throw std::runtime_error(std::string(owner_) + ": the device library " + eng_->origin + " has no lama_hip_map_frontiers (frontier clusters of device maps)");
    set = sdm::FrontierSet();
    sdm::GridOptions go;
    go.stride = o.stride; go.whole_map = o.whole_map; go.world_min = o.world_min; go.world_max = o.world_max;
    if (!grid_box(*eng_, ctx_, owner_, particle, LAMA_HIP_MAP_OCCUPANCY, resolution, go, set, kMaxFrontierSide)) return true;     // a map without patches: no frontier
    if (o.labels) set.labels.assign((size_t)set.width * set.height, 0xFFFFFFFFu);
    // the count first where the list is not capped: the records are 40 bytes each, the labelling itself is the smaller part of a call
    std::vector<lama_hip_frontier> recs(o.max_frontiers ? o.max_frontiers : 256u);
    uint32_t n = 0;
    for (;;) {
        check(eng_->map_frontiers(ctx_, particle, set.x0, set.y0, set.width, set.height, set.stride, o.min_pixels, (uint32_t)recs.size(), recs.data(), &n,
                                  &set.frontier_pixels, o.labels ? set.labels.data() : nullptr, nullptr),
              "lama_hip_map_frontiers");
        if (o.max_frontiers || n <= recs.size()) break;
        recs.resize(n);                                             // more clusters than the first guess: once more, with room for all
    }
    set.clusters = n;
    recs.resize(std::min<size_t>(recs.size(), n));
    set.frontiers.resize(recs.size());
    const double s = (double)set.stride, half = ((double)set.stride - 1.0) / 2.0;
    for (size_t k = 0; k < recs.size(); ++k) {
        const lama_hip_frontier& r = recs[k];
        sdm::Frontier& f = set.frontiers[k];
        f.label = r.label; f.pixels = r.pixels; f.min_i = r.min_i; f.min_j = r.min_j; f.max_i = r.max_i; f.max_j = r.max_j; f.sum_i = r.sum_i; f.sum_j = r.sum_j;
        const double ci = (double)r.sum_i / (double)r.pixels, cj = (double)r.sum_j / (double)r.pixels;
        f.centroid = Vector2d(set.origin[0] + resolution * (s * ci + half), set.origin[1] + resolution * (s * cj + half));
        f.seed = Vector2d(set.origin[0] + resolution * (s * (double)(r.label % set.width) + half), set.origin[1] + resolution * (s * (double)(r.label / set.width) + half));
    }
    return true;
}

// ---- routes (include/lama/sdm/travel.h) -----------------------------------------------------------------------------------------
bool DeviceContext::travel(uint32_t particle, double resolution, bool distance_only, const std::vector<Vector2d>& from, const std::vector<Vector2d>& goals,
                           sdm::RouteSet& set, const sdm::TravelOptions& o) const
{
    if (!ctx_) return false;
    if (!eng_->map_travel)
        throw std::runtime_error(std::string(owner_) + ": the device library " + eng_->origin + " has no lama_hip_map_travel (routes through device maps)");
    if (from.empty()) throw std::invalid_argument(std::string(owner_) + ": planRoutes needs at least one point to start from");
    if (!(o.robot_radius >= 0.0) || !(o.preferred_clearance >= 0.0)) throw std::invalid_argument(std::string(owner_) + ": planRoutes needs a robot radius and a preferred clearance >= 0");
    set = sdm::RouteSet();
    set.routes.resize(goals.size());
    sdm::GridOptions go;
    go.stride = o.stride; go.whole_map = o.whole_map; go.world_min = o.world_min; go.world_max = o.world_max;
    if (!grid_box(*eng_, ctx_, owner_, particle, distance_only ? LAMA_HIP_MAP_DISTANCE : LAMA_HIP_MAP_OCCUPANCY, resolution, go, set)) return true;   // a map without patches: nothing is reached
    const Map frame(resolution, sdm::kDistanceMap);                 // w2m of every map of this resolution
    auto cells = [&frame](const std::vector<Vector2d>& pts) {
        std::vector<uint32_t> xy(2 * pts.size());
        for (size_t k = 0; k < pts.size(); ++k) {
            const Vector3ui c = frame.w2m(Vector3d(pts[k][0], pts[k][1], 0.0));
            xy[2 * k] = c(0); xy[2 * k + 1] = c(1);
        }
        return xy;
    };
    const std::vector<uint32_t> src = cells(from), dst = cells(goals);
    const double inv = 1.0 / resolution;
    const double clear = std::ceil(o.robot_radius * inv), prefer = std::max(clear, std::ceil(o.preferred_clearance * inv));
    if (prefer > 65535.0) throw std::invalid_argument(std::string(owner_) + ": the preferred clearance of planRoutes exceeds 65535 cells");
    const uint32_t ng = (uint32_t)goals.size(), cap = o.max_path_points;
    std::vector<lama_hip_route> routes(ng);
    std::vector<uint32_t> paths((size_t)ng * cap);
    if (o.field) set.field.assign((size_t)set.width * set.height, 0xFFFFFFFFu);
    check(eng_->map_travel(ctx_, particle, set.x0, set.y0, set.width, set.height, set.stride, (uint32_t)clear, (uint32_t)prefer, o.near_factor, (uint32_t)from.size(),
                           src.data(), ng, ng ? dst.data() : nullptr, o.goal_reach, ng ? routes.data() : nullptr, cap, paths.empty() ? nullptr : paths.data(),
                           o.field ? set.field.data() : nullptr, &set.rounds, nullptr),
          "lama_hip_map_travel");
    const double s = (double)set.stride, half = ((double)set.stride - 1.0) / 2.0;
    for (uint32_t g = 0; g < ng; ++g) {
        sdm::Route& r = set.routes[g];
        r.status = routes[g].status; r.pixel = routes[g].pixel; r.cost = routes[g].cost; r.steps = routes[g].steps;
        if (r.status != sdm::kRouteReached) continue;
        r.length_m = (double)r.cost * set.cell_size / 5.0;
        const size_t n = (size_t)std::min<uint64_t>(cap, (uint64_t)r.steps + 1u);
        r.path.resize(n);
        for (size_t k = 0; k < n; ++k) {
            const uint32_t p = paths[(size_t)g * cap + k];
            r.path[k] = Vector2d(set.origin[0] + resolution * (s * (double)(p % set.width) + half), set.origin[1] + resolution * (s * (double)(p / set.width) + half));
        }
    }
    return true;
}

// ---- ray casts (include/lama/sdm/ray_cast.h) ------------------------------------------------------------------------------------
bool DeviceContext::castRays(uint32_t particle, double resolution, const std::vector<Pose2D>& poses, const PointCloudXYZ& surface, sdm::RayCastResult& r,
                             const sdm::RayCastOptions& o) const
{
    if (!ctx_) return false;
    if (!eng_->map_cast_rays)
        throw std::runtime_error(std::string(owner_) + ": the device library " + eng_->origin + " has no lama_hip_map_cast_rays (ray casts through device maps)");
    r = sdm::RayCastResult();
    r.num_poses = (uint32_t)poses.size(); r.n = (uint32_t)surface.points.size(); r.resolution = resolution;
    const size_t total = poses.size() * surface.points.size();
    std::vector<double> poses4(4 * poses.size());
    for (size_t k = 0; k < poses.size(); ++k) poses[k].state.toArray(&poses4[4 * k]);
    const detail::ScanArrays a(surface);
    r.status.assign(total, 0); r.step.assign(total, -1); r.nn.assign(total, 0); r.cell_xy.assign(2 * total, 0); r.end_sqdist.assign(total, 0);
    r.start_xy.assign(2 * poses.size(), 0);
    if (o.tolerance_cells >= 0) r.label.assign(total, 0);
    // (an empty pose list or scan goes to the device library too: it is the one place that says what is refused)
    check(eng_->map_cast_rays(ctx_, particle, (int32_t)o.map, r.num_poses, poses4.data(), a.pts.data(), r.n, a.o, a.q,
                              o.stop_at_unknown ? LAMA_HIP_RAY_STOP_UNKNOWN : 0u, o.tolerance_cells, r.status.data(), r.step.data(), r.nn.data(), r.cell_xy.data(),
                              r.end_sqdist.data(), r.label.empty() ? nullptr : r.label.data(), r.start_xy.data(), nullptr),
          "lama_hip_map_cast_rays");
    sdm::fillRayRanges(r);
    return true;
}

} // namespace lama
