// lama/device_context.h -- lama::DeviceContext: the device context of a host class (Slam2D, Loc2D, LidarOdometry2D, MapBuilder2D,
// PFSlam2D), owned by type: created once, destroyed exactly once, and the one place that turns a refused device call into the
// exception those classes throw.  Only forward declarations of the device C-ABI (include/lama_hip.h), like the class headers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "types.h"

struct lama_hip_ctx;
struct lama_hip_cfg;

namespace lama {

struct HipEngine;   // function table of include/lama_hip.h resolved with dlopen
namespace sdm { struct GridOptions; struct OccupancyGrid; struct DistanceGrid; }      // include/lama/sdm/grid.h
namespace sdm { struct RayCastOptions; struct RayCastResult; }                        // include/lama/sdm/ray_cast.h
namespace sdm { struct FrontierOptions; struct FrontierSet; }                         // include/lama/sdm/frontier.h
namespace sdm { struct TravelOptions; struct RouteSet; }                              // include/lama/sdm/travel.h
struct Pose2D;
struct PointCloudXYZ;

class DeviceContext {
public:
    // layout of a downloaded patch (the reference's records): 32 x 32 cells of 10 bytes (distance_t) or 4 bytes
    // (frequency / float log-odds), and one presence bit per cell
    static constexpr size_t kCellsPerPatch = 1024, kMaskWordsPerPatch = 16, kDistanceCellBytes = 10, kOccupancyCellBytes = 4;

    explicit DeviceContext(const char* owner) : owner_(owner) {}              // owner: "lama::Slam2D", ... (a string literal)
    DeviceContext(DeviceContext&& o) noexcept : eng_(std::move(o.eng_)), ctx_(o.ctx_), owner_(o.owner_) { o.ctx_ = nullptr; }
    DeviceContext& operator=(DeviceContext&& o) noexcept
    {
        if (this != &o) { reset(); eng_ = std::move(o.eng_); ctx_ = o.ctx_; owner_ = o.owner_; o.ctx_ = nullptr; }
        return *this;
    }
    ~DeviceContext() { reset(); }

    // a context of `engine` from cfg; throws std::runtime_error when the device library refuses (no device, unsupported options)
    void create(std::shared_ptr<HipEngine> engine, const lama_hip_cfg& cfg);
    void reset();                                                             // destroys the context, if any
    explicit operator bool() const { return ctx_ != nullptr; }
    lama_hip_ctx* get() const { return ctx_; }
    const std::shared_ptr<HipEngine>& engine() const { return eng_; }
    const HipEngine* operator->() const { return eng_.get(); }
    // rc != 0: throws std::runtime_error "<owner>: <what> failed (status <rc>): <the context's last error>"
    void check(int32_t rc, const char* what) const;
    // one particle's map of a kind (LAMA_HIP_MAP_*) in the reference's record formats; true with empty arrays when it has no patch
    bool download(uint32_t particle, int32_t kind, std::vector<uint64_t>& ids, std::vector<uint8_t>& cells, std::vector<uint64_t>& masks) const;
    // One particle's map written out dense on the device (lama_hip_map_bounds + lama_hip_map_rasterize, include/lama/sdm/grid.h):
    // the whole map or the world box of the options.  The snapshots behind download() are neither made nor touched.  Throws
    // std::runtime_error when the device library lacks the two entry points or refuses the call, std::invalid_argument for a
    // stride of 0 or a world box whose max lies below its min.
    bool occupancyGrid(uint32_t particle, double resolution, sdm::OccupancyGrid& grid, const sdm::GridOptions& options) const;
    bool distanceGrid(uint32_t particle, double resolution, double l2_max, sdm::DistanceGrid& grid, const sdm::GridOptions& options) const;
    // What a sensor at each pose would see in one particle's device map (lama_hip_map_cast_rays, include/lama/sdm/ray_cast.h): the
    // first cell of every beam of `surface` that stops the ray, ranges included.  false without a context.  Throws
    // std::runtime_error when the device library lacks the entry point or refuses the call (no pose, no point, a beam of more than
    // 8191 cells, stop_at_unknown on the distance map, ...).  No map, pose or snapshot changes.
    bool castRays(uint32_t particle, double resolution, const std::vector<Pose2D>& poses, const PointCloudXYZ& surface, sdm::RayCastResult& result,
                  const sdm::RayCastOptions& options) const;
    // The frontier clusters of one particle's occupancy map (lama_hip_map_frontiers, include/lama/sdm/frontier.h), over the box
    // occupancyGrid would take.  false without a context.  Throws std::runtime_error when the device library lacks the entry point
    // or refuses the call, std::invalid_argument as occupancyGrid does.  No map, pose or snapshot changes.
    bool frontiers(uint32_t particle, double resolution, sdm::FrontierSet& set, const sdm::FrontierOptions& options) const;
    // Routes through one particle's device maps (lama_hip_map_travel, include/lama/sdm/travel.h) from the world points `from` to each
    // of `goals`, over the box occupancyGrid would take -- or, with distance_only (a context whose only device map is the distance
    // map: lama::Loc2D), the box distanceGrid would take.  false without a context.  Throws as frontiers does; a point of `from`
    // outside the box is refused by the device library (std::runtime_error).  No map, pose or snapshot changes.
    bool travel(uint32_t particle, double resolution, bool distance_only, const std::vector<Vector2d>& from, const std::vector<Vector2d>& goals,
                sdm::RouteSet& set, const sdm::TravelOptions& options) const;

private:
    std::shared_ptr<HipEngine> eng_;
    lama_hip_ctx* ctx_ = nullptr;
    const char* owner_;
};

} // namespace lama
