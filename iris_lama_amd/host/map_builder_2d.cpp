// map_builder_2d.cpp -- host-side lama::MapBuilder2D (include/lama/map_builder_2d.h); the loop of src/graph_slam2d.cpp:131-164 as
// one device call per build, then the distance map of the occupied cells the way Loc2D::Init builds its map.
#include "lama/map_builder_2d.h"

#include <chrono>
#include <stdexcept>

#include "dm_builder.hpp"
#include "hip_engine.hpp"

namespace lama {

namespace {
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
uint32_t max_sqdist_of(double l2_max, double resolution)
{
    const uint32_t r = (uint32_t)std::ceil(l2_max * (1.0 / resolution));      // DynamicDistanceMap::setMaxDistance, src/sdm/dynamic_distance_map.cpp:149-153
    return r * r;
}
} // namespace

MapBuilder2D::MapBuilder2D(const Options& o) : opt_(o)
{
    const double reach = o.l2_max > 0.0 ? o.l2_max : 0.5;           // (a context always has a distance map; with l2_max == 0 it stays empty)
    std::shared_ptr<HipEngine> eng = defaultEngine(reach, o.resolution);
    if (!eng->map_integrate_scans || !eng->map_occupied_cells)
        throw std::runtime_error("lama::MapBuilder2D: the device library " + eng->origin + " has no lama_hip_map_integrate_scans");
    lama_hip_cfg cfg;
    eng->default_cfg(&cfg);
    cfg.particles = 1;
    cfg.resolution = o.resolution; cfg.patch_size = o.patch_size; cfg.l2_max = reach; cfg.device = o.gpu_device;
    if (o.window_patches) cfg.window_patches = o.window_patches;
    if (o.dm_patch_capacity) cfg.dm_patch_capacity = o.dm_patch_capacity;
    if (o.occ_patch_capacity) cfg.occ_patch_capacity = o.occ_patch_capacity;
    dev_.create(std::move(eng), cfg);
}

MapBuilder2D::~MapBuilder2D() = default;

size_t MapBuilder2D::add(const PointCloudXYZ::Ptr& cloud, const Pose2D& pose)
{
    if (!cloud) throw std::invalid_argument("lama::MapBuilder2D::add: null cloud");
    const PointCloudXYZ& s = *cloud;
    if ((uint64_t)offsets_.back() + s.points.size() > 0x7FFFFFFFull) throw std::length_error("lama::MapBuilder2D::add: more than 2^31 - 1 points");
    for (const Vector3d& p : s.points) { pts_.push_back(p.x()); pts_.push_back(p.y()); pts_.push_back(p.z()); }
    offsets_.push_back(offsets_.back() + (uint32_t)s.points.size());
    origins_.push_back(s.sensor_origin_.x()); origins_.push_back(s.sensor_origin_.y()); origins_.push_back(s.sensor_origin_.z());
    quats_.push_back(s.sensor_orientation_.w()); quats_.push_back(s.sensor_orientation_.x()); quats_.push_back(s.sensor_orientation_.y()); quats_.push_back(s.sensor_orientation_.z());
    poses_.push_back(pose);
    return poses_.size() - 1;
}

void MapBuilder2D::setPose(size_t key, const Pose2D& pose)
{
    poses_.at(key) = pose;
    if (key < built_) stale_ = true;
}

void MapBuilder2D::setPoses(const std::vector<Pose2D>& poses)
{
    if (poses.size() != poses_.size()) throw std::invalid_argument("lama::MapBuilder2D::setPoses: one pose per key");
    poses_ = poses;
    if (built_ > 0) stale_ = true;
}

void MapBuilder2D::reset()
{
    poses_.clear(); pts_.clear(); origins_.clear(); quats_.clear(); offsets_.assign(1, 0u); occupied_.clear();
    occ_view_.reset(); dm_view_.reset();
    if (has_map_) {                                               // an upload of no patches empties the map (Map::read of an empty file)
        dev_.check(dev_->pf_upload_map(dev_.get(), 0, LAMA_HIP_MAP_OCCUPANCY, 0, nullptr, nullptr, nullptr), "lama_hip_pf_upload_map (reset)");
        dev_.check(dev_->pf_upload_map(dev_.get(), 0, LAMA_HIP_MAP_DISTANCE, 0, nullptr, nullptr, nullptr), "lama_hip_pf_upload_map (reset)");
    }
    built_ = 0; stale_ = false; has_map_ = false;
}

void MapBuilder2D::build()
{
    occ_view_.reset(); dm_view_.reset();
    timing_ = Timing();
    double t0 = now_ms();
    if (stale_) {                                                 // poses of integrated keys changed: start from an empty occupancy map
        dev_.check(dev_->pf_upload_map(dev_.get(), 0, LAMA_HIP_MAP_OCCUPANCY, 0, nullptr, nullptr, nullptr), "lama_hip_pf_upload_map (rebuild)");
        built_ = 0; stale_ = false;
    }
    const size_t K = poses_.size() - built_;
    if (K > 0) {
        std::vector<double> p4(4 * K);
        for (size_t k = 0; k < K; ++k) poses_[built_ + k].state.toArray(&p4[4 * k]);
        const uint32_t flags = (opt_.full ? LAMA_HIP_MAP_BUILD_FULL : 0u) | (opt_.prune ? LAMA_HIP_MAP_BUILD_PRUNE : 0u);
        dev_.check(dev_->map_integrate_scans(dev_.get(), 0, (uint32_t)K, p4.data(), pts_.data(), offsets_.data() + built_, origins_.data() + 3 * built_,
                                             quats_.data() + 4 * built_, flags), "lama_hip_map_integrate_scans");
        built_ = poses_.size();
        has_map_ = true;
    }
    double t1 = now_ms();
    timing_.integrate_ms = t1 - t0;
    if (!(opt_.l2_max > 0.0) || !has_map_) return;
    // the distance map of the occupied cells: addObstacle for each + update() on an empty map
    uint32_t n = 0;
    dev_.check(dev_->map_occupied_cells(dev_.get(), 0, 0, nullptr, &n), "lama_hip_map_occupied_cells");
    occupied_.assign(2 * (size_t)n, 0u);
    if (n) dev_.check(dev_->map_occupied_cells(dev_.get(), 0, n, occupied_.data(), &n), "lama_hip_map_occupied_cells");
    double t2 = now_ms();
    timing_.occupied_ms = t2 - t1;
    dev_.check(dev_->pf_upload_map(dev_.get(), 0, LAMA_HIP_MAP_DISTANCE, 0, nullptr, nullptr, nullptr), "lama_hip_pf_upload_map (distance map)");
    if (n) {
        bool host_built = false; uint32_t processed = 0; const char* what = "";
        const int32_t rc = detail::add_obstacles_to_map(*dev_.engine(), dev_.get(), occupied_.data(), n, opt_.resolution, opt_.patch_size,
                                                        max_sqdist_of(opt_.l2_max, opt_.resolution), host_built, processed, what);
        dev_.check(rc, what);
    }
    timing_.distance_ms = now_ms() - t2;
}

bool MapBuilder2D::downloadOccupancyMap(sdm::HostMap& m) const
{
    m.kind = sdm::kFrequencyOccupancyMap; m.resolution = opt_.resolution;
    return has_map_ && dev_.download(0, LAMA_HIP_MAP_OCCUPANCY, m.ids, m.cells, m.masks);
}

bool MapBuilder2D::downloadDistanceMap(sdm::HostMap& m) const
{
    if (!(opt_.l2_max > 0.0)) return false;
    m.kind = sdm::kDistanceMap; m.resolution = opt_.resolution; m.max_sqdist = max_sqdist_of(opt_.l2_max, opt_.resolution);
    return has_map_ && dev_.download(0, LAMA_HIP_MAP_DISTANCE, m.ids, m.cells, m.masks);
}

const FrequencyOccupancyMap* MapBuilder2D::getOccupancyMap() const
{
    if (!occ_view_) {
        sdm::HostMap m;
        if (!downloadOccupancyMap(m)) return nullptr;
        occ_view_.reset(new FrequencyOccupancyMap(std::move(m)));
    }
    return occ_view_.get();
}

const DynamicDistanceMap* MapBuilder2D::getDistanceMap() const
{
    if (!dm_view_) {
        sdm::HostMap m;
        if (!downloadDistanceMap(m)) return nullptr;
        dm_view_.reset(new DynamicDistanceMap(std::move(m)));
        dm_view_->bindDevice(dev_.engine(), dev_.get(), 0u);
    }
    return dm_view_.get();
}

} // namespace lama
