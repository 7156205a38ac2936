// lama/loc2d.h -- host-side lama::Loc2D (localisation on a fixed map) on the MI355X path.
//
// Same class name, Options fields and public methods as the reference's include/lama/loc2d.h:47-165; update()
// follows src/loc2d.cpp:126-192.  The public members `occupancy_map` / `distance_map` have the reference's types
// (include/lama/loc2d.h:103-104): consumers (iris_lama_ros' loc2d_ros) fill them cell by cell before the first update.
// The SimpleOccupancyMap is a plain host map; the DynamicDistanceMap is LIVE: addObstacle() buffers cells on the host,
// update() runs DynamicDistanceMap::addObstacle + update() on the device, queries read a snapshot downloaded on first use
// (lama/sdm_maps.h).  On the device: scan matching with covariance
// (Solve(..., &cov)) and the RMSE (lama_hip_match_solve), the candidate evaluation of globalLocalization (:249-286,
// lama_hip_eval_batch; the candidates are drawn on the host from lama::random like the reference) and the likelihood
// samples of addSamplingCovariance (:199-247, lama_hip_map_sample_likelihood); strategy "lm" = Levenberg-Marquardt in the
// same kernel (cfg.solver_strategy).
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "correlative_search_2d.h"
#include "device_context.h"
#include "pose2d.h"
#include "sdm/dynamic_distance_map.h"
#include "sdm/grid.h"
#include "sdm/ray_cast.h"
#include "sdm/simple_occupancy_map.h"
#include "sdm/travel.h"

namespace lama {

class Loc2D {
public:
    struct Options {
        Options();
        double trans_thresh, rot_thresh, l2_max, resolution;
        uint32_t patch_size, max_iter;
        std::string strategy;
        uint32_t gloc_particles, gloc_iters;
        double gloc_thresh, cov_blend;
        int32_t gpu_device = 0;      // addition
    };

    SimpleOccupancyMap* occupancy_map = nullptr;      // include/lama/loc2d.h:103-104
    DynamicDistanceMap* distance_map = nullptr;

    Loc2D() = default;
    void Init(const Options& options = Options());
    virtual ~Loc2D();

    bool enoughMotion(const Pose2D& odometry);
    bool update(const PointCloudXYZ::Ptr& surface, const Pose2D& odometry, double timestamp, bool force_update = false);
    void triggerGlobalLocalization();
    // An addition (the reference has none): global localisation by exhaustive search instead of random samples.  The scan is scored at
    // every node of a pose lattice over occupancy_map's bounds() on the device (lama::CorrelativeSearch2D on this object's own
    // context); tile winners whose node is not a FREE cell of occupancy_map are dropped, as the reference draws its candidates from
    // free cells only (a tile keeps one node: a free node that scored behind a non-free one of its tile is not seen); the rest are
    // selected and refined as CorrelativeSearch2D::search does.  If the best candidate's rmse (MatchSurface2D::error()) is below
    // Options::gloc_thresh the pose is set as setPose() sets it and true is returned; otherwise nothing of the object changes.
    // triggerGlobalLocalization() / update() keep the reference's behaviour.
    bool relocalize(const PointCloudXYZ::Ptr& surface, const CorrelativeSearch2D::Options& options = CorrelativeSearch2D::Options());
    // the candidates of the last relocalize(), best first (instrumentation, like lastGlocPoses)
    const std::vector<CorrelativeSearch2D::Candidate>& lastRelocalizeCandidates() const { return reloc_; }
    void setPose(const Pose2D& pose) { pose_ = pose; has_first_scan = false; }
    const Pose2D& getPose() const { return pose_; }
    const Matrix3d& getCovar() const { return cov_; }     // Eigen::Matrix3d when Eigen is available (lama/types.h)
    double getRMSE() const { return rmse_; }
    bool globalLocalizationIsActive() const { return do_global_localization_; }
    // candidates and errors of the last globalLocalization call (instrumentation for the parity tests)
    const std::vector<double>& lastGlocPoses() const { return gloc_poses_; }
    const std::vector<double>& lastGlocErrors() const { return gloc_errors_; }
    const std::vector<double>& lastSamplingLikelihoods() const { return sampling_l_; }
    uint32_t getLastIterations() const { return last_iterations_; }
    // true when the first build of the distance map was replayed on the host and uploaded (iris_lama_amd/host/dm_builder.hpp)
    bool distanceMapBuiltOnHost() const { return host_built_; }
    // Dense grid of the DEVICE distance map, made on the device (lama/sdm/grid.h); false while there is no device map yet.
    // (occupancy_map is a host map: walk it on the host.  For the same reason there is no getFrontiers() here: lama/sdm/frontier.h
    // works on a DEVICE occupancy map, which Loc2D does not have.)
    bool getDistanceGrid(sdm::DistanceGrid& grid, const sdm::GridOptions& options = sdm::GridOptions()) const
    { return dev_ && dev_.distanceGrid(0, opt_.resolution, opt_.l2_max, grid, options); }
    // What a sensor at each of `poses` would see in the DEVICE distance map (lama/sdm/ray_cast.h; the occupancy map is a host map, so
    // options.map must be kRayDistanceMap: a beam stops at the first obstacle cell).  Obstacles added since the last update() are
    // brought in first.  false while there is no device map yet.
    bool castRays(const std::vector<Pose2D>& poses, const PointCloudXYZ::Ptr& surface, sdm::RayCastResult& result,
                  const sdm::RayCastOptions& options = distanceRays());
    // The scan checked against the map at the current pose, one RayLabel per point: kRayAgrees (it ends within tolerance_cells of a
    // mapped obstacle), kRayBlocked (it passes through a mapped obstacle more than tolerance_cells before its end: the pose is off or
    // the map is stale), kRayNovel (it ends where the map has nothing: a person, a moved pallet -- points to drop before matching).
    // Empty while there is no device map yet.
    std::vector<uint8_t> checkScan(const PointCloudXYZ::Ptr& surface, int32_t tolerance_cells = 2);
    // Routes over the floor plan (lama/sdm/travel.h) from the world points `from` to each of `goals`, relaxed on the device.  The
    // DISTANCE map alone decides what is traversable (occupancy_map is a host map): a pixel at least the robot's radius away from every
    // obstacle is, and a cell the distance map does not hold counts as max_distance away -- there is no "unknown" here, so bound the box
    // with TravelOptions::world_min / world_max where the plan's outside must not be driven through.  Obstacles added since the last
    // update() are brought in first.  false while there is no device map yet.
    bool planRoutes(const std::vector<Vector2d>& from, const std::vector<Vector2d>& goals, sdm::RouteSet& set, const sdm::TravelOptions& options = sdm::TravelOptions());
    static sdm::RayCastOptions distanceRays() { sdm::RayCastOptions o; o.map = sdm::kRayDistanceMap; return o; }
    lama_hip_ctx* deviceContext() const { return dev_.get(); }
    const HipEngine* engine() const { return dev_.engine().get(); }

private:
    void ensureContext();
    void solve(const PointCloudXYZ& surface, bool do_solve);
    void globalLocalization(const PointCloudXYZ& surface);
    void addSamplingCovariance(const PointCloudXYZ& surface);

    Options opt_;
    DeviceContext dev_{"lama::Loc2D"};       // outlives distance_map, whose writer works on it (deleted in the destructor's body)
    Pose2D odom_, pose_;
    Matrix3d cov_;
    double rmse_ = 0.0;
    bool has_first_scan = false;
    uint32_t last_iterations_ = 0;
    bool host_built_ = false;
    bool do_global_localization_ = false;
    uint32_t gloc_cur_iter_ = 0;
    double cov_blend_ = 0.0;
    std::vector<Vector2d> sampling_steps_;
    std::vector<double> gloc_poses_, gloc_errors_, sampling_l_;
    std::vector<CorrelativeSearch2D::Candidate> reloc_;
};

} // namespace lama
