// A consumer of lama::SolveBatch (include/lama/nlls/solver.h) written against the public headers only: the matching stage of loop
// closure.  Key scans are rebuilt into a map (lama::MapBuilder2D); one scan is then registered from K candidate poses at once with
// HuberWeight(0.15), one iteration and then up to a hundred, as GraphSlam2D::correlateCandidateScan does for every candidate, and
// the candidates are ranked by MatchSurface2D::error(), which the same launch returns.
// Without a device the constructor throws (no CPU fallback): the program reports that and exits 0.
#include <cmath>
#include <cstdio>
#include <exception>
#include <memory>
#include <vector>

#include "lama/map_builder_2d.h"
#include "lama/match_surface_2d.h"
#include "lama/nlls/solver.h"

static lama::PointCloudXYZ::Ptr room_scan(double x)
{
    lama::PointCloudXYZ::Ptr cloud(new lama::PointCloudXYZ);
    for (int i = 0; i < 360; ++i) {                // an elliptic room (half axes 4 m and 3 m) seen from (x, 0)
        const double a = i * 3.14159265358979 / 180.0, ca = std::cos(a), sa = std::sin(a);
        const double A = ca * ca / 16.0 + sa * sa / 9.0, Bq = x * ca / 16.0, Cq = x * x / 16.0 - 1.0;
        const double r = (-Bq + std::sqrt(Bq * Bq - A * Cq)) / A;
        cloud->points.push_back(lama::Vector3d(r * ca, r * sa, 0.0));
    }
    return cloud;
}

int main()
{
    try {
        lama::MapBuilder2D::Options o;
        o.l2_max = 1.0;
        lama::MapBuilder2D builder(o);
        for (int k = 0; k < 4; ++k) builder.add(room_scan(0.3 * k), lama::Pose2D(0.3 * k, 0.0, 0.0));
        builder.build();
        const lama::DynamicDistanceMap* dm = builder.getDistanceMap();
        if (!dm) { std::printf("no map\n"); return 1; }
        const int K = 5;
        const lama::PointCloudXYZ::Ptr scan = room_scan(0.45);
        std::vector<std::unique_ptr<lama::MatchSurface2D>> owned;
        std::vector<lama::MatchSurface2D*> problems;
        for (int k = 0; k < K; ++k) {
            owned.emplace_back(new lama::MatchSurface2D(dm, scan, lama::Pose2D(0.45 + 0.03 * (k - 2), 0.02 * (k - 2), 0.01 * (k - 2)).state));
            problems.push_back(owned.back().get());
        }
        lama::Solver::Options so;
        so.robust_cost.reset(new lama::HuberWeight(0.15));
        so.max_iterations = 1;
        lama::SolveBatch(so, problems);
        so.max_iterations = 100;
        std::vector<lama::MatrixXd> covs;
        std::vector<uint32_t> iterations;
        std::vector<double> errors;
        lama::SolveBatch(so, problems, &covs, &iterations, &errors);
        bool ok = covs.size() == (size_t)K && errors.size() == (size_t)K;
        double worst = 0.0;
        for (int k = 0; ok && k < K; ++k) {
            const lama::Pose2D p(problems[k]->getState());
            worst = std::fmax(worst, std::fmax(std::fabs(p.x() - 0.45), std::fabs(p.y())));
            ok = ok && errors[k] == problems[k]->error() && covs[k].rows() == 3;
        }
        // lama::Solve keeps its contract: this configuration has no single-problem device kernel
        bool refused = false;
        try { lama::Solve(so, *problems[0]); } catch (const std::invalid_argument&) { refused = true; }
        std::printf("device path ran: candidates %d worst offset %.4f error %.4f iterations %u solve refused %d\n", K, worst, errors[0], iterations[0], (int)refused);
        return (ok && refused && worst < 0.05) ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("no device: %s\n", e.what());
        return 0;
    }
}
