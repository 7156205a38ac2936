// lama/nlls/solver.h -- lama::Solver / lama::Solve with the reference's signatures (include/lama/nlls/solver.h:49-85).
//
// What runs where:
//   * a lama::MatchSurface2D problem (the scan-to-map registration of PFSlam2D / Slam2D / Loc2D) with GaussNewton or
//     LevenbergMarquard (default thresholds) and CauchyWeight(0.15) -- the configuration all of the reference's own classes
//     use -- is solved by ONE launch of the fused device solver (lama_hip_match_solve_with: evaluation, robust weights, the
//     3x3 normal equations and the step loop all on the GPU); the covariance follows Solver::calculateCovariance
//     (src/nlls/solver.cpp:133-150) from the weighted J'J the kernel returns;
//   * a MatchSurface2D problem with any other strategy options / weight function is rejected with std::invalid_argument:
//     there is no CPU version of the hot path to fall back to;
//   * MANY MatchSurface2D problems at once go through SolveBatch below: one launch of lama_hip_match_solve_batch solves them side by
//     side, one workgroup each, with any of the five RobustCost classes -- the matching stage of loop closure
//     (GraphSlam2D::correlateCandidateScan: HuberWeight(0.15) on every candidate), the refinement of many localisation candidates;
//   * any other (user-defined) Problem goes through the generic loop of src/nlls/solver.cpp:53-117 on the host: its eval()
//     is the user's code, the solver is glue around it.
#pragma once
#include <cstdint>
#include <vector>

#include "gauss_newton.h"
#include "levenberg_marquardt.h"
#include "problem.h"
#include "robust_cost.h"
#include "strategy.h"

namespace lama {

class Solver {
public:
    struct Options {
        Options();                       // src/nlls/solver.cpp:39-47: 100 iterations, GaussNewton, UnitWeight, quiet
        uint32_t max_iterations;
        Strategy::Ptr strategy;
        RobustCost::Ptr robust_cost;
        bool write_to_stdout;
    };
    Solver(const Options& options = Options()) : options_(options) {}
    void solve(Problem& problem, MatrixXd* cov = 0);
    uint32_t lastIterations() const { return last_iterations_; }

private:
    Options options_;
    uint32_t last_iterations_ = 0;
};

void Solve(const Solver::Options& options, Problem& problem, MatrixXd* cov = 0);

struct MatchSurface2D;

// Solve(options, *problems[b]) for every b in ONE device launch.  Every problem's distance map must live on the same device context
// (maps of different particles of one PFSlam2D are fine); otherwise, or for an empty pointer, std::invalid_argument.  options:
// GaussNewton or LevenbergMarquard at their default thresholds (others: std::invalid_argument, the device loop hard-codes 1e-4) and
// any of UnitWeight / TukeyWeight / TDistributionWeight / CauchyWeight / HuberWeight with any parameter the formula is defined
// for.  The states are written back into the problems.  covs[b] as Solver::solve computes it; iterations[b]; errors[b] =
// problems[b]->error() at the solution, from the same launch.  A problem whose step meets a zero-norm unit complex makes the call
// throw std::runtime_error AFTER the other problems' states and outputs were written.
// The second form gives every problem its own iteration limit (0: evaluate covariance and error at the given state).
void SolveBatch(const Solver::Options& options, const std::vector<MatchSurface2D*>& problems, std::vector<MatrixXd>* covs = nullptr,
                std::vector<uint32_t>* iterations = nullptr, std::vector<double>* errors = nullptr);
void SolveBatch(const Solver::Options& options, const std::vector<MatchSurface2D*>& problems, const std::vector<uint32_t>& max_iterations,
                std::vector<MatrixXd>* covs = nullptr, std::vector<uint32_t>* iterations = nullptr, std::vector<double>* errors = nullptr);

} // namespace lama
