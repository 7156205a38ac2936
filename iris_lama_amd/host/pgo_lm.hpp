// pgo_lm.hpp -- the Levenberg-Marquardt loop of lama::SimplePGO: minisam's LevenbergMarquardtOptimizer with its default parameters
// and the Cholesky (lower Hessian) linear solver, restated over a small linearisation interface.  The product implementation of the
// interface is the device (simple_pgo.cpp, lama_hip_pgo_*); the test-suite drives the same loop with the CPU oracle.
//
// Reference lines (vendor/minisam/minisam/nonlinear/):
//   parameters        NonlinearOptimizer.h:54-60, LevenbergMarquardtOptimizer.h:20-36, reset() LevenbergMarquardtOptimizer.cpp:35-44
//   outer loop        NonlinearOptimizer.cpp:175-233, stop test :237-240
//   one iteration     LevenbergMarquardtOptimizer.cpp:56-157 (undamped hessian_diag, tries while lambda < lambda_max)
//   one try           :160-262 (gain ratio, NaN = rejection), damping :265-318 + :369-374 (H_ii += (lambda - lambda_last) diag_i,
//                     incremental within one iteration), lambda rules :321-333
//   linear solver     linear/SparseCholesky.cpp (analysed once per optimize, factorised per try, NumericalIssue -> RANK_DEFICIENCY)
//
// Not in the reference: LmParams::linear_solver = SOLVER_DEVICE_PCG solves the damped system behind the interface (System::solvePcg,
// the device's block-Jacobi conjugate gradient) and forms the gain ratio from the model decrease it returns; nothing is analysed or
// factorised unless a solve reaches its iteration cap, in which case that try goes to the LDL^T below.
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "block_ldlt.hpp"

namespace lama {
namespace pgo {

// NonlinearOptimizationStatus (NonlinearOptimizer.h:69-75)
enum Status : int32_t { SUCCESS = 0, MAX_ITERATION = 1, ERROR_INCREASE = 2, RANK_DEFICIENCY = 3, INVALID = 4 };

// Outcome of one damped try, in the order they were made
enum TryOutcome : int8_t { TRY_REJECTED = 0, TRY_ACCEPTED = 1, TRY_RANK_DEFICIENT = 2 };

// What the loop needs from a linearisation of the graph.  The state lives behind the interface (the device keeps it resident).
struct System {
    virtual ~System() {}
    virtual uint32_t numPoses() const = 0;
    // lower block-CSR pattern of the Hessian (pgo_pattern.hpp)
    virtual void pattern(std::vector<int32_t>& row_ptr, std::vector<int32_t>& cols) = 0;
    // at the current state: blocks [nnzb][9], b = -J^T e [3N], undamped diagonal [3N]; returns 0.5 sum ||e||^2
    virtual double linearize(double* blocks, double* b, double* diag, double* device_ms) = 0;
    // candidate = current * exp(dx); returns 0.5 sum ||e||^2 at the candidate
    virtual double tryStep(const double* dx, double* device_ms) = 0;
    // the candidate becomes the current state
    virtual void accept() = 0;
    // ---- SOLVER_DEVICE_PCG only (an implementation without them cannot be asked for that solver)
    // (H + lambda diag) dx = b of the last linearize(), solved behind the interface; the solution stays there.  outcome: PcgOutcome;
    // model_decrease = 0.5 dx . (lambda diag dx + b)
    virtual void solvePcg(double /*lambda*/, double /*rel_tol*/, uint32_t /*max_iterations*/, uint32_t* /*iterations*/, int32_t* /*outcome*/,
                          double* /*model_decrease*/, double* /*device_ms*/)
    {
        throw std::runtime_error("lama::pgo::System: this linearisation has no device solver (solvePcg not supported)");
    }
    // tryStep with that solution
    virtual double trySolvedStep(double* /*device_ms*/)
    {
        throw std::runtime_error("lama::pgo::System: this linearisation has no device solver (trySolvedStep not supported)");
    }
};

enum LinearSolverKind : int32_t { SOLVER_HOST_LDLT = 0, SOLVER_DEVICE_PCG = 1 };
enum PcgOutcome : int32_t { PCG_CONVERGED = 0, PCG_CAP = 1, PCG_BREAKDOWN = 2 };     // LAMA_HIP_PCG_* (include/lama_hip.h)

struct LmParams {
    uint32_t max_iterations = 100;
    double min_rel_err_decrease = 1e-5, min_abs_err_decrease = 1e-5;
    double lambda_init = 1e-5, lambda_increase_factor_init = 2.0, lambda_increase_factor_update = 2.0;
    double lambda_decrease_factor_min = 1.0 / 3.0, lambda_min = 1e-20, lambda_max = 1e10, gain_ratio_thresh = 1e-3;
    int32_t linear_solver = SOLVER_HOST_LDLT;
    double pcg_rel_tol = 1e-10;
    uint32_t pcg_max_iterations = 0;                            // 0: max(100, 6 N)
};

struct LmResult {
    Status status = INVALID;
    uint32_t iterations = 0, tries = 0;
    double initial_error = 0.0, final_error = 0.0;
    uint64_t nnz_L = 0;
    double ms_device_linearize = 0.0, ms_device_try = 0.0;     // device time of the kernels
    double ms_analyze = 0.0, ms_factorize = 0.0;              // host: ordering + symbolic, numeric factorisation + solve
    double ms_total = 0.0;
    std::vector<int8_t> trace;                                 // TryOutcome per try
    // SOLVER_DEVICE_PCG
    uint64_t pcg_iterations = 0;                               // summed over the tries
    uint32_t pcg_max_iterations_seen = 0, pcg_fallbacks = 0;   // the longest solve; tries that hit the cap and went to the LDL^T
    double ms_device_solve = 0.0;
};

inline double msSince(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

inline LmResult levenbergMarquardt(System& sys, const LmParams& prm = LmParams(), bool natural_order = false)
{
    typedef std::chrono::steady_clock clock;
    const auto t_start = clock::now();
    LmResult res;
    const uint32_t N = sys.numPoses();
    std::vector<int32_t> row_ptr, cols;
    sys.pattern(row_ptr, cols);
    const size_t nnzb = cols.size();
    const bool pcg = prm.linear_solver == SOLVER_DEVICE_PCG;
    const uint32_t pcg_cap = prm.pcg_max_iterations ? prm.pcg_max_iterations : std::max<uint32_t>(100u, 6u * N);
    BlockLDLT ldlt;
    bool analyzed = false;
    auto t0 = clock::now();
    const auto analyze = [&]() {                               // (up front for the LDL^T; on first need for a fallback try of the PCG)
        t0 = clock::now();
        ldlt.analyze((int32_t)N, row_ptr.data(), cols.data(), natural_order);
        res.ms_analyze = msSince(t0);
        res.nnz_L = ldlt.nnzL();
        analyzed = true;
    };
    if (!pcg) analyze();
    std::vector<double> blocks, H, b, diag, dx;
    const auto host_arrays = [&]() { blocks.resize(9 * nnzb); H.resize(9 * nnzb); b.resize(3 * (size_t)N); diag.resize(3 * (size_t)N); dx.resize(3 * (size_t)N); };
    if (!pcg) host_arrays();

    double lambda = prm.lambda_init, increase = prm.lambda_increase_factor_init;
    double last_err = 0.0;
    bool have_err = false;
    res.iterations = 0;
    while (res.iterations < prm.max_iterations) {
        // ---- iterate(): linearise once
        double ms = 0.0;
        const double lin_err = pcg ? sys.linearize(nullptr, nullptr, nullptr, &ms) : sys.linearize(blocks.data(), b.data(), diag.data(), &ms);
        res.ms_device_linearize += ms;
        if (!have_err) { last_err = lin_err; res.initial_error = lin_err; have_err = true; }   // 0.5 errorSquaredNorm(init)
        const double values_curr_err = last_err;
        if (!pcg) H = blocks;
        bool on_host = !pcg;                                       // this iteration's system is in blocks / b / diag / H
        double last_lambda = 0.0;
        Status it_status = ERROR_INCREASE;
        double new_err = 0.0;
        while (lambda < prm.lambda_max) {
            if (pcg) {
                uint32_t its = 0;
                int32_t outcome = PCG_BREAKDOWN;
                double model = 0.0;
                ms = 0.0;
                sys.solvePcg(lambda, prm.pcg_rel_tol, pcg_cap, &its, &outcome, &model, &ms);
                res.ms_device_solve += ms;
                res.pcg_iterations += its;
                res.pcg_max_iterations_seen = std::max(res.pcg_max_iterations_seen, its);
                if (outcome != PCG_CAP) {
                    ++res.tries;
                    bool accepted = false;
                    if (outcome == PCG_CONVERGED) {
                        ms = 0.0;
                        const double err_upd = sys.trySolvedStep(&ms);
                        res.ms_device_try += ms;
                        const double ratio = (values_curr_err - err_upd) / model;
                        if (ratio > prm.gain_ratio_thresh) {            // (a NaN ratio is a rejection)
                            sys.accept();
                            new_err = err_upd;
                            accepted = true;
                            lambda *= std::max(prm.lambda_decrease_factor_min, 1.0 - std::pow(2.0 * ratio - 1.0, 3.0));
                            lambda = std::max(prm.lambda_min, lambda);
                            increase = prm.lambda_increase_factor_init;
                        }
                    }
                    res.trace.push_back(accepted ? TRY_ACCEPTED : outcome == PCG_CONVERGED ? TRY_REJECTED : TRY_RANK_DEFICIENT);
                    if (accepted) { it_status = SUCCESS; break; }
                    lambda *= increase;
                    increase *= prm.lambda_increase_factor_update;
                    continue;
                }
                // the cap: this try is the host's.  The system is downloaded once per iteration (the same kernels at the same state
                // give the same numbers), the ordering is made on first need.
                ++res.pcg_fallbacks;
                if (!analyzed) analyze();
                if (!on_host) {
                    host_arrays();
                    ms = 0.0;
                    sys.linearize(blocks.data(), b.data(), diag.data(), &ms);
                    res.ms_device_linearize += ms;
                    H = blocks;
                    last_lambda = 0.0;
                    on_host = true;
                }
            }
            // dumpLinearSystem_: H.diagonal() += (lambda - last_lambda) * hessian_diag
            const double dl = lambda - last_lambda;
            for (uint32_t v = 0; v < N; ++v) {
                double* D = &H[9 * (size_t)row_ptr[v]];            // (the diagonal block leads its row)
                for (int t = 0; t < 3; ++t) D[4 * t] += dl * diag[3 * (size_t)v + t];
            }
            last_lambda = lambda;
            ++res.tries;
            t0 = clock::now();
            const bool ok = ldlt.factorize(H.data());
            if (ok) ldlt.solve(b.data(), dx.data());
            res.ms_factorize += msSince(t0);
            bool accepted = false;
            if (ok) {
                ms = 0.0;
                const double err_upd = sys.tryStep(dx.data(), &ms);
                res.ms_device_try += ms;
                const double nonlinear = values_curr_err - err_upd;
                double dot = 0.0;
                for (size_t q = 0; q < dx.size(); ++q) dot += dx[q] * (lambda * diag[q] * dx[q] + b[q]);
                const double linear = 0.5 * dot;
                const double ratio = nonlinear / linear;
                if (ratio > prm.gain_ratio_thresh) {                // (a NaN ratio is a rejection)
                    sys.accept();
                    new_err = err_upd;
                    accepted = true;
                    // decreaseLambda_
                    lambda *= std::max(prm.lambda_decrease_factor_min, 1.0 - std::pow(2.0 * ratio - 1.0, 3.0));
                    lambda = std::max(prm.lambda_min, lambda);
                    increase = prm.lambda_increase_factor_init;
                }
            }
            res.trace.push_back(accepted ? TRY_ACCEPTED : ok ? TRY_REJECTED : TRY_RANK_DEFICIENT);
            if (accepted) { it_status = SUCCESS; break; }
            // increaseLambda_ (RANK_DEFICIENCY and ERROR_INCREASE alike)
            lambda *= increase;
            increase *= prm.lambda_increase_factor_update;
        }
        ++res.iterations;
        if (it_status != SUCCESS) { res.status = it_status; res.final_error = last_err; res.ms_total = msSince(t_start); return res; }
        const double curr_err = new_err;
        res.final_error = curr_err;
        if (curr_err - last_err > 1e-20) { res.status = ERROR_INCREASE; res.ms_total = msSince(t_start); return res; }
        if ((last_err - curr_err) < prm.min_abs_err_decrease || (last_err - curr_err) / last_err < prm.min_rel_err_decrease) {
            res.status = SUCCESS;
            res.ms_total = msSince(t_start);
            return res;
        }
        last_err = curr_err;
    }
    res.status = MAX_ITERATION;
    res.ms_total = msSince(t_start);
    return res;
}

} // namespace pgo
} // namespace lama
