// pgo_device.hpp -- the device behind the Levenberg-Marquardt loop of pgo_lm.hpp: the pose-graph entry points of the device library
// (lama_hip_pgo_*, include/lama_hip.h) resolved from the engine, and the loop's linearisation interface on top of them.  Shared by
// lama::SimplePGO (simple_pgo.cpp) and lama::PoseGraph2D (pose_graph_2d.cpp); `who` is the class name their messages begin with.
#pragma once

#include <dlfcn.h>

#include <memory>
#include <stdexcept>
#include <string>

#include "hip_engine.hpp"
#include "pgo_graph.hpp"
#include "pgo_lm.hpp"

namespace lama {
namespace pgo {


// The pose-graph entry points, resolved on first use: the engine loader binds the particle-filter C-ABI only (and the engine test
// double of the test-suite has no pose-graph part), so a missing entry point is reported here, by the only caller that needs it.
struct PgoApi {
    decltype(&lama_hip_pgo_create) create = nullptr;
    decltype(&lama_hip_pgo_destroy) destroy = nullptr;
    decltype(&lama_hip_pgo_last_error) last_error = nullptr;
    decltype(&lama_hip_pgo_pattern) pattern = nullptr;
    decltype(&lama_hip_pgo_set_poses) set_poses = nullptr;
    decltype(&lama_hip_pgo_get_poses) get_poses = nullptr;
    decltype(&lama_hip_pgo_linearize_system) linearize_system = nullptr;
    decltype(&lama_hip_pgo_try_step) try_step = nullptr;
    decltype(&lama_hip_pgo_accept) accept = nullptr;
    // optional: only linear_solver = DevicePCG needs them (an implementation of the C-ABI without them still serves the default solver)
    decltype(&lama_hip_pgo_solve_pcg) solve_pcg = nullptr;
    decltype(&lama_hip_pgo_try_solved_step) try_solved_step = nullptr;
    // optional: only a graph with per-factor losses (lama::PoseGraph2D) needs them
    decltype(&lama_hip_pgo_create_robust) create_robust = nullptr;
    decltype(&lama_hip_pgo_factor_weights) factor_weights = nullptr;
    std::shared_ptr<HipEngine> engine;
};

inline PgoApi resolvePgoApi(const std::string& who, bool need_pcg, bool need_robust = false)
{
    PgoApi a;
    a.engine = defaultEngine();
#define RESOLVE(field, sym)                                                                                                  \
    a.field = reinterpret_cast<decltype(a.field)>(a.engine->dl ? dlsym(a.engine->dl, #sym) : nullptr);                     \
    if (!a.field) throw std::runtime_error(who + ": symbol " #sym " missing in " + a.engine->origin +  \
                                           " (the pose-graph optimizer runs on the device; there is no CPU fallback)");
    RESOLVE(create, lama_hip_pgo_create)
    RESOLVE(destroy, lama_hip_pgo_destroy)
    RESOLVE(last_error, lama_hip_pgo_last_error)
    RESOLVE(pattern, lama_hip_pgo_pattern)
    RESOLVE(set_poses, lama_hip_pgo_set_poses)
    RESOLVE(get_poses, lama_hip_pgo_get_poses)
    RESOLVE(linearize_system, lama_hip_pgo_linearize_system)
    RESOLVE(try_step, lama_hip_pgo_try_step)
    RESOLVE(accept, lama_hip_pgo_accept)
#undef RESOLVE
#define OPTIONAL(field, sym)                                                                                                 \
    a.field = reinterpret_cast<decltype(a.field)>(a.engine->dl ? dlsym(a.engine->dl, #sym) : nullptr);                     \
    if (!a.field && need_pcg) throw std::runtime_error(who + ": symbol " #sym " missing in " + a.engine->origin + \
                                                       " (linear_solver = DevicePCG needs it; there is no CPU fallback)");
    OPTIONAL(solve_pcg, lama_hip_pgo_solve_pcg)
    OPTIONAL(try_solved_step, lama_hip_pgo_try_solved_step)
#undef OPTIONAL
#define ROBUST(field, sym)                                                                                                   \
    a.field = reinterpret_cast<decltype(a.field)>(a.engine->dl ? dlsym(a.engine->dl, #sym) : nullptr);                     \
    if (!a.field && need_robust) throw std::runtime_error(who + ": symbol " #sym " missing in " + a.engine->origin +         \
                                                          " (per-factor losses need it; there is no CPU fallback)");
    ROBUST(create_robust, lama_hip_pgo_create_robust)
    ROBUST(factor_weights, lama_hip_pgo_factor_weights)
#undef ROBUST
    return a;
}

// The product implementation of the loop's linearisation: the graph and both pose buffers live on the device.
class DeviceSystem : public System {
public:
    DeviceSystem(const PgoApi& api, const std::string& who, int device, const Graph& g) : api_(api), who_(who), N_(g.N), F_((uint32_t)g.fi.size())
    {
        const int32_t rc = g.loss_kind.empty()
            ? api_.create(device, g.N, g.fi.data(), g.fj.data(), g.meas4.data(), g.sqrt_info3.data(), F_, &h_)
            : api_.create_robust(device, g.N, g.fi.data(), g.fj.data(), g.meas4.data(), g.sqrt_info3.data(), g.loss_kind.data(),
                                 g.loss_param.data(), F_, &h_);
        if (rc != LAMA_HIP_OK || !h_)
            throw std::runtime_error(who_ + ": lama_hip_pgo_create failed (status " + std::to_string(rc) +
                                     "): no usable HIP device; there is no CPU fallback");
        check(api_.set_poses(h_, g.init4.data()));
    }
    ~DeviceSystem() override { if (h_) api_.destroy(h_); }
    DeviceSystem(const DeviceSystem&) = delete;
    DeviceSystem& operator=(const DeviceSystem&) = delete;

    uint32_t numPoses() const override { return N_; }
    void pattern(std::vector<int32_t>& row_ptr, std::vector<int32_t>& cols) override
    {
        uint32_t nnzb = 0;
        check(api_.pattern(h_, nullptr, nullptr, &nnzb));
        row_ptr.resize(N_ + 1);
        cols.resize(nnzb);
        check(api_.pattern(h_, row_ptr.data(), cols.data(), &nnzb));
    }
    double linearize(double* blocks, double* b, double* diag, double* device_ms) override
    {
        double half = 0.0;
        check(api_.linearize_system(h_, blocks, b, diag, &half, device_ms));
        return half;
    }
    double tryStep(const double* dx, double* device_ms) override
    {
        double half = 0.0;
        check(api_.try_step(h_, dx, &half, device_ms));
        return half;
    }
    void accept() override { check(api_.accept(h_)); }
    void solvePcg(double lambda, double rel_tol, uint32_t max_iterations, uint32_t* iterations, int32_t* outcome, double* model_decrease,
                  double* device_ms) override
    {
        check(api_.solve_pcg(h_, lambda, rel_tol, max_iterations, 0, nullptr, iterations, nullptr, outcome, model_decrease, device_ms));
    }
    double trySolvedStep(double* device_ms) override
    {
        double half = 0.0;
        check(api_.try_solved_step(h_, &half, device_ms));
        return half;
    }
    void poses(double* out4) { check(api_.get_poses(h_, out4)); }
    void weights(double* w) { check(api_.factor_weights(h_, w)); }        // of the last linearize()

private:
    void check(int32_t rc)
    {
        if (rc != LAMA_HIP_OK) throw std::runtime_error(who_ + ": " + api_.last_error(h_));
    }
    const PgoApi& api_;
    std::string who_;
    uint32_t N_, F_;
    lama_hip_pgo* h_ = nullptr;
};

// the loop's result as the public report (lama::SimplePGO::Report; lama::PoseGraph2D has the same)
inline void fillReport(const LmResult& r, SimplePGO::Report& report)
{
    report.status = r.status;
    report.iterations = r.iterations;
    report.tries = r.tries;
    report.initial_error = r.initial_error;
    report.final_error = r.final_error;
    report.nnz_L = r.nnz_L;
    report.ms_device_linearize = r.ms_device_linearize;
    report.ms_device_try = r.ms_device_try;
    report.ms_analyze = r.ms_analyze;
    report.ms_factorize = r.ms_factorize;
    report.ms_total = r.ms_total;
    report.pcg_iterations = r.pcg_iterations;
    report.pcg_max_iterations_seen = r.pcg_max_iterations_seen;
    report.pcg_fallbacks = r.pcg_fallbacks;
    report.ms_device_solve = r.ms_device_solve;
    report.trace.assign(r.trace.begin(), r.trace.end());
}

} // namespace pgo
} // namespace lama
