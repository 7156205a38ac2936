// pose_graph_2d.cpp -- lama::PoseGraph2D (include/lama/pose_graph_2d.h): a factor list with per-factor sigmas and robust losses as the
// flat arrays of the device C-ABI (pgo_graph.hpp), then lama::SimplePGO's optimizer unchanged: minisam's Levenberg-Marquardt
// (pgo_lm.hpp) over the device-resident linearisation (pgo_device.hpp, lama_hip_pgo_create_robust).
#include <cmath>
#include <string>

#include "lama/pose_graph_2d.h"
#include "pgo_device.hpp"

namespace lama {
namespace {

// false (and nothing built) for what the header lists: an empty graph, a bad index, a self edge, a bad sigma or loss
bool buildGraph(const PoseGraph2D& p, pgo::Graph& g)
{
    const size_t n = p.nodes.size();
    if (n == 0 || n > 0x7fffffffu || p.factors.empty() || p.factors.size() > 0x7fffffffu) return false;
    for (const auto& f : p.factors) {
        if (f.from < 0 || (size_t)f.from >= n || f.to < -1 || (f.to >= 0 && (size_t)f.to >= n) || f.to == f.from) return false;
        for (int r = 0; r < 3; ++r)
            if (!std::isfinite(f.sigmas[r]) || !(f.sigmas[r] > 0.0)) return false;
        if (f.loss.kind < LAMA_HIP_PGO_LOSS_NONE || f.loss.kind > LAMA_HIP_PGO_LOSS_DCS) return false;
        if (f.loss.kind != LAMA_HIP_PGO_LOSS_NONE && (!std::isfinite(f.loss.param) || !(f.loss.param > 0.0))) return false;
    }
    g = pgo::Graph();
    g.N = (uint32_t)n;
    for (const auto& f : p.factors) {
        g.add(f.from, f.to, f.measurement.state, f.sigmas[0], f.sigmas[1], f.sigmas[2]);
        g.loss_kind.push_back(f.loss.kind);
        g.loss_param.push_back(f.loss.kind == LAMA_HIP_PGO_LOSS_NONE ? 0.0 : f.loss.param);
    }
    g.init4.resize(4 * n);
    for (size_t i = 0; i < n; ++i) p.nodes[i].state.toArray(&g.init4[4 * i]);
    return true;
}

} // namespace

int PoseGraph2D::addNode(const Pose2D& pose)
{
    nodes.push_back(pose);
    return (int)nodes.size() - 1;
}

void PoseGraph2D::addPrior(int node, const Pose2D& measurement, const Vector3d& sigmas, Loss loss)
{
    Factor f;
    f.from = node; f.to = -1; f.measurement = measurement; f.sigmas = sigmas; f.loss = loss;
    factors.push_back(f);
}

void PoseGraph2D::addBetween(int from, int to, const Pose2D& measurement, const Vector3d& sigmas, Loss loss)
{
    Factor f;
    f.from = from; f.to = to; f.measurement = measurement; f.sigmas = sigmas; f.loss = loss;
    factors.push_back(f);
}

bool PoseGraph2D::optimize()
{
    report = Report();
    weights.clear();
    pgo::Graph g;
    if (!buildGraph(*this, g)) return false;
    const std::string who = "lama::PoseGraph2D";
    const pgo::PgoApi api = pgo::resolvePgoApi(who, linear_solver == DevicePCG, true);
    pgo::DeviceSystem sys(api, who, device, g);
    pgo::LmParams prm;
    prm.linear_solver = linear_solver == DevicePCG ? pgo::SOLVER_DEVICE_PCG : pgo::SOLVER_HOST_LDLT;
    prm.pcg_rel_tol = pcg_rel_tol;
    prm.pcg_max_iterations = pcg_max_iterations;
    const pgo::LmResult r = pgo::levenbergMarquardt(sys, prm);
    pgo::fillReport(r, report);
    // the loop linearises before every step, so the weights it left are those of the state before the last one: once more, at the end
    double ms = 0.0;
    sys.linearize(nullptr, nullptr, nullptr, &ms);
    report.ms_device_linearize += ms;
    weights.resize(factors.size());
    sys.weights(weights.data());
    if (r.status != pgo::SUCCESS) return false;
    std::vector<double> out(4 * (size_t)g.N);
    sys.poses(out.data());
    for (size_t i = 0; i < nodes.size(); ++i) nodes[i].state = SE2d::fromArray(&out[4 * i]);
    return true;
}

} // namespace lama
