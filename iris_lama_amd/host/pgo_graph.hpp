// pgo_graph.hpp -- the factor graph lama::SimplePGO::optimize builds (src/simple_pgo.cpp:48-105 of the reference), as the flat
// arrays of the device C-ABI: factor k on poses fi[k], fj[k] (fj = -1: a prior on fi), measurement {c, s, tx, ty}, sqrt_info = 1 / sigma
// (DiagonalLoss::Sigmas, vendor/minisam/minisam/core/LossFunction.cpp:71-74).  lama::PoseGraph2D (pose_graph_2d.cpp) fills the same
// arrays from its own factor list.
#pragma once

#include <cstdint>
#include <vector>

#include "lama/simple_pgo.h"

namespace lama {
namespace pgo {

struct Graph {
    uint32_t N = 0;
    std::vector<int32_t> fi, fj;
    std::vector<double> meas4, sqrt_info3, init4;
    // per-factor robust losses (lama::PoseGraph2D): both empty (what SimplePGO builds: lama_hip_pgo_create), or one entry per factor,
    // LAMA_HIP_PGO_LOSS_* and its parameter (lama_hip_pgo_create_robust)
    std::vector<int32_t> loss_kind;
    std::vector<double> loss_param;
    void add(int32_t i, int32_t j, const SE2d& z, double s0, double s1, double s2)
    {
        fi.push_back(i); fj.push_back(j);
        double m[4];
        z.toArray(m);
        meas4.insert(meas4.end(), m, m + 4);
        const double si[3] = {1.0 / s0, 1.0 / s1, 1.0 / s2};
        sqrt_info3.insert(sqrt_info3.end(), si, si + 3);
    }
};

// false (and nothing built) for an empty node list, an index outside it, or an edge from a node to itself
inline bool buildGraph(const SimplePGO& p, Graph& g)
{
    const size_t n = p.node_list.size();
    if (n == 0 || n > 0x7fffffffu) return false;
    for (const auto& e : p.edge_list)
        if (e.first < 0 || (size_t)e.first >= n || e.second.first < 0 || (size_t)e.second.first >= n || e.first == e.second.first) return false;
    for (const auto& f : p.fixed_list)
        if (f.first < 0 || (size_t)f.first >= n) return false;
    g = Graph();
    g.N = (uint32_t)n;
    if (p.fixed_list.empty()) g.add(0, -1, p.node_list[0].state, 1.0, 1.0, 1.0);        // keep the first pose fixed
    else for (const auto& f : p.fixed_list) g.add(f.first, -1, f.second.state, 0.1, 0.1, 0.1);
    for (size_t i = 0; i + 1 < n; ++i)                                                     // odometry: node_i - node_{i+1}
        g.add((int32_t)i, (int32_t)(i + 1), (p.node_list[i] - p.node_list[i + 1]).state, 0.5, 0.5, 0.1);
    for (const auto& e : p.edge_list)                                                      // loop closures (from > to happens)
        g.add(e.first, e.second.first, e.second.second.state, 0.5, 0.5, 0.1);
    g.init4.resize(4 * n);
    for (size_t i = 0; i < n; ++i) p.node_list[i].state.toArray(&g.init4[4 * i]);
    return true;
}

} // namespace pgo
} // namespace lama
