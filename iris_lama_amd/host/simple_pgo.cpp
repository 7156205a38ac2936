// simple_pgo.cpp -- lama::SimplePGO::optimize (include/lama/simple_pgo.h): the reference's graph (pgo_graph.hpp), minisam's
// Levenberg-Marquardt (pgo_lm.hpp) over the device-resident linearisation of lama_hip_pgo_* (include/lama_hip.h).  With
// linear_solver = DevicePCG the damped system is solved on the device too (lama_hip_pgo_solve_pcg, _try_solved_step).
#include <string>

#include "lama/simple_pgo.h"
#include "pgo_device.hpp"

namespace lama {

bool SimplePGO::optimize()
{
    report = Report();
    pgo::Graph g;
    if (!pgo::buildGraph(*this, g)) return false;
    const std::string who = "lama::SimplePGO";
    const pgo::PgoApi api = pgo::resolvePgoApi(who, linear_solver == DevicePCG);
    pgo::DeviceSystem sys(api, who, device, g);
    pgo::LmParams prm;
    prm.linear_solver = linear_solver == DevicePCG ? pgo::SOLVER_DEVICE_PCG : pgo::SOLVER_HOST_LDLT;
    prm.pcg_rel_tol = pcg_rel_tol;
    prm.pcg_max_iterations = pcg_max_iterations;
    const pgo::LmResult r = pgo::levenbergMarquardt(sys, prm);
    pgo::fillReport(r, report);
    if (r.status != pgo::SUCCESS) return false;
    std::vector<double> out(4 * (size_t)g.N);
    sys.poses(out.data());
    for (size_t i = 0; i < node_list.size(); ++i) node_list[i].state = SE2d::fromArray(&out[4 * i]);
    return true;
}

} // namespace lama
