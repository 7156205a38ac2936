"""-m gpu: the per-factor robust losses of the device pose graph (k_pgo_factors_robust, k_pgo_error_robust of
iris_lama_amd/csrc/lama_pgo.h) and lama::PoseGraph2D on the device.  The checks and their bounds are in
tests/_pgo_robust_checks.py, shared with the lane-simulator run of tests/test_robust_pgo_sim.py; here atan2 is OCML's, so a robust
factor's outputs are within K_ROBUST eps of the scales derived there instead of bit-equal, while a loss-free factor keeps the rule
of tests/_pgo_checks.py."""
import os
import subprocess

import numpy as np
import pytest

import _pgo_robust_checks as RC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def F():
    import iris_lama_amd.ffi as f
    if f.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need the MI355X box (there is no CPU fallback)")
    return f


def test_golden_cases_within_the_derived_allowance(F):
    RC.check_golden_cases(F, same_libm=False)


def test_robust_factors_on_both_sides_of_the_block_edge(F):
    RC.check_block_edges(F, same_libm=False)


def test_hub_of_alternating_robust_and_plain_factors_adds_up_in_factor_order(F):
    RC.check_hub(F, same_libm=False)


def test_error_kernel_applies_the_factor_kernels_weight(F):
    RC.check_try_step_equals_the_factor_kernel(F, same_libm=False)


def test_create_robust_without_a_robust_factor_is_create_output_for_output(F):
    RC.check_no_robust_factor_is_create(F)


def test_refused_losses_name_the_factor_and_weights_need_a_linearisation(F):
    RC.check_refusals(F)


@pytest.mark.parametrize("solver", ["ldlt", "pcg"])
def test_optimize_holds_false_closures_back_as_the_numpy_loop_does(F, solver):
    RC.check_ring(F, solver)


def test_invalid_graphs_return_false_with_nothing_run(F):
    RC.check_host_class_refusals(F)


def test_two_identical_runs_are_bitwise_identical(F):
    N, fi, fj, meas, sq, kind, param, init = RC.mixed_graph(300, 500, seed=21)
    outs = []
    for _ in range(2):
        g = F.PoseGraph(N, fi, fj, meas, sq, loss_kind=kind, loss_param=param)
        try:
            lin = g.linearize(init)
            sys = g.linearize_system()
            half, _ = g.try_step(np.full((N, 3), 0.01))
            outs.append([lin[k] for k in ("err", "Hdiag", "Hoff", "b")] + [np.float64(lin["chi2"]), sys["blocks"], np.float64(sys["half_chi2"]),
                                                                          np.float64(half), g.factor_weights()])
        finally:
            g.close()
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
    truth, nodes, factors, true_idx, false_idx = RC.ring_graph()
    with_loss = [f + (("huber", 0.1),) if k >= RC.RING_N else f for k, f in enumerate(factors)]
    for solver in ("ldlt", "pcg"):
        a = F.pose_graph_optimize(nodes, with_loss, solver=solver)
        b = F.pose_graph_optimize(nodes, with_loss, solver=solver)
        assert a[0] and b[0] and np.array_equal(a[1], b[1]) and list(a[2]["trace"]) == list(b[2]["trace"])
        assert np.array_equal(a[2]["weights"], b[2]["weights"]) and a[2]["final_error"] == b[2]["final_error"]


def test_cpp_program_using_pose_graph_2d_header(tmp_path):
    """A consumer of the public header builds the graph the reference's GraphSlam2D optimises -- prior 0.01, chain (0.25, 0.25, 0.15),
    closures under Huber(0.1) -- with one false closure among three, and optimises it on the device."""
    src = tmp_path / "use_pose_graph_2d.cpp"
    src.write_text(CPP_PROGRAM)
    exe = tmp_path / "use_pose_graph_2d"
    lib = os.path.join(ROOT, "iris_lama_amd", "lib")
    subprocess.run(["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib, "-llama_host",
                    "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ok, status, e0, e1, w_true0, w_true1, w_false, nweights = r.stdout.split()
    assert ok == "1" and status == "0" and float(e1) < float(e0) and nweights == "43"
    assert float(w_true0) == 1.0 and float(w_true1) == 1.0 and 0.0 < float(w_false) < 0.5


CPP_PROGRAM = r'''
#include <cmath>
#include <cstdio>
#include "lama/pose_graph_2d.h"
int main()
{
    using lama::Pose2D;
    using lama::Vector3d;
    typedef lama::PoseGraph2D::Loss Loss;
    const int n = 40;
    const double step = 2.0 * M_PI / n;
    lama::PoseGraph2D g;
    // dead reckoning round a ring of radius 5 m with a drifting heading; the true motion turns by `step` per pose
    const Pose2D motion(2.0 * 5.0 * std::sin(0.5 * step) * std::cos(0.5 * step), 2.0 * 5.0 * std::sin(0.5 * step) * std::sin(0.5 * step), step);
    Pose2D p(5.0, 0.0, 0.5 * M_PI);
    for (int i = 0; i < n; ++i) { g.addNode(p); p = p + Pose2D(motion.x() + 0.004, motion.y() - 0.003, step + 0.002); }
    g.addPrior(0, g.nodes[0], Vector3d(0.01, 0.01, 0.01));
    for (int i = 0; i + 1 < n; ++i) g.addBetween(i, i + 1, g.nodes[i] - g.nodes[i + 1], Vector3d(0.25, 0.25, 0.15));
    const Pose2D two = motion + motion;
    g.addBetween(n - 1, 0, motion, Vector3d(1, 1, 1), Loss::Huber(0.1));                  // the ring closes: 39 -> 0 is one true step
    g.addBetween(n - 2, 0, two, Vector3d(1, 1, 1), Loss::Huber(0.1));
    g.addBetween(10, 30, Pose2D(3.0, -2.5, 0.8), Vector3d(1, 1, 1), Loss::Huber(0.1));    // false: 10 -> 30 is half the ring
    const bool ok = g.optimize();
    std::printf("%d %d %.9g %.9g %.17g %.17g %.17g %zu\n", ok ? 1 : 0, g.report.status, g.report.initial_error, g.report.final_error,
                g.weights.size() > 42 ? g.weights[40] : -1.0, g.weights.size() > 42 ? g.weights[41] : -1.0,
                g.weights.size() > 42 ? g.weights[42] : -1.0, g.weights.size());
    return ok && std::isfinite(g.nodes[39].x()) ? 0 : 1;
}
'''
