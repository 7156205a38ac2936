"""lama::SimplePGO on the device (include/lama/simple_pgo.h): the Hessian assembly, the trial steps and the whole
Levenberg-Marquardt loop against the numpy restatement of minisam's (tests/_pgo_lm.py) with the CPU oracle's linearisation."""
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
import _pgo_lm as LM
import iris_lama_amd.ffi as F
from _posegraph import make_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _simple_pgo_inputs(N, loops, seed):
    """A make_graph trajectory as SimplePGO's lists: nodes = the dead-reckoned initial guess, edges = its loop closures."""
    fi, fj, meas, sq, truth, init = make_graph(N, loops, seed=seed)
    edges = [(int(fi[k]), int(fj[k]), meas[k]) for k in range(N, len(fi))]
    return init, edges, truth


def test_assembled_blocks_are_the_factor_order_scatter_of_linearize_bit_for_bit():
    N = 300
    fi, fj, meas, sq, truth, init = make_graph(N, 400, seed=4)
    # repeated pairs in both directions: several factors on one block
    extra = [(5, 17), (17, 5), (5, 17), (200, 3)]
    for a, b in extra:
        fi = np.append(fi, a).astype(np.int32); fj = np.append(fj, b).astype(np.int32)
        meas = np.vstack([meas, O.se2_mul(O.se2_inverse(truth[a]), truth[b])]); sq = np.vstack([sq, [2.0, 2.0, 10.0]])
    g = F.PoseGraph(N, fi, fj, meas, sq)
    lin = g.linearize(init)                       # (also makes init the current state)
    sys = g.linearize_system()
    row_ptr, cols = g.pattern()
    rp, cl, contrib = LM.lower_pattern(N, fi, fj)
    assert np.array_equal(row_ptr, rp) and np.array_equal(cols, cl)
    assert np.array_equal(sys["blocks"], LM.scatter_blocks(lin, cl, contrib, rp))
    assert np.array_equal(sys["b"], lin["b"])
    assert np.array_equal(sys["diag"], np.stack([np.diag(h) for h in lin["Hdiag"]]))
    assert abs(sys["half_chi2"] - 0.5 * lin["chi2"]) <= 1e-12 * lin["chi2"]
    g.close()


def test_try_step_retracts_right_multiplicatively_and_returns_the_error():
    N = 50
    fi, fj, meas, sq, truth, init = make_graph(N, 30, seed=8)
    g = F.PoseGraph(N, fi, fj, meas, sq)
    g.set_poses(init)
    assert np.array_equal(g.get_poses(), init)
    rng = np.random.default_rng(2)
    dx = rng.normal(0, [0.05, 0.05, 0.02], size=(N, 3))
    dx[::7, 2] = 0.0                              # the small-angle branch of SE2 exp (|theta| < 1e-10)
    dx[3::7, 2] = 3e-11
    half, _ = g.try_step(dx)
    g.accept()
    got = g.get_poses()
    expect = LM.retract(init, dx)                 # x * exp(dx): the oracle's statement of SE2d::exp and the renormalising product
    assert np.all(np.abs(got - expect) <= 1e-15 * np.maximum(1.0, np.abs(expect))), np.abs(got - expect).max()
    orc = O.pgo_linearize(got, fi, fj, meas, sq)
    assert abs(half - 0.5 * orc["chi2"]) <= 1e-12 * 0.5 * orc["chi2"]
    # a rejected candidate leaves the current state alone
    g.try_step(np.full((N, 3), 0.3))
    assert np.array_equal(g.get_poses(), got)
    g.close()


@pytest.mark.parametrize("N,loops,with_fixed", [(50, 30, False), (50, 30, True), (500, 600, False), (500, 600, True),
                                                (2000, 3000, False), (2000, 3000, True)])
def test_optimize_follows_minisams_levenberg_marquardt(N, loops, with_fixed):
    nodes, edges, truth = _simple_pgo_inputs(N, loops, seed=N + 7)
    fixed = [(0, nodes[0]), (N // 2, truth[N // 2]), (N - 1, truth[N - 1])] if with_fixed else []
    ok, poses, rep = F.simple_pgo(nodes, edges, fixed)
    fi, fj, meas, sq = LM.build_graph(nodes, edges, fixed)
    ref = LM.levenberg_marquardt(fi, fj, meas, sq, nodes)
    assert ok == (ref["status"] == LM.SUCCESS)
    LM.assert_same_run(rep, ref)
    assert abs(rep["initial_error"] - ref["initial_error"]) <= 1e-10 * ref["initial_error"]
    assert abs(rep["final_error"] - ref["final_error"]) <= 1e-8 * max(ref["final_error"], 1e-12)
    if ok:
        # the sparse LDL^T and the dense solve round differently and the loop stops on an error decrease, not on the step: the
        # poses agree to ~1e-10 of the trajectory's extent (3e-8 m on the 160 m of N = 2000)
        assert np.abs(poses - ref["poses"]).max() < 1e-8 * max(1.0, np.abs(ref["poses"]).max())
        assert rep["final_error"] < rep["initial_error"]
    else:
        assert np.array_equal(poses, nodes)


def test_graph_at_its_optimum_returns_false_after_lambda_runs_out():
    node = O.se2(1.5, -0.5, 0.3)
    fi, fj, meas, sq = LM.build_graph([node])
    assert O.pgo_linearize(node[None], fi, fj, meas, sq)["chi2"] == 0.0
    ok, poses, rep = F.simple_pgo([node])
    ref = LM.levenberg_marquardt(fi, fj, meas, sq, [node])
    assert not ok and rep["status"] == LM.ERROR_INCREASE == ref["status"]
    assert rep["iterations"] == 1 and list(rep["trace"]) == ref["trace"] and set(ref["trace"]) == {LM.REJECTED}
    assert np.array_equal(poses, node[None])


def test_empty_or_invalid_lists_return_false():
    ok, poses, rep = F.simple_pgo(np.zeros((0, 4)))
    assert not ok and rep["status"] == -1 and rep["tries"] == 0
    nodes, edges, truth = _simple_pgo_inputs(10, 3, seed=1)
    for bad_edges, bad_fixed in (([(0, 10, nodes[0])], []), ([(-1, 3, nodes[0])], []), ([], [(12, nodes[0])]), ([(4, 4, nodes[0])], [])):
        ok, poses, rep = F.simple_pgo(nodes, edges + bad_edges, bad_fixed)
        assert not ok and rep["status"] == -1 and np.array_equal(poses, nodes)


def test_two_optimizations_are_bitwise_identical():
    nodes, edges, truth = _simple_pgo_inputs(800, 1200, seed=11)
    a = F.simple_pgo(nodes, edges)
    b = F.simple_pgo(nodes, edges)
    assert a[0] and b[0] and np.array_equal(a[1], b[1]) and list(a[2]["trace"]) == list(b[2]["trace"])


def test_cpp_program_using_simple_pgo_header(tmp_path):
    """A consumer of the public header fills the three lists as the reference's users do and calls optimize() on the device."""
    src = tmp_path / "use_simple_pgo.cpp"
    src.write_text(r'''
#include <cmath>
#include <cstdio>
#include "lama/simple_pgo.h"
int main()
{
    lama::SimplePGO pgo;
    for (int i = 0; i < 40; ++i) pgo.node_list.push_back(lama::Pose2D(0.5 * i + 0.01 * (i % 3), 0.02 * i, 0.01 * i));
    pgo.edge_list.push_back({39, {0, lama::Pose2D(-19.5, 0.0, 0.0)}});
    pgo.edge_list.push_back({10, {30, lama::Pose2D(10.0, 0.0, 0.0)}});
    pgo.fixed_list.push_back({0, lama::Pose2D(0.0, 0.0, 0.0)});
    const bool ok = pgo.optimize();
    std::printf("%d %d %u %.9g %.9g\n", ok ? 1 : 0, pgo.report.status, pgo.report.iterations, pgo.report.initial_error,
                pgo.report.final_error);
    return ok && std::isfinite(pgo.node_list[39].x()) ? 0 : 1;
}
''')
    exe = tmp_path / "use_simple_pgo"
    lib = os.path.join(ROOT, "iris_lama_amd", "lib")
    subprocess.run(["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib, "-llama_host",
                    "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ok, status, iters, e0, e1 = r.stdout.split()
    assert ok == "1" and status == "0" and float(e1) < float(e0)
