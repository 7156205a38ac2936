"""lama::SimplePGO's host parts without a GPU (tests/pgo_shim.cpp): the sparse block LDL^T and its ordering, the C++
Levenberg-Marquardt loop driven with the CPU oracle's linearisation against the numpy restatement of minisam's (tests/_pgo_lm.py),
and the graph SimplePGO::optimize builds (src/simple_pgo.cpp:48-105 of the reference)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
import _pgo_lm as LM
import iris_lama_amd.ffi as F
from _posegraph import make_graph

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_shim = None


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _lib():
    global _shim
    if _shim is None:
        out = os.path.join(HERE, "cpu_engine", "_build", "libpgo_shim.so")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++14", "-fPIC", "-ffp-contract=off", "-shared", "-I", os.path.join(ROOT, "include"), "-o", out,
                        os.path.join(HERE, "pgo_shim.cpp"), os.path.join(ROOT, "iris_lama_amd", "host", "pose2d.cpp")], check=True)
        L = C.CDLL(out)
        L.shim_ldlt_solve.restype = C.c_int
        L.shim_build_graph.restype = C.c_int
        _shim = L
    return _shim


def _random_block_spd(N, extra, rng):
    """A random SPD matrix on a random lower block pattern (diagonal block first in each row) -> row_ptr, cols, blocks, dense."""
    pairs = set()
    for v in range(1, N):
        pairs.add((v, int(rng.integers(0, v))))
    for _ in range(extra):
        a, b = sorted(rng.choice(N, 2, replace=False))
        pairs.add((int(b), int(a)))
    rows = [[r] + sorted(c for (rr, c) in pairs if rr == r) for r in range(N)]
    row_ptr = np.cumsum([0] + [len(x) for x in rows]).astype(np.int32)
    cols = np.array([c for x in rows for c in x], dtype=np.int32)
    A = np.zeros((3 * N, 3 * N))
    for r, x in enumerate(rows):
        for c in x[1:]:
            A[3 * r:3 * r + 3, 3 * c:3 * c + 3] = rng.normal(size=(3, 3))
    A = A + A.T
    A += np.diag(np.abs(A).sum(axis=1) + rng.uniform(0.1, 1.0, 3 * N))        # diagonally dominant: SPD
    blocks = np.array([A[3 * r:3 * r + 3, 3 * c:3 * c + 3] for r, x in enumerate(rows) for c in x])
    return row_ptr, cols, np.ascontiguousarray(blocks), A


def _solve(row_ptr, cols, blocks, b, natural=False):
    N = len(row_ptr) - 1
    x = np.zeros(3 * N)
    nnz, ms = C.c_uint64(0), C.c_double(0)
    ok = _lib().shim_ldlt_solve(N, _p(row_ptr), _p(cols), _p(blocks), _p(b), _p(x), 1 if natural else 0, C.byref(nnz), C.byref(ms))
    return ok, x, nnz.value


@pytest.mark.parametrize("N,extra,seed", [(1, 0, 0), (7, 5, 1), (60, 150, 2), (300, 900, 3)])
def test_block_ldlt_matches_dense_solve(N, extra, seed):
    rng = np.random.default_rng(seed)
    row_ptr, cols, blocks, A = _random_block_spd(N, extra, rng)
    b = rng.normal(size=3 * N)
    for natural in (False, True):
        ok, x, _ = _solve(row_ptr, cols, blocks, b, natural)
        assert ok == 1
        ref = np.linalg.solve(A, b)
        assert np.allclose(x, ref, rtol=1e-10, atol=1e-12), np.abs(x - ref).max()


def test_block_ldlt_reports_a_zero_pivot():
    rng = np.random.default_rng(5)
    row_ptr, cols, blocks, _ = _random_block_spd(20, 30, rng)
    singular = np.ascontiguousarray(np.zeros_like(blocks))
    for r in range(20):
        singular[row_ptr[r]] = np.eye(3)
    singular[row_ptr[11]][2, 2] = 0.0         # identity system with one zero on the diagonal: the pivot is exactly zero
    ok, _, _ = _solve(row_ptr, cols, singular, np.ones(60))
    assert ok == 0
    singular[row_ptr[11]][2, 2] = np.nan
    ok, _, _ = _solve(row_ptr, cols, singular, np.ones(60))
    assert ok == 0


def _lawnmower(lanes, per_lane):
    """Boustrophedon trajectory: odometry along the path, closures between each pose and its neighbour in the next lane."""
    N = lanes * per_lane
    idx = lambda l, k: l * per_lane + (k if l % 2 == 0 else per_lane - 1 - k)
    fi, fj = [0], [-1]
    for v in range(N - 1):
        fi.append(v); fj.append(v + 1)
    for l in range(lanes - 1):
        for k in range(0, per_lane, 2):
            fi.append(idx(l + 1, k)); fj.append(idx(l, k))
    return N, np.array(fi, dtype=np.int32), np.array(fj, dtype=np.int32)


def test_minimum_degree_ordering_cuts_fill_on_a_lawnmower_graph():
    N, fi, fj = _lawnmower(60, 60)
    rp, cl, _ = LM.lower_pattern(N, fi, fj)
    blocks = np.zeros((len(cl), 3, 3))
    for r in range(N):
        blocks[rp[r]] = np.eye(3) * 10.0
    b = np.ones(3 * N)
    ok_md, x_md, nnz_md = _solve(rp, cl, blocks, b)
    ok_nat, x_nat, nnz_nat = _solve(rp, cl, blocks, b, natural=True)
    assert ok_md == 1 and ok_nat == 1 and np.allclose(x_md, x_nat)
    assert nnz_md < 0.5 * nnz_nat, (nnz_md, nnz_nat)


def _shim_lm(fi, fj, meas, sq, init):
    N, Fn = len(init), len(fi)
    out, st, it, tries, errs = np.zeros((N, 4)), C.c_int32(0), C.c_uint32(0), C.c_uint32(0), np.zeros(2)
    trace = np.zeros(1 << 14, dtype=np.int8)
    _lib().shim_lm(N, _p(np.ascontiguousarray(fi, dtype=np.int32)), _p(np.ascontiguousarray(fj, dtype=np.int32)),
                   _p(np.ascontiguousarray(meas)), _p(np.ascontiguousarray(sq)), Fn, _p(np.ascontiguousarray(init)), _p(out),
                   C.byref(st), C.byref(it), _p(trace), len(trace), C.byref(tries), _p(errs))
    return {"status": st.value, "iterations": it.value, "trace": list(trace[:tries.value]), "poses": out,
            "initial_error": errs[0], "final_error": errs[1]}


@pytest.mark.parametrize("N,loops,seed,fixed", [(40, 20, 3, False), (120, 150, 4, False), (120, 150, 4, True), (300, 400, 6, False)])
def test_cpp_lm_loop_reproduces_minisams_with_the_oracle_linearisation(N, loops, seed, fixed):
    fi0, fj0, meas0, sq0, truth, init = make_graph(N, loops, seed=seed)
    edges = [(int(fi0[k]), int(fj0[k]), meas0[k]) for k in range(N, len(fi0))]
    fx = [(0, init[0]), (N - 1, truth[N - 1])] if fixed else []
    fi, fj, meas, sq = LM.build_graph(init, edges, fx)
    got = _shim_lm(fi, fj, meas, sq, init)
    ref = LM.levenberg_marquardt(fi, fj, meas, sq, init)
    LM.assert_same_run(got, ref)
    # the two solvers (sparse LDL^T under a minimum-degree ordering, dense LU) round differently: the steps agree to about
    # cond(H) * eps, and the loop stops on an error decrease, not on the step -- the poses agree to about 1e-9 m on these graphs
    assert np.abs(got["poses"] - ref["poses"]).max() < 1e-8
    assert abs(got["final_error"] - ref["final_error"]) <= 1e-9 * ref["final_error"]
    assert got["final_error"] < got["initial_error"]


def test_cpp_lm_loop_gives_up_at_the_optimum():
    node = O.se2(0.2, 0.1, -0.4)
    fi, fj, meas, sq = LM.build_graph([node])
    got = _shim_lm(fi, fj, meas, sq, node[None])
    ref = LM.levenberg_marquardt(fi, fj, meas, sq, node[None])
    assert got["status"] == ref["status"] == LM.ERROR_INCREASE and got["iterations"] == 1
    assert got["trace"] == ref["trace"] and len(ref["trace"]) > 3


def _shim_graph(nodes, edges, fixed):
    nodes = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1, 4)
    ef = np.array([e[0] for e in edges], dtype=np.int32); et = np.array([e[1] for e in edges], dtype=np.int32)
    e4 = np.ascontiguousarray(np.array([e[2] for e in edges]).reshape(-1, 4))
    fx = np.array([f[0] for f in fixed], dtype=np.int32); f4 = np.ascontiguousarray(np.array([f[1] for f in fixed]).reshape(-1, 4))
    cap = len(nodes) + len(edges) + len(fixed) + 1
    fi, fj, meas, sq = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros((cap, 4)), np.zeros((cap, 3))
    n = _lib().shim_build_graph(_p(nodes), len(nodes), _p(ef), _p(et), _p(e4), len(edges), _p(fx), _p(f4), len(fixed),
                                _p(fi), _p(fj), _p(meas), _p(sq), cap)
    return None if n < 0 else (fi[:n], fj[:n], meas[:n], sq[:n])


def test_graph_construction_matches_simple_pgo_cpp():
    rng = np.random.default_rng(7)
    nodes = np.stack([O.se2(*rng.normal(0, [3, 3, 1])) for _ in range(12)])
    edges = [(9, 2, O.se2(0.1, 0.2, 0.3)), (3, 8, O.se2(-1, 0.5, -0.2))]          # from > to and from < to
    # no fixed nodes: a prior on node 0 at its own pose, sigmas 1
    fi, fj, meas, sq = _shim_graph(nodes, edges, [])
    assert list(fi) == [0] + list(range(11)) + [9, 3] and list(fj) == [-1] + list(range(1, 12)) + [2, 8]
    assert np.array_equal(meas[0], nodes[0]) and np.array_equal(sq[0], [1.0, 1.0, 1.0])
    for i in range(11):                                                            # node_list[i] - node_list[i+1]
        assert np.array_equal(meas[1 + i], O.se2_mul(O.se2_inverse(nodes[i]), nodes[i + 1]))
        assert np.array_equal(sq[1 + i], [2.0, 2.0, 10.0])
    assert np.array_equal(meas[12], edges[0][2]) and np.array_equal(sq[13], [2.0, 2.0, 10.0])
    ref = LM.build_graph(nodes, edges, [])
    for a, b in zip((fi, fj, meas, sq), ref):
        assert np.array_equal(a, b)
    # fixed nodes: one prior each at the given pose, sigmas 0.1, and none on node 0
    fixed = [(4, O.se2(1, 2, 0.5)), (0, nodes[0])]
    fi, fj, meas, sq = _shim_graph(nodes, edges, fixed)
    assert list(fi[:2]) == [4, 0] and list(fj[:2]) == [-1, -1] and np.array_equal(meas[0], fixed[0][1])
    assert np.allclose(sq[:2], 10.0) and np.array_equal(sq[:2], 1.0 / np.full((2, 3), 0.1)) and len(fi) == 2 + 11 + 2
    # what the reference leaves undefined is refused
    assert _shim_graph(np.zeros((0, 4)), [], []) is None
    assert _shim_graph(nodes, [(3, 12, nodes[0])], []) is None
    assert _shim_graph(nodes, [(3, 3, nodes[0])], []) is None
    assert _shim_graph(nodes, [], [(-1, nodes[0])]) is None


def test_simple_pgo_fails_loudly_without_the_device():
    if F.device_count() > 0:
        pytest.skip("a GPU is present")
    F.use_host_library(None)
    with pytest.raises(F.LamaError, match="no CPU fallback"):
        F.simple_pgo(np.array([[1.0, 0.0, 0.0, 0.0]]))


def test_simple_pgo_has_no_cpu_fallback_in_the_engine_test_double():
    """The test-suite's engine double (tests/cpu_engine) has no pose-graph part: optimize() names the missing entry point."""
    import _testhost
    _testhost.set_engine_library(_testhost.CPU_ENGINE)
    try:
        with pytest.raises(F.LamaError, match="lama_hip_pgo_create missing.*no CPU fallback"):
            F.simple_pgo(np.array([[1.0, 0.0, 0.0, 0.0], [1.0, 0.0, 1.0, 0.0]]))
    finally:
        _testhost.set_engine_library(None)
