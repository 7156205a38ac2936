"""Checks of the device solver of SimplePGO's damped system (iris_lama_amd/csrc/lama_pgo_pcg.h: lama_hip_pgo_solve_pcg,
lama_hip_pgo_try_solved_step) and of the whole Levenberg-Marquardt loop over it, shared by tests/test_pgo_pcg_sim.py (the lane
simulator of tests/sim, no GPU) and tests/test_pgo_pcg_gpu.py.

Every kernel check linearises a graph on the device, solves, and compares with the numpy restatement tests/_pgo_pcg.py fed with the
DOWNLOADED system: dx, the iteration count, r.r / b.b and the model decrease are BIT-EQUAL on the simulator and on the GPU alike -- the
solver holds +, -, *, / and comparisons only, in a fixed order.  Unless a check says otherwise it also asserts the true residual
||(H + lam D) dx - b|| <= 10 rel_tol ||b|| at rel_tol = 1e-10, computed in numpy from the downloaded blocks: the recurrence's residual
stops at 1.0 rel_tol, a plain numpy PCG's true residual stayed at or below 1.0 rel_tol on these graphs, the factor 10 is the margin
for another order of the sums.

The whole-loop checks compare lama::SimplePGO with linear_solver = DevicePCG against the numpy Levenberg-Marquardt of tests/_pgo_lm.py
(a dense direct solve): the same status, iteration count and accept / reject trace (LM.assert_same_run); initial error within 1e-10
relative; final error within 1e-7 relative (the numpy PCG inside that loop differed by at most 5e-10, from the loop's stop rule of
1e-5, not from the solver's tolerance); poses within 1e-8 max(1, extent), the bound of _pgo_checks.check_loop.
"""
import ctypes as C

import numpy as np

import _oracle as O
import _pgo_checks as P
import _pgo_lm as LM
import _pgo_pcg as R
from _posegraph import make_graph

REL_TOL = 1e-10
LAMBDA = 1e-5                 # LevenbergMarquardtOptimizer's first lambda
E_INVALID, E_STATE = -1, -5   # include/lama_hip.h


def perturbed(poses, seed, sigma=(0.05, 0.05, 0.02)):
    """the poses moved off whatever optimum they sit in, so that b is far from zero"""
    dx = np.random.default_rng(seed).normal(0, sigma, size=(len(poses), 3))
    return LM.retract(np.asarray(poses), dx)


def quick_graph(N, loops, seed):
    """A make_graph-shaped graph built with array operations (the large pose counts): prior on pose 0, odometry, `loops` closures
    between poses at most 200 apart in both directions; -> fi, fj, meas, sq, poses (the truth moved by noise)"""
    rng = np.random.default_rng(seed)
    th = np.cumsum(rng.normal(0, 0.15, N))
    xy = np.cumsum(np.stack([0.5 * np.cos(th), 0.5 * np.sin(th)], axis=1), axis=0)
    a = rng.integers(0, N - 2, loops)
    bnd = np.minimum(N, a + 200)
    b = a + 2 + (rng.random(loops) * (bnd - a - 2)).astype(np.int64)
    swap = rng.random(loops) < 0.5
    a, b = np.where(swap, b, a), np.where(swap, a, b)
    fi = np.concatenate([[0], np.arange(N - 1), a]).astype(np.int32)
    fj = np.concatenate([[-1], np.arange(1, N), b]).astype(np.int32)

    def se2(x, y, t):
        return np.stack([np.cos(t), np.sin(t), x, y], axis=1)

    i, j = fi[1:], fj[1:]
    dth = th[j] - th[i] + rng.normal(0, 0.01, len(i))
    dxw, dyw = xy[j, 0] - xy[i, 0], xy[j, 1] - xy[i, 1]
    dxl = np.cos(th[i]) * dxw + np.sin(th[i]) * dyw + rng.normal(0, 0.05, len(i))
    dyl = -np.sin(th[i]) * dxw + np.cos(th[i]) * dyw + rng.normal(0, 0.05, len(i))
    meas = np.concatenate([se2(xy[:1, 0], xy[:1, 1], th[:1]), se2(dxl, dyl, dth)])
    sq = np.tile([2.0, 2.0, 10.0], (len(fi), 1))
    sq[0] = 1.0
    poses = se2(xy[:, 0] + rng.normal(0, 0.05, N), xy[:, 1] + rng.normal(0, 0.05, N), th + rng.normal(0, 0.02, N))
    return fi, fj, meas, sq, poses


def true_residual(row_ptr, cols, sys, lam, dx):
    res = R.apply_system(row_ptr, cols, sys["blocks"], sys["diag"], lam, dx) - sys["b"]
    return float(np.linalg.norm(res)), float(np.linalg.norm(sys["b"]))


def assert_same_solve(dev, ref, what=""):
    assert dev["outcome"] == ref["outcome"], (what, "outcome", dev["outcome"], ref["outcome"])
    assert dev["iterations"] == ref["iterations"], (what, "iterations", dev["iterations"], ref["iterations"])
    assert np.array_equal(dev["dx"], ref["dx"]), (what, "dx", float(np.abs(dev["dx"] - ref["dx"]).max()))
    assert dev["rel_residual_sq"] == ref["rel_residual_sq"], (what, "r.r / b.b", dev["rel_residual_sq"], ref["rel_residual_sq"])
    assert dev["model_decrease"] == ref["model_decrease"], (what, "model decrease", dev["model_decrease"], ref["model_decrease"])


def solve_and_compare(g, lam=LAMBDA, what="", residual=True, expect=R.CONVERGED, **kw):
    """linearize_system -> solve_pcg at the graph's current poses against the restatement; -> (dev, ref, sys, (row_ptr, cols))"""
    sys = g.linearize_system()
    row_ptr, cols = g.pattern()
    dev = g.solve_pcg(lam, REL_TOL, **kw)
    ref = R.pcg(row_ptr, cols, sys["blocks"], sys["b"], sys["diag"], lam, REL_TOL, kw.get("max_iterations"))
    print(f"{what}: N = {g.N}, lambda = {lam:g}: {dev['iterations']} iterations (restatement {ref['iterations']}), outcome {dev['outcome']}, "
          f"r.r / b.b = {dev['rel_residual_sq']:.3e}")
    assert dev["outcome"] == expect, (what, dev["outcome"], dev["iterations"])
    assert_same_solve(dev, ref, what)
    assert np.all(np.isfinite(dev["dx"]))
    if residual:
        res, nb = true_residual(row_ptr, cols, sys, lam, dev["dx"])
        print(f"{what}: true residual {res / nb:.3e} of ||b||")
        assert res <= 10.0 * REL_TOL * nb, (what, res / nb)
        assert dev["rel_residual_sq"] <= REL_TOL * REL_TOL
    return dev, ref, sys, (row_ptr, cols)


def graph_at(F, N, fi, fj, meas, sq, poses):
    g = F.PoseGraph(N, fi, fj, meas, sq)
    g.set_poses(poses)
    return g


# ------------------------------------------------------------------------------------------------------------------
# 1. pose counts on the workgroup edges (256 poses per workgroup of the vector kernels, 32 rows per workgroup of the product)
# ------------------------------------------------------------------------------------------------------------------
def check_pose_counts(F):
    cases = [(N, 40) for N in (255, 256, 257)] + [(1, 0), (2, 0)]
    for N, loops in cases:
        fi, fj, meas, sq, truth, init = make_graph(N, loops, seed=N + loops)
        g = graph_at(F, N, fi, fj, meas, sq, perturbed(init, N))
        try:
            dev, ref, sys, _ = solve_and_compare(g, what=f"N{N}")
            assert dev["iterations"] >= 1 and np.all(np.any(dev["dx"] != 0, axis=1)), N      # the last pose is solved for as well
            # the solved step is the step: try_solved_step is try_step(dx)
            half, _ = g.try_solved_step()
            assert half == g.try_step(dev["dx"])[0], N
        finally:
            g.close()


# ------------------------------------------------------------------------------------------------------------------
# 2. row shapes: no lower neighbours, no transposed ones, a hub, a repeated pair
# ------------------------------------------------------------------------------------------------------------------
HUB_N, HUB = 400, 200


def hub_graph():
    """make_graph(400, 20) plus: pose 200 tied to every pose of 45 .. 355 but its chain neighbours (155 below, 154 above, directions
    alternating) and five factors on the pair (5, 17) in mixed direction"""
    rng = np.random.default_rng(HUB_N)
    fi, fj, meas, sq, truth, init = make_graph(HUB_N, 20, seed=HUB_N)
    fi, fj, meas, sq = list(fi), list(fj), list(meas), list(sq)
    extra = [((HUB, v) if v % 2 else (v, HUB)) for v in range(45, 356) if abs(v - HUB) > 1]
    extra += [((5, 17) if k % 2 else (17, 5)) for k in range(5)]
    for a, b in extra:
        d = O.se2_mul(O.se2_inverse(truth[a]), truth[b])
        fi.append(a); fj.append(b); meas.append(O.se2_mul(d, O.se2(*rng.normal(0, [0.05, 0.05, 0.01])))); sq.append([2.0, 2.0, 10.0])
    return HUB_N, np.array(fi, np.int32), np.array(fj, np.int32), np.array(meas), np.array(sq), init


def check_row_shapes(F):
    N, fi, fj, meas, sq, init = hub_graph()
    g = graph_at(F, N, fi, fj, meas, sq, perturbed(init, 2))
    try:
        row_ptr, cols = g.pattern()
        S = R.Structure(row_ptr, cols)
        lower = np.diff(row_ptr) - 1
        assert lower[0] == 0 and S.transposed[0] >= 1 and S.transposed[N - 1] == 0 and lower[N - 1] >= 1
        assert lower[HUB] >= 150 and S.transposed[HUB] >= 150 and lower[HUB] + S.transposed[HUB] >= 300
        assert len(S.by_step) > 300 // R.GROUP                   # the hub's row is many rounds of its lane group
        r17 = [q for q in range(row_ptr[17], row_ptr[18]) if cols[q] == 5]
        assert len(r17) == 1 and ((fi == 5) & (fj == 17)).sum() + ((fi == 17) & (fj == 5)).sum() == 5
        dev, ref, sys, _ = solve_and_compare(g, what="hub")
        # a product that dropped or doubled one of the hub's terms would not solve the system: the residual above is the check;
        # a changed order of them shows against the restatement.  Both at a second damping:
        solve_and_compare(g, lam=1e-2, what="hub, lambda 1e-2")
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. more than 64 partials: p.q has one per 32 rows (65 at N = 2049), r.r / r.z / b.b / the model one per 256 poses (65 at N = 16385)
# ------------------------------------------------------------------------------------------------------------------
def check_many_partials(F):
    # a strong damping keeps these solves short: the sums are what is looked at, not the conditioning.  With lambda = 10 the
    # preconditioned matrix is I + E with ||E|| <= 1 / 11 (E is the off-diagonal part over 11 times a diagonal it is dominated by), so
    # its condition is below 1.2 and the error shrinks by (sqrt(1.2) - 1) / (sqrt(1.2) + 1) < 0.05 per iteration: 1e-10 in 8 or so.
    for N in (2049, 2049 + 32, 16385, 16385 + 256):
        fi, fj, meas, sq, poses = quick_graph(N, N // 4, seed=N)
        g = graph_at(F, N, fi, fj, meas, sq, poses)
        try:
            assert (N + 31) // 32 > 64 and ((N + 255) // 256 > 64) == (N > 16384)
            dev, ref, sys, _ = solve_and_compare(g, lam=10.0, what=f"N{N}")
            assert 2 <= dev["iterations"] <= 40
        finally:
            g.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. the batch length does not change the result
# ------------------------------------------------------------------------------------------------------------------
def check_batch_independence(F):
    N = 300
    fi, fj, meas, sq, truth, init = make_graph(N, 100, seed=4)
    g = graph_at(F, N, fi, fj, meas, sq, perturbed(init, 4))
    try:
        g.linearize_system()
        runs = [g.solve_pcg(LAMBDA, REL_TOL, batch=batch) for batch in (1, 7, 0)]
        assert runs[0]["outcome"] == R.CONVERGED and runs[0]["iterations"] > 7 and runs[0]["iterations"] % 7 != 0
        for r in runs[1:]:
            assert_same_solve(r, runs[0], "batch")
        # and a cap that falls inside a batch is the cap
        capped = [g.solve_pcg(LAMBDA, REL_TOL, max_iterations=10, batch=batch) for batch in (1, 7, 0)]
        assert capped[0]["outcome"] == R.CAP and capped[0]["iterations"] == 10
        for r in capped[1:]:
            assert_same_solve(r, capped[0], "batch, capped")
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. the iteration cap
# ------------------------------------------------------------------------------------------------------------------
def check_cap(F):
    N = 120
    fi, fj, meas, sq, truth, init = make_graph(N, 0)
    g = graph_at(F, N, fi, fj, meas, sq, perturbed(init, 5))
    try:
        dev, ref, sys, _ = solve_and_compare(g, what="cap", residual=False, expect=R.CAP, max_iterations=50)
        assert dev["iterations"] == 50 and dev["rel_residual_sq"] > REL_TOL * REL_TOL
        # the capped solution stays on the device like a converged one (the host loop does not use it, the C-ABI allows it)
        assert g.try_solved_step()[0] == g.try_step(dev["dx"])[0]
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------
# 6. breakdown; lambda = 0
# ------------------------------------------------------------------------------------------------------------------
def check_breakdown(F):
    poses = np.stack([O.se2(0.1, 0.2, 0.05), O.se2(1.0, 0.1, 0.3), O.se2(2.0, -0.3, 0.1)])
    fi, fj = np.array([0, 0], np.int32), np.array([-1, 1], np.int32)
    meas = np.stack([O.se2(0, 0, 0), O.se2(1.1, 0.0, 0.2)])
    sq = np.array([[1.0, 1.0, 1.0], [2.0, 2.0, 10.0]])
    g = graph_at(F, 3, fi, fj, meas, sq, poses)
    try:
        for lam in (LAMBDA, 0.0):
            sys = g.linearize_system()
            assert not np.any(sys["blocks"][g.pattern()[0][2]]) and np.any(sys["b"][:2])      # pose 2: a zero diagonal block
            dev = g.solve_pcg(lam, REL_TOL)
            assert dev["outcome"] == R.BREAKDOWN and dev["iterations"] == 0, dev
            assert np.all(np.isfinite(dev["dx"])) and np.isfinite(dev["model_decrease"]) and np.isfinite(dev["rel_residual_sq"])
            ref = R.pcg(*g.pattern(), sys["blocks"], sys["b"], sys["diag"], lam, REL_TOL)
            assert_same_solve(dev, ref, "breakdown")
            assert np.array_equal(g.get_poses(), poses), "the pose buffer changed"
            rc = g.L.lama_hip_pgo_try_solved_step(g.h, C.byref(C.c_double(0)), None)
            assert rc == E_STATE, rc                              # a breakdown leaves no solution to try
            again = g.linearize_system()                          # and the graph goes on working
            for k in ("blocks", "b", "diag", "half_chi2"):
                assert np.array_equal(again[k], sys[k]), k
    finally:
        g.close()
    # positive definite through its prior alone: lambda = 0 converges
    N = 30
    fi, fj, meas, sq, truth, init = make_graph(N, 10, seed=6)
    g = graph_at(F, N, fi, fj, meas, sq, perturbed(init, 6))
    try:
        solve_and_compare(g, lam=0.0, what="lambda 0")
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------
# 7. b = 0
# ------------------------------------------------------------------------------------------------------------------
def check_zero_right_hand_side(F):
    node = O.se2(1.5, -0.5, 0.0)                                  # (heading 0: the prior's error is exactly zero)
    g = graph_at(F, 1, np.array([0], np.int32), np.array([-1], np.int32), node[None], np.array([[1.0, 1.0, 1.0]]), node[None])
    try:
        sys = g.linearize_system()
        assert not np.any(sys["b"]) and np.any(sys["blocks"])
        dev = g.solve_pcg(LAMBDA, REL_TOL)
        assert dev["outcome"] == R.CONVERGED and dev["iterations"] == 0 and not np.any(dev["dx"]), dev
        assert dev["model_decrease"] == 0.0 and dev["rel_residual_sq"] == 0.0
        assert_same_solve(dev, R.pcg(*g.pattern(), sys["blocks"], sys["b"], sys["diag"], LAMBDA, REL_TOL), "b = 0")
        assert g.try_solved_step()[0] == sys["half_chi2"] == 0.0
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------
# 8. state rules
# ------------------------------------------------------------------------------------------------------------------
def _raw_solve(g, lam, rel_tol, max_it, outs):
    dx, it, rel, oc, model, ms = outs
    return g.L.lama_hip_pgo_solve_pcg(g.h, lam, rel_tol, max_it, 0, dx.ctypes.data_as(C.c_void_p), C.byref(it), C.byref(rel), C.byref(oc),
                                      C.byref(model), C.byref(ms))


def _sentinels(N):
    return (np.full((N, 3), 7.25), C.c_uint32(77), C.c_double(7.5), C.c_int32(77), C.c_double(7.5), C.c_double(7.5))


def _untouched(outs):
    dx, it, rel, oc, model, ms = outs
    return bool(np.all(dx == 7.25)) and it.value == 77 and rel.value == 7.5 and oc.value == 77 and model.value == 7.5 and ms.value == 7.5


def check_state_rules(F):
    N = 50
    fi, fj, meas, sq, truth, init = make_graph(N, 30, seed=8)
    poses = perturbed(init, 8)
    g = F.PoseGraph(N, fi, fj, meas, sq)
    half = C.c_double(-1.0)

    def refused(rc, word, what):
        assert rc == E_STATE, (what, rc)
        assert word in g.L.lama_hip_pgo_last_error(g.h).decode(), (what, g.L.lama_hip_pgo_last_error(g.h).decode())

    try:
        g.set_poses(poses)
        outs = _sentinels(N)
        refused(_raw_solve(g, LAMBDA, REL_TOL, 100, outs), "linearize_system", "solve before any linearize_system")
        assert _untouched(outs)
        refused(g.L.lama_hip_pgo_try_solved_step(g.h, C.byref(half), None), "solve_pcg", "try_solved_step before a solve")
        g.linearize_system()
        refused(g.L.lama_hip_pgo_try_solved_step(g.h, C.byref(half), None), "solve_pcg", "try_solved_step after linearize_system only")
        assert half.value == -1.0
        for lam, tol, cap, what in ((-1e-5, REL_TOL, 100, "negative lambda"), (float("nan"), REL_TOL, 100, "NaN lambda"),
                                    (float("inf"), REL_TOL, 100, "infinite lambda"), (LAMBDA, 0.0, 100, "rel_tol 0"),
                                    (LAMBDA, 1.0, 100, "rel_tol 1"), (LAMBDA, float("nan"), 100, "rel_tol NaN"), (LAMBDA, -0.5, 100, "rel_tol < 0"),
                                    (LAMBDA, REL_TOL, 0, "max_iterations 0")):
            outs = _sentinels(N)
            assert _raw_solve(g, lam, tol, cap, outs) == E_INVALID, what
            assert _untouched(outs), what
        first = g.solve_pcg(LAMBDA, REL_TOL)                      # the refused calls left the system usable
        assert first["outcome"] == R.CONVERGED
        e1, _ = g.try_solved_step()
        assert e1 == g.try_step(first["dx"])[0]
        # a try leaves system and solution in place (the loop's rejected tries): a second damping, the first again
        second = g.solve_pcg(1e-2, REL_TOL)
        assert not np.array_equal(second["dx"], first["dx"])
        assert_same_solve(g.solve_pcg(LAMBDA, REL_TOL), first, "the same solve after a try and another solve")
        # accept after try_solved_step, as after try_step
        g.try_solved_step()
        g.accept()
        moved = g.get_poses()
        assert not np.array_equal(moved, poses)
        refused(_raw_solve(g, LAMBDA, REL_TOL, 100, _sentinels(N)), "linearize_system", "solve after accept")
        refused(g.L.lama_hip_pgo_try_solved_step(g.h, C.byref(half), None), "solve_pcg", "try_solved_step after accept")
        g.linearize_system()
        g.solve_pcg(LAMBDA, REL_TOL)
        g.set_poses(poses)
        refused(g.L.lama_hip_pgo_try_solved_step(g.h, C.byref(half), None), "solve_pcg", "try_solved_step after set_poses")
        refused(_raw_solve(g, LAMBDA, REL_TOL, 100, _sentinels(N)), "linearize_system", "solve after set_poses")
        g.linearize_system()
        g.solve_pcg(LAMBDA, REL_TOL)
        g.linearize(poses)
        refused(g.L.lama_hip_pgo_try_solved_step(g.h, C.byref(half), None), "solve_pcg", "try_solved_step after linearize")
        refused(_raw_solve(g, LAMBDA, REL_TOL, 100, _sentinels(N)), "linearize_system", "solve after linearize")
        with np.testing.assert_raises(F.LamaError):
            g.try_solved_step()
        # back at the first state the first solve comes out again
        g.linearize_system()
        assert_same_solve(g.solve_pcg(LAMBDA, REL_TOL), first, "after the refusals")
    finally:
        g.close()


def check_two_graphs(F):
    specs = []
    for N, loops, seed in ((50, 30, 1), (257, 300, 2)):
        fi, fj, meas, sq, truth, init = make_graph(N, loops, seed=seed)
        specs.append((N, fi, fj, meas, sq, perturbed(init, seed)))

    def script(g):
        sys = g.linearize_system()
        yield
        a = g.solve_pcg(LAMBDA, REL_TOL, batch=3)
        yield
        e = g.try_solved_step()[0]
        yield
        b = g.solve_pcg(1e-3, REL_TOL, batch=5)
        yield
        g.try_solved_step()
        g.accept()
        yield [sys["b"], a["dx"], np.float64(a["iterations"]), np.float64(a["model_decrease"]), np.float64(e), b["dx"], g.get_poses()]

    alone = []
    for s in specs:
        g = graph_at(F, *s)
        try:
            alone.append(list(script(g))[-1])
        finally:
            g.close()
    graphs = [graph_at(F, *s) for s in specs]
    try:
        runs = [script(g) for g in graphs]
        both = [None, None]
        for _ in range(5):
            for n in (0, 1):
                both[n] = next(runs[n])
    finally:
        for g in graphs:
            g.close()
    for n in (0, 1):
        for a, b in zip(both[n], alone[n]):
            assert np.array_equal(a, b), n


# ------------------------------------------------------------------------------------------------------------------
# 9. the solver only reads the system
# ------------------------------------------------------------------------------------------------------------------
def check_system_is_only_read(F):
    """The C-ABI downloads the system through linearize_system only, which also recomputes it; so besides comparing that download before
    and after, the solve itself is the witness: had a solve written into blocks, b or diag, the same solve run again after it and after
    a solve at another damping would not return the same bits."""
    N = 200
    fi, fj, meas, sq, truth, init = make_graph(N, 80, seed=9)
    g = graph_at(F, N, fi, fj, meas, sq, perturbed(init, 9))
    try:
        before = g.linearize_system()
        row_ptr, cols = g.pattern()
        ref = R.pcg(row_ptr, cols, before["blocks"], before["b"], before["diag"], LAMBDA, REL_TOL)
        first = g.solve_pcg(LAMBDA, REL_TOL)
        assert_same_solve(first, ref, "first solve")
        g.solve_pcg(1.0, REL_TOL)
        g.solve_pcg(LAMBDA, REL_TOL, max_iterations=3)
        assert_same_solve(g.solve_pcg(LAMBDA, REL_TOL), ref, "the same solve after three others")
        after = g.linearize_system()
        for k in ("blocks", "b", "diag"):
            assert np.array_equal(before[k], after[k]), k
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------
# 10. the whole loop: lama::SimplePGO with linear_solver = DevicePCG
# ------------------------------------------------------------------------------------------------------------------
PCG_KEYS = ("pcg_iterations", "pcg_max_iterations_seen", "pcg_fallbacks", "ms_device_solve")


def check_loop(F, nodes, edges, fixed, need_rejection=False, **kw):
    ok, poses, rep = F.simple_pgo(nodes, edges, fixed, solver="pcg", **kw)
    fi, fj, meas, sq = LM.build_graph(nodes, edges, fixed)
    ref = LM.levenberg_marquardt(fi, fj, meas, sq, nodes)
    print(f"N = {len(nodes)}: status {rep['status_name']}, {rep['iterations']} iterations, {rep['tries']} tries, {rep['pcg_iterations']} PCG "
          f"iterations (longest {rep['pcg_max_iterations_seen']}), {rep['pcg_fallbacks']} fallbacks; final error {rep['final_error']:.12g} "
          f"against {ref['final_error']:.12g}")
    assert all(k in rep for k in PCG_KEYS)
    assert ok == (ref["status"] == LM.SUCCESS)
    LM.assert_same_run(rep, ref)
    if need_rejection:                        # a rejected try with accepted iterations after it
        its = LM.iterations_of(rep["trace"])
        assert ok and any(LM.REJECTED in it for it in its[:-2]) and its[-1] == [LM.ACCEPTED], its
    assert abs(rep["initial_error"] - ref["initial_error"]) <= 1e-10 * ref["initial_error"]
    assert abs(rep["final_error"] - ref["final_error"]) <= 1e-7 * max(ref["final_error"], 1e-12)
    if ok:
        assert np.abs(poses - ref["poses"]).max() < 1e-8 * max(1.0, np.abs(ref["poses"]).max())
        assert rep["final_error"] < rep["initial_error"]
    else:
        assert np.array_equal(poses, nodes)
    return ok, rep, ref


def check_loop_on_pcg(F, N, loops, with_fixed, push):
    nodes, edges, fixed = P.loop_inputs(N, loops, with_fixed, push)
    ok, rep, ref = check_loop(F, nodes, edges, fixed, need_rejection=push != 0.0)
    assert ok and rep["pcg_fallbacks"] == 0 and rep["pcg_iterations"] > 0 and rep["nnz_L"] == 0
    assert 0 < rep["pcg_max_iterations_seen"] <= rep["pcg_iterations"] and rep["pcg_max_iterations_seen"] < max(100, 6 * N)


def check_loop_at_the_optimum(F):
    node = O.se2(1.5, -0.5, 0.3)
    ok, rep, ref = check_loop(F, node[None], [], [])
    assert not ok and rep["status"] == LM.ERROR_INCREASE == ref["status"]
    assert rep["iterations"] == 1 and list(rep["trace"]) == ref["trace"] and set(ref["trace"]) == {LM.REJECTED}
    assert rep["pcg_fallbacks"] == 0


def check_forced_fallback(F):
    nodes, edges, fixed = P.loop_inputs(40, 20, False, 0.0)
    ok, rep, ref = check_loop(F, nodes, edges, fixed, pcg_max_iterations=5)
    assert ok and rep["pcg_fallbacks"] > 0 and rep["pcg_max_iterations_seen"] == 5 and rep["nnz_L"] > 0
    ok2, rep2, _ = check_loop(F, nodes, edges, fixed)
    assert ok2 and rep2["pcg_fallbacks"] == 0
    LM.assert_same_run(rep, rep2)


def check_default_path(F):
    """the call without `solver` reports what it always did, and so does solver="ldlt"; an unknown solver is refused"""
    nodes, edges, fixed = P.loop_inputs(40, 20, False, 0.0)
    keys = {"status", "iterations", "tries", "initial_error", "final_error", "nnz_L", "ms_device_linearize", "ms_device_try", "ms_analyze",
            "ms_factorize", "ms_total", "status_name", "trace"}
    ok, poses, rep = F.simple_pgo(nodes, edges, fixed)
    assert ok and set(rep) == keys and rep["nnz_L"] > 0
    ok2, poses2, rep2 = F.simple_pgo(nodes, edges, fixed, solver="ldlt")
    assert ok2 and set(rep2) == keys and np.array_equal(poses, poses2) and list(rep["trace"]) == list(rep2["trace"])
    with np.testing.assert_raises(ValueError):
        F.simple_pgo(nodes, edges, fixed, solver="cholesky")
