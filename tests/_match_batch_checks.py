"""Checks of k_match_solve_batch / lama_hip_match_solve_batch / lama::SolveBatch, shared by tests/test_match_batch_sim.py (the lane
simulator, no GPU) and tests/test_match_batch_gpu.py.  Built on tests/_match_checks.py; every bound is one of its bounds:

  * a CauchyWeight(0.15) problem of a batch is BIT-EQUAL to lama_hip_match_solve_with on the same inputs -- pose, the six J^T J
    sums, the sum of r^2, the iteration count: the same workgroup runs the same code on the same beams (csrc/lama_match_batch.h);
  * against the CPU oracle (O.solve_full, Cauchy(0.15)) and against lama::Solver's generic host loop (the other weights): poses
    within POSE_TOL with EQUAL iteration counts, as check_solve asks;
  * a summed output against math.fsum of its per-beam terms within n * eps * sum|term| (assert_sum): the terms are the device's own
    per-beam residuals / Jacobian rows / cell distances at the returned pose (lama_hip_match_eval, lama_hip_match_cell_distances,
    pinned to the oracle by check_eval), weighted by the numpy restatement of RobustCost::value below, which
    tests/golden/robust_weights_golden.npz pins to the reference's own robust_cost.cpp;
  * MatchSurface2D::error() = sqrt(out8[7] / n) against O.match_error within 1e-12 (tests/_cmp.py:88).
"""
import os
import re

import numpy as np

import _match_checks as M
import _oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS_H = os.path.join(HERE, "..", "iris_lama_amd", "csrc", "lama_kernels.h")
GOLDEN = os.path.join(HERE, "golden", "robust_weights_golden.npz")
ERROR_TOL = 1e-12            # tests/_cmp.py:88
KINDS = [("unit", 0.0), ("tukey", 4.6851), ("tdist", 3.0), ("cauchy", 0.3), ("huber", 0.15)]


def kernel_constants():
    with open(KERNELS_H) as f:
        src = f.read()
    return {k: int(re.search(r"constexpr int " + k + r" = (\d+);", src).group(1)) for k in ("SM_BLOCK", "SM_NB", "SM_LUT")}


def slicing_sizes():
    """shorter than a wave, a wave and its neighbours, a block, one gather batch of the block, and one beam more"""
    c = kernel_constants()
    blk, batch = c["SM_BLOCK"], c["SM_NB"] * c["SM_BLOCK"]
    return [1, 63, 64, 65, blk, batch, batch + 1]


def robust_value(kind, param, x):
    """RobustCost::value (src/nlls/robust_cost.cpp:36-82) of the five classes, operation by operation"""
    x = np.asarray(x, dtype=np.float64)
    if kind == "unit":
        return np.ones_like(x)
    if kind == "tukey":
        bb = np.float64(param) * np.float64(param)
        xx = x * x
        w = 1.0 - xx / bb
        return np.where(xx <= bb, w * w, 0.0)
    if kind == "tdist":
        return (np.float64(param) + 1.0) / (np.float64(param) + (x * x))
    if kind == "cauchy":
        c = 1.0 / (np.float64(param) * np.float64(param))
        return 1.0 / (1.0 + x * x * c)
    if kind == "huber":
        with np.errstate(divide="ignore"):
            return np.where(x < param, 1.0, np.float64(param) / np.abs(x))
    raise KeyError(kind)


def slicing_problems():
    """seven problems: the sizes of slicing_sizes(), mounts mixed, start poses at heading 0 and at arbitrary headings"""
    x, y, yaw = M.SCAN_POSE
    mounts = [None, "offset", "yawed", None, "upside_down", "offset", None]
    starts = [O.se2(1.3, 1.65, 0.0), O.se2(x, y + 0.06, yaw - 0.02), O.se2(x + 0.03, y - 0.04, yaw + 0.015), O.se2(1.3, 1.68, 0.0),
              O.se2(x - 0.02, y + 0.05, yaw + 0.01), O.se2(x + 0.01, y + 0.03, yaw - 0.012), O.se2(x, y - 0.05, yaw + 0.02)]
    out = []
    for n, mount, start in zip(slicing_sizes(), mounts, starts):
        if mount is None:
            pts, origin, quat = M.scan_of(n), np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])
        else:
            pts, origin, quat = M.mounted_scan(n, M.MOUNTS[mount])
        assert len(pts) == n
        out.append((pts, origin, quat, start))
    return out


def run_batch(ctx, problems, order=None, particles=0, **kw):
    """problems: [(pts, origin, quat, start)] -> match_solve_batch's outputs, in the problems' order whatever `order` is"""
    order = list(range(len(problems))) if order is None else list(order)
    sel = [problems[i] for i in order]
    pa = np.broadcast_to(np.asarray(particles, dtype=np.uint32), (len(problems),))[order]
    mi = kw.pop("max_iterations", 100)
    mi = np.broadcast_to(np.asarray(mi, dtype=np.uint32), (len(problems),))[order]
    poses, out8, it, st = ctx.match_solve_batch(pa, [p[0] for p in sel], np.stack([p[3] for p in sel]), max_iterations=mi,
                                                origins=np.stack([p[1] for p in sel]), quats=np.stack([p[2] for p in sel]), **kw)
    inv = np.argsort(order)
    return poses[inv], out8[inv], it[inv], st[inv]


def assert_equals_single(ctx, problems, got, strategy, particles=0, max_iterations=100, what=""):
    """every problem of a Cauchy(0.15) batch against lama_hip_match_solve_with: bit for bit"""
    poses, out8, it, st = got
    pa = np.broadcast_to(np.asarray(particles), (len(problems),))
    mi = np.broadcast_to(np.asarray(max_iterations), (len(problems),))
    for b, (pts, origin, quat, start) in enumerate(problems):
        if mi[b] == 0:          # (lama_hip_match_solve_with reads 0 as "the context's limit": evaluate only is lama_hip_match_solve's do_solve = 0)
            p1, jtj, sr2, i1 = ctx.match_solve(int(pa[b]), pts, start, origin, quat, solve=False)
            o1 = np.concatenate([jtj, [sr2]])
        else:
            p1, o1, i1 = ctx.match_solve_with(int(pa[b]), pts, start, strategy=strategy, max_iterations=int(mi[b]), origin=origin, quat=quat)
        assert np.array_equal(poses[b], p1), (what, b, "pose", poses[b], p1)
        assert np.array_equal(out8[b, :7], o1), (what, b, "out7", out8[b, :7], o1)
        assert it[b] == i1 and st[b] == 0, (what, b, it[b], i1, st[b])


def assert_out8(ctx, dm, particle, pts, origin, quat, pose, out8, kind, param, same_libm, what):
    """the eight sums of one problem against fsum of the per-beam terms at the returned pose; error() against the oracle"""
    if dm is not None:
        r, J = M.check_eval(ctx, dm, pts, pose, origin, quat, same_libm, what)
        d = ctx.cell_distances(particle, pts, pose, origin, quat)
    else:
        r, J = ctx.match_eval(particle, pts, pose, origin, quat)
        d = ctx.cell_distances(particle, pts, pose, origin, quat)
    w = np.sqrt(robust_value(kind, param, r))
    j0, j1, j2 = J[:, 0] * w, J[:, 1] * w, J[:, 2] * w
    for k, t in enumerate((j0 * j0, j1 * j0, j1 * j1, j2 * j0, j2 * j1, j2 * j2)):
        M.assert_sum(out8[k], t, (what, "JtJ", k))
    M.assert_sum(out8[6], r * r, (what, "sum r^2"))
    M.assert_sum(out8[7], d * d, (what, "sum cell d^2"))
    if dm is not None:
        err = float(np.sqrt(out8[7] / len(pts)))
        want = O.match_error(dm, pts, pose, origin, quat)
        assert abs(err - want) <= ERROR_TOL, (what, "error()", err, want)


def check_slicing_and_ownership(ctx, dm, same_libm):
    """one call with B = 7 (slicing_problems), both strategies, and the batch reversed"""
    problems = slicing_problems()
    for strategy in (0, 1):
        got = run_batch(ctx, problems, strategy=strategy)
        assert_equals_single(ctx, problems, got, strategy, what=("strategy", strategy))
        rev = run_batch(ctx, problems, order=range(len(problems) - 1, -1, -1), strategy=strategy)
        for a, b in zip(got, rev):
            assert np.array_equal(a, b), ("reversed batch", strategy)
        for b, (pts, origin, quat, start) in enumerate(problems):
            opose, oit, _ = O.solve_full(dm, pts, start, lm=(strategy == 1), origin=origin, quat=quat)
            assert got[2][b] == oit, (strategy, b, got[2][b], oit)
            assert np.abs(got[0][b] - opose).max() <= M.POSE_TOL, (strategy, b, np.abs(got[0][b] - opose).max())
            if strategy == 0:
                assert_out8(ctx, dm, 0, pts, origin, quat, got[0][b], got[1][b], "cauchy", 0.15, same_libm, ("slicing", b))


def two_map_context(F, l2_max=1.0):
    """a 2-particle context whose particles hold different maps: the corridor with its blob, and the corridor shifted by 3 cells
    without it (16 m of each: the scans are taken near x = 1.3).  -> (ctx, [dm0, dm1])"""
    import math
    from _cmp import DM_FIELDS, assert_maps_equal
    from _worlds import open_corridor
    worlds = [M.world_obstacles(half_len=8.0), open_corridor(half_len=8.0) + np.array([0.15, 0.15])]
    ctx = F.HipContext(F.default_cfg(particles=2, l2_max=l2_max))
    dms = []
    for p, w in enumerate(worlds):
        cells = np.array([[int(c[0]), int(c[1])] for c in (O.w2m([x, y, 0.0]) for x, y in w)], dtype=np.uint32)
        dm = O.DM.new(l2_max=l2_max)
        for x, y in cells:
            dm.add(int(x), int(y))
        dm.update()
        assert dm.max_sqdist() == math.ceil(l2_max * (1.0 / 0.05)) ** 2
        ctx.add_obstacles(p, cells)
        dms.append(dm)
    for p in range(2):
        assert_maps_equal(ctx.download_map(p, F.MAP_DISTANCE), dms[p].dump(), DM_FIELDS, f"map of particle {p}")
    return ctx, dms


def small_problems(sizes=(65, 64, 257, 63), seed=5):
    """a few small problems with perturbed starts (seed stated: numpy default_rng(seed), N(0, [0.04, 0.04, 0.015]))"""
    rng = np.random.default_rng(seed)
    x, y, yaw = M.SCAN_POSE
    out = []
    for k, n in enumerate(sizes):
        if k % 2:
            pts, origin, quat = M.mounted_scan(n, M.MOUNTS["offset"])
        else:
            pts, origin, quat = M.scan_of(n), np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])
        start = O.se2_mul(O.se2(x, y, yaw), O.se2(*rng.normal(0, [0.04, 0.04, 0.015])))
        out.append((pts, origin, quat, start))
    return out


def check_maps_per_problem(F, same_libm):
    ctx, dms = two_map_context(F)
    try:
        problems = small_problems()
        pa = np.arange(len(problems)) % 2
        before = [ctx.map_checksums(k).copy() for k in (F.MAP_DISTANCE, F.MAP_OCCUPANCY)]
        got = run_batch(ctx, problems, particles=pa, strategy=0)
        assert_equals_single(ctx, problems, got, 0, particles=pa, what="two maps")
        for b, (pts, origin, quat, start) in enumerate(problems):
            opose, oit, _ = O.solve_full(dms[pa[b]], pts, start, origin=origin, quat=quat)
            assert got[2][b] == oit and np.abs(got[0][b] - opose).max() <= M.POSE_TOL, b
        # the two maps do differ: the same problem on the other particle's map ends elsewhere
        swapped = run_batch(ctx, problems, particles=1 - pa, strategy=0)
        assert not np.array_equal(swapped[0], got[0])
        after = [ctx.map_checksums(k) for k in (F.MAP_DISTANCE, F.MAP_OCCUPANCY)]
        for a, b in zip(before, after):
            assert np.array_equal(a, b), "a map changed"
    finally:
        ctx.close()


def check_iteration_limits(ctx, dm, same_libm):
    problems = small_problems(sizes=(65, 64, 257, 63), seed=6)
    limits = np.array([0, 1, 2, 100], dtype=np.uint32)
    for strategy in (0, 1):
        got = run_batch(ctx, problems, strategy=strategy, max_iterations=limits)
        assert_equals_single(ctx, problems, got, strategy, max_iterations=limits, what=("limits", strategy))
        assert np.array_equal(got[0][0], problems[0][3]) and got[2][0] == 0        # 0: the start pose, bit for bit
        assert got[2][1] <= 1 and got[2][2] <= 2
        pts, origin, quat, start = problems[0]
        assert_out8(ctx, dm, 0, pts, origin, quat, start, got[1][0], "cauchy", 0.15, same_libm, "evaluate only")
        # 1 iteration, then 100 from its output: what two single calls give
        first = run_batch(ctx, problems, strategy=strategy, max_iterations=1)
        cont = [(p[0], p[1], p[2], first[0][b]) for b, p in enumerate(problems)]
        second = run_batch(ctx, cont, strategy=strategy, max_iterations=100)
        for b, (pts, origin, quat, start) in enumerate(problems):
            p1, _, i1 = ctx.match_solve_with(0, pts, start, strategy=strategy, max_iterations=1, origin=origin, quat=quat)
            p2, o2, i2 = ctx.match_solve_with(0, pts, p1, strategy=strategy, max_iterations=100, origin=origin, quat=quat)
            assert np.array_equal(first[0][b], p1) and first[2][b] == i1
            assert np.array_equal(second[0][b], p2) and np.array_equal(second[1][b, :7], o2) and second[2][b] == i2


def check_refusals(F, ctx):
    """every LAMA_HIP_E_INVALID case: poses and outputs untouched; B == 0 succeeds"""
    import ctypes as C
    problems = small_problems(sizes=(9, 12), seed=7)
    pts = np.ascontiguousarray(np.concatenate([p[0] for p in problems]))
    offs = np.array([0, 9, 21], dtype=np.uint32)
    base = dict(pa=np.zeros(2, dtype=np.uint32), pts=pts, offs=offs, poses=np.stack([p[3] for p in problems]), mi=np.full(2, 100, dtype=np.uint32),
                strategy=0, kind=F.ROBUST_KINDS["huber"], param=0.15)

    def call(**kw):
        a = dict(base, **kw)
        poses = a["poses"].copy()
        out8, it, st = np.full((2, 8), -7.0), np.full(2, -7, dtype=np.int32), np.full(2, 7, dtype=np.uint32)
        rc = ctx.L.lama_hip_match_solve_batch(ctx.h, a.get("B", 2), F._p(a["pa"]), F._p(a["pts"]), F._p(a["offs"]), None, None, F._p(poses), F._p(a["mi"]),
                                              a["strategy"], a["kind"], C.c_double(a["param"]), F._p(out8), F._p(it), F._p(st))
        untouched = np.array_equal(poses, a["poses"], equal_nan=True) and np.all(out8 == -7.0) and np.all(it == -7) and np.all(st == 7)
        return rc, untouched

    assert call() == (0, False)                                      # the valid call does run
    assert call(B=0) == (0, True)
    bad_pts = pts.copy(); bad_pts[13, 1] = np.inf
    nan_pose = base["poses"].copy(); nan_pose[1, 2] = np.nan
    cases = {
        "empty slice": dict(offs=np.array([0, 9, 9], dtype=np.uint32)),
        "decreasing offsets": dict(offs=np.array([0, 9, 4], dtype=np.uint32)),
        "particle out of range": dict(pa=np.array([0, 1], dtype=np.uint32)),
        "non-finite point": dict(pts=bad_pts),
        "non-finite pose": dict(poses=nan_pose),
        "non-finite parameter": dict(param=float("nan")),
        "infinite parameter": dict(param=float("inf")),
        "unknown kind": dict(kind=5),
        "negative kind": dict(kind=-1),
        "unknown strategy": dict(strategy=2),
        "Tukey(0)": dict(kind=F.ROBUST_KINDS["tukey"], param=0.0),
        "Cauchy(0)": dict(kind=F.ROBUST_KINDS["cauchy"], param=0.0),
        "TDistribution(0)": dict(kind=F.ROBUST_KINDS["tdist"], param=0.0),
        "Huber(0)": dict(kind=F.ROBUST_KINDS["huber"], param=0.0),
        # the constant handed over as the class stores it (LAMA_HIP_ROBUST_STORED): bb_ of Tukey(0), c_ of Cauchy(0), an unknown kind
        "stored Tukey(0)": dict(kind=F.ROBUST_KINDS["tukey"] | F.ROBUST_STORED, param=0.0),
        "stored Cauchy(0)": dict(kind=F.ROBUST_KINDS["cauchy"] | F.ROBUST_STORED, param=float("inf")),
        "stored unknown kind": dict(kind=5 | F.ROBUST_STORED),
    }
    for name, kw in cases.items():
        assert call(**kw) == (-1, True), name


def check_zero_norm_status(F, ctx):
    """A start pose whose unit complex is (0, 0) -- finite, so it is not refused -- reads as heading atan2(0, 0) = 0; the first
    applied step multiplies it by exp(h) and normalises a complex of norm 0 (the reference throws SophusException there).  That
    problem gets its status word, its neighbours are solved as if alone, the call returns LAMA_HIP_E_NUMERIC."""
    problems = small_problems(sizes=(65, 64, 66), seed=8)
    bad = list(problems[1])
    bad[3] = np.array([0.0, 0.0, M.SCAN_POSE[0] + 0.03, M.SCAN_POSE[1] + 0.04])
    mixed = [problems[0], tuple(bad), problems[2]]
    poses, out8, it, st = run_batch(ctx, mixed, strategy=0, check=False)
    assert list(st) == [0, 1, 0]
    for b in (0, 2):
        pts, origin, quat, start = problems[b]
        p1, o1, i1 = ctx.match_solve_with(0, pts, start, strategy=0, max_iterations=100, origin=origin, quat=quat)
        assert np.array_equal(poses[b], p1) and np.array_equal(out8[b, :7], o1) and it[b] == i1
    try:
        run_batch(ctx, mixed, strategy=0)
    except F.LamaError as e:
        assert "status -6" in str(e) and "problem 1" in str(e), str(e)
    else:
        raise AssertionError("no LAMA_HIP_E_NUMERIC")
    # the context's own error word was not set: the next call on it succeeds
    got = run_batch(ctx, problems, strategy=0)
    assert list(got[3]) == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# the other robust costs, against lama::Solver's generic host loop, and the host class
# ---------------------------------------------------------------------------------------------------------------------
# seeds of the start poses (robust_starts).  Seed 0 was the first one tried for every kind, and with it the host loop and the device
# agree on the iteration count for all five kinds and both strategies in the simulator (test_match_batch_sim.py asserts exactly
# that), so no kind needed a second seed.
ROBUST_SEEDS = {"unit": 0, "tukey": 0, "tdist": 0, "cauchy": 0, "huber": 0}


def slam_with_map(F, beams=180, steps=3):
    """a lama::Slam2D that has mapped a few corridor scans -> (slam, a scan to register, the pose it was taken at)"""
    pts, odom, truth = F.corridor_log(steps, beams)
    h = F.Slam2D()
    h.set_pose(*odom[0])
    for k in range(steps + 1):
        h.update(pts[k], odom[k], float(k))
    return h, pts[steps], h.pose()


def robust_starts(kind, base, count=3):
    """start poses for one weight: numpy default_rng(ROBUST_SEEDS[kind]), N(0, [0.04, 0.04, 0.015]) around the mapped pose"""
    rng = np.random.default_rng(ROBUST_SEEDS[kind])
    return [O.se2_mul(base, O.se2(*rng.normal(0, [0.04, 0.04, 0.015]))) for _ in range(count)]


def check_robust_costs(F, h, scan, base):
    """the five weights: one batch of three starts each on the Slam2D's device context against the generic host loop run on the
    same map (poses within POSE_TOL, EQUAL iteration counts), and the eight sums against the weighted per-beam terms"""
    ctx = h.hip_context()
    z3, idq = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])
    for kind, param in KINDS:
        starts = robust_starts(kind, base)
        problems = [(scan, z3, idq, s) for s in starts]
        for strategy, sname in ((0, "gn"), (1, "lm")):
            poses, out8, it, st = run_batch(ctx, problems, strategy=strategy, robust=kind, robust_param=param)
            assert not st.any()
            for b, s in enumerate(starts):
                want, _, wit = h.match_solve_generic(scan, s, strategy=sname, weight=kind, weight_param=param)
                print(f"robust {kind} {sname} start {b}: device {it[b]} iterations, host loop {wit}, pose difference {np.abs(poses[b] - want).max():.3g}")
                assert it[b] == wit, (kind, sname, b, it[b], wit)
                assert np.abs(poses[b] - want).max() <= M.POSE_TOL, (kind, sname, b, np.abs(poses[b] - want).max())
                assert_out8(ctx, None, 0, scan, z3, idq, poses[b], out8[b], kind, param, False, (kind, sname, b))


def check_host_class(F, h, scan, base, other=None):
    """lama::SolveBatch over three MatchSurface2D of one Slam2D: states, covariances, iterations and errors equal to the C-ABI's"""
    from iris_lama_amd.ffi import LamaError
    ctx = h.hip_context()
    z3, idq = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])
    starts = robust_starts("huber", base)
    scans = [scan, scan[::2], scan[1::3]]
    problems = [(s, z3, idq, p) for s, p in zip(scans, starts)]
    for strategy, sname in ((0, "gn"), (1, "lm")):
        poses, cov, it, err = h.solve_batch(scans, starts, strategy=sname, weight="huber", weight_param=0.15)
        dposes, out8, dit, _ = run_batch(ctx, problems, strategy=strategy, robust="huber", robust_param=0.15)
        assert np.array_equal(poses, dposes) and np.array_equal(it, dit)
        for b in range(3):
            assert err[b] == np.sqrt(out8[b, 7] / len(scans[b]))
            a = out8[b]
            A = np.array([[a[0], a[1], a[3]], [a[1], a[2], a[4]], [a[3], a[4], a[5]]])
            assert np.allclose(cov[b], np.linalg.inv(A), rtol=1e-9, atol=0.0), (sname, b)
    # a per-problem limit; Cauchy(0.15) through the class equals lama::Solve on each problem
    poses, cov, it, err = h.solve_batch(scans, starts, weight="cauchy", weight_param=0.15, max_iterations=[0, 1, 100])
    assert np.array_equal(poses[0], starts[0]) and it[0] == 0 and it[1] <= 1
    p2, c2, i2 = h.match_solve(scans[2], starts[2], strategy="gn")
    assert np.array_equal(poses[2], p2) and it[2] == i2 and np.array_equal(cov[2], c2)
    for kind, param in KINDS:                                        # every class of robust_cost.h is accepted
        h.solve_batch(scans[:1], starts[:1], weight=kind, weight_param=param or 1.0)
    # a parameter the reference's formula divides by zero with is named as such, not as an unknown class
    try:
        h.solve_batch(scans[:1], starts[:1], weight="cauchy", weight_param=0.0)
    except LamaError as e:
        assert "CauchyWeight(param) needs param != 0" in str(e), str(e)
    else:
        raise AssertionError("CauchyWeight(0) was accepted")
    # non-default thresholds have no device kernel
    try:
        h.solve_batch(scans, starts, eps1=1e-6)
    except LamaError as e:
        assert "default thresholds" in str(e), str(e)
    else:
        raise AssertionError("non-default thresholds were accepted")
    # problems of two device contexts
    if other is not None:
        try:
            h.solve_batch(scans, starts, other=other)
        except LamaError as e:
            assert "different device contexts" in str(e), str(e)
        else:
            raise AssertionError("two contexts were accepted")
    # lama::Solve itself still refuses what it refused: the new entry points are the only way in
    for weight, wp in (("huber", 0.15), ("tukey", 4.6851), ("cauchy", 0.3)):
        try:
            h.match_solve(scan, base, weight=weight, weight_param=wp)
        except LamaError as e:
            assert "no device kernel" in str(e), str(e)
        else:
            raise AssertionError(f"lama::Solve accepted {weight}")
