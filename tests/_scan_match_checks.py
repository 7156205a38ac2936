"""Checks of k_scan_match (iris_lama_amd/csrc/lama_kernels.h) through lama_hip_pf_scan_match and the grouped step
(lama_hip_pf_match_and_map), case by case and per exit of the solver loop, shared by tests/test_scan_match_sim.py (the lane
simulator, no GPU) and tests/test_scan_match_gpu.py.  Built on tests/_match_checks.py and tests/_match_batch_checks.py; every bound
is one of theirs:

  * pose and iteration count of particle p are BIT-EQUAL to lama_hip_match_solve_with(p, scan, start_p, strategy, max_iterations) on
    the same context: the same workgroup runs the same gn_solve with the compiled-in Cauchy(0.15) weight;
  * against the CPU oracle (O.solve_stats on that particle's own oracle map): EQUAL iteration counts, poses within POSE_TOL;
  * the log-likelihood of particle p against math.fsum of -(r_i * r_i) / meas_sigma over the device's own per-beam residuals at the
    returned pose (lama_hip_match_eval, pinned to the oracle by check_eval) within n * eps * sum|term| (assert_sum).  That catches a
    likelihood taken at the trial state, at the start state, at the state of the previous linearisation or over the wrong beams.  A
    last-bit difference of the state (exp(-h) exp(h) x against x, after a reverted or rejected step) changes the likelihood only
    where it moves a beam's map coordinate across a rounding boundary; the bound sees nothing of it elsewhere, and the cases that
    are to catch a weight taken from the linearisation before such a step use starts where the oracle shows that it does
    (STARTS, assert_flip);
  * the deltas of the counters gn_iterations / gn_evals over one call equal the sums over the particles of the oracle's iterations and
    of its evaluations + 1: PFSlam2D::scanMatch adds calculateLikelihood to the solver's evaluations (src/pf_slam2d.cpp:433-436,
    oracle/lama_oracle.hpp scanMatch).  The counters need cfg.profile != 0 (include/lama_hip.h), which every context here sets.

Every exit case first asserts, from the oracle's own (iterations, evaluations) at the iteration limits 1, 2, ... (oracle_trace), that
the oracle took that exit: a change of the world or of a scan fails the case instead of emptying it.

Contexts with another configuration (cfg.max_iter and cfg.solver_strategy are fixed at creation) hold the map lama_hip_map_add_obstacles
built in the world's context, asserted bit-equal to the oracle's there, put in place by lama_hip_pf_upload_map (no second brushfire:
the lane simulator pays for every flooded cell) and compared by its device-side checksum.
"""
import math

import numpy as np

import _match_batch_checks as MB
from _group_cycle_checks import groups_env
import _match_checks as M
import _oracle as O

HALF_LEN = 8.0             # of the corridor (the scans are taken near x = 1.3 and reach 12 m: they see where the walls end)
EXIT_BEAMS = 65            # scan of the exit cases: one beam more than a wave
Z3, IDQ = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])

# Start poses of the exit cases: offsets (dx, dy, dyaw) from M.SCAN_POSE, start = O.se2(x + dx, y + dy, yaw + dyaw), for the scan
# M.scan_of(EXIT_BEAMS) on M.world_obstacles(HALF_LEN) at l2_max 1.0.  Found on the CPU with the oracle alone (O.solve_stats at the
# limits 1, 2, ..., both strategies), values rounded to four decimals and found again by the assertions of check_exit:
#   the two "..._accepted": numpy default_rng(22), uniform(-1, 1, 3) * [0.4, 0.4, 0.3], draws 0 and 6 of the first 30 (none of which
#                           reverts or rejects a step)
#   everything else:        numpy default_rng(23), uniform(-1, 1, 3) * [0.8, 0.8, 0.6], draws 42, 60, 108 and 138 of the first 150
#                           (14 of the 150 Gauss-Newton solves end with a reverted step, 6 of the Levenberg-Marquardt solves reject one)
# The letters are the oracle's steps, A accepted / R reverted or rejected.
STARTS = {
    "three_accepted": (-0.1069, -0.2406, -0.2469),     # GN AAA, then the small step
    "two_accepted": (-0.1047, 0.3319, -0.0662),        # GN AA, then the small step
    "revert_first": (0.4299, 0.5159, 0.3934),          # GN R;              LM RRAAAA
    "revert_second": (-0.2125, 0.1212, -0.5679),       # GN AR;             LM ARRAAAA
    "revert_third": (0.0974, 0.2069, 0.5459),          # GN AAR
    "lm_never_accepts": (-0.7561, -0.2828, -0.5628),   # LM RRRRRR, then the small step
    # Starts where the last bits matter.  A reverted or rejected step leaves exp(-h) exp(h) x, a few ulps from the linearised state x (5e-11 m after a long step);
    # the map coordinate (4.2e7 cells, ulp 7.5e-9) swallows that for almost every beam, and the two likelihoods are then the same
    # number (as for the starts above).  Here one beam's coordinate rounds the other way and they differ by 1e-9 .. 1e-8, a thousand
    # times the bound of the sum: the same search, comparing the oracle's likelihood at both states (assert_flip), kept at full
    # precision.  default_rng(101), draw 338 of 3000; default_rng(102), draws 2477 and 232281 of 400000 (about one reverted
    # Gauss-Newton solve in 400 does it, and 4 Levenberg-Marquardt solves of the 400000).
    "revert_first_flips": (0.39689908357490183, 0.7726572663957895, 0.5911249208571743),       # GN R
    "revert_third_flips": (-0.34036944465351465, -0.6460953798338457, -0.5175068459852957),    # GN AAR
    "lm_rejected_flips": (-0.5916924264205845, -0.37687737791406895, -0.5505476657959117),     # LM RRRRRR, then the small step
}
# the same search (default_rng(23), draw 6) on the worlds of check_bigsq: GN AR at l2_max 1.5 (HALF_LEN) and at 7.0 (half_len 4)
BIGSQ_REVERT = (0.1996, 0.3883, -0.5781)


def start_of(delta):
    x, y, yaw = M.SCAN_POSE
    return O.se2(x + delta[0], y + delta[1], yaw + delta[2])


# ---------------------------------------------------------------------------------------------------------------------
# contexts
# ---------------------------------------------------------------------------------------------------------------------
def build_world(F, l2_max=1.0, half_len=HALF_LEN):
    """M.build_world with the counters on -> (context of one particle, oracle map)"""
    return M.build_world(F, l2_max, half_len=half_len, profile=1)


def pool_context(F, sources, l2_max, **cfg):
    """A context of len(sources) particles; particle p holds the distance map of (context, particle) = sources[p], or no map at all
    where sources[p] is None (at least one particle must hold one: a map places the window)."""
    ctx = F.HipContext(F.default_cfg(particles=len(sources), l2_max=l2_max, profile=1, **cfg))
    maps = {}
    for p, src in enumerate(sources):
        if src is None:
            continue
        if src not in maps:
            maps[src] = (src[0].download_map(src[1], F.MAP_DISTANCE), src[0].map_checksums(F.MAP_DISTANCE)[src[1]])
        ctx.upload_map(p, F.MAP_DISTANCE, maps[src][0])
    sums = ctx.map_checksums(F.MAP_DISTANCE)
    for p, src in enumerate(sources):
        if src is not None:
            assert sums[p] == maps[src][1], f"uploaded map of particle {p}"
    return ctx


def empty_map(l2_max):
    return O.DM.new(l2_max=l2_max)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's exits
# ---------------------------------------------------------------------------------------------------------------------
def oracle_trace(dm, scan, start, lm, max_iter):
    """-> (iterations, evaluations, [step m accepted?]) of the oracle's solve, the steps read from its own counts at the limits m and
    m + 1: limit m + 1 either makes one more iteration, which evaluates the problem once to validate its step and once more, before,
    if step m was accepted (a rejected or reverted step leaves the linearisation: solver.cpp:69), or it stops at the step test, after
    that one evaluation if step m was accepted."""
    pts, origin, quat = scan

    def solve(limit):
        return O.solve_stats(dm, pts, start, max_iter=limit, lm=lm, origin=origin, quat=quat)[1:]
    it, ev = solve(max_iter)
    acc = []
    for m in range(1, it + 1):
        (i0, e0), (i1, e1) = solve(m), solve(m + 1)
        assert i0 == m, (m, i0)
        acc.append(e1 - e0 - (i1 - m) == 1)
    return it, ev, acc


def expected_evals(it, acc, lm, max_iter):
    """the evaluations of a solve with these steps, as the device counts them: a stop at the step test leaves 2 * iterations + 1, a
    reverted Gauss-Newton step or the limit 2 * iterations, and every pass that follows a rejected Levenberg-Marquardt step saves its
    linearisation"""
    if it == 0:
        return 1
    reverted = not lm and not acc[-1]
    passes = it if (reverted or it == max_iter) else it + 1
    return it + sum(1 for j in range(passes) if j == 0 or acc[j - 1])


# ---------------------------------------------------------------------------------------------------------------------
# the three comparisons and the counters
# ---------------------------------------------------------------------------------------------------------------------
def run_pool(ctx, scan, starts, grouped=False):
    """one scan match of the whole pool from `starts` -> (poses, log-likelihoods, iterations, gn_iterations delta, gn_evals delta)"""
    pts, origin, quat = scan
    starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(ctx.P, 4)
    c0 = ctx.counters()
    if grouped:
        poses, ll, it = ctx.match_and_map(pts, starts, origin, quat)
    else:
        ctx.set_poses(starts)
        poses, ll, it = ctx.scan_match(pts, origin, quat)
        assert np.array_equal(ctx.get_poses(), poses)
    c1 = ctx.counters()
    return poses, ll, it, c1["gn_iterations"] - c0["gn_iterations"], c1["gn_evals"] - c0["gn_evals"]


def assert_loglik(ctx, p, dm, scan, pose, ll, same_libm, what):
    """the weight of particle p: the sum of -(r * r) / meas_sigma over the device's per-beam residuals at `pose`"""
    pts, origin, quat = scan
    r, _ = M.check_eval(ctx, dm, pts, pose, origin, quat, same_libm, what, particle=p)
    M.assert_sum(ll, -(r * r) / M.MEAS_SIGMA, (what, "log-likelihood"))


def compare(ctx, dms, scan, starts, got, strategy, max_iter, same_libm, what):
    """every particle of one call against lama_hip_match_solve_with, the oracle on ITS map and the per-beam terms; the counters"""
    pts, origin, quat = scan
    poses, ll, it, d_it, d_ev = got
    starts = np.asarray(starts).reshape(ctx.P, 4)
    want_it = want_ev = 0
    for p, dm in enumerate(dms):
        w = (what, "particle", p)
        p1, _, i1 = ctx.match_solve_with(p, pts, starts[p], strategy=strategy, max_iterations=max_iter, origin=origin, quat=quat)
        assert np.array_equal(poses[p], p1) and it[p] == i1, (w, "single solver", poses[p], p1, it[p], i1)
        opose, oit, oev = O.solve_stats(dm, pts, starts[p], max_iter=max_iter, lm=(strategy == 1), origin=origin, quat=quat)
        assert it[p] == oit, (w, "iterations", it[p], oit)
        assert np.abs(poses[p] - opose).max() <= M.POSE_TOL, (w, "pose", np.abs(poses[p] - opose).max())
        assert_loglik(ctx, p, dm, scan, poses[p], ll[p], same_libm, w)
        want_it += oit
        want_ev += oev + 1                       # + calculateLikelihood
    assert d_it == want_it, (what, "gn_iterations", d_it, want_it)
    assert d_ev == want_ev, (what, "gn_evals", d_ev, want_ev)


# ---------------------------------------------------------------------------------------------------------------------
# 1. one case per exit
# ---------------------------------------------------------------------------------------------------------------------
# name: (start, strategy, cfg.max_iter, the exit the oracle must have taken[, the last bits of the state move the likelihood])
EXITS = {
    "small_step_after_two_accepted": ("two_accepted", 0, 100, "test"),
    "small_step_after_three_accepted": ("three_accepted", 0, 100, "test"),
    "reverted_first_step": ("revert_first", 0, 100, "revert"),
    "reverted_second_step": ("revert_second", 0, 100, "revert"),
    "reverted_third_step": ("revert_third", 0, 100, "revert"),
    "limit_1_after_an_accepted_step": ("three_accepted", 0, 1, "cap_accepted"),
    "limit_2_after_an_accepted_step": ("three_accepted", 0, 2, "cap_accepted"),
    "lm_accepts_after_rejecting": ("revert_second", 1, 100, "lm_reuse"),
    "lm_accepts_after_rejecting_twice_at_once": ("revert_first", 1, 100, "lm_reuse"),
    "lm_limit_2_in_the_rejected_state": ("revert_second", 1, 2, "cap_rejected"),
    "lm_limit_3_in_the_rejected_state": ("revert_second", 1, 3, "cap_rejected"),
    "lm_limit_1_in_the_rejected_state": ("revert_first", 1, 1, "cap_rejected"),
    "lm_small_step_in_the_rejected_state": ("lm_never_accepts", 1, 100, "test_rejected"),
    # the likelihood of the linearised state is NOT that of the returned state (assert_flip)
    "reverted_first_step_moves_a_beam_across_a_cell_edge": ("revert_first_flips", 0, 100, "revert", True),
    "reverted_third_step_moves_a_beam_across_a_cell_edge": ("revert_third_flips", 0, 100, "revert", True),
    "lm_small_step_in_the_rejected_state_moves_a_beam_across_a_cell_edge": ("lm_rejected_flips", 1, 100, "test_rejected", True),
}


def exit_scan():
    return M.scan_of(EXIT_BEAMS), Z3, IDQ


def assert_exit(name, kind, it, ev, acc, lm, max_iter):
    """the oracle took the exit the case is named after"""
    w = (name, it, ev, "".join("A" if a else "R" for a in acc))
    assert ev == expected_evals(it, acc, lm, max_iter), w
    if kind == "test":                    # stop on a small step that is not applied, after at least two accepted ones
        assert not lm and 2 <= it < max_iter and all(acc) and ev == 2 * it + 1, w
    elif kind == "revert":                # Gauss-Newton reverts its last step and stops
        assert not lm and 1 <= it < max_iter and all(acc[:-1]) and not acc[-1] and ev == 2 * it, w
    elif kind == "cap_accepted":          # the iteration limit right after an accepted step
        assert not lm and it == max_iter and all(acc) and ev == 2 * it, w
    elif kind == "lm_reuse":              # a rejected step followed by an accepted one: the kept linearisation is stepped from again
        assert lm and it < max_iter and any(not a and b for a, b in zip(acc, acc[1:])), w
    elif kind == "cap_rejected":          # the limit while the last step is rejected
        assert lm and it == max_iter and not acc[-1], w
    elif kind == "test_rejected":         # the small step right after a rejected one: stepped from the kept linearisation
        assert lm and 1 <= it < max_iter and not acc[-1], w
    else:
        raise KeyError(kind)


def assert_flip(name, dm, scan, start, lm, it, acc):
    """The oracle's likelihood at the state the last linearisation was taken at -- before the trailing reverted / rejected steps --
    differs from the one at the returned state by more than the bound of the sum: a weight taken from that linearisation fails."""
    pts, origin, quat = scan
    back = 0
    while back < it and not acc[it - 1 - back]:
        back += 1
    assert back >= 1, name
    lin = start if back == it else O.solve_stats(dm, pts, start, max_iter=it - back, lm=lm, origin=origin, quat=quat)[0]
    ret = O.solve_stats(dm, pts, start, lm=lm, origin=origin, quat=quat)[0]
    assert 0.0 < np.abs(lin - ret).max() <= 0.01 * M.POSE_TOL, (name, lin - ret)       # the same state but for the round trip's rounding
    t = [-(r * r) / M.MEAS_SIGMA for r in (O.eval_(dm, pts, q, origin, quat, jac=False) for q in (lin, ret))]
    gap, bound = abs(math.fsum(t[0]) - math.fsum(t[1])), len(pts) * M.EPS * math.fsum(np.abs(t[1]))
    assert gap > 10 * bound, (name, gap, bound)


def check_exit(F, world, name, same_libm):
    """one exit: the oracle's class first, then the three comparisons and the counters, on a context of one particle"""
    wctx, dm = world
    key, strategy, max_iter, kind = EXITS[name][:4]
    scan, start = exit_scan(), start_of(STARTS[key])
    it, ev, acc = oracle_trace(dm, scan, start, strategy == 1, max_iter)
    assert_exit(name, kind, it, ev, acc, strategy == 1, max_iter)
    if len(EXITS[name]) > 4:
        assert_flip(name, dm, scan, start, strategy == 1, it, acc)
    ctx = pool_context(F, [(wctx, 0)], 1.0, max_iter=max_iter, solver_strategy=strategy)
    try:
        got = run_pool(ctx, scan, [start])
        assert got[2][0] == it and got[4] == ev + 1, (name, got[2], it, got[4], ev + 1)
        compare(ctx, [dm], scan, [start], got, strategy, max_iter, same_libm, name)
    finally:
        ctx.close()


def check_gradient_exit(F, world, same_libm):
    """Iteration 0, the gradient test: a pose 40 m from every obstacle on particle 0 and the same scan on particle 1, whose map is
    empty (every corner reads max distance, every gradient is 0).  The pose comes back bit for bit with 0 iterations and one
    evaluation + the likelihood.  The edge scan at heading 0 has every bilinear weight 0 or 1, so its residuals are exactly
    d = sqrt(max_sqdist) * resolution = 1.0 and every partial sum of -(d * d) / meas_sigma = -20 is exact: n * -(d * d) / meas_sigma."""
    wctx, dm = world
    ctx = pool_context(F, [(wctx, 0), None], 1.0)
    dms = [dm, empty_map(1.0)]
    try:
        x, y, yaw = M.SCAN_POSE
        epts, epose = M.edge_scan()
        for what, scan, starts in (("far away / empty", exit_scan(), [O.se2(x, y + 40.0, yaw), start_of(STARTS["two_accepted"])]),
                                   ("edge scan, far away / empty", (epts, Z3, IDQ), [O.se2(0.5, 41.0, 0.0), epose])):
            n = len(scan[0])
            for p in range(2):
                it, ev, acc = oracle_trace(dms[p], scan, starts[p], False, 100)
                assert (it, ev, acc) == (0, 1, []), (what, p, it, ev)
            got = run_pool(ctx, scan, starts)
            assert np.array_equal(got[0], np.stack(starts)) and not got[2].any(), (what, got[0], got[2])
            assert got[3] == 0 and got[4] == 4, (what, got[3], got[4])
            compare(ctx, dms, scan, starts, got, 0, 100, same_libm, what)
            d = math.sqrt(dms[1].max_sqdist()) * 0.05
            if what.startswith("edge"):
                assert d == 1.0 and got[1][0] == got[1][1] == n * (-(d * d) / M.MEAS_SIGMA), (what, got[1])
            else:                       # the interpolation of four equal corners rounds: within the bound of the sum
                M.assert_sum(got[1][1], np.full(n, -(d * d) / M.MEAS_SIGMA), (what, "empty map"))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. beam slicing
# ---------------------------------------------------------------------------------------------------------------------
def slicing_problems():
    """MB.slicing_problems() (the sizes of MB.slicing_sizes(), three mounts, starts at heading 0 and elsewhere), the edge scan from
    five cells beside its pose (every hit of every linearisation's first pass exactly on a cell edge), and a scan started beside the
    blob (the last problem), where corners fall in no patch: check_slicing asserts that from the oracle's map"""
    epts, epose = M.edge_scan()
    out = list(MB.slicing_problems())
    out.append((epts, Z3, IDQ, O.se2(0.5, 1.25, 0.0)))
    out.append((M.scan_of(EXIT_BEAMS), Z3, IDQ, O.se2(*BESIDE_BLOB, 0.0)))
    return out


BESIDE_BLOB = (2.0, 6.5)


def corners_without_patch(dm, pts, x, y):
    """-> (bilinear corners of the scan's hits from (x, y, heading 0, no mount) that lie in no patch of the oracle's map, all corners)"""
    have = {int(i) for i in dm.patch_ids()}
    missing = total = 0
    for px, py, _ in pts:
        c = O.w2m([px + x, py + y, 0.0])
        for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            cell = np.array([c[0] + dx, c[1] + dy, 0], dtype=np.uint32)
            missing += int(O.lib().orc_m2p(0.05, 32, O._p(cell))) not in have
            total += 1
    return missing, total


def check_slicing(world, same_libm):
    """one pool of one particle, the scan changed per call"""
    ctx, dm = world
    missing, total = corners_without_patch(dm, M.scan_of(EXIT_BEAMS), *BESIDE_BLOB)
    assert total // 10 <= missing < total, ("corners without a patch beside the blob", missing, total)
    for k, (pts, origin, quat, start) in enumerate(slicing_problems()):
        scan = (pts, origin, quat)
        got = run_pool(ctx, scan, [start])
        compare(ctx, [dm], scan, [start], got, 0, 100, same_libm, ("slicing", k, len(pts)))


# ---------------------------------------------------------------------------------------------------------------------
# 3. every particle its own map and start
# ---------------------------------------------------------------------------------------------------------------------
POOL, POOL_EMPTY, POOL_GROUPS = 19, 7, 2      # 19 particles in two groups: pose-table blocks of 10 and 9 entries


def pool_starts(seed=12, count=POOL):
    """distinct starts, seeded like MB.small_problems: numpy default_rng(seed), N(0, [0.04, 0.04, 0.015]) around the scan's pose"""
    rng = np.random.default_rng(seed)
    x, y, yaw = M.SCAN_POSE
    return np.stack([O.se2_mul(O.se2(x, y, yaw), O.se2(*rng.normal(0, [0.04, 0.04, 0.015]))) for _ in range(count)])


def check_pool(F, same_libm):
    """19 particles alternating between the two worlds of MB.two_map_context, particle 7 with an empty map, distinct starts: through
    lama_hip_pf_scan_match, reversed, and through the grouped step"""
    src, dm2 = MB.two_map_context(F)
    ctxs = []
    try:
        which = [None if p == POOL_EMPTY else p % 2 for p in range(POOL)]
        dms = [empty_map(1.0) if w is None else dm2[w] for w in which]
        sources = [None if w is None else (src, w) for w in which]
        with groups_env(POOL_GROUPS):
            ctx = pool_context(F, sources, 1.0)
        ctxs.append(ctx)
        assert ctx.configured_step_groups() == POOL_GROUPS
        pts, origin, quat = M.mounted_scan(EXIT_BEAMS, M.MOUNTS["offset"])
        scan = (pts, origin, quat)
        starts = pool_starts()
        before = [ctx.map_checksums(k).copy() for k in (F.MAP_DISTANCE, F.MAP_OCCUPANCY)]
        got = run_pool(ctx, scan, starts)
        compare(ctx, dms, scan, starts, got, 0, 100, same_libm, "pool")
        for a, k in zip(before, (F.MAP_DISTANCE, F.MAP_OCCUPANCY)):
            assert np.array_equal(a, ctx.map_checksums(k)), "a map changed"
        # the maps decide: the same start on a particle that holds the other world ends elsewhere
        for p, w in enumerate(which):
            if w is None:
                continue
            q = which.index(1 - w)
            other, _, _ = ctx.match_solve_with(q, pts, starts[p], strategy=0, max_iterations=100, origin=origin, quat=quat)
            assert not np.array_equal(other, got[0][p]), ("the other world's map gives the same pose", p, q)
        assert len({got[0][p].tobytes() for p in range(POOL)}) == POOL
        # reversed: maps and starts move along, and so do the results, bit for bit -- nothing depends on the slot
        rev = pool_context(F, sources[::-1], 1.0)
        ctxs.append(rev)
        got_r = run_pool(rev, scan, starts[::-1])
        for a, b in zip(got[:3], got_r[:3]):
            assert np.array_equal(a, b[::-1]), "reversed pool"
        assert got[3:] == got_r[3:]
        # the grouped step (last: it goes on to integrate the scan into the maps): bit-equal to the single-stream call
        got_g = run_pool(ctx, scan, starts, grouped=True)
        assert ctx.step_groups() == POOL_GROUPS
        for a, b in zip(got[:3], got_g[:3]):
            assert np.array_equal(a, b), "grouped step"
        assert got[3:] == got_g[3:], ("counters of the grouped step", got[3:], got_g[3:])
        assert np.array_equal(ctx.get_poses(), got[0])
        ctx.sync()                             # (the queued map updates end without an error)
    finally:
        for c in ctxs:
            c.close()
        src.close()


BIG_POOL, BIG_L2_MAX = 34, 0.25       # two groups of 17 > ARG_BLOCK particles; a reach of 5 cells keeps the map update cheap


def check_groups_beyond_the_pose_table(F, same_libm):
    """Groups of more than ARG_BLOCK particles do not get their start poses as a launch argument: the group's launch reads prm.poses
    (the NoTable instantiation) with first_particle != 0 for the second group.  34 particles alternating between the two worlds:
    the grouped step bit-equal to the single-stream call, which is compared as everywhere."""
    src, dm2 = MB.two_map_context(F, l2_max=BIG_L2_MAX)
    ctx = None
    try:
        with groups_env(2):
            ctx = pool_context(F, [(src, p % 2) for p in range(BIG_POOL)], BIG_L2_MAX)
        assert ctx.configured_step_groups() == 2
        pts, origin, quat = M.mounted_scan(EXIT_BEAMS, M.MOUNTS["yawed"])
        scan, starts = (pts, origin, quat), pool_starts(seed=13, count=BIG_POOL)
        got = run_pool(ctx, scan, starts)
        compare(ctx, [dm2[p % 2] for p in range(BIG_POOL)], scan, starts, got, 0, 100, same_libm, "groups of 17")
        got_g = run_pool(ctx, scan, starts, grouped=True)
        assert ctx.step_groups() == 2
        for a, b in zip(got[:3], got_g[:3]):
            assert np.array_equal(a, b), "grouped step"
        assert got[3:] == got_g[3:], ("counters of the grouped step", got[3:], got_g[3:])
        ctx.sync()
    finally:
        if ctx is not None:
            ctx.close()
        src.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the BIGSQ instantiations (max_sqdist > SM_LUT: no square-root table) on both libraries
# ---------------------------------------------------------------------------------------------------------------------
def check_bigsq(F, l2_max, half_len, wide, same_libm):
    ctx, dm = build_world(F, l2_max, half_len)
    try:
        assert dm.max_sqdist() > MB.kernel_constants()["SM_LUT"]      # the launch takes <BIGSQ = true>
        assert F.needs_wide(l2_max, 0.05) == wide and ctx.L is F.hip_lib(wide=wide)
        pts, origin, quat, start = MB.small_problems(sizes=(64, 257), seed=9)[1]
        scan = (pts, origin, quat)
        compare(ctx, [dm], scan, [start], run_pool(ctx, scan, [start]), 0, 100, same_libm, ("bigsq", l2_max, "slicing"))
        scan, start = exit_scan(), start_of(BIGSQ_REVERT)
        it, ev, acc = oracle_trace(dm, scan, start, False, 100)
        assert_exit(("bigsq", l2_max), "revert", it, ev, acc, False, 100)
        got = run_pool(ctx, scan, [start])
        assert got[2][0] == it and got[4] == ev + 1
        compare(ctx, [dm], scan, [start], got, 0, 100, same_libm, ("bigsq", l2_max, "reverted step"))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. what include/lama_hip.h promises for the entry's arguments: any output may be NULL (it states no refusal for this entry)
# ---------------------------------------------------------------------------------------------------------------------
def check_null_outputs(F, world):
    ctx, dm = world
    scan, start = exit_scan(), start_of(STARTS["two_accepted"])
    want = run_pool(ctx, scan, [start])
    pts = np.ascontiguousarray(scan[0])
    ctx.set_poses(np.stack([start]))
    ctx._chk(ctx.L.lama_hip_pf_scan_match(ctx.h, F._p(pts), len(pts), None, None, None, None, None))
    assert np.array_equal(ctx.get_poses(), want[0])
    ll = np.zeros(1)
    ctx.set_poses(np.stack([start]))
    ctx._chk(ctx.L.lama_hip_pf_scan_match(ctx.h, F._p(pts), len(pts), None, None, None, F._p(ll), None))
    assert np.array_equal(ll, want[1]) and np.array_equal(ctx.get_poses(), want[0])
