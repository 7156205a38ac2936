"""Checks of what a particle group of the grouped step schedule (lama_hip_pf_match_and_map) puts on its stream between two
brushfires, shared by tests/test_group_cycle_gpu.py and the lane-simulator tests (tests/test_group_cycle_sim.py):

  * a block of at most 16 particles takes its predicted poses and its scan transforms along as launch arguments, a larger block
    copies them into d_poses / d_tfs as before (both paths side by side in one context: 34 particles in two groups are blocks of
    24 and 10, 17 particles blocks of 16 and 1);
  * on the step path k_pack_group clears the hand-over counts and statistics it has packed (no fills in front of the ray-cast); a
    call that drains the groups packs without clearing;
  * k_occ_reverse_dir scans only the directory rows of the mapped box.

They build on tests/_step_group_checks.py (device_step: the teacher-forced oracle, both maps of every particle by checksum, the
scan match within POSE_TOL of the oracle's solve) and on the pillar hall of tests/_window_checks.py (180 beams).  What the host
derives from a group's block -- poses, log-likelihoods and iteration counts, and the counters fed from the block's statistics, patch
counts and status words -- is compared with the single-stream schedule's, bit for bit."""
import math
import os

import numpy as np

import _oracle as O
import _step_group_checks as S
import _window_checks as W


class groups_env:
    """LAMA_HIP_STEP_GROUPS is read when a context is created (None: the default of three groups)"""

    def __init__(self, groups):
        self.groups = groups

    def __enter__(self):
        self.saved = os.environ.get("LAMA_HIP_STEP_GROUPS")
        if self.groups is None:
            os.environ.pop("LAMA_HIP_STEP_GROUPS", None)
        else:
            os.environ["LAMA_HIP_STEP_GROUPS"] = str(self.groups)

    def __exit__(self, *a):
        if self.saved is None:
            os.environ.pop("LAMA_HIP_STEP_GROUPS", None)
        else:
            os.environ["LAMA_HIP_STEP_GROUPS"] = self.saved


def _start(P, x, y, yaw):
    return np.stack([O.se2(x + W.OFFSETS[i % 3][0] + 0.02, y + W.OFFSETS[i % 3][1] - 0.015, yaw + 0.004 * (i % 7 + 1)) for i in range(P)])


def _resample_plan(P, k):
    """somebody dies, somebody is copied, another pattern every time; particles change blocks where there are several"""
    idx = np.arange(P, dtype=np.int32)
    if P == 1:
        return None
    idx[(2 * k + 1) % P] = idx[(5 * k) % P]
    if P > 4:
        idx[(3 * k + 2) % P] = idx[P - 1 - k % 2]
    return idx if len(set(idx.tolist())) < P else None


STOPS = ((0.3, 0.1, 0.05), (0.7, 0.3, 0.1), (1.2, 0.4, 0.02), (1.6, 0.2, -0.06), (2.1, 0.0, -0.02))


def run_schedule(F, P, groups, l2_max=None, stops=STOPS, every_scan=True, window=24):
    """`stops` steps through the hall with a resample after every second one, under `groups` (None: default, 1: single-stream).
    Every step is checked against the oracle by S.device_step (poses within POSE_TOL, log-likelihoods, both maps).  -> per step the
    poses the device matched, the group count, the counters.  (Log-likelihoods and iteration counts bit for bit between two
    schedules: check_results_bit_equal.)"""
    with groups_env(groups):
        pr = W.Pair(F, P, W._w(window, l2_max), W.START[0], W.START[1], 0.0, scan=W.scan_at(W.START[0], W.START[1], 0.0))
    ctx, out = pr.ctx, []
    for k, (dx, dy, yaw) in enumerate(stops):
        x, y = W.START[0] + dx, W.START[1] + dy
        start = _start(P, x, y, yaw)
        last = k == len(stops) - 1
        S.device_step(F, ctx, pr.pf, start, W.scan_at(x, y, yaw), f"P {P} groups {groups} step {k}", check_maps=every_scan or last)
        out.append((pr.pf.poses().copy(),))              # (= the device's: device_step has set the oracle's particles to them)
        idx = _resample_plan(P, k) if k % 2 == 1 and not last else None
        if idx is not None:
            pr.pf.stage_resample_with(idx)
            ctx.resample(idx)
    ran = ctx.step_groups()
    c = ctx.counters()
    pr.assert_maps("after the last step", slots=sorted({0, P // 2, P - 1}))
    pr.close()
    return out, ran, c


# counters that are sums over what the groups' blocks bring home (statistics, patch counts, status words)
BLOCK_COUNTERS = ("ray_cells", "bf_cells", "dm_patches", "occ_patches", "brushfire_handovers", "replay_handovers", "parallel_raycast_scans")


def check_grouped_equals_single_stream_equals_oracle(F, P, groups, blocks, l2_max=None, stops=STOPS, every_scan=True):
    """the same steps under `groups` and under the single-stream schedule: each against the oracle (device_step), and against each
    other bit for bit in the matched poses; the counters that the blocks feed are equal.  `blocks`: how many groups must have run"""
    got, ran, c = run_schedule(F, P, groups, l2_max=l2_max, stops=stops, every_scan=every_scan)
    assert ran == blocks, (ran, blocks)
    one, ran1, c1 = run_schedule(F, P, 1, l2_max=l2_max, stops=stops, every_scan=every_scan)
    assert ran1 == 1
    for k, (g, s) in enumerate(zip(got, one)):
        assert np.array_equal(g[0], s[0]), (P, groups, k)
    for n in BLOCK_COUNTERS:
        assert c[n] == c1[n], (n, c[n], c1[n])
    assert c["ray_cells"] > 0 and c["bf_cells"] > 0
    return c


def check_results_bit_equal(F, P, groups, blocks, l2_max=None, stops=STOPS[:3]):
    """what lama_hip_pf_match_and_map hands back -- poses, log-likelihoods, iteration counts: the block's first three arrays -- on the
    step path of the groups and under the single-stream schedule, from the same start poses on the same maps: bit for bit, every
    step, no other call in between"""
    res = []
    for gr in (groups, 1):
        with groups_env(gr):
            ctx = F.HipContext(F.default_cfg(particles=P, **W._w(24, l2_max)))
        ctx.init(W.scan_at(W.START[0], W.START[1], 0.0), O.se2(W.START[0], W.START[1], 0.0))
        steps = []
        for dx, dy, yaw in stops:
            x, y = W.START[0] + dx, W.START[1] + dy
            steps.append(ctx.match_and_map(W.scan_at(x, y, yaw), _start(P, x, y, yaw)))
        ran = ctx.step_groups()
        steps.append((ctx.map_checksums(F.MAP_DISTANCE), ctx.map_checksums(F.MAP_OCCUPANCY), ctx.get_poses()))
        c = ctx.counters()
        ctx.close()
        res.append((steps, ran, c))
    assert res[0][1] == blocks and res[1][1] == 1, (res[0][1], res[1][1])
    for k, (a, b) in enumerate(zip(res[0][0], res[1][0])):
        for u, v in zip(a, b):
            assert np.array_equal(u, v), (P, groups, k)
    assert int(np.min(res[0][0][0][2])) >= 1                 # the scan match iterated: the poses are not the start poses
    for n in BLOCK_COUNTERS:
        assert res[0][2][n] == res[1][2][n], (n, res[0][2][n], res[1][2][n])


def check_directory_rows(F, direction, groups=3, P=3, window=16, l2_max=None, reach=10.0):
    """A drive along +y / -y under groups until the window has moved: the mapped box then ends on the window's row 0 (+y: the
    origin follows the box's low end) or on its last row (-y), and k_occ_reverse_dir scans exactly the box's rows.  A patch in a row
    it skipped would keep a stale reverse entry: the ray-cast would then write its cells to another patch and the checksums against
    the oracle, taken after every step, differ.  -> (lowest, highest) window row the box was seen on"""
    d = W.DIRECTIONS[direction]
    assert d[0] == 0
    heading = math.atan2(d[1], d[0])
    with groups_env(groups):
        pr = W.Pair(F, P, W._w(window, l2_max), W.START[0], W.START[1], heading)
    ctx = pr.ctx
    c0 = ctx.counters()
    seen = []
    t = 0.0
    while t < reach:
        t += 2.0
        x, y = W.START[0], W.START[1] + t * d[1]
        S.device_step(F, ctx, pr.pf, _start(P, x, y, heading), W.scan_at(x, y, heading), f"{direction} t = {t}")
        h = W.export_blob(F, ctx, 0).header()
        seen.append((int(h[7]) & 0xFFFF, (int(h[7]) >> 16) & 0xFFFF, int(h[5])))
    c = ctx.counters()
    assert ctx.step_groups() == min(groups, P)
    assert c["window_shifts"] > c0["window_shifts"], (c0, c)
    pr.assert_maps(f"{direction}: after the drive")
    pr.close()
    return seen
