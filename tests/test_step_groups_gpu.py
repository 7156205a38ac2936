"""-m gpu: the grouped step schedule of small pools (lama_hip_pf_match_and_map, include/lama_hip.h): lama::PFSlam2D::update on one
shard runs predict -> device step (scan match, then the map update of the matched poses, queued) -> resample if due, and a pool
below 64 particles runs the device step as up to four particle groups on streams of their own.

What must hold: the order swap and the groups change NOTHING -- poses, weights and both maps of every particle equal, bit for bit,
those of the same object forced to the single-stream schedule (LAMA_HIP_STEP_GROUPS=1), and the maps equal the CPU oracle's, which
resamples BEFORE it updates the maps like the reference.  Against the oracle the poses are compared as the free-running tests of
tests/test_gpu_parity.py do (1e-6 m: device and host trig differ in the last bits and the filter runs free); weights and Neff
follow the poses (normalised weights lie in [0, 1]: 1e-6 absolute, Neff 1e-6 relative as there).
"""
import os
import re

import numpy as np
import pytest

import _oracle as O
import _step_group_checks as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import iris_lama_amd.ffi as f
    if f.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need the MI355X box (there is no CPU fallback)")
    return f


def _with_groups(groups):
    """the environment override is read when a context is created"""
    class _Env:
        def __enter__(self):
            self.saved = os.environ.get("LAMA_HIP_STEP_GROUPS")
            if groups is None:
                os.environ.pop("LAMA_HIP_STEP_GROUPS", None)
            else:
                os.environ["LAMA_HIP_STEP_GROUPS"] = str(groups)

        def __exit__(self, *a):
            if self.saved is None:
                os.environ.pop("LAMA_HIP_STEP_GROUPS", None)
            else:
                os.environ["LAMA_HIP_STEP_GROUPS"] = self.saved
    return _Env()


def _host_run(F, groups, P, beams, scans, seed=42, maps_every_scan=True, **opts):
    """lama::PFSlam2D free running on the corridor log -> per scan: update()'s result, poses, the three weight arrays, Neff, best
    particle, resamples so far, checksums of both maps of every particle; and the group count the device steps ran with.
    maps_every_scan=False: the checksums (a call that waits for all groups) are taken after the last scan only, so the steps follow
    each other as in a running filter: the status of a group's map update arrives with its next scan match"""
    pts, odom, truth = F.corridor_log(scans, beams)
    with _with_groups(groups):
        h = F.PFSlam2D(F.pf_options(particles=P, seed=seed, create_summary=0, **opts))       # (a Summary keeps the reference's order)
    assert h.engine_origin().endswith("liblama_hip.so")
    h.set_prior(*odom[0])
    ctx = h.hip_context()
    out = []
    for k in range(scans + 1):
        r = h.update(pts[k], odom[k], float(k))
        maps = maps_every_scan or k == scans
        out.append(dict(r=r, poses=h.poses().copy(), w=[a.copy() for a in h.weights()], neff=h.neff(), best=h.best(), resamples=h.num_resamples(),
                        dm=ctx.map_checksums(F.MAP_DISTANCE) if maps else None, occ=ctx.map_checksums(F.MAP_OCCUPANCY) if maps else None))
    ran = ctx.step_groups()
    c = ctx.counters()
    h.close()
    return out, ran, c


def _oracle_run(F, P, beams, scans, seed=42, **opts):
    pts, odom, truth = F.corridor_log(scans, beams)
    o = O.PF(O.default_options(particles=P, seed=seed, **opts))
    o.set_prior(O.se2(*odom[0]))
    out = []
    for k in range(scans + 1):
        r = o.update(pts[k], O.se2(*odom[k]), float(k))
        out.append(dict(r=r, poses=o.poses().copy(), w=[a.copy() for a in o.weights()], neff=o.neff(), best=o.best(), resamples=o.num_resamples(),
                        dm=o.map_checksums(0), occ=o.map_checksums(1)))
    return out


def _assert_same_run(got, want, what):
    """two runs of the device path: everything bit for bit"""
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["r"] == w["r"] and g["resamples"] == w["resamples"] and g["best"] == w["best"], (what, k)
        assert np.array_equal(g["poses"], w["poses"]), (what, k)
        for a, b in zip(g["w"], w["w"]):
            assert np.array_equal(a, b), (what, k)
        assert g["neff"] == w["neff"], (what, k)
        assert np.array_equal(g["dm"], w["dm"]), f"{what}: distance maps after scan {k}"
        assert np.array_equal(g["occ"], w["occ"]), f"{what}: occupancy maps after scan {k}"


def _assert_tracks_oracle(got, want, what):
    for k, (g, o) in enumerate(zip(got, want)):
        assert g["r"] == o["r"] and g["resamples"] == o["resamples"] and g["best"] == o["best"], (what, k)
        assert np.abs(g["poses"] - o["poses"]).max() < 1e-6, (what, k, np.abs(g["poses"] - o["poses"]).max())
        assert np.abs(g["w"][1] - o["w"][1]).max() < 1e-6, (what, k)                                     # normalised weights
        for j in (0, 2):                                                                                # weight, weight_sum
            assert np.abs(g["w"][j] - o["w"][j]).max() <= 1e-6 * max(1.0, np.abs(o["w"][j]).max()), (what, k, j)
        assert abs(g["neff"] - o["neff"]) <= 1e-6 * max(1.0, o["neff"]), (what, k)
        assert np.array_equal(g["dm"], o["dm"]), f"{what}: distance maps after scan {k}"
        assert np.array_equal(g["occ"], o["occ"]), f"{what}: occupancy maps after scan {k}"


# ---- 1. grouped = ungrouped = oracle, with resamples: 7 particles (uneven blocks for 2, 3 and 4 groups), 180 beams, 14 scans, a gain
# with which the filter resamples in about every second step
RESAMPLING = dict(P=7, beams=180, scans=14, meas_sigma_gain=0.01)
_shared = {}


def _resampling_references(F):
    if not _shared:
        _shared["oracle"] = _oracle_run(F, **RESAMPLING)
        _shared["single"], ran, _ = _host_run(F, 1, **RESAMPLING)
        assert ran == 0                                   # an override of 1: the reference's order through the three separate calls
    return _shared["oracle"], _shared["single"]


@pytest.mark.parametrize("groups", [1, 2, 3, 4])
def test_grouped_equals_ungrouped_equals_oracle_with_resamples(F, groups):
    oracle, single = _resampling_references(F)
    assert oracle[-1]["resamples"] > 0 and 0 < sum(1 for a, b in zip(oracle, oracle[1:]) if b["resamples"] > a["resamples"]) < RESAMPLING["scans"]
    got, ran, c = (single, 0, None) if groups == 1 else _host_run(F, groups, **RESAMPLING)
    assert ran == (groups if groups > 1 else 0)
    assert got[-1]["resamples"] > 0                       # the swap of resample and map update has been exercised
    _assert_same_run(got, single, f"{groups} groups against the single-stream schedule")
    _assert_tracks_oracle(got, oracle, f"{groups} groups against the oracle")


# ---- 2. the benchmark's pool: default gain, 30 particles, 1080 beams, 8 scans, the default number of groups
def test_default_groups_30_particles_equal_the_single_stream_schedule(F):
    kw = dict(P=30, beams=1080, scans=8, maps_every_scan=False)
    single, ran1, _ = _host_run(F, 1, **kw)
    got, ran, c = _host_run(F, None, **kw)
    assert ran1 == 0 and ran == 3                         # the documented default: three groups (10 + 10 + 10)
    assert c["brushfire_mode"] == 0
    _assert_same_run(got, single, "default groups against the single-stream schedule")
    print("default step groups at 30 particles:", ran)


# ---- 3. degenerate splits: more groups than particles
@pytest.mark.parametrize("P", [1, 2, 3])
def test_four_groups_for_one_two_and_three_particles(F, P):
    kw = dict(P=P, beams=90, scans=6)
    got, ran, _ = _host_run(F, 4, **kw)
    assert ran == P                                       # one particle per group, the other groups are empty and do not run
    _assert_tracks_oracle(got, _oracle_run(F, **kw), f"{P} particles in 4 groups")


# ---- 4. rare paths under groups (drained, then today's code on the main stream)
@pytest.mark.parametrize("groups,every_scan", [(2, True), (3, False), (4, False)])
def test_window_moves_and_grows_under_groups(F, groups, every_scan):
    with _with_groups(groups):
        S.check_window_moves_and_grows(F, groups, P=max(3, groups), every_scan=every_scan)       # (a particle per group at least)


@pytest.mark.parametrize("groups,every_scan", [(3, True), (2, False), (4, False)])
def test_clean_abort_grows_the_arenas_under_groups(F, groups, every_scan):
    with _with_groups(groups):
        S.check_clean_abort_grows_the_arenas(F, groups, P=max(3, groups), every_scan=every_scan)


# ---- 4b. a scan that cannot be grouped is one scan on one stream, not the end of the groups
def test_groups_resume_after_the_wrap_guard_probe(F):
    """A uint16 `visited` counter could wrap inside a scan once the host's bound of the largest counter plus the scan's beams reaches
    65536: that scan runs the probe and today's code on the main stream (the bound grows by the beams of every scan: every 16th scan
    at 4000 beams).  The scans after it must be grouped again.  Run A asks after every step how many groups it ran (a call that waits
    for the device) and so finds the ungroupable steps; run B makes the same steps with no other call in between -- the state a
    running filter is in -- and must be back at three groups after them; its maps equal A's and the single-stream schedule's."""
    scans, P = 19, 3
    pts, odom, truth = F.corridor_log(scans, 4000)
    assert all(len(p) <= 4000 for p in pts) and sum(len(p) for p in pts[:17]) > 65536

    def run(groups, ask):
        with _with_groups(groups):
            ctx = F.HipContext(F.default_cfg(particles=P))
        ctx.init(pts[0], O.se2(*odom[0]))
        ran, poses = [], None
        for k in range(1, scans + 1):
            start = np.stack([O.se2(truth[k][0] + 0.01 * i, truth[k][1] - 0.008 * i, truth[k][2] + 0.002 * i) for i in range(P)])
            poses, ll, it = ctx.match_and_map(pts[k], start)
            if ask:
                ran.append(ctx.step_groups())
        ran.append(ctx.step_groups())
        out = (poses, ctx.map_checksums(F.MAP_DISTANCE), ctx.map_checksums(F.MAP_OCCUPANCY), ctx.counters())
        ctx.close()
        return ran, out
    ran_a, a = run(3, True)
    single = [k for k, r in enumerate(ran_a[:-1]) if r == 1]
    assert single and set(ran_a) == {1, 3}, ran_a                     # some scan ran on one stream ...
    assert all(ran_a[k + 1] == 3 for k in single) and single[-1] < scans - 2, ran_a      # ... and the next one in three groups again
    assert a[3]["parallel_raycast_scans"] + a[3]["sequential_raycast_scans"] == scans + 1
    ran_b, b = run(3, False)
    assert ran_b == [3], ran_b
    _, one = run(1, False)
    for x, y, z in zip(a[:3], b[:3], one[:3]):
        assert np.array_equal(x, y) and np.array_equal(x, z)


# ---- 5. a deferred device error of one group's map update
@pytest.mark.parametrize("next_call", ["sync", "step"])
def test_deferred_error_of_a_group_surfaces_in_the_next_call(F, next_call):
    """One return 2 km away makes the scan's box wider than the largest window (1016 patches = 1.6 km): the window stays, the map
    update's allocation phase reports the cells outside it and modifies nothing -- an error of a QUEUED update.  It is returned by
    the next call on the context, and afterwards the context works on: with three groups exactly as with the single-stream schedule
    (same status, same maps after the next good step)."""
    pts, odom, truth = F.corridor_log(3, 180)
    pose0 = O.se2(*odom[0])
    bad = np.vstack([pts[1], [[2000.0, 0.0, 0.0]]])
    sums = []
    for groups in (1, 3):
        with _with_groups(groups):
            ctx = F.HipContext(F.default_cfg(particles=3))
        ctx.init(pts[0], pose0)
        start = np.stack([O.se2(truth[1][0] + 0.01 * i, truth[1][1] - 0.01 * i, truth[1][2]) for i in range(3)])
        ctx.match_and_map(bad, start)                                    # queued: no error yet
        with pytest.raises(F.LamaError, match=r"deferred from .*window") as ei:
            if next_call == "sync":
                ctx.sync()
            else:
                ctx.match_and_map(pts[2], start)
        start2 = np.stack([O.se2(truth[2][0] + 0.01 * i, truth[2][1] - 0.01 * i, truth[2][2]) for i in range(3)])
        poses, ll, it = ctx.match_and_map(pts[2], start2)
        assert ctx.step_groups() == groups
        sums.append((re.search(r"status (-\d+)", str(ei.value)).group(1), poses, ll, ctx.map_checksums(F.MAP_DISTANCE), ctx.map_checksums(F.MAP_OCCUPANCY)))
        ctx.close()
    assert sums[0][0] == sums[1][0]
    for a, b in zip(sums[0][1:], sums[1][1:]):
        assert np.array_equal(a, b)
