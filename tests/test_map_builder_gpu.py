"""lama::MapBuilder2D and the two device entry points under it (lama_hip_map_integrate_scans, lama_hip_map_occupied_cells) against
the reference's own map rebuild (GraphSlam2D::generateOccupancyMap, src/graph_slam2d.cpp:131-164) composed from the compiled
reference's primitives (tests/_mapbuild.py): patch ids, every cell's bytes and all mask words bit for bit."""
import numpy as np
import pytest

import _mapbuild as MB
import _reference as R
import iris_lama_amd.ffi as F
from _cmp import DM_FIELDS, OCC_FIELDS, assert_maps_equal
from _posegraph import make_graph

pytestmark = pytest.mark.gpu


def _ctx(**kw):
    return F.HipContext(F.default_cfg(particles=1, **kw))


def _occ(ctx):
    return ctx.download_map(0, F.MAP_OCCUPANCY)


@pytest.mark.parametrize("full,sensor", [(True, False), (False, False), (True, True), (False, True)])
def test_rebuild_of_a_random_room_from_40_posed_scans(full, sensor):
    poses4, _, scans, origins, quats = MB.room_log(3 if sensor else 2, K=40, beams=360, sensor=sensor)
    ref = MB.build(poses4, scans, origins, quats, full=full)
    ctx = _ctx()
    ctx.integrate_scans(0, poses4, scans, origins, quats, full=full, prune=False)
    dev = _occ(ctx)
    assert len(dev) > 8
    assert_maps_equal(dev, ref.dump(), OCC_FIELDS, f"full {full} sensor {sensor}")
    assert len(ctx.download_map(0, F.MAP_DISTANCE)) == 0           # the distance map is not touched
    ctx.close()


def test_coarse_variant_at_a_tenth_of_a_metre():
    poses4, _, scans, _, _ = MB.room_log(5, K=20, beams=360)
    ref = MB.build(poses4, scans, full=False, resolution=0.1)
    b = F.MapBuilder2D(full=0, resolution=0.1, prune=0, l2_max=0.0)
    for k in range(len(scans)):
        b.add(scans[k], poses4[k])
    b.build()
    assert_maps_equal(_occ(b.hip_context()), ref.dump(), OCC_FIELDS, "coarse")
    assert b.view_cells(1) is None                                  # l2_max 0: no distance map
    b.close()


def test_split_order_and_incremental_builds_give_the_same_map():
    poses4, _, scans, origins, quats = MB.room_log(7, K=40, beams=240, sensor=True)
    want = MB.build(poses4, scans, origins, quats, full=True).dump()
    a = 17
    ctx = _ctx()
    ctx.integrate_scans(0, poses4[:a], scans[:a], origins[:a], quats[:a], prune=False)
    ctx.integrate_scans(0, poses4[a:], scans[a:], origins[a:], quats[a:], prune=False)
    assert_maps_equal(_occ(ctx), want, OCC_FIELDS, "two calls")
    ctx.close()
    perm = np.random.default_rng(0).permutation(len(scans))
    ctx = _ctx()
    ctx.integrate_scans(0, poses4[perm], [scans[i] for i in perm], origins[perm], quats[perm], prune=False)
    assert_maps_equal(_occ(ctx), want, OCC_FIELDS, "shuffled")
    ctx.close()
    b = F.MapBuilder2D(prune=0)
    for k in range(a):
        assert b.add(scans[k], poses4[k], origins[k], quats[k]) == k
    b.build()
    for k in range(a, len(scans)):
        b.add(scans[k], poses4[k], origins[k], quats[k])
    b.build()
    assert_maps_equal(_occ(b.hip_context()), want, OCC_FIELDS, "build, add, build")
    b.build()                                                       # nothing new: nothing changes
    assert_maps_equal(_occ(b.hip_context()), want, OCC_FIELDS, "third build")
    b.close()


def test_prune_on_and_off():
    poses4, _, scans, _, _ = MB.room_log(9, K=6, beams=200)         # few scans: many cells seen once
    raw = MB.build(poses4, scans, full=True).dump()
    want = MB.pruned(raw)
    assert sum(int((c["visited"] != w["visited"]).sum()) for (c, _), (w, _) in zip(raw.values(), want.values())) > 50
    for prune, exp in ((False, raw), (True, want)):
        ctx = _ctx()
        ctx.integrate_scans(0, poses4, scans, full=True, prune=prune)
        assert_maps_equal(_occ(ctx), exp, OCC_FIELDS, f"prune {prune}")
        ctx.close()


def test_counters_wrap_per_field_inside_one_launch():
    """One posed scan of three points repeated in the scan list of ONE call: the hit cells collect more than 65,535 hits, the
    cells on the rays more than 65,535 free visits.  Expected by arithmetic modulo 2^16 per field from the reference's map of a
    single repetition (every repetition adds the same counts), cross-checked against the reference at 3 repetitions."""
    pose = R.pose_from_xyr(0.3, -0.2, 0.4)
    scan = np.array([[2.0, 0.1, 0.0], [1.5, 1.2, 0.0], [2.0, 0.1, 0.0]])       # one cell hit twice per repetition
    one = MB.build([pose], [scan], full=True).dump()

    def times(rep):
        out = {}
        for pid, (cells, mask) in one.items():
            c = cells.copy()
            c["occupied"] = (cells["occupied"].astype(np.uint64) * rep % 65536).astype(np.uint16)
            c["visited"] = (cells["visited"].astype(np.uint64) * rep % 65536).astype(np.uint16)
            out[pid] = (c, mask.copy())
        return out

    ref3 = MB.build([pose] * 3, [scan] * 3, full=True).dump()
    assert_maps_equal(times(3), ref3, OCC_FIELDS, "the arithmetic against the reference at 3 repetitions")
    for rep in (3, 40000, 65536, 65536 + 5):
        ctx = _ctx()
        ctx.integrate_scans(0, np.tile(pose, (rep, 1)), (np.tile(scan, (rep, 1)), np.arange(rep + 1) * 3), full=True, prune=False)
        dev = _occ(ctx)
        assert_maps_equal(dev, times(rep), OCC_FIELDS, f"{rep} repetitions")
        ctx.close()
    hits = max(int(c["occupied"].max()) for c, _ in one.values())
    assert hits == 2 and 40000 * hits > 65535                      # 40,000 repetitions: the doubly hit cell wraps, occupied alone


def test_accumulation_onto_a_map_that_update_maps_populated():
    poses4, xyr, scans, _, _ = MB.room_log(11, K=10, beams=240)
    ctx = _ctx()
    ctx.init(scans[0], poses4[0])
    ctx.set_poses(poses4[1:2])
    ctx.update_maps(scans[1])
    before = _occ(ctx)
    assert len(before) > 4
    # the reference: the same loop on a reference map that holds the same cells
    occ = R.Occ.new(0.05)
    for pid, (cells, mask) in before.items():
        ax, ay = (pid // 2642244) * 32, (pid % 2642244) * 32
        for ci in np.nonzero(cells["visited"])[0]:
            o, v = int(cells["occupied"][ci]), int(cells["visited"][ci])
            for _ in range(o):
                occ.set_occupied(ax + (int(ci) & 31), ay + (int(ci) >> 5))
            for _ in range(v - o):
                occ.set_free(ax + (int(ci) & 31), ay + (int(ci) >> 5))
    MB.integrate(occ, R.DM.new(0.05), poses4[2:], scans[2:], full=True)
    dm_before = ctx.map_checksums(F.MAP_DISTANCE)
    ctx.integrate_scans(0, poses4[2:], scans[2:], full=True, prune=False)
    got, want = _occ(ctx), occ.dump()
    assert_maps_equal(got, want, OCC_FIELDS, "accumulated")
    assert np.array_equal(ctx.map_checksums(F.MAP_DISTANCE), dm_before)
    ctx.close()


def test_error_paths_leave_the_map_untouched():
    poses4, _, scans, _, _ = MB.room_log(13, K=8, beams=200)
    ctx = _ctx()
    ctx.integrate_scans(0, poses4, scans)
    cks = ctx.map_checksums(F.MAP_OCCUPANCY)
    far = R.pose_from_xyr(1016 * 32 * 0.05 + 50.0, 0.0, 0.0)       # beyond the largest window (1016 patches) from the map so far
    rc = ctx.L.lama_hip_map_integrate_scans(ctx.h, 0, 1, F._p(np.ascontiguousarray(far)), F._p(np.ascontiguousarray(scans[0])),
                                            F._p(np.array([0, len(scans[0])], dtype=np.uint32)), None, None, 3)
    assert rc == -3, rc                                             # LAMA_HIP_E_WINDOW
    assert np.array_equal(ctx.map_checksums(F.MAP_OCCUPANCY), cks)
    with pytest.raises(F.LamaError):                                # a ray longer than the closed form's 8191 cells
        ctx.integrate_scans(0, poses4[:1], [np.array([[500.0, 0.0, 0.0]])])
    with pytest.raises(F.LamaError):
        ctx.integrate_scans(0, poses4[:1], [np.array([[np.nan, 0.0, 0.0]])])
    assert np.array_equal(ctx.map_checksums(F.MAP_OCCUPANCY), cks)
    ctx.integrate_scans(0, np.zeros((0, 4)), [])                    # num_scans = 0
    ctx.integrate_scans(0, poses4[:3], [np.zeros((0, 3))] * 3)      # empty scans
    assert np.array_equal(ctx.map_checksums(F.MAP_OCCUPANCY), cks)
    ctx.integrate_scans(0, poses4[:2], [scans[0], np.zeros((0, 3))], prune=False)      # an empty scan among others contributes nothing
    assert not np.array_equal(ctx.map_checksums(F.MAP_OCCUPANCY), cks)
    ctx.close()
    fresh = _ctx()                                                  # on a fresh context the same refusals, and nothing is placed
    with pytest.raises(F.LamaError):
        fresh.integrate_scans(0, poses4[:1], [np.array([[500.0, 0.0, 0.0]])])
    assert len(_occ(fresh)) == 0
    fresh.integrate_scans(0, poses4, scans)
    assert np.array_equal(fresh.map_checksums(F.MAP_OCCUPANCY), cks)
    fresh.close()


@pytest.mark.parametrize("l2_max", [0.5, 7.0])
def test_occupied_cells_distance_map_and_solve(l2_max):
    """Both device libraries: l2_max 0.5 m (10 cells) and 7 m (140 cells: the wide library)."""
    poses4, xyr, scans, _, _ = MB.room_log(17, K=30, beams=360)
    ref = MB.pruned(MB.build(poses4, scans, full=True).dump())
    want_cells = MB.occupied_cells(ref)
    b = F.MapBuilder2D(l2_max=l2_max)
    assert b.engine_origin().endswith("liblama_hip_wide.so" if l2_max > 6.35 else "liblama_hip.so")
    for k in range(len(scans)):
        b.add(scans[k], poses4[k])
    b.build()
    ctx = b.hip_context()
    assert_maps_equal(_occ(ctx), ref, OCC_FIELDS, "occupancy")
    assert len(want_cells) > 300
    assert np.array_equal(ctx.occupied_cells(0), want_cells)        # same cells, same order
    assert np.array_equal(b.occupied_cells(), want_cells)
    dm = MB.distance_map_of(want_cells, l2_max)
    assert_maps_equal(ctx.download_map(0, F.MAP_DISTANCE), dm.dump(), DM_FIELDS, f"distance map, l2_max {l2_max}")
    cells = b.view_cells(1)
    assert cells is not None and len(cells) > len(want_cells)
    # lama::Solve on getDistanceMap() against the reference's solver on the reference's map
    for k in (3, 11):
        start = xyr[k] + np.array([0.05, -0.04, 0.02])
        got, _ = b.match_solve(scans[k], R.pose_from_xyr(*start))
        want = R.solve(dm, scans[k], start)
        assert np.max(np.abs(got - want)) < 1e-8, (got, want)
    # a second build after new poses replaces both maps
    b.set_poses(poses4[::-1].copy())
    b.build()
    ref2 = MB.pruned(MB.build(poses4[::-1], scans, full=True).dump())
    assert_maps_equal(_occ(ctx), ref2, OCC_FIELDS, "rebuilt occupancy")
    assert_maps_equal(ctx.download_map(0, F.MAP_DISTANCE), MB.distance_map_of(MB.occupied_cells(ref2), l2_max).dump(), DM_FIELDS, "rebuilt distance map")
    b.reset()
    assert b.view_cells(0) is None and len(_occ(ctx)) == 0
    b.close()


def test_end_to_end_with_simple_pgo():
    N = 40
    fi, fj, meas, sq, truth, init = make_graph(N, 30, seed=5)
    rng = np.random.default_rng(5)
    kind = {"R": 60.0, "coef": [(m, rng.uniform(0.02, 0.08), rng.uniform(0, 2 * np.pi)) for m in (2, 3, 5, 7)]}
    import math
    from _stress import random_room_scan
    scans = [random_room_scan(rng, (t[2], t[3], math.atan2(t[1], t[0])), 240, kind)[::3] for t in truth]      # seen from the true poses
    b = F.MapBuilder2D()
    for k in range(N):
        b.add(scans[k], init[k])                                   # dead reckoning first
    b.build()
    edges = [(int(fi[k]), int(fj[k]), meas[k]) for k in range(N, len(fi))]
    ok, opt, rep = F.simple_pgo(init, edges)
    assert ok and rep["final_error"] < rep["initial_error"]
    b.set_poses(opt)
    b.build()
    ref = MB.pruned(MB.build(opt, scans, full=True).dump())
    assert_maps_equal(_occ(b.hip_context()), ref, OCC_FIELDS, "map at the optimised poses")
    cells = MB.occupied_cells(ref)
    assert np.array_equal(b.occupied_cells(), cells)
    assert_maps_equal(b.hip_context().download_map(0, F.MAP_DISTANCE), MB.distance_map_of(cells, 0.5).dump(), DM_FIELDS, "distance map")
    b.close()
