"""Checks of the transient-map bookkeeping behind Slam2D (transient_map) and LidarOdometry2D -- lama_hip_pf_patch_ids,
lama_hip_pf_delete_patches (iris_lama_amd/csrc/lama_hip.hip) and the log-odds cell policy of k_raycast (lama_kernels.h) -- case by
case, shared by tests/test_transient_gpu.py and the lane-simulator tests (tests/test_transient_sim.py).

A. The deletion itself needs no oracle: the download before the call, minus the listed ids (assert_deleted).  B. What later
kernels make of a compacted region runs against the CPU oracle, to whose maps the same patches are deleted (Map::deletePatchAt):
the particle filter (O.PF) under the frequency policy, O.LidarOdometry driven through update_maps_at under the log-odds policy
and the last-metre ray rule.  Every comparison is bit for bit (assert_maps_equal, array_equal); no tolerance anywhere.

Construction as in tests/_ray_checks.py: resolution 0.05 m, the sensor on a cell centre at yaw 0, points on the cell lattice, so a
case names its obstacle cells.  Cells are written relative to the map's origin cell (OFF, OFF), patches relative to its patch.
Every case first asserts ON THE ORACLE that it reaches the situation it is named after (the patch is absent before the update and
back after it, the tie branch ran, the clamps are reached, ...): a case that stops exercising its branch fails.
"""
import ctypes as C
import itertools

import numpy as np

import _oracle as O
import _raster as RS
import _ray_checks as RC
import _window_checks as W
from _cmp import DM_FIELDS, OCC_FIELDS, assert_maps_equal

UC = RS.UC
OFFP = UC >> 1                     # the patch of the map's origin cell
OFF = OFFP * 32
E_INVALID = -1


def pid(px, py):
    """id of the patch (px, py) counted from the origin's patch"""
    return (OFFP + px) * UC + (OFFP + py)


def cell_of(dump, x, y):
    """the record of cell (x, y) (relative to the origin cell) in a dump, with its mask bit -> (record or None, bit)"""
    p = pid(x >> 5, y >> 5)
    if p not in dump:
        return None, False
    ci = (x & 31) | ((y & 31) << 5)
    return dump[p][0][ci], bool((int(dump[p][1][ci >> 6]) >> (ci & 63)) & 1)


def is_obstacle(dump, x, y):
    c, _ = cell_of(dump, x, y)
    return c is not None and bool(c["valid"]) and int(c["sqdist"]) == 0


def beams(sensor, hits):
    """(pose, points) of a sensor on cell `sensor` whose beams end in the cells `hits`; the deltas are asserted"""
    deltas = [(hx - sensor[0], hy - sensor[1]) for hx, hy in hits]
    pose, pts = RC.sensor(*sensor), RC.lattice(deltas)
    RC.assert_deltas(pose, pts, deltas, f"beams from {sensor}")
    return pose, pts


def reach_cells(l2_max):
    return int(np.ceil((0.5 if l2_max is None else l2_max) / 0.05))


def _cfg(l2_max, **kw):
    return dict(kw) if l2_max is None else dict(kw, l2_max=l2_max)


def map_patches(ctx, particle, kind):
    n = C.c_uint32(0)
    assert ctx.L.lama_hip_pf_map_patches(ctx.h, particle, kind, C.byref(n)) == 0
    return int(n.value)


def downloads(F, ctx, particle):
    return ctx.download_map(particle, F.MAP_DISTANCE), ctx.download_map(particle, F.MAP_OCCUPANCY)


def oracle_delete(pf, particle, ids):
    """Map::deletePatchAt on both maps of an oracle particle, in list order -> distance-map patches removed"""
    n = 0
    for i in ids:
        pf.occ(particle).delete_patch(i)
        n += 1 if pf.dm(particle).delete_patch(i) else 0
    return n


def assert_deleted(F, ctx, pf, particle, ids, what, block=None):
    """lama_hip_pf_delete_patches(particle, ids) and everything the interface shows of the particle afterwards, against the downloads
    before the call minus the ids; the checksums against the oracle's maps after the same deletePatchAt calls"""
    before = downloads(F, ctx, particle)
    ids = [int(i) for i in ids]
    deleted = ctx.delete_patches(particle, np.array(ids, dtype=np.uint64))
    want = [{k: v for k, v in b.items() if k not in set(ids)} for b in before]
    assert deleted == len(before[0]) - len(want[0]), (what, deleted)
    assert oracle_delete(pf, particle, ids) == deleted, what
    for kind, w, fields, policy in ((F.MAP_DISTANCE, want[0], DM_FIELDS, 0), (F.MAP_OCCUPANCY, want[1], OCC_FIELDS, 1)):
        got = ctx.download_map(particle, kind)
        assert_maps_equal(got, w, fields, f"{what}: kind {kind}")
        assert ctx.patch_ids(particle, kind).tolist() == sorted(w), (what, kind)
        assert map_patches(ctx, particle, kind) == len(w), (what, kind)
        assert int(ctx.map_checksums(kind)[particle]) == int(pf.map_checksums(policy)[particle]), (what, kind)
        lo, hi, n = ctx.map_bounds(particle, kind)
        wlo, whi = RS.bounds(list(w))
        assert n == len(w) and np.array_equal(lo, wlo) and np.array_equal(hi, whi), (what, kind, lo, hi, n)
    if block is not None:
        x0, y0, width, height = block
        tri = ctx.rasterize(particle, F.RASTER_TRINARY, x0, y0, width, height, 1)
        assert np.array_equal(tri, RS.raster(ctx.download_map(particle, F.MAP_OCCUPANCY), RS.TRINARY, x0, y0, width, height, 1)), what
    return deleted


# ------------------------------------------------------------------------------------------------ A. the deletion itself
# A sensor in patch (1, 0) and one hit in each patch of the block (0 .. 2) x (0 .. 1), each somewhere else in its patch: the six
# patches differ in both maps.  (10, 61) lies 3 cells below patch (0, 2), which the brushfire enters and no ray does: a patch the
# occupancy map lacks.  The beam to (130, 30) crosses patch (3, 0) and ends in (4, 0); the oracle's distance map then loses
# (3, 0) by deletePatchAt: a patch only the occupancy map has.
BLOCK = [(px, py) for py in (0, 1) for px in (0, 1, 2)]
A_SENSOR = (40, 30)
A_HITS = [(10, 12), (50, 8), (80, 20), (12, 50), (45, 52), (85, 45), (10, 61), (130, 30)]
A_SENSORS3 = [(40, 30), (41, 30), (40, 31)]          # P = 3: the second scan from a cell of each particle's own
BLOCK_BOX = (OFF, OFF, 96, 64)


def block_ids():
    return [pid(*b) for b in BLOCK]


def block_filter(P, l2_max):
    """the oracle's filter after the block scan (P = 3: and a second one from three sensor cells), the distance maps without (3, 0)"""
    pose, pts = beams(A_SENSOR, A_HITS)
    pf = O.PF(O.default_options(particles=P, seed=3, **_cfg(l2_max)))
    pf.set_prior(pose)
    assert pf.update(pts, pose)
    if P > 1:
        pf.set_poses(np.stack([RC.sensor(*s) for s in A_SENSORS3[:P]])); pf.stage_set_scan(pts); pf.stage_update_maps()
    for i in range(P):
        assert pf.dm(i).delete_patch(pid(3, 0))
        dm, occ = set(pf.dm(i).patch_ids().tolist()), set(pf.occ(i).patch_ids().tolist())
        assert set(block_ids()) <= (dm & occ) and pid(3, 0) in occ - dm and pid(0, 2) in dm - occ, (sorted(dm), sorted(occ))
    if P > 1:
        assert len({pf.map_checksums(0)[i] for i in range(P)}) == P and len({pf.map_checksums(1)[i] for i in range(P)}) == P
    return pf


def upload_from(F, ctx, pf, particles=None):
    for i in (range(pf.P) if particles is None else particles):
        ctx.upload_map(i, F.MAP_DISTANCE, pf.dm(i).dump())
        ctx.upload_map(i, F.MAP_OCCUPANCY, pf.occ(i).dump())


def outside_ids(F, ctx):
    """ids one patch outside the context's window on each of its four sides (two of them below the window's origin)"""
    ox, oy, side = (int(v) for v in W.window_of(F, ctx))
    assert ox > 1 and oy > 1
    out = [(ox - 1) * UC + oy + 1, (ox + side) * UC + oy + 1, (ox + 1) * UC + oy - 1, (ox + 1) * UC + oy + side]
    return out, (ox, oy, side)


def deletion_lists(name, F=None, ctx=None):
    b = block_ids()
    if name == "every patch alone":
        return [[i] for i in b]
    if name == "every ordered pair":
        return [list(p) for p in itertools.permutations(b, 2)]
    if name == "all patches":
        return None                                                   # (every id either map holds: read from the context)
    assert name == "mixed list"
    absent = [pid(1, 3), pid(-1, 0), pid(7, 7)]
    outside, (ox, oy, side) = outside_ids(F, ctx)
    for i in b + [pid(3, 0), pid(0, 2)]:
        assert ox <= i // UC < ox + side and oy <= i % UC < oy + side
    # duplicates (next to each other and apart), absent ids, ids outside the window, ids only one map holds, valid ids in between
    return [[b[4], outside[0], b[4], absent[0], pid(3, 0), outside[2], b[0], absent[1], outside[1], pid(0, 2), b[0], outside[3], absent[2], b[5], b[4]]]


DELETION_CASES = ("every patch alone", "every ordered pair", "all patches", "mixed list")


def check_deletions(F, name, l2_max=None):
    """one particle: every list of the case from a freshly uploaded map"""
    ctx = F.HipContext(F.default_cfg(particles=1, **_cfg(l2_max)))
    pf = block_filter(1, l2_max)
    upload_from(F, ctx, pf)
    lists = deletion_lists(name, F, ctx)
    if lists is None:
        lists = [sorted(set(pf.dm(0).patch_ids().tolist()) | set(pf.occ(0).patch_ids().tolist()))]
    for k, ids in enumerate(lists):
        if k:
            pf = block_filter(1, l2_max)
            upload_from(F, ctx, pf)
        n = assert_deleted(F, ctx, pf, 0, ids, f"{name}: {[(i // UC - OFFP, i % UC - OFFP) for i in ids]}", BLOCK_BOX)
        assert n >= 1
    if name == "all patches":
        assert n == len(lists[0]) - 1 and downloads(F, ctx, 0) == ({}, {})      # ((3, 0) is not in the distance map)
    ctx.close()


def check_arguments(F, l2_max=None):
    ctx = F.HipContext(F.default_cfg(particles=1, **_cfg(l2_max)))
    pf = block_filter(1, l2_max)
    upload_from(F, ctx, pf)
    before = downloads(F, ctx, 0)
    sums = [int(ctx.map_checksums(k)[0]) for k in (F.MAP_DISTANCE, F.MAP_OCCUPANCY)]
    d = C.c_uint32(77)
    fn = ctx.L.lama_hip_pf_delete_patches
    assert fn(ctx.h, 0, None, 0, C.byref(d)) == 0 and d.value == 0               # n = 0 with a NULL list
    one = np.array([block_ids()[0]], dtype=np.uint64)
    assert fn(ctx.h, 1, one.ctypes.data_as(C.c_void_p), 1, C.byref(d)) == E_INVALID          # particle >= P
    assert fn(ctx.h, 0xFFFFFFFF, one.ctypes.data_as(C.c_void_p), 1, C.byref(d)) == E_INVALID
    assert fn(ctx.h, 0, None, 1, C.byref(d)) == E_INVALID                          # NULL with n > 0
    assert fn(ctx.h, 0, one.ctypes.data_as(C.c_void_p), 0, None) == 0              # n = 0 with a list, no counter
    after = downloads(F, ctx, 0)
    for a, b, f in zip(after, before, (DM_FIELDS, OCC_FIELDS)):
        assert_maps_equal(a, b, f, "refused and empty calls")
    assert sums == [int(ctx.map_checksums(k)[0]) for k in (F.MAP_DISTANCE, F.MAP_OCCUPANCY)]
    assert fn(ctx.h, 0, one.ctypes.data_as(C.c_void_p), 1, None) == 0              # a real deletion without a counter
    assert int(one[0]) not in ctx.patch_ids(0, F.MAP_DISTANCE).tolist() and int(one[0]) not in ctx.patch_ids(0, F.MAP_OCCUPANCY).tolist()
    ctx.close()


def check_deletion_on_a_resampled_particle(F, l2_max=None):
    """P = 3, homes permuted by the resample [2, 0, 0]; lists deleted on particle 1, each from fresh uploads.  Particles 0 and 2
    keep their downloads and checksums."""
    b = block_ids()
    for ids in ([b[0]], [b[5], b[2]], [b[1], b[1], pid(0, 2), pid(3, 0), b[3]]):
        pf = block_filter(3, l2_max)
        ctx = F.HipContext(F.default_cfg(particles=3, **_cfg(l2_max)))
        upload_from(F, ctx, pf)
        ctx.set_poses(pf.poses())
        idx = np.array([2, 0, 0], dtype=np.int32)
        pf.stage_resample_with(idx); ctx.resample(idx)
        for i in range(3):
            assert_maps_equal(ctx.download_map(i, F.MAP_DISTANCE), pf.dm(i).dump(), DM_FIELDS, f"resampled dm p{i}")
            assert_maps_equal(ctx.download_map(i, F.MAP_OCCUPANCY), pf.occ(i).dump(), OCC_FIELDS, f"resampled occ p{i}")
        others = {i: downloads(F, ctx, i) for i in (0, 2)}
        sums = [ctx.map_checksums(k) for k in (F.MAP_DISTANCE, F.MAP_OCCUPANCY)]
        assert_deleted(F, ctx, pf, 1, ids, f"particle 1 of 3: {ids}")
        for i, (dm, occ) in others.items():
            now = downloads(F, ctx, i)
            assert_maps_equal(now[0], dm, DM_FIELDS, f"dm p{i} after a deletion on p1"); assert_maps_equal(now[1], occ, OCC_FIELDS, f"occ p{i}")
            for k, kind in enumerate((F.MAP_DISTANCE, F.MAP_OCCUPANCY)):
                assert ctx.map_checksums(kind)[i] == sums[k][i] == pf.map_checksums(k)[i], (i, kind)
        ctx.close()


# ------------------------------------------------------------------------------------------------ B. later kernels
class PFPair(W.Pair):
    """tests/_window_checks.Pair on a lattice scan, with deletions on both sides"""

    def __init__(self, F, P, sensor, hits, l2_max=None, **cfg):
        pose, pts = beams(sensor, hits)
        super().__init__(F, P, _cfg(l2_max, **cfg), sensor[0] * RC.RES, sensor[1] * RC.RES, 0.0, scan=pts)
        assert np.array_equal(self.pf.poses()[0], pose)
        self.assert_maps("first scan")

    def delete(self, particle, ids, what=""):
        ids = [int(i) for i in ids]
        d = self.ctx.delete_patches(particle, np.array(ids, dtype=np.uint64))
        assert d == oracle_delete(self.pf, particle, ids), what
        self.assert_maps(f"{what}: after the deletion")
        return d

    def scan_from(self, sensors, hits, what):
        """one update: particle i's sensor on cell sensors[i], every beam with the deltas hits - sensors[0]"""
        _, pts = beams(sensors[0], hits)
        self.update(np.stack([RC.sensor(*s) for s in sensors]), pts, what)


# Patches A = (0, 0) and B = (1, 0) share the border x = 32.  OA = (30, 16) in A and OB further into B on the same row: the cells of
# B near the border hold offsets to OA.  The sensor sits at (33, 16) between them.  After A is deleted, scans whose first beam
# passes over OB and ends `far` cells further along +x (beyond the reach of the brushfire plus two cells from A: nothing but the
# obstacle reads can bring A back before the raise wave) free OB's cell until the occupancy policy removes the obstacle.
DA, DB = (0, 0), (1, 0)
OA, D_SENSOR = (30, 16), (33, 16)


def far_hit(l2_max, lidar=False):
    r = reach_cells(l2_max)
    x = 32 + r + 3
    return (max(x, 45), 16) if not lidar else (55, 16)


def _assert_offsets_to(dump, cells, target, what):
    for x, y in cells:
        c, bit = cell_of(dump, x, y)
        assert c is not None and bit and c["valid"] and (x + int(c["obstacle"][0]), y + int(c["obstacle"][1])) == target, (what, x, y, c)


def check_dangling_raise_pf(F, l2_max=None):
    """frequency policy: the raise wave of OB's removal reads OA through the offsets of B's cells"""
    ob = (36, 16)
    pr = PFPair(F, 1, D_SENSOR, [OA, ob], l2_max)
    _assert_offsets_to(pr.pf.dm(0).dump(), [(32, 16), (32, 15), (32, 17)], OA, "cells of B that point into A")
    assert pr.delete(0, [pid(*DA)], "A") == 1
    through = [far_hit(l2_max)]
    gone = False
    for k in range(8):
        dm = pr.pf.dm(0)
        assert pid(*DA) not in dm.patch_ids().tolist() and is_obstacle(dm.dump(), *ob), k
        pops = dm.stats()["raise_pops"]
        pr.scan_from([D_SENSOR], through, f"beam over OB, scan {k}")          # (compares both maps)
        if not is_obstacle(pr.pf.dm(0).dump(), *ob):
            gone = True
            break
        assert pid(*DA) not in pr.pf.dm(0).patch_ids().tolist(), k           # nothing else brings A back
    assert gone and k >= 2 and pr.pf.dm(0).stats()["raise_pops"] > pops
    after = pr.pf.dm(0).dump()
    assert pid(*DA) in after                                                   # the non-const read of OA re-created A ...
    c, bit = cell_of(after, *OA)
    assert bit and not c["valid"] and c["sqdist"] == 0                         # ... with an empty cell whose mask bit is on
    pr.close()


def check_dangling_lower_tie(F, l2_max=None):
    """OA = (30, 16) and, by add_obstacles, its mirror image M = (36, 16) about the column x = 33 of B: every cell (33, y) in reach
    still points at OA and is offered the same squared distance by M -- the tie test of lower() reads OA, in the deleted patch.
    (32, y) stays nearer to OA, so the wave from M never touches a cell of A: only the obstacle read brings A back."""
    r = reach_cells(l2_max)
    other = (33 + 2 * r + 3, 16)                                              # a second obstacle of the first scan, out of reach of all this
    pr = PFPair(F, 1, D_SENSOR, [OA, other], l2_max)
    _assert_offsets_to(pr.pf.dm(0).dump(), [(33, 16), (33, 14), (33, 18), (32, 16)], OA, "cells of B that point into A")
    assert pr.delete(0, [pid(*DA)], "A") == 1
    dm = pr.pf.dm(0)
    ties = dm.stats()["tie_overwrites"]
    m = np.array([[OFF + 36, OFF + 16]], dtype=np.uint32)
    dm.add(int(m[0, 0]), int(m[0, 1])); dm.update()
    pr.ctx.add_obstacles(0, m)
    assert dm.stats()["tie_overwrites"] > ties and pid(*DA) in dm.patch_ids().tolist()
    c, bit = cell_of(dm.dump(), *OA)
    assert bit and not c["valid"]
    assert not any(cell_of(dm.dump(), 31, y)[1] for y in range(10, 23))        # the wave itself touched no cell of A
    pr.assert_maps("after the tie")
    # one more scan on top: the re-created patch is a live one
    pr.scan_from([D_SENSOR], [(28, 20), (40, 12)], "a scan into the re-created patch")
    pr.close()


class LidarPair:
    """A one-particle context configured as LidarOdometry2D configures its own (tests/_ray_checks.check_third_axis_lidar_odometry_
    context) and the oracle's LidarOdometry driven through update_maps_at: the same scans at the same poses, no scan match"""

    def __init__(self, F, pose, pts):
        self.F, self.o = F, O.LidarOdometry()
        assert self.o.update_maps_at(pts, pose, prune=False) == 0
        self.ctx = F.HipContext(F.default_cfg(particles=1, device=0, l2_max=1.0, occupancy_policy=1, ray_rule=1, dm_patch_capacity=8,
                                              occ_patch_capacity=8, queue_capacity=1 << 18))
        self.ctx.init(pts, pose)
        self.check("first scan")

    def update(self, pose, pts, what, prune=False):
        """-> patches the oracle's transient step deleted (prune; the device is not pruned here)"""
        n = self.o.update_maps_at(pts, pose, prune=prune)
        self.ctx.set_poses(np.asarray(pose)[None]); self.ctx.update_maps(pts)
        if not prune:
            self.check(what)
        return n

    def delete(self, ids, what):
        ids = [int(i) for i in ids]
        d = self.ctx.delete_patches(0, np.array(ids, dtype=np.uint64))
        n = 0
        for i in ids:
            self.o.occ().delete_patch(i)
            n += 1 if self.o.dm().delete_patch(i) else 0
        assert d == n, what
        self.check(what)
        return d

    def occ_values(self):
        return {p: np.ascontiguousarray(c).view(np.float32).reshape(-1) for p, (c, _) in self.o.occ().dump().items()}

    def check(self, what):
        F = self.F
        assert_maps_equal(self.ctx.download_map(0, F.MAP_DISTANCE), self.o.dm().dump(), DM_FIELDS, f"{what}: dm")
        got, ref = self.ctx.download_map(0, F.MAP_OCCUPANCY), self.o.occ().dump()
        assert sorted(got) == sorted(ref), (what, sorted(got), sorted(ref))
        for p in ref:
            assert np.array_equal(np.ascontiguousarray(got[p][0]).view(np.uint32).reshape(-1), np.ascontiguousarray(ref[p][0]).view(np.uint32).reshape(-1)), (what, p)
            assert np.array_equal(got[p][1], ref[p][1]), (what, p)
        assert self.ctx.patch_ids(0, F.MAP_DISTANCE).tolist() == sorted(self.o.dm().patch_ids().tolist()), what
        assert self.ctx.patch_ids(0, F.MAP_OCCUPANCY).tolist() == sorted(ref), what

    def close(self):
        self.ctx.close()


def check_dangling_raise_lidar(F):
    """the same under the LidarOdometry2D configuration: log-odds cells, beams of a metre or more start a metre before their hit,
    the distance map reaches 20 cells.  The beam over OB is 22 cells long and so starts on (35, 16), one cell before OB."""
    ob = (36, 16)
    pose, pts = beams(D_SENSOR, [OA, ob])
    lp = LidarPair(F, pose, pts)
    _assert_offsets_to(lp.o.dm().dump(), [(32, 16), (32, 12), (32, 20)], OA, "cells of B that point into A")
    assert lp.delete([pid(*DA)], "A deleted") == 1
    _, through = beams(D_SENSOR, [far_hit(1.0, lidar=True)])
    gone = False
    for k in range(8):
        assert pid(*DA) not in lp.o.dm().patch_ids().tolist() and is_obstacle(lp.o.dm().dump(), *ob), k
        lp.update(pose, through, f"beam over OB, scan {k}")
        if not is_obstacle(lp.o.dm().dump(), *ob):
            gone = True
            break
        assert pid(*DA) not in lp.o.dm().patch_ids().tolist(), k
    assert gone and k >= 1
    after = lp.o.dm().dump()
    c, bit = cell_of(after, *OA)
    assert pid(*DA) in after and bit and not c["valid"]
    lp.close()


def check_vacated_slot_reused(F, l2_max=None):
    """Every patch of the block scan's distance map in turn -- one of them holds the region's last slot, the others are refilled from
    it -- is deleted from both maps of a fresh upload; the next scan is taken four patches further up and allocates patches of both
    maps there, the first of them in the slot the deletion vacated.  A byte the deletion left in any plane of that slot is a cell or
    a mask bit the oracle's new patch does not have."""
    pf = block_filter(1, l2_max)
    ids = sorted(set(pf.dm(0).patch_ids().tolist()) | {pid(3, 0)})
    ctx = F.HipContext(F.default_cfg(particles=1, **_cfg(l2_max)))
    sensor, hits = (40, 140), [(44, 150), (20, 133), (70, 138)]
    pose, pts = beams(sensor, hits)
    for k, i in enumerate(ids):
        if k:
            pf = block_filter(1, l2_max)
        upload_from(F, ctx, pf)
        ctx.set_poses(pose[None])
        d = ctx.delete_patches(0, np.array([i], dtype=np.uint64))
        assert d == oracle_delete(pf, 0, [i])
        n0 = len(pf.dm(0).patch_ids()), len(pf.occ(0).patch_ids())
        pf.set_poses(pose[None]); pf.stage_set_scan(pts); pf.stage_update_maps()
        ctx.update_maps(pts)
        assert len(pf.dm(0).patch_ids()) > n0[0] and len(pf.occ(0).patch_ids()) > n0[1]
        what = f"after deleting {(i // UC - OFFP, i % UC - OFFP)} and a scan elsewhere"
        assert_maps_equal(ctx.download_map(0, F.MAP_OCCUPANCY), pf.occ(0).dump(), OCC_FIELDS, f"{what}: occ")
        assert_maps_equal(ctx.download_map(0, F.MAP_DISTANCE), pf.dm(0).dump(), DM_FIELDS, f"{what}: dm")
    ctx.close()


def _block_pair(F, l2_max, **cfg):
    """three particles after the block scan and a second scan from a cell of each one's own"""
    pr = PFPair(F, 3, A_SENSOR, A_HITS, l2_max, **cfg)
    pr.scan_from(A_SENSORS3, A_HITS, "second scan")
    assert len(set(pr.pf.map_checksums(0).tolist())) == 3
    return pr


def check_clone_after_a_deletion(F, l2_max=None):
    """delete on particle 1, resample [1, 1, 0] (the compacted region is cloned twice), update: all maps equal"""
    pr = _block_pair(F, l2_max)
    b = block_ids()
    assert pr.delete(1, [b[1], b[5], b[0]], "p1") == 3
    pr.resample([1, 1, 0])
    pr.assert_maps("clones of the compacted region")
    pr.scan_from([(42, 29), (40, 32), (39, 30)], A_HITS, "update of the clones")
    pr.close()


def check_export_after_a_deletion(F, l2_max=None):
    """delete on particle 1, export it, import it into a context whose window sits elsewhere, update there"""
    pr = _block_pair(F, l2_max, window_patches=16)
    b = block_ids()
    assert pr.delete(1, [b[4], b[0]], "p1") == 2
    blob = W.export_blob(F, pr.ctx, 1)
    h = blob.header()
    assert h[0] == len(pr.pf.dm(1).dump()) and h[1] == len(pr.pf.occ(1).dump())
    # the receiver starts three patches up and two to the left: another window origin
    other = PFPair(F, 2, (A_SENSOR[0] - 64, A_SENSOR[1] + 96), [(A_SENSOR[0] - 60, A_SENSOR[1] + 100)], l2_max, window_patches=16)
    wa, wb = W.window_of(F, pr.ctx), W.window_of(F, other.ctx)
    assert np.any(wa[:2] != wb[:2]), (wa, wb)
    other.ctx.import_particle(0, blob.ptr, blob.n)
    assert_maps_equal(other.ctx.download_map(0, F.MAP_DISTANCE), pr.pf.dm(1).dump(), DM_FIELDS, "imported dm")
    assert_maps_equal(other.ctx.download_map(0, F.MAP_OCCUPANCY), pr.pf.occ(1).dump(), OCC_FIELDS, "imported occ")
    other.assert_maps("the receiver's own particle", [1])
    # one update there: slot 0 carries on as the sender's particle 1, slot 1 as the receiver's own
    _, pts = beams((41, 31), A_HITS)
    poses = np.stack([RC.sensor(41, 31), RC.sensor(A_SENSOR[0] - 63, A_SENSOR[1] + 97)])
    pr.pf.set_poses(np.stack([RC.sensor(0, 0), poses[0], RC.sensor(0, 0)]))
    other.pf.set_poses(poses); other.pf.stage_set_scan(pts); other.pf.stage_update_maps()
    pr.pf.stage_set_scan(pts)
    # (only the sender's oracle particle 1 matters: the other two integrate the scan somewhere and are not looked at again)
    pr.pf.stage_update_maps()
    other.ctx.set_poses(poses); other.ctx.update_maps(pts)
    assert_maps_equal(other.ctx.download_map(0, F.MAP_DISTANCE), pr.pf.dm(1).dump(), DM_FIELDS, "imported dm after an update")
    assert_maps_equal(other.ctx.download_map(0, F.MAP_OCCUPANCY), pr.pf.occ(1).dump(), OCC_FIELDS, "imported occ after an update")
    other.assert_maps("the receiver's own particle after an update", [1])
    pr.close(); other.close()


def check_deletion_waits_for_the_groups(F, groups, l2_max=None):
    """lama_hip_pf_match_and_map queues the map update of every group; delete_patches, called at once, must find the update done:
    the result is the oracle's update followed by its deletion.  The deleted patches are ones the update writes to."""
    pr = _block_pair(F, l2_max)
    _, pts = beams(A_SENSOR, A_HITS)
    start = np.stack([RC.sensor(*s) for s in A_SENSORS3])
    got, _, _ = pr.ctx.match_and_map(pts, start)
    b = block_ids()
    d = pr.ctx.delete_patches(1, np.array([b[1], b[3]], dtype=np.uint64))       # the sensor's patch and one a beam ends in
    assert pr.ctx.step_groups() == groups
    before = [pr.pf.occ(1).dump()[i][0].tobytes() for i in (b[1], b[3])]
    pr.pf.set_poses(got); pr.pf.stage_set_scan(pts); pr.pf.stage_update_maps()
    assert all(x != pr.pf.occ(1).dump()[i][0].tobytes() for x, i in zip(before, (b[1], b[3])))      # the queued update writes to both
    assert d == oracle_delete(pr.pf, 1, [b[1], b[3]]) == 2
    pr.assert_maps("update, then delete")
    pr.scan_from(A_SENSORS3, A_HITS, "the next update")
    pr.close()


def check_deletion_after_a_window_move(F, l2_max=None):
    """the driver of tests/_window_checks.py, one particle, a window of 16 patches: drive along -x until the window has moved,
    delete two patches at the edge the window moved towards, update"""
    pr = W.Pair(F, 1, W._w(16, l2_max), W.START[0], W.START[1], np.pi)
    w0 = W.window_of(F, pr.ctx)
    for t in (4.0, 8.0, 12.0):
        pr.drive_to(W.START[0] - t, W.START[1], np.pi, f"-x t = {t}")
        w1 = W.window_of(F, pr.ctx)
        if np.any(w1[:2] != w0[:2]):
            break
    assert np.any(w1[:2] != w0[:2]) and w1[2] == 16 and pr.ctx.counters()["window_shifts"] >= 1, (w0, w1)
    ids = pr.pf.dm(0).patch_ids().tolist()
    assert sorted(ids) == pr.ctx.patch_ids(0, pr.F.MAP_DISTANCE).tolist()
    lowest = min(i // UC for i in ids)
    edge = sorted(i for i in ids if i // UC == lowest)
    pick = [edge[0], edge[-1]] if len(edge) > 1 else [edge[0], sorted(ids)[1]]
    assert len(set(pick)) == 2 and all(i // UC - w1[0] < 6 for i in pick)
    n = len(ids)
    d = pr.ctx.delete_patches(0, np.array(pick, dtype=np.uint64))
    assert d == oracle_delete(pr.pf, 0, pick) == 2
    pr.assert_maps("deleted after the move")
    assert pr.ctx.patch_ids(0, pr.F.MAP_DISTANCE).tolist() == sorted(pr.pf.dm(0).patch_ids().tolist()) and len(pr.pf.dm(0).patch_ids()) == n - 2
    x, y, yaw = pr.at
    pr.drive_to(x - 0.4, y + 0.1, yaw, "update after the deletion")
    assert pr.ctx.patch_ids(0, pr.F.MAP_OCCUPANCY).tolist() == sorted(pr.pf.occ(0).patch_ids().tolist())
    pr.close()


# ---- log-odds clamps and crossings
L_SENSOR = (40, 40)
L_HITS = [(52, 40), (40, 49), (31, 33), (47, 47), (40, 28), (29, 40)]


def check_log_odds_clamps_and_crossings(F):
    """The same short scan eight times: the hit cells climb to clamp_max, the cells before them sink to clamp_min (asserted from
    the oracle's cells), every cast compared.  Then beams from the same pose that end two cells beyond the former hits: the former
    hit cells are missed until they cross zero downwards and the distance map loses their obstacles, the new hit cells cross it
    upwards.  Last, one update 4 m away with the transient step: the old patches go, on the device by the list of that step.
    (What this does NOT tell apart is the sum taken in float instead of double: the four parameters are float-rounded, the double
    sum of two floats of this range is exact and rounding is monotone, so `fminf(lp + hit, max)` is the same float for every cell
    value -- checked over the 400 000 values reachable from 0 and two million random ones.  The order of the visits is what matters:
    clamping does not commute, and every cast is compared.)"""
    miss, hit, cmin, cmax, _ = O.pocc_params()
    pose, pts = beams(L_SENSOR, L_HITS)
    lp = LidarPair(F, pose, pts)
    for k in range(7):
        lp.update(pose, pts, f"cast {k + 2} of 8")
    v = np.concatenate(list(lp.occ_values().values()))
    assert (v == np.float32(cmax)).sum() == len(L_HITS) and (v == np.float32(cmin)).sum() >= 40, ((v == np.float32(cmax)).sum(), (v == np.float32(cmin)).sum())
    assert all(is_obstacle(lp.o.dm().dump(), *h) for h in L_HITS)
    beyond = []
    for hx, hy in L_HITS:
        dx, dy = hx - L_SENSOR[0], hy - L_SENSOR[1]
        s = 2.0 / max(abs(dx), abs(dy))
        beyond.append((hx + int(round(dx * s)), hy + int(round(dy * s))))
    _, pts2 = beams(L_SENSOR, beyond)
    pops = lp.o.dm().stats()["raise_pops"]
    for k in range(12):
        lp.update(pose, pts2, f"beams two cells beyond, cast {k + 1}")
        if not any(is_obstacle(lp.o.dm().dump(), *h) for h in L_HITS):
            break
    dump = lp.o.dm().dump()
    assert not any(is_obstacle(dump, *h) for h in L_HITS) and all(is_obstacle(dump, *h) for h in beyond) and k >= 2
    assert lp.o.dm().stats()["raise_pops"] > pops
    # 4 m away, with the transient step: the list is what that step removes from the distance map the update left
    old = set(lp.o.dm().patch_ids().tolist())
    far = RC.sensor(L_SENSOR[0] + 80, L_SENSOR[1])
    deleted = lp.update(far, pts, "4 m away", prune=True)
    have = lp.ctx.patch_ids(0, F.MAP_DISTANCE).tolist()
    left = lp.o.dm().patch_ids().tolist()
    to_remove = [i for i in have if i not in left]
    assert deleted > 0 and deleted == lp.o.deleted_last() == len(to_remove) and set(to_remove) <= old
    assert lp.ctx.delete_patches(0, np.array(to_remove, dtype=np.uint64)) == deleted
    lp.check("after the transient step")
    lp.update(far, pts2, "one more cast there")
    lp.close()
