"""Checks of the code that only permutes window-directory entries -- k_shift_window (the window follows the robot and grows),
the directory row range of k_clone_particles (a resample right after a move), k_export_particles and the translating branch of
k_import_particles (particles shipped between contexts whose windows sit elsewhere and have other sides) -- shared by
tests/test_window_gpu.py and the lane-simulator tests (tests/test_window_sim.py).

The reference is the CPU oracle's particle filter (O.PF), whose maps have no extent.  Everything is compared bit for bit
(assert_maps_equal on OCC_FIELDS / DM_FIELDS, for EVERY particle of a context, after EVERY update); poses that travel with a
particle with array_equal.  The two exceptions are the final scan match of check_drive: poses within POSE_TOL (the value of
test_gpu_parity.py: libm against OCML trig, another summation order), iteration counts equal.

Workload: a hall of 0.4 m pillars about every metre with clear streets along the eight drive directions, a 180-beam scanner whose
returns beyond 3 m are dropped.  One update can then touch pose +- (3 m + guard patches): 8 - 9 patches of 1.6 m in the default
library (guard radius 1 patch), 16 - 17 in the wide one (l2_max = 7 m: 5 patches), so windows of 16 / 24 patches leave the same
slack of 7 patches and one trajectory serves both.  Which branch a case took is read from the context's counters and from the
header of an exported blob (window origin in int32 words 2 and 3 at byte 32, side in word 5; layout above k_export_particles):
a case that stops exercising its branch fails.
"""
import itertools
import math

import numpy as np
import pytest

import _oracle as O
from _cmp import DM_FIELDS, OCC_FIELDS, assert_maps_equal
from _worlds import segment_world_scan

POSE_TOL = 1e-8            # = test_gpu_parity.POSE_TOL
BEAMS, MAX_RANGE = 180, 3.0
PATCH_M = 1.6              # 32 cells of 0.05 m
START = (0.37, 0.21)
WIDE_L2 = 7.0              # 140 cells: liblama_hip_wide.so, guard radius 5 patches
DIRECTIONS = {"+x": (1, 0), "-x": (-1, 0), "+y": (0, 1), "-y": (0, -1),
              "+x+y": (1, 1), "+x-y": (1, -1), "-x+y": (-1, 1), "-x-y": (-1, -1)}
# a particle's constant offset from the true pose: less than half a cell, so every particle maps a consistent world of its own
# (the maps differ in the cells the rasterisation flips) and a copy that carries on in another slot stays consistent, too
OFFSETS = ((0.0, 0.0), (0.021, -0.016), (-0.018, 0.023))

_hall = None


def hall():
    """Wall segments (S, 4): square pillars of 0.4 m on a jittered 1 m lattice over [-26, 26]^2, none with its centre within
    0.45 m of the four lines through START along which the checks drive: 70 - 160 of the 180 beams return from anywhere on them."""
    global _hall
    if _hall is None:
        rng = np.random.default_rng(2024)
        segs = []
        for i in range(-26, 27):
            for j in range(-26, 27):
                cx, cy = 1.0 * i + rng.uniform(-0.2, 0.2), 1.0 * j + rng.uniform(-0.2, 0.2)
                u, v = cx - START[0], cy - START[1]
                if min(abs(u), abs(v), abs(u - v) / math.sqrt(2.0), abs(u + v) / math.sqrt(2.0)) < 0.45:
                    continue
                xa, xb, ya, yb = cx - 0.2, cx + 0.2, cy - 0.2, cy + 0.2
                segs += [(xa, ya, xb, ya), (xb, ya, xb, yb), (xb, yb, xa, yb), (xa, yb, xa, ya)]
        _hall = np.array(segs)
    return _hall


def scan_at(x, y, yaw):
    pts = segment_world_scan(hall(), x, y, yaw, beams=BEAMS, max_range=MAX_RANGE)
    assert 40 <= len(pts) <= BEAMS
    return pts


class Blob:
    """Memory for a particle blob that the library can address: device memory for the device libraries, host memory for the
    lane simulator (whose hipMalloc is malloc)."""

    def __init__(self, F, nbytes):
        self.n = int(nbytes)
        self._t = None
        if F.is_device_library(F.HIP_LIB):
            import torch
            self._t = torch.zeros(self.n, dtype=torch.uint8, device="cuda")
            self.ptr = self._t.data_ptr()
        else:
            self._a = np.zeros(self.n, dtype=np.uint8)
            self.ptr = self._a.ctypes.data

    def host(self, n=None):
        n = self.n if n is None else n
        return self._t[:n].cpu().numpy().copy() if self._t is not None else self._a[:n].copy()

    def store(self, arr):
        assert arr.dtype == np.uint8 and len(arr) == self.n
        if self._t is not None:
            import torch
            self._t.copy_(torch.from_numpy(arr))
            torch.cuda.synchronize()
        else:
            self._a[:] = arr

    def header(self):
        """the eight int32 header words: dm patches, occ patches, window origin x / y (patches), visited bound, window side, ..."""
        return self.host(64)[32:64].view(np.int32).copy()


def export_blob(F, ctx, particle):
    n = ctx.export_bytes(particle)
    blob = Blob(F, n)
    assert ctx.export_particle(particle, blob.ptr, n) == n
    return blob


def window_of(F, ctx):
    """(origin x, origin y, side) of the context's window in patches, from the header of an exported blob"""
    h = export_blob(F, ctx, 0).header()
    assert h[5] == ctx.counters()["window_patches"]
    return np.array([h[2], h[3], h[5]], dtype=np.int64)


class Pair:
    """A device context and the oracle's particle filter, fed the same scans at the same poses"""

    def __init__(self, F, P, cfg, x, y, yaw, scan=None, upload=False):
        """upload: the context does not integrate the first scan but is handed the oracle's first map (particle 0, the others are
        then resampled from it) -- its mapped box is the exact patch extent of that map, without the guard rows of an update"""
        self.F, self.P = F, P
        opts = dict(l2_max=cfg["l2_max"]) if "l2_max" in cfg else {}
        pose0 = O.se2(x, y, yaw)
        scan = scan_at(x, y, yaw) if scan is None else scan
        self.pf = O.PF(O.default_options(particles=P, seed=3, **opts))
        self.pf.set_prior(pose0)
        assert self.pf.update(scan, pose0)
        self.ctx = F.HipContext(F.default_cfg(particles=P, **cfg))
        if upload:
            self.ctx.upload_map(0, F.MAP_DISTANCE, self.pf.dm(0).dump())
            self.ctx.upload_map(0, F.MAP_OCCUPANCY, self.pf.occ(0).dump())
            self.ctx.set_poses(self.pf.poses())
        else:
            self.ctx.init(scan, pose0)
        self.at = (x, y, yaw)
        self.updates = 0

    def close(self):
        self.ctx.close()

    def poses_at(self, x, y, yaw):
        return np.stack([O.se2(x + OFFSETS[i][0], y + OFFSETS[i][1], yaw) for i in range(self.P)])

    def update(self, poses, scan, what=""):
        """one map update of every particle, then every particle's maps against the oracle's"""
        self.pf.set_poses(poses); self.pf.stage_set_scan(scan); self.pf.stage_update_maps()
        self.ctx.set_poses(poses); self.ctx.update_maps(scan)
        self.updates += 1
        self.assert_maps(what)

    def drive_to(self, x, y, yaw, what=""):
        self.at = (x, y, yaw)
        self.update(self.poses_at(x, y, yaw), scan_at(x, y, yaw), what)

    def resample(self, idx):
        idx = np.asarray(idx, dtype=np.int32)
        assert len(set(idx.tolist())) < self.P and max(np.bincount(idx)) >= 2      # somebody dies, somebody is copied
        self.pf.stage_resample_with(idx)
        self.ctx.resample(idx)
        assert np.array_equal(self.ctx.get_poses(), self.pf.poses())

    def assert_maps(self, what, slots=None):
        F = self.F
        for i in (range(self.P) if slots is None else slots):
            assert_maps_equal(self.ctx.download_map(i, F.MAP_OCCUPANCY), self.pf.occ(i).dump(), OCC_FIELDS, f"{what}: occ p{i}")
            assert_maps_equal(self.ctx.download_map(i, F.MAP_DISTANCE), self.pf.dm(i).dump(), DM_FIELDS, f"{what}: dm p{i}")

    def checksums(self):
        F = self.F
        return np.stack([self.ctx.map_checksums(F.MAP_DISTANCE), self.ctx.map_checksums(F.MAP_OCCUPANCY)])


def _w(window, l2_max=None):
    """configuration of a context / of the oracle's filter: the window side and, where given, the distance map's reach"""
    return dict(window_patches=window) if l2_max is None else dict(window_patches=window, l2_max=l2_max)


def _plans(P):
    """index vectors that kill at least one particle and copy another, a different pattern every time"""
    if P == 2:
        return itertools.cycle([[1, 1], [0, 0]])
    return itertools.cycle([[0, 0, 2], [2, 1, 1], [1, 0, 1], [2, 2, 2]])


def _in_pattern(delta, d):
    """every component of an origin move is zero or has the sign of d (a zero component of d: no move on that axis)"""
    return all(int(np.sign(delta[k])) in (0, d[k]) for k in (0, 1))


def check_drive(F, direction, P=3, window=16, l2_max=None, out=(2.0, 4.0, 6.0, 8.0), back=(6.0, 4.0, 2.0, 0.0, -2.0, -4.0, -6.0, -8.0, -10.0)):
    """The window follows the robot out along `direction` (leg 1: shifts, no growth), then back past the start until the mapped
    area outgrows it (leg 2: shifts the other way, then growth combined with a shift).  Maps of every particle bit-equal to the
    oracle's after every update; a resample that kills one particle and copies another follows every update that moved the
    window and the end of each leg, and the update after it is checked like all others (the clone's directory rows); at the end
    a scan match against the oracle's.  `out` / `back`: the distances from START (metres along each axis of the direction) at
    which a scan is integrated.  The window can only shift back towards higher coordinates while the mapped area still fits its
    side, which is between 0.6 and 3.8 m past the start: `back` needs a stop there.  -> the context's counters."""
    d = DIRECTIONS[direction]
    heading = math.atan2(d[1], d[0])
    pr = Pair(F, P, _w(window, l2_max), START[0], START[1], heading)
    ctx = pr.ctx
    pr.assert_maps("first scan")
    plans = _plans(P)
    w0 = window_of(F, ctx)
    c0 = ctx.counters()
    assert w0[2] == window and c0["window_growths"] == 0, (w0, c0)

    def leg(ts, yaw, sign, name):
        """-> [(origin move, grew)] of the updates that moved the window"""
        moves = []
        w = window_of(F, ctx)
        for k, t in enumerate(ts):
            c = ctx.counters()
            pr.drive_to(START[0] + t * d[0], START[1] + t * d[1], yaw + 0.05 * math.sin(1.3 * k), f"{direction} {name} t = {t}")
            c2 = ctx.counters()
            if c2["window_shifts"] != c["window_shifts"]:
                w2 = window_of(F, ctx)
                delta = w2[:2] - w[:2]
                grew = c2["window_growths"] != c["window_growths"]      # (a window that grows towards higher coordinates keeps its origin)
                assert _in_pattern(delta, (sign * d[0], sign * d[1])) and (grew or np.any(delta != 0)), (direction, name, t, w, w2)
                moves.append((delta, grew))
                w = w2
                pr.resample(next(plans))                 # a clone directly after the move: the next update shows what it copied
            else:
                assert np.array_equal(window_of(F, ctx), w)
        pr.resample(next(plans))
        return moves

    # leg 1: out, until the union of the boxes no longer fits where the first scan placed the window (but still fits its side)
    m1 = leg(out, heading, +1, "leg 1")
    w1, c1 = window_of(F, ctx), ctx.counters()
    assert c1["window_shifts"] > c0["window_shifts"] and c1["window_growths"] == 0 and w1[2] == window, (c0, c1)
    assert m1 and not any(g for _, g in m1)
    assert tuple(np.sign(w1[:2] - w0[:2])) == d, (direction, w0, w1)        # dx, dy of k_shift_window: the signs of d, zero included
    # leg 2: turn round, past the start, until the union is wider than the window
    m2 = leg(back, heading + math.pi, -1, "leg 2")
    w2, c2 = window_of(F, ctx), ctx.counters()
    assert c2["window_growths"] > 0 and c2["window_patches"] > window and w2[2] == c2["window_patches"], c2
    assert tuple(np.sign(w2[:2] - w1[:2])) == (-d[0], -d[1]), (direction, w1, w2)
    assert any(not g and np.any(dl != 0) for dl, g in m2), m2             # a plain shift the other way came first
    # A grown window extends towards higher coordinates, so its origin moves only where the way back leads to lower ones: growth
    # combined with a shift (dx or dy < 0, the other possibly 0) for every direction with a positive component, growth in place
    # (dx = dy = 0, Ws != Wd) for -x, -y and -x-y
    moved = [bool(np.any(dl != 0)) for dl, g in m2 if g]
    assert moved and all(moved) == (max(d) > 0), (direction, m2)
    # the update after the last resample
    x, y, yaw = pr.at
    pr.drive_to(x - 0.3 * d[0], y - 0.3 * d[1], yaw + 0.03, f"{direction} after the last resample")
    assert pr.updates <= 40
    # scan matching on the moved and grown window sees the map
    x, y, yaw = pr.at
    scan = scan_at(x, y, yaw)
    start = np.stack([O.se2(x + OFFSETS[i][0] + 0.04, y + OFFSETS[i][1] - 0.03, yaw + 0.01) for i in range(P)])
    pr.pf.set_poses(start); pr.pf.set_weights(w=np.zeros(P), ws=np.zeros(P)); pr.pf.stage_set_scan(scan); pr.pf.stage_scan_match()
    ctx.set_poses(start)
    g_poses, _, g_it = ctx.scan_match(scan)
    o_it = np.array([pr.pf.counters(i)["iterations"] for i in range(P)])
    assert np.array_equal(g_it, o_it) and o_it.min() >= 1, (direction, g_it, o_it)
    assert np.abs(g_poses - pr.pf.poses()).max() <= POSE_TOL, (direction, np.abs(g_poses - pr.pf.poses()).max())
    pr.close()
    return c2


PATCH_ID_STRIDE = 2642244      # patch id = x * stride + y (the reference's patch index, lama_hip_pf_upload_map)


def check_clone_with_a_tight_mapped_box(F, direction, P=2, window=16, stops=(10.0,), l2_max=None):
    """The rows a clone copies are those of the mapped box.  After an update the box has a guard row without patches at either end;
    an uploaded map's box is the exact extent of its patches, so its first and last row both hold some.  A context that starts
    from an uploaded map is resampled at once (the copies must hold every row), then continues 10 m further along +y or -y -- far
    enough that the update's own guard rows stay inside the box, which so remains tight at the end left behind, and that the
    window must move -- with a resample after that update.  Maps of every particle bit-equal to the oracle's after every update."""
    d = DIRECTIONS[direction]
    assert d[0] == 0
    heading = math.atan2(d[1], d[0])
    pr = Pair(F, P, _w(window, l2_max), START[0], START[1], heading, upload=True)
    ctx = pr.ctx
    rows = [pid % PATCH_ID_STRIDE for pid in pr.pf.dm(0).dump()]

    def mapped_rows():
        h = export_blob(F, ctx, 0).header()
        return int(h[3]) + (int(h[7]) & 0xFFFF), int(h[3]) + ((int(h[7]) >> 16) & 0xFFFF)
    assert mapped_rows() == (min(rows), max(rows))                       # tight at both ends: no guard rows
    plans = _plans(P)
    pr.resample([0] * P)
    pr.assert_maps(f"{direction}: copies of the uploaded map")
    c0 = ctx.counters()
    moved = 0
    for t in stops:
        c = ctx.counters()
        pr.drive_to(START[0], START[1] + t * d[1], heading, f"{direction} t = {t}")
        if ctx.counters()["window_shifts"] != c["window_shifts"]:
            moved += 1
            pr.resample(next(plans))
    c1 = ctx.counters()
    assert moved and c1["window_growths"] == c0["window_growths"], (c0, c1)
    lo, hi = mapped_rows()
    assert (lo == min(rows) and hi > max(rows)) if d[1] > 0 else (hi == max(rows) and lo < min(rows)), (lo, hi, min(rows), max(rows))
    pr.resample(next(plans))
    x, y, yaw = pr.at
    pr.drive_to(x, y - 0.3 * d[1], yaw + 0.03, f"{direction} after the last resample")
    pr.close()


def grow_by_driving(F, pr, window):
    """drive the pair along -x until its window has grown (leg 2 of check_drive, in strides of 4 m)"""
    for k in range(1, 5):
        pr.drive_to(START[0] - 4.0 * k, START[1], math.pi, f"sender t = {-4 * k}")
    c = pr.ctx.counters()
    assert c["window_growths"] >= 1 and c["window_patches"] > window, c


def check_ship(F, sender_cfg, receiver_cfg, offset, slots=(0,), receiver_particles=2, grow_sender=False, receiver_maps_more=False, l2_max=None):
    """Particle 1 of context a (two particles, window as sender_cfg) is exported and imported into `slots` of context b, which was
    initialised `offset` patches away.  The receiving slots must equal the oracle particle the blob came from (maps bit-equal, pose
    array_equal), b's other slots keep their checksums (and stay equal to b's own oracle), and one more update of b -- the imported
    particles near where they came from, the others where they were -- stays bit-equal: the imported particle is live and its new
    patches are allocated at the right place.  -> the facts by which a caller asserts the branch the import took:
      wd            b's window origin minus the blob's at the import (wdx, wdy of k_import_particles)
      Ws, W0, W     the blob's window side, b's side before and after the import
      shifts, growths   how much the import raised b's counters
      blob_counts, old_counts   (dm, occ) patches the blob brings / the (first) receiving slot held before"""
    j = 1
    if l2_max is not None:
        sender_cfg, receiver_cfg = dict(sender_cfg, l2_max=l2_max), dict(receiver_cfg, l2_max=l2_max)
    a = Pair(F, 2, sender_cfg, START[0], START[1], 0.0)
    if grow_sender:
        grow_by_driving(F, a, sender_cfg["window_patches"])
    else:
        a.drive_to(START[0] + 0.7, START[1] - 0.4, 0.1, "sender scan 1")
    bx, by = START[0] + offset[0] * PATCH_M, START[1] + offset[1] * PATCH_M
    b = Pair(F, receiver_particles, receiver_cfg, bx, by, 0.4)
    if receiver_maps_more:
        for k in range(1, 4):
            b.drive_to(bx + 2.0 * k * (1 if offset[0] >= 0 else -1), by, 0.4, f"receiver scan {k}")
    wa, wb = window_of(F, a.ctx), window_of(F, b.ctx)
    if not grow_sender and not receiver_maps_more and sender_cfg["window_patches"] == receiver_cfg["window_patches"]:
        # the first scan centres the window on its box: origins `offset` patches apart (the two scans' reaches may round differently)
        assert np.array_equal(np.sign(wb[:2] - wa[:2]), np.sign(offset)) and np.abs(wb[:2] - wa[:2] - offset).max() <= 1, (wa, wb, offset)
    blob = export_blob(F, a.ctx, j)
    h = blob.header()
    assert np.array_equal([h[2], h[3], h[5]], wa)
    assert h[0] == len(a.pf.dm(j).dump()) and h[1] == len(a.pf.occ(j).dump())
    old_counts = (len(b.ctx.download_map(slots[0], F.MAP_DISTANCE)), len(b.ctx.download_map(slots[0], F.MAP_OCCUPANCY)))
    others = [s for s in range(b.P) if s not in slots]
    assert others
    before, cb = b.checksums(), b.ctx.counters()
    if len(slots) == 1:
        b.ctx.import_particle(slots[0], blob.ptr, blob.n)
    else:                                                      # one blob into several slots, one launch
        b.ctx.import_particles(list(slots), [blob.ptr] * len(slots), [blob.n] * len(slots))
    after, ca, wb2 = b.checksums(), b.ctx.counters(), window_of(F, b.ctx)
    facts = dict(wd=tuple(int(v) for v in wb2[:2] - wa[:2]), Ws=int(wa[2]), W0=int(wb[2]), W=int(wb2[2]),
                 shifts=ca["window_shifts"] - cb["window_shifts"], growths=ca["window_growths"] - cb["window_growths"],
                 blob_counts=(int(h[0]), int(h[1])), old_counts=old_counts)
    assert np.array_equal(after[:, others], before[:, others]), (facts, "the other slots changed")
    b.assert_maps("other slots after the import", others)
    a.pf.stage_resample_with(np.array([j, j], dtype=np.int32))   # oracle particle k of a's filter is what slot slots[k] received
    pose_j = a.pf.poses()[0]
    for k, s in enumerate(slots):
        assert np.array_equal(b.ctx.get_poses()[s], pose_j), (facts, s)
        assert_maps_equal(b.ctx.download_map(s, F.MAP_OCCUPANCY), a.pf.occ(k).dump(), OCC_FIELDS, f"{facts}: imported occ, slot {s}")
        assert_maps_equal(b.ctx.download_map(s, F.MAP_DISTANCE), a.pf.dm(k).dump(), DM_FIELDS, f"{facts}: imported dm, slot {s}")
    # one more update of b: a scan taken next to where the sender was, integrated by every slot at its own pose
    x, y, yaw = a.at
    x, y = x + 0.3, y + 0.2
    scan = scan_at(x, y, yaw)
    poses = b.poses_at(b.at[0] + 0.1, b.at[1] - 0.1, b.at[2])
    for k, s in enumerate(slots):
        poses[s] = O.se2(x + 0.05 * k, y - 0.04 * k, yaw)
    apos = np.stack([poses[slots[k % len(slots)]] for k in range(2)])
    a.pf.set_poses(apos); a.pf.stage_set_scan(scan); a.pf.stage_update_maps()
    b.pf.set_poses(poses); b.pf.stage_set_scan(scan); b.pf.stage_update_maps()
    b.ctx.set_poses(poses); b.ctx.update_maps(scan)
    b.assert_maps(f"{facts}: other slots after the next update", others)
    for k, s in enumerate(slots):
        assert_maps_equal(b.ctx.download_map(s, F.MAP_OCCUPANCY), a.pf.occ(k).dump(), OCC_FIELDS, f"{facts}: occ after the next update, slot {s}")
        assert_maps_equal(b.ctx.download_map(s, F.MAP_DISTANCE), a.pf.dm(k).dump(), DM_FIELDS, f"{facts}: dm after the next update, slot {s}")
    a.close(); b.close()
    return facts




def _sign(v):
    return (v > 0) - (v < 0)


# name -> (arguments of check_ship, what the facts must show)
SHIP_CASES = {
    # equal sides, the receiver's origin on every side of the sender's
    "offset ++": (dict(sender_cfg=_w(16), receiver_cfg=_w(16), offset=(5, 4)), lambda f: (_sign(f["wd"][0]), _sign(f["wd"][1])) == (1, 1) and f["Ws"] == f["W"]),
    "offset +-": (dict(sender_cfg=_w(16), receiver_cfg=_w(16), offset=(5, -4)), lambda f: (_sign(f["wd"][0]), _sign(f["wd"][1])) == (1, -1) and f["Ws"] == f["W"]),
    "offset -+": (dict(sender_cfg=_w(16), receiver_cfg=_w(16), offset=(-5, 4)), lambda f: (_sign(f["wd"][0]), _sign(f["wd"][1])) == (-1, 1) and f["Ws"] == f["W"]),
    "offset --": (dict(sender_cfg=_w(16), receiver_cfg=_w(16), offset=(-5, -4)), lambda f: (_sign(f["wd"][0]), _sign(f["wd"][1])) == (-1, -1) and f["Ws"] == f["W"]),
    # the sender's window has grown beyond the receiver's, and so has its map: the receiver must grow to hold it
    "grown sender": (dict(sender_cfg=_w(16), receiver_cfg=_w(16), offset=(3, -2), grow_sender=True),
                     lambda f: f["Ws"] > f["W0"] and f["growths"] >= 1 and f["W"] > f["W0"] and f["wd"] != (0, 0)),
    # sides that differ while the map fits: the translating branch with Ws > W and with Ws < W, nothing moves or grows (a first scan
    # centres its window, so the origins differ by the offset -+ half the difference of the sides)
    "larger sender": (dict(sender_cfg=_w(24), receiver_cfg=_w(16), offset=(-3, 2)),
                      lambda f: f["Ws"] == 24 and f["W"] == 16 and f["shifts"] == 0 and f["wd"][0] > 0 and f["wd"][1] > 0),
    "larger receiver": (dict(sender_cfg=_w(16), receiver_cfg=_w(24), offset=(-1, 6)),
                        lambda f: f["Ws"] == 16 and f["W"] == 24 and f["shifts"] == 0 and f["wd"][0] < 0 and f["wd"][1] > 0),
    # one blob into two slots of one batched call, for which the receiver's window must move
    "two slots, window moves": (dict(sender_cfg=_w(16), receiver_cfg=_w(16), offset=(-5, 4), slots=(0, 2), receiver_particles=3),
                                lambda f: f["shifts"] >= 1 and f["growths"] == 0 and f["wd"][0] < 0 and f["wd"][1] > 0),
    # the receiving slot held more patches of both kinds than the blob brings: the surplus slots are zeroed, the next update re-uses them
    "over a larger map": (dict(sender_cfg=_w(16), receiver_cfg=_w(24), offset=(2, -1), receiver_maps_more=True),
                          lambda f: f["old_counts"][0] > f["blob_counts"][0] and f["old_counts"][1] > f["blob_counts"][1]),
    # the wide library: guard radius 5 patches, so larger boxes and mapped-area words in the header
    "wide, larger receiver": (dict(sender_cfg=_w(24, WIDE_L2), receiver_cfg=_w(32, WIDE_L2), offset=(-2, 6)),
                              lambda f: f["Ws"] == 24 and f["W"] == 32 and f["shifts"] == 0 and f["wd"][0] < 0 and f["wd"][1] > 0),
}


def run_ship_case(F, name, l2_max=None):
    kw, holds = SHIP_CASES[name]
    facts = check_ship(F, l2_max=l2_max, **kw)
    assert holds(facts), (name, facts)       # the case took the branch it names
    return facts


def check_import_too_far(F, l2_max=None):
    """A particle from 3 km away: the union of the two mapped areas is wider than the largest window (1016 patches = 1.6 km).  The
    import call itself must report it (status LAMA_HIP_E_WINDOW), not a later call.  (Nothing is asserted about the receiver's
    state afterwards.)"""
    scan = scan_at(START[0], START[1], 0.0)
    a = Pair(F, 2, _w(16, l2_max), START[0], START[1], 0.0, scan=scan)
    b = Pair(F, 2, _w(16, l2_max), START[0] + 3000.0, START[1], 0.0, scan=scan)
    blob = export_blob(F, a.ctx, 1)
    with pytest.raises(F.LamaError, match=r"status -\d+: .*window"):
        b.ctx.import_particle(0, blob.ptr, blob.n)
    a.close(); b.close()


def check_corrupt_blobs(F, l2_max=None):
    """A blob whose header does not fit is refused ("... does not match this context's geometry") before anything is written:
    the receiver's checksums stay.  The intact blob is then accepted, so each refusal was the corruption's."""
    a = Pair(F, 2, _w(16, l2_max), START[0], START[1], 0.0)
    b = Pair(F, 2, _w(16, l2_max), START[0] + 3 * PATCH_M, START[1] - 2 * PATCH_M, 0.4)
    blob = export_blob(F, a.ctx, 1)
    good = blob.host()
    before = b.checksums()
    cases = {"side no multiple of 8": (5, 20, blob.n), "side below 8": (5, 0, blob.n), "negative patch count": (0, -1, blob.n),
             "negative occupancy patch count": (1, -3, blob.n), "byte count against the header": (None, None, blob.n - 16)}
    for what, (word, value, nbytes) in cases.items():
        bad = good.copy()
        if word is not None:
            bad[32:64].view(np.int32)[word] = value
        blob.store(bad)
        with pytest.raises(F.LamaError, match="geometry"):
            b.ctx.import_particle(0, blob.ptr, nbytes)
        assert np.array_equal(b.checksums(), before), what
        b.assert_maps(f"after the refused blob ({what})")
    blob.store(good)
    b.ctx.import_particle(0, blob.ptr, blob.n)
    assert_maps_equal(b.ctx.download_map(0, F.MAP_DISTANCE), a.pf.dm(1).dump(), DM_FIELDS, "the intact blob")
    assert np.array_equal(b.checksums()[:, 1], before[:, 1])
    a.close(); b.close()
