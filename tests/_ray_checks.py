"""Checks of the integer beam geometry that decides which map cells a scan touches -- a beam's start and hit cell, the 3-axis
step count nn, the closed form floor((2 t a + nn) / (2 nn)), the per-patch step ranges, the patch walk and the 64-beam cone
records -- in its three copies: the beam-sequential k_raycast (lama_kernels.h), beam_geometry (lama_raycast_par.h) with
k_ray_hits / k_ray_alloc_walk / k_ray_patches / k_ray_replay (lama_raycast_patch.h), and k_mb_geom / k_mb_bin / k_mb_patches of
the map rebuild (lama_map_build.h).  Shared by tests/test_ray_geometry_gpu.py and the lane-simulator tests
(tests/test_ray_geometry_sim.py).

Construction: resolution 0.05 m, the sensor on a cell centre (pose (i, j) * 0.05, yaw 0), points (dx, dy, dz) * 0.05, so a
beam's cell deltas are the integers its case names.  Every case first derives, in the reference's own operation order and
through the reference's w2m (the oracle's where the compiled reference is absent), the start and hit cell of EVERY beam it
feeds and asserts the deltas and nn it names (geometry / assert_deltas): a beam that came out differently fails the case, none
is dropped.

References: the particle-filter path against the CPU oracle's particle filter (O.PF: stage_set_scan, stage_update_maps), the
rebuild against tests/_mapbuild.py (the compiled reference's computeRay, setFree, setOccupied).  Everything bit for bit
(assert_maps_equal: OCC_FIELDS and DM_FIELDS on the particle-filter path, OCC_FIELDS for the rebuild); no tolerance anywhere.
Every particle-filter case names its ray-cast form (sequential_raycast = 1 or 2) and asserts from the context's counters that
it took it.
"""
import math

import numpy as np
import pytest

import _oracle as O
import _reference as R
from _cmp import DM_FIELDS, OCC_FIELDS, assert_maps_equal
from _mapbuild import OFF, scan_tf

RES = 0.05
FORMS = (1, 2)                      # cfg.sequential_raycast: 1 = k_raycast, 2 = the parallel kernels
_grid = None


def w2m(p):
    """the reference's Map::w2m of a world point (the oracle's restatement where the compiled reference is not there)"""
    global _grid
    if R.available():
        if _grid is None:
            _grid = R.DM.new(RES)
        return _grid.w2m(p).astype(np.int64)
    return O.w2m(p, RES).astype(np.int64)


def sensor(i, j):
    """the pose whose sensor sits on the centre of cell (OFF + i, OFF + j): patch-local (i mod 32, j mod 32)"""
    return O.se2(i * RES, j * RES, 0.0)


def lattice(deltas):
    """points of a sensor at yaw 0 whose beams have the cell deltas `deltas` ((dx, dy) or (dx, dy, dz) each)"""
    d = np.array([tuple(v) + (0,) * (3 - len(v)) for v in deltas], dtype=np.float64).reshape(-1, 3)
    return d * RES


def geometry(pose4, pts, origin=None, quat=None, trunc_ray=0.0, trunc_range=0.0):
    """Start / hit cell of every beam as PFSlam2D::updateParticleMaps derives them (src/pf_slam2d.cpp:458-493, the transform in
    the operation order of tests/_mapbuild.scan_tf) -> (signed cell deltas (n, 3), nn (n,), mark_hit (n,), start cells (n, 3))."""
    Rm, t = scan_tf(pose4, origin, quat)
    deltas, marks, starts = [], [], []
    for p in np.asarray(pts, dtype=np.float64).reshape(-1, 3):
        px, py, pz = float(p[0]), float(p[1]), float(p[2])
        hit = [((Rm[i][0] * px + Rm[i][1] * py) + Rm[i][2] * pz) + t[i] for i in range(3)]
        start = list(t)
        ab, length, mark = [0.0, 0.0, 0.0], 1.0, True
        if trunc_range > 0.0:
            ab = [hit[i] - start[i] for i in range(3)]
            length = math.sqrt((ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2])
            if trunc_range < length:
                hit = [start[i] + ab[i] / length * trunc_range for i in range(3)]
                mark = False
        if mark and trunc_ray > 0.0:
            if trunc_range == 0.0:
                ab = [hit[i] - start[i] for i in range(3)]
                length = math.sqrt((ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2])
            if trunc_ray < length:
                start = [hit[i] - ab[i] / length * trunc_ray for i in range(3)]
        ms, mh = w2m(start), w2m(hit)
        deltas.append(mh - ms); marks.append(mark); starts.append(ms)
    d = np.array(deltas, dtype=np.int64).reshape(-1, 3)
    return d, np.abs(d).max(axis=1), np.array(marks), np.array(starts).reshape(-1, 3)


def assert_deltas(pose4, pts, want, what, mark=None, start=None, **kw):
    """every beam of the scan has the signed cell deltas `want` (and so the (a0, a1, a2, nn) its case names); mark / start: the
    expected mark_hit flags / start cells relative to the map's origin offset"""
    d, nn, mk, ms = geometry(pose4, pts, **kw)
    want = np.array([tuple(v) + (0,) * (3 - len(v)) for v in want], dtype=np.int64).reshape(-1, 3)
    assert np.array_equal(d, want), (what, np.nonzero((d != want).any(axis=1))[0][:8], d[(d != want).any(axis=1)][:8])
    assert np.array_equal(nn, np.abs(want).max(axis=1)), what
    if mark is not None:
        assert np.array_equal(mk, np.asarray(mark, dtype=bool)), (what, mk)
    if start is not None:
        assert np.array_equal(ms[:, :2] - OFF, np.asarray(start, dtype=np.int64).reshape(-1, 2)), (what, ms[:, :2] - OFF)
    return d, nn


# ------------------------------------------------------------------------------------------------ the two runners
class PFRun:
    """One particle of a device context and of the oracle's filter, fed the same scans at the same poses in the ray-cast form
    `form`; maps bit-equal after every scan, and every scan took the form it names (the counters)."""

    def __init__(self, F, form, pose4, scan, origin=None, quat=None, trunc_ray=0.0, trunc_range=0.0, l2_max=None, what=""):
        self.F, self.form, self.what, self.scans = F, form, what, 0
        self.sensor = dict(origin=O.ZERO3 if origin is None else np.asarray(origin, dtype=np.float64),
                           quat=O.IDENT_Q if quat is None else np.asarray(quat, dtype=np.float64))
        more = {} if l2_max is None else dict(l2_max=l2_max)
        self.pf = O.PF(O.default_options(particles=1, seed=3, truncated_ray=trunc_ray, truncated_range=trunc_range, **more))
        self.pf.set_prior(pose4)
        assert self.pf.update(scan, pose4, 0.0, **self.sensor)
        self.ctx = F.HipContext(F.default_cfg(particles=1, sequential_raycast=form, truncated_ray=trunc_ray, truncated_range=trunc_range, **more))
        self.ctx.init(scan, pose4, **self.sensor)
        self.check("first scan")

    def update(self, pose4, scan, what="", expect_form=None):
        self.pf.set_poses(pose4[None]); self.pf.stage_set_scan(scan, **self.sensor); self.pf.stage_update_maps()
        self.ctx.set_poses(pose4[None]); self.ctx.update_maps(scan, **self.sensor)
        self.check(what, expect_form)

    def check(self, what, expect_form=None):
        F, c = self.F, self.ctx.counters()
        form = self.form if expect_form is None else expect_form
        seq, par = c["sequential_raycast_scans"], c["parallel_raycast_scans"]
        self.scans += 1
        assert seq + par == self.scans, (self.what, what, c)
        if expect_form is None:
            assert (seq, par) == ((self.scans, 0) if form == 1 else (0, self.scans)), (self.what, what, form, seq, par)
        else:
            self.last_forms = (seq, par)
        assert_maps_equal(self.ctx.download_map(0, F.MAP_OCCUPANCY), self.pf.occ(0).dump(), OCC_FIELDS, f"{self.what} {what} form {self.form}: occ")
        assert_maps_equal(self.ctx.download_map(0, F.MAP_DISTANCE), self.pf.dm(0).dump(), DM_FIELDS, f"{self.what} {what} form {self.form}: dm")

    def checksums(self):
        F = self.F
        return np.concatenate([self.ctx.map_checksums(F.MAP_DISTANCE), self.ctx.map_checksums(F.MAP_OCCUPANCY)])

    def close(self):
        self.ctx.close()


def run_pf(F, form, pose4, scan, repeat=1, what="", **kw):
    """the scan as a first scan, then `repeat` more times onto the map it left (cells at the threshold: the ordered replay)"""
    run = PFRun(F, form, pose4, scan, what=what, **kw)
    for k in range(repeat):
        run.update(pose4, scan, f"repetition {k + 1}")
    c = run.ctx.counters()
    run.close()
    return c


def run_rebuild(F, poses4, scans, origins=None, quats=None, what="", fulls=(True, False)):
    """lama_hip_map_integrate_scans against the reference-composed rebuild, full and hits-only"""
    import _mapbuild as MB
    for full in fulls:
        want = MB.build(poses4, scans, origins, quats, full=full).dump()
        ctx = F.HipContext(F.default_cfg(particles=1))
        ctx.integrate_scans(0, poses4, scans, origins, quats, full=full, prune=False)
        assert_maps_equal(ctx.download_map(0, F.MAP_OCCUPANCY), want, OCC_FIELDS, f"{what}: rebuild, full {full}")
        ctx.close()


# ------------------------------------------------------------------------------------------------ 1. the third axis
# beams whose z delta sets nn: several steps then stay in one (x, y) cell, which is visited once per step, and the last of them
# lie in the hit cell.  (0, 0, 7): straight up, six free visits of the sensor's cell and the hit in it; (0, 0, 1): the hit alone;
# (5, 3, 5): a2 == a0 > a1; (5, 3, 6): a2 == a0 + 1; (2, -2, 70) and (0, -1, 100): more steps than a wave has lanes;
# (40, 10, 45) and (-33, 3, 90) leave the sensor's patch; some planar beams among them share their cells.
Z_SENSOR = (3, 5)
Z_DELTAS = [(0, 0, 7), (0, 0, 1), (3, 2, 9), (5, 3, 5), (5, 3, 6), (-4, 7, 20), (2, -2, 70), (0, -1, 100), (40, 10, 45), (3, 1, -8),
            (-33, 3, 90), (5, 3, 0), (0, 0, -3), (3, 2, 0), (-4, 7, 0), (0, 0, 7), (1, 1, 2), (7, 0, 8), (0, 6, -6), (0, 0, 64), (0, 0, 65)]


def check_third_axis_pf(F, form, l2_max=None):
    pose, pts = sensor(*Z_SENSOR), lattice(Z_DELTAS)
    d, nn = assert_deltas(pose, pts, Z_DELTAS, "third axis")
    a = np.abs(d)
    assert (a[:, 2] > np.maximum(a[:, 0], a[:, 1])).sum() >= 14 and ((a[:, 0] == 0) & (a[:, 1] == 0) & (a[:, 2] > 1)).sum() >= 4
    assert any(r[2] == r[0] > r[1] for r in a) and any(r[2] == r[0] + 1 and r[0] > r[1] for r in a)
    run_pf(F, form, pose, pts, repeat=2, what="third axis", l2_max=l2_max)


# a sensor mounted 0.3 m up and rolled by 90 degrees: the planar point (dx, dy, 0) * 0.05 lands at (dx, 0, dy) cells from the
# sensor -- the z delta dominates through the transform, not through the point
ROLL_ORIGIN = np.array([0.1, -0.05, 0.3])
ROLL_QUAT = np.array([math.sqrt(0.5), math.sqrt(0.5), 0.0, 0.0])
ROLL_POINTS = [(3, 9), (0, 12), (-5, 7), (6, 6), (6, 7), (10, -40), (4, 0), (-2, 80)]
ROLL_DELTAS = [(dx, 0, dy) for dx, dy in ROLL_POINTS]


def check_third_axis_through_the_transform_pf(F, form, l2_max=None):
    pose, pts = sensor(*Z_SENSOR), lattice(ROLL_POINTS)
    assert_deltas(pose, pts, ROLL_DELTAS, "rolled sensor", origin=ROLL_ORIGIN, quat=ROLL_QUAT, start=[(Z_SENSOR[0] + 2, Z_SENSOR[1] - 1)] * len(pts))
    run_pf(F, form, pose, pts, repeat=1, what="rolled sensor", origin=ROLL_ORIGIN, quat=ROLL_QUAT, l2_max=l2_max)


def check_third_axis_rebuild(F):
    poses = np.stack([sensor(*Z_SENSOR), sensor(40, -7), sensor(*Z_SENSOR)])
    scans = [lattice(Z_DELTAS), lattice(Z_DELTAS[::-1]), lattice(ROLL_POINTS)]
    origins = np.stack([np.zeros(3), np.zeros(3), ROLL_ORIGIN])
    quats = np.stack([O.IDENT_Q, O.IDENT_Q, ROLL_QUAT])
    assert_deltas(poses[0], scans[0], Z_DELTAS, "third axis")
    assert_deltas(poses[1], scans[1], Z_DELTAS[::-1], "third axis, second sensor")
    assert_deltas(poses[2], scans[2], ROLL_DELTAS, "rolled sensor", origin=ROLL_ORIGIN, quat=ROLL_QUAT)
    run_rebuild(F, poses, scans, origins, quats, "third axis")


LO_DELTAS = [(0, 0, 7), (0, 0, 1), (3, 2, 9), (5, 3, 6), (0, 0, 40), (12, 0, 16), (3, 2, 0), (-4, 7, 0)]


def check_third_axis_lidar_odometry(F):
    """One scan through LidarOdometry2D's map update: the last-metre ray rule (ray_rule = 1) and the log-odds cells
    (occupancy_policy = 1), which live in k_raycast only.  The rule starts a beam of a metre or more one metre before its hit, so
    the long beams are (0, 0, 40): straight up, 20 cells; (12, 0, 16): a 3-4-5 beam of exactly a metre in x and z."""
    pts = lattice(LO_DELTAS)
    assert_deltas(O.se2(0.0, 0.0, 0.0), pts, LO_DELTAS, "lidar odometry")
    o, h = O.LidarOdometry(), F.LidarOdometry2D()
    assert o.update(pts, 0.0) == h.update(pts, 0.0)
    assert_lidar_odometry_maps(F, h.hip_context(), o)
    h.close()


def assert_lidar_odometry_maps(F, ctx, o):
    assert ctx.counters()["sequential_raycast_scans"] == 1
    assert_maps_equal(ctx.download_map(0, F.MAP_DISTANCE), o.dm().dump(), DM_FIELDS, "lidar odometry: dm")
    got, ref = ctx.download_map(0, F.MAP_OCCUPANCY), o.occ().dump()
    assert sorted(got) == sorted(ref) and len(ref) >= 1
    for pid in ref:
        assert np.array_equal(np.ascontiguousarray(got[pid][0]).view(np.float32).reshape(-1), ref[pid][0]["prob"]), pid
        assert np.array_equal(got[pid][1], ref[pid][1]), pid


def check_third_axis_lidar_odometry_context(F):
    """The same scan through a one-particle context configured as LidarOdometry2D configures its own, but with regions of 8 patches:
    the update runs unguarded (no allocation phase under this ray rule), so the regions are grown to everything a scan of this
    reach can touch before the first launch.  (The host class is not loaded here: the lane simulator can run this form.)"""
    pts = lattice(LO_DELTAS)
    o = O.LidarOdometry()
    assert o.update(pts, 0.0)
    ctx = F.HipContext(F.default_cfg(particles=1, device=0, l2_max=1.0, occupancy_policy=1, ray_rule=1, dm_patch_capacity=8,
                                     occ_patch_capacity=8, queue_capacity=1 << 18))
    ctx.init(pts, O.se2(0.0, 0.0, 0.0))
    assert ctx.counters()["arena_growths"] >= 1
    assert_lidar_odometry_maps(F, ctx, o)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. truncation
# The sensor at (0.5, -0.25) and points on multiples of 0.25 m: hit - start is the point itself, exactly, and the 3-4-5 beams
# (0.75, 1.0) k have the lengths 1.25 k exactly -- the comparisons `limit < ray_length` are then decided by the limit's last bit.
T_POSE = (0.5, -0.25)
T_CELL = (10, -5)
T_L = 1.25
# (point in metres, cell deltas of the untruncated beam)
T_BEAMS = [((0.75, 1.0, 0.0), (15, 20, 0)), ((-0.75, 1.0, 0.0), (-15, 20, 0)), ((1.0, -0.75, 0.0), (20, -15, 0)), ((-1.0, -0.75, 0.0), (-20, -15, 0)),
           ((0.75, 0.0, 1.0), (15, 0, 20)), ((0.0, -1.0, -0.75), (0, -20, -15)),
           ((1.5, 2.0, 0.0), (30, 40, 0)), ((-2.0, 1.5, 0.0), (-40, 30, 0)), ((2.25, -3.0, 0.0), (45, -60, 0)),
           ((0.5, 0.25, 0.0), (10, 5, 0)), ((0.0, 0.25, 0.0), (0, 5, 0))]
T_LEN = [1.25] * 6 + [2.5, 2.5, 3.75, None, None]          # None: shorter than every limit used here


def _t_expect(trunc_ray, trunc_range):
    """the deltas, mark_hit flags and start cells the 3-4-5 beams must have: a beam of length 1.25 k has 5 k cells of (3, 4) / 5
    of its deltas per 0.25 m, so a limit of 1.25 m on a longer beam keeps 1.25 / length of them"""
    want, mark, start = [], [], []
    for (p, d), L in zip(T_BEAMS, T_LEN):
        d = np.array(d, dtype=np.int64)
        s = np.zeros(3, dtype=np.int64)
        m = True
        if L is not None and trunc_range > 0.0 and trunc_range < L:
            assert trunc_range >= 1.2 and (trunc_range < 1.3 or abs(trunc_range - 2.5) < 1e-9)
            d = d * (1 if trunc_range < 1.3 else 2) * 5 // int(round(L / 0.25))
            m = False
        if m and L is not None and trunc_ray > 0.0 and trunc_ray < L:
            keep = d * (1 if trunc_ray < 1.3 else 2) * 5 // int(round(L / 0.25))
            s, d = d - keep, keep
        want.append(tuple(int(v) for v in d)); mark.append(m); start.append((T_CELL[0] + int(s[0]), T_CELL[1] + int(s[1])))
    return want, mark, start


def _ulps(x):
    return (np.nextafter(x, 0.0), x, np.nextafter(x, 10.0))


TRUNCATIONS = {}
for _k, _v in zip(("below", "at", "above"), _ulps(T_L)):
    TRUNCATIONS[f"range one ulp {_k} the length" if _k != "at" else "range at the length"] = dict(trunc_ray=0.0, trunc_range=float(_v))
    TRUNCATIONS[f"ray one ulp {_k} the length" if _k != "at" else "ray at the length"] = dict(trunc_ray=float(_v), trunc_range=0.0)
TRUNCATIONS["both, range shorter than ray"] = dict(trunc_ray=2.5, trunc_range=1.25)
TRUNCATIONS["both, range equal to ray"] = dict(trunc_ray=1.25, trunc_range=1.25)
TRUNCATIONS["both, range longer than ray"] = dict(trunc_ray=1.25, trunc_range=2.5)


def check_truncation(F, form, name, l2_max=None):
    kw = TRUNCATIONS[name]
    pose = O.se2(T_POSE[0], T_POSE[1], 0.0)
    pts = np.array([p for p, _ in T_BEAMS])
    want, mark, start = _t_expect(**kw)
    assert_deltas(pose, pts, want, name, mark=mark, start=start, **kw)
    if kw["trunc_range"] == T_L:
        assert all(mark[:6])                       # at the tie the beam is NOT truncated: its hit is marked
    if 0.0 < kw["trunc_range"] < T_L:
        assert not any(mark[:9])
    run_pf(F, form, pose, pts, repeat=1, what=name, l2_max=l2_max, **kw)


T_FAN_RAY = 3.75


def truncated_ray_fan():
    """128 beams in counter-clockwise order, all 3 m long but ONE per chunk of 64, a 3-4-5 beam of 7.5 m that truncated_ray =
    3.75 m starts at its half, 75 cells from the sensor: lane 0 of the first chunk (the lane whose start cell the chunk record
    takes) and lane 54 of the second, each at its place in the angular order.  A chunk whose beams do not share their start
    cell keeps no cone: a cone with its apex at that far start cell would cut the patches around the sensor off.
    -> (points, deltas, start cells)"""
    pts, want, start = [], [], []
    th0 = math.atan2(-6.0, 4.5)
    for k in range(128):
        th = th0 + 0.001 + 2.0 * k / 127.0
        dx, dy = int(round(60 * math.cos(th))), int(round(60 * math.sin(th)))
        if k in (0, 118):
            sg = -1 if k == 0 else 1
            pts.append((4.5, sg * 6.0, 0.0)); want.append((45, sg * 60, 0)); start.append((T_CELL[0] + 45, T_CELL[1] + sg * 60))
        else:
            pts.append((dx * RES, dy * RES, 0.0)); want.append((dx, dy, 0)); start.append(T_CELL)
    ang = [math.atan2(p[1], p[0]) for p in pts]
    assert all(b >= a for a, b in zip(ang, ang[1:]))
    return np.array(pts), want, start


def check_truncated_ray_fan(F, form, l2_max=None):
    pose = O.se2(T_POSE[0], T_POSE[1], 0.0)
    pts, want, start = truncated_ray_fan()
    assert_deltas(pose, pts, want, "truncated_ray fan", start=start, trunc_ray=T_FAN_RAY)
    for c in (0, 1):
        assert sum(tuple(s) != T_CELL for s in start[64 * c:64 * c + 64]) == 1
    run_pf(F, form, pose, pts, repeat=1, what="truncated_ray fan", trunc_ray=T_FAN_RAY, l2_max=l2_max)


# ------------------------------------------------------------------------------------------------ 3. lattice directions, patch edges
AXIS = [(1, 0), (0, 1), (-1, 0), (0, -1)]
DIAG = [(1, 1), (-1, 1), (-1, -1), (1, -1)]
TWO_ONE = [(2 * sx, sy) for sx in (1, -1) for sy in (1, -1)]
ONE_TWO = [(sx, 2 * sy) for sx in (1, -1) for sy in (1, -1)]
LENGTHS = (1, 2, 31, 32, 33, 64)
CORNER_SENSORS = {"(0,0)": (64, 32), "(31,31)": (31, 63), "(0,31)": (-32, 31), "(31,0)": (95, -64)}


def direction_deltas():
    """axis, diagonal, 2:1 and 1:2 beams in all octants with nn of 1, 2, 31, 32, 33 and 64 (the 2:1 beams with an odd nn: the
    shorter axis rounded up), in angular order"""
    out = []
    for L in LENGTHS:
        out += [(L * x, L * y) for x, y in AXIS + DIAG]
        h = (L + 1) // 2
        out += [(L * (x // 2), h * y) for x, y in TWO_ONE] + [(h * x, L * (y // 2)) for x, y in ONE_TWO]
    out.sort(key=lambda d: (math.atan2(d[1], d[0]), abs(d[0]) + abs(d[1])))
    return out


def check_directions(F, form, corner, l2_max=None):
    """from a sensor on a corner cell of its patch: beams of 31 cells end on the far edge of the patch, beams of 32 and 33 on the
    first cells of the next one, a diagonal from the corner cell crosses the patch corner with both axes in one step"""
    i, j = CORNER_SENSORS[corner]
    assert (i % 32, j % 32) == tuple(int(v) for v in corner.strip("()").split(","))
    deltas = direction_deltas()
    pose, pts = sensor(i, j), lattice(deltas)
    d, nn = assert_deltas(pose, pts, deltas, f"directions from {corner}", start=[(i, j)] * len(pts))
    assert set(nn.tolist()) == set(LENGTHS) and len(deltas) == 16 * len(LENGTHS)
    hits = {((i + dx) % 32, (j + dy) % 32) for dx, dy in deltas}
    assert {h[0] for h in hits} >= {0, 31} and {h[1] for h in hits} >= {0, 31}
    run_pf(F, form, pose, pts, repeat=1, what=f"directions from {corner}", l2_max=l2_max)


def check_directions_rebuild(F):
    deltas = direction_deltas()
    poses = np.stack([sensor(*CORNER_SENSORS[c]) for c in sorted(CORNER_SENSORS)])
    for c, pose in zip(sorted(CORNER_SENSORS), poses):
        assert_deltas(pose, lattice(deltas), deltas, c)
    run_rebuild(F, poses, [lattice(deltas)] * len(poses), what="directions")


def ray_cells(frm, to):
    """the reference's computeRay (the oracle's where the compiled reference is absent): the free cells between two cells"""
    if R.available():
        global _grid
        if _grid is None:
            _grid = R.DM.new(RES)
        return _grid.compute_ray(frm, to).astype(np.int64)
    return O.compute_ray(frm, to).astype(np.int64)


def grazing(delta):
    """-> the cells of the beam `delta` from a patch-aligned cell that are the only cell of the beam in their patch, are a corner
    cell of it, and lie strictly on one side of the segment start -> hit (patch-relative coordinates from the start)"""
    base = np.array([OFF + 64, OFF + 64, OFF], dtype=np.int64)
    cells = ray_cells(base, base + np.array([delta[0], delta[1], 0]))[:, :2] - base[:2]
    cells = np.concatenate([cells, [[delta[0], delta[1]]]])
    patches = cells // 32
    out = []
    for k, (c, p) in enumerate(zip(cells[:-1], patches[:-1])):
        alone = int((patches == p).all(axis=1).sum()) == 1
        corner = (c[0] % 32 in (0, 31)) and (c[1] % 32 in (0, 31))
        side = delta[0] * c[1] - delta[1] * c[0]
        if alone and corner and side != 0:
            out.append((int(c[0]), int(c[1])))
    return out


_grazing = None


def grazing_beams(want=3):
    """the example of the issue, delta (100, 97), whose cell (32, 31) is the only one in its patch, and the first other such
    beams of an enumeration over deltas of 90 .. 110 cells with the reference's computeRay"""
    global _grazing
    if _grazing is not None:
        return _grazing
    assert (32, 31) in grazing((100, 97))
    found = [(100, 97)]
    for dx in range(90, 111):
        for dy in range(90, 111):
            if len(found) < want and (dx, dy) not in found and math.gcd(dx, dy) == 1 and grazing((dx, dy)):
                found.append((dx, dy))
    assert len(found) == want
    _grazing = found
    return found


def grazing_fan(delta, position, clockwise):
    """64 beams in angular order (counter-clockwise unless `clockwise`) with the grazing beam as its first, middle (lane 31) or
    last beam: as first or last it IS a cone bound of the chunk, whose test must not cut off the beam's lone corner cell."""
    th0 = math.atan2(delta[1], delta[0])
    n_before = {"first": 0, "middle": 31, "last": 63}[position]
    ks = list(range(-n_before, 0)) + list(range(1, 64 - n_before))
    fan = []
    for k in ks:                                         # a degree apart, 120 .. 179 cells long (rounding turns them by < 0.25 degrees):
        th, r = th0 + math.radians(1.0) * k, 120 + (37 * abs(k)) % 60          # the fan spans 63 degrees, so the chunk has a cone
        fan.append((k, (int(round(r * math.cos(th))), int(round(r * math.sin(th))))))
    fan.append((0, tuple(delta)))
    fan.sort(key=lambda e: e[0])
    deltas = [d for _, d in fan]
    ang = [math.atan2(d[1], d[0]) for d in deltas]
    assert all(b > a for a, b in zip(ang, ang[1:])) and deltas[n_before] == tuple(delta)       # strictly counter-clockwise
    return deltas[::-1] if clockwise else deltas


def check_grazing(F, form, position, clockwise, l2_max=None):
    for delta in grazing_beams():
        deltas = grazing_fan(delta, position, clockwise)
        pose, pts = sensor(64, 64), lattice(deltas)
        assert_deltas(pose, pts, deltas, f"grazing {delta} {position}")
        run_pf(F, form, pose, pts, repeat=0, what=f"grazing {delta} {position} {'cw' if clockwise else 'ccw'}", l2_max=l2_max)


# ------------------------------------------------------------------------------------------------ 4. chunks and scan sizes
def fan(n, span=1.5, start=-0.3, lo=12, hi=45, radius=None):
    """n beams in counter-clockwise order over `span` radians from `start`, lengths of lo .. hi cells (or radius(k)), on the lattice.
    (A chunk of 64 beams keeps a cone while all of them lie within 90 degrees of its first and its last beam: 1.5 rad = 86.)"""
    out = []
    for k in range(n):
        th = start + span * (k / (n - 1) if n > 1 else 0.5)
        r = lo + (k * 7) % (hi - lo + 1) if radius is None else radius(k)
        out.append((int(round(r * math.cos(th))), int(round(r * math.sin(th)))))
    return out


def _fan_case(name):
    """-> (sensor cell, deltas)"""
    if name.startswith("n = "):
        n = int(name[4:])
        if n >= 1024:
            # Thousands of beams share their hit cells, and every visit of a cell hit in the scan is order-sensitive: the active
            # list holds 8192 of them.  Beams of 150 cells, every eighth of 170 (its ray crosses the ring of the others' hits),
            # keep the scan at its n hits plus about n / 4 such visits.
            return (7, 9), fan(n, radius=lambda k: 150 if k % 8 else 170)
        return (7, 9), fan(n)
    if name == "clockwise sweep":
        return (7, 9), fan(128)[::-1]
    if name == "chunk wider than 180 degrees":
        return (7, 9), fan(64, span=5.4, start=-2.7)
    if name == "chunks wider than 90 degrees":                   # in order, but too wide for a cone: tested beam by beam
        return (7, 9), fan(128, span=4.4, start=-2.2)
    if name == "64 identical beams":
        return (7, 9), [(23, -17)] * 64
    if name == "ends of the chunk without free cells":          # lane 0: nn = 0, lane 63: nn = 1, lane 64 (the next chunk): nn = 1
        return (7, 9), [(0, 0)] + fan(62, span=1.4, start=0.2) + [(0, 1), (1, 0)] + fan(62, span=1.4, start=2.0)[::-1] + [(0, 0)]
    if name == "1024 beams inside the sensor's patch":
        # from patch-local (16, 16) to the 120 cells of the square ring 15 cells out, no angular order (no chunk has a cone): every
        # beam of the scan is a candidate of the one patch.  (Hits on every cell of the patch would make all ~10,000 visits
        # order-sensitive, more than the 8192 the active list holds: such a scan is refused, which is not what this case is about.)
        ring = [(x, y) for x in range(-15, 16) for y in range(-15, 16) if max(abs(x), abs(y)) == 15]
        order = np.random.default_rng(11).permutation(1024)
        return (16, 16), [ring[k % len(ring)] for k in order]
    raise KeyError(name)


FAN_CASES_SMALL = ["n = 1", "n = 63", "n = 64", "n = 65", "n = 128", "clockwise sweep", "chunk wider than 180 degrees", "chunks wider than 90 degrees", "64 identical beams",
                   "ends of the chunk without free cells", "1024 beams inside the sensor's patch"]
FAN_CASES_LARGE = ["n = 4095", "n = 4096"]


def check_fan(F, form, name, l2_max=None):
    (i, j), deltas = _fan_case(name)
    pose, pts = sensor(i, j), lattice(deltas)
    d, nn = assert_deltas(pose, pts, deltas, name, start=[(i, j)] * len(pts))
    if name == "1024 beams inside the sensor's patch":
        assert len(pts) == 1024 and all((i + dx) // 32 == 0 and (j + dy) // 32 == 0 for dx, dy in deltas)
    if name == "ends of the chunk without free cells":
        assert len(pts) == 128 and nn[0] == 0 and nn[63] == 1 and nn[64] == 1 and nn[127] == 0 and nn[1:63].min() > 1
    run_pf(F, form, pose, pts, repeat=1, what=name, l2_max=l2_max)


def check_scan_of_4097_points_goes_sequential(F):
    """one point more than k_ray_patches has chunk lanes for: the parallel form is asked for, the counters show k_raycast"""
    deltas = fan(4097)
    pose, pts = sensor(7, 9), lattice(deltas)
    assert_deltas(pose, pts, deltas, "n = 4097")
    run = PFRun(F, 2, pose, lattice(fan(64)), what="n = 4097")
    assert run.ctx.counters()["parallel_raycast_scans"] == 1
    run.update(pose, pts, "4097 points", expect_form=1)
    assert run.last_forms == (1, 1), run.last_forms
    run.close()


# ------------------------------------------------------------------------------------------------ 5. the length limit
LONGEST = 8191                                                     # cells: the closed form's multiplier holds 13 bits of nn
LONG_SCANS = {"axis": [(LONGEST, 0), (-3, 4), (0, -LONGEST)], "2:1": [(LONGEST, 4096), (-5, 2, 12), (-4096, -LONGEST)],
              "third axis": [(100, 0, LONGEST), (3, 4)]}


def check_longest_beam(F, form, which, l2_max=None):
    """a beam of exactly 8191 cells is mapped bit for bit, in a window that had to grow from its 128 patches to hold it"""
    deltas = LONG_SCANS[which]
    pose, pts = sensor(0, 0), lattice(deltas)
    d, nn = assert_deltas(pose, pts, deltas, f"longest beam, {which}")
    assert nn.max() == LONGEST
    c = run_pf(F, form, pose, pts, repeat=0, what=f"longest beam, {which}", l2_max=l2_max)
    if which != "third axis":
        assert c["window_patches"] >= 2 * 256 and c["window_patches"] % 8 == 0, c      # the sensor +- 8191 cells = 256 patches each way
    return c


def check_too_long_beam_pf(F, form, l2_max=None):
    """8192 cells: refused with the window status, both maps keep their checksums -- and the context still maps the next scan"""
    short = [(15, 20), (-7, 3), (0, -9)]
    pose = sensor(0, 0)
    run = PFRun(F, form, pose, lattice(short), what="too long", l2_max=l2_max)
    for long_one in [(LONGEST + 1, 0), (0, -(LONGEST + 1)), (3, 0, LONGEST + 1), (-(LONGEST + 1), 4096)]:
        deltas = short + [long_one]
        pts = lattice(deltas)
        d, nn = assert_deltas(pose, pts, deltas, "too long")
        assert nn.max() == LONGEST + 1
        before = run.checksums()
        run.ctx.set_poses(pose[None])
        with pytest.raises(F.LamaError, match=r"status -3: .*window"):
            run.ctx.update_maps(pts)
        assert np.array_equal(run.checksums(), before), long_one
        assert_maps_equal(run.ctx.download_map(0, F.MAP_OCCUPANCY), run.pf.occ(0).dump(), OCC_FIELDS, f"after the refused {long_one}")
    run.scans = run.ctx.counters()["sequential_raycast_scans"] + run.ctx.counters()["parallel_raycast_scans"]
    run.update(pose, lattice(short + [(LONGEST, 0)]), "the longest beam after the refusals")
    run.close()


def check_length_limit_rebuild(F):
    import _mapbuild as MB
    pose = sensor(0, 0)
    for which in sorted(LONG_SCANS):
        assert_deltas(pose, lattice(LONG_SCANS[which]), LONG_SCANS[which], which)
        run_rebuild(F, pose[None], [lattice(LONG_SCANS[which])], what=f"longest beam, {which}")
    short = [(15, 20), (-7, 3), (0, -9)]
    ctx = F.HipContext(F.default_cfg(particles=1))
    ctx.integrate_scans(0, pose[None], [lattice(short)], prune=False)
    want = MB.build(pose[None], [lattice(short)]).dump()
    cks = ctx.map_checksums(F.MAP_OCCUPANCY)
    for long_one in [(LONGEST + 1, 0), (0, -(LONGEST + 1)), (3, 0, LONGEST + 1)]:
        deltas = short + [long_one]
        d, nn = assert_deltas(pose, lattice(deltas), deltas, "too long")
        assert nn.max() == LONGEST + 1
        with pytest.raises(F.LamaError, match=r"status -3: .*8191"):
            ctx.integrate_scans(0, pose[None], [lattice(deltas)], prune=False)
        assert np.array_equal(ctx.map_checksums(F.MAP_OCCUPANCY), cks), long_one
        assert_maps_equal(ctx.download_map(0, F.MAP_OCCUPANCY), want, OCC_FIELDS, f"after the refused {long_one}")
    ctx.integrate_scans(0, pose[None], [lattice(deltas)], full=False, prune=False)       # hits only: no ray, nothing to refuse
    assert not np.array_equal(ctx.map_checksums(F.MAP_OCCUPANCY), cks)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. what the simulator compiles out
# dir_get_or_alloc's election among the lanes of a wave that miss a directory entry together (k_ray_hits: a lane per beam, its
# hit cell's patch).  Hits 40 cells up from patch-local (8, 8): row 1 of patches, columns as the case says.
ELECTION = {
    "64 distinct missing patches": [(32 * k + 3, 40) for k in range(64)],
    "two missing patches, interleaved": [(32 * (k & 1) + 1 + k // 4, 40 + k % 7) for k in range(64)],
    "one missing patch": [(1 + k % 16, 36 + k // 16) for k in range(64)],
}


def check_election(F, name):
    """a fresh particle: its first scan's 64 hits are the first wave that asks for these patches"""
    pose, deltas = sensor(8, 8), ELECTION[name]
    pts = lattice(deltas)
    assert_deltas(pose, pts, deltas, name)
    cols = {(8 + dx) // 32 for dx, dy in deltas}
    assert len(cols) == {"64 distinct missing patches": 64, "two missing patches, interleaved": 2, "one missing patch": 1}[name]
    assert {(8 + dy) // 32 for dx, dy in deltas} == {1}
    for form in FORMS:
        run_pf(F, form, pose, pts, repeat=0, what=name)


def check_election_with_half_the_patches_there(F):
    """The first scan maps the even patch columns of the row, the second one hits all 64 columns from one wave.  truncated_ray =
    0.5 m keeps every ray inside its hit's patch (a full ray to column k would cross, and allocate, the columns before it); the
    deltas of such beams are not lattice numbers, so the case names their hit cells and the patch of their start cells."""
    pose, tr = sensor(8, 8), 0.5
    even = [(32 * k + 3, 40) for k in range(0, 64, 2)]
    every = [(32 * k + 5, 44) for k in range(64)]
    for deltas in (even, every):
        d, nn, mk, ms = geometry(pose, lattice(deltas), trunc_ray=tr)
        hits = (ms + d)[:, :2] - OFF
        assert np.array_equal(hits, np.array(deltas) + 8) and mk.all()
        assert np.array_equal((ms[:, :2] - OFF) // 32, hits // 32) and nn.min() >= 7 and nn.max() <= 10      # the ray stays in the hit's patch
    col = lambda k: ((OFF + 8 + 32 * k) // 32) * 2642244 + (OFF + 8 + 44) // 32                  # the reference's patch id: x-major
    for form in FORMS:
        run = PFRun(F, form, pose, lattice(even), what="half the patches exist", trunc_ray=tr)
        have = set(run.ctx.download_map(0, F.MAP_OCCUPANCY))
        assert [col(k) in have for k in range(64)] == [k % 2 == 0 for k in range(64)]
        run.update(pose, lattice(every), "all columns")
        assert all(col(k) in set(run.ctx.download_map(0, F.MAP_OCCUPANCY)) for k in range(64))
        run.close()


def bin_add_log():
    """200 posed scans of 1 to 3 points with their sensors in 12 patches: 70 of them in one patch with beams that stay inside it,
    60 in a second one, 7 in each of ten more.  -> (sensor cells, deltas per scan, patch number per scan) in an order in which the
    patch changes from scan to scan."""
    rng = np.random.default_rng(29)
    owner = [0] * 70 + [1] * 60 + [2 + k % 10 for k in range(70)]
    owner = [owner[k] for k in rng.permutation(200)]
    cells, scans = [], []
    for k, o in enumerate(owner):
        px, py = o % 4, o // 4
        n = 1 + k % 3
        if o == 0:                                               # around the middle of the patch, hits within it
            cells.append((32 * px + int(rng.integers(12, 20)), 32 * py + int(rng.integers(12, 20))))
            scans.append([(int(rng.integers(-10, 11)), int(rng.integers(-10, 11))) for _ in range(n)])
        else:
            cells.append((32 * px + int(rng.integers(0, 32)), 32 * py + int(rng.integers(0, 32))))
            scans.append([(int(rng.integers(-60, 61)), int(rng.integers(-60, 61))) for _ in range(n)])
    return cells, scans, owner


def _waves(values):
    """the values of the lanes of every full wave of k_mb_bin (a thread per point, 64 consecutive points)"""
    return [values[w:w + 64] for w in range(0, len(values) - 63, 64)]


def check_bin_add(F):
    """mb_bin_add's shared atomic: the lanes whose bin is the first active lane's add together, the others on their own.  In the
    mixed order every wave holds many different bins (for the hits and for the first patch of the rays); sorted by patch, whole
    waves share one bin in both."""
    cells, deltas, owner = bin_add_log()
    assert len(set(owner)) == 12 and len({(i // 32, j // 32) for i, j in cells}) == 12
    npts = sum(len(d) for d in deltas)
    assert 390 <= npts <= 410
    for name, idx in (("mixed bins", list(range(200))), ("sorted by bin", sorted(range(200), key=lambda k: owner[k]))):
        poses = np.stack([sensor(*cells[k]) for k in idx])
        scans = [lattice(deltas[k]) for k in idx]
        for k in idx:
            assert_deltas(sensor(*cells[k]), lattice(deltas[k]), deltas[k], name, start=[cells[k]] * len(deltas[k]))
        start_bin = [owner[k] for k in idx for _ in deltas[k]]
        hit_bin = [((cells[k][0] + dx) // 32, (cells[k][1] + dy) // 32) for k in idx for dx, dy in deltas[k]]
        if name == "mixed bins":
            assert all(len(set(w)) >= 6 for w in _waves(start_bin)) and all(len(set(w)) >= 6 for w in _waves(hit_bin))
        else:
            assert any(len(set(w)) == 1 and len(set(h)) == 1 for w, h in zip(_waves(start_bin), _waves(hit_bin)))
        run_rebuild(F, poses, scans, what=name, fulls=(True,))


def check_oracle_against_the_reference_on_the_third_axis():
    """The oracle's particle filter is pinned to the reference on planar scans; this pins its first map update on beams whose z
    delta sets nn: the occupancy map of the first scan is the reference-composed rebuild of that scan."""
    import _mapbuild as MB
    for pts, kw in ((lattice(Z_DELTAS), {}), (lattice(ROLL_POINTS), dict(origin=ROLL_ORIGIN, quat=ROLL_QUAT))):
        pose = sensor(*Z_SENSOR)
        pf = O.PF(O.default_options(particles=1, seed=3))
        pf.set_prior(pose)
        assert pf.update(pts, pose, 0.0, **kw)
        want = MB.build(pose[None], [pts], None if not kw else kw["origin"][None], None if not kw else kw["quat"][None], full=True).dump()
        assert_maps_equal(pf.occ(0).dump(), want, OCC_FIELDS, "oracle against the reference")
