"""The cases of lama_hip_map_cast_rays (iris_lama_amd/csrc/lama_raycast_query.h), shared by the lane-simulator run
(tests/test_raycast_query_sim.py) and the run on the device (tests/test_raycast_query_gpu.py).  `F` is iris_lama_amd.ffi bound to
the library under test.  Every expected result is computed by tests/_raycast_query.py from HipContext.download_map, the reference's
w2m and the reference's computeRay; every comparison is array_equal, ranges included.

Construction as in tests/_ray_checks.py: resolution 0.05 m, the sensor on a cell centre (RY.sensor), points on the lattice
(RY.lattice), so a beam's cell deltas are the integers its case names; cells are named relative to the map's origin cell OFF."""
import ctypes as C
import math

import numpy as np

import _raster as RS
import _raster_checks as RC
import _raycast_query as RQ
import _ray_checks as RY
from _mapbuild import OFF

E_INVALID, E_WINDOW = -1, -3
OFFP = OFF >> 5
FREE_CELL, OCC_CELL, QUARTER_CELL, NEW_CELL = (0, 9), (5, 9), (2, 8), (0, 0)      # (occupied, visited)
assert OFF % 32 == 0 and OFFP == RC.OFF_PATCH


# ------------------------------------------------------------------------------------------------ constructed maps
def _mask(bits):
    m = np.zeros(16, dtype=np.uint64)
    for c in np.flatnonzero(np.asarray(bits).reshape(-1)):
        m[c >> 6] |= np.uint64(1) << np.uint64(c & 63)
    return m


def patches_over(cells, extra=()):
    """the patch columns / rows (relative to the origin's patch) that hold the given relative cells"""
    return sorted({(x >> 5, y >> 5) for x, y in list(cells) + list(extra)})


def occupancy_map(F, patches, special, fill=FREE_CELL, mask_off=()):
    """{patch id: (cells, mask)}: the listed patches filled with `fill`, then {(x, y): (occupied, visited)} of `special`; the mask
    bit of a cell is "visited != 0" unless it is in mask_off"""
    out = {}
    for px, py in patches:
        a = np.zeros((32, 32), dtype=F.FREQ_T)
        a["occupied"], a["visited"] = fill
        on = np.ones((32, 32), dtype=bool)
        for (x, y), v in special.items():
            if (x >> 5, y >> 5) == (px, py):
                a[y & 31, x & 31] = v
        for x, y in mask_off:
            if (x >> 5, y >> 5) == (px, py):
                on[y & 31, x & 31] = False
        out[RS.patch_id(OFFP + px, OFFP + py)] = (a.reshape(-1), _mask(on))
    return out


def logodds_map(F, patches, special, fill=-0.4, mask_off=()):
    """the same with float log-odds cells (cfg.occupancy_policy 1)"""
    out = {}
    for px, py in patches:
        l = np.full((32, 32), fill, dtype=np.float32)
        on = np.ones((32, 32), dtype=bool)
        for (x, y), v in special.items():
            if (x >> 5, y >> 5) == (px, py):
                l[y & 31, x & 31] = v
        for x, y in mask_off:
            if (x >> 5, y >> 5) == (px, py):
                on[y & 31, x & 31] = False
        out[RS.patch_id(OFFP + px, OFFP + py)] = (np.ascontiguousarray(l).view(F.FREQ_T).reshape(-1), _mask(on))
    return out


def distance_map(F, patches, special, fill=(4, 1), mask_off=()):
    """the same with distance cells: {(x, y): (sqdist, valid)}"""
    out = {}
    for px, py in patches:
        a = np.zeros((32, 32), dtype=F.DIST_T)
        a["sqdist"], a["valid"] = fill
        on = np.ones((32, 32), dtype=bool)
        for (x, y), v in special.items():
            if (x >> 5, y >> 5) == (px, py):
                a["sqdist"][y & 31, x & 31], a["valid"][y & 31, x & 31] = v
        for x, y in mask_off:
            if (x >> 5, y >> 5) == (px, py):
                on[y & 31, x & 31] = False
        out[RS.patch_id(OFFP + px, OFFP + py)] = (a.reshape(-1), _mask(on))
    return out


class Case:
    """a one-particle context with an uploaded map of one kind; cast() runs the call and compares it with the numpy expectation"""

    def __init__(self, F, kind, patches, policy=0, l2_max=None, dm_patches=None):
        kw = {}
        if policy:
            kw.update(occupancy_policy=1, ray_rule=1, l2_max=1.0)
        if l2_max is not None:
            kw["l2_max"] = l2_max
        self.F, self.kind, self.policy = F, kind, policy
        self.ctx = F.HipContext(F.default_cfg(particles=1, **kw))
        self.mx = RC.max_sqdist_of(self.ctx.cfg)
        self.upload(patches, dm_patches)

    def upload(self, patches, dm_patches=None):
        F = self.F
        self.ctx.upload_map(0, self.kind, patches)
        if dm_patches is not None:
            self.ctx.upload_map(0, F.MAP_DISTANCE, dm_patches)
        self.dump = self.ctx.download_map(0, self.kind)
        self.dm = self.ctx.download_map(0, F.MAP_DISTANCE)
        assert sorted(self.dump) == sorted(patches)

    def cast(self, poses4, pts, what, stop_unknown=False, tolerance=-1, origin=None, quat=None):
        F = self.F
        poses4 = np.asarray(poses4, dtype=np.float64).reshape(-1, 4)
        want = RQ.expected(poses4, pts, self.dump, self.kind == F.MAP_DISTANCE, self.dm, self.mx, origin=origin, quat=quat, policy=self.policy,
                           stop_unknown=stop_unknown, tolerance=tolerance)
        before = (self.ctx.map_checksums(F.MAP_DISTANCE), self.ctx.map_checksums(F.MAP_OCCUPANCY)) if self.policy == 0 else None      # (checksums cover frequency cells)
        got = self.ctx.cast_rays(0, self.kind, poses4, pts, origin, quat, stop_unknown, tolerance)
        RQ.assert_equal(got, want, what)
        if before is not None:                                   # read-only: no map changed
            assert np.array_equal(before[0], self.ctx.map_checksums(F.MAP_DISTANCE)) and np.array_equal(before[1], self.ctx.map_checksums(F.MAP_OCCUPANCY)), what
        return want

    def close(self):
        self.ctx.close()


def stops(want):
    """{(relative stopping cell): class} over all rays that stopped"""
    out = {}
    for k, i in np.argwhere(want.status != RQ.NONE):
        out[(int(want.cell_xy[k, i, 0]) - OFF, int(want.cell_xy[k, i, 1]) - OFF)] = int(want.stop_class[k, i])
    return out


# ------------------------------------------------------------------------------------------------ 1. cell classes on constructed maps
# Row y = 5 of a map whose patches span exactly the 128 patch columns of a fresh context's window: columns 0, 1, 3 and 127 exist,
# column 2 is absent, and the cells x < 0 and x >= 4096 lie outside the window.
ROW = 5
ROW_SENSORS = [8, 13, 20, 97, 4090, -6]
ROW_BEAMS = [(3, 0), (5, 0), (7, 0), (10, 0), (26, 0), (90, 0), (116, 0)]
ROW_PATCHES = [(0, 0), (1, 0), (3, 0), (127, 0)]


def _row_case(case, what):
    F = case.F
    assert case.ctx.counters()["window_patches"] == 128          # columns 0 .. 127: the window cannot lie anywhere else along x
    poses = np.stack([RY.sensor(x, ROW) for x in ROW_SENSORS])
    pts = RY.lattice(ROW_BEAMS)
    for k, x in enumerate(ROW_SENSORS):
        RY.assert_deltas(poses[k], pts, ROW_BEAMS, what, start=[(x, ROW)] * len(pts))
    plain = case.cast(poses, pts, f"{what}, unknown cells pass")
    su = case.cast(poses, pts, f"{what}, unknown cells stop", stop_unknown=True) if case.kind == F.MAP_OCCUPANCY else None
    return plain, su


def check_cell_classes_frequency(F):
    special = {(12, ROW): QUARTER_CELL, (14, ROW): NEW_CELL, (100, ROW): OCC_CELL}
    case = Case(F, F.MAP_OCCUPANCY, occupancy_map(F, ROW_PATCHES, special))
    plain, su = _row_case(case, "frequency cells")
    # every class is the stopping one of some ray: equality, visited == 0, the absent patch, outside the window on either side, occupied
    s = stops(su)
    assert s[(12, ROW)] == RQ.UNKNOWN and s[(14, ROW)] == RQ.UNKNOWN and s[(64, ROW)] == RQ.UNKNOWN and s[(4096, ROW)] == RQ.UNKNOWN
    assert s[(-5, ROW)] == RQ.UNKNOWN and s[(100, ROW)] == RQ.OCCUPIED
    assert set(stops(plain).items()) == {((100, ROW), RQ.OCCUPIED)} and (plain.status == RQ.NONE).sum() > 20
    # the ray from x = 20 to x = 110 meets free cells, the absent patch and then the occupied cell; the one from x = -6 every class in turn
    k, i = ROW_SENSORS.index(20), ROW_BEAMS.index((90, 0))
    assert plain.status[k, i] == RQ.OCCUPIED and plain.step[k, i] == 79 and su.step[k, i] == 43
    k, i = ROW_SENSORS.index(-6), ROW_BEAMS.index((116, 0))
    assert plain.status[k, i] == RQ.OCCUPIED and plain.step[k, i] == 105 and su.status[k, i] == RQ.UNKNOWN and su.step[k, i] == 0
    assert plain.range[k, i] == 0.05 * math.sqrt(106.0 * 106.0)
    k, i = ROW_SENSORS.index(8), ROW_BEAMS.index((3, 0))        # free cells only: nothing stops the ray either way
    assert plain.status[k, i] == su.status[k, i] == RQ.NONE and np.isinf(su.range[k, i])
    case.close()


def check_cell_classes_log_odds(F):
    # l > 0 with the mask bit OFF is not a cell (Map::get): unknown; l == 0 with the bit on is unknown; l < 0 is free
    special = {(12, ROW): 0.0, (14, ROW): 0.85, (100, ROW): 0.85, (10, ROW): -2.0}
    case = Case(F, F.MAP_OCCUPANCY, logodds_map(F, ROW_PATCHES, special, mask_off=[(14, ROW)]), policy=1)
    plain, su = _row_case(case, "log-odds cells")
    s = stops(su)
    assert s[(12, ROW)] == RQ.UNKNOWN and s[(14, ROW)] == RQ.UNKNOWN and s[(64, ROW)] == RQ.UNKNOWN and s[(4096, ROW)] == RQ.UNKNOWN
    assert s[(-5, ROW)] == RQ.UNKNOWN and s[(100, ROW)] == RQ.OCCUPIED
    assert set(stops(plain).items()) == {((100, ROW), RQ.OCCUPIED)}
    case.close()


def check_cell_classes_distance(F, l2_max=None):
    # valid with sqdist 1, INVALID with sqdist 0, a cell whose mask bit is off, and two obstacle cells (valid, sqdist 0)
    special = {(12, ROW): (1, 1), (14, ROW): (0, 0), (16, ROW): (0, 0), (40, ROW): (0, 1), (100, ROW): (0, 1)}
    case = Case(F, F.MAP_DISTANCE, distance_map(F, ROW_PATCHES, special, mask_off=[(16, ROW)]), l2_max=l2_max)
    assert case.ctx.L is F.hip_lib(wide=l2_max is not None and F.needs_wide(l2_max, 0.05))
    plain, _ = _row_case(case, f"distance cells, reach {case.mx}")
    assert set(stops(plain).items()) == {((40, ROW), RQ.OCCUPIED), ((100, ROW), RQ.OCCUPIED)}
    k, i = ROW_SENSORS.index(8), ROW_BEAMS.index((90, 0))       # past 12, 14 and 16 to the obstacle at 40
    assert plain.step[k, i] == 31 and plain.end_sqdist[k, i] == 4
    k, i = ROW_SENSORS.index(8), ROW_BEAMS.index((10, 0))       # ... and short of it: nothing stops the ray
    assert plain.status[k, i] == RQ.NONE
    k, i = ROW_SENSORS.index(20), ROW_BEAMS.index((90, 0))      # the hit cell (110, 5) is free, 100 is on the way, 40 too
    assert plain.step[k, i] == 19
    k = ROW_SENSORS.index(4090)                                  # hit cells outside the window: the largest distance
    assert np.all(plain.end_sqdist[k, 3:] == case.mx)
    case.close()


# ------------------------------------------------------------------------------------------------ 2. directions and geometry
SENSOR = (7, 9)
Z_BEAMS = [(5, 3, 6), (3, 2, 9), (0, 0, 7)]
PLACES = ("step 0", "middle", "hit", "beside", "start")


GRAZING_SENSOR = (64, 64)            # patch-aligned, as RY.grazing takes it: the lone corner cells are lone from here


def _beams():
    """(sensor cell, deltas)"""
    return [(SENSOR, tuple(d)) for d in RY.direction_deltas()] + [(SENSOR, d) for d in Z_BEAMS] + [(GRAZING_SENSOR, tuple(d)) for d in RY.grazing_beams()]


def _single_obstacle(F, case, SENSOR, delta, place, lone=None):
    """one beam from SENSOR over free cells with ONE occupied cell at `place` of its sequence -> (want, sequence, obstacle cell)"""
    pose, pts = RY.sensor(*SENSOR), RY.lattice([delta])
    d, nn, _, starts = RY.geometry(pose, pts)
    start, hit = starts[0], starts[0] + d[0]
    seq = RQ.sequence(start, hit) - OFF
    on_path = {(int(x), int(y)) for x, y in seq}
    if place == "step 0":
        cell = tuple(int(v) for v in seq[0])
    elif place == "middle":
        cell = lone if lone is not None else tuple(int(v) for v in seq[len(seq) // 2])
    elif place == "hit":
        cell = tuple(int(v) for v in seq[-1])
    elif place == "start":
        cell = SENSOR
    else:                                                         # one cell beside the walk, not on it
        mid = seq[len(seq) // 2]
        cell = next(c for c in ((int(mid[0]) + dx, int(mid[1]) + dy) for dx, dy in ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (-1, -1))) if c not in on_path and c != SENSOR)
    box = [SENSOR, (int(hit[0]) - OFF, int(hit[1]) - OFF), cell]
    lo, hi = np.min(box, axis=0) >> 5, np.max(box, axis=0) >> 5
    patches = [(px, py) for px in range(int(lo[0]), int(hi[0]) + 1) for py in range(int(lo[1]), int(hi[1]) + 1)]
    case.upload(occupancy_map(F, patches, {cell: OCC_CELL}))
    want = case.cast(pose, pts, f"beam {delta}, obstacle at {place} {cell}")
    return want, seq, cell, on_path


def check_directions(F, place):
    """every direction of RY.direction_deltas (all octants, the axes, the diagonals, 1 .. 64 cells), beams whose third axis sets the
    step count, and the grazing beams with the obstacle on their lone corner cell"""
    case = Case(F, F.MAP_OCCUPANCY, occupancy_map(F, [(0, 0)], {}))
    graze = {tuple(d): RY.grazing(d)[0] for d in RY.grazing_beams()}
    seen = 0
    for sensor, delta in _beams():
        lone = None
        if sensor == GRAZING_SENSOR:                             # RY.grazing names the cell relative to the beam's start
            g = graze[tuple(delta)]
            lone = (sensor[0] + g[0], sensor[1] + g[1])
        want, seq, cell, on_path = _single_obstacle(F, case, sensor, delta, place, lone)
        planar = len(delta) == 2
        nn = len(seq)
        assert want.nn[0, 0] == nn == max(abs(v) for v in delta)
        if place in ("step 0", "middle", "hit") and planar:
            k = {"step 0": 0, "middle": nn // 2, "hit": nn - 1}[place]
            if lone is not None and place == "middle":
                assert lone in on_path, (delta, lone)            # the lone corner cell IS a cell of the walk
                k = [tuple(int(v) for v in c) for c in seq].index(lone)
            assert want.status[0, 0] == RQ.OCCUPIED and want.step[0, 0] == k, (delta, place, want.step)
            assert (int(want.cell_xy[0, 0, 0]) - OFF, int(want.cell_xy[0, 0, 1]) - OFF) == cell
            seen += 1
        if place in ("beside", "start") and planar:              # neither stops the ray: the start cell is never tested
            assert want.status[0, 0] == RQ.NONE and want.step[0, 0] == -1 and np.isinf(want.range[0, 0]), (delta, place)
            seen += 1
    assert seen >= 96 + 3
    case.close()


def check_beam_inside_the_sensor_cell(F):
    """nn == 0: none / -1, whatever the cell holds; beside a beam of one cell in the same call"""
    case = Case(F, F.MAP_OCCUPANCY, occupancy_map(F, [(0, 0)], {SENSOR: OCC_CELL, (SENSOR[0] + 1, SENSOR[1]): OCC_CELL}))
    for su in (False, True):
        want = case.cast(RY.sensor(*SENSOR), RY.lattice([(0, 0), (1, 0), (0, 0, 0)]), "nn == 0", stop_unknown=su)
        assert want.nn[0].tolist() == [0, 1, 0] and want.status[0].tolist() == [RQ.NONE, RQ.OCCUPIED, RQ.NONE] and want.step[0].tolist() == [-1, 0, -1]
    case.close()


def check_patch_crossings(F):
    """a ray that starts at patch-local 31 and crosses into the next patch on its first step; a ray across four patches with its
    obstacle in the fourth, in the third (an absent patch before it), and nowhere"""
    case = Case(F, F.MAP_OCCUPANCY, occupancy_map(F, [(0, 0), (1, 0)], {(32, 9): OCC_CELL}))
    pose, pts = RY.sensor(31, 9), RY.lattice([(5, 0), (5, 5), (0, 5)])
    RY.assert_deltas(pose, pts, [(5, 0), (5, 5), (0, 5)], "from local 31", start=[(31, 9)] * 3)
    want = case.cast(pose, pts, "first step into the next patch")
    assert want.status[0].tolist() == [RQ.OCCUPIED, RQ.NONE, RQ.NONE] and want.step[0, 0] == 0
    beams = [(120, 2), (120, 0), (100, 2)]
    pose, pts = RY.sensor(3, 9), RY.lattice(beams)
    for patches, special, first in (([(0, 0), (1, 0), (2, 0), (3, 0)], {(123, 11): OCC_CELL}, 119), ([(0, 0), (2, 0), (3, 0)], {(70, 10): OCC_CELL}, 66),
                                    ([(0, 0), (1, 0), (2, 0), (3, 0)], {}, -1)):
        case.upload(occupancy_map(F, patches, special))
        for su in (False, True):
            want = case.cast(pose, pts, f"four patches, obstacle {sorted(special)}, stop_unknown {su}", stop_unknown=su)
            if not su:
                assert want.step[0, 0] == first, (want.step, first)
            elif len(patches) == 3:
                assert want.status[0, 0] == RQ.UNKNOWN and want.step[0, 0] == 28            # x = 32: the first cell of the absent patch
    case.close()


# ------------------------------------------------------------------------------------------------ 3. edges of the launch
def _walled_room(F):
    """3 x 3 patches of free cells around the sensor's patch with a wall along x = 27 and one along y = -14"""
    patches = [(px, py) for px in (-1, 0, 1) for py in (-1, 0, 1)]
    special = {(27, y): OCC_CELL for y in range(-32, 64)}
    special.update({(x, -14): OCC_CELL for x in range(-32, 64)})
    return occupancy_map(F, patches, special)


def check_scan_sizes(F):
    case = Case(F, F.MAP_OCCUPANCY, _walled_room(F))
    for n in (1, 64, 65, 256, 257):
        deltas = RY.fan(n)
        pose, pts = RY.sensor(*SENSOR), RY.lattice(deltas)
        RY.assert_deltas(pose, pts, deltas, f"n = {n}")
        want = case.cast(pose, pts, f"n = {n}", stop_unknown=(n % 2 == 0))
        if n > 1:
            assert (want.status == RQ.OCCUPIED).any() and (want.status == RQ.NONE).any(), n
    case.close()


def check_three_poses(F):
    case = Case(F, F.MAP_OCCUPANCY, _walled_room(F))
    deltas = RY.fan(65)
    poses, pts = np.stack([RY.sensor(7, 9), RY.sensor(12, 9), RY.sensor(7, 30)]), RY.lattice(deltas)
    want = case.cast(poses, pts, "three poses")
    assert not np.array_equal(want.step[0], want.step[1]) and not np.array_equal(want.step[0], want.step[2]) and not np.array_equal(want.step[1], want.step[2])
    one = case.cast(poses[1:2], pts, "the second pose alone")
    assert np.array_equal(one.step[0], want.step[1]) and np.array_equal(one.range[0], want.range[1])
    case.close()


def check_mixed_wave(F):
    """64 beams of ONE wave, interleaved: stop at step 0, at step 1, at step nn - 1, never"""
    beams = []
    for i in range(16):
        beams += [(10 + i, i % 3), (0, 5 + i), (-20, 15 - 2 * i), (15 + i, 20 + i)]
    special = {(SENSOR[0] + 1, SENSOR[1]): OCC_CELL, (SENSOR[0], SENSOR[1] + 2): OCC_CELL}
    special.update({(SENSOR[0] - 20, SENSOR[1] + 15 - 2 * i): OCC_CELL for i in range(16)})
    patches = [(px, py) for px in (-1, 0, 1) for py in (-1, 0, 1)]
    case = Case(F, F.MAP_OCCUPANCY, occupancy_map(F, patches, special))
    pose, pts = RY.sensor(*SENSOR), RY.lattice(beams)
    RY.assert_deltas(pose, pts, beams, "mixed wave")
    want = case.cast(pose, pts, "mixed wave")
    assert len(beams) == 64
    assert want.step[0, 0::4].tolist() == [0] * 16 and want.step[0, 1::4].tolist() == [1] * 16
    assert want.step[0, 2::4].tolist() == [19] * 16 and want.nn[0, 2::4].tolist() == [20] * 16 and want.step[0, 3::4].tolist() == [-1] * 16
    case.close()


# ------------------------------------------------------------------------------------------------ 4. a built map
FAN = (360, -math.pi, 2.0 * math.pi / 360.0, 12.0)
BUILT_POSES = [(0.3, -0.2, 0.4), (-1.0, 0.8, 2.0), (1.2, 0.9, -1.1)]


class BuiltRoom:
    """RC.BuiltMap with denser scans, so that the walls close: six posed scans of up to 1080 beams of a star-shaped room through
    the map rebuild, the occupied cells into the distance map"""

    def __init__(self, F):
        import _mapbuild as MB
        poses4, _, scans, origins, quats = MB.room_log(21, K=6, beams=1080, sensor=True)
        self.F = F
        self.ctx = F.HipContext(F.default_cfg(particles=1))
        self.mx = RC.max_sqdist_of(self.ctx.cfg)
        self.ctx.integrate_scans(0, poses4, scans, origins, quats, full=True, prune=True)
        self.ctx.add_obstacles(0, self.ctx.occupied_cells(0))
        self.occ = self.ctx.download_map(0, F.MAP_OCCUPANCY)
        self.dm = self.ctx.download_map(0, F.MAP_DISTANCE)

    def close(self):
        self.ctx.close()


def check_built_map(m):
    """a 360-beam fan of 12 m from three poses inside the room, on the occupancy map and on the distance map"""
    import _reference as R
    F, ctx = m.F, m.ctx
    pts = F.fan_points(*FAN)
    poses = np.stack([R.pose_from_xyr(*p) for p in BUILT_POSES])
    for kind, dump, distance in ((F.MAP_OCCUPANCY, m.occ, False), (F.MAP_DISTANCE, m.dm, True)):
        for su in ((False, True) if not distance else (False,)):
            want = RQ.expected(poses, pts, dump, distance, m.dm, m.mx, stop_unknown=su, tolerance=1)
            got = ctx.cast_rays(0, kind, poses, pts, stop_at_unknown=su, tolerance_cells=1, resolution=0.05)
            RQ.assert_equal(got, want, f"built map, kind {kind}, stop_unknown {su}")
            assert got.kernel_ms is not None and got.kernel_ms >= 0.0
            if su:
                assert (want.status == RQ.UNKNOWN).sum() >= 1
            else:
                assert (want.status == RQ.OCCUPIED).sum() * 4 >= want.status.size, (kind, (want.status == RQ.OCCUPIED).sum())
                assert (want.status == RQ.NONE).sum() >= 1
                assert np.isfinite(want.range).sum() == (want.status == RQ.OCCUPIED).sum() and want.range[np.isfinite(want.range)].max() <= 12.0 + 0.1


# ------------------------------------------------------------------------------------------------ 5. labels
def check_labels(F):
    """a wall along x = 37 (30 cells from the sensor) with the distance map a brushfire leaves beside it; beams that end on it, one
    and three cells short of it and three cells behind it"""
    wall_x, ys = SENSOR[0] + 30, range(-32, 64)
    patches = [(px, py) for px in (0, 1) for py in (-1, 0, 1)]
    occ = occupancy_map(F, patches, {(wall_x, y): OCC_CELL for y in ys})
    near = {}
    for dxy in range(-4, 5):
        for y in ys:
            near[(wall_x + dxy, y)] = (dxy * dxy, 1)
    dm = distance_map(F, patches, near, fill=(0, 0))           # elsewhere: no valid obstacle
    beams = [(30, 0), (29, 0), (27, 0), (33, 0), (30, 7), (29, 7), (27, 6), (33, 8)]
    pose, pts = RY.sensor(*SENSOR), RY.lattice(beams)
    RY.assert_deltas(pose, pts, beams, "labels")
    seen = set()
    for kind in (F.MAP_OCCUPANCY, F.MAP_DISTANCE):
        case = Case(F, kind, occ if kind == F.MAP_OCCUPANCY else dm, dm_patches=dm if kind == F.MAP_OCCUPANCY else None)
        for tol, labels in ((0, [RQ.AGREES, RQ.NOVEL, RQ.NOVEL, RQ.BLOCKED]), (1, [RQ.AGREES, RQ.AGREES, RQ.NOVEL, RQ.BLOCKED]), (3, [RQ.AGREES] * 4)):
            want = case.cast(pose, pts, f"labels, kind {kind}, tolerance {tol}", tolerance=tol)
            assert want.label[0, :4].tolist() == labels and want.label[0, 4:].tolist() == labels, (kind, tol, want.label)
            assert want.end_sqdist[0, :4].tolist() == [0, 1, 9, 9]
            seen |= set(want.label.ravel().tolist())
        none = case.cast(pose, pts, "no tolerance: no labels")
        assert none.label is None
        case.close()
    assert seen == {RQ.AGREES, RQ.BLOCKED, RQ.NOVEL}


# ------------------------------------------------------------------------------------------------ 6. limits
def raw_cast(ctx, particle, kind, poses4, pts, n, num_poses, flags=0, tolerance=-1, origin=None, quat=None, with_status=True):
    """the C call with every output prefilled -> (status code, True when every output is untouched)"""
    cap = 64
    outs = [np.full(cap, 0x5A, dtype=np.uint8), np.full(cap, 0x5A5A5A5A, dtype=np.int32), np.full(cap, 0x5A5A5A5A, dtype=np.uint32),
            np.full(2 * cap, 0x5A5A5A5A, dtype=np.uint32), np.full(cap, 0x5A5A5A5A, dtype=np.uint32), np.full(cap, 0x5A, dtype=np.uint8),
            np.full(2 * cap, 0x5A5A5A5A, dtype=np.uint32)]
    keep = [o.copy() for o in outs]
    p = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.c_void_p)
    ptr = [o.ctypes.data_as(C.c_void_p) for o in outs]
    rc = ctx.L.lama_hip_map_cast_rays(ctx.h, particle, kind, num_poses, p(poses4), p(pts), n, p(origin), p(quat), flags, tolerance,
                                      ptr[0] if with_status else None, ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], ptr[6], None)
    return rc, all(np.array_equal(a, b) for a, b in zip(outs, keep))


def check_limits(F):
    case = Case(F, F.MAP_OCCUPANCY, occupancy_map(F, [(0, 0)], {}))
    ctx, pose = case.ctx, RY.sensor(0, 0)
    for deltas in ([(RY.LONGEST, 0), (3, 4)], [(-4096, -RY.LONGEST)], [(100, 0, RY.LONGEST)]):
        d, nn = RY.assert_deltas(pose, RY.lattice(deltas), deltas, "longest beam")
        assert nn.max() == RY.LONGEST
        want = case.cast(pose, RY.lattice(deltas), f"a beam of 8191 steps {deltas[0]}")
        assert want.nn[0, 0] == 8191
    su = case.cast(pose, RY.lattice([(RY.LONGEST, 0)]), "a beam of 8191 steps, unknown cells stop", stop_unknown=True)
    assert su.step[0, 0] == 31 and su.status[0, 0] == RQ.UNKNOWN            # the free patch ends at x = 31
    for long_one in [(RY.LONGEST + 1, 0), (0, -(RY.LONGEST + 1)), (3, 0, RY.LONGEST + 1)]:
        deltas = [(3, 4), long_one]
        d, nn = RY.assert_deltas(pose, RY.lattice(deltas), deltas, "too long")
        assert nn.max() == RY.LONGEST + 1
        rc, untouched = raw_cast(ctx, 0, F.MAP_OCCUPANCY, pose, RY.lattice(deltas), 2, 1)
        assert rc == E_WINDOW and untouched and "8191" in ctx._error(), (long_one, rc, ctx._error())
    pts = RY.lattice([(3, 4), (5, 0)])
    nan, inf = float("nan"), float("inf")
    bad_pt = pts.copy(); bad_pt[1, 1] = nan
    inf_pt = pts.copy(); inf_pt[0, 2] = inf
    refusals = {
        "n == 0": dict(n=0), "num_poses == 0": dict(num_poses=0), "a NULL status": dict(with_status=False),
        "a NaN point": dict(pts=bad_pt), "an infinite point": dict(pts=inf_pt),
        "a NaN pose": dict(poses4=np.array([1.0, 0.0, nan, 0.0])), "an infinite pose": dict(poses4=np.array([1.0, 0.0, 0.0, -inf])),
        "a NaN mount origin": dict(origin=np.array([0.0, nan, 0.0])), "an infinite mount quaternion": dict(quat=np.array([1.0, 0.0, inf, 0.0])),
        "particle out of range": dict(particle=1), "kind 2": dict(kind=2), "kind -1": dict(kind=-1), "flag 2": dict(flags=2), "flag 3": dict(flags=3),
        "stop_unknown on the distance map": dict(kind=F.MAP_DISTANCE, flags=F.RAY_STOP_UNKNOWN),
        "2^31 beams": dict(num_poses=1 << 20, n=1 << 11), "2^31 beams the other way": dict(num_poses=1 << 31, n=1),
        "start cell above the 32-bit range": dict(poses4=np.array([1.0, 0.0, 1e9, 0.0])),
        "start cell below 0": dict(poses4=np.array([1.0, 0.0, 0.0, -3e6])),
        "hit cell above the 32-bit range": dict(pts=np.array([[3e8, 0.0, 0.0], [1.0, 0.0, 0.0]])),
    }
    for what, kw in refusals.items():
        a = dict(particle=0, kind=F.MAP_OCCUPANCY, poses4=pose, pts=pts, n=2, num_poses=1)
        a.update(kw)
        rc, untouched = raw_cast(ctx, **a)
        assert rc == E_INVALID and untouched, (what, rc, untouched)
    rc, untouched = raw_cast(ctx, 0, F.MAP_OCCUPANCY, pose, pts, 2, 1)              # the same call without a fault is served
    assert rc == 0 and not untouched
    rc, _ = raw_cast(ctx, 0, F.MAP_DISTANCE, pose, pts, 2, 1, tolerance=2)
    assert rc == 0
    case.close()


def check_scan_of_5000_points(F):
    """no 4096-point cap: 5000 beams, every one with the answer of its twin in a scan of 100"""
    case = Case(F, F.MAP_OCCUPANCY, _walled_room(F))
    deltas = RY.fan(100)
    pose = RY.sensor(*SENSOR)
    small = case.cast(pose, RY.lattice(deltas), "100 beams")
    got = case.ctx.cast_rays(0, F.MAP_OCCUPANCY, pose, RY.lattice(deltas * 50))
    for name in ("status", "step", "nn", "end_sqdist", "range"):
        assert np.array_equal(getattr(got, name)[0].reshape(50, 100), np.tile(getattr(small, name)[0], (50, 1))), name
    case.close()


def check_more_poses_than_a_grid_has_rows(F):
    """65,540 poses, five more than the y dimension of a grid holds: every pose with the answer of its twin among the four it repeats"""
    case = Case(F, F.MAP_OCCUPANCY, _walled_room(F))
    deltas = RY.fan(3)
    four = np.stack([RY.sensor(7, 9), RY.sensor(12, 9), RY.sensor(7, 30), RY.sensor(20, 1)])
    small = case.cast(four, RY.lattice(deltas), "four poses")
    assert len({tuple(r) for r in small.step.tolist()}) >= 3
    got = case.ctx.cast_rays(0, F.MAP_OCCUPANCY, np.tile(four, (16385, 1)), RY.lattice(deltas), tolerance_cells=1)
    assert got.status.shape == (65540, 3)
    for name in ("status", "step", "nn", "end_sqdist", "range", "cell_xy", "start_xy"):
        a, b = getattr(got, name), getattr(small, name)
        assert np.array_equal(a.reshape((16385,) + b.shape), np.broadcast_to(b, (16385,) + b.shape)), name
    case.close()
