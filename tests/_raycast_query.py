"""What lama_hip_map_cast_rays must return, restated in numpy from maps in the record format of HipContext.download_map -- test
infrastructure: nothing here calls the code under test.  Start / hit cells: _ray_checks.geometry (PFSlam2D::updateParticleMaps'
transform in the reference's operation order, the reference's w2m).  The sequence of a beam: _ray_checks.ray_cells (the compiled
reference's Map::computeRay, the oracle's where it is absent) followed by the hit cell.  Cell classes: _raster.cell_values (the
reference's isOccupied / isFree in double, the log-odds rule, the distance rule, each behind Map::get)."""
import numpy as np

import _raster as RS
import _ray_checks as RY

NONE, OCCUPIED, UNKNOWN = 0, 1, 2          # status
AGREES, BLOCKED, NOVEL = 0, 1, 2           # label
FREE = 3                                   # a class of its own here; the device reports a free cell by passing it


class Expected:
    def __init__(self, K, n):
        self.status = np.zeros((K, n), dtype=np.uint8)
        self.step = np.full((K, n), -1, dtype=np.int32)
        self.nn = np.zeros((K, n), dtype=np.uint32)
        self.cell_xy = np.zeros((K, n, 2), dtype=np.uint32)
        self.end_sqdist = np.zeros((K, n), dtype=np.uint32)
        self.label = None
        self.start_xy = np.zeros((K, 2), dtype=np.uint32)
        self.range = np.full((K, n), np.inf)
        self.stop_class = np.zeros((K, n), dtype=np.uint8)       # the class of the stopping cell (0: none stopped the ray)


class CellClasses:
    """class of a map cell: OCCUPIED, FREE or UNKNOWN (a cell of an absent patch -- outside the window there is none -- is unknown)"""

    def __init__(self, dump, distance, policy=0, max_sqdist=None):
        self.distance = distance
        self.v = RS.cell_values(dump, RS.SQDIST if distance else RS.TRINARY, policy, max_sqdist)

    def of(self, x, y):
        v = self.v.get(RS.patch_id(int(x) >> 5, int(y) >> 5))
        if v is None:
            return UNKNOWN
        c = int(v[int(y) & 31, int(x) & 31])
        if self.distance:                                         # present, valid_obstacle and a squared distance of 0 (max_sqdist > 0)
            return OCCUPIED if c == 0 else FREE
        return OCCUPIED if c == 100 else (FREE if c == 0 else UNKNOWN)


def sequence(start, hit):
    """the cells a beam is tested on: Map::computeRay(start, hit) in order, then the hit cell; none for start == hit"""
    nn = int(np.abs(hit - start).max())
    if nn == 0:
        return np.zeros((0, 2), dtype=np.int64)
    ray = RY.ray_cells(start, hit)
    assert len(ray) == nn - 1, (start, hit, len(ray))
    return np.concatenate([ray[:, :2], hit[None, :2]]).astype(np.int64)


def expected(poses4, pts, dump, distance, dm_dump, max_sqdist, resolution=RY.RES, origin=None, quat=None, policy=0, stop_unknown=False, tolerance=-1):
    """-> Expected for the map `dump` (an occupancy dump, or with distance=True a distance dump); dm_dump: the particle's distance
    map for end_sqdist ({} / None: the context has none)"""
    poses4 = np.asarray(poses4, dtype=np.float64).reshape(-1, 4)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    cls = CellClasses(dump, distance, policy, max_sqdist)
    sq = RS.cell_values(dm_dump or {}, RS.SQDIST, 0, max_sqdist)
    e = Expected(len(poses4), len(pts))
    if tolerance >= 0:
        e.label = np.zeros(e.status.shape, dtype=np.uint8)
    for k, pose in enumerate(poses4):
        d, nn, _, starts = RY.geometry(pose, pts, origin, quat)
        e.start_xy[k] = starts[0][:2]
        for i in range(len(pts)):
            start, hit = starts[i], starts[i] + d[i]
            seq = sequence(start, hit)
            e.nn[k, i] = len(seq)
            e.cell_xy[k, i] = hit[:2]
            for s, (x, y) in enumerate(seq):
                c = cls.of(x, y)
                if c == OCCUPIED or (c == UNKNOWN and stop_unknown):
                    e.status[k, i], e.step[k, i], e.cell_xy[k, i], e.stop_class[k, i] = c, s, (x, y), c
                    dx, dy = int(x) - int(start[0]), int(y) - int(start[1])
                    e.range[k, i] = resolution * np.sqrt(np.float64(dx * dx + dy * dy))
                    break
            v = sq.get(RS.patch_id(int(hit[0]) >> 5, int(hit[1]) >> 5))
            e.end_sqdist[k, i] = max_sqdist if v is None else int(v[int(hit[1]) & 31, int(hit[0]) & 31])
            if tolerance >= 0:
                blocked = e.status[k, i] == OCCUPIED and int(e.nn[k, i]) - 1 - int(e.step[k, i]) > tolerance
                e.label[k, i] = BLOCKED if blocked else (AGREES if int(e.end_sqdist[k, i]) <= tolerance * tolerance else NOVEL)
    return e


def assert_equal(got, want, what):
    """array_equal on status, step, nn, cell, end_sqdist, label, start cell and range: no tolerance anywhere"""
    for name in ("status", "step", "nn", "cell_xy", "end_sqdist", "start_xy", "label", "range"):
        g, w = getattr(got, name), getattr(want, name)
        if w is None:
            assert g is None, (what, name)
            continue
        assert g is not None and g.dtype == w.dtype and g.shape == w.shape, (what, name, None if g is None else (g.dtype, g.shape), (w.dtype, w.shape))
        assert np.array_equal(g, w), f"{what}: {name} differs at {np.argwhere(g != w)[:4].tolist()}: got {g[g != w][:4].tolist()}, want {w[g != w][:4].tolist()}"
