"""The reference's map rebuild from posed key scans (GraphSlam2D::generateOccupancyMap, src/graph_slam2d.cpp:131-164) composed from
the compiled reference's own primitives (tests/_reference.py: Occ.set_occupied / set_free, DM.compute_ray / w2m), for the
MapBuilder2D tests.  Test infrastructure."""
import math

import numpy as np

import _reference as R
from _stress import random_room_scan

OFF = (2642244 >> 1) * 32          # Map's origin offset in cells (src/sdm/map.cpp:55-58)


def scan_tf(pose4, origin=None, quat=None):
    """tf = Translation(x, y, 0) * AngleAxis(pose.rotation(), Z) * Translation(sensor origin) * sensor orientation, in the operation
    order of Eigen's products (the order the device library's host side uses for every map update): (R 3x3, t 3)."""
    w, x, y, z = (1.0, 0.0, 0.0, 0.0) if quat is None else [float(v) for v in quat]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    M = [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]
    mt = [0.0, 0.0, 0.0] if origin is None else [float(v) for v in origin]
    theta = math.atan2(float(pose4[1]), float(pose4[0]))
    sn, cs = math.sin(theta), math.cos(theta)
    Fm = [[cs, 0.0 - sn, 0.0], [sn, cs, 0.0], [0.0, 0.0, (1.0 - cs) + cs]]
    ft = [float(pose4[2]), float(pose4[3]), 0.0]
    Rm = [[(Fm[i][0] * M[0][j] + Fm[i][1] * M[1][j]) + Fm[i][2] * M[2][j] for j in range(3)] for i in range(3)]
    t = [((Fm[i][0] * mt[0] + Fm[i][1] * mt[1]) + Fm[i][2] * mt[2]) + ft[i] for i in range(3)]
    return Rm, t


def integrate(occ, grid, poses4, scans, origins=None, quats=None, full=True):
    """The loop body of generateOccupancyMap for every (pose, scan) on the reference map `occ`; `grid` is a reference map of the
    same resolution whose w2m / computeRay are used (they are Map's, the same for every map class)."""
    for k, pts in enumerate(scans):
        Rm, t = scan_tf(poses4[k], None if origins is None else origins[k], None if quats is None else quats[k])
        so = grid.w2m(t)
        for p in np.asarray(pts, dtype=np.float64).reshape(-1, 3):
            px, py, pz = float(p[0]), float(p[1]), float(p[2])
            hit = [((Rm[i][0] * px + Rm[i][1] * py) + Rm[i][2] * pz) + t[i] for i in range(3)]
            mh = grid.w2m(hit)
            occ.set_occupied(int(mh[0]), int(mh[1]), int(mh[2]))
            if full:
                for c in grid.compute_ray(so, mh):
                    occ.set_free(int(c[0]), int(c[1]), int(c[2]))


def build(poses4, scans, origins=None, quats=None, full=True, resolution=0.05):
    occ = R.Occ.new(resolution)
    integrate(occ, R.DM.new(resolution), poses4, scans, origins, quats, full)
    return occ


def pruned(dump):
    """FrequencyOccupancyMap::prune (src/sdm/frequency_occupancy_map.cpp:149-158) applied to a dump {id: (cells, mask)}: a masked cell
    with visited == 1 and occupied <= 1 becomes {0, 0}; masks and patches stay."""
    out = {}
    for pid, (cells, mask) in dump.items():
        cells = cells.copy()
        bits = ((mask[np.arange(1024) >> 6] >> (np.arange(1024) & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
        cut = bits & (cells["visited"] == 1) & (cells["occupied"] <= 1)
        cells["occupied"][cut] = 0
        cells["visited"][cut] = 0
        out[pid] = (cells, mask.copy())
    return out


def occupied_cells(dump):
    """The occupied cells of a dump in Map::visit_all_cells order (ascending patch index, then cell index; masked cells only) with
    isOccupied = visited != 0 and occupied / visited > 0.25 in double (src/sdm/frequency_occupancy_map.cpp:38-45,132-138)."""
    out = []
    for pid in sorted(dump):
        cells, mask = dump[pid]
        ax, ay = (pid // 2642244) * 32, (pid % 2642244) * 32
        ci = np.arange(1024)
        bits = ((mask[ci >> 6] >> (ci & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
        vis = cells["visited"].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            occd = bits & (cells["visited"] != 0) & (cells["occupied"].astype(np.float64) / vis > 0.25)
        for c in ci[occd]:
            out.append((ax + (c & 31), ay + (c >> 5)))
    return np.array(out, dtype=np.uint32).reshape(-1, 2)


def distance_map_of(cells_xy, l2_max, resolution=0.05):
    """The reference DynamicDistanceMap fed addObstacle for every listed cell, then update()."""
    dm = R.DM.new(resolution, 32, l2_max)
    for x, y in cells_xy:
        dm.add(int(x), int(y))
    dm.update()
    return dm


def room_log(seed, K=40, beams=120, sensor=False):
    """K posed scans of a random star-shaped room (tests/_stress.py): poses4 (K, 4), xyr (K, 3), scans, origins, quats (None unless
    `sensor`: then every scan has its own non-identity sensor origin and orientation, a yaw about z)."""
    rng = np.random.default_rng(4000 + seed)
    kind = {"R": rng.uniform(3.0, 7.0), "coef": [(m, rng.uniform(0.02, 0.12), rng.uniform(0, 2 * np.pi)) for m in (2, 3, 5, 7)]}
    xyr = np.stack([rng.uniform(-0.35, 0.35, K) * kind["R"], rng.uniform(-0.35, 0.35, K) * kind["R"], rng.uniform(-np.pi, np.pi, K)], axis=1)
    origins = quats = None
    if sensor:
        origins = np.stack([rng.uniform(-0.2, 0.2, K), rng.uniform(-0.2, 0.2, K), np.zeros(K)], axis=1)
        a = rng.uniform(-0.5, 0.5, K)
        quats = np.stack([np.cos(a / 2), np.zeros(K), np.zeros(K), np.sin(a / 2)], axis=1)
    scans = []
    for k in range(K):
        sx, sy, syaw = xyr[k]
        if sensor:      # where the sensor really is: pose * (origin, yaw)
            c, s = math.cos(syaw), math.sin(syaw)
            sx, sy, syaw = sx + c * origins[k, 0] - s * origins[k, 1], sy + s * origins[k, 0] + c * origins[k, 1], syaw + a[k]
        n = int(rng.integers(beams // 2, beams + 1))
        scans.append(random_room_scan(rng, (sx, sy, syaw), n, kind))
    poses4 = np.stack([R.pose_from_xyr(*p) for p in xyr])
    return poses4, xyr, scans, origins, quats
