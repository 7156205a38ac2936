"""Checks of k_search_lattice / lama_hip_match_search_lattice (iris_lama_amd/csrc/lama_correlative.h) and of lama::CorrelativeSearch2D /
Loc2D::relocalize, shared by tests/test_correlative_sim.py (the lane simulator, no GPU) and tests/test_correlative_gpu.py.

The kernel checks have NO tolerance: a node's score is a sum of the squared cell distances the map stores, added as integers, and
the cell of every point comes from a transform that the library composes on the host -- so the numpy restatement below (the oracle's
scan transform and w2m for the cells, the oracle map's dump for the lookup) is the device's result bit for bit, in the simulator and
on the device, at every heading.
"""
import ctypes as C
import math

import numpy as np

import _match_batch_checks as MB
import _match_checks as M
import _oracle as O

PATCH_STRIDE = 2642244          # Map::m2p: patch id = px * stride + py
E_INVALID = -1
HEADINGS3 = (0.0, 0.12, 2.5)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
class Dense:
    """The squared-distance lookup of an oracle distance map as one array over the box of its patches: sqdist where valid_obstacle is
    set, max_sqdist everywhere else (and outside the box); `present` marks the cells that lie in a patch of the map at all."""

    def __init__(self, dm, maxsq=None):
        """dm: an oracle distance map, or a dump {patch id: (cells, mask)} with its max_sqdist"""
        dump = dm if isinstance(dm, dict) else dm.dump()
        self.maxsq = int(dm.max_sqdist() if maxsq is None else maxsq)
        px = np.array([pid // PATCH_STRIDE for pid in dump], dtype=np.int64)
        py = np.array([pid % PATCH_STRIDE for pid in dump], dtype=np.int64)
        self.x0, self.y0 = int(px.min()) * 32, int(py.min()) * 32
        self.x1, self.y1 = (int(px.max()) + 1) * 32, (int(py.max()) + 1) * 32          # (exclusive)
        self.q = np.full((self.y1 - self.y0, self.x1 - self.x0), self.maxsq, dtype=np.uint32)
        self.present = np.zeros(self.q.shape, dtype=bool)
        for pid, (cells, _) in dump.items():
            ax, ay = (pid // PATCH_STRIDE) * 32 - self.x0, (pid % PATCH_STRIDE) * 32 - self.y0
            v = np.where(cells["valid"] != 0, cells["sqdist"].astype(np.uint32), np.uint32(self.maxsq)).reshape(32, 32)   # [y][x]
            self.q[ay:ay + 32, ax:ax + 32] = v
            self.present[ay:ay + 32, ax:ax + 32] = True

    def lookup(self, x, y):
        """x, y: int64 arrays of map cell coordinates -> (q uint32, in a patch of the map)"""
        inside = (x >= self.x0) & (x < self.x1) & (y >= self.y0) & (y < self.y1)
        xi, yi = np.where(inside, x - self.x0, 0), np.where(inside, y - self.y0, 0)
        return np.where(inside, self.q[yi, xi], np.uint32(self.maxsq)).astype(np.uint32), inside & self.present[yi, xi]


def scan_tf(pose4, origin, quat):
    out = np.zeros(12)
    O.lib().orc_scan_tf(O._p(np.ascontiguousarray(pose4, dtype=np.float64)), O._p(np.ascontiguousarray(origin, dtype=np.float64)),
                        O._p(np.ascontiguousarray(quat, dtype=np.float64)), O._p(out))
    return out


def point_cells(pts, cs, wx0, wy0, origin, quat, res=0.05):
    """the cells of the given points at pose {c, s, wx0, wy0}: the oracle's scan transform, hit = (R p) + t in MatchSurface2D's order, w2m"""
    t = scan_tf([cs[0], cs[1], wx0, wy0], origin, quat)
    out = np.zeros((len(pts), 2), dtype=np.int64)
    for i, p in enumerate(pts):
        px, py, pz = float(p[0]), float(p[1]), float(p[2])
        hx = ((t[0] * px + t[1] * py) + t[2] * pz) + t[9]
        hy = ((t[3] * px + t[4] * py) + t[5] * pz) + t[10]
        c = O.w2m([hx, hy, 0.0], res=res)
        out[i] = (int(c[0]), int(c[1]))
    return out


def headings_cs(angles):
    return np.array([[math.cos(a), math.sin(a)] for a in angles])


def restate(dense, pts, cs, wx0, wy0, cell_step, nx, ny, tile, point_step=1, origin=O.ZERO3, quat=O.IDENT_Q, res=0.05):
    """-> (best (H, TY, TX) uint64, scores (H, ny, nx) uint32, absent (H, ny, nx): terms of the node that fall in no patch of the map,
    cells [H] of the used points)"""
    used = np.ascontiguousarray(pts, dtype=np.float64)[::point_step]
    H = len(cs)
    assert len(used) * dense.maxsq < 2 ** 32
    scores = np.zeros((H, ny, nx), dtype=np.uint32)
    absent = np.zeros((H, ny, nx), dtype=np.int64)
    dx = (cell_step * np.arange(nx, dtype=np.int64))[None, :, None]
    dy = (cell_step * np.arange(ny, dtype=np.int64))[:, None, None]
    all_cells = []
    for h in range(H):
        cells = point_cells(used, cs[h], wx0, wy0, origin, quat, res)
        all_cells.append(cells)
        x = np.broadcast_to(cells[None, None, :, 0] + dx, (ny, nx, len(cells)))
        y = np.broadcast_to(cells[None, None, :, 1] + dy, (ny, nx, len(cells)))
        q, present = dense.lookup(x, y)
        scores[h] = q.sum(axis=2, dtype=np.uint64).astype(np.uint32)
        absent[h] = (~present).sum(axis=2)
    return tile_keys(scores, tile), scores, absent, all_cells


def tile_keys(scores, tile):
    H, ny, nx = scores.shape
    index = np.arange(H * ny * nx, dtype=np.uint64).reshape(H, ny, nx)
    keys = (scores.astype(np.uint64) << np.uint64(32)) | index
    TY, TX = (ny + tile - 1) // tile, (nx + tile - 1) // tile
    best = np.zeros((H, TY, TX), dtype=np.uint64)
    for ty in range(TY):
        for tx in range(TX):
            best[:, ty, tx] = keys[:, ty * tile:(ty + 1) * tile, tx * tile:(tx + 1) * tile].reshape(H, -1).min(axis=1)
    return best


def assert_lattice(ctx, dense, pts, angles, wx0, wy0, cell_step, nx, ny, tile, point_step=1, origin=O.ZERO3, quat=O.IDENT_Q, particle=0, what=""):
    """one call against the restatement: scores and keys, exactly; the keys alone (scores_out NULL) are the same keys"""
    cs = headings_cs(angles)
    best, scores = ctx.search_lattice(particle, pts, cs, wx0, wy0, cell_step, nx, ny, tile=tile, point_step=point_step, origin=origin, quat=quat)
    wbest, wscores, absent, _ = restate(dense, pts, cs, wx0, wy0, cell_step, nx, ny, tile, point_step, origin, quat, res=ctx.cfg.resolution)
    assert np.array_equal(scores, wscores), (what, "scores", int((scores != wscores).sum()), np.argwhere(scores != wscores)[:4])
    assert np.array_equal(best, wbest), (what, "keys", np.argwhere(best != wbest)[:4])
    best2, none = ctx.search_lattice(particle, pts, cs, wx0, wy0, cell_step, nx, ny, tile=tile, point_step=point_step, origin=origin, quat=quat, scores=False)
    assert none is None and np.array_equal(best2, wbest), (what, "keys without scores")
    return wbest, wscores, absent


# ---------------------------------------------------------------------------------------------------------------------
# kernel checks
# ---------------------------------------------------------------------------------------------------------------------
def check_point_slicing(ctx, dm):
    """n in {1, 63, 64, 65, 257} x point_step in {1, 3, n}: 3 headings, lattice 9 x 7, cell_step 1, tile 4 (partial tiles on both
    edges, a one-node tile in the corner, the last wave's partial chunk); a mounted sensor once"""
    dense = Dense(dm)
    x, y, _ = M.SCAN_POSE
    for n in (1, 63, 64, 65, 257):
        pts = M.scan_of(n)
        for step in sorted({1, 3, n}):
            assert_lattice(ctx, dense, pts, HEADINGS3, x - 0.2, y - 0.15, 1, 9, 7, 4, point_step=step, what=("slicing", n, step))
    pts, origin, quat = M.mounted_scan(65, M.MOUNTS["offset"])
    assert_lattice(ctx, dense, pts, HEADINGS3, x - 0.2, y - 0.15, 1, 9, 7, 4, point_step=3, origin=origin, quat=quat, what="mounted")


def check_stride_and_tiles(ctx, dm):
    dense = Dense(dm)
    x, y, _ = M.SCAN_POSE
    pts = M.scan_of(65)
    for cell_step in (1, 4):
        for tile in (1, 8):
            assert_lattice(ctx, dense, pts, HEADINGS3[:2], x - 0.3, y - 0.3, cell_step, 11, 9, tile, what=("stride", cell_step, tile))
    assert_lattice(ctx, dense, pts, HEADINGS3, x, y, 3, 1, 1, 8, what="one node")
    assert_lattice(ctx, dense, pts, HEADINGS3[:1], x - 0.4, y - 0.2, 2, 16, 5, 8, what="nx a multiple of the tile")
    assert_lattice(ctx, dense, pts, HEADINGS3[1:2], x - 0.4, y - 0.2, 1, 12, 6, 3, what="tile 3 (rows of a tile do not fill a lane group)")


def check_absent_and_window(ctx, dm):
    """cells in no patch, beyond the window on the high side, and below its origin (the unsigned wrap of the window test).  The window
    of a context holds its whole map and is `window_patches` patches wide, so a cell more than that far above the map's lowest patch
    (below its highest) is outside it wherever it was placed."""
    dense = Dense(dm)
    WC = 32 * int(ctx.counters()["window_patches"])
    pts = M.scan_of(65)
    bx, by = M.BLOB
    _, _, absent = assert_lattice(ctx, dense, pts, HEADINGS3, bx - 1.0, by - 1.0, 4, 10, 10, 8, what="blob")
    assert absent.max() > 0 and (dense.present.sum() < dense.present.size)
    # high side: node columns 512 cells apart, the last ones beyond any window that holds the map
    cs = headings_cs(HEADINGS3[:2])
    _, _, absent, cells = restate(dense, pts, cs, 1.0, 1.0, 512, 12, 3, 4)
    assert max(int(c[:, 0].max()) for c in cells) + 512 * 11 > dense.x0 + WC
    assert_lattice(ctx, dense, pts, HEADINGS3[:2], 1.0, 1.0, 512, 12, 3, 4, what="past the window, high side")
    _, _, absent, cells = restate(dense, pts, cs, 1.0, 1.0, 700, 2, 9, 4)
    assert max(int(c[:, 1].max()) for c in cells) + 700 * 8 > dense.y0 + WC
    assert_lattice(ctx, dense, pts, HEADINGS3[:2], 1.0, 1.0, 700, 2, 9, 4, what="past the window, high side (y)")
    # low side: the lattice starts more than a window below the map's highest patch; its node (7, 7) is the pose the scan was taken at
    sx, sy, syaw = M.SCAN_POSE
    assert syaw == HEADINGS3[1]
    wx, wy = sx - 7 * 600 * 0.05, sy - 7 * 600 * 0.05
    _, wscores, absent, cells = restate(dense, pts, cs, wx, wy, 600, 9, 9, 4)
    assert min(int(c[:, 0].min()) for c in cells) < dense.x1 - WC and min(int(c[:, 1].min()) for c in cells) < dense.y1 - WC
    assert absent[:, 0, 0].min() == len(pts)
    assert wscores[1, 7, 7] < len(pts) * dense.maxsq // 4        # (and the far nodes of that lattice do reach the map)
    assert_lattice(ctx, dense, pts, HEADINGS3[:2], wx, wy, 600, 9, 9, 4, what="below the window")


def O_OFF():
    return int(O.w2m([0.0, 0.0, 0.0])[0])


def check_ties(F):
    """every score equal over empty space: each tile's key is its smallest index; two equal obstacles tile * cell_step cells apart:
    equal minima in different tiles"""
    tile, cell_step = 4, 2
    c0 = O.w2m([2.0, 2.0, 0.0])
    cells = np.array([[int(c0[0]), int(c0[1])], [int(c0[0]) + tile * cell_step, int(c0[1])]], dtype=np.uint32)
    dm = O.DM.new(l2_max=1.0)
    for x, y in cells:
        dm.add(int(x), int(y))
    dm.update()
    ctx = F.HipContext(F.default_cfg(particles=1, l2_max=1.0))
    try:
        ctx.add_obstacles(0, cells)
        dense = Dense(dm)
        pts = np.array([[0.0, 0.0, 0.0], [0.3, 0.0, 0.0], [0.0, 0.35, 0.0]])
        # empty space: 40 m away
        best, scores, _ = assert_lattice(ctx, dense, pts, HEADINGS3, 42.0, 41.0, cell_step, 9, 7, tile, what="empty")
        assert np.all(scores == len(pts) * dense.maxsq)
        H, ny, nx = scores.shape
        for h in range(H):
            for ty in range(best.shape[1]):
                for tx in range(best.shape[2]):
                    assert int(best[h, ty, tx]) & 0xFFFFFFFF == (h * ny + ty * tile) * nx + tx * tile
        # a single point: its score over the lattice is the map itself, so the two obstacles give two zeros a tile apart
        one = np.array([[0.0, 0.0, 0.0]])
        wx, wy = 2.0 - 0.05 * cell_step * 1, 2.0 - 0.05 * cell_step * 2
        best, scores, _ = assert_lattice(ctx, dense, one, (0.0,), wx, wy, cell_step, 2 * tile, tile, tile, what="two obstacles")
        assert best.shape == (1, 1, 2) and int(best[0, 0, 0]) >> 32 == 0 and int(best[0, 0, 1]) >> 32 == 0
        assert (int(best[0, 0, 1]) & 0xFFFFFFFF) - (int(best[0, 0, 0]) & 0xFFFFFFFF) == tile
    finally:
        ctx.close()


def check_maps_per_particle(F):
    ctx, dms = MB.two_map_context(F)
    try:
        pts = M.scan_of(65)
        x, y, _ = M.SCAN_POSE
        before = [ctx.map_checksums(k).copy() for k in (F.MAP_DISTANCE, F.MAP_OCCUPANCY)]
        poses = ctx.get_poses().copy()
        got = []
        for p in range(2):
            _, s, _ = assert_lattice(ctx, Dense(dms[p]), pts, HEADINGS3, x - 0.3, y - 0.2, 2, 9, 7, 4, particle=p, what=("particle", p))
            got.append(s)
        assert not np.array_equal(got[0], got[1])
        after = [ctx.map_checksums(k) for k in (F.MAP_DISTANCE, F.MAP_OCCUPANCY)]
        for a, b in zip(before, after):
            assert np.array_equal(a, b), "a map changed"
        assert np.array_equal(poses, ctx.get_poses()), "a pose changed"
    finally:
        ctx.close()


def check_refusals(F, ctx, dm):
    """every LAMA_HIP_E_INVALID case: outputs untouched; the context works afterwards"""
    pts = np.ascontiguousarray(M.scan_of(12))
    cs = headings_cs(HEADINGS3)
    maxsq = int(dm.max_sqdist())
    base = dict(particle=0, pts=pts, n=len(pts), origin=np.zeros(3), quat=np.array([1.0, 0.0, 0.0, 0.0]), step=1, cs=cs, H=3, wx0=1.0, wy0=1.5,
                cell_step=2, nx=5, ny=4, tile=4)
    SENT64, SENT32 = np.uint64(0x1234567890ABCDEF), np.uint32(0xA5A5A5A5)

    def call(**kw):
        a = dict(base, **kw)
        best = np.full(4096, SENT64, dtype=np.uint64)
        scores = np.full(4096, SENT32, dtype=np.uint32)
        rc = ctx.L.lama_hip_match_search_lattice(ctx.h, a["particle"], F._p(a["pts"]), a["n"], F._p(a["origin"]), F._p(a["quat"]), a["step"], F._p(a["cs"]),
                                                 a["H"], C.c_double(a["wx0"]), C.c_double(a["wy0"]), a["cell_step"], a["nx"], a["ny"], a["tile"],
                                                 F._p(best), F._p(scores))
        return rc, bool(np.all(best == SENT64) and np.all(scores == SENT32))

    assert call() == (0, False)
    bad_pts = pts.copy(); bad_pts[7, 1] = np.inf
    nan_pts = pts.copy(); nan_pts[11, 2] = np.nan
    bad_cs = cs.copy(); bad_cs[2, 0] = np.nan
    cases = {
        "n == 0": dict(n=0),
        "point_step == 0": dict(step=0),
        "no heading": dict(H=0),
        "nx == 0": dict(nx=0), "ny == 0": dict(ny=0), "cell_step == 0": dict(cell_step=0), "tile == 0": dict(tile=0),
        "tile above the workgroup's nodes": dict(tile=9),
        "tile whose square wraps": dict(tile=65536),
        "non-finite point": dict(pts=bad_pts), "NaN point": dict(pts=nan_pts),
        "non-finite mount origin": dict(origin=np.array([0.0, np.inf, 0.0])),
        "non-finite mount orientation": dict(quat=np.array([1.0, 0.0, np.nan, 0.0])),
        "non-finite heading": dict(cs=bad_cs),
        "non-finite origin x": dict(wx0=float("inf")), "non-finite origin y": dict(wy0=float("nan")),
        "particle out of range": dict(particle=1),
        "H nx ny >= 2^32": dict(nx=65536, ny=21846, cell_step=1),          # 3 * 65536 * 21846 = 2^32 + 2 * 65536
        "nx ny >= 2^32": dict(H=1, nx=65536, ny=65536, cell_step=1),
        "far corner wraps the cell coordinates": dict(cell_step=2 ** 31, nx=3, ny=1, H=1),
        "far corner wraps the cell coordinates (y)": dict(cell_step=65536, nx=1, ny=65536, H=1),
        "origin below cell 0": dict(wx0=-3.0e6),
        "origin above cell 2^32": dict(wy0=2.2e8),
    }
    for name, kw in cases.items():
        assert call(**kw) == (E_INVALID, True), name
    # the context is as usable as before
    assert_lattice(ctx, Dense(dm), pts, HEADINGS3, 1.0, 1.5, 2, 5, 4, 4, what="after the refusals")


def check_wide(F):
    ctx, dm = M.build_world(F, 7.0, half_len=4.0)
    try:
        assert F.needs_wide(7.0, 0.05) and ctx.L is F.hip_lib(wide=True)
        x, y, _ = M.SCAN_POSE
        _, scores, _ = assert_lattice(ctx, Dense(dm), M.scan_of(65), HEADINGS3, x - 0.4, y - 0.4, 3, 9, 7, 4, point_step=2, what="wide")
        assert scores.max() > 0x3FFF                                # (sums of squared distances the 14-bit plane could not even store once)
        # a score must fit 32 bits: ceil(n / point_step) * max_sqdist >= 2^32 is refused, the same scan thinned is not (the wide map's
        # max_sqdist of 140^2 makes the smallest such scan 219,131 points)
        maxsq = int(dm.max_sqdist())
        big = np.ascontiguousarray(np.tile(M.scan_of(12), ((2 ** 32 // maxsq) // 12 + 1, 1)))
        assert len(big) * maxsq >= 2 ** 32 and (len(big) - 12) * maxsq < 2 ** 32
        cs = headings_cs((0.12,))
        for step, want in ((1, E_INVALID), (2, 0)):
            best, sc = np.full(1, 7, dtype=np.uint64), np.full(1, 7, dtype=np.uint32)
            rc = ctx.L.lama_hip_match_search_lattice(ctx.h, 0, F._p(big), len(big), None, None, step, F._p(cs), 1, C.c_double(x), C.c_double(y), 1, 1, 1, 1,
                                                     F._p(best), F._p(sc))
            assert rc == want and (best[0] == 7 and sc[0] == 7) == (want != 0), (step, rc)
    finally:
        ctx.close()


def check_more_workgroups_than_the_chip(ctx, dm):
    """160 x 160 x 4 headings, tile 8: 1600 workgroups, 102,400 scores"""
    x, y, _ = M.SCAN_POSE
    angles = (0.0, 0.12, 2.5, -1.3)
    best, scores, _ = assert_lattice(ctx, Dense(dm), M.scan_of(65), angles, x - 4.0, y - 4.0, 1, 160, 160, 8, what="1600 workgroups")
    assert best.size == 1600 and scores.size == 102400


# ---------------------------------------------------------------------------------------------------------------------
# lama::CorrelativeSearch2D and Loc2D::relocalize through the ffi wrappers
# ---------------------------------------------------------------------------------------------------------------------
# The world: hall_segments(10 m, 2 x 2 bays, 2 m openings) -- every bay has its pillar at (0.3, 0.7) of the bay, so no rotation or
# reflection of the hall maps it onto itself.  The map is built from MAP_POSES, the query scan is taken at TRUE_POSE, which is none
# of them.  The lattice is coarse (0.4 m, 15 degrees, every second point) so that the simulator scores it in seconds; whether the
# best node of such a lattice lies in the solver's basin is a property of world and pose: check_class asserts it of the restatement
# refined by the ORACLE's solver before it asserts it of the device.
HALL = dict(side=10.0, rooms=2, gap=2.0)
MAP_POSES = [(2.5, 2.5, 0.0), (2.5, 2.5, 2.0), (7.5, 2.5, 1.0), (7.5, 7.5, 3.0), (2.5, 7.5, -1.5), (5.0, 2.5, -2.5)]
TRUE_POSE = (8.1, 1.9, 0.7)
SEARCH = dict(linear_step=0.4, angular_step=math.radians(15.0), point_step=2, tile=4, max_candidates=6)
BEAMS = 240


def hall_scan(pose, beams=BEAMS):
    from _worlds import hall_segments, segment_world_scan
    return segment_world_scan(hall_segments(**HALL), *pose, beams=beams, max_range=12.0)


def slam_with_hall(F):
    """a lama::Slam2D that mapped the hall from MAP_POSES (odometry = the true poses)"""
    h = F.Slam2D()
    h.set_pose(*MAP_POSES[0])
    for k, pose in enumerate(MAP_POSES):
        h.update(hall_scan(pose), pose, float(k))
    return h


def lattice_of(resolution, n, box_min, box_max, linear_step, angular_step, point_step, tile, **_):
    """CorrelativeSearch2D::lattice, restated"""
    cell_step = int(max(1.0, round(linear_step / resolution)))
    H = int(max(1.0, round(2.0 * math.pi / angular_step)))
    node = cell_step * resolution
    nx = int(math.floor((box_max[0] - box_min[0]) / node)) + 1
    ny = int(math.floor((box_max[1] - box_min[1]) / node)) + 1
    return dict(cell_step=cell_step, nx=nx, ny=ny, headings=H, point_step=point_step if point_step else max(n // 256, 1), tile=tile)


def lattice_angles(H):
    return [-math.pi + h * (2.0 * math.pi / H) for h in range(H)]


def select(best, lat, max_candidates, keep=None):
    """the selection rule on the tile keys: ascending; take a key unless a taken one is within one tile in x and y and within one
    heading, circularly -> [(score, h, ix, iy)]"""
    H, nx, ny, tile = lat["headings"], lat["nx"], lat["ny"], lat["tile"]
    taken = []
    for key in np.sort(best.reshape(-1)):
        if len(taken) >= max_candidates:
            break
        key = int(key)
        score, index = key >> 32, key & 0xFFFFFFFF
        h, iy, ix = index // (nx * ny), (index // nx) % ny, index % nx
        if keep is not None and not keep(ix, iy):
            continue
        if any(abs(ix // tile - t[2] // tile) <= 1 and abs(iy // tile - t[3] // tile) <= 1 and min(abs(h - t[1]), H - abs(h - t[1])) <= 1 for t in taken):
            continue
        taken.append((score, h, ix, iy))
    return taken


def coarse_poses(taken, lat, box_min, resolution):
    node = lat["cell_step"] * resolution
    ang = lattice_angles(lat["headings"])
    return np.array([[math.cos(ang[h]), math.sin(ang[h]), box_min[0] + ix * node, box_min[1] + iy * node] for _, h, ix, iy in taken]).reshape(-1, 4)


def oracle_map_of(F, ctx, maxsq, tmp_path, l2_max):
    """the device's distance map as an oracle map (through a .sdm file, like tests/test_sdm_io.py)"""
    f = str(tmp_path / "correlative_dm.sdm")
    dump = ctx.download_map(0, F.MAP_DISTANCE)
    F.sdm_write(f, dump, F.MAP_DISTANCE, 0.05, maxsq)
    dm = O.DM.new(0.05, 32, l2_max)
    assert dm.read(f) and dm.max_sqdist() == maxsq
    return dm, dump


def within_one_step(pose4, truth, linear_step, angular_step):
    dth = math.atan2(pose4[1], pose4[0]) - truth[2]
    dth = abs(math.atan2(math.sin(dth), math.cos(dth)))
    return abs(pose4[2] - truth[0]) <= linear_step and abs(pose4[3] - truth[1]) <= linear_step and dth <= angular_step


def oracle_best(dm, scan, coarse):
    """what the class does with the taken nodes, by the oracle alone: refine each (GaussNewton, Cauchy(0.15), 100 iterations), keep
    the one with the smallest MatchSurface2D::error() -> its pose"""
    refined = [O.solve_full(dm, scan, c)[0] for c in coarse]
    return refined[int(np.argmin([O.match_error(dm, scan, p) for p in refined]))]


def sort_rows(a):
    a = np.asarray(a).reshape(len(a), -1)
    return a[np.lexsort(a.T[::-1])]


def check_class(F, h, tmp_path):
    """CorrelativeSearch2D::search on a Slam2D map: lattice, taken keys, refinement, order, and the end-to-end condition"""
    res, maxsq = 0.05, 100                                             # Slam2D's defaults: l2_max 0.5 m
    ctx = h.hip_context()
    scan = hall_scan(TRUE_POSE)
    n = len(scan)
    _, _, wmn, wmx = h.view_bounds(1)
    box_min, box_max = (float(wmn[0]), float(wmn[1])), (float(wmx[0]), float(wmx[1]))
    cand, lat = h.correlative_search(scan, box_min, box_max, **SEARCH)
    want_lat = lattice_of(res, n, box_min, box_max, **SEARCH)
    assert lat == want_lat, (lat, want_lat)
    # the keys and the selection, restated on the oracle's copy of the device map
    dm, dump = oracle_map_of(F, ctx, maxsq, tmp_path, 0.5)
    dense = Dense(dump, maxsq)
    cs = headings_cs(lattice_angles(lat["headings"]))
    best, _, _, _ = restate(dense, scan, cs, box_min[0], box_min[1], lat["cell_step"], lat["nx"], lat["ny"], lat["tile"], lat["point_step"])
    taken = select(best, lat, SEARCH["max_candidates"])
    want_coarse = coarse_poses(taken, lat, box_min, res)
    assert len(cand["coarse"]) == len(taken) >= 2
    got = np.concatenate([cand["coarse"], cand["score"][:, None].astype(np.float64)], axis=1)
    want = np.concatenate([want_coarse, np.array([[float(t[0])] for t in taken])], axis=1)
    assert np.array_equal(sort_rows(got), sort_rows(want)), (got, want)
    # the refinement: one batch call on the same starts gives the same bits
    B = len(taken)
    poses, out8, it, st = ctx.match_solve_batch(0, [scan] * B, cand["coarse"], max_iterations=100, strategy=0, robust="cauchy", robust_param=0.15)
    assert not st.any()
    assert np.array_equal(poses, cand["pose"]) and np.array_equal(it.astype(np.uint32), cand["iterations"])
    assert np.array_equal(np.sqrt(out8[:, 7] / n), cand["rmse"])
    assert np.all(np.diff(cand["rmse"]) >= 0.0), cand["rmse"]
    # without refinement: the coarse pose, rmse evaluated there
    c0, _ = h.correlative_search(scan, box_min, box_max, refine=False, **SEARCH)
    p0, o0, i0, _ = ctx.match_solve_batch(0, [scan] * B, c0["coarse"], max_iterations=0)
    assert np.array_equal(c0["pose"], c0["coarse"]) and not c0["iterations"].any() and np.array_equal(np.sqrt(o0[:, 7] / n), c0["rmse"])
    assert np.array_equal(sort_rows(c0["coarse"]), sort_rows(cand["coarse"]))
    # end to end.  First the condition on the world, on the CPU alone: the restatement's keys, refined and ranked by the oracle
    assert taken[0][0] == min(t[0] for t in taken) and np.array_equal(cand["coarse"][0], want_coarse[0])      # (here the best key is also the best fit)
    opose = oracle_best(dm, scan, want_coarse)
    assert within_one_step(opose, TRUE_POSE, SEARCH["linear_step"], SEARCH["angular_step"]), (opose, TRUE_POSE)
    assert within_one_step(cand["pose"][0], TRUE_POSE, SEARCH["linear_step"], SEARCH["angular_step"]), (cand["pose"][0], TRUE_POSE)
    return cand


def loc_with_hall(F, gloc_thresh=0.15):
    """a lama::Loc2D on the hall: obstacles every 0.05 m along the walls, every cell further than 0.15 m from a wall free"""
    from _worlds import hall_segments
    segs = hall_segments(**HALL)
    obst = []
    for x0, y0, x1, y1 in segs:
        m = int(round(max(abs(x1 - x0), abs(y1 - y0)) / 0.05)) + 1
        t = np.linspace(0.0, 1.0, m)
        obst.append(np.stack([x0 + t * (x1 - x0), y0 + t * (y1 - y0)], axis=1))
    obst = np.concatenate(obst)
    loc = F.Loc2D(gloc_thresh=gloc_thresh)                             # (l2_max 1 m: max_sqdist 400)
    loc.set_obstacles_world(obst)
    off = O_OFF()
    g = np.arange(int(round(HALL["side"] / 0.05)) + 1)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    ocell = np.unique(np.floor(obst * 20.0 + 0.5).astype(np.int64), axis=0)
    near = np.zeros(gx.shape, dtype=bool)
    for dx in range(-3, 4):
        for dy in range(-3, 4):
            ix, iy = ocell[:, 0] + dx, ocell[:, 1] + dy
            ok = (ix >= 0) & (ix < near.shape[0]) & (iy >= 0) & (iy < near.shape[1])
            near[ix[ok], iy[ok]] = True
    free = np.stack([gx[~near] + off, gy[~near] + off], axis=1).astype(np.uint32)
    loc.occ_set_cells(free, -1)
    return loc, free


def check_relocalize(F, tmp_path):
    """Loc2D::relocalize from a wrong pose: true, on the best candidate; with gloc_thresh below the achieved rmse: false, nothing changes"""
    scan = hall_scan(TRUE_POSE)
    wrong = (TRUE_POSE[0] - 3.5, TRUE_POSE[1] + 4.0, TRUE_POSE[2] + math.pi / 2)
    kw = {k: SEARCH[k] for k in ("linear_step", "angular_step", "point_step", "tile", "max_candidates")}
    loc, free = loc_with_hall(F)
    try:
        loc.set_pose(*wrong)
        # the condition on the world first: the restatement over the occupancy map's bounds, free nodes only, refined by the oracle
        ctx = loc.hip_context()
        dm, dump = oracle_map_of(F, ctx, 400, tmp_path, 1.0)
        mn, mx = loc.occ_bounds()
        box_min, box_max = (float(mn[0]), float(mn[1])), (float(mx[0]), float(mx[1]))
        lat = lattice_of(0.05, len(scan), box_min, box_max, **SEARCH)
        cs = headings_cs(lattice_angles(lat["headings"]))
        best, _, _, _ = restate(Dense(dump, 400), scan, cs, box_min[0], box_min[1], lat["cell_step"], lat["nx"], lat["ny"], lat["tile"], lat["point_step"])
        freeset = set(map(tuple, free.tolist()))
        node = lat["cell_step"] * 0.05

        def keep(ix, iy):
            c = O.w2m([box_min[0] + ix * node, box_min[1] + iy * node, 0.0])
            return (int(c[0]), int(c[1])) in freeset

        taken = select(best, lat, SEARCH["max_candidates"], keep)
        want_coarse = coarse_poses(taken, lat, box_min, 0.05)
        opose = oracle_best(dm, scan, want_coarse)
        assert within_one_step(opose, TRUE_POSE, SEARCH["linear_step"], SEARCH["angular_step"]), (opose, TRUE_POSE)
        # the device
        assert loc.relocalize(scan, **kw) is True
        cand = loc.relocalize_candidates()
        assert np.array_equal(sort_rows(cand["coarse"]), sort_rows(want_coarse))
        assert np.all(np.diff(cand["rmse"]) >= 0.0) and cand["rmse"][0] < 0.15
        assert np.array_equal(loc.pose(), cand["pose"][0])
        assert within_one_step(loc.pose(), TRUE_POSE, SEARCH["linear_step"], SEARCH["angular_step"]), (loc.pose(), TRUE_POSE)
        assert not loc.global_localization_active()
        achieved = float(cand["rmse"][0])
    finally:
        loc.close()
    loc, _ = loc_with_hall(F, gloc_thresh=0.5 * achieved)
    try:
        loc.set_pose(*wrong)
        loc.update(scan, (0.0, 0.0, 0.0), 0.0)                        # (the first update only latches the odometry: has_first_scan)
        before = (loc.pose().copy(), loc.covar().copy(), loc.global_localization_active(), loc.rmse())
        assert loc.relocalize(scan, **kw) is False
        assert np.array_equal(loc.pose(), before[0]) and np.array_equal(loc.covar(), before[1])
        assert loc.global_localization_active() == before[2] and loc.rmse() == before[3]
        # an update with little motion is still skipped: has_first_scan was not reset
        assert loc.update(scan, (0.01, 0.0, 0.0), 1.0) is False
        loc.trigger_global_localization()
        assert loc.global_localization_active()
        assert loc.relocalize(scan, **kw) is False and loc.global_localization_active()
    finally:
        loc.close()


def check_missing_entry(F):
    """on an engine without the entry (the test double of tests/cpu_engine) search throws, naming it"""
    h = F.Slam2D()
    try:
        pose = MAP_POSES[0]
        h.set_pose(*pose)
        h.update(hall_scan(pose, beams=60), pose, 0.0)
        try:
            h.correlative_search(hall_scan(pose, beams=60), (0.0, 0.0), (1.0, 1.0))
        except F.LamaError as e:
            assert "lama_hip_match_search_lattice" in str(e) and "missing entry" in str(e), str(e)
        else:
            raise AssertionError("the search ran on an engine without lama_hip_match_search_lattice")
    finally:
        h.close()
