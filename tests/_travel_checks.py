"""The cases of lama_hip_map_travel (iris_lama_amd/csrc/lama_travel.h), shared by the lane-simulator run (tests/test_travel_sim.py)
and the run on the device (tests/test_travel_gpu.py).  `F` is iris_lama_amd.ffi bound to the library under test.  Maps are built
pixel by pixel and uploaded with HipContext.upload_map, occupancy AND distance cells (the two need not be consistent: the kernel reads
what is stored); every expected value is computed by tests/_travel.py from the grids tests/_raster.py makes of HipContext.download_map;
every comparison is array_equal or ==."""
import ctypes as C

import numpy as np

import _frontier_checks as FC
import _raster as RS
import _raster_checks as RC
import _travel as TR

OFF = RC.OFF_PATCH
E_INVALID = RC.E_INVALID
U, FREE, OCC = FC.U, FC.FREE, FC.OCC
NONE = TR.NONE
SENTINEL = 0x5A5A5A5A


def _pad(pic, fill, dtype):
    pic = np.asarray(pic, dtype=dtype)
    h, w = pic.shape
    out = np.full(((h + 31) // 32 * 32, (w + 31) // 32 * 32), fill, dtype=dtype)
    out[:h, :w] = pic
    return out


def distance_patches(F, sq, px, py, valid=None):
    """{patch id: (cells, mask)} of a picture of squared distances whose cell (0, 0) is the first cell of patch (px, py); every cell
    present, valid_obstacle set unless `valid` says otherwise"""
    out = {}
    for b in range(sq.shape[0] // 32):
        for a in range(sq.shape[1] // 32):
            cells = np.zeros((32, 32), dtype=F.DIST_T)
            cells["sqdist"] = sq[32 * b:32 * b + 32, 32 * a:32 * a + 32]
            cells["valid"] = 1 if valid is None else valid[32 * b:32 * b + 32, 32 * a:32 * a + 32]
            out[RS.patch_id(px + a, py + b)] = (cells.reshape(-1).copy(), np.full(16, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))
    return out


class Scene:
    """one context whose maps are replaced per picture; occupancy=False: a context with a distance map only (lama::Loc2D's)"""

    def __init__(self, F, occupancy=True):
        self.F, self.occupancy = F, occupancy
        self.ctx = F.HipContext(F.default_cfg(particles=1))
        self.mx = RC.max_sqdist_of(self.ctx.cfg)

    def close(self):
        self.ctx.close()

    def load(self, occ, sq=None, px=OFF + 2, py=OFF - 3):
        """occ: picture of U / FREE / OCC; sq: picture of squared distances (None: max_sqdist everywhere).  Padded to whole patches
        with unknown cells / max_sqdist."""
        F = self.F
        occ = np.asarray(occ, dtype=np.int8)
        self.shape = occ.shape
        sq = np.full(occ.shape, self.mx, dtype=np.uint16) if sq is None else np.asarray(sq, dtype=np.uint16)
        assert sq.shape == occ.shape
        self.dump_occ = None
        if self.occupancy:
            patches = FC.patches_of(F, _pad(occ, U, np.int8), px, py)
            self.ctx.upload_map(0, F.MAP_OCCUPANCY, patches)
            self.dump_occ = self.ctx.download_map(0, F.MAP_OCCUPANCY)
            assert sorted(self.dump_occ) == sorted(patches)
        patches = distance_patches(F, _pad(sq, self.mx, np.uint16), px, py)
        self.ctx.upload_map(0, F.MAP_DISTANCE, patches)
        self.dump_dm = self.ctx.download_map(0, F.MAP_DISTANCE)
        assert sorted(self.dump_dm) == sorted(patches)
        self.x0, self.y0 = 32 * px, 32 * py
        return self

    def grids(self, box, stride=1):
        occ = RS.raster(self.dump_occ, RS.TRINARY, *box, stride) if self.dump_occ is not None else None
        return occ, RS.raster(self.dump_dm, RS.SQDIST, *box, stride, max_sqdist=self.mx)

    def check(self, what, sources, goals=(), box=None, stride=1, clearance=0, prefer=None, near_factor=1, reach=0, path_cap=64, inner=0):
        """The whole result against the restatement: field, routes and paths.  sources / goals: PIXELS (i, j) of the box; a goal
        may lie outside it.  inner: the cell of the pixel's block that is handed to the call (0 .. stride - 1).  -> (got, F, routes, paths)"""
        if box is None:
            box = (self.x0, self.y0, self.shape[1] // stride, self.shape[0] // stride)
        prefer = clearance if prefer is None else prefer
        x0, y0, w, h = box
        cells = lambda pts: [(x0 + i * stride + inner, y0 + j * stride + inner) for i, j in pts]
        got = self.ctx.travel(0, x0, y0, w, h, cells(sources), cells(goals), stride=stride, clearance_cells=clearance, prefer_cells=prefer, near_factor=near_factor,
                              goal_reach=reach, path_cap=path_cap, field=True)
        occ, sq = self.grids(box, stride)
        inside = [(i, j) if 0 <= i < w and 0 <= j < h else None for i, j in goals]
        Fx, routes, paths = TR.expect(occ, sq, clearance, prefer, near_factor, sources, inside, reach, path_cap)
        bad = np.argwhere(got.field != Fx)
        assert len(bad) == 0, f"{what}: {len(bad)} field pixels differ, first at (j, i) {bad[:4].tolist()}: got {[int(got.field[j, i]) for j, i in bad[:4]]}, want {[int(Fx[j, i]) for j, i in bad[:4]]}"
        assert got.routes.dtype == routes.dtype and np.array_equal(got.routes, routes), (what, got.routes[:6], routes[:6])
        if path_cap and len(goals):
            assert np.array_equal(got.paths, paths), (what, np.argwhere(got.paths != paths)[:4].tolist())
        return got, Fx, routes, paths


def room(h, w, border=True):
    pic = np.full((h, w), FREE, dtype=np.int8)
    if border:
        pic[0, :], pic[-1, :], pic[:, 0], pic[:, -1] = OCC, OCC, OCC, OCC
    return pic


# ------------------------------------------------------------------------------------------------ 1. open floor, one tile
def check_open_floor(F):
    s = Scene(F).load(np.full((20, 20), FREE, dtype=np.int8))
    goals = [(2, 1), (19, 19), (7, 3), (0, 19)]
    got, Fx, routes, paths = s.check("open floor, source (0, 0)", [(0, 0)], goals)
    dx, dy = np.meshgrid(np.arange(20), np.arange(20))
    assert np.array_equal(got.field, (7 * np.minimum(dx, dy) + 5 * np.abs(dx - dy)).astype(np.uint32))
    # (2, 1) has the equal predecessors (1, 0) [5 + 7] and (1, 1) [7 + 5]: the smaller index is taken
    assert got.path(0).tolist() == [0, 1, 22] and tuple(got.routes[0]) == (TR.REACHED, 22, 12, 2)
    assert got.routes[1]["steps"] == 19 and got.routes[1]["cost"] == 7 * 19
    got, _, _, _ = s.check("open floor, source (19, 19)", [(19, 19)], [(17, 18), (0, 0)])
    assert got.field[0, 0] == 7 * 19
    assert got.path(0).tolist() == [399, 378, 377]                   # predecessors (18, 18) = 378 and (18, 19) = 398
    s.close()


# ------------------------------------------------------------------------------------------------ 2. the move rules
def move_rules_picture():
    pic = room(24, 24)
    pic[:, 8] = OCC                                                  # a wall with a one-pixel door at (8, 12)
    pic[12, 8] = FREE
    pic[1:8, 16], pic[7, 16:23] = OCC, OCC                           # a closet in the upper right corner ...
    pic[7, 16] = FREE                                                # ... whose only opening is the corner pixel of its walls: it
                                                                     # touches the inside, (17, 6), by a corner between two occupied pixels
    pic[16:20, 12:16] = U                                            # a patch of unknown pixels in the middle of the right room
    pic[18, 14] = FREE                                               # with a free pixel inside that nothing can reach
    return pic


def check_move_rules(F):
    pic = move_rules_picture()
    s = Scene(F).load(pic)
    goals = [(20, 3), (4, 4), (18, 14), (12, 12), (22, 22)]
    got, Fx, routes, _ = s.check("the move rules", [(2, 2)], goals)
    assert Fx[12, 8] != NONE and Fx[12, 12] != NONE                  # through the one-pixel door
    assert Fx[7, 16] != NONE and Fx[6, 17] == NONE and Fx[3, 20] == NONE and routes[0]["status"] == TR.UNREACHED      # the diagonal gap is not passed
    assert np.all(Fx[16:20, 12:16] == NONE)                          # unknown pixels are not entered, nor what they enclose
    assert np.all(Fx[pic != FREE] == NONE)
    # the closet is entered when the source stands in it
    got, Fx, _, _ = s.check("from inside the closet", [(20, 3)], goals)
    assert Fx[3, 20] == 0 and Fx[2, 2] == NONE
    # a non-traversable source expands: from the wall pixel (8, 5) both rooms are reached
    got, Fx, _, _ = s.check("a source on a wall pixel", [(8, 5)], goals)
    assert Fx[5, 8] == 0 and Fx[5, 7] == 5 and Fx[5, 9] == 5 and Fx[4, 7] == 10 and Fx[20, 20] != NONE      # (no diagonal past the wall pixel above it)
    # ... and still blocks a neighbour's diagonal: an occupied pixel (4, 15) in open space, as a source and beside one
    pic2 = pic.copy()
    pic2[15, 4] = OCC
    s.load(pic2)
    got, Fx, _, _ = s.check("an occupied source beside a free one", [(4, 15)], goals)
    assert Fx[15, 4] == 0 and Fx[14, 4] == 5 and Fx[15, 3] == 5 and Fx[14, 3] == 7           # it expands by edges and by diagonals
    got, Fx, _, _ = s.check("a free source whose diagonal is blocked by an occupied pixel", [(3, 14)], goals)
    assert Fx[15, 4] == NONE and Fx[14, 4] == 5 and Fx[15, 3] == 5
    assert Fx[16, 4] == 15 and Fx[15, 5] == 15                       # round the occupied pixel by edges: no diagonal cuts its corner (5 + 5 + 5, not 5 + 7)
    got, Fx, _, _ = s.check("both", [(3, 14), (4, 15)], goals)
    assert Fx[15, 4] == 0 and Fx[16, 4] == 5 and Fx[15, 5] == 5
    assert Fx[16, 3] == 7                                            # the occupied source is LEFT by a diagonal between two free pixels
    s.close()


# ------------------------------------------------------------------------------------------------ 3. clearance and preference
def check_clearance_and_preference(F):
    s = Scene(F)
    pic = room(16, 30)
    pic[1:15, 10:20] = OCC                                           # two rooms joined by a corridor along row 7
    pic[7, 10:20] = FREE
    sq = np.full(pic.shape, 81, dtype=np.uint16)
    sq[7, 10:20] = 4                                                 # the corridor is 2 cells from its walls
    s.load(pic, sq)
    _, Fx, routes, _ = s.check("clearance 3 closes the corridor", [(3, 3)], [(25, 12)], clearance=3)
    assert routes[0]["status"] == TR.UNREACHED and Fx[7, 12] == NONE and Fx[7, 9] != NONE
    _, Fx, routes, _ = s.check("clearance 2 opens it", [(3, 3)], [(25, 12)], clearance=2)
    assert routes[0]["status"] == TR.REACHED and Fx[7, 12] != NONE
    # a room whose rim is close to the walls: hugging the upper wall is the straight way, the middle of the room the cheap one
    pic = room(14, 32)
    sq = np.full(pic.shape, 100, dtype=np.uint16)
    sq[1:4, :], sq[10:13, :], sq[:, 1:4], sq[:, 28:31] = 4, 4, 4, 4
    s.load(pic, sq)
    src, goal = [(2, 2)], [(29, 2)]
    _, Fa, ra, pa = s.check("near_factor 4", src, goal, clearance=1, prefer=3, near_factor=4)
    _, Fb, rb, pb = s.check("near_factor 1", src, goal, clearance=1, prefer=3, near_factor=1)
    _, Fc, rc, pc = s.check("prefer == clearance switches the aversion off", src, goal, clearance=1, prefer=1, near_factor=4)
    assert rb[0]["cost"] == 5 * 27 and rb[0]["steps"] == 27 and np.array_equal(Fb, Fc) and np.array_equal(pb, pc)
    assert 5 * 27 < ra[0]["cost"] < 4 * 5 * 27 and not np.array_equal(pa, pb)      # the two routes differ: down into the middle of the room and up again
    rows = pa[0][pa[0] != NONE] // 32
    assert rows.max() >= 4 and rows[0] == 2 and rows[-1] == 2
    s.close()


# ------------------------------------------------------------------------------------------------ 4. tiles
def u_picture():
    pic = np.full((45, 70), FREE, dtype=np.int8)
    pic[10, 0:34] = OCC                                              # a wall from the left edge to just past the tile rim x = 32
    return pic


def serpentine_picture():
    pic = np.full((45, 70), FREE, dtype=np.int8)
    for k, y in enumerate(range(4, 44, 5)):                          # walls every 5 rows with the gap alternating between the two ends
        if k % 2 == 0:
            pic[y, 0:67] = OCC
        else:
            pic[y, 3:70] = OCC
    return pic


def check_tiles(F):
    s = Scene(F)
    s.load(u_picture())
    goals = [(2, 20), (2, 11), (69, 44), (33, 10), (40, 30)]
    got, Fx, routes, paths = s.check("a U across a tile rim", [(2, 2)], goals, path_cap=128)
    way = got.path(1)
    assert (way % 70).max() >= 34 and way[0] == 2 * 70 + 2 and way[-1] == 11 * 70 + 2           # out of the first tile and back into it
    assert got.rounds >= 2
    s.load(serpentine_picture())
    got, Fx, routes, paths = s.check("a serpentine through all six tiles", [(0, 0)], [(69, 44), (0, 44), (35, 22)], path_cap=700)
    tiles = {(int(p) % 70 // 32, int(p) // 70 // 32) for p in got.path(0)}
    assert len(tiles) == 6 and routes[0]["steps"] > 8 * 60 and got.rounds >= 6
    capped, _, _, _ = s.check("the same with a short cap", [(0, 0)], [(69, 44)], path_cap=9)
    assert np.array_equal(capped.paths[0], got.paths[0][:9]) and capped.routes[0]["steps"] == routes[0]["steps"]
    # the corner where four tiles meet: (31, 31) and (32, 32) touch by their corners only
    for name, side_a, side_b, want in (("both side pixels free", FREE, FREE, 7), ("one side pixel occupied", OCC, FREE, 10), ("the other", FREE, OCC, 10),
                                       ("both occupied", OCC, OCC, NONE)):
        pic = np.full((45, 70), OCC, dtype=np.int8)
        pic[31, 29:32], pic[32, 32:35] = FREE, FREE
        pic[31, 32], pic[32, 31] = side_a, side_b
        s.load(pic)
        got, Fx, _, _ = s.check(f"across the corner of four tiles, {name}", [(31, 31)], [(34, 32)])
        assert Fx[32, 32] == want, (name, int(Fx[32, 32]))
        got, Fx, _, _ = s.check(f"across the corner of four tiles the other way, {name}", [(32, 32)], [(29, 31)])
        assert Fx[31, 31] == want, (name, int(Fx[31, 31]))
    for a, b in (((32, 31), (31, 32)), ((31, 32), (32, 31))):        # the other diagonal of the same corner
        pic = np.full((45, 70), OCC, dtype=np.int8)
        pic[31, 32], pic[32, 31] = FREE, FREE
        s.load(pic)
        _, Fx, _, _ = s.check("the anti-diagonal with both side pixels occupied", [a], [b])
        assert Fx[b[1], b[0]] == NONE
        pic[31, 31], pic[32, 32] = FREE, FREE
        s.load(pic)
        _, Fx, _, _ = s.check("the anti-diagonal, open", [a], [b])
        assert Fx[b[1], b[0]] == 7
    s.close()


# ------------------------------------------------------------------------------------------------ 5. many sources
def check_many_sources(F):
    pic = room(40, 66)
    pic[1:39, 22], pic[1:39, 44] = OCC, OCC                          # three rooms side by side; the middle one is shared
    pic[30, 22], pic[8, 44] = FREE, FREE
    s = Scene(F).load(pic)
    a, b = (3, 3), (62, 36)
    goals = [(33, 20), (5, 30), (60, 5)]
    _, Fa, _, _ = s.check("the left source", [a], goals)
    _, Fb, _, _ = s.check("the right source", [b], goals)
    _, Fab, _, _ = s.check("both sources", [a, b], goals)
    assert np.array_equal(Fab, np.minimum(Fa, Fb))
    mid = Fab[1:39, 23:44]
    assert np.any(mid == Fa[1:39, 23:44]) and np.any(mid == Fb[1:39, 23:44]) and np.any(Fa[1:39, 23:44] != Fb[1:39, 23:44])
    _, Fd, _, _ = s.check("a source given twice", [a, b, a], goals)
    assert np.array_equal(Fd, Fab)
    s.close()


# ------------------------------------------------------------------------------------------------ 6. goals
def check_goals(F):
    pic = np.full((40, 40), FREE, dtype=np.int8)
    pic[25:32, 25:32] = OCC                                          # a sealed room
    pic[26:31, 26:31] = FREE
    s = Scene(F).load(pic)
    src = [(20, 10)]
    # below the source, in the sealed room, two corners, two outside the box, above the room's wall, the source itself, anywhere
    goals = [(20, 16), (28, 28), (0, 0), (39, 39), (45, 10), (10, 50), (28, 23), (20, 10), (26, 4)]
    for reach in (0, 3):
        got, Fx, routes, paths = s.check(f"goal_reach {reach}", src, goals, reach=reach)
        assert routes[4]["status"] == routes[5]["status"] == TR.OUTSIDE
        assert routes[1]["status"] == TR.UNREACHED                   # inside the sealed room, window and all
        assert routes[7]["status"] == TR.REACHED and routes[7]["cost"] == 0 and routes[7]["steps"] == 0 and paths[7][0] == 10 * 40 + 20
    assert routes[0]["pixel"] == 13 * 40 + 20 and routes[2]["pixel"] == 3 * 40 + 3           # clipped at the box's corner
    assert routes[6]["status"] == TR.REACHED                         # (28, 23): the room's wall is in the window, free pixels above it too
    # ties: with the goal straight above the source and reach 1 the window's best row is the nearest one, its middle pixel alone;
    # once that pixel is occupied its two neighbours tie and the smaller index wins
    got, Fx, routes, _ = s.check("a tie between the pixels left and right of the source", [(20, 20)], [(20, 14)], reach=1)
    assert routes[0]["pixel"] == 15 * 40 + 20
    pic2 = pic.copy()
    pic2[15, 20] = OCC
    s.load(pic2)
    got, Fx, routes, _ = s.check("a tie, the middle pixel occupied", [(20, 20)], [(20, 14)], reach=1)
    assert Fx[15, 19] == Fx[15, 21] == 5 * 4 + 7 and routes[0]["pixel"] == 15 * 40 + 19
    # path_cap below the path's length: the source end is written, steps is in full, the rest is untouched
    for cap in (1, 4, 64):
        got, Fx, routes, paths = s.check(f"path_cap {cap}", [(2, 38)], [(38, 2), (28, 28)], path_cap=cap)
        assert routes[0]["steps"] == 36 and got.paths[0][0] == 38 * 40 + 2
        assert np.all(got.paths[1] == NONE) and np.all(got.paths[0][37:] == NONE)
    got, _, routes, _ = s.check("no paths asked for", [(2, 38)], [(38, 2)], path_cap=0)
    assert got.paths is None and routes[0]["steps"] == 36
    s.check("no goals", [(2, 2)], [])
    s.close()


# ------------------------------------------------------------------------------------------------ 7. strides, boxes beyond the map
def check_strides_and_boxes(F):
    rng = np.random.default_rng(11)
    pic = np.where(rng.random((64, 64)) < 0.12, OCC, FREE).astype(np.int8)
    pic[20:28, 20:28] = FREE
    sq = rng.integers(4, 101, (64, 64)).astype(np.uint16)
    both, dist_only = Scene(F).load(pic, sq), Scene(F, occupancy=False).load(pic, sq)
    for stride in (2, 4):
        n = 64 // stride
        inside = (both.x0, both.y0, n, n)
        wide = (both.x0 - 32, both.y0 - 64, n + 48 // stride, n + 96 // stride)       # beside and beyond the allocated patches
        src_in = [(24 // stride, 24 // stride)]
        src_wide = [(24 // stride + 32 // stride, 24 // stride + 64 // stride)]
        goals = [(1, 1), (n - 1, n - 1), (n + 40 // stride, n + 80 // stride), (n // 2 + 32 // stride, 64 // stride + 2)]
        for name, s in (("both maps", both), ("distance only", dist_only)):
            s.check(f"stride {stride}, {name}, the patches' box", src_in, goals, box=inside, stride=stride, clearance=2, prefer=5, near_factor=3, reach=1, inner=stride - 1)
            got, Fx, routes, _ = s.check(f"stride {stride}, {name}, a wider box", src_wide, goals, box=wide, stride=stride, clearance=2, prefer=5, near_factor=3, reach=1)
            outside = np.ones(Fx.shape, dtype=bool)
            outside[64 // stride:64 // stride + n, 32 // stride:32 // stride + n] = False
            if s.occupancy:
                assert np.all(Fx[outside] == NONE)                   # absent patches are unknown: not traversable
            else:
                assert np.all(Fx[outside] != NONE)                   # absent cells are max_sqdist away from anything: traversable
                assert routes[2]["status"] == TR.REACHED
    both.close()
    dist_only.close()


# ------------------------------------------------------------------------------------------------ 8. refusals, the map without patches
def raw(ctx, box, stride=1, clearance=0, prefer=0, near_factor=1, sources=((0, 0),), goals=((1, 1),), reach=0, cap=4, particle=0,
        null_sources=False, null_goals=False, null_routes=False, null_paths=False):
    """-> (rc, the output buffers) with every output filled with a sentinel before the call"""
    src = np.array(sources, dtype=np.uint32).reshape(-1, 2)
    gl = np.array(goals, dtype=np.uint32).reshape(-1, 2)
    out = {"routes": np.full(4 * max(len(gl), 1), SENTINEL, dtype=np.uint32), "paths": np.full(max(len(gl), 1) * max(cap, 1), SENTINEL, dtype=np.uint32),
           "field": np.full(64 * 64, SENTINEL, dtype=np.uint32), "rounds": np.full(1, SENTINEL, dtype=np.uint32), "ms": np.full(1, -7.0)}
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = ctx.L.lama_hip_map_travel(ctx.h, particle, *box, stride, clearance, prefer, near_factor, len(src), None if null_sources else p(src), len(gl),
                                   None if null_goals else p(gl), reach, None if null_routes else p(out["routes"]), cap, None if null_paths else p(out["paths"]),
                                   p(out["field"]), p(out["rounds"]), p(out["ms"]))
    return rc, out


def untouched(out):
    return all(np.all(out[k] == SENTINEL) for k in ("routes", "paths", "field", "rounds")) and out["ms"][0] == -7.0


def check_refusals(F):
    s = Scene(F).load(np.full((32, 32), FREE, dtype=np.int8))
    x0, y0 = s.x0, s.y0
    at = lambda i, j: (x0 + i, y0 + j)
    ok = dict(sources=(at(1, 1),), goals=(at(5, 5),))
    cases = {
        "stride 3": dict(box=(x0 // 3 * 3, y0 // 3 * 3, 8, 8), stride=3, sources=((x0 // 3 * 3, y0 // 3 * 3),)),
        "stride 0": dict(box=(x0, y0, 8, 8), stride=0, **ok),
        "stride 64": dict(box=(x0, y0, 8, 8), stride=64, **ok),
        "x0 not a multiple of the stride": dict(box=(x0 + 2, y0, 8, 8), stride=4, sources=(at(4, 4),)),
        "y0 not a multiple of the stride": dict(box=(x0, y0 + 1, 8, 8), stride=2, sources=(at(4, 4),)),
        "width 0": dict(box=(x0, y0, 0, 8), **ok),
        "height 0": dict(box=(x0, y0, 8, 0), **ok),
        "width 32769": dict(box=(x0, y0, 32769, 2), **ok),
        "height 32769": dict(box=(x0, y0, 2, 32769), **ok),
        "a cost could wrap": dict(box=(x0, y0, 32768, 18725), **ok),                 # 32768 * 18725 * 7 = 2^32 + 2^15 * 7 * ... >= 2^32
        "a cost could wrap with the factor": dict(box=(x0, y0, 4096, 4096), near_factor=37, **ok),
        "particle out of range": dict(box=(x0, y0, 8, 8), particle=1, **ok),
        "no source": dict(box=(x0, y0, 8, 8), sources=(), goals=(at(5, 5),)),
        "NULL sources": dict(box=(x0, y0, 8, 8), null_sources=True, **ok),
        "NULL goals": dict(box=(x0, y0, 8, 8), null_goals=True, **ok),
        "NULL routes": dict(box=(x0, y0, 8, 8), null_routes=True, **ok),
        "NULL paths with a cap": dict(box=(x0, y0, 8, 8), null_paths=True, **ok),
        "a source left of the box": dict(box=(x0 + 4, y0, 8, 8), sources=(at(3, 2),), goals=(at(5, 5),)),
        "a source below the box": dict(box=(x0, y0, 8, 8), sources=(at(2, 8),), goals=(at(5, 5),)),
        "the second source outside": dict(box=(x0, y0, 8, 8), sources=(at(2, 2), at(8, 2)), goals=(at(5, 5),)),
        "clearance beyond max_sqdist": dict(box=(x0, y0, 8, 8), clearance=11, prefer=11, **ok),
        "prefer below clearance": dict(box=(x0, y0, 8, 8), clearance=3, prefer=2, **ok),
        "near_factor 0": dict(box=(x0, y0, 8, 8), near_factor=0, **ok),
        "near_factor 65": dict(box=(x0, y0, 8, 8), near_factor=65, **ok),
        "goal_reach 17": dict(box=(x0, y0, 8, 8), reach=17, **ok),
    }
    assert s.mx == 100 and 32768 * 18725 * 7 >= 2 ** 32 > 32768 * 18724 * 7 and 4096 * 4096 * 7 * 37 >= 2 ** 32 > 4096 * 4096 * 7 * 36
    for what, kw in cases.items():
        rc, out = raw(s.ctx, **kw)
        assert rc == E_INVALID, (what, rc)
        assert untouched(out), what
        assert "lama_hip_map_travel" in s.ctx._error(), what
    rc, out = raw(s.ctx, box=(x0, y0, 8, 8), clearance=10, prefer=10, near_factor=64, reach=16, **ok)           # the limits themselves are accepted
    assert rc == 0 and out["routes"][0] == TR.REACHED and out["rounds"][0] >= 1
    s.close()


def check_empty_map(F):
    """neither map has a patch: the field is 0 at the sources and unreached elsewhere, a goal is reached only where its window holds
    a source, and no round runs"""
    ctx = F.HipContext(F.default_cfg(particles=2))
    x0, y0 = OFF * 32 - 40, OFF * 32 + 8
    got = ctx.travel(1, x0, y0, 70, 33, [(x0 + 3, y0 + 4), (x0 + 69, y0 + 32)], [(x0 + 10, y0 + 10), (x0 + 4, y0 + 4), (x0 + 80, y0), (x0 + 3, y0 + 4)],
                     goal_reach=1, path_cap=4, field=True)
    want = np.full((33, 70), NONE, dtype=np.uint32)
    want[4, 3], want[32, 69] = 0, 0
    assert np.array_equal(got.field, want) and got.rounds == 0
    assert [tuple(r) for r in got.routes] == [(TR.UNREACHED, NONE, NONE, 0), (TR.REACHED, 4 * 70 + 3, 0, 0), (TR.OUTSIDE, NONE, NONE, 0), (TR.REACHED, 4 * 70 + 3, 0, 0)]
    assert got.paths.tolist() == [[NONE] * 4, [4 * 70 + 3] + [NONE] * 3, [NONE] * 4, [4 * 70 + 3] + [NONE] * 3]
    assert ctx.travel_stats() == {"rounds": 0, "tiles_run": 0, "max_tiles": 0, "readbacks": 0}
    ctx.close()


# ------------------------------------------------------------------------------------------------ 9. random pictures
RANDOM_SEEDS = (90210, 90211, 90212)
RANDOM_SHARES = (0.75, 0.20, 0.05)                                   # free, occupied, unknown


def random_case(seed, mx=100):
    """-> (occ picture, sq picture, source pixel, 32 goal pixels, the call's parameters)"""
    rng = np.random.default_rng(seed)
    pic = rng.choice(np.array([FREE, OCC, U], dtype=np.int8), size=(96, 96), p=RANDOM_SHARES)
    sq = rng.integers(0, mx + 1, (96, 96)).astype(np.uint16)
    goals = [(int(i), int(j)) for i, j in rng.integers(0, 96, (32, 2))]
    kw = dict(clearance=1, prefer=4, near_factor=1 + seed % 4, reach=0)
    return pic, sq, goals, kw


def random_conditions(routes):
    """what makes a random case worth running; the restatement alone must meet it"""
    reached = int((routes["status"] == TR.REACHED).sum())
    assert reached >= 8 and reached < len(routes), reached


def check_random_pictures(F):
    s = Scene(F)
    for seed in RANDOM_SEEDS:
        pic, sq, goals, kw = random_case(seed, s.mx)
        s.load(pic, sq)
        occ, sqg = s.grids((s.x0, s.y0, 96, 96))
        trav, _ = TR.classify(occ, sqg, kw["clearance"], kw["prefer"])
        src, size = TR.largest_component_source(trav)
        assert size > 1000
        _, _, routes, _ = s.check(f"random picture {seed}", [src], goals, path_cap=96, **kw)
        random_conditions(routes)
    s.close()
