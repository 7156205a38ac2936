"""The cases of lama_hip_map_rasterize / lama_hip_map_bounds (iris_lama_amd/csrc/lama_raster.h), shared by the lane-simulator run
(tests/test_raster_sim.py) and the run on the device (tests/test_raster_gpu.py).  `F` is iris_lama_amd.ffi bound to the library
under test.  Every expected grid is computed by tests/_raster.py from HipContext.download_map; every comparison is array_equal."""
import ctypes as C
import math

import numpy as np

import _raster as RS

OFF_PATCH = 2642244 >> 1           # the patch of the map's origin (src/sdm/map.cpp:55-58)
E_INVALID = -1


def max_sqdist_of(cfg):
    r = math.ceil(cfg.l2_max * (1.0 / cfg.resolution))              # DynamicDistanceMap::setMaxDistance
    return r * r


def layers_of(ctx, layer, x0, y0, width, height, stride, dump, what, policy=0, max_sqdist=None):
    got = ctx.rasterize(0, layer, x0, y0, width, height, stride)
    want = RS.raster(dump, layer, x0, y0, width, height, stride, policy, max_sqdist)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {want.size} pixels differ, first at {np.argwhere(got != want)[:4].tolist()}"
    return got


def over_bounds(ctx, kind, stride=1):
    lo, hi, n = ctx.map_bounds(0, kind)
    assert n > 0
    return int(lo[0]), int(lo[1]), (int(hi[0]) - int(lo[0])) // stride, (int(hi[1]) - int(lo[1])) // stride


# ------------------------------------------------------------------------------------------------ 1. every cell state, constructed
FREE_UNKNOWN = [(0, 0), (0, 1), (1, 5), (0, 65535)]                 # region A: free and unknown only
ALL_UNKNOWN = [(0, 0), (1, 4), (2, 8), (16383, 65532)]              # region B: unknown only (visited == 0, or prob == 0.25 exactly)
FREE_OCCUPIED = [(1, 3), (0, 1), (16384, 65535), (0, 65535), (65535, 65535), (1, 5), (1, 1), (0, 1)]      # region C: occupied / free by column


def constructed_occupancy():
    """{patch id: (cells, mask)}: patch A with three 8 x 8 regions of chosen states (rows 0 .. 7; columns 0 .. 7, 8 .. 15, 16 .. 23) and
    random cells elsewhere, an ABSENT patch, and patch B two patches further along x holding free and unknown cells only."""
    import iris_lama_amd.ffi as F
    rng = np.random.default_rng(77)
    cells = np.zeros((32, 32), dtype=F.FREQ_T)
    vis = rng.integers(0, 65536, (32, 32))
    vis[rng.random((32, 32)) < 0.2] = 0
    cells["visited"] = vis
    cells["occupied"] = (rng.random((32, 32)) * (vis + 1)).astype(np.int64).clip(0, vis)
    cells["occupied"][24:26, 24:28] = 40000                          # occupied > visited (a wrapped visited): the probability is capped
    cells["visited"][24:26, 24:28] = 7
    on = np.ones((32, 32), dtype=bool)
    for y in range(8):
        for x in range(8):
            cells[y, x] = FREE_UNKNOWN[(x + 2 * y) % 4] if (x & 1) else (0, 0)         # every 2 x 2 block: unknown columns beside free ones
            cells[y, 8 + x] = ALL_UNKNOWN[(x + y) % 4]
            cells[y, 16 + x] = FREE_OCCUPIED[x]
            on[y, 8 + x] = not (cells[y, 8 + x]["visited"] == 0 and (y & 1))          # (0, 0) with the mask bit on, and with it off
    b = np.zeros((32, 32), dtype=F.FREQ_T)
    b["visited"][::3, ::2] = 9
    b["occupied"][::3, ::2] = 2                                      # 8 < 9: free
    px, py = OFF_PATCH + 3, OFF_PATCH - 2

    def mask(bits):
        m = np.zeros(16, dtype=np.uint64)
        for c in np.flatnonzero(bits.reshape(-1)):
            m[c >> 6] |= np.uint64(1) << np.uint64(c & 63)
        return m
    return {RS.patch_id(px, py): (cells.reshape(-1), mask(on)), RS.patch_id(px + 2, py): (b.reshape(-1), mask(b["visited"] != 0))}, (px * 32, py * 32)


def check_constructed_cell_states(F):
    patches, (ax, ay) = constructed_occupancy()
    ctx = F.HipContext(F.default_cfg(particles=1))
    ctx.upload_map(0, F.MAP_OCCUPANCY, patches)
    dump = ctx.download_map(0, F.MAP_OCCUPANCY)
    assert sorted(dump) == sorted(patches)
    lo, hi, n = ctx.map_bounds(0, F.MAP_OCCUPANCY)
    assert n == 2 and lo.tolist() == [ax, ay] and hi.tolist() == [ax + 96, ay + 32]
    for stride in (1, 2, 8, 32):
        box = over_bounds(ctx, F.MAP_OCCUPANCY, stride)
        tri = layers_of(ctx, F.RASTER_TRINARY, *box, stride, dump, f"trinary, stride {stride}")
        prob = layers_of(ctx, F.RASTER_PROBABILITY, *box, stride, dump, f"probability, stride {stride}")
        if stride == 1:
            a = patches[min(patches)][0].reshape(32, 32)
            quarter = (a["visited"] != 0) & (4 * a["occupied"].astype(np.int64) == a["visited"])
            assert quarter.sum() >= 40 and np.all(tri[:32, :32][quarter] == -1)                  # prob == 0.25: unknown
            assert np.all(tri[:8, 8:16] == -1) and np.all(prob[:8, 8:16][a["visited"][:8, 8:16] == 0] == -1)
            assert set(np.unique(tri[:8, :8])) == {-1, 0} and set(np.unique(tri[:8, 16:24])) == {0, 100}
            assert np.all(prob[24:26, 24:28] == 100) and prob[0, 16] == 33 and prob[0, 18] == 25 and prob[0, 21] == 20
            assert np.all(tri[:, 32:64] == -1) and set(np.unique(tri[:, 64:])) == {-1, 0}      # the absent patch; free and unknown only
        if stride in (2, 8):
            k = 8 // stride
            assert np.all(tri[:k, :k] == 0)                          # free with unknown only -> free
            assert np.all(tri[:k, k:2 * k] == -1)                    # all unknown
            assert np.all(tri[:k, 2 * k:3 * k] == 100)               # free with occupied -> occupied
        if stride == 32:
            assert tri.tolist() == [[100, -1, 0]] and prob[0, 1] == -1
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. distance states
def check_distance_states(F, l2_max=None, extra=()):
    cfg = F.default_cfg(particles=1) if l2_max is None else F.default_cfg(particles=1, l2_max=l2_max)
    mx = max_sqdist_of(cfg)
    rng = np.random.default_rng(5)
    cells = np.zeros((32, 32), dtype=F.DIST_T)
    cells["sqdist"] = rng.integers(0, mx + 1, (32, 32))
    cells["valid"] = rng.random((32, 32)) < 0.6                      # valid_obstacle = 0 with an arbitrary sqdist among them
    states = [0, 1, mx - 1, mx] + list(extra)
    for k, sq in enumerate(states):
        cells["sqdist"][k, 3:11] = sq
        cells["valid"][k, 3:11] = 1
    cells["sqdist"][12:16, 12:16] = 7                                # a whole stride-4 block without a valid obstacle
    cells["valid"][12:16, 12:16] = 0
    on = np.ones(1024, dtype=bool)
    on[rng.integers(0, 1024, 40)] = False                            # Map::get: a cell whose mask bit is off does not exist
    on[:len(states) * 32] = True
    mask = np.zeros(16, dtype=np.uint64)
    for c in np.flatnonzero(on):
        mask[c >> 6] |= np.uint64(1) << np.uint64(c & 63)
    px, py = OFF_PATCH - 1, OFF_PATCH + 4
    ctx = F.HipContext(cfg)
    ctx.upload_map(0, F.MAP_DISTANCE, {RS.patch_id(px, py): (cells.reshape(-1), mask)})
    dump = ctx.download_map(0, F.MAP_DISTANCE)
    for stride in (1, 4):
        x0, y0, w, h = over_bounds(ctx, F.MAP_DISTANCE, stride)
        pad = 8 // stride                                            # a margin of absent cells around the patch
        g = layers_of(ctx, F.RASTER_SQDIST, x0 - 8, y0 - 8, w + 2 * pad, h + 2 * pad, stride, dump, f"sqdist, stride {stride}, max {mx}", max_sqdist=mx)
        if stride == 1:
            assert [int(g[8 + k, 8 + 3]) for k in range(len(states))] == states
            assert np.all(g[:8] == mx) and np.all(g[8 + 12:8 + 16, 8 + 12:8 + 16] == mx)
        else:
            assert g[2 + 3, 2 + 3] == mx
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. / 4. / 5. a built map
class BuiltMap:
    """MapBuilder2D's two device steps on a one-particle context: key scans integrated, the occupied cells into the distance map"""

    def __init__(self, F):
        import _mapbuild as MB
        poses4, _, scans, origins, quats = MB.room_log(21, K=6, beams=60, sensor=True)
        self.F = F
        self.ctx = F.HipContext(F.default_cfg(particles=1))
        self.mx = max_sqdist_of(self.ctx.cfg)
        self.ctx.integrate_scans(0, poses4, scans, origins, quats, full=True, prune=True)
        self.occupied = self.ctx.occupied_cells(0)
        self.ctx.add_obstacles(0, self.occupied)
        self.occ = self.ctx.download_map(0, F.MAP_OCCUPANCY)
        self.dm = self.ctx.download_map(0, F.MAP_DISTANCE)

    def close(self):
        self.ctx.close()

    def check(self, layer, x0, y0, w, h, stride, what):
        dump = self.dm if layer == self.F.RASTER_SQDIST else self.occ
        return layers_of(self.ctx, layer, x0, y0, w, h, stride, dump, what, max_sqdist=self.mx)


def check_built_map(m):
    F, ctx = m.F, m.ctx
    assert len(m.occ) > 4 and len(m.dm) > 4 and len(m.occupied) > 20
    for kind, dump in ((F.MAP_OCCUPANCY, m.occ), (F.MAP_DISTANCE, m.dm)):
        lo, hi, n = ctx.map_bounds(0, kind)
        wlo, whi = RS.bounds(list(dump))
        assert n == len(dump) and np.array_equal(lo, wlo) and np.array_equal(hi, whi), (kind, lo, hi, wlo, whi)
    x0, y0, w, h = over_bounds(ctx, F.MAP_OCCUPANCY)
    tri = m.check(F.RASTER_TRINARY, x0, y0, w, h, 1, "built map, trinary")
    m.check(F.RASTER_PROBABILITY, x0, y0, w, h, 1, "built map, probability")
    sq = m.check(F.RASTER_SQDIST, *over_bounds(ctx, F.MAP_DISTANCE), 1, "built map, sqdist")
    assert (sq == 0).sum() == len(m.occupied) and (tri == 0).sum() > 100
    yx = np.argwhere(tri == 100)
    got = np.stack([yx[:, 1] + x0, yx[:, 0] + y0], axis=1)
    assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, m.occupied.tolist()))          # exactly the set occupied_cells lists


def check_boxes(m):
    F, ctx = m.F, m.ctx
    x0, y0, w, h = over_bounds(ctx, F.MAP_OCCUPANCY)
    layers = (F.RASTER_TRINARY, F.RASTER_PROBABILITY, F.RASTER_SQDIST)
    for layer in layers:
        m.check(layer, x0 - 32, y0 - 32, w + 64, h + 64, 1, f"one patch beyond the bounds, layer {layer}")
        g = m.check(layer, x0 - 64 + 5, y0 - 64 + 7, 20, 19, 1, f"inside an absent patch, layer {layer}")
        assert np.all(g == (m.mx if layer == F.RASTER_SQDIST else -1))
        m.check(layer, x0 + 6, y0 + 10, 37, 5, 2, f"ragged row segments, layer {layer}")
        m.check(layer, x0 + 6, y0 + 10, 37, 5, 1, f"ragged row segments at stride 1, layer {layer}")
        # 73,600 cells along x: further than the largest window (1016 patches = 32,512 cells) on both sides of the map
        m.check(layer, x0 - 32 * 1100, y0, 2300, 3, 32, f"beyond the window, layer {layer}")
    ox, oy = (int(v) for v in m.occupied[len(m.occupied) // 2])
    assert ctx.rasterize(0, F.RASTER_TRINARY, ox, oy, 1, 1).tolist() == [[100]]
    assert ctx.rasterize(0, F.RASTER_SQDIST, ox, oy, 1, 1).tolist() == [[0]]
    m.check(F.RASTER_TRINARY, 0, 0, 3, 2, 32, "the first cells of the coordinate space")
    m.check(F.RASTER_SQDIST, 0xFFFFFFE0, 0xFFFFFFC0, 5, 4, 32, "past the last cell of the coordinate space")


def raw_rasterize(ctx, particle, layer, x0, y0, width, height, stride, out, out_bytes=None):
    return ctx.L.lama_hip_map_rasterize(ctx.h, particle, layer, x0, y0, width, height, stride, out.ctypes.data_as(C.c_void_p),
                                        out.nbytes if out_bytes is None else out_bytes)


def check_refusals(m):
    F, ctx = m.F, m.ctx
    x0, y0, _, _ = over_bounds(ctx, F.MAP_OCCUPANCY)
    cases = {
        "stride 3": (0, F.RASTER_TRINARY, x0 // 3 * 3, y0 // 3 * 3, 8, 8, 3, None),
        "stride 0": (0, F.RASTER_TRINARY, x0, y0, 8, 8, 0, None),
        "stride 64": (0, F.RASTER_TRINARY, x0, y0, 8, 8, 64, None),
        "x0 not a multiple of the stride": (0, F.RASTER_TRINARY, x0 + 2, y0, 8, 8, 4, None),
        "y0 not a multiple of the stride": (0, F.RASTER_SQDIST, x0, y0 + 1, 8, 8, 2, None),
        "width 0": (0, F.RASTER_TRINARY, x0, y0, 0, 8, 1, 64),
        "height 32769": (0, F.RASTER_TRINARY, x0, y0, 1, 32769, 1, 64),
        "out_bytes of the wrong layer": (0, F.RASTER_SQDIST, x0, y0, 8, 8, 1, 64),
        "out_bytes too large": (0, F.RASTER_TRINARY, x0, y0, 8, 8, 1, 65),
        "unknown layer": (0, 3, x0, y0, 8, 8, 1, None),
        "negative layer": (0, -1, x0, y0, 8, 8, 1, None),
        "particle >= particles": (1, F.RASTER_TRINARY, x0, y0, 8, 8, 1, None),
    }
    for what, (particle, layer, bx, by, w, h, stride, nbytes) in cases.items():
        out = np.full(128, 0x5A, dtype=np.uint8)
        rc = raw_rasterize(ctx, particle, layer, bx, by, w, h, stride, out, 64 if nbytes is None else nbytes)
        assert rc == E_INVALID, (what, rc)
        assert np.all(out == 0x5A), what
    out = np.full(128, 0x5A, dtype=np.uint8)
    assert raw_rasterize(ctx, 0, F.RASTER_TRINARY, x0, y0, 8, 8, 1, out, 64) == 0 and np.all(out[64:] == 0x5A) and not np.all(out[:64] == 0x5A)
    lo = np.zeros(2, dtype=np.uint32)
    assert ctx.L.lama_hip_map_bounds(ctx.h, 1, F.MAP_OCCUPANCY, lo.ctypes.data_as(C.c_void_p), None, None) == E_INVALID
    assert ctx.L.lama_hip_map_bounds(ctx.h, 0, 2, lo.ctypes.data_as(C.c_void_p), None, None) == E_INVALID


# ------------------------------------------------------------------------------------------------ 6. log-odds policy
def small_scan(n=48, r=1.6):
    a = np.linspace(-2.2, 2.2, n)
    rr = r + 0.3 * np.sin(3.0 * a)
    return np.stack([rr * np.cos(a), rr * np.sin(a), np.zeros(n)], axis=1)


def check_log_odds_policy(F):
    ctx = F.HipContext(F.default_cfg(particles=1, occupancy_policy=1, ray_rule=1, l2_max=1.0))
    pts = small_scan()
    ctx.init(pts, np.array([1.0, 0.0, 0.0, 0.0]))
    for _ in range(2):
        ctx.update_maps(pts)
    dump = ctx.download_map(0, F.MAP_OCCUPANCY)
    for stride in (1, 4):
        box = over_bounds(ctx, F.MAP_OCCUPANCY, stride)
        g = layers_of(ctx, F.RASTER_TRINARY, *box, stride, dump, f"log-odds, stride {stride}", policy=1)
        assert {-1, 0, 100} == set(np.unique(g).tolist())
    out = np.full(64, 0x5A, dtype=np.uint8)
    assert raw_rasterize(ctx, 0, F.RASTER_PROBABILITY, box[0], box[1], 8, 8, 1, out) == E_INVALID and np.all(out == 0x5A)
    assert "occupancy_policy" in ctx._error()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 7. empty map
def check_empty_map(F):
    ctx = F.HipContext(F.default_cfg(particles=2))
    mx = max_sqdist_of(ctx.cfg)
    for kind in (F.MAP_DISTANCE, F.MAP_OCCUPANCY):
        lo, hi, n = ctx.map_bounds(1, kind)
        assert n == 0 and lo.tolist() == [0xFFFFFFFF] * 2 and hi.tolist() == [32, 32]
        wlo, whi = RS.bounds([])
        assert np.array_equal(lo, wlo) and np.array_equal(hi, whi)
    x0 = OFF_PATCH * 32
    assert np.all(ctx.rasterize(1, F.RASTER_TRINARY, x0 - 40, x0 + 8, 70, 33, 1) == -1)
    assert np.all(ctx.rasterize(0, F.RASTER_PROBABILITY, x0, x0, 9, 5, 8) == -1)
    g = ctx.rasterize(1, F.RASTER_SQDIST, x0, x0, 33, 3, 2)
    assert g.shape == (3, 33) and np.all(g == mx)
    ctx.close()
