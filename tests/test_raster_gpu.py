"""lama_hip_map_rasterize / lama_hip_map_bounds (iris_lama_amd/csrc/lama_raster.h) on the device, and the grid methods of the host
classes over them.  The cases are in tests/_raster_checks.py, the expected grids in tests/_raster.py (numpy, from download_map)."""
import numpy as np
import pytest

import _raster as RS
import _raster_checks as RC
import iris_lama_amd.ffi as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    m = RC.BuiltMap(F)
    yield m
    m.close()


def test_every_cell_state_constructed():
    RC.check_constructed_cell_states(F)


def test_distance_states():
    RC.check_distance_states(F)


def test_distance_states_of_the_wide_library_at_a_reach_of_200_cells():
    assert F.needs_wide(10.0, 0.05)
    RC.check_distance_states(F, l2_max=10.0, extra=(16384, 20000))


def test_a_built_map_all_layers_bounds_and_the_occupied_set(built):
    RC.check_built_map(built)


def test_boxes_beside_inside_and_beyond_the_map(built):
    RC.check_boxes(built)


def test_refusals_leave_the_output_untouched(built):
    RC.check_refusals(built)


def test_log_odds_policy():
    RC.check_log_odds_policy(F)


def test_empty_map():
    RC.check_empty_map(F)


def test_host_classes_hand_out_the_grids_of_their_device_maps():
    pts, odom, _ = F.corridor_log(8, 120)
    s = F.Slam2D(trans_thresh=0.01, rot_thresh=0.01)
    assert s.occupancy_grid() is None and s.distance_grid() is None          # before the first scan
    for k in range(8):
        s.update(pts[k], odom[k])
    g0, d0 = s.occupancy_grid(), s.distance_grid()                             # before the snapshots exist
    mn, mx, wmn, _ = s.view_bounds(0)                                          # getOccupancyMap(): downloads the snapshot
    cells_before = s.view_cells(0)
    g, d = s.occupancy_grid(), s.distance_grid()
    assert np.array_equal(s.view_cells(0), cells_before)                       # the snapshot is neither remade nor dropped
    for a, b in ((g0, g), (d0, d)):
        assert np.array_equal(a.data, b.data) and (a.x0, a.y0, a.width, a.height) == (b.x0, b.y0, b.width, b.height)
    assert (g.x0, g.y0, g.width, g.height, g.stride) == (mn[0], mn[1], mx[0] - mn[0], mx[1] - mn[1], 1)
    assert g.cell_size == 0.05 and g.origin.tolist() == [wmn[0], wmn[1], 0.0]
    xs, ys = np.meshgrid(np.arange(mn[0], mx[0], dtype=np.uint32), np.arange(mn[1], mx[1], dtype=np.uint32))
    fr, oc, _, _ = s.view_occupancy(np.stack([xs.ravel(), ys.ravel()], axis=1))
    want = np.where(fr, 0, np.where(oc, 100, -1)).astype(np.int8).reshape(g.height, g.width)      # isFree / else isOccupied / else
    assert (want == 100).sum() > 50 and (want == 0).sum() > 1000
    assert np.array_equal(g.data, want)
    dmn, dmx, _, _ = s.view_bounds(1)
    assert (d.x0, d.y0, d.width, d.height) == (dmn[0], dmn[1], dmx[0] - dmn[0], dmx[1] - dmn[1]) and d.max_distance == 0.5
    xs, ys = np.meshgrid(np.arange(dmn[0], dmx[0], dtype=np.uint32), np.arange(dmn[1], dmx[1], dtype=np.uint32))
    assert np.array_equal(d.metres(), s.view_distance_cells(np.stack([xs.ravel(), ys.ravel()], axis=1)).reshape(d.height, d.width))
    coarse = s.occupancy_grid(stride=8, world_box=(wmn[0] + 0.3, wmn[1] + 0.2, wmn[0] + 3.0, wmn[1] + 1.5))
    dump = s.hip_context().download_map(0, F.MAP_OCCUPANCY)
    assert coarse.x0 % 8 == 0 and coarse.y0 % 8 == 0 and coarse.width >= 54 // 8 and coarse.cell_size == 8 * 0.05
    assert np.array_equal(coarse.data, RS.raster(dump, RS.TRINARY, coarse.x0, coarse.y0, coarse.width, coarse.height, 8))
    s.close()

    pf = F.PFSlam2D(F.pf_options(particles=4, seed=3, trans_thresh=0.01, rot_thresh=0.01))
    pf.set_prior(*odom[0])
    for k in range(8):
        pf.update(pts[k], odom[k])
    i = (pf.best() + 1) % 4
    ctx = pf.hip_context()
    for grid, kind, layer in ((pf.occupancy_grid(particle=i), F.MAP_OCCUPANCY, RS.TRINARY), (pf.distance_grid(particle=i), F.MAP_DISTANCE, RS.SQDIST)):
        lo, hi, _ = ctx.map_bounds(i, kind)
        assert (grid.x0, grid.y0, grid.width, grid.height) == (lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1])
        assert np.array_equal(grid.data, RS.raster(ctx.download_map(i, kind), layer, grid.x0, grid.y0, grid.width, grid.height, 1, max_sqdist=100))
    best = pf.occupancy_grid()
    assert np.array_equal(best.data, pf.occupancy_grid(particle=pf.best()).data) and pf.occupancy_grid(particle=4) is None
    pf.close()
