"""lama_hip_map_frontiers (iris_lama_amd/csrc/lama_frontier.h) on the device, and getFrontiers of the host classes over it.  The
cases are in tests/_frontier_checks.py, the expected clusters in tests/_frontier.py (numpy / Python, from download_map)."""
import numpy as np
import pytest

import _frontier as FR
import _frontier_checks as FC
import iris_lama_amd.ffi as F

pytestmark = pytest.mark.gpu


def test_the_pixel_rule():
    FC.check_pixel_rule(F)


def test_the_pixel_rule_with_log_odds_cells():
    FC.check_pixel_rule(F, policy=1)


def test_cells_outside_the_map_window_are_unknown():
    FC.check_window_edge(F)


def test_the_halo():
    FC.check_halo(F)


def test_a_box_at_coordinate_zero_has_no_halo_below_it():
    FC.check_coordinate_zero(F)


def test_connectivity_across_patch_seams():
    FC.check_seams(F)


def test_diagonal_connections_through_the_corner_of_four_patches():
    FC.check_corner_diagonals(F)


def test_the_label_is_the_smallest_index_whatever_the_scan_order():
    FC.check_label_propagation(F)


def test_records_min_pixels_and_cap():
    FC.check_records(F)


def test_strides_and_boxes_beside_and_beyond_the_map():
    FC.check_strides_and_boxes(F)


def test_refusals_leave_every_output_untouched():
    FC.check_refusals(F)


def test_empty_map():
    FC.check_empty_map(F)


def test_random_maps():
    FC.check_random_maps(F)


def test_one_hot_root():
    """every lane of a wave adds to the same root: the sums and the box must be exact"""
    FC.check_hot_root(F)


def _check_set(fs, grid, what):
    """a FrontierSet against the restatement on the occupancy grid of the same (whole-map) box, and the two world-frame formulas"""
    assert (fs.x0, fs.y0, fs.width, fs.height, fs.stride) == (grid.x0, grid.y0, grid.width, grid.height, grid.stride), what
    assert fs.resolution == grid.resolution and fs.cell_size == grid.cell_size and np.array_equal(fs.origin, grid.origin), what
    recs, labels, pixels = FR.expect_of_grid(grid.data)
    assert fs.clusters == len(recs) >= 1 and fs.frontier_pixels == pixels and np.array_equal(fs.labels, labels), what
    for name in FR.FRONTIER_T.names:
        assert np.array_equal(fs.frontiers[name], recs[name]), (what, name)
    s, half = float(fs.stride), (float(fs.stride) - 1.0) / 2.0
    for f in fs.frontiers:
        ci, cj = float(f["sum_i"]) / float(f["pixels"]), float(f["sum_j"]) / float(f["pixels"])
        assert f["centroid"].tolist() == [fs.origin[0] + fs.resolution * (s * ci + half), fs.origin[1] + fs.resolution * (s * cj + half)], what
        li, lj = float(int(f["label"]) % fs.width), float(int(f["label"]) // fs.width)
        assert f["seed"].tolist() == [fs.origin[0] + fs.resolution * (s * li + half), fs.origin[1] + fs.resolution * (s * lj + half)], what
        assert grid.data[int(f["label"]) // fs.width, int(f["label"]) % fs.width] == 0           # the seed is a free pixel
    return recs


def test_host_classes_hand_out_the_frontiers_of_their_device_maps():
    pts, odom, _ = F.corridor_log(8, 120)
    s = F.Slam2D(trans_thresh=0.01, rot_thresh=0.01)
    assert s.frontiers() is None                                               # before the first scan
    for k in range(8):
        s.update(pts[k], odom[k])
    s.view_bounds(0)                                                           # getOccupancyMap(): downloads the snapshot
    cells_before = s.view_cells(0)
    for stride in (1, 4):
        _check_set(s.frontiers(stride=stride, labels=True), s.occupancy_grid(stride=stride), f"Slam2D, stride {stride}")
    assert np.array_equal(s.view_cells(0), cells_before)                       # the snapshot is neither remade nor dropped
    few, whole = s.frontiers(min_pixels=3, max_frontiers=2), s.frontiers(min_pixels=3)
    assert few.clusters == whole.clusters == len(whole.frontiers) and len(few.frontiers) == min(2, few.clusters) and few.labels is None
    assert np.array_equal(few.frontiers, whole.frontiers[:2])
    s.close()

    pf = F.PFSlam2D(F.pf_options(particles=4, seed=3, trans_thresh=0.01, rot_thresh=0.01))
    pf.set_prior(*odom[0])
    for k in range(8):
        pf.update(pts[k], odom[k])
    i = (pf.best() + 1) % 4
    _check_set(pf.frontiers(particle=i, labels=True), pf.occupancy_grid(particle=i), "PFSlam2D, another particle")
    assert np.array_equal(pf.frontiers().frontiers, pf.frontiers(particle=pf.best()).frontiers) and pf.frontiers(particle=4) is None
    pf.close()

    mb = F.MapBuilder2D()
    for k in range(4):
        mb.add(pts[k], F.pose_from_xyr(*odom[k]))
    assert mb.frontiers() is None                                              # before the first build
    mb.build()
    _check_set(mb.frontiers(labels=True), mb.occupancy_grid(), "MapBuilder2D")
    mb.close()
