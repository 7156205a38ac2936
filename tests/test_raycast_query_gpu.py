"""lama_hip_map_cast_rays (iris_lama_amd/csrc/lama_raycast_query.h) on the device, and castRays / checkScan of the host classes over
it.  The cases are in tests/_raycast_query_checks.py, the expected results in tests/_raycast_query.py (numpy, from download_map, the
reference's w2m and computeRay)."""
import math

import numpy as np
import pytest

import _raycast_query as RQ
import _raycast_query_checks as QC
import iris_lama_amd.ffi as F

pytestmark = pytest.mark.gpu


def test_both_libraries_export_the_call():
    assert hasattr(F.hip_lib(), "lama_hip_map_cast_rays") and hasattr(F.hip_lib(wide=True), "lama_hip_map_cast_rays")


def test_cell_classes_frequency():
    QC.check_cell_classes_frequency(F)


def test_cell_classes_log_odds():
    QC.check_cell_classes_log_odds(F)


def test_cell_classes_distance():
    QC.check_cell_classes_distance(F)


def test_cell_classes_distance_of_the_wide_library():
    assert F.needs_wide(10.0, 0.05)
    QC.check_cell_classes_distance(F, l2_max=10.0)


@pytest.mark.parametrize("place", QC.PLACES)
def test_directions_with_one_obstacle(place):
    QC.check_directions(F, place)


def test_beam_inside_the_sensor_cell():
    QC.check_beam_inside_the_sensor_cell(F)


def test_patch_crossings():
    QC.check_patch_crossings(F)


def test_scan_sizes():
    QC.check_scan_sizes(F)


def test_three_poses_three_answers():
    QC.check_three_poses(F)


def test_one_wave_with_every_exit():
    QC.check_mixed_wave(F)


def test_a_built_map():
    m = QC.BuiltRoom(F)
    QC.check_built_map(m)
    m.close()


def test_labels():
    QC.check_labels(F)


def test_limits_and_refusals():
    QC.check_limits(F)


def test_scan_of_5000_points():
    QC.check_scan_of_5000_points(F)


def test_more_poses_than_a_grid_has_rows():
    QC.check_more_poses_than_a_grid_has_rows(F)


FAN = (90, -math.pi, 2.0 * math.pi / 90.0, 12.0)


def test_slam2d_and_pfslam2d_cast_rays_through_their_device_maps():
    pts, odom, truth = F.corridor_log(8, 360)
    fan = F.fan_points(*FAN)
    poses = np.stack([F.pose_from_xyr(*truth[k]) for k in (0, 4, 8)])
    s = F.Slam2D(trans_thresh=0.01, rot_thresh=0.01)
    assert s.cast_rays(poses, fan) is None and s.expected_ranges(poses, *FAN) is None          # before the first scan
    for k in range(9):
        s.update(pts[k], odom[k])
    ctx = s.hip_context()
    occ, dm = ctx.download_map(0, F.MAP_OCCUPANCY), ctx.download_map(0, F.MAP_DISTANCE)
    for su in (False, True):
        want = RQ.expected(poses, fan, occ, False, dm, 100, stop_unknown=su, tolerance=1)
        RQ.assert_equal(s.cast_rays(poses, fan, stop_at_unknown=su, tolerance_cells=1), want, f"Slam2D, stop_at_unknown {su}")
        RQ.assert_equal(ctx.cast_rays(0, F.MAP_OCCUPANCY, poses, fan, stop_at_unknown=su, tolerance_cells=1, resolution=0.05), want, "its context")
    want = RQ.expected(poses, fan, occ, False, dm, 100)
    assert (want.status == RQ.OCCUPIED).sum() > 60 and np.array_equal(s.expected_ranges(poses, *FAN), want.range)
    RQ.assert_equal(s.cast_rays(poses, fan, distance_map=True), RQ.expected(poses, fan, dm, True, dm, 100), "Slam2D, distance map")
    s.close()

    pf = F.PFSlam2D(F.pf_options(particles=4, seed=3, trans_thresh=0.01, rot_thresh=0.01))
    pf.set_prior(*odom[0])
    assert pf.cast_rays(poses, fan) is None
    for k in range(9):
        pf.update(pts[k], odom[k])
    i = (pf.best() + 1) % 4
    ctx = pf.hip_context()
    occ, dm = ctx.download_map(i, F.MAP_OCCUPANCY), ctx.download_map(i, F.MAP_DISTANCE)
    want = RQ.expected(poses, fan, occ, False, dm, 100, stop_unknown=True, tolerance=0)
    assert (want.status == RQ.OCCUPIED).sum() > 60
    RQ.assert_equal(pf.cast_rays(poses, fan, particle=i, stop_at_unknown=True, tolerance_cells=0), want, f"PFSlam2D particle {i}")
    RQ.assert_equal(ctx.cast_rays(i, F.MAP_OCCUPANCY, poses, fan, stop_at_unknown=True, tolerance_cells=0, resolution=0.05), want, "its context")
    best = pf.cast_rays(poses, fan)
    assert np.array_equal(best.step, pf.cast_rays(poses, fan, particle=pf.best()).step) and pf.cast_rays(poses, fan, particle=4) is None
    pf.close()


def test_loc2d_casts_rays_and_checks_its_scan_on_the_distance_map():
    from _worlds import corridor_obstacles
    pts, odom, truth = F.corridor_log(4, 360)
    fan = F.fan_points(*FAN)
    h = F.Loc2D()
    poses = np.stack([F.pose_from_xyr(*truth[k]) for k in (0, 2, 4)])
    assert h.cast_rays(poses, fan) is None and h.check_scan(pts[0]) is None                    # no device map yet
    h.set_obstacles_world(corridor_obstacles())
    h.set_pose(*(truth[0] + np.array([0.04, -0.03, 0.01])))
    for k in range(5):
        h.update(pts[k], odom[k], float(k), force=(k == 0))
    ctx = h.hip_context()
    dm = ctx.download_map(0, F.MAP_DISTANCE)
    want = RQ.expected(poses, fan, dm, True, dm, 400, tolerance=2)
    assert (want.status == RQ.OCCUPIED).sum() > 60
    RQ.assert_equal(h.cast_rays(poses, fan, tolerance_cells=2), want, "Loc2D")
    RQ.assert_equal(ctx.cast_rays(0, F.MAP_DISTANCE, poses, fan, tolerance_cells=2, resolution=0.05), want, "its context")
    with pytest.raises(F.LamaError, match="STOP_UNKNOWN"):
        h.cast_rays(poses, fan, stop_at_unknown=True)
    # the scan it was just localised with, in the static corridor: a share is enough here -- the pose is an optimiser's result
    labels = h.check_scan(pts[4], tolerance_cells=2)
    assert labels.shape == (360,) and np.array_equal(labels, ctx.cast_rays(0, F.MAP_DISTANCE, h.pose(), pts[4], tolerance_cells=2).label[0])
    print("check_scan: agrees", int((labels == F.RAY_AGREES).sum()), "blocked", int((labels == F.RAY_BLOCKED).sum()), "novel", int((labels == F.RAY_NOVEL).sum()))
    assert (labels == F.RAY_AGREES).sum() >= 0.9 * len(labels)
    h.close()
