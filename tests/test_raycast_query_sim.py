"""lama_hip_map_cast_rays (iris_lama_amd/csrc/lama_raycast_query.h) under the lane-level simulator of tests/sim (the kernel SOURCES
compiled for the host, see tests/test_kernel_sim.py): runs where there is no GPU.  The cases are in tests/_raycast_query_checks.py,
the expected results in tests/_raycast_query.py."""
import os
import subprocess

import pytest

import _raycast_query_checks as QC
import _reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_LIB = os.path.join(HERE, "sim", "_build", "liblama_hip_sim.so")
SIM_LIB_WIDE = os.path.join(HERE, "sim", "_build", "liblama_hip_sim_wide.so")
needs_reference = pytest.mark.skipif(not R.available(), reason="the compiled reference (oracle/_ref, made by build()) poses the key scans")


@pytest.fixture(scope="module")
def Fsim():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "sim")], check=True)
    import iris_lama_amd.ffi as F
    saved = F.HIP_LIB, F._hip, F.HIP_LIB_WIDE, F._hip_wide
    F.HIP_LIB, F._hip, F.HIP_LIB_WIDE, F._hip_wide = SIM_LIB, None, SIM_LIB_WIDE, None
    yield F
    F.HIP_LIB, F._hip, F.HIP_LIB_WIDE, F._hip_wide = saved


def test_the_simulated_library_exports_the_call(Fsim):
    assert hasattr(Fsim.hip_lib(), "lama_hip_map_cast_rays") and hasattr(Fsim.hip_lib(wide=True), "lama_hip_map_cast_rays")


def test_cell_classes_frequency(Fsim):
    QC.check_cell_classes_frequency(Fsim)


def test_cell_classes_log_odds(Fsim):
    QC.check_cell_classes_log_odds(Fsim)


def test_cell_classes_distance(Fsim):
    QC.check_cell_classes_distance(Fsim)


def test_cell_classes_distance_of_the_wide_build(Fsim):
    assert Fsim.needs_wide(10.0, 0.05)
    QC.check_cell_classes_distance(Fsim, l2_max=10.0)


@pytest.mark.parametrize("place", QC.PLACES)
def test_directions_with_one_obstacle(Fsim, place):
    QC.check_directions(Fsim, place)


def test_beam_inside_the_sensor_cell(Fsim):
    QC.check_beam_inside_the_sensor_cell(Fsim)


def test_patch_crossings(Fsim):
    QC.check_patch_crossings(Fsim)


def test_scan_sizes(Fsim):
    QC.check_scan_sizes(Fsim)


def test_three_poses_three_answers(Fsim):
    QC.check_three_poses(Fsim)


def test_one_wave_with_every_exit(Fsim):
    QC.check_mixed_wave(Fsim)


@needs_reference
def test_a_built_map(Fsim):
    m = QC.BuiltRoom(Fsim)
    QC.check_built_map(m)
    m.close()


def test_labels(Fsim):
    QC.check_labels(Fsim)


def test_limits_and_refusals(Fsim):
    QC.check_limits(Fsim)


def test_scan_of_5000_points(Fsim):
    QC.check_scan_of_5000_points(Fsim)
