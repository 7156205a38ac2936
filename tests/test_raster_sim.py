"""lama_hip_map_rasterize / lama_hip_map_bounds (iris_lama_amd/csrc/lama_raster.h) under the lane-level simulator of tests/sim (the
kernel SOURCES compiled for the host, see tests/test_kernel_sim.py): runs where there is no GPU.  The cases are in
tests/_raster_checks.py, the expected grids in tests/_raster.py."""
import os
import subprocess

import pytest

import _raster_checks as RC
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


@pytest.fixture(scope="module")
def built(Fsim):
    m = RC.BuiltMap(Fsim)
    yield m
    m.close()


def test_every_cell_state_constructed(Fsim):
    RC.check_constructed_cell_states(Fsim)


def test_distance_states(Fsim):
    RC.check_distance_states(Fsim)


def test_distance_states_of_the_wide_build_at_a_reach_of_200_cells(Fsim):
    assert Fsim.needs_wide(10.0, 0.05)
    RC.check_distance_states(Fsim, l2_max=10.0, extra=(16384, 20000))


@needs_reference
def test_a_built_map_all_layers_bounds_and_the_occupied_set(built):
    RC.check_built_map(built)


@needs_reference
def test_boxes_beside_inside_and_beyond_the_map(built):
    RC.check_boxes(built)


@needs_reference
def test_refusals_leave_the_output_untouched(built):
    RC.check_refusals(built)


def test_log_odds_policy(Fsim):
    RC.check_log_odds_policy(Fsim)


def test_empty_map(Fsim):
    RC.check_empty_map(Fsim)
