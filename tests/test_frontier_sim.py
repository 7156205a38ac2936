"""lama_hip_map_frontiers (iris_lama_amd/csrc/lama_frontier.h) under the lane-level simulator of tests/sim (the kernel SOURCES
compiled for the host, see tests/test_kernel_sim.py): runs where there is no GPU.  The cases are in tests/_frontier_checks.py, the
expected clusters in tests/_frontier.py."""
import os
import subprocess

import pytest

import _frontier_checks as FC

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_LIB = os.path.join(HERE, "sim", "_build", "liblama_hip_sim.so")
SIM_LIB_WIDE = os.path.join(HERE, "sim", "_build", "liblama_hip_sim_wide.so")


@pytest.fixture(scope="module")
def Fsim():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "sim")], check=True)
    import iris_lama_amd.ffi as F
    saved = F.HIP_LIB, F._hip, F.HIP_LIB_WIDE, F._hip_wide
    F.HIP_LIB, F._hip, F.HIP_LIB_WIDE, F._hip_wide = SIM_LIB, None, SIM_LIB_WIDE, None
    yield F
    F.HIP_LIB, F._hip, F.HIP_LIB_WIDE, F._hip_wide = saved


def test_the_pixel_rule(Fsim):
    FC.check_pixel_rule(Fsim)


def test_the_pixel_rule_with_log_odds_cells(Fsim):
    FC.check_pixel_rule(Fsim, policy=1)


def test_cells_outside_the_map_window_are_unknown(Fsim):
    FC.check_window_edge(Fsim)


def test_the_halo(Fsim):
    FC.check_halo(Fsim)


def test_a_box_at_coordinate_zero_has_no_halo_below_it(Fsim):
    FC.check_coordinate_zero(Fsim)


def test_connectivity_across_patch_seams(Fsim):
    FC.check_seams(Fsim)


def test_diagonal_connections_through_the_corner_of_four_patches(Fsim):
    FC.check_corner_diagonals(Fsim)


def test_the_label_is_the_smallest_index_whatever_the_scan_order(Fsim):
    FC.check_label_propagation(Fsim)


def test_records_min_pixels_and_cap(Fsim):
    FC.check_records(Fsim)


def test_strides_and_boxes_beside_and_beyond_the_map(Fsim):
    FC.check_strides_and_boxes(Fsim)


def test_refusals_leave_every_output_untouched(Fsim):
    FC.check_refusals(Fsim)


def test_empty_map(Fsim):
    FC.check_empty_map(Fsim)


def test_random_maps(Fsim):
    FC.check_random_maps(Fsim)


def test_one_hot_root(Fsim):
    FC.check_hot_root(Fsim)
