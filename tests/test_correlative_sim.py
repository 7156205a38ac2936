"""k_search_lattice (iris_lama_amd/csrc/lama_correlative.h), lama_hip_match_search_lattice, lama::CorrelativeSearch2D and
Loc2D::relocalize under the lane-level simulator of tests/sim (the kernel SOURCES compiled for the host, see tests/test_kernel_sim.py):
runs where there is no GPU.  The checks are in tests/_correlative_checks.py; the kernel checks are exact."""
import os
import subprocess

import pytest

import _correlative_checks as CK
import _match_checks as M
import _testhost

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


@pytest.fixture(scope="module")
def world(Fsim):
    ctx, dm = M.build_world(Fsim, 1.0)
    yield ctx, dm
    ctx.close()


def test_point_slices_and_wave_split_equal_the_restatement(world):
    CK.check_point_slicing(*world)


def test_cell_stride_and_tile_edges(world):
    CK.check_stride_and_tiles(*world)


def test_absent_patches_and_cells_beyond_the_window(world):
    CK.check_absent_and_window(*world)


def test_ties_go_to_the_smaller_index(Fsim):
    CK.check_ties(Fsim)


def test_every_particle_is_scored_on_its_own_map_and_nothing_changes(Fsim):
    CK.check_maps_per_particle(Fsim)


def test_invalid_arguments_are_refused_with_the_outputs_untouched(Fsim, world):
    CK.check_refusals(Fsim, *world)


def test_wide_library(Fsim):
    CK.check_wide(Fsim)


@pytest.fixture(scope="module")
def hall_slam(Fsim):
    """lama::Slam2D of the test-suite's host build, bound to the simulator as its device library"""
    _testhost.set_engine_library(SIM_LIB)
    h = CK.slam_with_hall(Fsim)
    assert h.engine_origin() == SIM_LIB
    yield h
    h.close()
    _testhost.set_engine_library(None)


def test_class_search_equals_restatement_selection_and_batch_refinement(Fsim, hall_slam, tmp_path):
    CK.check_class(Fsim, hall_slam, tmp_path)


def test_loc2d_relocalize_from_a_wrong_pose_and_below_the_threshold(Fsim, hall_slam, tmp_path):
    CK.check_relocalize(Fsim, tmp_path)


def test_search_on_an_engine_without_the_entry_names_it():
    """the test double of tests/cpu_engine implements the device C-ABI without lama_hip_match_search_lattice"""
    import iris_lama_amd.ffi as F
    _testhost.set_engine_library(_testhost.CPU_ENGINE)
    try:
        CK.check_missing_entry(F)
    finally:
        _testhost.set_engine_library(None)
