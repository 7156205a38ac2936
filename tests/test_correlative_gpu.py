"""-m gpu: k_search_lattice (iris_lama_amd/csrc/lama_correlative.h), lama_hip_match_search_lattice, lama::CorrelativeSearch2D and
Loc2D::relocalize on the device.  The checks are those of tests/test_correlative_sim.py (tests/_correlative_checks.py): the kernel
checks are exact here too, because the transform of every heading is composed on the host and the scores are integer sums."""
import pytest

import iris_lama_amd.ffi as F

import _correlative_checks as CK
import _match_checks as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    ctx, dm = M.build_world(F, 1.0)
    yield ctx, dm
    ctx.close()


def test_point_slices_and_wave_split_equal_the_restatement(world):
    CK.check_point_slicing(*world)


def test_cell_stride_and_tile_edges(world):
    CK.check_stride_and_tiles(*world)


def test_absent_patches_and_cells_beyond_the_window(world):
    CK.check_absent_and_window(*world)


def test_ties_go_to_the_smaller_index():
    CK.check_ties(F)


def test_every_particle_is_scored_on_its_own_map_and_nothing_changes():
    CK.check_maps_per_particle(F)


def test_invalid_arguments_are_refused_with_the_outputs_untouched(world):
    CK.check_refusals(F, *world)


def test_wide_library():
    CK.check_wide(F)


def test_more_workgroups_than_the_chip(world):
    CK.check_more_workgroups_than_the_chip(*world)


@pytest.fixture(scope="module")
def hall_slam():
    h = CK.slam_with_hall(F)
    assert F.is_device_library(h.engine_origin())
    yield h
    h.close()


def test_class_search_equals_restatement_selection_and_batch_refinement(hall_slam, tmp_path):
    CK.check_class(F, hall_slam, tmp_path)


def test_loc2d_relocalize_from_a_wrong_pose_and_below_the_threshold(tmp_path):
    CK.check_relocalize(F, tmp_path)
