"""-m gpu: the canonical brushfire (cfg.brushfire_mode = 1, k_brushfire_canon) on obstacle events constructed cell by cell
(tests/_bf_canon_checks.py): the per-branch cases of the exact brushfire's checks, additions alone across the wave and thread edges
of the list, levels that take several passes, more new cells in one level than the LDS table holds, the cases in which the kernel
declines at entry and the exact stages do the update, five particles in one launch.  Against the canonical oracle bit for bit,
against the faithful oracle in everything but the offsets of proven ties, and against a brute-force distance transform where a case
only adds.  tests/test_brushfire_canon_sim.py runs the same cases in the lane simulator."""
import pytest

import _bf_canon_checks as CN
import _bf_checks as BF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import iris_lama_amd.ffi as f
    if f.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need the MI355X box (there is no CPU fallback)")
    return f


def test_single_events(F):
    CN.check_single_add(F)
    CN.check_single_add_on_a_patch_corner(F)
    CN.check_single_removal(F)
    CN.check_single_removal_on_a_patch_corner(F)


@pytest.mark.parametrize("which", sorted(BF.PAIR_OFFSETS))
def test_one_of_two_obstacles_removed(F, which):
    CN.check_one_of_two_removed(F, which)


def test_both_removed_and_one_removed_while_a_third_is_added(F):
    CN.check_both_removed(F)
    CN.check_removal_and_addition_in_one_update(F)


def test_same_cell_twice_in_one_update(F):
    CN.check_removed_then_added_again(F)
    CN.check_added_then_removed(F)


def test_cells_equidistant_from_several_obstacles(F):
    assert CN.check_ties_on_addition(F) > 0
    for which in (1, 2):
        CN.check_ties_on_removal(F, which)


def test_ties_with_a_dead_obstacle(F):
    CN.check_tie_with_a_dead_obstacle(F)
    CN.check_tie_with_a_dead_obstacle_among_other_events(F)


@pytest.mark.parametrize("n", CN.ADDS_ONLY)
def test_additions_alone_across_the_wave_and_thread_edges(F, n):
    CN.check_adds_only(F, n)


@pytest.mark.parametrize("m", CN.MULTI_PASS)
def test_level_of_isolated_points_in_one_two_and_three_passes(F, m):
    CN.check_grid_in_passes(F, m)


def test_more_new_obstacle_cells_in_one_scan_than_the_table_holds(F):
    CN.check_more_new_obstacles_than_the_table(F)


def test_reach_of_32_cells_is_the_last_the_kernel_takes(F):
    CN.check_reach_of_32_cells_runs_canonical(F)


def test_reach_of_33_cells_falls_through_to_the_exact_stages(F):
    CN.check_reach_of_33_cells_falls_through(F)


def test_wide_library_falls_through_to_the_exact_stages(F):
    CN.check_wide_library_falls_through(F)


def test_more_raise_entries_than_half_the_queue_fall_through_to_the_exact_stages(F):
    CN.check_more_raise_entries_than_half_the_queue(F)


def test_more_lower_entries_than_half_the_queue_fall_through_to_the_exact_stages(F):
    CN.check_more_lower_entries_than_half_the_queue(F)

def test_five_particles_with_different_events_in_one_launch(F):
    CN.check_five_particles(F)
