"""The canonical brushfire (cfg.brushfire_mode = 1, k_brushfire_canon) on obstacle events constructed cell by cell
(tests/_bf_canon_checks.py), executed lane by lane on the CPU (tests/sim, see tests/test_kernel_sim.py): the per-branch cases of the
exact brushfire's checks, additions alone across the wave and thread edges of the list (the path on which a store to LDS once had no
barrier behind it), levels that take several passes, more new cells in one level than the LDS table holds, the cases in which the
kernel declines at entry and the exact stages do the update, five particles in one launch.  Against the canonical oracle bit for
bit, against the faithful oracle in everything but the offsets of proven ties, and against a brute-force distance transform where a
case only adds.  tests/test_brushfire_canon_gpu.py runs the same cases on the device."""
import pytest

import _bf_canon_checks as CN
import _bf_checks as BF
from test_kernel_sim import Fsim, Fsim_wide  # noqa: F401  (the fixtures)


def test_single_events(Fsim):
    CN.check_single_add(Fsim)
    CN.check_single_add_on_a_patch_corner(Fsim)
    CN.check_single_removal(Fsim)
    CN.check_single_removal_on_a_patch_corner(Fsim)


@pytest.mark.parametrize("which", sorted(BF.PAIR_OFFSETS))
def test_one_of_two_obstacles_removed(Fsim, which):
    CN.check_one_of_two_removed(Fsim, which)


def test_both_removed_and_one_removed_while_a_third_is_added(Fsim):
    CN.check_both_removed(Fsim)
    CN.check_removal_and_addition_in_one_update(Fsim)


def test_same_cell_twice_in_one_update(Fsim):
    CN.check_removed_then_added_again(Fsim)
    CN.check_added_then_removed(Fsim)


def test_cells_equidistant_from_several_obstacles(Fsim):
    assert CN.check_ties_on_addition(Fsim) > 0
    for which in (1, 2):
        CN.check_ties_on_removal(Fsim, which)


def test_ties_with_a_dead_obstacle(Fsim):
    CN.check_tie_with_a_dead_obstacle(Fsim)
    CN.check_tie_with_a_dead_obstacle_among_other_events(Fsim)


@pytest.mark.parametrize("n", CN.ADDS_ONLY)
def test_additions_alone_across_the_wave_and_thread_edges(Fsim, n):
    CN.check_adds_only(Fsim, n)


@pytest.mark.parametrize("m", CN.MULTI_PASS)
def test_level_of_isolated_points_in_one_two_and_three_passes(Fsim, m):
    CN.check_grid_in_passes(Fsim, m)


def test_more_new_obstacle_cells_in_one_scan_than_the_table_holds(Fsim):
    CN.check_more_new_obstacles_than_the_table(Fsim)


def test_reach_of_32_cells_is_the_last_the_kernel_takes(Fsim):
    CN.check_reach_of_32_cells_runs_canonical(Fsim)


def test_reach_of_33_cells_falls_through_to_the_exact_stages(Fsim):
    CN.check_reach_of_33_cells_falls_through(Fsim)


def test_wide_library_falls_through_to_the_exact_stages(Fsim_wide):
    CN.check_wide_library_falls_through(Fsim_wide)


def test_more_raise_entries_than_half_the_queue_fall_through_to_the_exact_stages(Fsim):
    CN.check_more_raise_entries_than_half_the_queue(Fsim)


def test_more_lower_entries_than_half_the_queue_fall_through_to_the_exact_stages(Fsim):
    CN.check_more_lower_entries_than_half_the_queue(Fsim)

def test_five_particles_with_different_events_in_one_launch(Fsim):
    CN.check_five_particles(Fsim)
