"""The exact brushfire on obstacle events constructed cell by cell (tests/_bf_checks.py), executed lane by lane on the CPU
(tests/sim, see tests/test_kernel_sim.py): single additions and removals in open space and on a patch corner, one of two
obstacles removed at five distances, the same cell removed and added in one update, cells equidistant from several obstacles with
one of them removed (a tie with a dead obstacle among them), patches that evict each other from the directory cache, the size
thresholds of the three stages at entry and in mid-run, a reach of 127 cells (narrow build: one obstacle, two tied ones, a
removal) and of 128 (wide build: one obstacle, two tied ones), five particles that end in different stages in one launch.
Against the oracle, bit for bit, in the wave-pair and the one-wave form; every case asserts from the oracle's statistics and the
device counters that it reached its regime.  tests/test_brushfire_gpu.py runs the same cases on the device, and the reach of 255
cells (2 x 10^5 pops and more) there only."""
import pytest

import _bf_checks as BF
import _reference as R
from test_kernel_sim import Fsim, Fsim_wide  # noqa: F401  (the fixtures)

needs_reference = pytest.mark.skipif(not R.available(), reason="the compiled reference (oracle/_ref, made by build()) is not there")


@needs_reference
def test_oracle_equals_the_reference_on_the_constructed_event_sequences():
    BF.check_oracle_against_the_reference()


@pytest.mark.parametrize("waves", BF.WAVES)
def test_single_events(Fsim, waves):
    BF.check_single_add(Fsim, waves)
    BF.check_single_add_on_a_patch_corner(Fsim, waves)
    BF.check_single_removal(Fsim, waves)
    BF.check_single_removal_on_a_patch_corner(Fsim, waves)


@pytest.mark.parametrize("waves", BF.WAVES)
@pytest.mark.parametrize("which", sorted(BF.PAIR_OFFSETS))
def test_one_of_two_obstacles_removed(Fsim, which, waves):
    BF.check_one_of_two_removed(Fsim, waves, which)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_both_removed_and_one_removed_while_a_third_is_added(Fsim, waves):
    BF.check_both_removed(Fsim, waves)
    BF.check_removal_and_addition_in_one_update(Fsim, waves)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_same_cell_twice_in_one_update(Fsim, waves):
    BF.check_removed_then_added_again(Fsim, waves)
    BF.check_added_then_removed(Fsim, waves)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_cells_equidistant_from_several_obstacles(Fsim, waves):
    BF.check_ties_on_addition(Fsim, waves)
    for which in (1, 2, 4):
        BF.check_ties_on_removal(Fsim, waves, which)
    BF.check_tie_with_a_dead_obstacle(Fsim, waves)
    BF.check_tie_with_a_dead_obstacle_among_other_events(Fsim, waves)


@pytest.mark.parametrize("n", [2, 3])
def test_patches_that_evict_each_other_from_the_directory_cache(Fsim, n):
    BF.check_directory_cache_thrash(Fsim, n)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_patches_that_evict_each_other_while_their_discs_are_raised(Fsim, waves):
    BF.check_directory_cache_thrash_on_removal(Fsim, waves)


def test_additions_across_the_first_stage_queue_at_entry(Fsim):
    BF.check_additions_at_entry(Fsim, (1019, 1020, 1021, 1022), BF.LQ)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_removals_across_the_first_stage_queue_at_entry(Fsim, waves):
    BF.check_removals_at_entry(Fsim, waves, (251, 252, 253, 254), BF.RQ)


def test_wall_outgrows_the_lower_window_in_mid_lower(Fsim):
    BF.check_wall_hands_over_in_mid_lower(Fsim, BF.WALL_SWEEP)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_grid_of_points_drawn_by_a_scan_outgrows_the_lower_window(Fsim, waves):
    BF.check_grid_through_a_scan(Fsim, waves)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_raise_queue_outgrows_the_first_stage_in_mid_raise(Fsim, waves):
    BF.check_raise_queue_outgrows_the_first_stage(Fsim, waves)


def test_wall_grows_through_2047_entries_in_the_resume_stage(Fsim):
    BF.check_wall_in_the_resume_stage(Fsim)


def test_additions_across_the_resume_stage_queue_into_the_slow_stage(Fsim):
    BF.check_additions_at_entry(Fsim, (8187, 8188, 8189, 8190), BF.LQ_BIG)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_removals_across_the_resume_stage_queue_into_the_slow_stage(Fsim, waves):
    BF.check_removals_at_entry(Fsim, waves, (2043, 2044, 2045, 2046), BF.RQ_BIG)


def test_reach_of_127_cells_in_the_narrow_build(Fsim):
    BF.check_reach(Fsim, 6.35)


def test_reach_of_128_cells_in_the_wide_build(Fsim_wide):
    BF.check_reach(Fsim_wide, 6.4)


def test_two_tied_obstacles_at_a_reach_of_127_cells(Fsim):
    BF.check_reach(Fsim, 6.35, cells=((0, 0), (6, 2)), what="two tied")


def test_two_tied_obstacles_at_a_reach_of_128_cells(Fsim_wide):
    BF.check_reach(Fsim_wide, 6.4, cells=((0, 0), (6, 2)), what="two tied")


@pytest.mark.parametrize("waves", BF.WAVES)
def test_removal_at_a_reach_of_127_cells(Fsim, waves):
    BF.check_reach_removal(Fsim, waves)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_five_particles_end_in_different_stages(Fsim, waves):
    BF.check_five_particles(Fsim, waves)


def test_five_particles_with_one_of_them_routed(Fsim, monkeypatch):
    monkeypatch.setenv("LAMA_HIP_BF_ROUTE", "1,0,150,1")
    BF.check_five_particles(Fsim, 2, route=True)
