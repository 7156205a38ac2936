"""-m gpu: the exact brushfire on obstacle events constructed cell by cell (tests/_bf_checks.py): single additions and removals in
open space and on a patch corner, one of two obstacles removed at five distances, the same cell removed and added in one update,
cells equidistant from several obstacles with one of them removed (a tie with a dead obstacle among them), patches that evict each
other from the directory cache, the size thresholds of the three stages at entry and in mid-run, a reach of 127 cells in the narrow
library and of 128 and 255 in the wide one, five particles that end in different stages in one launch.  Against the oracle, bit
for bit, in the wave-pair and the one-wave form; every case asserts from the oracle's statistics and the device counters that it
reached its regime."""
import pytest

import _bf_checks as BF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import iris_lama_amd.ffi as f
    if f.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need the MI355X box (there is no CPU fallback)")
    return f


@pytest.mark.parametrize("waves", BF.WAVES)
def test_single_events(F, waves):
    BF.check_single_add(F, waves)
    BF.check_single_add_on_a_patch_corner(F, waves)
    BF.check_single_removal(F, waves)
    BF.check_single_removal_on_a_patch_corner(F, waves)


@pytest.mark.parametrize("waves", BF.WAVES)
@pytest.mark.parametrize("which", sorted(BF.PAIR_OFFSETS))
def test_one_of_two_obstacles_removed(F, which, waves):
    BF.check_one_of_two_removed(F, waves, which)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_both_removed_and_one_removed_while_a_third_is_added(F, waves):
    BF.check_both_removed(F, waves)
    BF.check_removal_and_addition_in_one_update(F, waves)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_same_cell_twice_in_one_update(F, waves):
    BF.check_removed_then_added_again(F, waves)
    BF.check_added_then_removed(F, waves)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_cells_equidistant_from_several_obstacles(F, waves):
    BF.check_ties_on_addition(F, waves)
    for which in (1, 2, 4):
        BF.check_ties_on_removal(F, waves, which)
    BF.check_tie_with_a_dead_obstacle(F, waves)
    BF.check_tie_with_a_dead_obstacle_among_other_events(F, waves)


@pytest.mark.parametrize("n", [2, 3])
def test_patches_that_evict_each_other_from_the_directory_cache(F, n):
    BF.check_directory_cache_thrash(F, n)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_patches_that_evict_each_other_while_their_discs_are_raised(F, waves):
    BF.check_directory_cache_thrash_on_removal(F, waves)


def test_additions_across_the_first_stage_queue_at_entry(F):
    BF.check_additions_at_entry(F, (1019, 1020, 1021, 1022), BF.LQ)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_removals_across_the_first_stage_queue_at_entry(F, waves):
    BF.check_removals_at_entry(F, waves, (251, 252, 253, 254), BF.RQ)


def test_wall_outgrows_the_lower_window_in_mid_lower(F):
    BF.check_wall_hands_over_in_mid_lower(F, BF.WALL_SWEEP)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_grid_of_points_drawn_by_a_scan_outgrows_the_lower_window(F, waves):
    BF.check_grid_through_a_scan(F, waves)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_raise_queue_outgrows_the_first_stage_in_mid_raise(F, waves):
    BF.check_raise_queue_outgrows_the_first_stage(F, waves)


def test_wall_grows_through_2047_entries_in_the_resume_stage(F):
    BF.check_wall_in_the_resume_stage(F)


def test_additions_across_the_resume_stage_queue_into_the_slow_stage(F):
    BF.check_additions_at_entry(F, (8187, 8188, 8189, 8190), BF.LQ_BIG)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_removals_across_the_resume_stage_queue_into_the_slow_stage(F, waves):
    BF.check_removals_at_entry(F, waves, (2043, 2044, 2045, 2046), BF.RQ_BIG)


@pytest.mark.parametrize("l2_max", [6.35, 6.4, 12.75])
def test_reach_to_the_ends_of_the_offset_fields(F, l2_max):
    BF.check_reach(F, l2_max)


@pytest.mark.parametrize("l2_max", [6.35, 6.4, 12.75])
def test_two_tied_obstacles_at_full_reach(F, l2_max):
    BF.check_reach(F, l2_max, cells=((0, 0), (6, 2)), what="two tied")


@pytest.mark.parametrize("waves", BF.WAVES)
def test_removal_at_a_reach_of_127_cells(F, waves):
    BF.check_reach_removal(F, waves)


@pytest.mark.parametrize("waves", BF.WAVES)
def test_five_particles_end_in_different_stages(F, waves):
    BF.check_five_particles(F, waves)


def test_five_particles_with_one_of_them_routed(F, monkeypatch):
    monkeypatch.setenv("LAMA_HIP_BF_ROUTE", "1,0,150,1")
    BF.check_five_particles(F, 2, route=True)
