"""-m gpu: lama_hip_pf_patch_ids / lama_hip_pf_delete_patches and the log-odds cells of k_raycast case by case
(tests/_transient_checks.py) on the device: the compaction on every patch of a block alone, in every ordered pair, all at once
and in a list of duplicates, absent and out-of-window ids, with refused and empty calls, and on a particle whose home is not its
index; then what the kernels that run afterwards make of a compacted region -- obstacle offsets into a deleted patch read by the
raise wave (frequency policy and the LidarOdometry2D configuration) and by the tie of lower(), the vacated slot's next tenant,
clones, an exported particle in a context with another window origin, a deletion right behind a grouped step, a moved window --
and the log-odds arithmetic at its clamps and zero crossings, ending in the transient step's own deletion.  The distance maps
reach their default 10 cells here, 20 in the lidar-odometry cases.  Bit for bit against the download before the call and
against the oracle; every case asserts on the oracle that it reaches the situation it names."""
import pytest

import _transient_checks as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import iris_lama_amd.ffi as f
    if f.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need the MI355X box (there is no CPU fallback)")
    return f


@pytest.mark.parametrize("name", T.DELETION_CASES)
def test_deletion_leaves_the_download_minus_the_ids(F, name):
    T.check_deletions(F, name)


def test_empty_and_refused_calls_change_nothing(F):
    T.check_arguments(F)


def test_deletion_on_a_particle_whose_home_is_not_its_index(F):
    T.check_deletion_on_a_resampled_particle(F)


def test_raise_wave_reads_an_obstacle_in_a_deleted_patch(F):
    T.check_dangling_raise_pf(F)


def test_raise_wave_reads_an_obstacle_in_a_deleted_patch_lidar_odometry(F):
    T.check_dangling_raise_lidar(F)


def test_tie_of_lower_reads_an_obstacle_in_a_deleted_patch(F):
    T.check_dangling_lower_tie(F)


def test_vacated_slot_is_the_next_patch(F):
    T.check_vacated_slot_reused(F)


def test_clones_of_a_compacted_region(F):
    T.check_clone_after_a_deletion(F)


def test_exported_particle_after_a_deletion(F):
    T.check_export_after_a_deletion(F)


@pytest.mark.parametrize("groups", [2, 3])
def test_deletion_waits_for_the_groups(F, monkeypatch, groups):
    monkeypatch.setenv("LAMA_HIP_STEP_GROUPS", str(groups))
    T.check_deletion_waits_for_the_groups(F, groups)


def test_deletion_after_a_window_move(F):
    T.check_deletion_after_a_window_move(F)


def test_log_odds_clamps_and_zero_crossings(F):
    T.check_log_odds_clamps_and_crossings(F)
