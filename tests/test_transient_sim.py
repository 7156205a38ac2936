"""lama_hip_pf_patch_ids / lama_hip_pf_delete_patches and the log-odds cells of k_raycast case by case (tests/_transient_checks.py),
with the kernels executed lane by lane on the CPU (tests/sim, see tests/test_kernel_sim.py): the compaction on every patch of a
block alone, in every ordered pair, all at once and in a list of duplicates, absent and out-of-window ids; on a resampled
particle; then what the kernels that run afterwards make of it -- obstacle offsets into a deleted patch (raise and the tie of
lower), the vacated slot's next tenant, clones, exported particles, a grouped step, a moved window -- and the log-odds arithmetic
at its clamps and zero crossings.  Bit for bit against the download before the call and against the oracle.
tests/test_transient_gpu.py runs the same cases on the device.

The simulator pays for every cell the brushfire floods: the distance maps of the frequency-policy cases reach 5 cells here
(tests/test_window_sim.py); the lidar-odometry cases keep the 20 cells the oracle's class has, on scans of a few beams."""
import pytest

import _transient_checks as T
from test_kernel_sim import Fsim  # noqa: F401  (the fixture)

L2_MAX = 0.25


@pytest.mark.parametrize("name", T.DELETION_CASES)
def test_deletion_leaves_the_download_minus_the_ids(Fsim, name):
    T.check_deletions(Fsim, name, l2_max=L2_MAX)


def test_empty_and_refused_calls_change_nothing(Fsim):
    T.check_arguments(Fsim, l2_max=L2_MAX)


def test_deletion_on_a_particle_whose_home_is_not_its_index(Fsim):
    T.check_deletion_on_a_resampled_particle(Fsim, l2_max=L2_MAX)


def test_raise_wave_reads_an_obstacle_in_a_deleted_patch(Fsim):
    T.check_dangling_raise_pf(Fsim, l2_max=L2_MAX)


def test_raise_wave_reads_an_obstacle_in_a_deleted_patch_lidar_odometry(Fsim):
    T.check_dangling_raise_lidar(Fsim)


def test_tie_of_lower_reads_an_obstacle_in_a_deleted_patch(Fsim):
    T.check_dangling_lower_tie(Fsim, l2_max=L2_MAX)


def test_vacated_slot_is_the_next_patch(Fsim):
    T.check_vacated_slot_reused(Fsim, l2_max=L2_MAX)


def test_clones_of_a_compacted_region(Fsim):
    T.check_clone_after_a_deletion(Fsim, l2_max=L2_MAX)


def test_exported_particle_after_a_deletion(Fsim):
    T.check_export_after_a_deletion(Fsim, l2_max=L2_MAX)


def test_deletion_waits_for_the_groups(Fsim, monkeypatch):
    monkeypatch.setenv("LAMA_HIP_STEP_GROUPS", "2")
    T.check_deletion_waits_for_the_groups(Fsim, 2, l2_max=L2_MAX)


def test_deletion_after_a_window_move(Fsim):
    T.check_deletion_after_a_window_move(Fsim, l2_max=L2_MAX)


def test_log_odds_clamps_and_zero_crossings(Fsim):
    T.check_log_odds_clamps_and_crossings(Fsim)
