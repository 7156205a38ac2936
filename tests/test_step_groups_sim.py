"""The host side of the grouped step schedule (lama_hip_pf_match_and_map) on the lane simulator (tests/sim, see
tests/test_kernel_sim.py): group blocks, the per-group words and lists, the block a group's results and status travel in, the
deferred status, the drain in front of every other entry point, the window check per block, the repeat of a cleanly aborted
update.  The simulator runs every launch to completion in program order, so it checks the bookkeeping and the indexing, not the
overlap; tests/test_step_groups_gpu.py runs the same checks, and the host class, on the device.

The simulator pays for every cell the brushfire floods: the distance maps reach 5 cells here (tests/test_window_sim.py)."""
import pytest

import _step_group_checks as S
from test_kernel_sim import Fsim  # noqa: F401  (the fixture)

L2_MAX = 0.25


@pytest.mark.parametrize("groups,every_scan", [(2, True), (3, False)])
def test_window_moves_and_grows_under_groups(Fsim, monkeypatch, groups, every_scan):
    monkeypatch.setenv("LAMA_HIP_STEP_GROUPS", str(groups))
    S.check_window_moves_and_grows(Fsim, groups, l2_max=L2_MAX, every_scan=every_scan)


@pytest.mark.parametrize("groups,every_scan", [(3, True), (2, False)])
def test_clean_abort_grows_the_arenas_under_groups(Fsim, monkeypatch, groups, every_scan):
    monkeypatch.setenv("LAMA_HIP_STEP_GROUPS", str(groups))
    S.check_clean_abort_grows_the_arenas(Fsim, groups, l2_max=L2_MAX, every_scan=every_scan)


@pytest.mark.parametrize("P", [1, 2, 5])
def test_more_groups_than_particles_and_uneven_blocks(Fsim, monkeypatch, P):
    """four groups for one, two and five particles: empty groups, one-particle groups, blocks of 1 and 2"""
    monkeypatch.setenv("LAMA_HIP_STEP_GROUPS", "4")
    S.check_window_moves_and_grows(Fsim, {1: 1, 2: 2, 5: 3}[P], P=P, stops=(4.0, 8.0), l2_max=L2_MAX, every_scan=False, must_grow=False)      # (5: 2 + 2 + 1)


def test_override_one_is_the_single_stream_schedule(Fsim, monkeypatch):
    monkeypatch.setenv("LAMA_HIP_STEP_GROUPS", "1")
    S.check_window_moves_and_grows(Fsim, 1, stops=(4.0, 8.0), l2_max=L2_MAX, must_grow=False)
