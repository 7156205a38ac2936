"""The cycle of a particle group (tests/_group_cycle_checks.py) on the lane simulator (tests/sim, see tests/test_kernel_sim.py):
poses and scan transforms as launch arguments beside the copy path, k_pack_group clearing what it has packed, the directory rows of
k_occ_reverse_dir.  The simulator runs every launch to completion in program order: it checks the indexing and the bookkeeping of
the clearing, not the ordering between streams;
tests/test_group_cycle_gpu.py runs the same checks on the device.

The simulator pays for every cell the brushfire floods: the distance maps reach 5 cells here (tests/test_window_sim.py)."""
import pytest

import _group_cycle_checks as G
from test_kernel_sim import Fsim  # noqa: F401  (the fixture)

L2_MAX = 0.25


@pytest.mark.parametrize("P,groups,blocks,every_scan", [(1, None, 1, True), (3, None, 3, False), (6, None, 3, True), (17, 2, 2, False)])
def test_grouped_equals_single_stream_equals_oracle(Fsim, P, groups, blocks, every_scan):
    """(17 in two groups: a block of 16, the largest whose tables are launch arguments, and a block of 1)"""
    G.check_grouped_equals_single_stream_equals_oracle(Fsim, P, groups, blocks, l2_max=L2_MAX, stops=G.STOPS[:4], every_scan=every_scan)


def test_copy_path_beside_the_argument_path(Fsim):
    """34 particles in two groups: a block of 24 (poses and transforms copied into d_poses / d_tfs) and one of 10 (launch arguments)"""
    G.check_results_bit_equal(Fsim, 34, 2, 2, l2_max=L2_MAX, stops=G.STOPS[:2])


@pytest.mark.parametrize("P,groups,blocks", [(1, None, 1), (17, 2, 2)])
def test_step_results_equal_the_single_stream_schedules(Fsim, P, groups, blocks):
    G.check_results_bit_equal(Fsim, P, groups, blocks, l2_max=L2_MAX)


@pytest.mark.parametrize("direction", ["+y", "-y"])
def test_directory_rows_of_the_mapped_box(Fsim, direction):
    seen = G.check_directory_rows(Fsim, direction, l2_max=L2_MAX)
    if direction == "+y":
        assert min(lo for lo, hi, w in seen) == 0, seen                    # the box starts on the window's row 0
    else:
        assert any(hi == w - 1 for lo, hi, w in seen), seen               # the box ends on the window's last row
