"""-m gpu: the cycle of a particle group of the grouped step schedule (lama_hip_pf_match_and_map) -- poses and scan transforms as
launch arguments, k_pack_group clearing what it has packed, k_occ_reverse_dir over the rows of the mapped box.  The checks are tests/_group_cycle_checks.py's; the existing
suites (test_step_groups_gpu, test_window_gpu, test_gpu_parity) cover window moves, clean aborts, the wrap-guard probe and
deferred errors under the same path."""
import pytest

import _group_cycle_checks as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import iris_lama_amd.ffi as f
    if f.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need the MI355X box (there is no CPU fallback)")
    return f


@pytest.mark.parametrize("P,groups,blocks,every_scan", [(1, None, 1, True), (3, None, 3, False), (6, None, 3, True), (30, None, 3, False),
                                                        (17, 2, 2, True), (34, 2, 2, False)])
def test_grouped_equals_single_stream_equals_oracle(F, P, groups, blocks, every_scan):
    """(17 in two groups: blocks of 16 -- the largest whose tables are launch arguments -- and 1; 34: blocks of 24, which copies its
    poses and transforms into d_poses / d_tfs, and 10)"""
    G.check_grouped_equals_single_stream_equals_oracle(F, P, groups, blocks, every_scan=every_scan)


@pytest.mark.parametrize("P,groups,blocks", [(1, None, 1), (17, 2, 2), (34, 2, 2)])
def test_step_results_equal_the_single_stream_schedules(F, P, groups, blocks):
    G.check_results_bit_equal(F, P, groups, blocks)


@pytest.mark.parametrize("direction", ["+y", "-y"])
def test_directory_rows_of_the_mapped_box(F, direction):
    seen = G.check_directory_rows(F, direction)
    if direction == "+y":
        assert min(lo for lo, hi, w in seen) == 0, seen                    # the box starts on the window's row 0
    else:
        assert any(hi == w - 1 for lo, hi, w in seen), seen               # the box ends on the window's last row
