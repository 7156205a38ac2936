"""-m gpu: the six pose-graph kernels of iris_lama_amd/csrc/lama_pgo.h on the device at their branches, block edges and hubs.  The
checks and their bounds are in tests/_pgo_checks.py, shared with the lane-simulator run of tests/test_pgo_sim.py; here atan2, sin
and cos are OCML's, so err, b and the retracted poses are within K_LIBM eps of the sum of their terms' magnitudes instead of
bit-equal, while everything made of the Jacobians alone (Hoff, Hdiag, the assembled blocks) and the order of every sum stays
bit-equal."""
import pytest

import _pgo_checks as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import iris_lama_amd.ffi as f
    if f.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need the MI355X box (there is no CPU fallback)")
    return f


def test_log_takes_the_small_angle_branch_just_below_its_threshold_only(F):
    P.check_log_branch(F, same_libm=False)


def test_rotation_errors_next_to_the_cut_of_atan2(F):
    P.check_rotation_cut(F, same_libm=False)


def test_factor_and_pose_counts_on_the_block_edges(F):
    P.check_block_edges(F, same_libm=False)


def test_more_than_64_partial_sums(F):
    P.check_many_partials(F, same_libm=False)


def test_hub_and_repeated_pair_add_up_in_factor_order(F):
    P.check_hub(F, same_libm=False)


def test_retract_at_the_branch_of_exp_and_next_to_the_cut(F):
    P.check_retract(F, same_libm=False)


def test_accept_without_a_pending_candidate_is_refused(F):
    P.check_accept_needs_a_candidate(F)


def test_two_graphs_alive_at_once(F):
    P.check_two_graphs_do_not_disturb_each_other(F)
