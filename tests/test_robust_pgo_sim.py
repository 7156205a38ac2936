"""The per-factor robust losses of the device pose graph (k_pgo_factors_robust, k_pgo_error_robust of iris_lama_amd/csrc/lama_pgo.h)
and lama::PoseGraph2D's whole loop under the lane-level simulator of tests/sim (the kernel SOURCES compiled for the host): runs where
there is no GPU.  The checks are in tests/_pgo_robust_checks.py, shared with tests/test_robust_pgo_gpu.py; the simulator links the
host's libm and everything is built with -ffp-contract=off, so the restatement's values are the kernels' bit for bit (same_libm)."""
import pytest

import _pgo_robust_checks as RC
from test_match_batch_sim import Fsim  # noqa: F401  (the fixture)
from test_pgo_sim import Fhost  # noqa: F401  (lama::PoseGraph2D of the test-suite's host build, bound to the simulator)


def test_golden_cases_equal_the_restatement_and_minisam_bit_for_bit(Fsim):
    RC.check_golden_cases(Fsim, same_libm=True)


def test_robust_factors_on_both_sides_of_the_block_edge(Fsim):
    RC.check_block_edges(Fsim, same_libm=True)


def test_hub_of_alternating_robust_and_plain_factors_adds_up_in_factor_order(Fsim):
    RC.check_hub(Fsim, same_libm=True)


def test_error_kernel_applies_the_factor_kernels_weight(Fsim):
    RC.check_try_step_equals_the_factor_kernel(Fsim, same_libm=True)


def test_create_robust_without_a_robust_factor_is_create_output_for_output(Fsim):
    RC.check_no_robust_factor_is_create(Fsim)


def test_refused_losses_name_the_factor_and_weights_need_a_linearisation(Fsim):
    RC.check_refusals(Fsim)


def test_ring_seed_meets_the_input_condition():
    """RING_SEED (tests/_pgo_robust_checks.py): the numpy Levenberg-Marquardt alone -- no device code -- returns SUCCESS, keeps every
    false closure below a weight of 1 and every true one at 1, and ends closer to the truth than without a loss."""
    assert RC.ring_meets_the_input_condition()
    assert not any(RC.ring_meets_the_input_condition(seed) for seed in range(RC.RING_SEED))        # the smallest such seed


@pytest.mark.parametrize("solver", ["ldlt", "pcg"])
def test_optimize_holds_false_closures_back_as_the_numpy_loop_does(Fhost, solver):
    RC.check_ring(Fhost, solver)


def test_invalid_graphs_return_false_with_nothing_run(Fhost):
    RC.check_host_class_refusals(Fhost)
