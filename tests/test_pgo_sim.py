"""The six pose-graph kernels of iris_lama_amd/csrc/lama_pgo.h and lama::SimplePGO's whole loop under the lane-level simulator of
tests/sim (the kernel SOURCES compiled for the host, see tests/test_kernel_sim.py): runs where there is no GPU.  The checks and
their bounds are in tests/_pgo_checks.py, shared with tests/test_pgo_kernels_gpu.py.  The simulator links the host's libm and
everything is built with -ffp-contract=off, so the oracle's values are the kernels' bit for bit (same_libm)."""
import numpy as np
import pytest

import _oracle as O
import _pgo_checks as P
import _pgo_lm as LM
import _testhost
from test_match_batch_sim import SIM_LIB, Fsim  # noqa: F401  (the fixture)


@pytest.fixture(scope="module")
def Fhost(Fsim):
    """lama::SimplePGO of the test-suite's host build, bound to the simulator as its device library.  SimplePGO keeps no handle
    to ask, so the binding is read from a LidarOdometry2D made under the same override: both take defaultEngine()."""
    _testhost.set_engine_library(SIM_LIB)
    try:
        assert Fsim.HOST_LIB == _testhost.TEST_HOST
        lo = Fsim.LidarOdometry2D()
        try:
            assert lo.engine_origin() == SIM_LIB
        finally:
            lo.close()
        yield Fsim
    finally:
        _testhost.set_engine_library(None)


def test_log_takes_the_small_angle_branch_just_below_its_threshold_only(Fsim):
    P.check_log_branch(Fsim, same_libm=True)


def test_rotation_errors_next_to_the_cut_of_atan2(Fsim):
    P.check_rotation_cut(Fsim, same_libm=True)


def test_factor_and_pose_counts_on_the_block_edges(Fsim):
    P.check_block_edges(Fsim, same_libm=True)


def test_more_than_64_partial_sums(Fsim):
    P.check_many_partials(Fsim, same_libm=True)


def test_hub_and_repeated_pair_add_up_in_factor_order(Fsim):
    P.check_hub(Fsim, same_libm=True)


def test_retract_at_the_branch_of_exp_and_next_to_the_cut(Fsim):
    P.check_retract(Fsim, same_libm=True)


def test_accept_without_a_pending_candidate_is_refused(Fsim):
    P.check_accept_needs_a_candidate(Fsim)


def test_two_graphs_alive_at_once(Fsim):
    P.check_two_graphs_do_not_disturb_each_other(Fsim)


@pytest.mark.parametrize("N,loops,with_fixed,push", [(40, 20, False, 0.0), (40, 20, True, 0.0), (120, 150, False, 0.5)])
def test_optimize_follows_minisams_levenberg_marquardt(Fhost, N, loops, with_fixed, push):
    nodes, edges, fixed = P.loop_inputs(N, loops, with_fixed, push)
    ok, rep, ref = P.check_loop(Fhost, nodes, edges, fixed, need_rejection=push != 0.0)
    assert ok


def test_graph_at_its_optimum_returns_false_after_lambda_runs_out(Fhost):
    node = O.se2(1.5, -0.5, 0.3)
    ok, rep, ref = P.check_loop(Fhost, node[None], [], [])
    assert not ok and rep["status"] == LM.ERROR_INCREASE == ref["status"]
    assert rep["iterations"] == 1 and list(rep["trace"]) == ref["trace"] and set(ref["trace"]) == {LM.REJECTED}

