"""The device solver of SimplePGO's damped system (iris_lama_amd/csrc/lama_pgo_pcg.h) and lama::SimplePGO's loop over it under the
lane-level simulator of tests/sim (the kernel SOURCES compiled for the host, see tests/test_kernel_sim.py): runs where there is no GPU.
The checks and their bounds are in tests/_pgo_pcg_checks.py, shared with tests/test_pgo_pcg_gpu.py; the numpy restatement the
solves are compared with bit for bit is tests/_pgo_pcg.py."""
import pytest

import _pgo_pcg_checks as PC
import _testhost
from test_match_batch_sim import SIM_LIB, Fsim  # noqa: F401  (the fixture)


@pytest.fixture(scope="module")
def Fhost(Fsim):
    """lama::SimplePGO of the test-suite's host build, bound to the simulator as its device library (as tests/test_pgo_sim.py does:
    SimplePGO keeps no handle to ask, so the binding is read from a LidarOdometry2D made under the same override)."""
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


def test_pose_counts_on_the_workgroup_edges(Fsim):
    PC.check_pose_counts(Fsim)


def test_rows_without_lower_or_transposed_blocks_a_hub_and_a_repeated_pair(Fsim):
    PC.check_row_shapes(Fsim)


def test_more_than_64_partials_per_dot_product(Fsim):
    PC.check_many_partials(Fsim)


def test_the_batch_length_does_not_change_the_result(Fsim):
    PC.check_batch_independence(Fsim)


def test_the_iteration_cap_stops_the_solve_where_the_restatement_stops(Fsim):
    PC.check_cap(Fsim)


def test_an_untouched_pose_is_a_breakdown_and_lambda_zero_converges_behind_a_prior(Fsim):
    PC.check_breakdown(Fsim)


def test_zero_right_hand_side_converges_at_once(Fsim):
    PC.check_zero_right_hand_side(Fsim)


def test_call_sequence_and_argument_refusals(Fsim):
    PC.check_state_rules(Fsim)


def test_two_graphs_alive_at_once(Fsim):
    PC.check_two_graphs(Fsim)


def test_the_solver_only_reads_the_system(Fsim):
    PC.check_system_is_only_read(Fsim)


@pytest.mark.parametrize("N,loops,with_fixed,push", [(40, 20, False, 0.0), (40, 20, True, 0.0), (120, 150, False, 0.5)])
def test_optimize_on_the_device_solver_follows_minisams_levenberg_marquardt(Fhost, N, loops, with_fixed, push):
    PC.check_loop_on_pcg(Fhost, N, loops, with_fixed, push)


def test_graph_at_its_optimum_returns_false_after_lambda_runs_out(Fhost):
    PC.check_loop_at_the_optimum(Fhost)


def test_a_solve_that_reaches_its_cap_falls_back_to_the_host_factorisation(Fhost):
    PC.check_forced_fallback(Fhost)


def test_the_default_call_reports_what_it_always_did(Fhost):
    PC.check_default_path(Fhost)
