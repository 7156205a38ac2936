"""-m gpu: the device solver of SimplePGO's damped system (iris_lama_amd/csrc/lama_pgo_pcg.h) and lama::SimplePGO's loop over it on
the device.  The checks and their bounds are in tests/_pgo_pcg_checks.py, shared with the lane-simulator run of
tests/test_pgo_pcg_sim.py; the solver holds no libm call, so its results are bit-equal to the numpy restatement tests/_pgo_pcg.py here
as they are there."""
import pytest

import _pgo_pcg_checks as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import iris_lama_amd.ffi as f
    if f.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need the MI355X box (there is no CPU fallback)")
    return f


def test_pose_counts_on_the_workgroup_edges(F):
    PC.check_pose_counts(F)


def test_rows_without_lower_or_transposed_blocks_a_hub_and_a_repeated_pair(F):
    PC.check_row_shapes(F)


def test_more_than_64_partials_per_dot_product(F):
    PC.check_many_partials(F)


def test_the_batch_length_does_not_change_the_result(F):
    PC.check_batch_independence(F)


def test_the_iteration_cap_stops_the_solve_where_the_restatement_stops(F):
    PC.check_cap(F)


def test_an_untouched_pose_is_a_breakdown_and_lambda_zero_converges_behind_a_prior(F):
    PC.check_breakdown(F)


def test_zero_right_hand_side_converges_at_once(F):
    PC.check_zero_right_hand_side(F)


def test_call_sequence_and_argument_refusals(F):
    PC.check_state_rules(F)


def test_two_graphs_alive_at_once(F):
    PC.check_two_graphs(F)


def test_the_solver_only_reads_the_system(F):
    PC.check_system_is_only_read(F)


@pytest.mark.parametrize("N,loops,with_fixed,push", [(40, 20, False, 0.0), (40, 20, True, 0.0), (120, 150, False, 0.5)])
def test_optimize_on_the_device_solver_follows_minisams_levenberg_marquardt(F, N, loops, with_fixed, push):
    PC.check_loop_on_pcg(F, N, loops, with_fixed, push)


def test_graph_at_its_optimum_returns_false_after_lambda_runs_out(F):
    PC.check_loop_at_the_optimum(F)


def test_a_solve_that_reaches_its_cap_falls_back_to_the_host_factorisation(F):
    PC.check_forced_fallback(F)


def test_the_default_call_reports_what_it_always_did(F):
    PC.check_default_path(F)
