"""-m gpu: k_match_solve_batch (iris_lama_amd/csrc/lama_match_batch.h), lama_hip_match_solve_batch and lama::SolveBatch on the device.
The checks and their bounds are in tests/_match_batch_checks.py, shared with the lane-simulator run of tests/test_match_batch_sim.py;
here the rotation of a pose comes from OCML's trig, so per-beam values are bit-equal to the oracle's only at heading 0 and within
the parity tolerances of tests/_match_checks.py elsewhere.  The bit-equality of every CauchyWeight(0.15) problem with
lama_hip_match_solve_with holds at every heading: both sides run the same device code."""
import numpy as np
import pytest

import _match_batch_checks as MB
import _match_checks as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import iris_lama_amd.ffi as f
    if f.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need the MI355X box (there is no CPU fallback)")
    return f


@pytest.fixture(scope="module")
def world(F):
    ctx, dm = M.build_world(F, 1.0)
    yield ctx, dm
    ctx.close()


@pytest.fixture(scope="module")
def slam(F):
    h, scan, base = MB.slam_with_map(F)
    assert h.engine_origin().endswith("liblama_hip.so")
    yield h, scan, base
    h.close()


def test_slices_mounts_and_beam_ownership_equal_the_single_solver_bit_for_bit(world):
    ctx, dm = world
    MB.check_slicing_and_ownership(ctx, dm, same_libm=False)


def test_every_problem_reads_its_own_particles_map(F):
    MB.check_maps_per_problem(F, same_libm=False)


def test_iteration_limits_per_problem(world):
    ctx, dm = world
    MB.check_iteration_limits(ctx, dm, same_libm=False)


def test_invalid_arguments_are_refused_with_everything_untouched(F, world):
    MB.check_refusals(F, world[0])


def test_zero_norm_state_marks_its_problem_only(F, world):
    MB.check_zero_norm_status(F, world[0])


def test_five_robust_costs_against_the_generic_host_loop(F, slam):
    h, scan, base = slam
    MB.check_robust_costs(F, h, scan, base)


def test_solve_batch_class_equals_the_c_abi_and_solve_keeps_its_refusals(F, slam):
    h, scan, base = slam
    other, _, _ = MB.slam_with_map(F, beams=60, steps=1)
    try:
        MB.check_host_class(F, h, scan, base, other=other)
    finally:
        other.close()


def test_a_batch_larger_than_the_chip(world):
    """B = 600 > 256 CUs: more than one workgroup per CU, every problem still its own (Cauchy(0.15): equal to the single solver for a
    sample of them; equal problems give equal results wherever they ran)"""
    ctx, dm = world
    base = MB.small_problems(sizes=(65, 257, 63), seed=11)
    problems = [base[b % 3] for b in range(600)]
    got = MB.run_batch(ctx, problems, strategy=0)
    MB.assert_equals_single(ctx, base, [g[:3] for g in got], 0, what="B = 600")
    for g in got:
        assert np.array_equal(g, np.concatenate([g[:3]] * 200)), "equal problems, different results"


def test_wide_library_bigsq_path(F):
    """l2_max = 7 m: liblama_hip_wide.so (a 4-byte distance plane) and the BIGSQ instantiations, which take the square root"""
    ctx, dm = M.build_world(F, 7.0, half_len=4.0)
    try:
        assert F.needs_wide(7.0, 0.05) and ctx.L is F.hip_lib(wide=True)
        problems = MB.small_problems(sizes=(65, 257), seed=9)
        for kind, param in (("cauchy", 0.15), ("huber", 0.15)):
            got = MB.run_batch(ctx, problems, strategy=0, robust=kind, robust_param=param)
            if kind == "cauchy":
                MB.assert_equals_single(ctx, problems, got, 0, what="wide")
            for b, (pts, origin, quat, start) in enumerate(problems):
                MB.assert_out8(ctx, dm, 0, pts, origin, quat, got[0][b], got[1][b], kind, param, False, ("wide", kind, b))
    finally:
        ctx.close()
