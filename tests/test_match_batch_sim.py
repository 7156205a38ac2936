"""k_match_solve_batch (iris_lama_amd/csrc/lama_match_batch.h), lama_hip_match_solve_batch and lama::SolveBatch under the lane-level
simulator of tests/sim (the kernel SOURCES compiled for the host, see tests/test_kernel_sim.py): runs where there is no GPU.  The
checks and their bounds are in tests/_match_batch_checks.py.  The simulator links the host's libm, so the oracle's per-beam values
are the kernel's bit for bit at every heading (same_libm)."""
import os
import subprocess

import numpy as np
import pytest

import _match_batch_checks as MB
import _match_checks as M
import _testhost

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_LIB = os.path.join(HERE, "sim", "_build", "liblama_hip_sim.so")
SIM_LIB_WIDE = os.path.join(HERE, "sim", "_build", "liblama_hip_sim_wide.so")


@pytest.fixture(scope="module")
def Fsim():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "sim")], check=True)
    import iris_lama_amd.ffi as F
    saved = F.HIP_LIB, F._hip, F.HIP_LIB_WIDE, F._hip_wide
    F.HIP_LIB, F._hip, F.HIP_LIB_WIDE, F._hip_wide = SIM_LIB, None, SIM_LIB_WIDE, None
    yield F
    F.HIP_LIB, F._hip, F.HIP_LIB_WIDE, F._hip_wide = saved


@pytest.fixture(scope="module")
def world(Fsim):
    ctx, dm = M.build_world(Fsim, 1.0)
    yield ctx, dm
    ctx.close()


@pytest.fixture(scope="module")
def slam(Fsim):
    """lama::Slam2D of the test-suite's host build, bound to the simulator as its device library"""
    _testhost.set_engine_library(SIM_LIB)
    h, scan, base = MB.slam_with_map(Fsim)
    assert h.engine_origin() == SIM_LIB
    yield h, scan, base
    h.close()
    _testhost.set_engine_library(None)


def test_slices_mounts_and_beam_ownership_equal_the_single_solver_bit_for_bit(world):
    ctx, dm = world
    MB.check_slicing_and_ownership(ctx, dm, same_libm=True)


def test_every_problem_reads_its_own_particles_map(Fsim):
    MB.check_maps_per_problem(Fsim, same_libm=True)


def test_iteration_limits_per_problem(world):
    ctx, dm = world
    MB.check_iteration_limits(ctx, dm, same_libm=True)


def test_invalid_arguments_are_refused_with_everything_untouched(Fsim, world):
    MB.check_refusals(Fsim, world[0])


def test_zero_norm_state_marks_its_problem_only(Fsim, world):
    MB.check_zero_norm_status(Fsim, world[0])


def test_five_robust_costs_against_the_generic_host_loop(Fsim, slam):
    h, scan, base = slam
    MB.check_robust_costs(Fsim, h, scan, base)


def test_solve_batch_class_equals_the_c_abi_and_solve_keeps_its_refusals(Fsim, slam):
    h, scan, base = slam
    other, _, _ = MB.slam_with_map(Fsim, beams=60, steps=1)
    try:
        MB.check_host_class(Fsim, h, scan, base, other=other)
    finally:
        other.close()


def test_wide_library_bigsq_path(Fsim):
    """l2_max = 7 m: the wide build (a 4-byte distance plane) and the BIGSQ instantiations, which take the square root"""
    ctx, dm = M.build_world(Fsim, 7.0, half_len=4.0)
    try:
        assert Fsim.needs_wide(7.0, 0.05) and ctx.L is Fsim.hip_lib(wide=True)
        problems = MB.small_problems(sizes=(65, 257), seed=9)
        for kind, param in (("cauchy", 0.15), ("huber", 0.15)):
            got = MB.run_batch(ctx, problems, strategy=0, robust=kind, robust_param=param)
            if kind == "cauchy":
                MB.assert_equals_single(ctx, problems, got, 0, what="wide")
            for b, (pts, origin, quat, start) in enumerate(problems):
                MB.assert_out8(ctx, dm, 0, pts, origin, quat, got[0][b], got[1][b], kind, param, True, ("wide", kind, b))
    finally:
        ctx.close()


def test_robust_weight_restatement_equals_the_reference_values():
    """tests/golden/robust_weights_golden.npz: x and RobustCost::value(x) written by the reference's own robust_cost.cpp
    (tests/golden/make_robust_golden.py), the kinks of Huber and Tukey at, one ulp below and one ulp above included"""
    g = np.load(MB.GOLDEN)
    for kind, param in MB.KINDS:
        x, want = g[kind + "_x"], g[kind + "_value"]
        assert float(g[kind + "_param"]) == (param if kind != "tukey" else float(np.float64(param)))
        assert len(x) >= 100
        assert np.array_equal(MB.robust_value(kind, param, x), want), kind
    k = 0.15
    assert {k, np.nextafter(k, 0.0), np.nextafter(k, 1.0)} <= set(g["huber_x"])
    b = 4.6851
    assert {b, np.nextafter(b, 0.0), np.nextafter(b, 9.0)} <= set(g["tukey_x"])
