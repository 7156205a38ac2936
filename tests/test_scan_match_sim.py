"""k_scan_match (iris_lama_amd/csrc/lama_kernels.h) through lama_hip_pf_scan_match and the grouped step under the lane-level
simulator of tests/sim (the kernel SOURCES compiled for the host, see tests/test_kernel_sim.py): runs where there is no GPU.  The
checks and their bounds are in tests/_scan_match_checks.py.  The simulator links the host's libm, so the oracle's per-beam values
are the kernel's bit for bit at every heading (same_libm)."""
import os
import subprocess

import pytest

import _scan_match_checks as SC

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
    ctx, dm = SC.build_world(Fsim)
    yield ctx, dm
    ctx.close()


def test_gradient_exit_at_iteration_0_far_away_and_on_an_empty_map(Fsim, world):
    SC.check_gradient_exit(Fsim, world, same_libm=True)


@pytest.mark.parametrize("name", list(SC.EXITS))
def test_exit(Fsim, world, name):
    SC.check_exit(Fsim, world, name, same_libm=True)


def test_beam_slicing_mounts_cell_edges_and_missing_patches(world):
    SC.check_slicing(world, same_libm=True)


def test_every_particle_its_own_map_start_and_slot(Fsim):
    SC.check_pool(Fsim, same_libm=True)


def test_groups_of_more_particles_than_the_pose_table_holds(Fsim):
    SC.check_groups_beyond_the_pose_table(Fsim, same_libm=True)


def test_bigsq_on_the_narrow_library(Fsim):
    """l2_max = 1.5 m: 30 cells, max_sqdist 900 > SM_LUT on the build with the 2-byte distance plane"""
    SC.check_bigsq(Fsim, 1.5, SC.HALF_LEN, wide=False, same_libm=True)


def test_bigsq_on_the_wide_library(Fsim):
    """l2_max = 7 m, as tests/test_match_batch_sim.py's wide case"""
    SC.check_bigsq(Fsim, 7.0, 4.0, wide=True, same_libm=True)


def test_outputs_may_be_null(Fsim, world):
    SC.check_null_outputs(Fsim, world)
