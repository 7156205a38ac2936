"""-m gpu: k_scan_match (iris_lama_amd/csrc/lama_kernels.h) through lama_hip_pf_scan_match and the grouped step on the device.  The
checks and their bounds are in tests/_scan_match_checks.py, shared with the lane-simulator run of tests/test_scan_match_sim.py; here
the rotation of a pose comes from OCML's trig, so per-beam values are bit-equal to the oracle's only at heading 0 and within the
parity tolerances of tests/_match_checks.py elsewhere.  The bit-equality of every particle with lama_hip_match_solve_with holds at
every heading: both sides run the same device code."""
import pytest

import _scan_match_checks as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import iris_lama_amd.ffi as f
    if f.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need the MI355X box (there is no CPU fallback)")
    return f


@pytest.fixture(scope="module")
def world(F):
    ctx, dm = SC.build_world(F)
    yield ctx, dm
    ctx.close()


def test_gradient_exit_at_iteration_0_far_away_and_on_an_empty_map(F, world):
    SC.check_gradient_exit(F, world, same_libm=False)


@pytest.mark.parametrize("name", list(SC.EXITS))
def test_exit(F, world, name):
    SC.check_exit(F, world, name, same_libm=False)


def test_beam_slicing_mounts_cell_edges_and_missing_patches(world):
    SC.check_slicing(world, same_libm=False)


def test_every_particle_its_own_map_start_and_slot(F):
    SC.check_pool(F, same_libm=False)


def test_groups_of_more_particles_than_the_pose_table_holds(F):
    SC.check_groups_beyond_the_pose_table(F, same_libm=False)


def test_bigsq_on_the_narrow_library(F):
    """l2_max = 1.5 m: 30 cells, max_sqdist 900 > SM_LUT on liblama_hip.so"""
    SC.check_bigsq(F, 1.5, SC.HALF_LEN, wide=False, same_libm=False)


def test_bigsq_on_the_wide_library(F):
    """l2_max = 7 m: liblama_hip_wide.so"""
    SC.check_bigsq(F, 7.0, 4.0, wide=True, same_libm=False)


def test_outputs_may_be_null(F, world):
    SC.check_null_outputs(F, world)
