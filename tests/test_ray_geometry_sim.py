"""The integer beam geometry of the ray-cast and map-rebuild kernels on beams constructed cell by cell (tests/_ray_checks.py),
executed lane by lane on the CPU (tests/sim, see tests/test_kernel_sim.py): the third axis setting the step count, truncation
limits at, one ulp below and one ulp above a beam's length, lattice directions from the corner cells of a patch, beams that graze
a patch corner as the bound of their chunk's cone, chunk and scan-size structure up to 128 beams and one 1024-beam scan, the
8191-cell limit.  Particle-filter cases in both ray-cast forms against the oracle's filter, rebuild cases against the
reference-composed rebuild, all bit for bit.  tests/test_ray_geometry_gpu.py runs the same cases, the large scans and the two
paths the simulator compiles out (dir_get_or_alloc's election, mb_bin_add's shared atomic) on the device."""
import pytest

import _ray_checks as RC
import _reference as R
from test_kernel_sim import Fsim  # noqa: F401  (the fixture)

needs_reference = pytest.mark.skipif(not R.available(), reason="the compiled reference (oracle/_ref, made by build()) is not there")
# The geometry does not depend on the reach of the distance map, and the simulator pays for every cell the brushfire floods:
# 5 cells here instead of 10.
L2_MAX = 0.25


@needs_reference
def test_oracle_equals_the_reference_where_the_third_axis_sets_the_step_count():
    RC.check_oracle_against_the_reference_on_the_third_axis()


@pytest.mark.parametrize("form", RC.FORMS)
def test_third_axis_sets_the_step_count(Fsim, form):
    RC.check_third_axis_pf(Fsim, form, l2_max=L2_MAX)
    RC.check_third_axis_through_the_transform_pf(Fsim, form, l2_max=L2_MAX)


def test_third_axis_in_an_unguarded_context_with_the_lidar_odometry_ray_rule(Fsim):
    RC.check_third_axis_lidar_odometry_context(Fsim)


@needs_reference
def test_third_axis_in_the_map_rebuild(Fsim):
    RC.check_third_axis_rebuild(Fsim)


@pytest.mark.parametrize("form", RC.FORMS)
@pytest.mark.parametrize("name", sorted(RC.TRUNCATIONS))
def test_truncation_limit_against_the_length_of_a_3_4_5_beam(Fsim, name, form):
    RC.check_truncation(Fsim, form, name, l2_max=L2_MAX)


@pytest.mark.parametrize("form", RC.FORMS)
def test_one_beam_of_a_chunk_starts_elsewhere_under_truncated_ray(Fsim, form):
    RC.check_truncated_ray_fan(Fsim, form, l2_max=L2_MAX)


@pytest.mark.parametrize("form", RC.FORMS)
@pytest.mark.parametrize("corner", sorted(RC.CORNER_SENSORS))
def test_lattice_directions_from_the_corner_cells_of_a_patch(Fsim, corner, form):
    RC.check_directions(Fsim, form, corner, l2_max=L2_MAX)


@needs_reference
def test_lattice_directions_in_the_map_rebuild(Fsim):
    RC.check_directions_rebuild(Fsim)


@pytest.mark.parametrize("clockwise", [False, True], ids=["ccw", "cw"])
@pytest.mark.parametrize("position", ["first", "middle", "last"])
def test_beam_that_grazes_a_patch_corner_bounds_its_chunk(Fsim, position, clockwise):
    RC.check_grazing(Fsim, 2, position, clockwise, l2_max=L2_MAX)


@pytest.mark.parametrize("name", RC.FAN_CASES_SMALL)
def test_chunk_and_scan_size_structure(Fsim, name):
    RC.check_fan(Fsim, 2, name, l2_max=L2_MAX)


@pytest.mark.parametrize("name", ["n = 65", "ends of the chunk without free cells"])
def test_chunk_cases_in_the_sequential_form(Fsim, name):
    RC.check_fan(Fsim, 1, name, l2_max=L2_MAX)


@pytest.mark.parametrize("form", RC.FORMS)
@pytest.mark.parametrize("which", sorted(RC.LONG_SCANS))
def test_beam_of_8191_cells_is_mapped_in_a_grown_window(Fsim, which, form):
    RC.check_longest_beam(Fsim, form, which, l2_max=L2_MAX)


@pytest.mark.parametrize("form", RC.FORMS)
def test_beam_of_8192_cells_is_refused_and_the_maps_stay(Fsim, form):
    RC.check_too_long_beam_pf(Fsim, form, l2_max=L2_MAX)


@needs_reference
def test_length_limit_in_the_map_rebuild(Fsim):
    RC.check_length_limit_rebuild(Fsim)
