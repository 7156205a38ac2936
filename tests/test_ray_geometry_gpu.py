"""-m gpu: the integer beam geometry of the ray-cast and map-rebuild kernels on beams constructed cell by cell
(tests/_ray_checks.py): the third axis setting the step count (particle-filter path in both ray-cast forms, the rebuild full and
hits-only, LidarOdometry2D's ray rule and log-odds cells), truncation limits at, one ulp below and one ulp above a beam's length,
lattice directions from the corner cells of a patch, beams that graze a patch corner as the bound of their chunk's cone, scans of
1 to 4096 points in the parallel form and 4097 in the sequential one, the 8191-cell limit, and the two paths the lane simulator
compiles out: dir_get_or_alloc's election and mb_bin_add's shared atomic.  Against the oracle's particle filter and the
reference-composed rebuild, bit for bit; every case asserts its beams' cells first and its ray-cast form from the counters."""
import pytest

import _ray_checks as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import iris_lama_amd.ffi as f
    if f.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need the MI355X box (there is no CPU fallback)")
    return f


@pytest.mark.parametrize("form", RC.FORMS)
def test_third_axis_sets_the_step_count(F, form):
    RC.check_third_axis_pf(F, form)
    RC.check_third_axis_through_the_transform_pf(F, form)


def test_third_axis_in_the_map_rebuild(F):
    RC.check_third_axis_rebuild(F)


def test_third_axis_under_the_lidar_odometry_ray_rule_and_log_odds_cells(F):
    RC.check_third_axis_lidar_odometry(F)


def test_third_axis_in_an_unguarded_context_with_the_lidar_odometry_ray_rule(F):
    RC.check_third_axis_lidar_odometry_context(F)


@pytest.mark.parametrize("form", RC.FORMS)
@pytest.mark.parametrize("name", sorted(RC.TRUNCATIONS))
def test_truncation_limit_against_the_length_of_a_3_4_5_beam(F, name, form):
    RC.check_truncation(F, form, name)


@pytest.mark.parametrize("form", RC.FORMS)
def test_one_beam_of_a_chunk_starts_elsewhere_under_truncated_ray(F, form):
    RC.check_truncated_ray_fan(F, form)


@pytest.mark.parametrize("form", RC.FORMS)
@pytest.mark.parametrize("corner", sorted(RC.CORNER_SENSORS))
def test_lattice_directions_from_the_corner_cells_of_a_patch(F, corner, form):
    RC.check_directions(F, form, corner)


def test_lattice_directions_in_the_map_rebuild(F):
    RC.check_directions_rebuild(F)


@pytest.mark.parametrize("form", RC.FORMS)
@pytest.mark.parametrize("clockwise", [False, True], ids=["ccw", "cw"])
@pytest.mark.parametrize("position", ["first", "middle", "last"])
def test_beam_that_grazes_a_patch_corner_bounds_its_chunk(F, position, clockwise, form):
    RC.check_grazing(F, form, position, clockwise)


@pytest.mark.parametrize("name", RC.FAN_CASES_SMALL + RC.FAN_CASES_LARGE)
def test_chunk_and_scan_size_structure(F, name):
    RC.check_fan(F, 2, name)


@pytest.mark.parametrize("name", ["n = 65", "ends of the chunk without free cells", "n = 4096"])
def test_chunk_cases_in_the_sequential_form(F, name):
    RC.check_fan(F, 1, name)


def test_scan_of_4097_points_goes_beam_by_beam(F):
    RC.check_scan_of_4097_points_goes_sequential(F)


@pytest.mark.parametrize("form", RC.FORMS)
@pytest.mark.parametrize("which", sorted(RC.LONG_SCANS))
def test_beam_of_8191_cells_is_mapped_in_a_grown_window(F, which, form):
    RC.check_longest_beam(F, form, which)


@pytest.mark.parametrize("form", RC.FORMS)
def test_beam_of_8192_cells_is_refused_and_the_maps_stay(F, form):
    RC.check_too_long_beam_pf(F, form)


def test_length_limit_in_the_map_rebuild(F):
    RC.check_length_limit_rebuild(F)


@pytest.mark.parametrize("name", sorted(RC.ELECTION))
def test_one_wave_asks_for_missing_patches_together(F, name):
    RC.check_election(F, name)


def test_half_of_a_waves_patches_exist_already(F):
    RC.check_election_with_half_the_patches_there(F)


def test_bins_of_one_wave_differ_or_coincide_in_the_map_rebuild(F):
    RC.check_bin_add(F)
