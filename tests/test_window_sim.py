"""k_shift_window, the directory rows of k_clone_particles, k_export_particles and the translating branch of k_import_particles
executed lane by lane on the CPU (tests/sim, see tests/test_kernel_sim.py) on a reduced matrix of tests/_window_checks.py: two
particles, the drives towards -x, -y and one diagonal with fewer stops, one negative offset and the two shipments between
windows of different sides, a clone of an uploaded map (whose mapped box has no guard rows), both loud failures.  These kernels are plain index code and the window placement is host code, so
the simulator runs exactly their logic; tests/test_window_gpu.py runs the full matrix on the device."""
import pytest

import _window_checks as W
from test_kernel_sim import Fsim  # noqa: F401  (the fixture)

# Fewer stops than on the device: 8 m out shifts the window, 2 m past the start shifts it back, 6 m past the start makes it grow.
# The simulator pays for every cell the brushfire floods, so the distance maps reach 5 cells here instead of 10 (the guard radius,
# which is what the window code sees of it, stays one patch): a drive takes 3 s instead of 9.
STOPS = dict(out=(4.0, 8.0), back=(-2.0, -6.0))
L2_MAX = 0.25


@pytest.mark.parametrize("direction", ["-x", "-y", "+x-y"])
def test_window_follows_the_robot_and_grows_on_the_way_back(Fsim, direction):
    c = W.check_drive(Fsim, direction, P=2, l2_max=L2_MAX, **STOPS)
    assert c["window_shifts"] >= 3 and c["window_growths"] == 1, c


@pytest.mark.parametrize("case", ["offset --", "grown sender", "larger sender", "larger receiver"])
def test_shipped_particle_lands_where_the_oracle_has_it(Fsim, case):
    W.run_ship_case(Fsim, case, l2_max=L2_MAX)


def test_clone_copies_the_first_row_of_a_tight_mapped_box(Fsim):
    W.check_clone_with_a_tight_mapped_box(Fsim, "+y", l2_max=L2_MAX)


def test_import_that_cannot_be_placed_fails_in_the_import_call(Fsim):
    W.check_import_too_far(Fsim, l2_max=L2_MAX)


def test_blob_with_a_corrupt_header_is_refused(Fsim):
    W.check_corrupt_blobs(Fsim, l2_max=L2_MAX)
