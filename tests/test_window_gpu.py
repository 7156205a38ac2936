"""-m gpu: window moves, growth and particle shipping in every direction (tests/_window_checks.py) against the CPU oracle's
particle filter, whose maps have no extent: k_shift_window with dx, dy of every sign (zero included) and with Ws != Wd, a
resample directly after every move (the directory rows k_clone_particles copies), k_export_particles and the translating
branch of k_import_particles for every sign of the offset between the two windows, for senders with a larger and a smaller
window than the receiver, for a receiver that must shift or grow, for one blob into two slots and over a slot that held a
larger map; clones of an uploaded map, whose mapped box has patches in its first and last row; the two loud failures of the
import.  Default library, and the wide one (l2_max = 7 m), whose guard radius -- and
with it the box padding and the clone's row range -- is 5 patches instead of 1.

Maps bit-equal for every particle after every update; the final scan match within POSE_TOL with equal iteration counts.  Every
case asserts from the counters and the blob header that it took the branch it names."""
import pytest

import _window_checks as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import iris_lama_amd.ffi as f
    if f.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need the MI355X box (there is no CPU fallback)")
    return f


@pytest.mark.parametrize("direction", sorted(W.DIRECTIONS))
def test_window_follows_the_robot_and_grows_on_the_way_back(F, direction):
    c = W.check_drive(F, direction)
    assert c["window_shifts"] >= 3 and c["window_growths"] == 1, c


@pytest.mark.parametrize("direction", ["+x-y", "-x+y"])
def test_window_moves_in_the_wide_library(F, direction):
    assert F.needs_wide(W.WIDE_L2, 0.05)
    c = W.check_drive(F, direction, window=24, l2_max=W.WIDE_L2)
    assert c["window_shifts"] >= 3 and c["window_growths"] == 1, c


@pytest.mark.parametrize("case", sorted(W.SHIP_CASES))
def test_shipped_particle_lands_where_the_oracle_has_it(F, case):
    W.run_ship_case(F, case)


@pytest.mark.parametrize("direction", ["+y", "-y"])
def test_clone_copies_the_end_rows_of_a_tight_mapped_box(F, direction):
    W.check_clone_with_a_tight_mapped_box(F, direction)


def test_import_that_cannot_be_placed_fails_in_the_import_call(F):
    W.check_import_too_far(F)


def test_blob_with_a_corrupt_header_is_refused(F):
    W.check_corrupt_blobs(F)
