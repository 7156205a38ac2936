"""lama_hip_map_travel (iris_lama_amd/csrc/lama_travel.h) under the lane-level simulator of tests/sim (the kernel SOURCES compiled
for the host, see tests/test_kernel_sim.py): runs where there is no GPU.  The cases are in tests/_travel_checks.py, the expected
fields, routes and paths in tests/_travel.py."""
import os
import subprocess

import pytest

import _travel_checks as TC

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
def Fwide(Fsim):
    """the same module bound to the wide build (a 4-byte distance plane) in place of the default one"""
    saved = Fsim.HIP_LIB, Fsim._hip
    Fsim.HIP_LIB, Fsim._hip = SIM_LIB_WIDE, None
    yield Fsim
    Fsim.HIP_LIB, Fsim._hip = saved


def test_open_floor_in_one_tile(Fsim):
    TC.check_open_floor(Fsim)


def test_the_move_rules(Fsim):
    TC.check_move_rules(Fsim)


def test_clearance_and_preference_from_the_distance_layer(Fsim):
    TC.check_clearance_and_preference(Fsim)


def test_clearance_and_preference_in_the_wide_build(Fwide):
    TC.check_clearance_and_preference(Fwide)


def test_tiles(Fsim):
    TC.check_tiles(Fsim)


def test_many_sources(Fsim):
    TC.check_many_sources(Fsim)


def test_goals(Fsim):
    TC.check_goals(Fsim)


def test_strides_and_boxes_beside_and_beyond_the_map(Fsim):
    TC.check_strides_and_boxes(Fsim)


def test_strides_and_boxes_in_the_wide_build(Fwide):
    TC.check_strides_and_boxes(Fwide)


def test_refusals_leave_every_output_untouched(Fsim):
    TC.check_refusals(Fsim)


def test_a_map_without_patches(Fsim):
    TC.check_empty_map(Fsim)


def test_random_pictures(Fsim):
    TC.check_random_pictures(Fsim)


def test_the_random_pictures_meet_their_conditions_by_the_restatement_alone():
    """no library: the seeds are chosen so that the restatement reaches at least 8 goals and misses at least 1"""
    import _raster_checks  # noqa: F401
    import _travel as TR
    import numpy as np
    for seed in TC.RANDOM_SEEDS:
        pic, sq, goals, kw = TC.random_case(seed)
        occ = np.where(pic == TC.OCC, 100, np.where(pic == TC.FREE, 0, -1)).astype(np.int8)
        trav, _ = TR.classify(occ, sq, kw["clearance"], kw["prefer"])
        src, size = TR.largest_component_source(trav)
        assert size > 1000
        _, routes, _ = TR.expect(occ, sq, kw["clearance"], kw["prefer"], kw["near_factor"], [src], goals, kw["reach"], 0)
        TC.random_conditions(routes)
