"""The map-rebuild kernels (iris_lama_amd/csrc/lama_map_build.h) under the lane-level simulator of tests/sim (the kernel SOURCES
compiled for the host, see tests/test_kernel_sim.py) against the reference-composed map at small size: full / hits-only with a
sensor transform, split invariance, prune, a counter wrap inside one call, the occupied-cell list.  Runs where there is no GPU."""
import os
import subprocess

import numpy as np
import pytest

import _reference as R
from _cmp import OCC_FIELDS, assert_maps_equal

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_LIB = os.path.join(HERE, "sim", "_build", "liblama_hip_sim.so")
pytestmark = pytest.mark.skipif(not R.available(), reason="the compiled reference (oracle/_ref, made by build()) is not there")


@pytest.fixture()
def Fsim():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "sim")], check=True)
    import iris_lama_amd.ffi as F
    saved, saved_lib = F.HIP_LIB, getattr(F, "_hip", None)
    F.HIP_LIB = SIM_LIB
    F._hip = None
    yield F
    F.HIP_LIB, F._hip = saved, saved_lib


def test_rebuild_split_prune_and_occupied_cells_on_the_simulator(Fsim):
    import _mapbuild as MB
    F = Fsim
    poses4, _, scans, origins, quats = MB.room_log(21, K=6, beams=60, sensor=True)
    for full in (True, False):
        raw = MB.build(poses4, scans, origins, quats, full=full).dump()
        ctx = F.HipContext(F.default_cfg(particles=1))
        ctx.integrate_scans(0, poses4[:2], scans[:2], origins[:2], quats[:2], full=full, prune=False)
        ctx.integrate_scans(0, poses4[2:], scans[2:], origins[2:], quats[2:], full=full, prune=False)
        assert_maps_equal(ctx.download_map(0, F.MAP_OCCUPANCY), raw, OCC_FIELDS, f"two calls, full {full}")
        assert np.array_equal(ctx.occupied_cells(0), MB.occupied_cells(raw))
        ctx.close()
        ctx = F.HipContext(F.default_cfg(particles=1))
        ctx.integrate_scans(0, poses4, scans, origins, quats, full=full, prune=True)
        assert_maps_equal(ctx.download_map(0, F.MAP_OCCUPANCY), MB.pruned(raw), OCC_FIELDS, f"pruned, full {full}")
        ctx.close()


def test_counter_wrap_on_the_simulator(Fsim):
    import _mapbuild as MB
    F = Fsim
    pose = R.pose_from_xyr(0.1, 0.2, -0.3)
    scan = np.array([[0.4, 0.05, 0.0], [0.4, 0.05, 0.0]])           # a short ray, its cell hit twice per repetition
    one = MB.build([pose], [scan], full=True).dump()
    rep = 32768 + 3                                                 # occupied and visited of the hit cell pass 65,535
    want = {}
    for pid, (cells, mask) in one.items():
        c = cells.copy()
        c["occupied"] = (cells["occupied"].astype(np.uint64) * rep % 65536).astype(np.uint16)
        c["visited"] = (cells["visited"].astype(np.uint64) * rep % 65536).astype(np.uint16)
        want[pid] = (c, mask.copy())
    ctx = F.HipContext(F.default_cfg(particles=1))
    ctx.integrate_scans(0, np.tile(pose, (rep, 1)), (np.tile(scan, (rep, 1)), np.arange(rep + 1) * 2), full=True, prune=False)
    assert_maps_equal(ctx.download_map(0, F.MAP_OCCUPANCY), want, OCC_FIELDS, "wrap")
    ctx.close()
