"""lama::DeviceContext -- the type that owns a host class's device context and turns a refused device call into the class's
exception -- and its mirror in ffi.py (one base class for close / __del__ / _chk / _scan / hip_context), on the engine test
double tests/cpu_engine (no GPU).  The double counts the contexts it creates and destroys and the map downloads it is asked for
with a capacity of 0 (lama_cpu_engine_call_counts), and refuses a scan with a non-finite point the way the device library does."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _testhost
import iris_lama_amd.ffi as F
from _testhost import CPU_ENGINE

HERE = os.path.dirname(os.path.abspath(__file__))
NON_FINITE = "the scan holds a non-finite point"      # the double's (and the device library's) lama_hip_last_error text


@pytest.fixture(scope="module", autouse=True)
def cpu_engine():
    _testhost.set_engine_library(CPU_ENGINE)      # builds tests/cpu_engine, switches ffi to the -DLAMA_TESTING host build
    yield
    _testhost.set_engine_library(None)


@pytest.fixture(scope="module")
def log():
    pts, odom, _ = F.corridor_log(1, 90)
    bad = pts[0].copy()
    bad[5, 0] = np.nan
    return pts, odom, bad


def _counts():
    """(contexts created, contexts destroyed, downloads asked for with cap == 0) of the double, process-wide"""
    out = (C.c_uint64 * 3)()
    C.CDLL(CPU_ENGINE).lama_cpu_engine_call_counts(out)
    return tuple(out)


def _room(side=4.0, step=0.05):
    t = np.arange(0.0, side + step / 2, step)
    z, s = np.zeros_like(t), np.full_like(t, side)
    return np.concatenate([np.stack([t, z], 1), np.stack([t, s], 1), np.stack([z, t], 1), np.stack([s, t], 1)])


def _refused(excinfo, cls, call, status, text):
    """today's format of every host class: "<class>: <C-ABI call> failed (status <rc>): <lama_hip_last_error>" """
    msg = str(excinfo.value)
    assert msg.startswith(f"lama::{cls}: {call} failed (status {status}): "), msg
    assert text in msg, msg


def test_slam2d_names_class_call_status_and_engine_error(log):
    pts, odom, bad = log
    s = F.Slam2D()
    with pytest.raises(F.LamaError) as e:
        s.update(bad, odom[0])
    _refused(e, "Slam2D", "lama_hip_pf_init", -1, NON_FINITE)
    s.close()


def test_pf_slam2d_names_class_call_status_and_engine_error(log):
    pts, odom, bad = log
    pf = F.PFSlam2D(F.pf_options(particles=3, seed=5))
    pf.set_prior(*odom[0])
    with pytest.raises(F.LamaError) as e:
        pf.update(bad, odom[0])
    _refused(e, "PFSlam2D", "lama_hip_pf_init", -1, NON_FINITE)
    pf.close()


def test_lidar_odometry_2d_names_class_call_status_and_engine_error(log):
    lo = F.LidarOdometry2D()
    with pytest.raises(F.LamaError) as e:
        lo.update(log[2])
    _refused(e, "LidarOdometry2D", "lama_hip_pf_init", -1, NON_FINITE)
    lo.close()


def test_loc2d_names_class_call_status_and_engine_error(log):
    pts, odom, bad = log
    loc = F.Loc2D()
    loc.set_obstacles_world(_room())
    with pytest.raises(F.LamaError) as e:
        loc.update(bad, odom[0], force=True)
    _refused(e, "Loc2D", "lama_hip_match_solve", -1, NON_FINITE)
    loc.close()


def test_map_builder_2d_names_class_call_status_and_engine_error(log):
    pts, odom, bad = log
    mb = F.MapBuilder2D()
    mb.add(pts[0], F.pose_from_xyr(*odom[0]))
    mb.add(bad, F.pose_from_xyr(*odom[1]))
    with pytest.raises(F.LamaError) as e:
        mb.build()
    _refused(e, "MapBuilder2D", "lama_hip_map_integrate_scans", -1, "a key scan holds a non-finite point")
    mb.close()


def _make(cls, log):
    """an object of the class with a live device context, the particles of that context and a map kind that has patches"""
    pts, odom, _ = log
    if cls is F.PFSlam2D:
        obj = cls(F.pf_options(particles=3, seed=5))
        obj.set_prior(*odom[0])
        obj.update(pts[0], odom[0])
        return obj, 3, F.MAP_DISTANCE
    obj = cls()
    if cls is F.Slam2D:
        obj.update(pts[0], odom[0])
    elif cls is F.LidarOdometry2D:
        obj.update(pts[0])
    elif cls is F.Loc2D:
        obj.set_obstacles_world(_room())          # Loc2D creates its context with the first device call
    else:
        obj.add(pts[0], F.pose_from_xyr(*odom[0]))
        obj.build()
        return obj, 1, F.MAP_OCCUPANCY            # (one pruned scan leaves no occupied cell: the distance map is empty)
    return obj, 1, F.MAP_DISTANCE


@pytest.mark.parametrize("cls", [F.Slam2D, F.Loc2D, F.LidarOdometry2D, F.MapBuilder2D, F.PFSlam2D], ids=lambda c: c.__name__)
def test_hip_context_is_borrowed_and_reports_the_particles(cls, log):
    created0, destroyed0, _ = _counts()
    obj, particles, kind = _make(cls, log)
    ctx = obj.hip_context()
    assert isinstance(ctx, F.HipContext) and ctx._is_borrowed and ctx.P == particles and ctx.cfg is None
    assert ctx.h.value and ctx.h.value == getattr(obj.L, cls._context)(obj.h)
    assert len(ctx.download_map(particles - 1, kind)) > 0                     # the view works on the owner's maps
    ctx.close()
    ctx.close()
    assert ctx.h is None and _counts()[:2] == (created0 + 1, destroyed0)      # closing the view leaves the context to its owner
    again = obj.hip_context()
    assert len(again.download_map(0, kind)) > 0                               # ... which still has it
    del again
    obj.close()
    obj.close()
    assert obj.h is None and _counts()[:2] == (created0 + 1, destroyed0 + 1)  # destroyed by the owner, exactly once


def test_map_without_patches_downloads_as_empty_without_a_zero_capacity_call(log):
    pts, odom, _ = log
    mb = F.MapBuilder2D()
    mb.add(np.zeros((0, 3)), F.pose_from_xyr(*odom[0]))       # an empty cloud contributes nothing: the built map has no patch
    mb.build()
    zero_cap0 = _counts()[2]
    cells = mb.view_cells(0)                                   # getOccupancyMap(): a download of that map
    assert cells is not None and cells.shape == (0, 2)
    assert mb.view_cells(1) is not None and len(mb.view_cells(1)) == 0
    assert _counts()[2] == zero_cap0
    mb.close()


def test_sanitized_life_cycle_program():
    """tests/cpu_engine/host_lifecycle.cpp under -fsanitize=address,undefined, as an ordinary executable: every class constructed,
    updated and destroyed; Loc2D::Init a second time with another resolution (not reachable through the host C-ABI) gives a working
    object and destroys the first context exactly once; a moved DeviceContext; downloads of maps without patches."""
    d = os.path.join(HERE, "cpu_engine")
    subprocess.run(["make", "-s", "-j8", "-C", d, "sanitized"], check=True)
    r = subprocess.run([os.path.join(d, "_build", "host_lifecycle"), os.path.join(d, "_build", "liblama_cpu_engine_san.so")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host life cycle OK: 10 contexts created and destroyed" in r.stdout and not r.stderr, r.stdout + r.stderr
