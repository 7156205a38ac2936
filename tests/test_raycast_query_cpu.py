"""castRays of the host classes on a device library WITHOUT lama_hip_map_cast_rays (the engine test double tests/cpu_engine lacks
it: the symbol is optional, like lama_hip_map_rasterize), and the host-side helpers of include/lama/sdm/ray_cast.h and their Python
twins: the fan of a beam model and the range formula.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import _testhost
import iris_lama_amd.ffi as F
from _testhost import CPU_ENGINE

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cpu_engine():
    _testhost.set_engine_library(CPU_ENGINE)      # builds tests/cpu_engine, switches ffi to the -DLAMA_TESTING host build
    yield
    _testhost.set_engine_library(None)


def test_the_double_lacks_the_symbol_and_the_bindings_name_it(cpu_engine):
    assert not hasattr(C.CDLL(CPU_ENGINE), "lama_hip_map_cast_rays")
    assert "lama_hip_map_cast_rays" in F.HIP_SYMBOLS
    for name in ("lama_slam_cast_rays", "lama_pf_cast_rays", "lama_mapbuilder_cast_rays", "lama_lo_cast_rays", "lama_loc_cast_rays", "lama_loc_check_scan"):
        assert name in F.HOST_SYMBOLS and hasattr(F.host_lib(), name), name


def test_cast_rays_names_the_missing_symbol_and_the_object_goes_on_working(cpu_engine):
    pts, odom, _ = F.corridor_log(3, 90)
    fan = F.fan_points(16, -1.0, 0.125, 6.0)
    poses = np.stack([F.pose_from_xyr(*odom[0])])
    s = F.Slam2D(trans_thresh=0.01, rot_thresh=0.01)
    assert s.cast_rays(poses, fan) is None                          # before the first scan: no map, no device call
    assert s.update(pts[0], odom[0])
    for call in (lambda: s.cast_rays(poses, fan), lambda: s.expected_ranges(poses, 16, -1.0, 0.125, 6.0), lambda: s.cast_rays(poses, fan, distance_map=True)):
        with pytest.raises(F.LamaError) as e:
            call()
        assert "lama_hip_map_cast_rays" in str(e.value) and str(e.value).startswith("lama::Slam2D: "), str(e.value)
    assert s.update(pts[1], odom[1]) and s.update(pts[2], odom[2])  # every other call still works
    assert len(s.view_cells(1)) > 0
    s.close()
    mb = F.MapBuilder2D()
    mb.add(pts[0], F.pose_from_xyr(*odom[0]))
    assert mb.cast_rays(poses, fan) is None                         # before the first build
    mb.close()
    loc = F.Loc2D()
    assert loc.cast_rays(poses, fan) is None and loc.check_scan(pts[0]) is None      # no device map yet
    loc.close()


def _helper_output(tmp_path, n, a0, da, r):
    exe = str(tmp_path / "raycast_fan")
    subprocess.run(["g++", "-O1", "-std=c++14", "-ffp-contract=off", "-I" + os.path.join(HERE, "..", "include"), os.path.join(HERE, "raycast_fan.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe, str(n), repr(a0), repr(da), repr(r)], check=True, capture_output=True, text=True).stdout.split("\n")
    pts = np.array([[float.fromhex(v) for v in line.split()] for line in out[:n]])
    return pts, np.array([float.fromhex(v) for v in out[n:] if v])


def test_the_fan_helper_and_the_range_formula(tmp_path):
    n, a0, da, r = 1080, -2.356194490192345, 0.004363323129985824, 12.0
    cpp_pts, cpp_ranges = _helper_output(tmp_path, n, a0, da, r)
    # beam i at angle_min + i * angle_increment, max_range long, cos and sin from libm once per beam.  Python's twin bit for bit; the
    # C++ helper within 4 units in the last place: a compiler may take both from one sincos call, whose results lie within an ulp of
    # the true value like cos' and sin' own (two ulps apart at most), and the product with max_range rounds once on either side
    want = np.array([(r * math.cos(a0 + i * da), r * math.sin(a0 + i * da), 0.0) for i in range(n)])
    assert np.array_equal(F.fan_points(n, a0, da, r), want)
    assert cpp_pts.shape == (n, 3) and np.all(np.abs(cpp_pts - want) <= 4.0 * np.spacing(np.abs(want))) and np.all(cpp_pts[:, 2] == 0.0)
    assert np.allclose(np.hypot(want[:, 0], want[:, 1]), r, rtol=1e-15) and want[0, 0] < 0 and want[0, 1] < 0
    assert F.fan_points(1, 0.0, 0.1, 5.0).tolist() == [[5.0, 0.0, 0.0]] and F.fan_points(0, 0.0, 0.1, 5.0).shape == (0, 3)
    # range = resolution * sqrt(dx^2 + dy^2) of the stopping cell's integer offset from the start cell, +inf for status none
    start = np.array([[100, 200], [4000000000, 7]], dtype=np.uint32)
    cells = np.array([[[103, 204], [0, 0], [100, 200]], [[4000000000 - 8191, 7 + 4096], [4000000001, 7], [5, 5]]], dtype=np.uint32)
    status = np.array([[1, 0, 2], [1, 1, 0]], dtype=np.uint8)
    got = F.ray_ranges(0.05, start, cells, status)
    by_hand = [0.05 * math.sqrt(25.0), math.inf, 0.0, 0.05 * math.sqrt(float(8191 * 8191 + 4096 * 4096)), 0.05, math.inf]
    assert got.ravel().tolist() == by_hand and got[0, 0] == 0.25
    assert cpp_ranges.tolist() == by_hand
