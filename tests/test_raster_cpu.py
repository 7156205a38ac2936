"""The grid methods of the host classes on a device library WITHOUT lama_hip_map_bounds / lama_hip_map_rasterize: the engine test
double tests/cpu_engine lacks both (the two symbols are optional, like lama_hip_map_occupied_cells), so getOccupancyGrid /
getDistanceGrid throw an error that names what is missing and everything else goes on working.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import _testhost
import iris_lama_amd.ffi as F
from _testhost import CPU_ENGINE


@pytest.fixture(scope="module", autouse=True)
def cpu_engine():
    _testhost.set_engine_library(CPU_ENGINE)      # builds tests/cpu_engine, switches ffi to the -DLAMA_TESTING host build
    yield
    _testhost.set_engine_library(None)


def test_the_double_has_neither_symbol():
    L = C.CDLL(CPU_ENGINE)
    assert not hasattr(L, "lama_hip_map_rasterize") and not hasattr(L, "lama_hip_map_bounds")
    assert "lama_hip_map_rasterize" in F.HIP_SYMBOLS and "lama_hip_map_bounds" in F.HIP_SYMBOLS


def test_grid_methods_name_the_missing_symbol_and_the_object_goes_on_working():
    pts, odom, _ = F.corridor_log(3, 90)
    s = F.Slam2D(trans_thresh=0.01, rot_thresh=0.01)
    assert s.occupancy_grid() is None                               # before the first scan: no map, no device call
    assert s.update(pts[0], odom[0])
    for call in (s.occupancy_grid, s.distance_grid):
        with pytest.raises(F.LamaError) as e:
            call()
        assert "lama_hip_map_rasterize" in str(e.value) and str(e.value).startswith("lama::Slam2D: "), str(e.value)
    assert s.update(pts[1], odom[1]) and s.update(pts[2], odom[2])  # every other call still works
    mn, mx, _, _ = s.view_bounds(0)
    assert np.all(mx > mn) and len(s.view_cells(1)) > 0
    s.close()
    mb = F.MapBuilder2D()
    mb.add(pts[0], F.pose_from_xyr(*odom[0]))
    assert mb.occupancy_grid() is None                              # before the first build
    mb.close()
