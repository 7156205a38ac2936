"""planRoutes of the host classes on a device library WITHOUT lama_hip_map_travel: the engine test double tests/cpu_engine lacks it
(the symbol is optional, like lama_hip_map_frontiers), so the methods throw an error that names what is missing and everything else
goes on working.  No GPU."""
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


def test_the_double_lacks_the_symbol():
    assert not hasattr(C.CDLL(CPU_ENGINE), "lama_hip_map_travel")
    assert "lama_hip_map_travel" in F.HIP_SYMBOLS


def test_routes_name_the_missing_symbol_and_the_object_goes_on_working():
    pts, odom, _ = F.corridor_log(3, 90)
    s = F.Slam2D(trans_thresh=0.01, rot_thresh=0.01)
    here, there = [odom[0][:2]], [[odom[0][0] + 1.0, odom[0][1]]]
    assert s.routes(here, there) is None                            # before the first scan: no map, no device call
    assert s.update(pts[0], odom[0])
    with pytest.raises(F.LamaError) as e:
        s.routes(here, there)
    assert "lama_hip_map_travel" in str(e.value) and str(e.value).startswith("lama::Slam2D: "), str(e.value)
    assert s.update(pts[1], odom[1]) and s.update(pts[2], odom[2])  # every other call still works
    mn, mx, _, _ = s.view_bounds(0)
    assert np.all(mx > mn) and len(s.view_cells(1)) > 0
    s.close()
    mb = F.MapBuilder2D()
    mb.add(pts[0], F.pose_from_xyr(*odom[0]))
    assert mb.routes(here, there) is None                           # before the first build
    mb.close()


def test_the_other_classes_name_it_too():
    pts, odom, _ = F.corridor_log(2, 90)
    here, there = [odom[0][:2]], [[odom[0][0] + 1.0, odom[0][1]]]
    pf = F.PFSlam2D(F.pf_options(particles=3, seed=2))
    assert pf.routes(here, there) is None and pf.routes(here, there, particle=1) is None
    assert pf.update(pts[0], odom[0])
    for kw in ({}, {"particle": 1}):
        with pytest.raises(F.LamaError) as e:
            pf.routes(here, there, **kw)
        assert "lama_hip_map_travel" in str(e.value) and str(e.value).startswith("lama::PFSlam2D: "), str(e.value)
    pf.close()
