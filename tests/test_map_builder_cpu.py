"""lama::MapBuilder2D without a GPU: the C-ABI declares and both device libraries export the two entry points, the bindings'
argument checks reject before a device is touched, the public header compiles in a package consumer with and without
LAMA_USE_EIGEN, the class fails loudly without a device, and the new kernels keep the library's rule for scalar loads."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import iris_lama_amd.ffi as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lama_hip_map_integrate_scans", "lama_hip_map_occupied_cells")


def _hip_libs():
    if not (os.path.exists(F.HIP_LIB) and os.path.exists(F.HIP_LIB_WIDE)):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "iris_lama_amd"), "hip"], check=True)
    return F.HIP_LIB, F.HIP_LIB_WIDE


def test_header_declares_and_both_libraries_export_the_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lama_hip.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\bint32_t\s+" + n + r"\s*\(", src), n
        assert n in F.HIP_SYMBOLS
    assert re.search(r"lama_hip_map_integrate_scans\s*\(\s*lama_hip_ctx\*\s*ctx,\s*uint32_t\s+particle,\s*uint32_t\s+num_scans,\s*const double\*\s*poses4", src)
    for path in _hip_libs():
        L = C.CDLL(path)
        for n in NEW:
            assert hasattr(L, n), (path, n)
    host = open(os.path.join(ROOT, "include", "lama_host.h")).read()
    for n in F.HOST_SYMBOLS:
        if n.startswith("lama_mapbuilder_"):
            assert re.search(r"\b" + n + r"\s*\(", host), n
    assert sum(n.startswith("lama_mapbuilder_") for n in F.HOST_SYMBOLS) >= 10


def test_entry_points_reject_bad_arguments_without_a_context():
    L = C.CDLL(_hip_libs()[0])
    F._bind_hip(L)
    n = C.c_uint32(7)
    assert L.lama_hip_map_integrate_scans(None, 0, 1, None, None, None, None, None, 3) == -1      # LAMA_HIP_E_INVALID
    assert L.lama_hip_map_occupied_cells(None, 0, 0, None, C.byref(n)) == -1


def test_scan_packing_checks_its_arguments_before_any_device_is_touched():
    pts = np.zeros((10, 3))
    p, o = F.pack_scans([pts[:4], pts[4:4], pts[4:]])
    assert p.shape == (10, 3) and o.tolist() == [0, 4, 4, 10] and o.dtype == np.uint32
    p, o = F.pack_scans((pts, [0, 3, 10]))
    assert o.tolist() == [0, 3, 10]
    assert F.pack_scans([])[1].tolist() == [0]
    for bad in ([0, 5, 3, 10], [0, 3, 9], [1, 3, 10], [0, -1, 10], []):
        with pytest.raises(ValueError):
            F.pack_scans((pts, bad))
    with pytest.raises(ValueError):
        F.pack_scans((np.zeros((10, 2)), [0, 10]))
    with pytest.raises(ValueError):
        F.pack_scans([np.zeros((5, 2))])

    class NoDevice(F.HipContext):                                   # the checks of integrate_scans come before the library call
        def __init__(self):
            self.h = None

            class L:
                @staticmethod
                def lama_hip_map_integrate_scans(*a):
                    raise AssertionError("the device library was called")
            self.L = L
    ctx = NoDevice()
    for kw in (dict(poses4=np.zeros((2, 4)), scans=[pts]), dict(poses4=np.zeros((1, 4)), scans=[pts], origins=np.zeros((2, 3))),
               dict(poses4=np.zeros((1, 4)), scans=[pts], quats=np.zeros((3, 4))), dict(poses4=np.zeros((1, 4)), scans=(pts, [0, 11]))):
        with pytest.raises(ValueError):
            ctx.integrate_scans(0, **kw)


def test_map_builder_fails_loudly_without_a_gpu():
    if F.device_count() != 0:                                       # with a device the class starts (tests/test_map_builder_gpu.py does the rest)
        F.MapBuilder2D().close()
        return
    with pytest.raises(F.LamaError) as e:
        F.MapBuilder2D()
    assert "no CPU fallback" in str(e.value)
    with pytest.raises(F.LamaError):
        F.MapBuilder2D(l2_max=7.0)                                  # the wide library: the same refusal


def _run_consumer(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    if F.device_count() == 0:
        assert "no device" in r.stdout and "no CPU fallback" in r.stdout
    else:
        assert "device path ran: keys 5" in r.stdout and "wall 1 inside 1" in r.stdout, r.stdout
    return r.stdout


def test_package_consumer_of_the_class_builds(tmp_path):
    if shutil.which("cmake") is None:
        pytest.skip("cmake not available")
    build = str(tmp_path / "build")
    subprocess.run(["cmake", "-S", os.path.join(ROOT, "tests", "map_builder_consumer"), "-B", build, f"-Diris_lama_DIR={os.path.join(ROOT, 'cmake')}"],
                   check=True, capture_output=True)
    subprocess.run(["cmake", "--build", build], check=True, capture_output=True)
    _run_consumer(os.path.join(build, "consumer"))


def test_class_builds_with_eigen_typed_public_types(tmp_path):
    """LAMA_USE_EIGEN switches include/lama/types.h to Eigen's types; <Eigen/...> comes from the API stand-in the reference-build
    checker uses (as tests/test_cabi.py does for the other classes)."""
    out = tmp_path / "eigen_typed"
    out.mkdir()
    flags = ["-O1", "-std=c++14", "-fPIC", "-ffp-contract=off", "-pthread", "-DLAMA_USE_EIGEN", "-I" + os.path.join(ROOT, "include"),
             "-I" + os.path.join(ROOT, "oracle", "ref_shim")]
    srcs = sorted(glob.glob(os.path.join(ROOT, "iris_lama_amd", "host", "*.cpp")))
    subprocess.run(["g++", *flags, "-shared", "-o", str(out / "liblama_host.so"), *srcs, "-ldl"], check=True, capture_output=True)
    subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "map_builder_consumer", "consumer.cpp"), "-o", str(out / "consumer"),
                    "-L" + str(out), "-llama_host", "-Wl,-rpath," + str(out), "-ldl"], check=True, capture_output=True)
    for lib in _hip_libs():
        shutil.copy(lib, str(out / os.path.basename(lib)))          # the siblings it dlopen()s
    _run_consumer(str(out / "consumer"))


@pytest.mark.parametrize("wide", [False, True])
def test_new_kernels_add_no_scalar_loads_of_rewritten_data(wide):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_scalar_loads.py")] + (["--wide"] if wide else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
