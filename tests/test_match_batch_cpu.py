"""No GPU: what lama_hip_match_solve_batch and lama::SolveBatch promise before a device is touched -- the header declares the entry
points and both device libraries export them, a NULL context is refused, the Python wrapper checks its arguments, and a C++
consumer of the class written against the installed headers configures, builds and runs (without a device: it reports that)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import iris_lama_amd.ffi as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_both_libraries_export_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "lama_hip.h")).read()
    name = "lama_hip_match_solve_batch"
    assert name + "(" in hdr
    for lib in (F.HIP_LIB, F.HIP_LIB_WIDE):
        assert hasattr(C.CDLL(lib), name), (name, lib)
    for k, v in F.ROBUST_KINDS.items():
        macro = {"unit": "UNIT", "tukey": "TUKEY", "tdist": "TDIST", "cauchy": "CAUCHY", "huber": "HUBER"}[k]
        assert f"#define LAMA_HIP_ROBUST_{macro} {v}\n" in hdr
    assert hasattr(C.CDLL(F.HOST_LIB), "lama_slam_solve_batch")


def test_null_context_is_refused():
    L = F.hip_lib()
    z = np.zeros(8)
    assert L.lama_hip_match_solve_batch(None, 1, None, None, None, None, None, None, None, 0, 4, C.c_double(0.15), F._p(z), None, None) == -1
    assert L.lama_hip_match_solve_batch(None, 0, None, None, None, None, None, None, None, 0, 4, C.c_double(0.15), None, None, None) == -1


def test_python_wrapper_checks_its_arguments_before_any_device_is_touched():
    ctx = F.HipContext.__new__(F.HipContext)          # no device context behind it: a call that reached the library would crash
    ctx.h = None
    scans = [np.zeros((3, 3)), np.zeros((2, 3))]
    with pytest.raises(ValueError, match="poses"):
        ctx.match_solve_batch(0, scans, np.zeros((3, 4)))
    with pytest.raises(ValueError, match="origins"):
        ctx.match_solve_batch(0, scans, np.zeros((2, 4)), origins=np.zeros((1, 3)))
    with pytest.raises(ValueError, match="orientations"):
        ctx.match_solve_batch(0, scans, np.zeros((2, 4)), quats=np.zeros((3, 4)))
    with pytest.raises(KeyError):
        ctx.match_solve_batch(0, scans, np.zeros((2, 4)), robust="welsch")


def test_package_consumer_of_solve_batch_builds_and_runs(tmp_path):
    if shutil.which("cmake") is None:
        pytest.skip("cmake not available")
    build = str(tmp_path / "build")
    subprocess.run(["cmake", "-S", os.path.join(ROOT, "tests", "solve_batch_consumer"), "-B", build, f"-Diris_lama_DIR={os.path.join(ROOT, 'cmake')}"],
                   check=True, capture_output=True)
    subprocess.run(["cmake", "--build", build], check=True, capture_output=True)
    r = subprocess.run([os.path.join(build, "consumer")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    if F.device_count() == 0:
        assert "no device" in r.stdout and "no CPU fallback" in r.stdout
    else:
        assert "device path ran: candidates 5" in r.stdout and "solve refused 1" in r.stdout, r.stdout
