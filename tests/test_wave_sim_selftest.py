"""The lane simulator's own check (tests/sim/wave_sim.hpp): lanes of one wave that meet at a workgroup barrier from different call
sites are reported.  Two toy kernels, host only (tests/sim/barrier_selftest.cpp), each in a process of its own because the report ends
the process: the one in step runs to its end, the one in which thread 255 skips a loop trip and its barriers -- the shape of the
fault k_brushfire_canon had, which ran a whole launch under the simulator without a word -- must not."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
TOY = os.path.join(HERE, "sim", "_build", "barrier_selftest")


def _run(mode):
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "sim"), "_build/barrier_selftest"], check=True)
    return subprocess.run([TOY, mode], capture_output=True, text=True, timeout=60)


def test_threads_in_step_pass_their_barriers():
    r = _run("in-step")
    assert r.returncode == 0 and r.stdout.strip() == f"sum {256 * (1 + 2 + 3)}", (r.returncode, r.stdout, r.stderr)


def test_thread_that_skips_a_barrier_set_is_reported():
    r = _run("mis-stepped")
    assert r.returncode != 0 and "sum" not in r.stdout, (r.returncode, r.stdout)
    assert "lanes of one wave met at different workgroup barriers" in r.stderr and "divergent barrier" in r.stderr, r.stderr
    assert "lane 63 waits" in r.stderr or "lane 63 arrives" in r.stderr, r.stderr         # thread 255
