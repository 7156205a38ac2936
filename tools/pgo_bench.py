"""BASELINE config 5 through lama::SimplePGO: a 10k-pose / 50k-factor graph (tests/_posegraph.py make_graph(10000, 40000, seed=1))
optimised on the device (residuals, Jacobians, Hessian assembly, trial steps) with the sparse LDL^T on the host (--solver ldlt, the
default) or with the damped system solved on the device as well (--solver pcg: block-Jacobi conjugate gradient).  Prints one JSON
line: status, iterations, tries, device ms (linearise + assemble; trial steps), host ms (ordering; factorisation + solve), total ms
and nnz(L); with pcg also the conjugate-gradient iterations (summed, longest solve), the tries that fell back to the LDL^T and the
device ms of the solves.  Usage: python tools/pgo_bench.py [--poses N] [--loops M] [--seed S] [--solver ldlt|pcg]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=10000)
    ap.add_argument("--loops", type=int, default=40000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--solver", choices=("ldlt", "pcg"), default="ldlt")
    a = ap.parse_args()
    import iris_lama_amd.ffi as F
    from _posegraph import make_graph
    fi, fj, meas, sq, truth, init = make_graph(a.poses, a.loops, seed=a.seed)
    edges = [(int(fi[k]), int(fj[k]), meas[k]) for k in range(a.poses, len(fi))]
    t0 = time.perf_counter()
    if a.solver == "pcg":
        ok, poses, rep = F.simple_pgo(init, edges, device=a.device, solver="pcg")
    else:
        ok, poses, rep = F.simple_pgo(init, edges, device=a.device)
    wall = (time.perf_counter() - t0) * 1e3
    out = {
        "workload": "simple_pgo", "solver": a.solver, "poses": a.poses, "factors": len(fi), "ok": bool(ok), "status": rep["status_name"],
        "iterations": rep["iterations"], "tries": rep["tries"], "initial_error": rep["initial_error"], "final_error": rep["final_error"],
        "device_linearize_ms": round(rep["ms_device_linearize"], 3), "device_try_ms": round(rep["ms_device_try"], 3),
        "host_ordering_ms": round(rep["ms_analyze"], 1), "host_factorize_ms": round(rep["ms_factorize"], 1),
        "total_ms": round(rep["ms_total"], 1), "wall_ms": round(wall, 1), "nnz_L": rep["nnz_L"]}
    if a.solver == "pcg":
        out.update({"pcg_iterations": rep["pcg_iterations"], "pcg_max_iterations_seen": rep["pcg_max_iterations_seen"],
                    "pcg_fallbacks": rep["pcg_fallbacks"], "device_solve_ms": round(rep["ms_device_solve"], 3)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
