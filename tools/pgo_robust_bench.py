"""Device time of one pose-graph linearisation with and without robust losses: the 10k-pose / 50k-factor graph of tools/pgo_bench.py
(tests/_posegraph.py make_graph(10000, 40000, seed=1)) linearised at its dead-reckoning start, once as lama_hip_pgo_create builds
it (k_pgo_factors: the loss-free kernel) and once with Huber(0.1) on every loop closure (lama_hip_pgo_create_robust:
k_pgo_factors_robust).  kernel_ms is the device-event time of lama_hip_pgo_linearize_system (factors, reduce, assemble, sum); the
two graphs alternate, the first --warmup rounds are dropped, the median and the spread of the rest are printed as one JSON line.
Usage: python tools/pgo_robust_bench.py [--poses N] [--loops M] [--seed S] [--rounds R] [--warmup W]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=10000)
    ap.add_argument("--loops", type=int, default=40000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import iris_lama_amd.ffi as F
    from _posegraph import make_graph
    fi, fj, meas, sq, truth, init = make_graph(a.poses, a.loops, seed=a.seed)
    kind = np.where(np.arange(len(fi)) >= a.poses, F.PGO_LOSS_HUBER, F.PGO_LOSS_NONE).astype(np.int32)
    param = np.where(kind != 0, 0.1, 0.0)
    graphs = {"loss_free": F.PoseGraph(a.poses, fi, fj, meas, sq, device=a.device),
              "huber_closures": F.PoseGraph(a.poses, fi, fj, meas, sq, device=a.device, loss_kind=kind, loss_param=param)}
    ms = {k: [] for k in graphs}
    try:
        for g in graphs.values():
            g.set_poses(init)
        for r in range(a.warmup + a.rounds):
            for name, g in graphs.items():
                t = g.linearize_system()["kernel_ms"]
                if r >= a.warmup:
                    ms[name].append(t)
        w = graphs["huber_closures"].factor_weights()
    finally:
        for g in graphs.values():
            g.close()
    out = {"workload": "pgo_linearize_system", "poses": a.poses, "factors": len(fi), "robust_factors": int((kind != 0).sum()),
           "robust_factors_below_weight_1": int((w < 1.0).sum()), "rounds": a.rounds}
    for name, v in ms.items():
        out[name + "_kernel_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
