"""B scan-to-map registrations in one launch (lama_hip_match_solve_batch, HuberWeight(0.15), GaussNewton, 100 iterations) against
the same B problems as B sequential lama_hip_match_solve_with calls (CauchyWeight(0.15): the only weight that call has -- it is the
API the parent commit offers, hence the baseline).

Workload: the corridor's static map (the obstacle cells of ffi.corridor_log's world, as lama::Loc2D loads them), 1080-beam scans of
the seeded log, start poses = the scan's true pose perturbed by N(0, [0.04, 0.04, 0.015]) (numpy default_rng(1)).
B = 1, 16, 64, 256, 1024; 2 warm-up runs and 7 timed runs of each; median [min, max] of the wall clock around the call (which ends
in a stream synchronise) and ms per problem.  Plus ragged batches -- 256 and 4,096 problems whose scans have 90 .. 5,000 points (log-uniform) -- in three
launch orders: shuffled, longest last, longest first (workgroup b takes problem b, so the order of the call is the launch order).

Prints one JSON line per row and, with --out, writes the list to a file (profiles/match_solve_batch.json).
Usage: python tools/match_batch_bench.py [--sizes 1,16,64,256,1024] [--ragged 256,4096] [--repeats 7] [--warmup 2] [--out F]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def timed(fn, warmup, repeats):
    out = []
    for r in range(warmup + repeats):
        t0 = time.perf_counter()
        fn()
        if r >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def resample_scan(pts, n):
    """n points of the scan's outline: the scan's own points (n <= len) or linear interpolation between neighbours (n > len)"""
    t = np.linspace(0.0, len(pts) - 1.0, n)
    i = np.minimum(t.astype(int), len(pts) - 2)
    f = (t - i)[:, None]
    return pts[i] * (1.0 - f) + pts[i + 1] * f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,64,256,1024")
    ap.add_argument("--beams", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ragged", default="256,4096")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import iris_lama_amd.ffi as F
    from _worlds import corridor_obstacles
    if F.device_count() == 0:
        raise SystemExit("match_batch_bench needs an MI355X: there is no CPU fallback")
    steps = 40
    pts, _, truth = F.corridor_log(steps=steps, beams=a.beams)
    loc = F.Loc2D()
    loc.set_obstacles_world(corridor_obstacles())
    ctx = loc.hip_context()
    rng = np.random.default_rng(1)

    def problem(b):
        k = b % (steps + 1)
        d = rng.normal(0, [0.04, 0.04, 0.015])
        return pts[k], F.pose_from_xyr(truth[k][0] + d[0], truth[k][1] + d[1], truth[k][2] + d[2])

    rows = []
    for B in [int(s) for s in a.sizes.split(",")]:
        probs = [problem(b) for b in range(B)]
        scans, starts = [p[0] for p in probs], np.stack([p[1] for p in probs])
        packed = F.pack_scans(scans)
        res = {}

        def batch():
            res["b"] = ctx.match_solve_batch(0, packed, starts, max_iterations=100, strategy=0, robust="huber", robust_param=0.15)

        def sequential():
            res["s"] = [ctx.match_solve_with(0, scans[b], starts[b], strategy=0, max_iterations=100) for b in range(B)]

        tb, ts = timed(batch, a.warmup, a.repeats), timed(sequential, a.warmup, a.repeats)
        row = {"workload": "match_solve_batch", "B": B, "beams": a.beams, "robust": "huber(0.15) batch / cauchy(0.15) sequential",
               "batch_ms": spread(tb), "sequential_ms": spread(ts),
               "batch_ms_per_problem": round(statistics.median(tb) / B, 5), "sequential_ms_per_problem": round(statistics.median(ts) / B, 5),
               "speedup": round(statistics.median(ts) / statistics.median(tb), 2),
               "batch_iterations_mean": round(float(np.mean(res["b"][2])), 2), "sequential_iterations_mean": round(float(np.mean([r[2] for r in res["s"]])), 2)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    for B in [int(x) for x in a.ragged.split(",") if x]:
        sizes = np.round(np.exp(rng.uniform(np.log(90), np.log(5000), B))).astype(int)
        sizes[rng.integers(B)] = 5000
        probs = [problem(b) for b in range(B)]
        scans = [resample_scan(probs[b][0], int(sizes[b])) for b in range(B)]
        starts = np.stack([p[1] for p in probs])
        row = {"workload": "match_solve_batch_ragged", "B": B, "points_min": int(sizes.min()), "points_max": int(sizes.max()), "points_total": int(sizes.sum())}
        # workgroup b takes problem b, so the order of the problems in the call IS the launch order
        orders = {"shuffled": rng.permutation(B), "longest_last": np.argsort(sizes, kind="stable"), "longest_first": np.argsort(-sizes, kind="stable")}
        outs = {}
        for name, order in orders.items():
            packed, st = F.pack_scans([scans[i] for i in order]), starts[order]

            def run():
                outs[name] = ctx.match_solve_batch(0, packed, st, max_iterations=100, strategy=0, robust="huber", robust_param=0.15)
            row[name + "_ms"] = spread(timed(run, a.warmup, a.repeats))
            inv = np.argsort(order)
            outs[name] = [x[inv] for x in outs[name]]
        row["orders_agree"] = bool(all(np.array_equal(x, y) for n in ("longest_last", "longest_first") for x, y in zip(outs["shuffled"], outs[n])))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
    loc.close()


if __name__ == "__main__":
    main()
