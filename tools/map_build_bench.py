"""Map rebuild from K posed key scans of the seeded corridor log (ffi.corridor_log, 1080 beams) at several K:
  (a) lama::MapBuilder2D::build() -- a full rebuild (occupancy map cleared, all keys integrated, occupied list, distance map), split
      by stage (wall clock around calls that end in a stream synchronise), plus the device time of the integrate kernels alone
      (hipEvents on the context's stream, cfg.profile) with their achieved bytes/s against the algorithmic traffic
      cells visited x 4 B + patches x 4 KB;
  (b) the replay a one-particle context offers without it: lama_hip_pf_set_poses + lama_hip_pf_update_maps per key scan;
  (c) the reference's loop on one host core through tests/_reference.py (Occ.set_occupied, DM.compute_ray, Occ.set_free): one ctypes
      call per cell, so this figure includes the Python call overhead -- it is the loop the tests use as their expectation, not a
      tuned CPU implementation.
Warm-up runs first, then `--repeats` timed runs of each; median and min / max are reported.  Prints one JSON line per K and, with
--out, writes the list to a file.  Usage: python tools/map_build_bench.py [--keys 10,40,160] [--repeats 7] [--ref-max-keys 40] [--out F]"""
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
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", default="10,40,160")
    ap.add_argument("--beams", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ref-max-keys", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import iris_lama_amd.ffi as F
    if F.device_count() == 0:
        raise SystemExit("map_build_bench needs an MI355X: there is no CPU fallback")
    rows = []
    for K in [int(k) for k in a.keys.split(",")]:
        pts, _, truth = F.corridor_log(steps=K - 1, beams=a.beams)
        poses4 = np.stack([F.pose_from_xyr(*t) for t in truth])
        scans = [pts[k] for k in range(K)]
        row = {"workload": "map_build", "keys": K, "beams": a.beams}
        # ---- (a) MapBuilder2D: full rebuilds of the same keys
        b = F.MapBuilder2D()
        for k in range(K):
            b.add(scans[k], poses4[k])
        stages = {"integrate_ms": [], "occupied_ms": [], "distance_ms": [], "build_ms": []}
        for r in range(a.warmup + a.repeats):
            b.set_poses(poses4)                                     # marks the map stale: the next build starts from an empty map
            t0 = time.perf_counter()
            b.build()
            wall = (time.perf_counter() - t0) * 1e3
            if r >= a.warmup:
                t = b.timing()
                for k in ("integrate_ms", "occupied_ms", "distance_ms"):
                    stages[k].append(t[k])
                stages["build_ms"].append(wall)
        row["builder"] = {k: spread(v) for k, v in stages.items()}
        row["occupied_cells"] = int(len(b.occupied_cells()))
        b.close()
        # the integrate kernels alone, by events on the context's stream
        dev, calls = [], []
        cells = patches = 0
        for r in range(a.warmup + a.repeats):
            ctx = F.HipContext(F.default_cfg(particles=1, profile=1))
            packed = F.pack_scans(scans)
            t0 = time.perf_counter()
            ctx.integrate_scans(0, poses4, packed, full=True, prune=True)
            wall = (time.perf_counter() - t0) * 1e3
            c = ctx.counters()
            if r >= a.warmup:
                dev.append(c["ms_raycast"]); calls.append(wall)
            cells, patches = int(c["ray_cells"]), int(c["occ_patches"])
            ctx.close()
        row["integrate_call_fresh_context_ms"] = spread(calls)
        row["integrate_kernels_ms"] = spread(dev)
        traffic = cells * 4 + patches * 4096
        row["cells_visited"] = cells; row["occ_patches"] = patches; row["algorithmic_bytes"] = traffic
        row["integrate_achieved_GBps"] = round(traffic / (statistics.median(dev) * 1e-3) / 1e9, 3)
        # ---- (b) replay: set_poses + update_maps per key scan on a one-particle context
        rep = []
        for r in range(a.warmup + a.repeats):
            ctx = F.HipContext(F.default_cfg(particles=1))
            t0 = time.perf_counter()
            ctx.init(scans[0], poses4[0])
            for k in range(1, K):
                ctx.set_poses(poses4[k:k + 1])
                ctx.update_maps(scans[k])
            wall = (time.perf_counter() - t0) * 1e3
            if r >= a.warmup:
                rep.append(wall)
            ctx.close()
        row["replay_update_maps_ms"] = spread(rep)
        # ---- (c) the reference's loop, one host core, through the ctypes view
        import _reference as R
        if R.available() and K <= a.ref_max_keys:
            import _mapbuild as MB
            t0 = time.perf_counter()
            MB.build(poses4, scans, full=True)
            row["reference_loop_ctypes_ms"] = {"median": round((time.perf_counter() - t0) * 1e3, 1), "n": 1}
        else:
            row["reference_loop_ctypes_ms"] = "not measured"
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
