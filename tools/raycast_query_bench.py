"""Ray casts through a device map (castRays -> lama_hip_map_cast_rays, iris_lama_amd/csrc/lama_raycast_query.h) against the path a
caller had before them, on the corridor map: lama::Slam2D over the seeded corridor log of bench.py (ffi.corridor_log, 1080 beams)
after 40 steps.  Two shapes, a fan of 1080 beams of 12 m each: ONE pose (a simulated scan, a scan check) and 3000 poses (candidate
gating), the poses drawn around the driven path.  Every repeat makes one more update() -- which drops the snapshots, as in a node
that asks every few updates -- and then times
  (a) the device: kernel_ms (hipEvents around the launch) and the wall clock around the context-level call (upload, launch, the
      download of all six arrays, one stream synchronise) and around Slam2D.cast_rays (the same plus the host class's ranges);
  (b) the old path for the same answer: getOccupancyMap() with a cold snapshot (lama_slam_view_bounds: the sparse download plus the
      host index) and then lama_slam_view_cast_rays, the host loop of computeRay's cells + isOccupied per cell on one core; the loop
      is reported on its own as well (a caller who already holds a snapshot pays only that).
The order of (a) and (b) alternates between repeats; medians, minima and maxima are printed.  Also on the distance map (what
lama::Loc2D has on the device; no host path to compare with: its occupancy map never was on the device).  The steps the host loop finds
are compared with the device's (`agree`: the share of beams with the same first occupied cell; the host loop composes the pose
with plain products, the device as the map update does, so a beam on a cell boundary may differ).
Prints one JSON line per shape.  Usage: python tools/raycast_query_bench.py [--repeats 7] [--warmup 2] [--poses 3000] [--out F]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--beams", type=int, default=1080)
    ap.add_argument("--poses", type=int, default=3000)
    ap.add_argument("--range", type=float, default=12.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import iris_lama_amd.ffi as F
    if F.device_count() == 0:
        raise SystemExit("raycast_query_bench needs an MI355X: there is no CPU fallback")
    shapes = [1, a.poses]
    total = a.warmup + a.repeats
    pts, odom, truth = F.corridor_log(steps=40 + len(shapes) * total, beams=a.beams)
    s = F.Slam2D(trans_thresh=0.01, rot_thresh=0.01)
    for k in range(41):
        s.update(pts[k], odom[k])
    ctx = s.hip_context()
    fan = F.fan_points(a.beams, -math.pi, 2.0 * math.pi / a.beams, a.range)
    rng = np.random.default_rng(7)
    rows, step = [], 41
    for K in shapes:
        base = truth[rng.integers(0, 41, K)] + np.stack([rng.normal(0, 0.15, K), rng.normal(0, 0.15, K), rng.uniform(-math.pi, math.pi, K)], axis=1)
        poses = np.stack([F.pose_from_xyr(*p) for p in base])
        new = {"kernel_ms": [], "context_call_ms": [], "slam2d_cast_rays_ms": [], "distance_map_kernel_ms": [], "distance_map_call_ms": []}
        old = {"cold_snapshot_ms": [], "host_loop_ms": []}
        agree = []
        for r in range(total):
            s.update(pts[step], odom[step]); step += 1                # drops the snapshots
            acc = {}

            def new_path():
                acc["context_call_ms"], got = timed(lambda: ctx.cast_rays(0, F.MAP_OCCUPANCY, poses, fan, resolution=0.05))
                acc["kernel_ms"] = got.kernel_ms
                acc["slam2d_cast_rays_ms"], _ = timed(lambda: s.cast_rays(poses, fan))
                acc["distance_map_call_ms"], d = timed(lambda: ctx.cast_rays(0, F.MAP_DISTANCE, poses, fan, tolerance_cells=2, resolution=0.05))
                acc["distance_map_kernel_ms"] = d.kernel_ms
                return got

            def old_path():
                acc["cold_snapshot_ms"], _ = timed(lambda: s.view_bounds(0))
                acc["host_loop_ms"], steps = timed(lambda: s.view_cast_rays(poses, fan))
                return steps
            if r % 2 == 0:
                got = new_path(); steps = old_path()
            else:
                steps = old_path(); got = new_path()
            agree.append(float((np.where(got.status == F.RAY_OCCUPIED, got.step, -1) == steps).mean()))
            if r >= a.warmup:
                for k in new:
                    new[k].append(acc[k])
                for k in old:
                    old[k].append(acc[k])
        row = {"workload": "raycast_query_corridor", "poses": K, "beams": a.beams, "range_m": a.range, "steps": 40,
               "rays_stopped_share": round(float((got.status == F.RAY_OCCUPIED).mean()), 4), "cells_walked": int(np.where(got.step >= 0, got.step + 1, got.nn).sum()),
               "device": {k: spread(v) for k, v in new.items()}, "old_path": {k: spread(v) for k, v in old.items()},
               "old_path_with_download_ms": round(statistics.median(old["cold_snapshot_ms"]) + statistics.median(old["host_loop_ms"]), 4),
               "agree": round(min(agree), 5)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    s.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
