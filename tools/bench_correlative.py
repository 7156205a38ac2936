"""The pose-lattice search (lama_hip_match_search_lattice, csrc/lama_correlative.h) on the README's floor-plan case, beside the only way
the parent commit has to score a pose: lama_hip_eval_batch (Loc2D::globalLocalization's candidate evaluation).

Workload: the lama::Loc2D map of the generated 100 m x 60 m office floor that bench.py's loc2d_map_load row builds (l2_max 1 m,
0.05 m cells); a 1080-beam, 270-degree scan taken inside one of its rooms; the lattice over the whole plan at linear_step 0.2 m
(4 cells) and angular_step 5 degrees (72 headings), every 4th point, tiles of 8 x 8 nodes.  Timed: the host clock around the call, which
uploads the scan and the headings' transforms, runs the kernel, downloads the tile keys and ends in a stream synchronise; warm-up
calls first, then `--repeats` calls, median [min, max].  Beside it: lama_hip_eval_batch on 3000 random poses of the same scan, timed
the same way, and Loc2D::relocalize end to end (search, selection, one refinement batch).  Derived: time per pose and map lookups per
second (lattice: one per used point and pose; eval_batch: four bilinear corners per point and pose).

One process; every device step runs under its own time limit, and nothing more is started after one that failed or ran out of time.
Prints one JSON line and, with --out, writes it to a file (profiles/correlative_search.json).
Usage: python tools/bench_correlative.py [--repeats 9] [--warmup 3] [--out F] [--plan 100,60] [--linear-step 0.2] [--eval-poses 3000]"""
import argparse
import contextlib
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OFF = (2642244 >> 1) * 32


@contextlib.contextmanager
def step_limit(seconds, what):
    def expired(*_):
        raise TimeoutError(f"{what}: no result within {seconds} s")
    old = signal.signal(signal.SIGALRM, expired)
    signal.setitimer(signal.ITIMER_REAL, seconds)
    try:
        yield
    finally:
        signal.setitimer(signal.ITIMER_REAL, 0)
        signal.signal(signal.SIGALRM, old)


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


def grid_scan(cells, pose, beams=1080, fov=np.deg2rad(270.0), max_range=25.0, res=0.05):
    """sensor-frame points of a scanner at `pose` in the occupancy grid given by its occupied cells: every beam is walked in steps of
    half a cell to its first occupied cell"""
    xs, ys = cells[:, 0].astype(np.int64) - OFF, cells[:, 1].astype(np.int64) - OFF
    occ = np.zeros((int(ys.max()) + 2, int(xs.max()) + 2), dtype=bool)
    occ[ys, xs] = True
    x, y, yaw = pose
    phi = -fov / 2 + fov * np.arange(beams) / (beams - 1)
    r = np.arange(0.1, max_range, res / 2)
    px, py = x + np.cos(yaw + phi)[:, None] * r[None, :], y + np.sin(yaw + phi)[:, None] * r[None, :]
    ix, iy = np.floor(px / res + 0.5).astype(np.int64), np.floor(py / res + 0.5).astype(np.int64)
    ok = (ix >= 0) & (iy >= 0) & (ix < occ.shape[1]) & (iy < occ.shape[0])
    hit = np.zeros(ok.shape, dtype=bool)
    hit[ok] = occ[iy[ok], ix[ok]]
    first = hit.argmax(axis=1)
    got = hit.any(axis=1)
    rr = r[first][got]
    return np.stack([rr * np.cos(phi[got]), rr * np.sin(phi[got]), np.zeros(got.sum())], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--plan", default="100,60", help="width,height of the generated floor plan in metres")
    ap.add_argument("--linear-step", type=float, default=0.2)
    ap.add_argument("--eval-poses", type=int, default=3000)
    a = ap.parse_args()
    import bench
    import iris_lama_amd.ffi as F
    if F.device_count() == 0:
        raise SystemExit("bench_correlative needs an MI355X: there is no CPU fallback")
    W, Hm = (float(v) for v in a.plan.split(","))
    cells = bench.floor_plan_cells(W, Hm)
    world = (cells.astype(np.float64) - OFF) * 0.05
    true_pose = (W / 2 + 1.3, Hm / 2 - 0.9, 0.4)            # inside a room, off its centre
    scan = grid_scan(cells, true_pose)
    row = {"workload": "correlative_search", "plan_m": [W, Hm], "occupied_cells": int(len(cells)), "l2_max_m": 1.0, "resolution_m": 0.05,
           "scan_points": int(len(scan)), "true_pose": list(true_pose)}
    try:
        import torch
        row["machine"] = torch.cuda.get_device_name(0)
    except Exception:
        row["machine"] = "unknown"
    with step_limit(240, "map load"):
        loc = F.Loc2D(l2_max=1.0)
        t0 = time.perf_counter()
        loc.set_obstacles_world(world)
        row["map_load_seconds"] = round(time.perf_counter() - t0, 3)
    ctx = loc.hip_context()
    # ---- the lattice
    linear_step, angular_step, point_step, tile = a.linear_step, np.deg2rad(5.0), 4, 8
    cell_step = max(1, int(round(linear_step / 0.05)))
    H = max(1, int(round(2 * np.pi / angular_step)))
    nx, ny = int(np.floor(W / (cell_step * 0.05))) + 1, int(np.floor(Hm / (cell_step * 0.05))) + 1
    angles = -np.pi + np.arange(H) * (2 * np.pi / H)
    n_used = (len(scan) + point_step - 1) // point_step
    poses_l = H * nx * ny
    res = {}

    def lattice():
        res["best"], _ = ctx.search_lattice(0, scan, angles, 0.0, 0.0, cell_step, nx, ny, tile=tile, point_step=point_step, scores=False)

    with step_limit(120, "lattice search"):
        tl = timed(lattice, a.warmup, a.repeats)
    key = int(res["best"].min())
    index = key & 0xFFFFFFFF
    bh, biy, bix = index // (nx * ny), (index // nx) % ny, index % nx
    row["lattice"] = {"linear_step_m": linear_step, "angular_step_deg": 5.0, "cell_step": cell_step, "nx": nx, "ny": ny, "headings": H, "tile": tile,
                      "point_step": point_step, "points_used": n_used, "poses": poses_l, "workgroups": int(res["best"].size), "call_ms": spread(tl),
                      "ns_per_pose": round(1e6 * statistics.median(tl) / poses_l, 4),
                      "lookups_per_second": round(poses_l * n_used / (1e-3 * statistics.median(tl)), 1),
                      "best_node": {"score": key >> 32, "x": bix * cell_step * 0.05, "y": biy * cell_step * 0.05, "heading": float(angles[bh])}}
    # ---- the yardstick: eval_batch on 3000 random poses of the same scan
    rng = np.random.default_rng(3)
    B = a.eval_poses
    xyr = np.stack([rng.uniform(0, W, B), rng.uniform(0, Hm, B), rng.uniform(-np.pi, np.pi, B)], axis=1)
    poses = np.stack([F.pose_from_xyr(*p) for p in xyr])

    def evalb():
        res["sq"] = ctx.eval_batch(0, scan, poses)

    with step_limit(120, "eval_batch"):
        te = timed(evalb, a.warmup, a.repeats)
    row["eval_batch"] = {"poses": B, "points": int(len(scan)), "call_ms": spread(te), "ns_per_pose": round(1e6 * statistics.median(te) / B, 2),
                         "lookups_per_second": round(B * len(scan) * 4 / (1e-3 * statistics.median(te)), 1)}
    row["per_pose_ratio_eval_batch_over_lattice"] = round(row["eval_batch"]["ns_per_pose"] / row["lattice"]["ns_per_pose"], 1)
    row["order_of_magnitude_cheaper"] = bool(row["per_pose_ratio_eval_batch_over_lattice"] >= 10.0)
    # ---- the class path end to end: every cell further than 0.15 m from a wall is free
    occ = np.zeros((int(round(Hm / 0.05)) + 8, int(round(W / 0.05)) + 8), dtype=bool)
    occ[cells[:, 1].astype(np.int64) - OFF, cells[:, 0].astype(np.int64) - OFF] = True
    near = occ.copy()
    for d in range(1, 4):
        near[d:, :] |= occ[:-d, :]; near[:-d, :] |= occ[d:, :]
    near2 = near.copy()
    for d in range(1, 4):
        near2[:, d:] |= near[:, :-d]; near2[:, :-d] |= near[:, d:]
    fy, fx = np.nonzero(~near2[:int(round(Hm / 0.05)), :int(round(W / 0.05))])
    loc.occ_set_cells(np.stack([fx + OFF, fy + OFF], axis=1).astype(np.uint32), -1)
    loc.set_pose(3.0, 3.0, -2.0)
    out = {}

    def reloc():
        out["ok"] = loc.relocalize(scan, linear_step=linear_step, angular_step=angular_step, point_step=point_step, tile=tile)

    with step_limit(120, "relocalize"):
        tr = timed(reloc, 1, max(a.repeats // 3, 3))
    p = loc.pose()
    row["relocalize"] = {"call_ms": spread(tr), "returned": bool(out["ok"]), "pose": [float(p[2]), float(p[3]), float(np.arctan2(p[1], p[0]))],
                         "best_rmse": float(loc.relocalize_candidates()["rmse"][0])}
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)
            f.write("\n")
    loc.close()


if __name__ == "__main__":
    main()
