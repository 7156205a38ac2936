"""Dense grids of device maps (getOccupancyGrid / getDistanceGrid -> lama_hip_map_rasterize) against the path a map publisher had
before them, on two maps:
  corridor : lama::Slam2D over the seeded corridor log of bench.py (ffi.corridor_log, 1080 beams) after 40 steps.  Every repeat makes
             one more update() -- which drops the snapshots, as in a publisher that runs every few updates -- and then times
             (a) occupancy_grid / distance_grid at strides 1 and 8 (wall clock around calls that end in a stream synchronise), and
             (b) the old path for the same answer: getOccupancyMap() with a cold snapshot (lama_slam_view_bounds: the sparse download
                 plus the host index) and the host loop over bounds() (lama_slam_view_occupancy: isFree, isOccupied, isUnknown and
                 getProbability per cell through Map::get's hash lookup -- four queries where a publisher needs two, so the loop is
                 reported on its own and halved in `old_path_two_queries_ms`).
  builder  : lama::MapBuilder2D over 160 posed key scans (the largest workload of tools/map_build_bench.py): the same grid calls, and
             the sparse download of the same maps alone (lama_hip_pf_download_map: the floor of the old path, no host loop).
The order of (a) and (b) alternates between repeats.  Also printed per map: the bytes a raster call moves by its algorithm (present
patches x their cell bytes + 128 B of mask where the layer reads it, plus the output) -- over the kernel's time from a separate
`rocprofv3 --kernel-trace` run of `--loop N` (this tool with nothing but N raster calls per layer over the corridor map and, with
--box S, N more over an S x S pixel box around it, the fixed window of a costmap: mostly absent patches) that gives bytes/s;
`--loop N --kernel-db FILE` reads the database that run wrote and prints the rates instead of running anything.
Prints one JSON line per map.  Usage: python tools/raster_bench.py [--repeats 7] [--warmup 2] [--keys 160] [--loop N [--box S] [--kernel-db F]] [--out F]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


GRIDS = [("occupancy", 1), ("occupancy", 8), ("distance", 1), ("distance", 8)]


def grid_calls(obj, acc):
    last = {}
    for what, stride in GRIDS:
        ms, g = timed(lambda: (obj.occupancy_grid if what == "occupancy" else obj.distance_grid)(stride=stride))
        acc.setdefault(f"{what}_grid_stride{stride}_ms", []).append(ms)
        last[(what, stride)] = g
    return last


def algorithmic_bytes(F, ctx, wide):
    """bytes one stride-1 raster of the whole map reads and writes, per layer"""
    out = {}
    for what, kind, cell in (("occupancy", F.MAP_OCCUPANCY, 4), ("distance", F.MAP_DISTANCE, 4 if wide else 2)):
        lo, hi, n = ctx.map_bounds(0, kind)
        pixels = int(hi[0] - lo[0]) * int(hi[1] - lo[1])
        out[what] = {"patches": n, "pixels": pixels, "bytes": n * (1024 * cell + (128 if what == "distance" else 0)) + pixels * (2 if what == "distance" else 1)}
    return out


def kernel_rates(db_file, bytes_by_layer, box_pixels=0):
    """median k_raster time per instantiation from the database a `rocprofv3 --kernel-trace` run of `--loop N` wrote (its `kernels`
    view: name, start, end in ns, grid) -> GB/s against the algorithmic bytes; launches over the large --box are listed apart"""
    import sqlite3
    out = {}
    rows = sqlite3.connect(db_file).execute("select name, end - start, grid_x * grid_y from kernels where name like '%k_raster%'").fetchall()
    for name in sorted({r[0] for r in rows}):
        what = "distance" if "k_raster<2>" in name else "occupancy"
        small = min(r[2] for r in rows if r[0] == name)
        for label, sel in (("map", [r[1] for r in rows if r[0] == name and r[2] == small]), ("box", [r[1] for r in rows if r[0] == name and r[2] != small])):
            if not sel:
                continue
            nbytes = bytes_by_layer[what]["bytes"] + (0 if label == "map" else (box_pixels - bytes_by_layer[what]["pixels"]) * (2 if what == "distance" else 1))
            ns = statistics.median(sel)
            out[f"{what}_{label}"] = {"launches": len(sel), "median_ns": ns, "min_ns": min(sel), "max_ns": max(sel), "bytes": nbytes, "GBps": round(nbytes / ns, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--beams", type=int, default=1080)
    ap.add_argument("--keys", type=int, default=160)
    ap.add_argument("--loop", type=int, default=0, help="only N stride-1 raster calls per layer on the corridor map (for a profiler run)")
    ap.add_argument("--box", type=int, default=0, help="--loop: also N calls per layer over a box of this many pixels a side centred on the map")
    ap.add_argument("--kernel-db", default=None, help="--loop: the rocprofv3 database of an earlier --loop run with the same --box")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import iris_lama_amd.ffi as F
    if F.device_count() == 0:
        raise SystemExit("raster_bench needs an MI355X: there is no CPU fallback")
    rows = []
    total = a.warmup + a.repeats
    # ---- corridor: Slam2D after 40 steps, one more update per repeat
    pts, odom, _ = F.corridor_log(steps=40 + total, beams=a.beams)
    s = F.Slam2D(trans_thresh=0.01, rot_thresh=0.01)
    for k in range(41):
        s.update(pts[k], odom[k])
    ctx = s.hip_context()
    if a.loop:
        lo, hi, _ = ctx.map_bounds(0, F.MAP_OCCUPANCY)
        dlo, dhi, _ = ctx.map_bounds(0, F.MAP_DISTANCE)
        row = {"workload": "raster_loop", "calls_per_layer": a.loop, "box": a.box, "algorithmic": algorithmic_bytes(F, ctx, False)}
        if a.kernel_db:
            row["kernel"] = kernel_rates(a.kernel_db, row["algorithmic"], a.box * a.box)
        else:
            cx, cy = (int(lo[0]) + int(hi[0])) // 2, (int(lo[1]) + int(hi[1])) // 2
            for _ in range(a.loop):
                ctx.rasterize(0, F.RASTER_TRINARY, lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1])
                ctx.rasterize(0, F.RASTER_SQDIST, dlo[0], dlo[1], dhi[0] - dlo[0], dhi[1] - dlo[1])
                if a.box:
                    ctx.rasterize(0, F.RASTER_TRINARY, cx - a.box // 2, cy - a.box // 2, a.box, a.box)
                    ctx.rasterize(0, F.RASTER_SQDIST, cx - a.box // 2, cy - a.box // 2, a.box, a.box)
        print(json.dumps(row), flush=True)
        return
    row = {"workload": "raster_corridor", "steps": 40, "beams": a.beams}
    new, old = {}, {"cold_snapshot_ms": [], "host_loop_four_queries_ms": []}
    for r in range(total):
        s.update(pts[41 + r], odom[41 + r])                          # drops the snapshots
        acc_new, acc_old = {}, {}

        def new_path():
            return grid_calls(s, acc_new)

        def old_path():
            ms, b = timed(lambda: s.view_bounds(0))
            acc_old["cold_snapshot_ms"] = ms
            mn, mx = b[0], b[1]
            xs, ys = np.meshgrid(np.arange(mn[0], mx[0], dtype=np.uint32), np.arange(mn[1], mx[1], dtype=np.uint32))
            cells = np.ascontiguousarray(np.stack([xs.ravel(), ys.ravel()], axis=1))
            acc_old["host_loop_four_queries_ms"], q = timed(lambda: s.view_occupancy(cells))
            return np.where(q[0], 0, np.where(q[1], 100, -1)).astype(np.int8).reshape(ys.shape)
        if r % 2 == 0:
            grids = new_path(); want = old_path()
        else:
            want = old_path(); grids = new_path()
        if not np.array_equal(grids[("occupancy", 1)].data, want):
            raise SystemExit("the grid differs from the host loop over the snapshot")
        if r >= a.warmup:
            for k, v in acc_new.items():
                new.setdefault(k, []).extend(v)
            for k, v in acc_old.items():
                old[k].append(v)
    row["grid"] = {k: spread(v) for k, v in new.items()}
    row["old_path"] = {k: spread(v) for k, v in old.items()}
    row["old_path_two_queries_ms"] = round(statistics.median(old["cold_snapshot_ms"]) + statistics.median(old["host_loop_four_queries_ms"]) / 2, 3)
    row["algorithmic"] = algorithmic_bytes(F, ctx, False)
    s.close()
    print(json.dumps(row), flush=True)
    rows.append(row)
    # ---- builder: MapBuilder2D over --keys posed key scans
    K = a.keys
    pts, _, truth = F.corridor_log(steps=K - 1, beams=a.beams)
    b = F.MapBuilder2D()
    for k in range(K):
        b.add(pts[k], F.pose_from_xyr(*truth[k]))
    b.build()
    ctx = b.hip_context()
    row = {"workload": "raster_builder", "keys": K, "beams": a.beams}
    new, dl = {}, {"download_occupancy_ms": [], "download_distance_ms": []}
    for r in range(total):
        acc = {}
        grid_calls(b, acc)
        t_occ, _ = timed(lambda: ctx.download_map(0, F.MAP_OCCUPANCY))
        t_dm, _ = timed(lambda: ctx.download_map(0, F.MAP_DISTANCE))
        if r >= a.warmup:
            for k, v in acc.items():
                new.setdefault(k, []).extend(v)
            dl["download_occupancy_ms"].append(t_occ); dl["download_distance_ms"].append(t_dm)
    row["grid"] = {k: spread(v) for k, v in new.items()}
    row["sparse_download_alone"] = {k: spread(v) for k, v in dl.items()}
    row["algorithmic"] = algorithmic_bytes(F, ctx, False)
    b.close()
    print(json.dumps(row), flush=True)
    rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
