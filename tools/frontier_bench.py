"""Frontier clusters of device occupancy maps (getFrontiers -> lama_hip_map_frontiers) on two maps:
  corridor : lama::Slam2D over the seeded corridor log of bench.py (ffi.corridor_log, 1080 beams) after 40 steps; every repeat makes
             one more update() and then times the calls below.
  builder  : lama::MapBuilder2D over 160 posed key scans (the map of a few hundred patches of tools/raster_bench.py).
Per map and repeat, in an order that alternates between repeats:
  frontiers_ms        wall clock of one frontiers() call over the whole map (it ends in a stream synchronise);
  kernel_ms           the device time of the same box through HipContext.map_frontiers (events around its launches);
  occupancy_grid_ms   wall clock of occupancy_grid() for the same box: the only route to frontiers before this entry existed, and
                      one that still leaves the labelling to the host -- the FLOOR of the old path, not its cost.
Also printed: the box, the number of clusters and of frontier pixels.  No time here is an acceptance condition.
Prints one JSON line per map.  Usage: python tools/frontier_bench.py [--repeats 7] [--warmup 2] [--keys 160] [--stride 1] [--out F]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def one_repeat(obj, ctx, stride, flip, acc):
    def new_path():
        ms, fs = timed(lambda: obj.frontiers(stride=stride))
        acc.setdefault("frontiers_ms", []).append(ms)
        raw = ctx.map_frontiers(0, fs.x0, fs.y0, fs.width, fs.height, stride)
        acc.setdefault("kernel_ms", []).append(raw.kernel_ms)
        if raw.n != fs.clusters or raw.frontier_pixels != fs.frontier_pixels:
            raise SystemExit("the context call and the class call disagree")
        return fs

    def old_floor():
        ms, g = timed(lambda: obj.occupancy_grid(stride=stride))
        acc.setdefault("occupancy_grid_ms", []).append(ms)
        return g
    if flip:
        g = old_floor(); fs = new_path()
    else:
        fs = new_path(); g = old_floor()
    if (g.x0, g.y0, g.width, g.height) != (fs.x0, fs.y0, fs.width, fs.height):
        raise SystemExit("the grid and the frontiers cover different boxes")
    return fs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--beams", type=int, default=1080)
    ap.add_argument("--keys", type=int, default=160)
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import iris_lama_amd.ffi as F
    if F.device_count() == 0:
        raise SystemExit("frontier_bench needs an MI355X: there is no CPU fallback")
    rows = []
    total = a.warmup + a.repeats

    def report(row, fs, ctx, acc):
        row.update({"stride": a.stride, "box": [fs.x0, fs.y0, fs.width, fs.height], "patches": ctx.map_bounds(0, F.MAP_OCCUPANCY)[2],
                    "clusters": int(fs.clusters), "frontier_pixels": int(fs.frontier_pixels), "largest": int(fs.frontiers["pixels"][0]) if len(fs.frontiers) else 0})
        row["times"] = {k: spread(v[a.warmup:]) for k, v in acc.items()}
        print(json.dumps(row), flush=True)
        rows.append(row)

    # ---- corridor: Slam2D after 40 steps, one more update per repeat
    pts, odom, _ = F.corridor_log(steps=40 + total, beams=a.beams)
    s = F.Slam2D(trans_thresh=0.01, rot_thresh=0.01)
    for k in range(41):
        s.update(pts[k], odom[k])
    acc = {}
    for r in range(total):
        s.update(pts[41 + r], odom[41 + r])
        fs = one_repeat(s, s.hip_context(), a.stride, r % 2 == 1, acc)
    report({"workload": "frontier_corridor", "steps": 40, "beams": a.beams}, fs, s.hip_context(), acc)
    s.close()
    # ---- builder: MapBuilder2D over --keys posed key scans
    K = a.keys
    pts, _, truth = F.corridor_log(steps=K - 1, beams=a.beams)
    b = F.MapBuilder2D()
    for k in range(K):
        b.add(pts[k], F.pose_from_xyr(*truth[k]))
    b.build()
    acc = {}
    for r in range(total):
        fs = one_repeat(b, b.hip_context(), a.stride, r % 2 == 1, acc)
    report({"workload": "frontier_builder", "keys": K, "beams": a.beams}, fs, b.hip_context(), acc)
    b.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
