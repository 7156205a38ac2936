"""Routes through device maps (planRoutes -> lama_hip_map_travel) in two settings:
  corridor   : lama::Slam2D over the seeded corridor log of bench.py (ffi.corridor_log, 1080 beams) after 40 steps; every repeat makes
               one more update() and then plans from a fixed start to every frontier seed, goal_reach 2.
  floor_plan : lama::Loc2D on a generated office floor of 100 m x 60 m at 0.05 m (bench.floor_plan_cells: rooms of 4 m, doors of
               1 m), stride 1, one source, 64 random goals, goal_reach 4 -- the distance map alone decides what is traversable.
Per setting and repeat, in an order that alternates between repeats:
  routes_ms      wall clock of one routes() call (it ends in a stream synchronise);
  kernel_ms      the device time of the same call through HipContext.travel (events around its launches; the host's batched
                 read-backs lie inside), with rounds, tiles run, tiles per round, the largest round and the read-backs;
  host_path_ms   the path a caller has without the entry point: the dense grid(s) of the same box down (occupancy_grid() and / or
                 distance_grid()), then classification, a binary-heap Dijkstra over the same move rules, the goals' answers and the
                 walks back, in C++ on one core (tools/travel_host_path.cpp, built here with g++ -O2); grids_ms is its download part.
The host path's routes must equal the device's.  No time here is an acceptance condition.
Prints one JSON line per setting.  Usage: python tools/travel_bench.py [--repeats 7] [--warmup 2] [--plan 100,60] [--out F]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OFF = (2642244 >> 1) * 32
NONE = 0xFFFFFFFF


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def host_helper():
    src, out = os.path.join(ROOT, "tools", "travel_host_path.cpp"), os.path.join(ROOT, "tools", "_tmp", "libtravel_host_path.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", out], check=True)
    L = C.CDLL(out)
    vp, u32 = C.c_void_p, C.c_uint32
    L.travel_host_path.argtypes = [vp, vp, u32, u32, u32, u32, u32, u32, vp, u32, vp, u32, vp, vp]
    L.travel_host_path.restype = C.c_uint64
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Setting:
    """one object, one box and one set of parameters; sources and goals as world points"""

    def __init__(self, F, H, obj, ctx, opts, world_box, distance_only):
        self.F, self.H, self.obj, self.ctx, self.opts, self.world_box, self.distance_only = F, H, obj, ctx, opts, world_box, distance_only

    def grids(self):
        occ = None if self.distance_only else self.obj.occupancy_grid(world_box=self.world_box)
        ref = occ
        if ref is None:
            dist = self.obj.distance_grid(world_box=self.world_box)
        else:
            res = ref.resolution
            dist = self.obj.distance_grid(world_box=(ref.origin[0], ref.origin[1], ref.origin[0] + (ref.width - 1) * res, ref.origin[1] + (ref.height - 1) * res))
        return occ, dist

    def pixels(self, g, pts):
        inv = 1.0 / g.resolution
        out = []
        for x, y in pts:                                            # Map::w2m: (uint32_t)(x / resolution + offset + 0.5)
            cx, cy = int(inv * x + OFF + 0.5), int(inv * y + OFF + 0.5)
            i, j = cx - g.x0, cy - g.y0
            out.append(j * g.width + i if 0 <= i < g.width and 0 <= j < g.height else NONE)
        return np.array(out, dtype=np.uint32)

    def host_path(self, here, goals):
        t_grid, (occ, dist) = timed(self.grids)
        inv = 1.0 / dist.resolution
        clear = math.ceil(self.opts["robot_radius"] * inv)
        prefer = max(clear, math.ceil(self.opts["preferred_clearance"] * inv))
        src, gl = self.pixels(dist, [here]), self.pixels(dist, goals)
        field = np.empty((dist.height, dist.width), dtype=np.uint32)
        routes = np.zeros((len(gl), 4), dtype=np.uint32)

        def run():
            return self.H.travel_host_path(_p(None if occ is None else np.ascontiguousarray(occ.data)), _p(np.ascontiguousarray(dist.data)), dist.width, dist.height, clear,
                                           prefer, self.opts["near_factor"], len(src), _p(src), len(gl), _p(gl), self.opts["goal_reach"], _p(field), _p(routes))
        t_run, pops = timed(run)
        return t_grid, t_grid + t_run, routes, field, dist, (clear, prefer), int(pops)

    def one_repeat(self, here, goals, flip, acc, info):
        def new_path():
            ms, rs = timed(lambda: self.obj.routes([here], goals, world_box=self.world_box, **self.opts))
            acc.setdefault("routes_ms", []).append(ms)
            return rs

        def old_path():
            t_grid, t_all, routes, field, dist, cells, pops = self.host_path(here, goals)
            acc.setdefault("grids_ms", []).append(t_grid)
            acc.setdefault("host_path_ms", []).append(t_all)
            return routes, dist, cells, pops
        if flip:
            (hr, dist, cells, pops), rs = old_path(), new_path()
        else:
            rs, (hr, dist, cells, pops) = new_path(), old_path()
        if (dist.x0, dist.y0, dist.width, dist.height) != (rs.x0, rs.y0, rs.width, rs.height):
            raise SystemExit("the grids and the routes cover different boxes")
        for k, name in enumerate(("status", "pixel", "cost", "steps")):
            if not np.array_equal(rs.routes[name], hr[:, k]):
                raise SystemExit(f"the host path and the device disagree on {name}")
        inv = 1.0 / rs.resolution
        cell = lambda pts: [(int(inv * x + OFF + 0.5), int(inv * y + OFF + 0.5)) for x, y in pts]
        raw = self.ctx.travel(0, rs.x0, rs.y0, rs.width, rs.height, cell([here]), cell(goals), clearance_cells=cells[0], prefer_cells=cells[1],
                              near_factor=self.opts["near_factor"], goal_reach=self.opts["goal_reach"], path_cap=self.opts["max_path_points"])
        if not np.array_equal(raw.routes["cost"], rs.routes["cost"]):
            raise SystemExit("the context call and the class call disagree")
        st = self.ctx.travel_stats()
        acc.setdefault("kernel_ms", []).append(raw.kernel_ms)
        for k in ("rounds", "tiles_run", "max_tiles", "readbacks"):
            acc.setdefault(k, []).append(st[k])
        info.update({"box": [rs.x0, rs.y0, rs.width, rs.height], "tiles": ((rs.width + 31) // 32) * ((rs.height + 31) // 32), "goals": len(goals),
                     "reached": int((rs.routes["status"] == 0).sum()), "longest_steps": int(rs.routes["steps"].max()) if len(goals) else 0,
                     "clearance_cells": cells[0], "prefer_cells": cells[1], "host_heap_pops": pops})

    def find_start(self, candidates):
        """the first candidate from which the host path reaches at least 1000 pixels"""
        for here in candidates:
            _, _, _, field, _, _, _ = self.host_path(here, [])
            if int((field != NONE).sum()) >= 1000:
                return here
        raise SystemExit("no start point with room to move")


def report(row, acc, info, warmup, rows):
    row.update(info)
    row["times"] = {k: spread(v[warmup:]) for k, v in acc.items() if k.endswith("_ms")}
    row["rounds"] = spread(acc["rounds"][warmup:])
    row["tiles_run"] = spread(acc["tiles_run"][warmup:])
    row["tiles_per_round"] = round(statistics.median(t / max(r, 1) for t, r in zip(acc["tiles_run"][warmup:], acc["rounds"][warmup:])), 2)
    row["largest_round"] = max(acc["max_tiles"][warmup:])
    row["readbacks"] = spread(acc["readbacks"][warmup:])
    print(json.dumps(row), flush=True)
    rows.append(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--beams", type=int, default=1080)
    ap.add_argument("--plan", default="100,60", help="width,height of the generated floor plan in metres")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    import iris_lama_amd.ffi as F
    if F.device_count() == 0:
        raise SystemExit("travel_bench needs an MI355X: there is no CPU fallback")
    H = host_helper()
    rows, total = [], a.warmup + a.repeats
    # ---- corridor: Slam2D after 40 steps, one more update per repeat; routes to the frontier seeds
    opts = dict(robot_radius=0.1, preferred_clearance=0.4, near_factor=3, goal_reach=2, max_path_points=256)
    pts, odom, _ = F.corridor_log(steps=40 + total, beams=a.beams)
    s = F.Slam2D(trans_thresh=0.01, rot_thresh=0.01)
    for k in range(41):
        s.update(pts[k], odom[k])
    st = Setting(F, H, s, s.hip_context(), opts, None, False)
    occ, dist = st.grids()
    order = np.argsort(-np.where(occ.data == 0, dist.data.astype(np.int64), -1), axis=None, kind="stable")[:64]
    here = st.find_start([(occ.origin[0] + occ.resolution * float(p % occ.width), occ.origin[1] + occ.resolution * float(p // occ.width)) for p in order])
    acc, info = {}, {}
    for r in range(total):
        s.update(pts[41 + r], odom[41 + r])
        goals = [f["seed"].tolist() for f in s.frontiers(min_pixels=2).frontiers]
        st.one_repeat(here, goals, r % 2 == 1, acc, info)
    report({"workload": "travel_corridor", "steps": 40, "beams": a.beams, **opts}, acc, info, a.warmup, rows)
    s.close()
    # ---- floor plan: Loc2D, the distance map only
    W, Hm = (float(v) for v in a.plan.split(","))
    cells = bench.floor_plan_cells(W, Hm)
    world = (cells.astype(np.float64) - OFF) * 0.05
    loc = F.Loc2D(l2_max=1.0)
    loc.set_obstacles_world(world)
    opts = dict(robot_radius=0.2, preferred_clearance=0.5, near_factor=3, goal_reach=4, max_path_points=256)
    st = Setting(F, H, loc, loc.hip_context(), opts, (0.0, 0.0, W - 0.05, Hm - 0.05), True)
    here = (W / 2 + 1.3, Hm / 2 - 0.9)                               # inside a room, off its centre
    rng = np.random.default_rng(7)
    goals = np.stack([rng.uniform(0.5, W - 0.5, 64), rng.uniform(0.5, Hm - 0.5, 64)], axis=1).tolist()
    acc, info = {}, {}
    for r in range(total):
        st.one_repeat(here, goals, r % 2 == 1, acc, info)
    report({"workload": "travel_floor_plan", "plan_m": [W, Hm], "resolution_m": 0.05, "l2_max_m": 1.0, **opts}, acc, info, a.warmup, rows)
    loc.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
