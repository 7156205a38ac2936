#!/usr/bin/env python3
"""Schedule model of the grouped filter step (lama_hip_pf_match_and_map): what does a pool of 30 particles gain
when contiguous particle groups run ahead of each other on streams of their own?  CPU only.

The exact brushfire is one serial chain of pops per particle, so a step lasts as long as the longest chain among the particles that
have to finish together.  The chains are counted on the CPU oracle for the run bench.py times (seed 42, corridor log, 1080 beams,
5 warm-up + 30 timed updates; `bf_processed` per particle and update), then put into a schedule:

  today      one launch per kernel over the pool, and the next step's first call waits for the map update:
             step = scan match + round trip + ray-cast + pace * longest chain of the pool + round trip
  G groups   per group g, on its own stream: scan match (may start once the host has issued the step and g's previous map update has
             finished) -> round trip -> ray-cast -> pace * longest chain of the group.  The host issues step t + 1 when the scan
             matches of ALL groups of step t are back (the resample decision needs every log-likelihood).  G = 1 only takes the
             wait for the previous map update off the critical path.

Assumed: kernels of different streams overlap freely; a group's scan match and ray-cast take as long as the pool's (latency chains
per particle); launching G times as many kernels costs the host nothing.  The output is a prediction to hold a measurement against
(profiles/INDEX.md), nothing more.

    python tools/chain_schedule_model.py                       # counts the chains (about a minute), prints both tables
    python tools/chain_schedule_model.py --pace 0.636 --scan-match 95 --raycast 96 --round-trip 27 --groups 1,2,3,4,8,30
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def count_chains(particles, warmup, steps, beams, seed):
    """-> pops[update][particle] of the warm-up and timed updates (the first scan, which initialises the filter, left out)"""
    import _oracle as O
    import iris_lama_amd.ffi as F
    pts, odom, _ = F.corridor_log(warmup + steps, beams)
    pf = O.PF(O.default_options(particles=particles, seed=seed))
    pf.set_prior(O.se2(*odom[0]))
    pops = []
    for k in range(warmup + steps + 1):
        assert pf.update(pts[k], O.se2(*odom[k]), float(k))
        if k > 0:                                                   # (the counters are those of the last update)
            pops.append([pf.counters(i)["bf_processed"] for i in range(particles)])
    return np.array(pops)


def blocks(particles, groups):
    """the library's split (lama_hip_ctx_create): contiguous blocks of ceil(P / G), of the next multiple of 8 where that still makes G"""
    per = -(-particles // groups)
    per8 = -(-per // 8) * 8
    if -(-particles // per8) == groups:
        per = per8
    return [(min(particles, k * per), min(particles, (k + 1) * per)) for k in range(groups) if min(particles, k * per) < particles]


def today(pops, a):
    return sum(a.scan_match + a.round_trip + a.raycast + a.pace * p.max() + a.round_trip for p in pops)


def grouped(pops, groups, a):
    bl = blocks(pops.shape[1], groups)
    free = [0.0] * len(bl)            # when group g's stream has finished its previous map update
    host = 0.0                        # when the host issues the step
    for p in pops:
        back = []
        for g, (lo, hi) in enumerate(bl):
            matched = max(host, free[g]) + a.scan_match + a.round_trip
            back.append(matched)
            free[g] = matched + a.raycast + a.pace * p[lo:hi].max()
        host = max(back)
    return max(free)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--particles", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--beams", type=int, default=1080)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--pace", type=float, default=0.636, help="us per pop of a brushfire chain")
    ap.add_argument("--scan-match", type=float, default=95.0, help="us")
    ap.add_argument("--raycast", type=float, default=96.0, help="us, the six ray-cast kernels together")
    ap.add_argument("--round-trip", type=float, default=27.0, help="us per host round trip")
    ap.add_argument("--groups", type=str, default="1,2,3,4,8,30")
    a = ap.parse_args()
    pops = count_chains(a.particles, a.warmup, a.steps, a.beams, a.seed)
    windows = {f"{a.steps} timed steps": pops[a.warmup:], "the 20-step window": pops[a.warmup:a.warmup + 20]}
    timed = pops[a.warmup:]
    per_particle = timed.sum(axis=0)
    print(f"pops per particle and update, {a.particles} particles, {a.beams} beams, seed {a.seed}, updates {a.warmup + 1} .. {a.warmup + a.steps}")
    print(f"  sum over steps of the longest chain of the step   {int(timed.max(axis=1).sum()):>8}")
    print(f"  longest per-particle total over the same steps    {int(per_particle.max()):>8}")
    print(f"  mean per-particle total                           {per_particle.mean():>10.1f}")
    print(f"  particle with the longest chain, step by step     {timed.argmax(axis=1).tolist()}")
    print(f"constants: pace {a.pace} us/pop, scan match {a.scan_match} us, ray-cast {a.raycast} us, round trip {a.round_trip} us")
    print("| groups | blocks | " + " | ".join(f"step time vs today, {w}" for w in windows) + " |")
    print("|---:|---|" + "---:|" * len(windows))
    for g in [int(x) for x in a.groups.split(",") if x]:
        g = min(g, a.particles)
        cells = [f"{grouped(p, g, a) / today(p, a):.3f}" for p in windows.values()]
        sizes = [hi - lo for lo, hi in blocks(a.particles, g)]
        print(f"| {g} | {'+'.join(str(s) for s in sizes) if len(sizes) <= 8 else str(len(sizes)) + ' blocks'} | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()
