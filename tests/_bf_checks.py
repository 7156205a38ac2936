"""Checks of the exact brushfire (k_brushfire / bf_particle, k_brushfire_slow: lama_kernels.h) on obstacle events constructed cell by
cell, one regime of the pop body per case.  Shared by tests/test_brushfire_gpu.py and the lane-simulator tests
(tests/test_brushfire_sim.py).

Two forms.  dm_case: obstacle cells through lama_hip_map_add_obstacles (k_dm_add_obstacles and the three brushfire stages -- that
entry point always launches the wave pair) against the oracle's DynamicDistanceMap add + update.  EventRun: the oracle filter's own
maps are edited in place (solid obstacles, cells ARMED so that one more free visit removes them: 4 * occupied == visited), uploaded
to the device, and ONE lattice scan (tests/_ray_checks.py: sensor on a cell centre, integer cell deltas) is fed to both; the
add / remove events that scan produces are derived first, by replaying its cells -- the reference's computeRay -- against the
uploaded counts, and asserted to be exactly the ones the case lists.  The form of the first stage (cfg.brushfire_waves 2 or 1) is
asserted from the counters.

Reference: the oracle, bit for bit (assert_maps_equal: DM_FIELDS, OCC_FIELDS, masks, patch sets), no tolerance anywhere; the
counter delta bf_cells equals the oracle's pop count.  Every case asserts from the oracle's stats() deltas and the device
counters that it reached the regime it names; a case that did not fails.
"""
import math

import numpy as np

import _oracle as O
import _ray_checks as RC
import _reference as R
from _cmp import DM_FIELDS, OCC_FIELDS, assert_maps_equal
from _mapbuild import OFF

WAVES = (2, 1)
STRIDE = 2642244                    # patch id = (x >> 5) * STRIDE + (y >> 5), cell = (x & 31) | (y & 31) << 5 (Map::m2p / m2c)
BASE = (160, 96)                    # where the cases are built, in cells from the first sensor: patch aligned, 5 patches off
FIRST_SCAN = [(0, 3)]               # the filter's first scan: one beam, far from BASE
LQ, RQ = 1024, 256                  # first-stage LDS queues (lama_kernels.h: LQ_SMALL, RQ_SMALL)
LQ_BIG, RQ_BIG = 8192, 2048         # resume stage
DISC_10 = 305                       # cells with dx^2 + dy^2 < 100: what one obstacle lowers at l2_max = 0.5 m


def disc(r):
    """number of cells one isolated obstacle lowers at a reach of r cells (new_sqdist < max_sqdist: strictly inside)"""
    return sum(1 for x in range(-r, r + 1) for y in range(-r, r + 1) if x * x + y * y < r * r)


assert disc(10) == DISC_10


def _cell_of(dump, x, y):
    p = dump.get((x >> 5) * STRIDE + (y >> 5))
    return None if p is None else p[0][(x & 31) | ((y & 31) << 5)]


def stats_delta(after, before):
    d = {k: after[k] - before[k] for k in after}
    d["max_queue_last"] = after["max_queue_last"]
    d["pops"] = d["raise_pops"] + d["lower_pops"]
    return d


# ------------------------------------------------------------------------------------------------ additions
def dm_case(F, cells, l2_max, what=""):
    """`cells` (relative to BASE) through lama_hip_map_add_obstacles on a fresh context, against DM.add + update -> (oracle stats,
    device counters, oracle map)"""
    cells = np.array([(OFF + BASE[0] + x, OFF + BASE[1] + y) for x, y in cells], dtype=np.uint32)
    dm = O.DM.new(l2_max=l2_max)
    for x, y in cells:
        dm.add(int(x), int(y))
    pops = dm.update()
    st = dm.stats()
    assert pops == st["raise_pops"] + st["lower_pops"] and st["raise_pops"] == 0
    ctx = F.HipContext(F.default_cfg(particles=1, l2_max=l2_max))
    try:
        ctx.add_obstacles(0, cells)
        c = ctx.counters()
        assert_maps_equal(ctx.download_map(0, F.MAP_DISTANCE), dm.dump(), DM_FIELDS, f"{what}: dm")
        assert c["bf_cells"] == pops, (what, c["bf_cells"], pops)
    finally:
        ctx.close()
    return st, c, dm


# ------------------------------------------------------------------------------------------------ removals and mixed events
def set_counts(occ, cell, occupied, visited):
    """a fresh cell of the oracle's occupancy map to (occupied, visited)"""
    for _ in range(occupied):
        occ.set_occupied(*cell)
    for _ in range(visited - occupied):
        occ.set_free(*cell)


def arm(occ, dm, cell):
    """an obstacle that the next free visit removes: occupied / visited = 1 / 4 is neither free nor occupied, 1 / 5 is free"""
    set_counts(occ, cell, 1, 4)
    dm.add(*cell)


def solid(occ, dm, cell):
    """an obstacle that survives the free visits of a case (8 / 8) and takes a hit without an event"""
    set_counts(occ, cell, 8, 8)
    dm.add(*cell)


class EventRun:
    """P particles of the oracle's filter with maps edited in place, the same maps uploaded to a device context, one scan for both."""

    def __init__(self, F, waves, l2_max=0.5, P=1, base=BASE, what="", **cfg):
        self.F, self.waves, self.P, self.base, self.what = F, waves, P, base, what
        pose0 = RC.sensor(0, 0)
        self.pf = O.PF(O.default_options(particles=P, seed=3, l2_max=l2_max))
        self.pf.set_prior(pose0)
        assert self.pf.update(RC.lattice(FIRST_SCAN), pose0, 0.0)
        self.ctx = F.HipContext(F.default_cfg(particles=P, brushfire_waves=waves, l2_max=l2_max, **cfg))
        self.uploaded = False

    def abs(self, c):
        return (OFF + self.base[0] + int(c[0]), OFF + self.base[1] + int(c[1]))

    def rel(self, x, y):
        return (int(x) - OFF - self.base[0], int(y) - OFF - self.base[1])

    def prepare(self, armed=(), solids=(), counts=None, p=None):
        """edit particle p's maps (all particles': p None); cells relative to the base"""
        for q in (range(self.P) if p is None else [p]):
            occ, dm = self.pf.occ(q), self.pf.dm(q)
            for c in armed:
                arm(occ, dm, self.abs(c))
            for c in solids:
                solid(occ, dm, self.abs(c))
            for c, (o, v) in (counts or {}).items():
                set_counts(occ, self.abs(c), o, v)

    def upload(self):
        F = self.F
        for q in range(self.P):
            self.pf.dm(q).update()
            self.ctx.upload_map(q, F.MAP_DISTANCE, self.pf.dm(q).dump())
            self.ctx.upload_map(q, F.MAP_OCCUPANCY, self.pf.occ(q).dump())
        self.ctx.set_poses(self.pf.poses())
        self.uploaded = True
        self.compare("after the upload")

    def events(self, q, pose, pts):
        """the add / remove events of the scan for particle q, in order: PFSlam2D::updateParticleMaps on the uploaded counts
        (setOccupied of the hit first, then setFree along the reference's computeRay), -> [("add" | "remove", relative cell)]"""
        occ, dm = self.pf.occ(q).dump(), self.pf.dm(q).dump()
        cnt, obst, out = {}, {}, []

        def load(x, y):
            if (x, y) not in cnt:
                f, d = _cell_of(occ, x, y), _cell_of(dm, x, y)
                cnt[(x, y)] = [0, 0] if f is None else [int(f["occupied"]), int(f["visited"])]
                obst[(x, y)] = d is not None and bool(d["valid"]) and int(d["sqdist"]) == 0
            return cnt[(x, y)]

        prob = lambda f: 0.25 if f[1] == 0 else f[0] / f[1]
        d, _, marks, starts = RC.geometry(pose, pts)
        for k in range(len(d)):
            start = starts[k]
            hit = start + d[k]
            if marks[k]:
                f = load(int(hit[0]), int(hit[1]))
                was = prob(f) > 0.25
                f[0] += 1; f[1] += 1
                if not was and prob(f) > 0.25 and not obst[(int(hit[0]), int(hit[1]))]:
                    obst[(int(hit[0]), int(hit[1]))] = True
                    out.append(("add", self.rel(hit[0], hit[1])))
            for c in RC.ray_cells(start, hit):
                key = (int(c[0]), int(c[1]))
                f = load(*key)
                was = prob(f) < 0.25
                f[1] += 1
                if not was and prob(f) < 0.25 and obst[key]:
                    obst[key] = False
                    out.append(("remove", self.rel(*key)))
        return out

    def scan(self, sensor, deltas, expect, what="", exact=True):
        """one scan from the cell `sensor` (relative to the base) with the beams `deltas`; `expect`: the ordered events, one list
        for all particles or a list per particle -> (oracle stats delta per particle, device counter delta).  exact=False
        (tests/_bf_canon_checks.py: cfg.brushfire_mode = 1) leaves out the two assertions that hold for the exact kernels only:
        the form of the first stage, and bf_cells == pops (the canonical kernel does not pop a cell's duplicates again)."""
        if not self.uploaded:
            self.upload()
        pose = RC.sensor(self.base[0] + sensor[0], self.base[1] + sensor[1])
        pts = RC.lattice(deltas)
        RC.assert_deltas(pose, pts, deltas, f"{self.what} {what}")
        per = expect if (len(expect) == self.P and expect and isinstance(expect[0], list)) else [expect] * self.P
        for q in range(self.P):
            got = self.events(q, pose, pts)
            assert got == [(k, tuple(c)) for k, c in per[q]], (self.what, what, q, got[:12], len(got), len(per[q]))
        before = [self.pf.dm(q).stats() for q in range(self.P)]
        c0 = self.ctx.counters()
        poses = np.stack([pose] * self.P)
        self.pf.set_poses(poses); self.pf.stage_set_scan(pts); self.pf.stage_update_maps()
        self.ctx.set_poses(poses); self.ctx.update_maps(pts)
        c1 = self.ctx.counters()
        st = [stats_delta(self.pf.dm(q).stats(), before[q]) for q in range(self.P)]
        dc = {k: c1[k] - c0[k] for k in ("bf_cells", "brushfire_handovers", "brushfire_routed", "brushfire_early")}
        dc["brushfire_waves"] = c1["brushfire_waves"]
        assert not exact or dc["brushfire_waves"] == self.waves, (self.what, what, dc)
        self.compare(what)
        assert not exact or dc["bf_cells"] == sum(s["pops"] for s in st), (self.what, what, dc, [s["pops"] for s in st])
        return st, dc

    def compare(self, what):
        F = self.F
        for q in range(self.P):
            tag = f"{self.what} {what} waves {self.waves} p{q}"
            assert_maps_equal(self.ctx.download_map(q, F.MAP_OCCUPANCY), self.pf.occ(q).dump(), OCC_FIELDS, tag + ": occ")
            assert_maps_equal(self.ctx.download_map(q, F.MAP_DISTANCE), self.pf.dm(q).dump(), DM_FIELDS, tag + ": dm")

    def close(self):
        self.ctx.close()


def run_events(F, waves, armed=(), solids=(), counts=None, sensor=(0, 0), deltas=(), expect=(), l2_max=0.5, what="", base=BASE):
    run = EventRun(F, waves, l2_max=l2_max, what=what, base=base)
    try:
        run.prepare(armed, solids, counts)
        st, dc = run.scan(sensor, list(deltas), list(expect), what)
        return st[0], dc, run.pf.dm(0).dump()
    finally:
        run.close()


# A removal beam: from the sensor at (-30, y) along +x to a solid cell at (+30, y) -- both 30 cells, three reaches, from everything
# a case builds around (0, 0), so neither the far end's disc nor the first scan's touches it.
FAR = 30


def row_beam(y=0):
    """-> (sensor, delta, solid end) of the beam that crosses every cell (-29 .. 29, y)"""
    return (-FAR, y), (2 * FAR, 0), (FAR, y)


# ------------------------------------------------------------------------------------------------ 1. single events
def check_single_add(F, waves):
    """one hit on an untouched cell in empty space: the disc of 305 cells, every pop fires lower(), no raise"""
    st, dc, _ = run_events(F, waves, sensor=(-4, 0), deltas=[(4, 0)], expect=[("add", (0, 0))], what="single add")
    assert st["raise_pops"] == 0 and st["lower_fired"] == DISC_10 and st["tie_overwrites"] == 0 and dc["brushfire_handovers"] == 0, (st, dc)


def check_single_add_on_a_patch_corner(F, waves):
    """the same on cell (31, 31) of a patch, none of the three patches around that corner allocated: lower() allocates them
    (patch sets and mask bits are part of the comparison)"""
    run = EventRun(F, waves, what="add on a patch corner")
    try:
        cx, cy = run.abs((31, 31))
        before = set(run.pf.dm(0).dump())
        around = {((cx + dx) >> 5) * STRIDE + ((cy + dy) >> 5) for dx in (0, 1) for dy in (0, 1)}
        assert len(around) == 4 and not (around & before) and (cx & 31, cy & 31) == (31, 31)
        st, _ = run.scan((31, 27), [(0, 4)], [("add", (31, 31))])
        assert around <= set(run.pf.dm(0).dump()) and st[0]["lower_fired"] == DISC_10 and st[0]["raise_pops"] == 0, st
    finally:
        run.close()


def check_single_removal(F, waves):
    """one armed obstacle in open space: its whole disc is raised, nothing is lowered again"""
    s, d, end = row_beam()
    st, _, _ = run_events(F, waves, armed=[(0, 0)], solids=[end], sensor=s, deltas=[d], expect=[("remove", (0, 0))], what="single removal")
    assert st["raise_pops"] == DISC_10 and st["lower_pops"] == 0 and st["lower_fired"] == 0, st


def check_single_removal_on_a_patch_corner(F, waves):
    """raise() get()s all four neighbours of the cell it pops.  An obstacle that exists has had them since its lower() ran, so the
    cell (31, 31) is added AND removed in this update (a free cell seen twice, 0 / 2, is hit and then crossed twice): addObstacle
    allocates its own patch, the raise pop the neighbour's across the patch edge, and the lower pop finds no obstacle -- the patch
    to the right exists only because raise() allocated it."""
    run = EventRun(F, waves, what="removal on a patch corner")
    try:
        run.prepare(solids=[(31, 31 + FAR)], counts={(31, 31): (0, 2)})
        cx, cy = run.abs((31, 31))
        own, right = (cx >> 5) * STRIDE + (cy >> 5), ((cx + 1) >> 5) * STRIDE + (cy >> 5)
        run.pf.dm(0).update()
        have = set(run.pf.dm(0).dump())
        assert own not in have and right not in have and (cx & 31, cy & 31) == (31, 31)
        up = (0, 2 * FAR)
        st, _ = run.scan((31, 31 - FAR), [(0, FAR), up, up], [("add", (31, 31)), ("remove", (31, 31))])
        have = set(run.pf.dm(0).dump())
        assert st[0]["raise_pops"] == 1 and st[0]["lower_pops"] == 1 and st[0]["lower_fired"] == 0 and own in have and right in have, st
    finally:
        run.close()


# ------------------------------------------------------------------------------------------------ 2. two obstacles
PAIR_OFFSETS = {"1": (0, 1), "sqrt 2": (1, 1), "2": (0, 2), "5": (3, 4), "11": (0, 11)}


def check_one_of_two_removed(F, waves, which):
    """the survivor at `which` cells from the removed one: the raise wave meets cells that point at the survivor (pushed into the
    lower queue), and the lower wave re-floods what was raised -- the raise -> lower switch with a lower queue filled by raise()"""
    s, d, end = row_beam()
    off = PAIR_OFFSETS[which]
    st, _, _ = run_events(F, waves, armed=[(0, 0)], solids=[end, off], sensor=s, deltas=[d], expect=[("remove", (0, 0))], what=f"pair at {which}")
    assert st["raise_pops"] >= 100 and st["lower_fired"] >= 50 and st["lower_pops"] >= st["lower_fired"], st


def check_both_removed(F, waves):
    s, d, end = row_beam()
    st, _, _ = run_events(F, waves, armed=[(0, 0), (3, 0)], solids=[end], sensor=s, deltas=[d], expect=[("remove", (0, 0)), ("remove", (3, 0))], what="both removed")
    assert st["raise_pops"] > DISC_10 and st["lower_fired"] == 0, st


def check_removal_and_addition_in_one_update(F, waves):
    """both queues hold an entry when the brushfire starts"""
    s, d, end = row_beam()
    st, _, _ = run_events(F, waves, armed=[(0, 0)], solids=[end, (0, 5)], sensor=s, deltas=[(FAR + 4, 3), d],
                           expect=[("add", (4, 3)), ("remove", (0, 0))], what="removal and addition")
    assert st["raise_pops"] >= 100 and st["lower_fired"] >= 100, st


# ------------------------------------------------------------------------------------------------ 3. the same cell twice
def check_removed_then_added_again(F, waves):
    """an early beam crosses the armed cell (1 / 4 -> 1 / 5: removed), a later one hits it (2 / 6: added): it is in both queues"""
    s, d, end = row_beam()
    st, _, _ = run_events(F, waves, armed=[(0, 0)], solids=[end, (6, 2)], sensor=s, deltas=[d, (FAR, 0)],
                           expect=[("remove", (0, 0)), ("add", (0, 0))], what="removed, added again")
    # the raise pop finds the cell an obstacle again: its four neighbours go to the lower queue, nothing else is raised; the lower
    # pop of the cell itself does not fire (raise() has cleared its is_queued), the four neighbours' do
    assert st["raise_pops"] == 1 and st["lower_pops"] == 5 and st["lower_fired"] == 4, st


def check_added_then_removed(F, waves):
    """a free cell seen twice (0 / 2) is hit (1 / 3: added) and crossed by two later beams (1 / 4, 1 / 5: removed)"""
    s, d, end = row_beam()
    st, _, _ = run_events(F, waves, solids=[end, (6, 2)], counts={(0, 0): (0, 2)}, sensor=s, deltas=[(FAR, 0), d, d],
                           expect=[("add", (0, 0)), ("remove", (0, 0))], what="added, removed")
    assert st["raise_pops"] >= 1 and st["lower_pops"] >= 1, st


# ------------------------------------------------------------------------------------------------ 4. ties
# cells equidistant from two and from four obstacles: (+-1, +-2)-type offsets (5 = 1 + 4) and 25 = 9 + 16 = 0 + 25
TIE_OBSTACLES = [(0, 0), (2, 4), (4, 0), (-3, 4), (5, 5), (-5, 0), (0, -5), (3, -4), (10, 0), (7, 4)]


def check_ties_on_addition(F, waves):
    deltas = [(x + FAR, y + 7) for x, y in TIE_OBSTACLES]
    st, _, _ = run_events(F, waves, sensor=(-FAR, -7), deltas=deltas, expect=[("add", c) for c in TIE_OBSTACLES], what="ties, added")
    # cells lowered twice before they are popped: the second pop finds is_queued cleared and does not fire (NOT the fast path's
    # `stale` branch, which needs the older of two entries to pop first: DESIGN.md 2d)
    assert st["lower_pops"] > st["lower_fired"] > DISC_10, st


def tied_cells(obstacles, r=10):
    """cells within reach whose two nearest obstacles are equally far"""
    out = 0
    for x in range(-r - 6, r + 12):
        for y in range(-r - 6, r + 12):
            d = sorted((x - a) ** 2 + (y - b) ** 2 for a, b in obstacles)
            out += d[0] < r * r and d[0] == d[1]
    return out


def check_ties_on_removal(F, waves, which):
    """`which` of the tied obstacles are removed: the lower wave floods the raised cells again from the survivors, whose fronts
    meet on cells that are equally far from two of them (the comparison of dynamic_distance_map.cpp:308-317 with a live obstacle)"""
    s, d, end = row_beam()
    solids = [c for c in TIE_OBSTACLES if c[1] != 0]
    armed = [c for c in TIE_OBSTACLES if c[1] == 0][:which]
    assert tied_cells(solids) >= 10
    st, _, _ = run_events(F, waves, armed=armed, solids=solids + [end], sensor=s, deltas=[d], expect=[("remove", c) for c in sorted(armed)],
                           what=f"ties, {which} removed")
    assert st["raise_pops"] >= 30 and st["lower_fired"] >= 30, st


# Found by a search over random event sequences on the oracle (tie_overwrites > 0 in 3 of 1,513 four-update sequences, in none of
# 30,000 single updates of a map built in one go), minimised: obstacles that arrive in SEPARATE updates leave cells that keep their
# first obstacle although a later one is as near.  The raise wave of (4, 10) then does not reach every cell that points at it, and
# the lower wave meets a cell whose obstacle is dead at the very distance it offers: the overwrite rule's last term.
DEAD_TIE = [(2, 9), (4, 10), (5, 11)]


def check_tie_with_a_dead_obstacle(F, waves):
    run = EventRun(F, waves, what="tie with a dead obstacle")
    try:
        run.prepare(solids=[(4, 10 + FAR)])
        for k, c in enumerate(DEAD_TIE):
            run.prepare(armed=[c]) if k == 1 else run.prepare(solids=[c])
            run.pf.dm(0).update()
        st, _ = run.scan((4, 10 - FAR), [(0, 2 * FAR)], [("remove", DEAD_TIE[1])])
        assert st[0]["tie_overwrites"] >= 1 and 0 < st[0]["raise_pops"] < DISC_10 and st[0]["lower_fired"] > 0, st
    finally:
        run.close()


# ------------------------------------------------------------------------------------------------ cases with a history
# Branches that only stale obstacle offsets reach need a map with a history: obstacles that came and went in EARLIER updates.  A
# case is {history: [[("add" | "remove", cell), ...] per earlier update], armed: cells the scan removes, adds: cells it hits}.  The
# history runs on the oracle's distance map alone; then every live obstacle gets solid counts, the armed ones armed counts, and
# one scan from H_SENSOR follows: a beam through every armed cell to the solid cell twice as far, then the hits.
H_SENSOR = (12, -40)


def check_history_case(F, waves, case, l2_max=0.5, what="history"):
    run = EventRun(F, waves, l2_max=l2_max, what=what)
    try:
        dm, occ = run.pf.dm(0), run.pf.occ(0)
        live = []
        for events in case["history"]:
            for kind, c in events:
                (dm.add if kind == "add" else dm.remove)(*run.abs(c))
                live.append(c) if kind == "add" else live.remove(c)
            dm.update()
        ends = [(2 * x - H_SENSOR[0], 2 * y - H_SENSOR[1]) for x, y in case["armed"]]
        for c in live:
            set_counts(occ, run.abs(c), *((1, 4) if c in case["armed"] else (8, 8)))
        run.prepare(solids=[e for e in ends if e not in live])
        deltas = [(ex - H_SENSOR[0], ey - H_SENSOR[1]) for ex, ey in ends] + [(x - H_SENSOR[0], y - H_SENSOR[1]) for x, y in case["adds"]]
        expect = [("remove", c) for c in case["armed"]] + [("add", c) for c in case["adds"]]
        st, dc = run.scan(H_SENSOR, deltas, expect, what)
        return st[0], dc
    finally:
        run.close()


# frozen from the same search (40 histories with tie overwrites among 7,987 random ones): two removals and an addition in the update
# that meets the dead obstacle
HISTORY_TIE = dict(history=[[("add", (5, 10)), ("add", (1, 2))], [("add", (2, 4)), ("add", (4, 0)), ("add", (0, 1))]],
                   armed=[(1, 2), (5, 10)], adds=[(7, 4)])


def check_tie_with_a_dead_obstacle_among_other_events(F, waves):
    st, _ = check_history_case(F, waves, HISTORY_TIE, what="tie with a dead obstacle, mixed events")
    assert st["tie_overwrites"] >= 1 and st["raise_pops"] > 0 and st["lower_pops"] > st["lower_fired"] > 0, st


# ------------------------------------------------------------------------------------------------ 5. directory-cache thrash
W_DEFAULT = 128                     # lama_hip_default_cfg().window_patches (asserted from the counters)


def dir_index(pidx):
    """DirCache::index (lama_kernels.h): the slot of the direct-mapped LDS cache that window patch pidx = wy * W + wx takes"""
    return (pidx ^ (pidx >> 9) ^ (pidx >> 5)) & 511


def window_origin(patches, r=1, W=W_DEFAULT):
    """where lama_hip_map_add_obstacles places the window of a fresh context: centred on the box of the listed cells' patches,
    widened by r patches (ensure_window, lama_hip.hip).  A COPY of the host's placement rule: nothing the device reports gives the
    window's origin, only window_patches and window_shifts are checked against it.  If that rule changes, the directory-cache
    cases below go on passing without their patches colliding -- re-derive this function and _box_origin then (a kernel whose
    fast paths take any non-empty cache word for a hit must fail them: DESIGN.md 2d, the two added mutants)."""
    xs, ys = [p[0] for p in patches], [p[1] for p in patches]
    return (min(xs) - r + max(xs) + r + 1) // 2 - W // 2, (min(ys) - r + max(ys) + r + 1) // 2 - W // 2


def pidx_of(patches, W=W_DEFAULT):
    ox, oy = window_origin(patches)
    return [(py - oy) * W + (px - ox) for px, py in patches]


def colliding_patches(n):
    """n patches, the first the one BASE lies in, whose directory entries share a cache slot and differ in their tags: by brute
    force over the patches up to 110 to the right and above (the box of all of them fits the window's 128)"""
    p0 = ((OFF + BASE[0]) >> 5, (OFF + BASE[1]) >> 5)
    cand = [(p0[0] + dx, p0[1] + dy) for dy in range(0, 110) for dx in range(0, 110) if max(dx, dy) >= 3]

    def ok(ps):
        idx = pidx_of(ps)
        far = all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 3 for i, a in enumerate(ps) for b in ps[:i])
        return far and len({dir_index(i) for i in idx}) == 1 and len({i >> 3 for i in idx}) == len(ps)
    for a in cand:
        if ok([p0, a]):
            if n == 2:
                return [p0, a]
            for b in cand:
                if b > a and ok([p0, a, b]):
                    return [p0, a, b]
    raise AssertionError(f"no {n} colliding patches")


def check_directory_cache_thrash(F, n):
    """one obstacle in the middle of each of n patches whose directory entries evict each other: the discs (reach 10 cells, inside
    their patches) are flooded level by level in turn, so a pop finds the other patch's entry in its slot -- not cached: the
    general pop"""
    ps = colliding_patches(n)
    idx = pidx_of(ps)
    assert len({dir_index(i) for i in idx}) == 1 and len({i >> 3 for i in idx}) == n, idx
    cells = [(px * 32 + 16 - OFF - BASE[0], py * 32 + 16 - OFF - BASE[1]) for px, py in ps]
    st, c, _ = dm_case(F, cells, 0.5, f"{n} colliding patches")
    assert c["window_patches"] == W_DEFAULT and st["lower_fired"] == n * DISC_10 and st["max_queue_last"] >= n * 30, (st, c)


def _box_origin(x0, x1, y0, y1, W=W_DEFAULT):
    return (x0 + x1 + 1) // 2 - W // 2, (y0 + y1 + 1) // 2 - W // 2


def check_directory_cache_thrash_on_removal(F, waves):
    """The same with removals: an armed obstacle in the middle of two colliding patches, one beam through both (its delta is a
    multiple of the patch offset, so it passes through both cell centres) to a solid cell beyond.  The two discs are raised level
    by level in turn.  An uploaded map's window is centred on the box of its distance-map patches (lama_hip_pf_upload_map,
    ensure_window); the second patch is searched with the box predicted and the collision asserted on the box the map really has."""
    p0 = ((OFF + BASE[0]) >> 5, (OFF + BASE[1]) >> 5)
    lo = (p0[0] - 6, p0[1] - 4)                                  # the first scan's obstacle, 5 x 3 patches from the base, and its disc

    def plan(dx, dy):
        j = -(-FAR // max(dx, dy))
        c0 = (16, 16)
        c1, end = (c0[0] + 32 * dx, c0[1] + 32 * dy), (c0[0] + (32 + j) * dx, c0[1] + (32 + j) * dy)
        hi = (p0[0] + (end[0] + 10) // 32, p0[1] + (end[1] + 10) // 32)
        return c0, c1, end, j, hi

    found = None
    for dy in range(0, 100):
        for dx in range(0, 100):
            if max(dx, dy) < 3 or found:
                continue
            c0, c1, end, j, hi = plan(dx, dy)
            ox, oy = _box_origin(lo[0], hi[0], lo[1], hi[1])
            if hi[0] - lo[0] >= W_DEFAULT - 2 or hi[1] - lo[1] >= W_DEFAULT - 2:
                continue
            i0, i1 = [(py - oy) * W_DEFAULT + (px - ox) for px, py in (p0, (p0[0] + dx, p0[1] + dy))]
            if dir_index(i0) == dir_index(i1) and (i0 >> 3) != (i1 >> 3):
                found = (dx, dy)
    assert found
    dx, dy = found
    c0, c1, end, j, hi = plan(dx, dy)
    run = EventRun(F, waves, what="colliding patches, removal")
    try:
        run.prepare(armed=[c0, c1], solids=[end])
        run.pf.dm(0).update()
        ids = list(run.pf.dm(0).dump())
        xs, ys = [i // STRIDE for i in ids], [i % STRIDE for i in ids]
        ox, oy = _box_origin(min(xs), max(xs), min(ys), max(ys))
        i0, i1 = [(py - oy) * W_DEFAULT + (px - ox) for px, py in (p0, (p0[0] + dx, p0[1] + dy))]
        assert dir_index(i0) == dir_index(i1) and (i0 >> 3) != (i1 >> 3), (found, i0, i1)
        st, _ = run.scan((c0[0] - dx, c0[1] - dy), [((33 + j) * dx, (33 + j) * dy)], [("remove", c0), ("remove", c1)])
        c = run.ctx.counters()
        assert c["window_patches"] == W_DEFAULT and c["window_shifts"] == 0, c
        assert st[0]["raise_pops"] == 2 * DISC_10 and st[0]["lower_fired"] == 0 and st[0]["max_queue_last"] >= 40, st
    finally:
        run.close()


# ------------------------------------------------------------------------------------------------ 6. size thresholds
def isolated(n, pitch=3):
    """n cells of a row, `pitch` apart"""
    return [(pitch * k, 0) for k in range(n)]


def check_additions_at_entry(F, sizes, limit):
    """n obstacles whose discs are the cells themselves (l2_max = 0.05 m: no pop pushes): the queue is largest when the brushfire
    starts.  n + 4 > limit hands the particle to the next stage before its first pop.  With limit = LQ both outcomes are
    asserted from brushfire_handovers.  With limit = LQ_BIG (the resume stage's queue, into k_brushfire_slow) there is no
    counter that tells a particle the resume stage finished from one the slow stage finished: the sizes lie on both sides of
    the threshold by construction (the oracle's queue length at entry), and what is checked on the device is the map alone."""
    for n in sizes:
        st, c, _ = dm_case(F, isolated(n, 2), 0.05, f"{n} additions")
        assert st["max_queue_last"] == n and st["lower_pops"] == n, st
        assert c["brushfire_handovers"] == (1 if n + 4 > LQ else 0), (n, c["brushfire_handovers"])
    assert {n + 4 > limit for n in sizes} == {False, True}                     # (of the sizes, not of anything the device reports)


def check_removals_at_entry(F, waves, sizes, limit, base=BASE):
    """the same for the raise queue (limit = RQ: both outcomes from brushfire_handovers; limit = RQ_BIG: the map alone, see above)"""
    for n in sizes:
        row = [(k, 0) for k in range(1, n + 1)]
        # (the beam ends two cells past the row: at this reach a cell next to the solid end would push it into the lower queue)
        st, dc, _ = run_events(F, waves, armed=row, solids=[(n + 2, 0)], sensor=(0, 0), deltas=[(n + 2, 0)], expect=[("remove", c) for c in row],
                               l2_max=0.05, what=f"{n} removals", base=base)
        assert st["raise_pops"] == n and st["max_queue_last"] == n and st["lower_pops"] == 0, st
        assert dc["brushfire_handovers"] == (1 if n + 4 > RQ else 0), (n, dc)
    assert {n + 4 > limit for n in sizes} == {False, True}                     # (of the sizes)


def wall(n):
    return [(k, 0) for k in range(n)]


# At l2_max = 0.25 m a wall of n collinear cells makes the lower queue 2 n + 22 entries long at its largest (asserted from the
# oracle's statistics where it is used): 1,274 .. 1,280 across the first stage's 1,276, 2,046 .. 2,050 across the 2,047 entries above
# which the resume stage's heap pop takes its third round.
WALL_SWEEP = (626, 627, 628, 629)
WALL_RESUME = (1012, 1013, 1014, 1500)      # ... and 3,022: a thousand pops of a heap that needs the third round


def check_wall_in_the_resume_stage(F, sizes=WALL_RESUME, l2_max=0.25):
    """walls that the first stage hands over in mid-lower and whose queue then grows and shrinks through 2,047 entries in the
    resume stage (lds_pop_flat's third round).  Which round a pop took is not observable: the queue lengths are the oracle's, the
    device is checked by the map and the pop count alone -- a heap popped with too few rounds comes out in another order.  The
    walls of 1012 .. 1014 put at most three entries on the heap's twelfth level; the wall of 1500 (3,022 entries) is the one that
    tells."""
    for n in sizes:
        st, c, _ = dm_case(F, wall(n), l2_max, f"wall of {n}")
        assert c["brushfire_handovers"] == 1 and st["max_queue_last"] == 2 * n + 22 and st["max_queue_last"] + 4 <= LQ_BIG, (st, c)
    assert min(sizes) * 2 + 22 <= 2047 < 3000 < 2 * max(sizes) + 22


def check_wall_hands_over_in_mid_lower(F, sizes, l2_max=0.25):
    """walls of n collinear cells: the lower queue grows while the wall floods.  The pair's first stage keeps the particle while the
    queue stays within its 1,280-entry lower window (LQ + RQ) less the four pushes of a pop: the oracle's largest queue decides."""
    out = {}
    for n in sizes:
        st, c, _ = dm_case(F, wall(n), l2_max, f"wall of {n}")
        assert n + 4 <= LQ and st["max_queue_last"] > n
        out[n] = (st["max_queue_last"], c["brushfire_handovers"])
        assert c["brushfire_handovers"] == (1 if st["max_queue_last"] > LQ + RQ - 4 else 0), out
    assert {h for _, h in out.values()} == {0, 1}, out
    return out


# Isolated obstacles through a scan: a long wall cannot be drawn by one sensor (the shallow beams to its far cells cross the near
# ones often enough to remove them again), a grid of points 12 cells apart can -- nearest first, so that a cell is hit before the
# beams to the points behind it cross it.  At l2_max = 0.25 m every point's front is 24 entries at its widest and all fronts grow
# in step: m points make the lower queue 24 m entries long (asserted from the oracle's statistics).
GRID = sorted(((12 * i + 5, 12 * j + 7) for i in range(-6, 7) for j in range(0, 10)), key=lambda c: (c[0] ** 2 + c[1] ** 2, c))
GRID_SWEEP = (52, 53, 54, 55)       # 1,248, 1,272 | 1,296, 1,320 entries: across the first stage's lower window


def check_grid_through_a_scan(F, waves, sizes=GRID_SWEEP, l2_max=0.25):
    """the hand-over in mid-lower in the form cfg.brushfire_waves names"""
    out = {}
    for m in sizes:
        cells = GRID[:m]
        st, dc, _ = run_events(F, waves, sensor=(0, 0), deltas=cells, expect=[("add", c) for c in cells], l2_max=l2_max, what=f"grid of {m}")
        assert st["max_queue_last"] == 24 * m and m + 4 <= LQ, st
        out[m] = (st["max_queue_last"], dc["brushfire_handovers"])
        assert dc["brushfire_handovers"] == (1 if st["max_queue_last"] > LQ + RQ - 4 else 0), (waves, out)
    assert {h for _, h in out.values()} == {0, 1}, out
    return out


# A wall of n armed cells removed by one beam along it: the raise queue holds n entries at the start and grows as the wall's band
# is raised, to 2 n + 11 entries (l2_max = 0.25 m, the solid end next to the wall); with one more armed cell 13 cells past the
# wall, raised beside it, to 2 n + 46.  Odd and even lengths across the 252 entries the first stage's raise queue takes in mid-run
# (nr + 4 > RQ after the pushes of a pop): 249, 251 | 253, 255 and 250, 252 | 254, 256.
RAISE_SWEEP = ((119, False), (120, False), (121, False), (122, False), (102, True), (103, True), (104, True), (105, True))
RAISE_GAP = 13


def check_raise_queue_outgrows_the_first_stage(F, waves, sizes=RAISE_SWEEP, l2_max=0.25):
    """the hand-over in mid-raise, both outcomes next to each other from brushfire_handovers (the lower queue stays far below its
    window)"""
    out = {}
    for n, extra in sizes:
        row = [(k, 0) for k in range(1, n + 1)] + ([(n + RAISE_GAP, 0)] if extra else [])
        end = (n + 2 * RAISE_GAP, 0) if extra else (n + 1, 0)
        st, dc, _ = run_events(F, waves, armed=row, solids=[end], sensor=(0, 0), deltas=[end], expect=[("remove", c) for c in row], l2_max=l2_max,
                               what=f"wall of {n} removed{' and a cell' if extra else ''}")
        assert len(row) + 4 <= RQ and st["max_queue_last"] == (2 * n + 46 if extra else 2 * n + 11) and st["lower_pops"] < 200, st
        out[(n, extra)] = (st["max_queue_last"], dc["brushfire_handovers"])
        assert dc["brushfire_handovers"] == (1 if st["max_queue_last"] + 4 > RQ else 0), (waves, out)
    assert {q: h for q, h in out.values() if 251 <= q <= 254} == {251: 0, 252: 0, 253: 1, 254: 1}, out
    return out


# ------------------------------------------------------------------------------------------------ 7. reach
def check_reach(F, l2_max, cells=((0, 0),), what=""):
    """obstacles at a reach of 127 cells (narrow library: the queue entries' 8-bit offsets run to both ends in x and y), 128 and
    255 (wide library) -- one obstacle, or two with a tie line between them"""
    r = math.ceil(l2_max * 20.0)
    assert F.needs_wide(l2_max, 0.05) == (r > 127)
    st, c, dm = dm_case(F, cells, l2_max, f"reach {r} {what}")
    dump = dm.dump()
    xs = max(int(np.abs(cl["obstacle"][:, :2].astype(np.int64)).max()) for cl, _ in dump.values())
    assert xs == r - 1, (xs, r, st)
    # (the front of one disc of 127 or 128 cells stays within the first stage's lower window, that of 255 cells does not)
    assert c["brushfire_handovers"] == (1 if st["max_queue_last"] > LQ + RQ - 4 else 0), (st, c)
    if len(cells) == 1:
        assert st["lower_fired"] == disc(r), st
    else:
        assert st["lower_pops"] > st["lower_fired"], st
    return st


def check_reach_removal(F, waves, l2_max=6.35):
    r = math.ceil(l2_max * 20.0)
    far = 2 * r + 8
    st, _, _ = run_events(F, waves, armed=[(0, 0)], solids=[(far, 0)], sensor=(-far, 0), deltas=[(2 * far, 0)], expect=[("remove", (0, 0))], l2_max=l2_max,
                           what=f"removal at reach {r}", base=(32 * 24, 32 * 24))
    assert st["raise_pops"] == disc(r) and st["lower_fired"] == 0, st


# ------------------------------------------------------------------------------------------------ 8. several particles in one launch
def check_five_particles(F, waves, route=False, l2_max=0.25):
    """five particles, one scan: (0) no event, (1) one addition, (2) a grid of 60 points that outgrows the first stage in mid-lower,
    (3) more removals than the first stage's raise queue takes: straight to the resume stage, (4) more than the resume stage's:
    finished by the slow stage.  The beam along y = 0 ends on a solid cell past the longest row; the other beams hit the grid."""
    n3, n4, m = RQ, RQ_BIG, 60
    end = (n4 + 2, 0)
    grid = GRID[:m]
    run = EventRun(F, waves, l2_max=l2_max, P=5, what="five particles")
    try:
        run.prepare(solids=[end])
        run.prepare(solids=grid, p=0)                                        # every hit cell is solid already
        run.prepare(solids=grid[:-1], p=1)                                   # ... but the last
        run.prepare(solids=grid, armed=[(k, 0) for k in range(1, n3 + 1)], p=3)
        run.prepare(solids=grid, armed=[(k, 0) for k in range(1, n4 + 1)], p=4)
        deltas = [end] + grid
        expect = [[], [("add", grid[-1])], [("add", c) for c in grid],
                  [("remove", (k, 0)) for k in range(1, n3 + 1)], [("remove", (k, 0)) for k in range(1, n4 + 1)]]
        st, dc = run.scan((0, 0), deltas, expect)
        assert st[0]["pops"] == 0 and 0 < st[1]["pops"] < 100, st
        assert st[2]["max_queue_last"] > LQ + RQ - 4 and m + 4 <= LQ, st[2]
        assert RQ_BIG >= st[3]["max_queue_last"] + 4 > RQ and st[4]["max_queue_last"] + 4 > RQ_BIG, (st[3], st[4])
        if route:
            assert dc["brushfire_routed"] >= 1, dc
        else:
            assert dc["brushfire_handovers"] == 3 and dc["brushfire_routed"] == 0, dc
    finally:
        run.close()


# ------------------------------------------------------------------------------------------------ the oracle itself
def check_oracle_against_the_reference():
    """the event sequences of the cases above -- additions, then removals and additions on the map they left -- through the
    oracle's and the compiled reference's DynamicDistanceMap: the maps bit-equal after every update()"""
    seqs = [([("add", c) for c in TIE_OBSTACLES], [("remove", (0, 0)), ("remove", (4, 0)), ("add", (1, 1))]),
            ([("add", (0, 0)), ("add", (0, 1))], [("remove", (0, 0))]),
            ([("add", c) for c in wall(40)], [("remove", c) for c in wall(40)[5:30]] + [("add", (7, 3))]),
            ([("add", (31, 31))], [("remove", (31, 31)), ("add", (31, 31))])]
    for l2_max in (0.25, 0.5):
        for first, second in seqs:
            o, r = O.DM.new(l2_max=l2_max), R.DM.new(0.05, l2_max=l2_max)
            for events in (first, second):
                for kind, (x, y) in events:
                    for m in (o, r):
                        (m.add if kind == "add" else m.remove)(OFF + BASE[0] + x, OFF + BASE[1] + y)
                assert o.update() == r.update()
                assert_maps_equal(o.dump(), r.dump(), DM_FIELDS, f"oracle against the reference, l2_max {l2_max}")
