"""Checks of the canonical brushfire (cfg.brushfire_mode = 1: k_brushfire_canon, lama_brushfire_canon.h) on the constructed obstacle
events of tests/_bf_checks.py.  Shared by tests/test_brushfire_canon_gpu.py and the lane-simulator tests
(tests/test_brushfire_canon_sim.py).

CanonRun is an EventRun with two oracle filters that are edited alike with the FAITHFUL update(); their maps are equal, bit for bit,
when they are uploaded.  Then the distance maps of one of them are switched to update_canonical(), and the one scan of the case goes
to the device and to both.  Every case asserts counters()["brushfire_mode"] == 1 and, as EventRun does, that the scan produced
exactly the listed add / remove events.  Three comparisons, all of integers, no tolerance anywhere:

(a) device against the canonical oracle, bit for bit (assert_maps_equal: DM_FIELDS, OCC_FIELDS, masks, patch sets);
(b) device against the faithful oracle: patch sets, masks, sqdist, valid, queued equal, and every cell whose obstacle offset differs
    is a tie -- both offsets point at live obstacles of the faithful map (valid, sqdist == 0) and both have the squared length that
    is the cell's sqdist.  This part does not lean on update_canonical().  Its precondition, that the two oracles agree outside the
    offsets, is asserted first; only the two cases with a dead obstacle may skip (b) when the oracles themselves disagree there
    (EXEMPTED names what did);
(c) addition-only cases: sqdist equals the brute-force truncated squared distance wherever that is below max_sqdist (edt(), pinned
    to _brute_edt of tests/test_oracle_kat.py on the small cases).

The regime a case names is asserted from the FAITHFUL oracle's statistics (update_canonical() keeps none).  A case in which the
kernel declines at entry (fall-through) is an EventRun with brushfire_mode = 1 against the faithful oracle alone, bit for bit, with
the exact kernels' own assertions (bf_cells == pops)."""
import numpy as np

import _bf_checks as BF
import _oracle as O
import _ray_checks as RC
from _bf_checks import FAR, STRIDE, _cell_of, row_beam, stats_delta
from _cmp import DM_FIELDS, OCC_FIELDS, assert_maps_equal, diff_maps
from _mapbuild import OFF
from test_oracle_kat import _brute_edt

CN_TBL = 4096                       # lama_brushfire_canon.h: entries of the LDS table
CN_HIST_MAX = 1024                  # ... the largest max_sqdist the kernel takes
QCAP_MIN = 8192                     # the smallest cfg.queue_capacity a context accepts (LQ_BIG)
EXEMPTED = {}                       # case -> the oracles' own diff, where (b) was skipped


def offer_passes(nf):
    """passes of stages B / C for a level of nf fired cells (four offers each, half the table a pass)"""
    return (4 * nf + CN_TBL // 2 - 1) // (CN_TBL // 2)


def select_passes(entries):
    """passes of stage A for a level of `entries` list entries"""
    return (entries + CN_TBL // 2 - 1) // (CN_TBL // 2)


# ------------------------------------------------------------------------------------------------ the comparisons
def live_obstacles(dump):
    out = set()
    for pid, (cells, _) in dump.items():
        for i in np.nonzero((cells["valid"] != 0) & (cells["sqdist"] == 0))[0]:
            out.add(((pid // STRIDE) * 32 + (int(i) & 31), (pid % STRIDE) * 32 + (int(i) >> 5)))
    return out


def assert_ties(dev, faithful, what):
    """every cell whose obstacle offset differs is equidistant from two live obstacles -> the number of such cells"""
    n = 0
    for pid in dev.keys() & faithful.keys():
        dc, fc = dev[pid][0], faithful[pid][0]
        for i in np.nonzero((dc["obstacle"] != fc["obstacle"]).any(axis=1))[0]:
            x, y = (pid // STRIDE) * 32 + (int(i) & 31), (pid % STRIDE) * 32 + (int(i) >> 5)
            assert fc["valid"][i], (what, x, y)
            for o in (dc["obstacle"][i], fc["obstacle"][i]):
                ox, oy = int(o[0]), int(o[1])
                t = _cell_of(faithful, x + ox, y + oy)
                assert int(o[2]) == 0 and ox * ox + oy * oy == int(fc["sqdist"][i]), (what, x, y, o, int(fc["sqdist"][i]))
                assert t is not None and t["valid"] and int(t["sqdist"]) == 0, (what, x, y, o)
            n += 1
    return n


def outside_offsets(a, b):
    d = diff_maps(a, b, DM_FIELDS)
    return {k: v for k, v in d.items() if k != "obstacle" and v}


def edt(dump, obstacles, max_sq):
    """the brute-force truncated squared distance over the box of the dump's patches, one pass per offset within reach
    -> (sqdist of the dump or -1 where a cell is absent / not valid, the brute-force distance, the box's origin)"""
    xs, ys = [p // STRIDE for p in dump], [p % STRIDE for p in dump]
    r = int(np.ceil(np.sqrt(max_sq)))
    x0, y0 = min(xs) * 32 - r, min(ys) * 32 - r
    W, H = (max(xs) + 1) * 32 + r - x0, (max(ys) + 1) * 32 + r - y0
    got = np.full((H, W), -1, dtype=np.int64)
    for pid, (cells, _) in dump.items():
        px, py = (pid // STRIDE) * 32 - x0, (pid % STRIDE) * 32 - y0
        got[py:py + 32, px:px + 32] = np.where(cells["valid"] != 0, cells["sqdist"].astype(np.int64), -1).reshape(32, 32)
    ob = np.zeros((H + 2 * r, W + 2 * r), dtype=bool)
    for x, y in obstacles:
        assert 0 <= x - x0 < W and 0 <= y - y0 < H, (x, y)
        ob[y - y0 + r, x - x0 + r] = True
    want = np.full((H, W), max_sq, dtype=np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            d2 = dx * dx + dy * dy
            if d2 < max_sq:
                np.minimum(want, np.where(ob[r + dy:r + dy + H, r + dx:r + dx + W], d2, max_sq), out=want)
    return got, want, (x0, y0)


def assert_edt(dump, obstacles, max_sq, what):
    assert live_obstacles(dump) == set(obstacles), (what, len(obstacles))
    got, want, (x0, y0) = edt(dump, obstacles, max_sq)
    near = want < max_sq
    bad = np.nonzero(near & (got != want))
    assert len(bad[0]) == 0, (what, len(bad[0]), [(int(x) + x0, int(y) + y0, int(got[y, x]), int(want[y, x])) for y, x in zip(bad[0][:6], bad[1][:6])])
    if len(obstacles) <= 70:         # (the pass-per-offset form above against the per-cell form of tests/test_oracle_kat.py)
        ys, xs = np.nonzero(near)
        cells = [(int(x) + x0, int(y) + y0) for y, x in zip(ys, xs)]
        truth = _brute_edt(obstacles, cells, max_sq)
        assert all(truth[c] == int(want[c[1] - y0, c[0] - x0]) for c in cells), what
    return int(near.sum())


# ------------------------------------------------------------------------------------------------ the runner
class CanonRun(BF.EventRun):
    def __init__(self, F, l2_max=0.5, P=1, base=BF.BASE, what="", **cfg):
        super().__init__(F, 2, l2_max=l2_max, P=P, base=base, what=what, brushfire_mode=1, **cfg)
        pose0 = RC.sensor(0, 0)
        self.canon = self.pf                      # (canonical from the upload on)
        self.faithful = O.PF(O.default_options(particles=P, seed=3, l2_max=l2_max))
        self.faithful.set_prior(pose0)
        assert self.faithful.update(RC.lattice(BF.FIRST_SCAN), pose0, 0.0)
        self.first = (OFF + BF.FIRST_SCAN[0][0], OFF + BF.FIRST_SCAN[0][1])

    def both(self, fn):
        """fn(dm, occ) on every particle of both filters (edits that EventRun.prepare does not know)"""
        for pf in (self.canon, self.faithful):
            for q in range(self.P):
                fn(pf.dm(q), pf.occ(q))

    def prepare(self, *a, **k):
        for pf in (self.canon, self.faithful):
            self.pf = pf
            super().prepare(*a, **k)
        self.pf = self.canon

    def upload(self):
        for q in range(self.P):
            self.faithful.dm(q).update()
        super().upload()
        for q in range(self.P):
            assert_maps_equal(self.canon.dm(q).dump(), self.faithful.dm(q).dump(), DM_FIELDS, f"{self.what}: the two oracles before the scan, dm p{q}")
            assert_maps_equal(self.canon.occ(q).dump(), self.faithful.occ(q).dump(), OCC_FIELDS, f"{self.what}: the two oracles before the scan, occ p{q}")
            self.canon.dm(q).set_canonical(True)

    def max_sqdist(self):
        return self.canon.dm(0).max_sqdist()

    def scan(self, sensor, deltas, expect, what="", may_exempt=False):
        """-> (the FAITHFUL oracle's stats delta per particle, the number of tie cells per particle; None where (b) was skipped)"""
        if not self.uploaded:
            self.upload()
        before = [self.faithful.dm(q).stats() for q in range(self.P)]
        super().scan(sensor, deltas, expect, what, exact=False)              # the events, then (a)
        c = self.ctx.counters()
        assert c["brushfire_mode"] == 1, c
        pose = RC.sensor(self.base[0] + sensor[0], self.base[1] + sensor[1])
        poses = np.stack([pose] * self.P)
        self.faithful.set_poses(poses); self.faithful.stage_set_scan(RC.lattice(deltas)); self.faithful.stage_update_maps()
        st = [stats_delta(self.faithful.dm(q).stats(), before[q]) for q in range(self.P)]
        ties = [self.compare_faithful(q, what, may_exempt) for q in range(self.P)]
        return st, ties

    def compare_faithful(self, q, what, may_exempt):
        F, tag = self.F, f"{self.what} {what} p{q}"
        fa, ca = self.faithful.dm(q).dump(), self.canon.dm(q).dump()
        pre = outside_offsets(ca, fa)
        if pre:                                  # the oracles themselves: the algorithm may leak a tie into a distance
            assert may_exempt, (tag, "the canonical and the faithful oracle differ outside the obstacle offsets", pre)
            EXEMPTED[tag] = pre
            return None
        dev = self.ctx.download_map(q, F.MAP_DISTANCE)
        assert not outside_offsets(dev, fa), (tag, "device against the faithful oracle", diff_maps(dev, fa, DM_FIELDS))
        assert_maps_equal(self.ctx.download_map(q, F.MAP_OCCUPANCY), self.faithful.occ(q).dump(), OCC_FIELDS, tag + ": occ against the faithful oracle")
        return assert_ties(dev, fa, tag)

    def assert_edt(self, adds, q=0, what=""):
        """(c) for particle q, whose obstacles are the first scan's and `adds`"""
        obstacles = {self.first} | {self.abs(c) for c in adds}
        return assert_edt(self.ctx.download_map(q, self.F.MAP_DISTANCE), obstacles, self.max_sqdist(), f"{self.what} {what} edt")


def run_canon(F, armed=(), solids=(), counts=None, sensor=(0, 0), deltas=(), expect=(), l2_max=0.5, what="", edt_adds=None, may_exempt=False,
              base=BF.BASE, **cfg):
    """-> (faithful stats delta, tie cells)"""
    run = CanonRun(F, l2_max=l2_max, what=what, base=base, **cfg)
    try:
        run.prepare(armed, solids, counts)
        st, ties = run.scan(sensor, list(deltas), list(expect), what, may_exempt=may_exempt)
        if edt_adds is not None:
            run.assert_edt(edt_adds)
        return st[0], ties[0]
    finally:
        run.close()


# ------------------------------------------------------------------------------------------------ 1. the per-branch cases of _bf_checks
def check_single_add(F):
    st, ties = run_canon(F, sensor=(-4, 0), deltas=[(4, 0)], expect=[("add", (0, 0))], what="single add", edt_adds=[(0, 0)])
    assert st["raise_pops"] == 0 and st["lower_fired"] == BF.DISC_10 and ties == 0, (st, ties)


def check_single_add_on_a_patch_corner(F):
    run = CanonRun(F, what="add on a patch corner")
    try:
        cx, cy = run.abs((31, 31))
        before = set(run.canon.dm(0).dump())
        around = {((cx + dx) >> 5) * STRIDE + ((cy + dy) >> 5) for dx in (0, 1) for dy in (0, 1)}
        assert len(around) == 4 and not (around & before) and (cx & 31, cy & 31) == (31, 31)
        st, _ = run.scan((31, 27), [(0, 4)], [("add", (31, 31))])
        assert around <= set(run.ctx.download_map(0, F.MAP_DISTANCE)) and st[0]["lower_fired"] == BF.DISC_10 and st[0]["raise_pops"] == 0, st
        run.assert_edt([(31, 31)])
    finally:
        run.close()


def check_single_removal(F):
    s, d, end = row_beam()
    st, _ = run_canon(F, armed=[(0, 0)], solids=[end], sensor=s, deltas=[d], expect=[("remove", (0, 0))], what="single removal")
    assert st["raise_pops"] == BF.DISC_10 and st["lower_pops"] == 0, st


def check_single_removal_on_a_patch_corner(F):
    """(31, 31) added AND removed in this update: the raise round allocates the neighbour's patch across the edge"""
    run = CanonRun(F, what="removal on a patch corner")
    try:
        run.prepare(solids=[(31, 31 + FAR)], counts={(31, 31): (0, 2)})
        cx, cy = run.abs((31, 31))
        own, right = (cx >> 5) * STRIDE + (cy >> 5), ((cx + 1) >> 5) * STRIDE + (cy >> 5)
        run.both(lambda dm, occ: dm.update())
        have = set(run.canon.dm(0).dump())
        assert own not in have and right not in have
        up = (0, 2 * FAR)
        st, _ = run.scan((31, 31 - FAR), [(0, FAR), up, up], [("add", (31, 31)), ("remove", (31, 31))])
        have = set(run.ctx.download_map(0, F.MAP_DISTANCE))
        assert st[0]["raise_pops"] == 1 and st[0]["lower_pops"] == 1 and own in have and right in have, st
    finally:
        run.close()


def check_one_of_two_removed(F, which):
    s, d, end = row_beam()
    st, _ = run_canon(F, armed=[(0, 0)], solids=[end, BF.PAIR_OFFSETS[which]], sensor=s, deltas=[d], expect=[("remove", (0, 0))], what=f"pair at {which}")
    assert st["raise_pops"] >= 100 and st["lower_fired"] >= 50, st


def check_both_removed(F):
    s, d, end = row_beam()
    st, _ = run_canon(F, armed=[(0, 0), (3, 0)], solids=[end], sensor=s, deltas=[d], expect=[("remove", (0, 0)), ("remove", (3, 0))], what="both removed")
    assert st["raise_pops"] > BF.DISC_10 and st["lower_fired"] == 0, st


def check_removal_and_addition_in_one_update(F):
    s, d, end = row_beam()
    st, _ = run_canon(F, armed=[(0, 0)], solids=[end, (0, 5)], sensor=s, deltas=[(FAR + 4, 3), d],
                      expect=[("add", (4, 3)), ("remove", (0, 0))], what="removal and addition")
    assert st["raise_pops"] >= 100 and st["lower_fired"] >= 100, st


def check_removed_then_added_again(F):
    s, d, end = row_beam()
    st, _ = run_canon(F, armed=[(0, 0)], solids=[end, (6, 2)], sensor=s, deltas=[d, (FAR, 0)],
                      expect=[("remove", (0, 0)), ("add", (0, 0))], what="removed, added again")
    assert st["raise_pops"] == 1 and st["lower_pops"] == 5 and st["lower_fired"] == 4, st


def check_added_then_removed(F):
    s, d, end = row_beam()
    st, _ = run_canon(F, solids=[end, (6, 2)], counts={(0, 0): (0, 2)}, sensor=s, deltas=[(FAR, 0), d, d],
                      expect=[("add", (0, 0)), ("remove", (0, 0))], what="added, removed")
    assert st["raise_pops"] >= 1 and st["lower_pops"] >= 1, st


def check_ties_on_addition(F):
    deltas = [(x + FAR, y + 7) for x, y in BF.TIE_OBSTACLES]
    st, ties = run_canon(F, sensor=(-FAR, -7), deltas=deltas, expect=[("add", c) for c in BF.TIE_OBSTACLES], what="ties, added", edt_adds=BF.TIE_OBSTACLES)
    assert st["lower_pops"] > st["lower_fired"] > BF.DISC_10, st
    return ties


def check_ties_on_removal(F, which):
    s, d, end = row_beam()
    solids = [c for c in BF.TIE_OBSTACLES if c[1] != 0]
    armed = [c for c in BF.TIE_OBSTACLES if c[1] == 0][:which]
    st, ties = run_canon(F, armed=armed, solids=solids + [end], sensor=s, deltas=[d], expect=[("remove", c) for c in sorted(armed)], what=f"ties, {which} removed")
    assert st["raise_pops"] >= 30 and st["lower_fired"] >= 30, st
    return ties


def check_tie_with_a_dead_obstacle(F):
    run = CanonRun(F, what="tie with a dead obstacle")
    try:
        run.prepare(solids=[(4, 10 + FAR)])
        for k, c in enumerate(BF.DEAD_TIE):
            run.prepare(armed=[c]) if k == 1 else run.prepare(solids=[c])
            run.both(lambda dm, occ: dm.update())
        st, _ = run.scan((4, 10 - FAR), [(0, 2 * FAR)], [("remove", BF.DEAD_TIE[1])], may_exempt=True)
        assert st[0]["tie_overwrites"] >= 1 and 0 < st[0]["raise_pops"] < BF.DISC_10 and st[0]["lower_fired"] > 0, st
    finally:
        run.close()


def check_tie_with_a_dead_obstacle_among_other_events(F, case=BF.HISTORY_TIE):
    """check_history_case of _bf_checks on both filters"""
    run = CanonRun(F, what="tie with a dead obstacle, mixed events")
    try:
        live = []
        for events in case["history"]:
            for kind, c in events:
                run.both(lambda dm, occ: (dm.add if kind == "add" else dm.remove)(*run.abs(c)))
                live.append(c) if kind == "add" else live.remove(c)
            run.both(lambda dm, occ: dm.update())
        hs = BF.H_SENSOR
        ends = [(2 * x - hs[0], 2 * y - hs[1]) for x, y in case["armed"]]
        for c in live:
            run.both(lambda dm, occ: BF.set_counts(occ, run.abs(c), *((1, 4) if c in case["armed"] else (8, 8))))
        run.prepare(solids=[e for e in ends if e not in live])
        deltas = [(ex - hs[0], ey - hs[1]) for ex, ey in ends] + [(x - hs[0], y - hs[1]) for x, y in case["adds"]]
        expect = [("remove", c) for c in case["armed"]] + [("add", c) for c in case["adds"]]
        st, _ = run.scan(hs, deltas, expect, may_exempt=True)
        assert st[0]["tie_overwrites"] >= 1 and st[0]["raise_pops"] > 0 and st[0]["lower_pops"] > st[0]["lower_fired"] > 0, st
    finally:
        run.close()


# ------------------------------------------------------------------------------------------------ 2. adds only, across the thread and wave edges
ADDS_ONLY = (1, 63, 64, 65, 255, 256, 257, 600)


def check_adds_only(F, n, l2_max=0.25):
    """isolated(n) added by one scan: the scan removes nothing, so the raise loop and its barriers are skipped and the level loop
    follows the entry barrier at once.  List indices of 64 and above belong to waves 1 .. 3, of 256 and above to a thread's second
    trip.  The sensor stands n / 2 + 40 cells below the middle of the row: a beam touches the row in at most three cells, its own
    and two beside it, and the points are three apart."""
    cells = sorted(BF.isolated(n), key=lambda c: (abs(2 * c[0] - 3 * (n - 1)), c))           # nearest first
    sx, sy = (3 * (n - 1)) // 2, -(n // 2 + 40)
    st, ties = run_canon(F, sensor=(sx, sy), deltas=[(x - sx, y - sy) for x, y in cells], expect=[("add", c) for c in cells], l2_max=l2_max,
                         what=f"{n} adds only", edt_adds=cells)
    assert st["raise_pops"] == 0 and st["lower_fired"] >= n, st
    return ties


# ------------------------------------------------------------------------------------------------ 3. multi-pass levels
# The GRID of _bf_checks holds 130 points, and a larger one around the sensor cannot be drawn: a point 9 cells away lies under the beams
# to dozens of points behind it and is removed again (four free visits after its hit).  Points at 60 cells and more from the sensor,
# all around it, nearest first and without the diagonal x = -y, whose points lie on one beam: no point's cell is crossed more than three
# times (EventRun asserts the events).
BIG_GRID = sorted(((12 * i + 5, 12 * j + 7) for i in range(-30, 30) for j in range(-30, 30) if (12 * i + 5) ** 2 + (12 * j + 7) ** 2 >= 60 * 60 and i + j != -1),
                  key=lambda c: (c[0] ** 2 + c[1] ** 2, c))
BIG_BASE = (32 * 24, 32 * 24)       # three hundred cells and more from the first scan's obstacle
# The kernel's pending list is append-only: cfg.queue_capacity bounds the cells ONE update lowers (1025 discs of 69 cells: 70,725), not, as
# for the exact kernels, the front at its widest.  Beyond it the update ends with LAMA_HIP_E_CAPACITY, as include/lama_hip.h says.
BIG_QCAP = 1 << 17
MULTI_PASS = (511, 512, 513, 1025)
assert [offer_passes(n) for n in MULTI_PASS] == [1, 1, 2, 3] and len(BIG_GRID) >= max(MULTI_PASS)
# (isolated points at a reach of 5 cells: 4 cells a point at level 1, 8 at level 5 -- a level of 1025 points holds 8,200 distinct cells,
# twice the table: stage A's passes)
assert [select_passes(8 * n) for n in MULTI_PASS] == [2, 2, 3, 5]


def check_grid_in_passes(F, m, l2_max=0.25):
    """m isolated points drawn by one scan, as check_grid_through_a_scan: all of them fire at level 0, in offer_passes(m) passes"""
    cells = BIG_GRID[:m]
    st, ties = run_canon(F, sensor=(0, 0), deltas=cells, expect=[("add", c) for c in cells], l2_max=l2_max, what=f"grid of {m}", edt_adds=cells,
                         base=BIG_BASE, dm_patch_capacity=512, occ_patch_capacity=512, queue_capacity=BIG_QCAP)
    assert st["max_queue_last"] == 24 * m and st["lower_fired"] == m * BF.disc(5) and ties == 0, (st, ties)


# ------------------------------------------------------------------------------------------------ 4. a level with more cells than the table
RING = 525


def ring(h=RING):
    """the 8 h cells on the border of the square of half-side h around the sensor: a beam crosses inner cells only"""
    return [(x, -h) for x in range(-h, h)] + [(h, y) for y in range(-h, h)] + [(x, h) for x in range(h, -h, -1)] + [(-h, y) for y in range(h, -h, -1)]


def check_more_new_obstacles_than_the_table(F, h=RING, l2_max=0.25, **cfg):
    """8 h > CN_TBL new obstacle cells in one scan: level 0 holds more distinct cells than the table"""
    cells = ring(h)
    assert len(set(cells)) == 8 * h > CN_TBL
    run = CanonRun(F, l2_max=l2_max, what=f"ring of {8 * h}", base=BIG_BASE, dm_patch_capacity=512, occ_patch_capacity=2048, queue_capacity=BIG_QCAP, **cfg)
    try:
        st, ties = run.scan((0, 0), cells, [("add", c) for c in cells])
        assert st[0]["raise_pops"] == 0 and st[0]["lower_fired"] > 8 * h, st
        run.assert_edt(cells)
    finally:
        run.close()


# ------------------------------------------------------------------------------------------------ 5. fall-through to the exact stages
TIED_PAIR = [(0, 0), (6, 2)]


def _tied_pair_oracles_differ(l2_max):
    """the two oracles on the tied pair: they differ (in offsets), so a device map tells which algorithm made it"""
    a, b = O.DM.new(l2_max=l2_max), O.DM.new(l2_max=l2_max)
    b.set_canonical(True)
    for m in (a, b):
        for x, y in TIED_PAIR:
            m.add(OFF + BF.BASE[0] + x, OFF + BF.BASE[1] + y)
        m.update()
    d = diff_maps(a.dump(), b.dump(), DM_FIELDS)
    assert d["obstacle"] > 0, d
    return a.max_sqdist()


PAIR_SCAN = dict(sensor=(3, -20), deltas=[(-3, 20), (3, 22)], expect=[("add", (0, 0)), ("add", (6, 2))])


def check_reach_of_32_cells_runs_canonical(F, l2_max=1.58):
    assert _tied_pair_oracles_differ(l2_max) == CN_HIST_MAX == 32 * 32
    st, ties = run_canon(F, l2_max=l2_max, what="reach 32", edt_adds=TIED_PAIR, **PAIR_SCAN)
    assert ties > 0, ties          # (equal to the canonical oracle and, in these cells, not to the faithful one)


def run_declined(F, what, l2_max, armed=(), solids=(), sensor=(0, 0), deltas=(), expect=(), base=BF.BASE, **cfg):
    """mode 1 asked for, the canonical kernel declines at entry: the FAITHFUL oracle, bit for bit, and the exact kernels' pop count"""
    run = BF.EventRun(F, 2, l2_max=l2_max, what=what, base=base, brushfire_mode=1, **cfg)
    try:
        run.prepare(armed, solids)
        st, dc = run.scan(sensor, list(deltas), list(expect), what)
        c = run.ctx.counters()
        assert c["brushfire_mode"] == 1, c
        return st[0], run.pf.dm(0).max_sqdist()
    finally:
        run.close()


def check_reach_of_33_cells_falls_through(F, l2_max=1.63):
    assert _tied_pair_oracles_differ(l2_max) == 33 * 33 == 1089 > CN_HIST_MAX
    st, msq = run_declined(F, "reach 33", l2_max, **PAIR_SCAN)
    assert msq == 1089 and st["lower_pops"] > st["lower_fired"] > BF.disc(33), st


def check_wide_library_falls_through(F, l2_max=7.0):
    assert F.needs_wide(l2_max, 0.05)
    _tied_pair_oracles_differ(l2_max)
    st, msq = run_declined(F, "wide library", l2_max, base=(32 * 24, 32 * 24), **PAIR_SCAN)
    assert msq == 140 * 140 and st["lower_pops"] > st["lower_fired"] > BF.disc(140), st


def check_more_raise_entries_than_half_the_queue(F, l2_max=0.05):
    """queue_capacity 8192, the smallest a context takes: 4097 armed cells on two rows, removed by one scan of two beams"""
    n = QCAP_MIN // 2 + 1
    nx, ny = n // 2 + 1, n - (n // 2 + 1)
    armed = [(k, 0) for k in range(1, nx + 1)] + [(0, k) for k in range(1, ny + 1)]
    ends = [(nx + 2, 0), (0, ny + 2)]
    assert len(armed) == n > QCAP_MIN // 2
    st, _ = run_declined(F, f"{n} removals", l2_max, armed=armed, solids=ends, sensor=(0, 0), deltas=ends, expect=[("remove", c) for c in armed],
                         base=(32 * 8, 32 * 8), queue_capacity=QCAP_MIN, dm_patch_capacity=512, occ_patch_capacity=512)
    assert st["raise_pops"] == n and st["max_queue_last"] == n, st


def check_more_lower_entries_than_half_the_queue(F, h=RING, l2_max=0.05):
    """the 4200 new cells of the ring at queue_capacity 8192: the fired cells of level 0 would not fit half the queue.  (A reach of one
    cell: no pop pushes, so the exact kernels' queue, 4200 entries at entry, fits.)"""
    cells = ring(h)
    assert QCAP_MIN >= len(cells) > QCAP_MIN // 2
    st, _ = run_declined(F, f"ring of {len(cells)}, small queue", l2_max, sensor=(0, 0), deltas=cells, expect=[("add", c) for c in cells], base=BIG_BASE,
                         queue_capacity=QCAP_MIN, dm_patch_capacity=512, occ_patch_capacity=2048)
    assert st["raise_pops"] == 0 and st["lower_pops"] == len(cells) == st["max_queue_last"], st


# ------------------------------------------------------------------------------------------------ 6. five particles in one launch
def check_five_particles(F, l2_max=0.25):
    """check_five_particles of _bf_checks: no event, one addition, a grid of 60 points, 256 removals, 2048 removals -- all five in the
    one launch of k_brushfire_canon"""
    n3, n4, m = BF.RQ, BF.RQ_BIG, 60
    end = (n4 + 2, 0)
    grid = BF.GRID[:m]
    run = CanonRun(F, l2_max=l2_max, P=5, what="five particles")
    try:
        run.prepare(solids=[end])
        run.prepare(solids=grid, p=0)
        run.prepare(solids=grid[:-1], p=1)
        run.prepare(solids=grid, armed=[(k, 0) for k in range(1, n3 + 1)], p=3)
        run.prepare(solids=grid, armed=[(k, 0) for k in range(1, n4 + 1)], p=4)
        expect = [[], [("add", grid[-1])], [("add", c) for c in grid],
                  [("remove", (k, 0)) for k in range(1, n3 + 1)], [("remove", (k, 0)) for k in range(1, n4 + 1)]]
        st, ties = run.scan((0, 0), [end] + grid, expect)
        assert st[0]["pops"] == 0 and 0 < st[1]["pops"] < 100 and st[2]["lower_fired"] == m * BF.disc(5), st
        assert st[3]["raise_pops"] >= n3 and st[4]["raise_pops"] >= n4, (st[3], st[4])
        run.assert_edt([end] + grid, q=2)
    finally:
        run.close()
