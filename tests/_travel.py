"""The routes of lama_hip_map_travel restated in plain numpy / Python from the two dense grids of the box (tests/_raster.py gives
them from a map in the record format of HipContext.download_map): the classification with numpy, the field with a heapq Dijkstra over
exactly the move rules of include/lama_hip.h, then the goal's answer and the descent.  Test infrastructure: nothing here calls the
code under test."""
import heapq

import numpy as np

NONE = 0xFFFFFFFF
REACHED, UNREACHED, OUTSIDE = 0, 1, 2
ROUTE_T = np.dtype([("status", "<u4"), ("pixel", "<u4"), ("cost", "<u4"), ("steps", "<u4")])
# the eight neighbours (di, dj) in ascending pixel index
NEIGHBOURS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))


def classify(occ, sq, clearance_cells, prefer_cells):
    """occ: int8 trinary grid or None (a context without an occupancy map); sq: uint16 grid -> (traversable, near) bool grids"""
    sq = sq.astype(np.int64)
    trav = sq >= clearance_cells * clearance_cells
    if occ is not None:
        trav &= occ == 0
    return trav, sq < prefer_cells * prefer_cells


def legal(trav, pi, pj, qi, qj):
    """may a step from p enter q?  Both are in the box and neighbours."""
    if not trav[qj, qi]:
        return False
    if pi != qi and pj != qj:
        return bool(trav[pj, qi] and trav[qj, pi])                   # the two pixels that share an edge with p and with q
    return True


def field(trav, near, near_factor, sources):
    """sources: pixel (i, j) pairs -> F as Python integers in an object-free int64 grid, NONE where unreached"""
    h, w = trav.shape
    F = np.full((h, w), NONE, dtype=np.int64)
    heap = []
    for i, j in sources:
        F[j, i] = 0
        heap.append((0, int(i), int(j)))
    heapq.heapify(heap)
    while heap:
        d, i, j = heapq.heappop(heap)
        if d > F[j, i]:
            continue
        for di, dj in NEIGHBOURS:
            a, b = i + di, j + dj
            if not (0 <= a < w and 0 <= b < h) or not legal(trav, i, j, a, b):
                continue
            nd = d + (7 if di and dj else 5) * (near_factor if near[b, a] else 1)
            if nd < F[b, a]:
                F[b, a] = nd
                heapq.heappush(heap, (nd, a, b))
    assert F[F != NONE].max(initial=0) < NONE
    return F


def answer(F, goal, reach):
    """goal: pixel (i, j) or None (outside the box) -> (status, pixel, cost)"""
    if goal is None:
        return OUTSIDE, NONE, NONE
    h, w = F.shape
    i, j = goal
    best, at = NONE, NONE
    for b in range(max(j - reach, 0), min(j + reach, h - 1) + 1):
        for a in range(max(i - reach, 0), min(i + reach, w - 1) + 1):
            if F[b, a] < best:                                       # ascending index: `<` keeps the smallest among equals
                best, at = int(F[b, a]), b * w + a
    return (UNREACHED, NONE, NONE) if best == NONE else (REACHED, at, best)


def descend(F, trav, near, near_factor, pixel):
    """the pixels from the answer pixel down to a source"""
    h, w = F.shape
    p, out = int(pixel), [int(pixel)]
    while F[p // w, p % w] != 0:
        i, j = p % w, p // w
        m = near_factor if near[j, i] else 1
        for di, dj in NEIGHBOURS:
            a, b = i + di, j + dj
            if 0 <= a < w and 0 <= b < h and F[b, a] != NONE and legal(trav, a, b, i, j) and F[b, a] + (7 if di and dj else 5) * m == F[j, i]:
                p = b * w + a
                break
        else:
            raise AssertionError("the restatement's field has a pixel without a predecessor")
        out.append(p)
    return out


def expect(occ, sq, clearance_cells, prefer_cells, near_factor, sources, goals, reach, path_cap):
    """-> (F uint32 (h, w), routes ROUTE_T, paths (goals, path_cap) uint32 filled with NONE past what is written, or None)"""
    trav, near = classify(occ, sq, clearance_cells, prefer_cells)
    F = field(trav, near, near_factor, sources)
    routes = np.zeros(len(goals), dtype=ROUTE_T)
    paths = np.full((len(goals), path_cap), NONE, dtype=np.uint32) if path_cap else None
    for g, goal in enumerate(goals):
        status, pixel, cost = answer(F, goal, reach)
        steps = 0
        if status == REACHED:
            way = descend(F, trav, near, near_factor, pixel)[::-1]   # source first
            steps = len(way) - 1
            if path_cap:
                paths[g, :min(path_cap, len(way))] = way[:path_cap]
        routes[g] = (status, pixel, cost, steps)
    return F.astype(np.uint32), routes, paths


def largest_component_source(trav):
    """the traversable pixel (i, j) of smallest index in the largest 4-connected component of traversable pixels (the first such
    component among equals), and the component's size"""
    h, w = trav.shape
    seen = np.zeros((h, w), dtype=bool)
    best = (0, None)
    for j0, i0 in np.argwhere(trav).tolist():
        if seen[j0, i0]:
            continue
        seen[j0, i0] = True
        stack, n = [(i0, j0)], 0
        while stack:
            i, j = stack.pop()
            n += 1
            for a, b in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
                if 0 <= a < w and 0 <= b < h and trav[b, a] and not seen[b, a]:
                    seen[b, a] = True
                    stack.append((a, b))
        if n > best[0]:
            best = (n, (i0, j0))
    return best[1], best[0]
