"""The frontier clusters of lama_hip_map_frontiers restated in plain numpy / Python from a map in the record format of
HipContext.download_map: _raster.raster() of the box widened by one pixel per side, the 4-neighbour rule, a breadth-first 8-connected
labelling in raster order, sums and boxes in Python integers.  Test infrastructure: nothing here calls the code under test."""
from collections import deque

import numpy as np

import _raster as RS

NONE = 0xFFFFFFFF
ABSENT = 1                          # a halo pixel that does not exist (below cell 0 or above cell 2^32 - 1): neither free nor unknown
FRONTIER_T = np.dtype([("label", "<u4"), ("pixels", "<u4"), ("min_i", "<u4"), ("min_j", "<u4"), ("max_i", "<u4"), ("max_j", "<u4"),
                       ("sum_i", "<u8"), ("sum_j", "<u8")])


def widened(dump, x0, y0, width, height, stride=1, policy=0):
    """(height + 2, width + 2) int8: the trinary raster of the box and its halo, ABSENT where a halo pixel does not exist"""
    ox, oy = (1 if x0 >= stride else 0), (1 if y0 >= stride else 0)
    ex, ey = (1 if x0 + width * stride <= 0xFFFFFFFF else 0), (1 if y0 + height * stride <= 0xFFFFFFFF else 0)
    g = np.full((height + 2, width + 2), ABSENT, dtype=np.int8)
    r = RS.raster(dump, RS.TRINARY, x0 - ox * stride, y0 - oy * stride, width + ox + ex, height + oy + ey, stride, policy)
    g[1 - oy:height + 1 + ey, 1 - ox:width + 1 + ex] = r
    return g


def frontier_mask(g):
    """g: the widened grid -> bool (height, width): free with an unknown EDGE neighbour"""
    c = g[1:-1, 1:-1]
    unknown = (g[1:-1, :-2] == -1) | (g[1:-1, 2:] == -1) | (g[:-2, 1:-1] == -1) | (g[2:, 1:-1] == -1)
    return (c == 0) & unknown


def clusters(mask, min_pixels=1):
    """-> (records sorted by pixels descending then label ascending, with pixels >= max(min_pixels, 1); labels (height, width) uint32;
    the number of frontier pixels).  8-connected components by a breadth-first search started in raster order: the start pixel is the
    component's smallest index."""
    h, w = mask.shape
    labels = np.full((h, w), NONE, dtype=np.uint32)
    recs = []
    for j0, i0 in np.argwhere(mask).tolist():
        if labels[j0, i0] != NONE:
            continue
        label = j0 * w + i0
        labels[j0, i0] = label
        queue, cells = deque([(i0, j0)]), []
        while queue:
            i, j = queue.popleft()
            cells.append((i, j))
            for dj in (-1, 0, 1):
                for di in (-1, 0, 1):
                    a, b = i + di, j + dj
                    if 0 <= a < w and 0 <= b < h and mask[b, a] and labels[b, a] == NONE:
                        labels[b, a] = label
                        queue.append((a, b))
        assert min(b * w + a for a, b in cells) == label
        recs.append((label, len(cells), min(a for a, _ in cells), min(b for _, b in cells), max(a for a, _ in cells), max(b for _, b in cells),
                     sum(a for a, _ in cells), sum(b for _, b in cells)))
    recs = sorted((r for r in recs if r[1] >= max(int(min_pixels), 1)), key=lambda r: (-r[1], r[0]))
    return np.array(recs, dtype=FRONTIER_T), labels, int(mask.sum())


def expect(dump, x0, y0, width, height, stride=1, policy=0, min_pixels=1):
    return clusters(frontier_mask(widened(dump, x0, y0, width, height, stride, policy)), min_pixels)


def expect_of_grid(grid, min_pixels=1):
    """the same on a dense trinary grid whose surroundings are all unknown (a whole-map box: outside Map::bounds every patch is absent)"""
    g = np.full((grid.shape[0] + 2, grid.shape[1] + 2), -1, dtype=np.int8)
    g[1:-1, 1:-1] = grid
    return clusters(frontier_mask(g), min_pixels)
