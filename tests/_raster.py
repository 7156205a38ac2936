"""The dense grids of lama_hip_map_rasterize / lama_hip_map_bounds restated in numpy from a map in the record format of
HipContext.download_map ({reference patch id: (cells[1024], mask[16])}, whose bytes the suite pins to the reference elsewhere).
The cell rules are the reference's as include/lama/sdm_maps.h restates them: the frequency rule in DOUBLE (:187-194), the log-odds
rule (:208-210), the distance rule (:319-324), each behind Map::get (a cell of an absent patch or with its mask bit off does not
exist); Map::bounds from the patch ids (src/sdm/map.cpp:139-157).  Test infrastructure: nothing here calls the code under test."""
import numpy as np

UC = 2642244                       # Map's UNIVERSAL_CONSTANT: patch id = (x >> 5) * UC + (y >> 5)
TRINARY, PROBABILITY, SQDIST = 0, 1, 2


def patch_id(px, py):
    return int(px) * UC + int(py)


def mask_bits(mask):
    ci = np.arange(1024)
    return ((np.asarray(mask, dtype=np.uint64)[ci >> 6] >> (ci & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def bounds(ids):
    """Map::bounds: (min (2,), max (2,)) in cells as uint32; no patches: min = 0xFFFFFFFF, max = 0 + 32."""
    if len(ids) == 0:
        return np.array([0xFFFFFFFF] * 2, dtype=np.uint32), np.array([32, 32], dtype=np.uint32)
    ids = np.array(sorted(ids), dtype=np.uint64)
    ax, ay = (ids // np.uint64(UC)) * np.uint64(32), (ids % np.uint64(UC)) * np.uint64(32)
    return (np.array([ax.min(), ay.min()], dtype=np.uint32), np.array([ax.max() + np.uint64(32), ay.max() + np.uint64(32)], dtype=np.uint32))


def _freq_trinary(cells, present):
    o, v = cells["occupied"].astype(np.float64), cells["visited"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        prob = np.where(cells["visited"] == 0, 0.25, o / v)          # FrequencyOccupancyMap::prob, in double
    out = np.full(cells.shape, -1, dtype=np.int8)
    out[present & (prob > 0.25)] = 100                                # isFree first, else isOccupied, else unknown (they exclude each other)
    out[present & (prob < 0.25)] = 0
    return out


def _freq_probability(cells, present):
    o, v = cells["occupied"].astype(np.int64), cells["visited"].astype(np.int64)
    q = np.minimum((200 * o + v) // np.maximum(2 * v, 1), 100)
    return np.where(present & (v != 0), q, -1).astype(np.int8)


def _logodds_trinary(cells, present):
    l = np.ascontiguousarray(cells).view(np.float32).reshape(cells.shape)
    out = np.full(cells.shape, -1, dtype=np.int8)
    out[present & (l > np.float32(0.0))] = 100
    out[present & (l < np.float32(0.0))] = 0
    return out


def _sqdist(cells, present, max_sqdist):
    return np.where(present & (cells["valid"] != 0), cells["sqdist"], max_sqdist).astype(np.uint16)


def cell_values(dump, layer, policy=0, max_sqdist=None):
    """{patch id: values[32, 32] (row = y)} of every patch of the dump"""
    out = {}
    for pid, (cells, mask) in dump.items():
        present = mask_bits(mask)
        if layer == SQDIST:
            v = _sqdist(cells, present, max_sqdist)
        elif layer == PROBABILITY:
            v = _freq_probability(cells, present)
        else:
            v = _logodds_trinary(cells, present) if policy else _freq_trinary(cells, present)
        out[pid] = v.reshape(32, 32)
    return out


def raster(dump, layer, x0, y0, width, height, stride=1, policy=0, max_sqdist=None):
    """The expected grid (height, width): per-cell values over the box's cells, absent cells unknown / max_sqdist, then the block
    rule: a signed maximum for the int8 layers (occupied 100 > free 0 > unknown -1; the largest probability, -1 if none), the
    minimum for the squared distance."""
    fill = max_sqdist if layer == SQDIST else -1
    dt = np.uint16 if layer == SQDIST else np.int8
    W, H = width * stride, height * stride
    full = np.full((H, W), fill, dtype=dt)
    for pid, v in cell_values(dump, layer, policy, max_sqdist).items():
        ax, ay = (pid // UC) * 32 - int(x0), (pid % UC) * 32 - int(y0)       # the patch's anchor relative to the box
        cx0, cx1, cy0, cy1 = max(ax, 0), min(ax + 32, W), max(ay, 0), min(ay + 32, H)
        if cx0 < cx1 and cy0 < cy1:
            full[cy0:cy1, cx0:cx1] = v[cy0 - ay:cy1 - ay, cx0 - ax:cx1 - ax]
    blocks = full.reshape(height, stride, width, stride)
    return blocks.min(axis=(1, 3)) if layer == SQDIST else blocks.max(axis=(1, 3))
