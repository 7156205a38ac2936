"""ctypes bindings of include/lama_hip.h and include/lama_host.h."""
import ctypes as C
import math
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB = os.path.join(_HERE, "lib", "liblama_hip.so")
HIP_LIB_WIDE = os.path.join(_HERE, "lib", "liblama_hip_wide.so")
HOST_LIB = os.path.join(_HERE, "lib", "liblama_host.so")
_PRODUCT_HOST_LIB = HOST_LIB

MAP_DISTANCE, MAP_OCCUPANCY = 0, 1

# the reference's record formats (what lama_hip_pf_download_map returns)
DIST_T = np.dtype([("obstacle", "<i2", (3,)), ("sqdist", "<u2"), ("valid", "u1"), ("queued", "u1")])
FREQ_T = np.dtype([("occupied", "<u2"), ("visited", "<u2")])


class LamaError(RuntimeError):
    pass


class HipCfg(C.Structure):
    _fields_ = [("particles", C.c_uint32), ("resolution", C.c_double), ("patch_size", C.c_uint32),
                ("l2_max", C.c_double), ("meas_sigma", C.c_double), ("max_iter", C.c_uint32),
                ("truncated_ray", C.c_double), ("truncated_range", C.c_double), ("device", C.c_int32),
                ("window_patches", C.c_uint32), ("dm_patch_capacity", C.c_uint32),
                ("occ_patch_capacity", C.c_uint32), ("queue_capacity", C.c_uint32), ("profile", C.c_uint32),
                ("active_capacity", C.c_uint32), ("sequential_raycast", C.c_uint32), ("brushfire_mode", C.c_uint32),
                ("brushfire_waves", C.c_uint32), ("occupancy_policy", C.c_uint32), ("ray_rule", C.c_uint32),
                ("solver_strategy", C.c_uint32)]


class HipCounters(C.Structure):
    _fields_ = [("ms_scan_match", C.c_double), ("launches_scan_match", C.c_uint64),
                ("ms_update_maps", C.c_double), ("launches_update_maps", C.c_uint64),
                ("ms_raycast", C.c_double), ("launches_raycast", C.c_uint64),
                ("ms_brushfire", C.c_double), ("launches_brushfire", C.c_uint64),
                ("ms_resample", C.c_double), ("launches_resample", C.c_uint64),
                ("gn_iterations", C.c_uint64), ("gn_evals", C.c_uint64), ("ray_cells", C.c_uint64),
                ("bf_cells", C.c_uint64), ("dm_patches", C.c_uint64), ("occ_patches", C.c_uint64),
                ("ms_eval_batch", C.c_double), ("launches_eval_batch", C.c_uint64), ("arena_growths", C.c_uint64), ("window_shifts", C.c_uint64), ("wrap_guard_scans", C.c_uint64),
                ("brushfire_mode", C.c_uint32), ("brushfire_waves", C.c_uint32),
                ("sequential_raycast_scans", C.c_uint64), ("parallel_raycast_scans", C.c_uint64),
                ("brushfire_handovers", C.c_uint32), ("replay_handovers", C.c_uint32),
                ("window_patches", C.c_uint32), ("window_growths", C.c_uint32),
                ("bf_longest_chain_sum", C.c_uint64), ("bf_longest_chain_last", C.c_uint64), ("brushfire_early", C.c_uint64), ("brushfire_routed", C.c_uint64),
                ("pool_growths", C.c_uint64), ("resample_clones", C.c_uint64), ("resample_bytes", C.c_uint64),
                ("hbm_bytes_allocated", C.c_uint64), ("hbm_bytes_used", C.c_uint64), ("hbm_bytes_total", C.c_uint64),
                ("peer_access", C.c_uint32), ("struct_bytes", C.c_uint32), ("peer_copy_ms", C.c_double), ("peer_copy_bytes", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def _hip_signatures():
    vp, i32, u32, u64, d = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_double
    required = {
        "lama_hip_default_cfg": [vp], "lama_hip_device_count": [vp], "lama_hip_ctx_create": [vp, vp], "lama_hip_ctx_destroy": [vp],
        "lama_hip_last_error": [vp], "lama_hip_pf_init": [vp, vp, u32, vp, vp, vp], "lama_hip_pf_set_poses": [vp, vp],
        "lama_hip_pf_get_poses": [vp, vp], "lama_hip_pf_scan_match": [vp, vp, u32, vp, vp, vp, vp, vp], "lama_hip_pf_resample": [vp, vp],
        "lama_hip_pf_update_maps": [vp, vp, u32, vp, vp], "lama_hip_pf_update_maps_begin": [vp, vp, u32, vp, vp], "lama_hip_sync": [vp],
        "lama_hip_ctx_device": [vp], "lama_hip_pf_map_patches": [vp, u32, i32, vp],
        "lama_hip_pf_download_map": [vp, u32, i32, u32, vp, vp, vp, vp], "lama_hip_pf_upload_map": [vp, u32, i32, u32, vp, vp, vp],
        "lama_hip_match_batch": [vp, u32, vp, u32, vp, vp, vp, u32, vp], "lama_hip_pf_export_particle": [vp, u32, vp, u64, vp],
        "lama_hip_pf_import_particle": [vp, u32, vp, u64], "lama_hip_pf_export_particles": [vp, u32, vp, vp, vp, vp],
        "lama_hip_pf_import_particles": [vp, u32, vp, vp, vp], "lama_hip_get_counters": [vp, vp], "lama_hip_get_counters_sized": [vp, vp, u32],
        "lama_hip_counters_bytes": [], "lama_hip_reset_counters": [vp], "lama_hip_map_add_obstacles": [vp, u32, vp, u32],
        "lama_hip_match_solve": [vp, u32, vp, u32, vp, vp, vp, vp, vp, i32], "lama_hip_eval_batch": [vp, u32, vp, u32, vp, vp, vp, u32, vp, vp],
        "lama_hip_pf_patch_ids": [vp, u32, i32, u32, vp, vp], "lama_hip_pf_delete_patches": [vp, u32, vp, u32, vp],
        "lama_hip_map_sample_likelihood": [vp, u32, vp, u32, vp, vp, d, vp, u32, u32, vp],
        "lama_hip_match_eval": [vp, u32, vp, u32, vp, vp, vp, vp, vp], "lama_hip_match_cell_distances": [vp, u32, vp, u32, vp, vp, vp, vp],
        "lama_hip_match_solve_with": [vp, u32, vp, u32, vp, vp, vp, vp, vp, i32, u32],
        "lama_hip_blob_alloc": [vp, u64, vp], "lama_hip_blob_free": [vp, vp], "lama_hip_blob_copy": [vp, vp, vp, vp, u64],
    }
    # groups the engine test double (tests/cpu_engine) may lack: a library has a whole group or none of it, probed by its first name
    optional = [
        {"lama_hip_map_integrate_scans": [vp, u32, u32, vp, vp, vp, vp, vp, u32], "lama_hip_map_occupied_cells": [vp, u32, u32, vp, vp]},
        {"lama_hip_map_bounds": [vp, u32, i32, vp, vp, vp], "lama_hip_map_rasterize": [vp, u32, i32, u32, u32, u32, u32, u32, vp, u64]},
        {"lama_hip_map_cast_rays": [vp, u32, i32, u32, vp, vp, u32, vp, vp, u32, i32, vp, vp, vp, vp, vp, vp, vp, vp]},
        {"lama_hip_map_frontiers": [vp, u32, u32, u32, u32, u32, u32, u32, u32, vp, vp, vp, vp, vp]},
        {"lama_hip_map_travel": [vp, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, vp, u32, vp, u32, vp, u32, vp, vp, vp, vp],
         "lama_hip_map_travel_stats": [vp, vp, vp, vp, vp]},
        {"lama_hip_match_solve_batch": [vp, u32, vp, vp, vp, vp, vp, vp, vp, i32, i32, d, vp, vp, vp]},
        {"lama_hip_match_search_lattice": [vp, u32, vp, u32, vp, vp, u32, vp, u32, d, d, u32, u32, u32, u32, vp, vp]},
        {"lama_hip_pf_map_checksums": [vp, i32, vp]},                                            # device-only diagnostic
        {"lama_hip_pf_match_and_map": [vp, vp, u32, vp, vp, vp, vp, vp, vp], "lama_hip_pf_step_groups": [vp, vp, vp]},   # whole device step
        {"lama_hip_pgo_create": [i32, u32, vp, vp, vp, vp, u32, vp], "lama_hip_pgo_destroy": [vp], "lama_hip_pgo_last_error": [vp],
         "lama_hip_pgo_linearize": [vp, vp, vp, vp, vp, vp, vp, vp], "lama_hip_pgo_pattern": [vp, vp, vp, vp], "lama_hip_pgo_set_poses": [vp, vp],
         "lama_hip_pgo_get_poses": [vp, vp], "lama_hip_pgo_linearize_system": [vp, vp, vp, vp, vp, vp], "lama_hip_pgo_try_step": [vp, vp, vp, vp],
         "lama_hip_pgo_accept": [vp], "lama_hip_pgo_solve_pcg": [vp, d, d, u32, u32, vp, vp, vp, vp, vp, vp],
         "lama_hip_pgo_try_solved_step": [vp, vp, vp], "lama_hip_pgo_create_robust": [i32, u32, vp, vp, vp, vp, vp, vp, u32, vp],
         "lama_hip_pgo_factor_weights": [vp, vp]},
    ]
    # every other entry point returns an int32_t status
    restypes = {"lama_hip_default_cfg": None, "lama_hip_ctx_destroy": None, "lama_hip_last_error": C.c_char_p, "lama_hip_pgo_destroy": None,
                "lama_hip_pgo_last_error": C.c_char_p}
    return required, optional, restypes


_HIP_REQUIRED, _HIP_OPTIONAL, _HIP_RESTYPES = _hip_signatures()
HIP_SYMBOLS = list(_HIP_REQUIRED) + [name for group in _HIP_OPTIONAL for name in group]

_hip = None
_hip_wide = None


def _torch_runtime_first():
    """A process that also uses PyTorch-ROCm must load torch's HIP runtime FIRST: torch bundles its own libamdhip64, and when
    /opt/rocm's copy (which liblama_hip.so links) is already loaded, torch.cuda finds "no HIP GPUs" afterwards (measured on the
    MI355X box; the other order works: liblama_hip.so then binds to the copy torch brought).  Importing torch is enough; done
    before the device library is loaded -- directly or through liblama_host.so -- whenever torch is installed."""
    if "torch" not in sys.modules and not os.environ.get("LAMA_NO_TORCH_PRELOAD"):
        try:
            import importlib.util
            if importlib.util.find_spec("torch") is not None:
                import torch  # noqa: F401
        except Exception:      # torch is optional: a broken install must not make liblama_hip.so unloadable (set LAMA_NO_TORCH_PRELOAD=1
            pass               # to skip the import altogether, e.g. for pure-ctypes users who never touch torch)


def hip_lib(wide=False):
    """Load liblama_hip.so -- or, with wide=True, liblama_hip_wide.so, the build of the same sources for distance maps with an
    l2_max of 128 .. 255 cells (csrc/lama_dev.h).  Raises if it has not been built: there is no fallback path."""
    global _hip, _hip_wide
    if wide:
        if _hip_wide is None:
            if not os.path.exists(HIP_LIB_WIDE):
                raise LamaError(f"{HIP_LIB_WIDE} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU fallback.")
            _torch_runtime_first()
            L = C.CDLL(HIP_LIB_WIDE)
            _bind_hip(L)
            _hip_wide = L
        return _hip_wide
    if _hip is None:
        if not os.path.exists(HIP_LIB):
            raise LamaError(f"{HIP_LIB} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        _torch_runtime_first()
        L = C.CDLL(HIP_LIB)
        _bind_hip(L)
        _hip = L
    return _hip


def needs_wide(l2_max, resolution):
    """True when a distance map of this reach needs liblama_hip_wide.so: ceil(l2_max / resolution) > 127 cells (as
    lama_hip_ctx_create and the host classes compute it, DynamicDistanceMap::setMaxDistance)."""
    return resolution > 0.0 and math.ceil(l2_max * (1.0 / resolution)) > 127


def is_device_library(path):
    """Is this engine origin one of the two device libraries (and not the test double of tests/cpu_engine)?"""
    return path.endswith("liblama_hip.so") or path.endswith("liblama_hip_wide.so")


def _lib_of_origin(path):
    if path.endswith("liblama_hip.so"):
        return hip_lib()
    if path.endswith("liblama_hip_wide.so"):
        return hip_lib(wide=True)
    L = C.CDLL(path)                   # test double bound through set_engine_library()
    _bind_hip(L)
    return L


def hip_lib_or_none():
    return _hip


def _bind_hip(L):
    for group in [_HIP_REQUIRED] + [g for g in _HIP_OPTIONAL if hasattr(L, next(iter(g)))]:
        for name, argtypes in group.items():
            f = getattr(L, name)
            f.argtypes = argtypes
            f.restype = _HIP_RESTYPES.get(name, C.c_int32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


_IDQ = np.array([1.0, 0.0, 0.0, 0.0])
_Z3 = np.zeros(3)


MAP_BUILD_FULL, MAP_BUILD_PRUNE = 1, 2
RASTER_TRINARY, RASTER_PROBABILITY, RASTER_SQDIST = 0, 1, 2      # LAMA_HIP_RASTER_*
RAY_STOP_UNKNOWN = 1                                               # LAMA_HIP_RAY_STOP_UNKNOWN
RAY_NONE, RAY_OCCUPIED, RAY_UNKNOWN = 0, 1, 2                      # LAMA_HIP_RAY_* status
RAY_AGREES, RAY_BLOCKED, RAY_NOVEL = 0, 1, 2                       # LAMA_HIP_RAY_* label
ROBUST_KINDS = {"unit": 0, "tukey": 1, "tdist": 2, "cauchy": 3, "huber": 4}      # LAMA_HIP_ROBUST_*
ROBUST_STORED = 0x100     # LAMA_HIP_ROBUST_STORED: robust_param is the constant as the class stores it (b * b, 1 / param^2)
E_NUMERIC = -6


def pack_scans(scans):
    """A list of (n_k, 3) point arrays -> (points (N, 3) float64, offsets (K + 1,) uint32); a (points, offsets) tuple is checked and
    passed on.  Raises ValueError -- before any device is touched -- for offsets that decrease, do not start at 0 or do not end at
    the number of points, and for point arrays that are not (n, 3)."""
    if isinstance(scans, tuple) and len(scans) == 2 and not (hasattr(scans[1], "ndim") and np.ndim(scans[1]) == 2):
        pts = np.ascontiguousarray(scans[0], dtype=np.float64)
        offs = np.asarray(scans[1])
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError("points must be (N, 3)")
        if offs.ndim != 1 or len(offs) < 1 or np.any(offs < 0) or np.any(offs > 0xFFFFFFFF):
            raise ValueError("offsets must be K + 1 non-negative 32-bit numbers")
        offs = np.ascontiguousarray(offs, dtype=np.uint32)
        if np.any(np.diff(offs.astype(np.int64)) < 0):
            raise ValueError("scan offsets must not decrease")
        if offs[0] != 0 or offs[-1] != len(pts):
            raise ValueError(f"scan offsets must run from 0 to the number of points ({len(pts)}), got {offs[0]} .. {offs[-1]}")
        return pts, offs
    arrs = []
    for a in scans:
        a = np.asarray(a, dtype=np.float64)
        if a.size == 0:
            a = a.reshape(0, 3)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError("every scan must be (n, 3)")
        arrs.append(a)
    offs = np.zeros(len(arrs) + 1, dtype=np.uint32)
    if arrs:
        offs[1:] = np.cumsum([len(a) for a in arrs])
    pts = np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros((0, 3)), dtype=np.float64)
    return pts, offs


def default_cfg(**kw):
    cfg = HipCfg()
    hip_lib().lama_hip_default_cfg(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def device_count():
    n = C.c_int32(0)
    hip_lib().lama_hip_device_count(C.byref(n))
    return n.value


class GridOptions(C.Structure):
    """lama_grid_options (include/lama_host.h): lama::sdm::GridOptions"""
    _fields_ = [("stride", C.c_uint32), ("probability", C.c_int32), ("whole_map", C.c_int32), ("world_min", C.c_double * 2), ("world_max", C.c_double * 2)]


class GridHeader(C.Structure):
    """lama_grid (include/lama_host.h)"""
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("stride", C.c_uint32),
                ("element_bytes", C.c_uint32), ("resolution", C.c_double), ("cell_size", C.c_double), ("max_distance", C.c_double),
                ("origin", C.c_double * 3)]


class Grid:
    """A dense grid of a device map (lama::sdm::OccupancyGrid / DistanceGrid): `data` is (height, width), int8 occupancy values
    (0 free, 100 occupied, -1 unknown; or 0 .. 100) or uint16 squared cell distances; pixel (i, j) = data[j, i] covers the map cells
    from (x0 + i * stride, y0 + j * stride); origin = Map::m2w of cell (x0, y0)."""

    def __init__(self, hdr, data):
        for name, _ in GridHeader._fields_:
            setattr(self, name, getattr(hdr, name))
        self.origin = np.array(list(hdr.origin))
        self.data = data

    def metres(self):
        """DistanceGrid::metres of every pixel: sqrt(sqdist) * resolution"""
        return np.sqrt(self.data.astype(np.float64)) * self.resolution


# lama_hip_frontier (include/lama_hip.h), 40 bytes
FRONTIER_T = np.dtype([("label", "<u4"), ("pixels", "<u4"), ("min_i", "<u4"), ("min_j", "<u4"), ("max_i", "<u4"), ("max_j", "<u4"),
                       ("sum_i", "<u8"), ("sum_j", "<u8")])
NO_FRONTIER = 0xFFFFFFFF                                            # labels: not a frontier pixel


class Frontiers:
    """What lama_hip_map_frontiers returned: records (FRONTIER_T, the first min(cap, n) clusters by pixels descending, then label
    ascending), n (clusters with pixels >= min_pixels), frontier_pixels (all of them), labels ((height, width) uint32, NO_FRONTIER
    where the pixel is none; None unless asked for), kernel_ms."""

    def __init__(self, records, n, frontier_pixels, labels, kernel_ms):
        self.records, self.n, self.frontier_pixels, self.labels, self.kernel_ms = records, n, frontier_pixels, labels, kernel_ms


class FrontierOptions(C.Structure):
    """lama_frontier_options (include/lama_host.h): lama::sdm::FrontierOptions"""
    _fields_ = [("stride", C.c_uint32), ("whole_map", C.c_int32), ("world_min", C.c_double * 2), ("world_max", C.c_double * 2),
                ("min_pixels", C.c_uint32), ("max_frontiers", C.c_uint32), ("labels", C.c_int32)]


class FrontierSetHeader(C.Structure):
    """lama_frontier_set (include/lama_host.h)"""
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("stride", C.c_uint32), ("count", C.c_uint32),
                ("resolution", C.c_double), ("cell_size", C.c_double), ("origin", C.c_double * 3), ("frontier_pixels", C.c_uint64), ("clusters", C.c_uint64)]


# lama_frontier (include/lama_host.h), 72 bytes: the device record plus centroid and seed in world metres
HOST_FRONTIER_T = np.dtype(FRONTIER_T.descr + [("centroid", "<f8", (2,)), ("seed", "<f8", (2,))])


class FrontierSet:
    """lama::sdm::FrontierSet: the box (x0, y0, width, height, stride, resolution, cell_size, origin as in Grid), `frontiers`
    (HOST_FRONTIER_T, by pixels descending then label ascending), frontier_pixels, clusters, labels ((height, width) uint32 or None)."""

    def __init__(self, hdr, frontiers, labels):
        for name, _ in FrontierSetHeader._fields_:
            setattr(self, name, getattr(hdr, name))
        self.origin = np.array(list(hdr.origin))
        self.frontiers, self.labels = frontiers, labels


# lama_hip_route (include/lama_hip.h), 16 bytes
ROUTE_T = np.dtype([("status", "<u4"), ("pixel", "<u4"), ("cost", "<u4"), ("steps", "<u4")])
ROUTE_REACHED, ROUTE_UNREACHED, ROUTE_OUTSIDE = 0, 1, 2
NO_ROUTE = 0xFFFFFFFF                                               # the field at an unreached pixel; pixel and cost of a route not REACHED


class Travel:
    """What lama_hip_map_travel returned: routes (ROUTE_T, one per goal), paths ((goals, path_cap) uint32 pixel indices, SOURCE
    first; row g holds min(path_cap, steps + 1) entries, the rest is NO_ROUTE; None with path_cap 0), field ((height, width) uint32,
    NO_ROUTE where unreached; None unless asked for), rounds and kernel_ms (diagnostics)."""

    def __init__(self, routes, paths, field, rounds, kernel_ms):
        self.routes, self.paths, self.field, self.rounds, self.kernel_ms = routes, paths, field, rounds, kernel_ms

    def path(self, g):
        """the pixels of goal g's path that were written, source first"""
        r = self.routes[g]
        return self.paths[g, :min(self.paths.shape[1], int(r["steps"]) + 1)] if r["status"] == ROUTE_REACHED else self.paths[g, :0]


class TravelOptions(C.Structure):
    """lama_travel_options (include/lama_host.h): lama::sdm::TravelOptions"""
    _fields_ = [("stride", C.c_uint32), ("whole_map", C.c_int32), ("world_min", C.c_double * 2), ("world_max", C.c_double * 2),
                ("robot_radius", C.c_double), ("preferred_clearance", C.c_double), ("near_factor", C.c_uint32), ("goal_reach", C.c_uint32),
                ("max_path_points", C.c_uint32), ("field", C.c_int32)]


class RouteSetHeader(C.Structure):
    """lama_route_set (include/lama_host.h)"""
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("stride", C.c_uint32), ("count", C.c_uint32),
                ("resolution", C.c_double), ("cell_size", C.c_double), ("origin", C.c_double * 3), ("path_points", C.c_uint64), ("rounds", C.c_uint32),
                ("has_field", C.c_uint32)]


# lama_route (include/lama_host.h), 40 bytes
HOST_ROUTE_T = np.dtype(ROUTE_T.descr + [("length_m", "<f8"), ("path_first", "<u8"), ("path_points", "<u4"), ("reserved", "<u4")])


class RouteSet:
    """lama::sdm::RouteSet: the box (x0, y0, width, height, stride, resolution, cell_size, origin as in Grid), `routes` (HOST_ROUTE_T,
    one per goal), `paths` (per route an (n, 2) array of world points, source first; empty unless reached), `field` ((height, width)
    uint32, NO_ROUTE where no route leads, or None), rounds."""

    def __init__(self, hdr, routes, points, field):
        for name, _ in RouteSetHeader._fields_:
            setattr(self, name, getattr(hdr, name))
        self.origin = np.array(list(hdr.origin))
        self.routes, self.field = routes, field
        self.paths = [points[int(r["path_first"]):int(r["path_first"]) + int(r["path_points"])] for r in routes]


class RayOptions(C.Structure):
    """lama_ray_options (include/lama_host.h): lama::sdm::RayCastOptions"""
    _fields_ = [("map", C.c_int32), ("stop_at_unknown", C.c_int32), ("tolerance_cells", C.c_int32)]


class RayResultPointers(C.Structure):
    """lama_ray_result (include/lama_host.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("status", "step", "nn", "cell_xy", "end_sqdist", "label", "start_xy", "range")]


def ray_ranges(resolution, start_xy, cell_xy, status):
    """lama::sdm::rayRange over a result: resolution * sqrt(dx^2 + dy^2) of the stopping cell's integer offset from its pose's start
    cell (one correctly rounded square root of an exact integer), +inf where status is RAY_NONE.  start_xy (K, 2), cell_xy (K, n, 2)."""
    d = (cell_xy.astype(np.int64) - start_xy.astype(np.int64)[:, None, :]).astype(np.float64)     # (below 2^14 cells where a ray stopped: exact)
    r = float(resolution) * np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    return np.where(status != RAY_NONE, r, np.inf)


class RayCast:
    """What lama_hip_map_cast_rays / castRays returned, every array (num_poses, n) -- cell_xy (num_poses, n, 2), start_xy
    (num_poses, 2): status (RAY_NONE / RAY_OCCUPIED / RAY_UNKNOWN), step (-1: nothing stopped the beam), nn, cell_xy (the stopping
    cell, else the point's), end_sqdist, label (RAY_AGREES / RAY_BLOCKED / RAY_NOVEL, None without a tolerance), range in metres
    (+inf where nothing stopped the beam), kernel_ms (context-level calls)."""

    def __init__(self, K, n, labels):
        self.status = np.zeros((K, n), dtype=np.uint8)
        self.step = np.zeros((K, n), dtype=np.int32)
        self.nn = np.zeros((K, n), dtype=np.uint32)
        self.cell_xy = np.zeros((K, n, 2), dtype=np.uint32)
        self.end_sqdist = np.zeros((K, n), dtype=np.uint32)
        self.label = np.zeros((K, n), dtype=np.uint8) if labels else None
        self.start_xy = np.zeros((K, 2), dtype=np.uint32)
        self.range = None
        self.kernel_ms = None


def fan_points(n, angle_min, angle_increment, max_range):
    """lama::sdm::makeFan: the points (n, 3) of n beams from angle_min with angle_increment, each max_range long (sensor frame)"""
    a = [angle_min + float(i) * angle_increment for i in range(int(n))]      # (libm's cos / sin per beam, as the C++ helper takes them)
    return np.array([(max_range * math.cos(t), max_range * math.sin(t), 0.0) for t in a], dtype=np.float64).reshape(-1, 3)


class _Handle:
    """A native handle `h` of the library `L`: the names of its destroy and last-error entry points and -- for the host classes --
    of the accessor of the device context, whose particle count is `_ctx_P`."""
    _destroy = _last_error = _context = None
    _ctx_P = 1
    _grid_prefix = None            # "lama_slam", ...: the class has <prefix>_occupancy_grid / <prefix>_distance_grid

    def _grid(self, what, args, stride, probability, world_box):
        o = GridOptions()
        self.L.lama_grid_default_options(C.byref(o))
        o.stride, o.probability = int(stride), 1 if probability else 0
        if world_box is not None:
            o.whole_map = 0
            o.world_min[0], o.world_min[1], o.world_max[0], o.world_max[1] = (float(v) for v in world_box)
        hdr = GridHeader()
        rc = getattr(self.L, f"{self._grid_prefix}_{what}_grid")(self.h, *args, C.byref(o), C.byref(hdr))
        if rc < 0:
            raise LamaError(self._error())
        if rc == 0:
            return None
        data = np.zeros((hdr.height, hdr.width), dtype=np.uint16 if hdr.element_bytes == 2 else np.int8)
        assert self.L.lama_grid_fetch(_p(data), data.nbytes) == data.nbytes
        return Grid(hdr, data)

    def occupancy_grid(self, stride=1, probability=False, world_box=None):
        """getOccupancyGrid: the dense occupancy grid made on the device -> Grid, or None while there is no map.  world_box =
        (min x, min y, max x, max y) in metres instead of the whole map."""
        return self._grid("occupancy", (), stride, probability, world_box)

    def distance_grid(self, stride=1, world_box=None):
        """getDistanceGrid -> Grid of uint16 squared cell distances (Grid.metres()), or None while there is no map."""
        return self._grid("distance", (), stride, False, world_box)

    def frontiers(self, stride=1, min_pixels=1, max_frontiers=0, labels=False, world_box=None, _args=()):
        """getFrontiers: the clusters of free pixels that border unknown space in the object's device occupancy map, labelled on the
        device -> FrontierSet, or None while there is no map.  world_box as for occupancy_grid."""
        o = FrontierOptions()
        self.L.lama_frontier_default_options(C.byref(o))
        o.stride, o.min_pixels, o.max_frontiers, o.labels = int(stride), int(min_pixels), int(max_frontiers), 1 if labels else 0
        if world_box is not None:
            o.whole_map = 0
            o.world_min[0], o.world_min[1], o.world_max[0], o.world_max[1] = (float(v) for v in world_box)
        hdr = FrontierSetHeader()
        rc = getattr(self.L, f"{self._grid_prefix}_frontiers")(self.h, *_args, C.byref(o), C.byref(hdr))
        if rc < 0:
            raise LamaError(self._error())
        if rc == 0:
            return None
        recs = np.zeros(hdr.count, dtype=HOST_FRONTIER_T)
        lab = np.full((hdr.height, hdr.width), NO_FRONTIER, dtype=np.uint32) if labels else None
        assert self.L.lama_frontiers_fetch(_p(recs), len(recs), _p(lab), 0 if lab is None else lab.size) == hdr.count
        return FrontierSet(hdr, recs, lab)

    def routes(self, from_xy, goals_xy, stride=1, robot_radius=0.0, preferred_clearance=0.0, near_factor=1, goal_reach=0, max_path_points=1024, field=False,
               world_box=None, _args=()):
        """planRoutes: from the world points from_xy ((n, 2) metres, or one point) to each of goals_xy ((m, 2)) through the object's
        device maps -- reachability, cost and path, relaxed on the device -> RouteSet, or None while there is no map.  world_box as
        for occupancy_grid."""
        o = TravelOptions()
        self.L.lama_travel_default_options(C.byref(o))
        o.stride, o.robot_radius, o.preferred_clearance = int(stride), float(robot_radius), float(preferred_clearance)
        o.near_factor, o.goal_reach, o.max_path_points, o.field = int(near_factor), int(goal_reach), int(max_path_points), 1 if field else 0
        if world_box is not None:
            o.whole_map = 0
            o.world_min[0], o.world_min[1], o.world_max[0], o.world_max[1] = (float(v) for v in world_box)
        src = np.ascontiguousarray(np.asarray(from_xy, dtype=np.float64).reshape(-1, 2))
        gl = np.ascontiguousarray(np.asarray(goals_xy, dtype=np.float64).reshape(-1, 2))
        hdr = RouteSetHeader()
        rc = getattr(self.L, f"{self._grid_prefix}_plan_routes")(self.h, *_args, _p(src), len(src), _p(gl), len(gl), C.byref(o), C.byref(hdr))
        if rc < 0:
            raise LamaError(self._error())
        if rc == 0:
            return None
        recs = np.zeros(hdr.count, dtype=HOST_ROUTE_T)
        pts = np.zeros((hdr.path_points, 2))
        fld = np.zeros((hdr.height, hdr.width), dtype=np.uint32) if hdr.has_field else None
        assert self.L.lama_routes_fetch(_p(recs), len(recs), _p(pts), len(pts), _p(fld), 0 if fld is None else fld.size) == hdr.count
        return RouteSet(hdr, recs, pts, fld)

    def cast_rays(self, poses4, pts, origin=None, quat=None, distance_map=False, stop_at_unknown=False, tolerance_cells=-1, _args=()):
        """castRays: what a sensor at each pose {c, s, tx, ty} of poses4 (K, 4) would see in the object's device map -- the
        occupancy map, or with distance_map=True the distance map (lama::Loc2D: always) -> RayCast, or None while there is no map."""
        pts, origin, quat = self._scan(pts, origin, quat)
        poses4 = np.ascontiguousarray(poses4, dtype=np.float64).reshape(-1, 4)
        o = RayOptions(0 if distance_map or self._grid_prefix == "lama_loc" else 1, 1 if stop_at_unknown else 0, int(tolerance_cells))
        r = RayCast(len(poses4), len(pts), tolerance_cells >= 0)
        r.range = np.zeros(r.status.shape)
        ptrs = RayResultPointers(*[_p(a) for a in (r.status, r.step, r.nn, r.cell_xy, r.end_sqdist, r.label, r.start_xy, r.range)])
        rc = getattr(self.L, f"{self._grid_prefix}_cast_rays")(self.h, *_args, _p(poses4), len(poses4), _p(pts), len(pts), _p(origin), _p(quat), C.byref(o), C.byref(ptrs))
        if rc < 0:
            raise LamaError(self._error())
        return r if rc else None

    def expected_ranges(self, poses4, n, angle_min, angle_increment, max_range, origin=None, quat=None, **kw):
        """The simulated scan of a beam model: the range (K, n) at which each beam of a fan of max_range first meets an occupied
        cell, +inf where it meets none; None while there is no map."""
        r = self.cast_rays(poses4, fan_points(n, angle_min, angle_increment, max_range), origin, quat, **kw)
        return None if r is None else r.range

    def close(self):
        if getattr(self, "h", None) and not getattr(self, "_is_borrowed", False):
            getattr(self.L, self._destroy)(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def _error(self):
        return getattr(self.L, self._last_error)(self.h).decode()

    def _chk(self, rc):
        if rc < 0:
            raise LamaError(self._error())
        return rc

    @staticmethod
    def _scan(pts, origin, quat):
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        origin = np.ascontiguousarray(_Z3 if origin is None else origin, dtype=np.float64)
        quat = np.ascontiguousarray(_IDQ if quat is None else quat, dtype=np.float64)
        return pts, origin, quat

    def hip_context(self):
        """Borrowed HipContext view of the object's device context (export/import, counters, map downloads): closing it leaves the
        context to its owner."""
        ctx = HipContext.__new__(HipContext)
        ctx.L = _lib_of_origin(self.engine_origin())
        ctx.cfg = None
        ctx.P = self._ctx_P
        ctx.h = C.c_void_p(getattr(self.L, self._context)(self.h))
        ctx._is_borrowed = True
        return ctx


class HipContext(_Handle):
    """One device context = one shard of the particle pool (include/lama_hip.h)."""
    _destroy, _last_error = "lama_hip_ctx_destroy", "lama_hip_last_error"

    def __init__(self, cfg):
        self.L = hip_lib(wide=needs_wide(cfg.l2_max, cfg.resolution))
        self.cfg = cfg
        self.P = cfg.particles
        h = C.c_void_p()
        rc = self.L.lama_hip_ctx_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise LamaError(f"lama_hip_ctx_create failed with status {rc} (no usable HIP device or invalid cfg)")
        self.h = h

    def _chk(self, rc):
        if rc != 0:
            raise LamaError(f"status {rc}: {self._error()}")

    def init(self, pts, pose0, origin=None, quat=None):
        pts, origin, quat = self._scan(pts, origin, quat)
        pose0 = np.ascontiguousarray(pose0, dtype=np.float64)
        self._chk(self.L.lama_hip_pf_init(self.h, _p(pts), len(pts), _p(origin), _p(quat), _p(pose0)))

    def set_poses(self, poses):
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        assert poses.shape == (self.P, 4)
        self._chk(self.L.lama_hip_pf_set_poses(self.h, _p(poses)))

    def get_poses(self):
        out = np.zeros((self.P, 4))
        self._chk(self.L.lama_hip_pf_get_poses(self.h, _p(out)))
        return out

    def scan_match(self, pts, origin=None, quat=None):
        pts, origin, quat = self._scan(pts, origin, quat)
        poses = np.zeros((self.P, 4))
        ll = np.zeros(self.P)
        it = np.zeros(self.P, dtype=np.int32)
        self._chk(self.L.lama_hip_pf_scan_match(self.h, _p(pts), len(pts), _p(origin), _p(quat), _p(poses), _p(ll), _p(it)))
        return poses, ll, it

    def resample(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        assert idx.shape == (self.P,)
        self._chk(self.L.lama_hip_pf_resample(self.h, _p(idx)))

    def update_maps(self, pts, origin=None, quat=None):
        pts, origin, quat = self._scan(pts, origin, quat)
        self._chk(self.L.lama_hip_pf_update_maps(self.h, _p(pts), len(pts), _p(origin), _p(quat)))

    def match_and_map(self, pts, poses, origin=None, quat=None):
        """One whole device step: scan match from `poses`, then the map update of the matched poses, queued (its status is collected
        by the next call on the context).  Pools below 64 particles run it as particle groups on streams of their own."""
        pts, origin, quat = self._scan(pts, origin, quat)
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        assert poses.shape == (self.P, 4)
        out = np.zeros((self.P, 4))
        ll = np.zeros(self.P)
        it = np.zeros(self.P, dtype=np.int32)
        self._chk(self.L.lama_hip_pf_match_and_map(self.h, _p(pts), len(pts), _p(origin), _p(quat), _p(poses), _p(out), _p(ll), _p(it)))
        return out, ll, it

    def step_groups(self):
        """Particle groups the last match_and_map ran (1: the single-stream schedule; 0: none yet).  Waits for the device."""
        n = C.c_uint32(0)
        self._chk(self.L.lama_hip_pf_step_groups(self.h, C.byref(n), None))
        return int(n.value)

    def configured_step_groups(self):
        """Groups a step of this context is split into when it can be (0: never, the single-stream schedule).  Waits for nothing."""
        n = C.c_uint32(0)
        self._chk(self.L.lama_hip_pf_step_groups(self.h, None, C.byref(n)))
        return int(n.value)

    def download_map(self, particle, kind):
        """{reference patch id: (cells[1024] in the reference record format, mask[16])}"""
        n = C.c_uint32(0)
        self._chk(self.L.lama_hip_pf_map_patches(self.h, particle, kind, C.byref(n)))
        n = n.value
        ids = np.zeros(n, dtype=np.uint64)
        dt = DIST_T if kind == MAP_DISTANCE else FREQ_T
        cells = np.zeros((n, 1024), dtype=dt)
        masks = np.zeros((n, 16), dtype=np.uint64)
        got = C.c_uint32(0)
        self._chk(self.L.lama_hip_pf_download_map(self.h, particle, kind, n, _p(ids), _p(cells), _p(masks), C.byref(got)))
        assert got.value == n
        return {int(ids[k]): (cells[k], masks[k]) for k in range(n)}

    def upload_map(self, particle, kind, patches):
        """The inverse of download_map: replace the particle's map of `kind` by {patch id: (cells[1024], mask[16])}."""
        ids = np.array(sorted(patches), dtype=np.uint64)
        dt = DIST_T if kind == MAP_DISTANCE else FREQ_T
        cells = np.zeros((len(ids), 1024), dtype=dt)
        masks = np.zeros((len(ids), 16), dtype=np.uint64)
        for k, i in enumerate(ids):
            cells[k], masks[k] = patches[int(i)]
        self._chk(self.L.lama_hip_pf_upload_map(self.h, particle, kind, len(ids), _p(ids), _p(cells), _p(masks)))

    def match_batch(self, particle, pts, poses, origin=None, quat=None):
        pts, origin, quat = self._scan(pts, origin, quat)
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        out = np.zeros(len(poses))
        self._chk(self.L.lama_hip_match_batch(self.h, particle, _p(pts), len(pts), _p(origin), _p(quat), _p(poses), len(poses), _p(out)))
        return out

    def update_maps_begin(self, pts, origin=None, quat=None):
        """Queues the map update and returns; status and counters are collected by sync() or the next call."""
        pts, origin, quat = self._scan(pts, origin, quat)
        self._chk(self.L.lama_hip_pf_update_maps_begin(self.h, _p(pts), len(pts), _p(origin), _p(quat)))

    def sync(self):
        self._chk(self.L.lama_hip_sync(self.h))

    def device(self):
        """HIP device ordinal of the context."""
        return int(self.L.lama_hip_ctx_device(self.h))

    def map_checksums(self, kind):
        """One 64-bit checksum per particle of its distance / occupancy map (patch set, cells, masks), computed on the device."""
        out = np.zeros(self.P, dtype=np.uint64)
        self._chk(self.L.lama_hip_pf_map_checksums(self.h, kind, _p(out)))
        return out

    def patch_ids(self, particle, kind):
        n = C.c_uint32(0)
        self._chk(self.L.lama_hip_pf_patch_ids(self.h, particle, kind, 0, None, C.byref(n)))
        ids = np.zeros(n.value, dtype=np.uint64)
        self._chk(self.L.lama_hip_pf_patch_ids(self.h, particle, kind, n.value, _p(ids), C.byref(n)))
        return ids

    def delete_patches(self, particle, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        d = C.c_uint32(0)
        self._chk(self.L.lama_hip_pf_delete_patches(self.h, particle, _p(ids), len(ids), C.byref(d)))
        return d.value

    def eval_batch(self, particle, pts, poses, origin=None, quat=None):
        """-> (squared residual norm, log-likelihood) per pose (Loc2D::globalLocalization's candidate evaluation)"""
        pts, origin, quat = self._scan(pts, origin, quat)
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        sq, ll = np.zeros(len(poses)), np.zeros(len(poses))
        self._chk(self.L.lama_hip_eval_batch(self.h, particle, _p(pts), len(pts), _p(origin), _p(quat), _p(poses), len(poses), _p(sq), _p(ll)))
        return sq, ll

    def sample_likelihood(self, particle, pts, yaw, xy, point_step, origin=None, quat=None):
        pts, origin, quat = self._scan(pts, origin, quat)
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        out = np.zeros(len(xy))
        self._chk(self.L.lama_hip_map_sample_likelihood(self.h, particle, _p(pts), len(pts), _p(origin), _p(quat), float(yaw), _p(xy),
                                                        len(xy), int(point_step), _p(out)))
        return out

    def add_obstacles(self, particle, cells_xy):
        cells = np.ascontiguousarray(cells_xy, dtype=np.uint32).reshape(-1, 2)
        self._chk(self.L.lama_hip_map_add_obstacles(self.h, particle, _p(cells), len(cells)))

    def integrate_scans(self, particle, poses4, scans, origins=None, quats=None, full=True, prune=True):
        """lama_hip_map_integrate_scans: `scans` is a list of (n_k, 3) point arrays -- or a tuple (points, offsets) already
        concatenated --, poses4 (K, 4) {c, s, tx, ty}, origins (K, 3) / quats (K, 4) per scan (None: zero / identity)."""
        pts, offs = pack_scans(scans)
        K = len(offs) - 1
        poses4 = np.ascontiguousarray(poses4, dtype=np.float64).reshape(-1, 4)
        if len(poses4) != K:
            raise ValueError(f"{len(poses4)} poses for {K} scans")
        if origins is not None:
            origins = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
            if len(origins) != K:
                raise ValueError(f"{len(origins)} sensor origins for {K} scans")
        if quats is not None:
            quats = np.ascontiguousarray(quats, dtype=np.float64).reshape(-1, 4)
            if len(quats) != K:
                raise ValueError(f"{len(quats)} sensor orientations for {K} scans")
        flags = (MAP_BUILD_FULL if full else 0) | (MAP_BUILD_PRUNE if prune else 0)
        self._chk(self.L.lama_hip_map_integrate_scans(self.h, particle, K, _p(poses4), _p(pts), _p(offs), _p(origins), _p(quats), flags))

    def occupied_cells(self, particle):
        """lama_hip_map_occupied_cells: (n, 2) map coordinates of the occupied cells, in visit_all_cells order."""
        n = C.c_uint32(0)
        self._chk(self.L.lama_hip_map_occupied_cells(self.h, particle, 0, None, C.byref(n)))
        out = np.zeros((n.value, 2), dtype=np.uint32)
        if n.value:
            self._chk(self.L.lama_hip_map_occupied_cells(self.h, particle, n.value, _p(out), C.byref(n)))
        return out

    def map_bounds(self, particle, kind):
        """lama_hip_map_bounds: Map::bounds of the device map -> (min (2,) uint32, max (2,) uint32, number of patches)."""
        lo, hi, n = np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint32), C.c_uint32(0)
        self._chk(self.L.lama_hip_map_bounds(self.h, particle, kind, _p(lo), _p(hi), C.byref(n)))
        return lo, hi, int(n.value)

    def rasterize(self, particle, layer, x0, y0, width, height, stride=1):
        """lama_hip_map_rasterize: the dense grid of a box of the map, shape (height, width); int8 for RASTER_TRINARY (0 free, 100
        occupied, -1 unknown) and RASTER_PROBABILITY (0 .. 100, -1), uint16 squared cell distances for RASTER_SQDIST."""
        out = np.zeros((int(height), int(width)), dtype=np.uint16 if layer == RASTER_SQDIST else np.int8)
        self._chk(self.L.lama_hip_map_rasterize(self.h, particle, int(layer), int(x0), int(y0), int(width), int(height), int(stride), _p(out), out.nbytes))
        return out

    def map_frontiers(self, particle, x0, y0, width, height, stride=1, min_pixels=1, cap=None, labels=False):
        """lama_hip_map_frontiers: the frontier clusters (free pixels with an unknown edge neighbour, 8-connected) of a box of
        `particle`'s occupancy map -> Frontiers.  cap=None: every cluster (a second call where more than 1024 exist)."""
        lab = np.zeros((int(height), int(width)), dtype=np.uint32) if labels else None
        n, fp, ms = C.c_uint32(0), C.c_uint64(0), C.c_double(0.0)
        want = 1024 if cap is None else int(cap)
        while True:
            rec = np.zeros(want, dtype=FRONTIER_T)
            self._chk(self.L.lama_hip_map_frontiers(self.h, int(particle), int(x0), int(y0), int(width), int(height), int(stride), int(min_pixels), want,
                                                    _p(rec) if want else None, C.byref(n), C.byref(fp), _p(lab), C.byref(ms)))
            if cap is not None or n.value <= want:
                break
            want = n.value
        return Frontiers(rec[:min(want, n.value)], int(n.value), int(fp.value), lab, ms.value)

    def travel(self, particle, x0, y0, width, height, sources, goals=(), stride=1, clearance_cells=0, prefer_cells=None, near_factor=1, goal_reach=0,
               path_cap=0, field=False):
        """lama_hip_map_travel: the travel-cost field of a box of `particle`'s maps from `sources` ((n, 2) map cells), the best pixel
        within goal_reach of each of `goals` ((m, 2) map cells) and the path to it -> Travel.  prefer_cells=None: clearance_cells."""
        if not hasattr(self.L, "lama_hip_map_travel"):
            raise LamaError("the device library has no lama_hip_map_travel (routes through device maps)")
        src = np.ascontiguousarray(np.asarray(sources, dtype=np.uint32).reshape(-1, 2))
        gl = np.ascontiguousarray(np.asarray(goals, dtype=np.uint32).reshape(-1, 2))
        routes = np.zeros(len(gl), dtype=ROUTE_T)
        paths = np.full((len(gl), int(path_cap)), NO_ROUTE, dtype=np.uint32) if path_cap else None
        fld = np.zeros((int(height), int(width)), dtype=np.uint32) if field else None
        rounds, ms = C.c_uint32(0), C.c_double(0.0)
        self._chk(self.L.lama_hip_map_travel(self.h, int(particle), int(x0), int(y0), int(width), int(height), int(stride), int(clearance_cells),
                                             int(clearance_cells if prefer_cells is None else prefer_cells), int(near_factor), len(src), _p(src) if len(src) else None,
                                             len(gl), _p(gl) if len(gl) else None, int(goal_reach), _p(routes) if len(gl) else None, int(path_cap),
                                             _p(paths) if paths is not None and paths.size else None, _p(fld), C.byref(rounds), C.byref(ms)))
        return Travel(routes, paths, fld, int(rounds.value), ms.value)

    def travel_stats(self):
        """lama_hip_map_travel_stats -> dict(rounds, tiles_run, max_tiles, readbacks) of the context's last travel call"""
        r, t, m, b = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
        self._chk(self.L.lama_hip_map_travel_stats(self.h, C.byref(r), C.byref(t), C.byref(m), C.byref(b)))
        return {"rounds": int(r.value), "tiles_run": int(t.value), "max_tiles": int(m.value), "readbacks": int(b.value)}

    def cast_rays(self, particle, kind, poses4, pts, origin=None, quat=None, stop_at_unknown=False, tolerance_cells=-1, resolution=None):
        """lama_hip_map_cast_rays: per pose of poses4 (K, 4) and point of pts (n, 3) the first cell of `particle`'s map of `kind`
        (MAP_DISTANCE / MAP_OCCUPANCY) that stops the beam -> RayCast (range from `resolution`, default the context's cfg)."""
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        poses4 = np.ascontiguousarray(poses4, dtype=np.float64).reshape(-1, 4)
        origin = None if origin is None else np.ascontiguousarray(origin, dtype=np.float64)
        quat = None if quat is None else np.ascontiguousarray(quat, dtype=np.float64)
        r = RayCast(len(poses4), len(pts), tolerance_cells >= 0)
        ms = C.c_double(0.0)
        self._chk(self.L.lama_hip_map_cast_rays(self.h, int(particle), int(kind), len(poses4), _p(poses4), _p(pts), len(pts), _p(origin), _p(quat),
                                                RAY_STOP_UNKNOWN if stop_at_unknown else 0, int(tolerance_cells), _p(r.status), _p(r.step), _p(r.nn),
                                                _p(r.cell_xy), _p(r.end_sqdist), _p(r.label), _p(r.start_xy), C.byref(ms)))
        r.kernel_ms = ms.value
        res = resolution if resolution is not None else (self.cfg.resolution if self.cfg is not None else None)
        if res is not None:
            r.range = ray_ranges(res, r.start_xy, r.cell_xy, r.status)
        return r

    def match_solve(self, particle, pts, pose4, origin=None, quat=None, solve=True):
        """-> (pose, JtJ lower [00,10,11,20,21,22], sum r^2 (unweighted), iterations)"""
        pts, origin, quat = self._scan(pts, origin, quat)
        pose = np.array(pose4, dtype=np.float64)
        out = np.zeros(7)
        it = C.c_int32(0)
        self._chk(self.L.lama_hip_match_solve(self.h, particle, _p(pts), len(pts), _p(origin), _p(quat), _p(pose), _p(out),
                                              C.byref(it), 1 if solve else 0))
        return pose, out[:6].copy(), float(out[6]), it.value

    def match_solve_with(self, particle, pts, pose4, strategy=0, max_iterations=0, origin=None, quat=None):
        """lama_hip_match_solve_with -> (pose, out7, iterations): strategy 0 = GaussNewton, 1 = LevenbergMarquard; Cauchy(0.15)"""
        pts, origin, quat = self._scan(pts, origin, quat)
        pose = np.array(pose4, dtype=np.float64)
        out = np.zeros(7)
        it = C.c_int32(0)
        self._chk(self.L.lama_hip_match_solve_with(self.h, particle, _p(pts), len(pts), _p(origin), _p(quat), _p(pose), _p(out),
                                                   C.byref(it), int(strategy), int(max_iterations)))
        return pose, out, it.value

    def match_solve_batch(self, particles, scans, poses4, max_iterations=100, strategy=0, robust="cauchy", robust_param=0.15,
                          origins=None, quats=None, check=True):
        """lama_hip_match_solve_batch: B registrations in one launch.  `scans` is a list of (n_b, 3) point arrays or a
        (points, offsets) tuple (pack_scans); particles (B,) or one number; poses4 (B, 4) {c, s, tx, ty}; max_iterations (B,) or one
        number (0: evaluate only); robust a name of ROBUST_KINDS or a LAMA_HIP_ROBUST_* number; origins (B, 3) / quats (B, 4) or
        None.  -> (poses (B, 4), out8 (B, 8), iterations (B,), status (B,)).  With check=False a LAMA_HIP_E_NUMERIC return (some
        problem met a zero-norm unit complex; status marks it) does not raise."""
        pts, offs = pack_scans(scans)
        B = len(offs) - 1
        poses = np.array(poses4, dtype=np.float64).reshape(-1, 4)
        if len(poses) != B:
            raise ValueError(f"{len(poses)} poses for {B} problems")
        pa = np.ascontiguousarray(np.broadcast_to(np.asarray(particles, dtype=np.uint32), (B,)))
        mi = np.ascontiguousarray(np.broadcast_to(np.asarray(max_iterations, dtype=np.uint32), (B,)))
        if origins is not None:
            origins = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
            if len(origins) != B:
                raise ValueError(f"{len(origins)} sensor origins for {B} problems")
        if quats is not None:
            quats = np.ascontiguousarray(quats, dtype=np.float64).reshape(-1, 4)
            if len(quats) != B:
                raise ValueError(f"{len(quats)} sensor orientations for {B} problems")
        kind = ROBUST_KINDS[robust] if isinstance(robust, str) else int(robust)
        out8, it, st = np.zeros((B, 8)), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint32)
        args = (self.h, B, _p(pa), _p(pts), _p(offs), _p(origins), _p(quats), _p(poses), _p(mi), int(strategy), kind, float(robust_param),
                _p(out8), _p(it), _p(st))
        rc = self.L.lama_hip_match_solve_batch(*args)
        if rc != 0 and (check or rc != E_NUMERIC):
            self._chk(rc)
        return poses, out8, it, st

    def search_lattice(self, particle, pts, headings, wx0, wy0, cell_step, nx, ny, tile=8, point_step=1, origin=None, quat=None, scores=True):
        """lama_hip_match_search_lattice: the score of every node of a pose lattice and the best key of every tile.  `headings` are
        angles in radians (their cos / sin are taken here, on the host) or an (H, 2) array of {cos, sin}; node (0, 0) is at the
        world position (wx0, wy0), node (ix, iy) cell_step * (ix, iy) cells further.
        -> (best (H, ceil(ny / tile), ceil(nx / tile)) uint64 keys score << 32 | index, scores (H, ny, nx) uint32 or None)"""
        pts, origin, quat = self._scan(pts, origin, quat)
        hd = np.asarray(headings, dtype=np.float64)
        cs = np.ascontiguousarray(hd if hd.ndim == 2 else np.stack([np.cos(hd), np.sin(hd)], axis=1).reshape(-1, 2))
        H, nx, ny, tile = len(cs), int(nx), int(ny), int(tile)
        if nx < 1 or ny < 1 or tile < 1:
            raise ValueError("nx, ny and tile are at least 1")
        best = np.zeros((H, (ny + tile - 1) // tile, (nx + tile - 1) // tile), dtype=np.uint64)
        sc = np.zeros((H, ny, nx), dtype=np.uint32) if scores else None
        self._chk(self.L.lama_hip_match_search_lattice(self.h, particle, _p(pts), len(pts), _p(origin), _p(quat), int(point_step), _p(cs), H,
                                                       float(wx0), float(wy0), int(cell_step), nx, ny, tile, _p(best), _p(sc)))
        return best, sc

    def match_eval(self, particle, pts, pose4, origin=None, quat=None, jac=True):
        """-> (residuals[n], Jacobian n x 3 or None): MatchSurface2D::eval on the particle's distance map, no robust weight"""
        pts, origin, quat = self._scan(pts, origin, quat)
        n = len(pts)
        pose = np.ascontiguousarray(pose4, dtype=np.float64)
        r, J = np.zeros(n), (np.zeros((3, n)) if jac else None)
        self._chk(self.L.lama_hip_match_eval(self.h, particle, _p(pts), n, _p(origin), _p(quat), _p(pose), _p(r), _p(J)))
        return r, (J.T.copy() if jac else None)

    def cell_distances(self, particle, pts, pose4, origin=None, quat=None):
        """-> distance of the cell w2m(tf * p_i) of every point, no interpolation (MatchSurface2D::error's terms)"""
        pts, origin, quat = self._scan(pts, origin, quat)
        n = len(pts)
        pose = np.ascontiguousarray(pose4, dtype=np.float64)
        d = np.zeros(n)
        self._chk(self.L.lama_hip_match_cell_distances(self.h, particle, _p(pts), n, _p(origin), _p(quat), _p(pose), _p(d)))
        return d

    def export_bytes(self, particle):
        n = C.c_uint64(0)
        self._chk(self.L.lama_hip_pf_export_particle(self.h, particle, None, 0, C.byref(n)))
        return n.value

    def export_particle(self, particle, device_ptr, cap):
        n = C.c_uint64(0)
        self._chk(self.L.lama_hip_pf_export_particle(self.h, particle, C.c_void_p(device_ptr), cap, C.byref(n)))
        return n.value

    def import_particle(self, particle, device_ptr, nbytes):
        self._chk(self.L.lama_hip_pf_import_particle(self.h, particle, C.c_void_p(device_ptr), nbytes))

    def export_sizes(self, particles):
        """Blob sizes of a batch of particles (host mirror of the patch counts: no device work)."""
        pa = np.ascontiguousarray(particles, dtype=np.uint32)
        out = np.zeros(len(pa), dtype=np.uint64)
        self._chk(self.L.lama_hip_pf_export_particles(self.h, len(pa), _p(pa), None, None, _p(out)))
        return out

    def export_particles(self, particles, device_ptrs, caps):
        """All outgoing particles of a resample in one launch (device_ptrs: one buffer address per particle)."""
        pa = np.ascontiguousarray(particles, dtype=np.uint32)
        ptrs = np.ascontiguousarray(device_ptrs, dtype=np.uint64)
        cp = np.ascontiguousarray(caps, dtype=np.uint64)
        out = np.zeros(len(pa), dtype=np.uint64)
        self._chk(self.L.lama_hip_pf_export_particles(self.h, len(pa), _p(pa), _p(ptrs), _p(cp), _p(out)))
        return out

    def import_particles(self, particles, device_ptrs, nbytes):
        pa = np.ascontiguousarray(particles, dtype=np.uint32)
        ptrs = np.ascontiguousarray(device_ptrs, dtype=np.uint64)
        nb = np.ascontiguousarray(nbytes, dtype=np.uint64)
        self._chk(self.L.lama_hip_pf_import_particles(self.h, len(pa), _p(pa), _p(ptrs), _p(nb)))

    def counters(self):
        c = HipCounters()
        self._chk(self.L.lama_hip_get_counters(self.h, C.byref(c)))
        d = c.as_dict()
        if hasattr(self.L, "lama_hip_pf_step_groups"):        # (its own getter: the struct's tail is pinned by a consumer check)
            d["step_groups"] = self.step_groups()
        return d

    def reset_counters(self):
        self._chk(self.L.lama_hip_reset_counters(self.h))


# ------------------------------------------------------------------------------------------------ host library
_host = None


def host_lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise LamaError(f"{HOST_LIB} is missing: run `make -C iris_lama_amd host`")
        _torch_runtime_first()                                # (the host library loads liblama_hip.so when a device object is created)
        L = C.CDLL(HOST_LIB)
        L.lama_corridor_generate.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.lama_corridor_generate.restype = C.c_int
        _host = L
    return _host


def corridor_log(steps=40, beams=1080):
    """Seeded synthetic corridor log: pts (steps+1, beams, 3), odom xyr, truth xyr."""
    pts = np.zeros((steps + 1, beams, 3))
    odom = np.zeros((steps + 1, 3))
    truth = np.zeros((steps + 1, 3))
    rc = host_lib().lama_corridor_generate(steps, beams, _p(pts), _p(odom), _p(truth))
    if rc != 0:
        raise LamaError("lama_corridor_generate failed")
    return pts, odom, truth


# ------------------------------------------------------------------------------------------------ lama::PFSlam2D
class PFOptions(C.Structure):
    _fields_ = [("particles", C.c_uint32), ("srr", C.c_double), ("str", C.c_double), ("stt", C.c_double),
                ("srt", C.c_double), ("meas_sigma", C.c_double), ("meas_sigma_gain", C.c_double),
                ("trans_thresh", C.c_double), ("rot_thresh", C.c_double), ("l2_max", C.c_double),
                ("truncated_ray", C.c_double), ("truncated_range", C.c_double), ("resolution", C.c_double),
                ("patch_size", C.c_uint32), ("max_iter", C.c_uint32), ("seed", C.c_uint32),
                ("create_summary", C.c_int32), ("gpu_device", C.c_int32), ("shard_rank", C.c_uint32),
                ("shard_world", C.c_uint32), ("profile", C.c_int32), ("brushfire_mode", C.c_uint32),
                ("window_patches", C.c_uint32), ("dm_patch_capacity", C.c_uint32), ("occ_patch_capacity", C.c_uint32),
                ("queue_capacity", C.c_uint32), ("gpus", C.c_int32)]


HOST_SYMBOLS = [
    "lama_corridor_generate", "lama_pf_default_options", "lama_pf_engine_origin",
    "lama_pf_create", "lama_pf_destroy", "lama_pf_last_error", "lama_pf_set_prior", "lama_pf_update",
    "lama_pf_update_begin", "lama_pf_local_range", "lama_pf_local_loglik", "lama_pf_plan_resample",
    "lama_pf_apply_resample", "lama_pf_update_maps", "lama_pf_device_context", "lama_pf_get_poses",
    "lama_pf_set_pose", "lama_pf_get_weights", "lama_pf_set_weights", "lama_pf_neff", "lama_pf_best",
    "lama_pf_best_pose_xyr", "lama_pf_num_resamples", "lama_pf_exchange_times", "lama_pf_shard_context", "lama_pf_memory_usage", "lama_pf_summary",
    "lama_pf_last_times", "lama_pf_draw_from_motion", "lama_pf_normalize", "lama_pf_resample_indices",
    "lama_pose_minus", "lama_pose_from_xyr",
    "lama_slam_default_options", "lama_slam_create", "lama_slam_destroy", "lama_slam_last_error", "lama_slam_set_pose",
    "lama_slam_get_pose", "lama_slam_update", "lama_slam_enough_motion", "lama_slam_processed_cells",
    "lama_slam_iterations", "lama_slam_device_context", "lama_slam_engine_origin", "lama_slam_deleted_patches", "lama_loc_create3",
    "lama_slam_view_bounds", "lama_slam_view_cells", "lama_slam_view_occupancy", "lama_slam_view_distance_cells", "lama_slam_view_distance_points",
    "lama_slam_match_eval", "lama_slam_match_solve", "lama_slam_match_solve_generic", "lama_slam_solve_batch",
    "lama_slam_correlative_search", "lama_loc_relocalize", "lama_loc_relocalize_candidates",
    "lama_loc_create", "lama_loc_destroy", "lama_loc_last_error", "lama_loc_engine_origin", "lama_loc_set_obstacles_world",
    "lama_loc_write_distance_map", "lama_loc_read_distance_map", "lama_loc_device_context",
    "lama_loc_set_pose", "lama_loc_get_pose", "lama_loc_update", "lama_loc_covar", "lama_loc_rmse", "lama_loc_iterations",
    "lama_loc_create2", "lama_loc_occ_set_cells", "lama_loc_occ_bounds", "lama_loc_trigger_global_localization",
    "lama_loc_global_localization_active", "lama_loc_gloc_candidates", "lama_loc_sampling_likelihoods",
    "lama_random_set_seed", "lama_random_uniform",
    "lama_frontier_default_options", "lama_frontiers_fetch", "lama_slam_frontiers", "lama_pf_frontiers", "lama_mapbuilder_frontiers", "lama_lo_frontiers",
    "lama_travel_default_options", "lama_routes_fetch", "lama_slam_plan_routes", "lama_pf_plan_routes", "lama_mapbuilder_plan_routes", "lama_lo_plan_routes",
    "lama_loc_plan_routes",
    "lama_sdm_write", "lama_sdm_read", "lama_sdm_image", "lama_sdm_export_png", "lama_dm_build", "lama_dm_build_fetch",
    "lama_lo_create", "lama_lo_destroy", "lama_lo_last_error", "lama_lo_engine_origin", "lama_lo_update", "lama_lo_get_odom",
    "lama_lo_iterations", "lama_lo_deleted_patches", "lama_lo_device_context",
    "lama_pgo_optimize", "lama_pgo_optimize_with", "lama_pose_graph_optimize",
    "lama_mapbuilder_default_options", "lama_mapbuilder_create", "lama_mapbuilder_destroy", "lama_mapbuilder_last_error",
    "lama_mapbuilder_engine_origin", "lama_mapbuilder_device_context", "lama_mapbuilder_add", "lama_mapbuilder_set_pose",
    "lama_mapbuilder_set_poses", "lama_mapbuilder_build", "lama_mapbuilder_reset", "lama_mapbuilder_occupied_cells",
    "lama_mapbuilder_timing", "lama_mapbuilder_view_cells", "lama_mapbuilder_match_solve",
    "lama_grid_default_options", "lama_grid_fetch", "lama_slam_occupancy_grid", "lama_slam_distance_grid", "lama_pf_occupancy_grid",
    "lama_pf_distance_grid", "lama_mapbuilder_occupancy_grid", "lama_mapbuilder_distance_grid", "lama_lo_occupancy_grid",
    "lama_lo_distance_grid", "lama_loc_distance_grid",
    "lama_ray_default_options", "lama_slam_cast_rays", "lama_pf_cast_rays", "lama_mapbuilder_cast_rays", "lama_lo_cast_rays",
    "lama_loc_cast_rays", "lama_loc_check_scan", "lama_slam_view_cast_rays",
]


def _bind_host(L):
    vp, i32, u32, d = C.c_void_p, C.c_int32, C.c_uint32, C.c_double
    sig = {
        "lama_pf_default_options": (None, [vp]),
        "lama_pf_engine_origin": (C.c_char_p, [vp]), "lama_pf_create": (vp, [vp, vp, i32]),
        "lama_pf_destroy": (None, [vp]), "lama_pf_last_error": (C.c_char_p, [vp]),
        "lama_pf_set_prior": (None, [vp, d, d, d]), "lama_pf_update": (i32, [vp, vp, u32, vp, vp, vp, d]),
        "lama_pf_update_begin": (i32, [vp, vp, u32, vp, vp, vp, d]), "lama_pf_local_range": (i32, [vp, vp, vp]),
        "lama_pf_local_loglik": (i32, [vp, vp]), "lama_pf_plan_resample": (i32, [vp, vp, vp]),
        "lama_pf_apply_resample": (i32, [vp, vp]), "lama_pf_update_maps": (i32, [vp]),
        "lama_pf_device_context": (vp, [vp]), "lama_pf_get_poses": (i32, [vp, vp]),
        "lama_pf_set_pose": (i32, [vp, u32, vp]), "lama_pf_get_weights": (i32, [vp, vp, vp, vp]),
        "lama_pf_set_weights": (i32, [vp, vp, vp]), "lama_pf_neff": (d, [vp]), "lama_pf_best": (i32, [vp]),
        "lama_pf_best_pose_xyr": (i32, [vp, vp]), "lama_pf_num_resamples": (u32, [vp]),
        "lama_pf_exchange_times": (i32, [vp, vp]), "lama_pf_shard_context": (vp, [vp, u32]),
        "lama_pf_memory_usage": (C.c_uint64, [vp]), "lama_pf_summary": (i32, [vp, vp, i32]),
        "lama_pf_last_times": (i32, [vp, vp]), "lama_pf_draw_from_motion": (i32, [vp, vp, vp]),
        "lama_pf_normalize": (d, [vp]), "lama_pf_resample_indices": (i32, [vp, d, vp]),
        "lama_pose_minus": (None, [vp, vp, vp]), "lama_pose_from_xyr": (None, [d, d, d, vp]),
        "lama_slam_default_options": (None, [vp]), "lama_slam_create": (vp, [vp, vp, i32]), "lama_slam_destroy": (None, [vp]),
        "lama_slam_last_error": (C.c_char_p, [vp]), "lama_slam_set_pose": (None, [vp, d, d, d]),
        "lama_slam_get_pose": (i32, [vp, vp]), "lama_slam_update": (i32, [vp, vp, u32, vp, vp, vp, d]),
        "lama_slam_enough_motion": (i32, [vp, vp]), "lama_slam_processed_cells": (u32, [vp]),
        "lama_slam_iterations": (u32, [vp]), "lama_slam_device_context": (vp, [vp]), "lama_slam_deleted_patches": (u32, [vp]),
        "lama_slam_engine_origin": (C.c_char_p, [vp]),
        "lama_slam_view_bounds": (i32, [vp, i32, vp, vp, vp, vp]), "lama_slam_view_cells": (C.c_int64, [vp, i32, vp, C.c_uint64]),
        "lama_slam_view_occupancy": (i32, [vp, C.c_uint64, vp, vp, vp, vp, vp]),
        "lama_slam_view_distance_cells": (i32, [vp, C.c_uint64, vp, vp]), "lama_slam_view_distance_points": (i32, [vp, C.c_uint64, vp, vp]),
        "lama_slam_match_eval": (i32, [vp, vp, u32, vp, vp, vp, vp, vp, vp]),
        "lama_slam_match_solve": (i32, [vp, vp, u32, vp, vp, vp, C.c_char_p, C.c_char_p, d, u32, vp, vp]),
        "lama_slam_match_solve_generic": (i32, [vp, vp, u32, vp, vp, vp, C.c_char_p, C.c_char_p, d, u32, vp, vp]),
        "lama_slam_solve_batch": (i32, [vp, vp, u32, vp, vp, vp, vp, vp, vp, C.c_char_p, d, C.c_char_p, d, vp, vp, vp]),
        "lama_slam_correlative_search": (i32, [vp, vp, u32, vp, vp, vp, d, d, u32, u32, u32, i32, u32, u32, vp, vp, vp, vp, vp, vp, vp]),
        "lama_loc_relocalize": (i32, [vp, vp, u32, vp, vp, d, d, u32, u32, u32, u32]),
        "lama_loc_relocalize_candidates": (u32, [vp, u32, vp, vp, vp, vp, vp]),
        "lama_loc_create": (vp, [d, d, d, d, u32, i32, vp, i32]), "lama_loc_destroy": (None, [vp]),
        "lama_loc_last_error": (C.c_char_p, [vp]), "lama_loc_engine_origin": (C.c_char_p, [vp]),
        "lama_loc_set_obstacles_world": (i32, [vp, vp, u32]), "lama_loc_write_distance_map": (i32, [vp, C.c_char_p]), "lama_loc_read_distance_map": (i32, [vp, C.c_char_p]), "lama_loc_device_context": (vp, [vp]), "lama_loc_set_pose": (None, [vp, d, d, d]),
        "lama_loc_get_pose": (i32, [vp, vp]), "lama_loc_update": (i32, [vp, vp, u32, vp, vp, vp, d, i32]),
        "lama_loc_covar": (i32, [vp, vp]), "lama_loc_rmse": (d, [vp]), "lama_loc_iterations": (u32, [vp]),
        "lama_loc_create2": (vp, [d, d, d, d, u32, u32, u32, d, d, i32, vp, i32]),
        "lama_loc_create3": (vp, [d, d, d, d, u32, u32, u32, d, d, C.c_char_p, i32, vp, i32]),
        "lama_loc_occ_set_cells": (i32, [vp, vp, u32, i32]), "lama_loc_occ_bounds": (i32, [vp, vp]),
        "lama_loc_trigger_global_localization": (None, [vp]), "lama_loc_global_localization_active": (i32, [vp]),
        "lama_loc_gloc_candidates": (u32, [vp, vp, vp, u32]), "lama_loc_sampling_likelihoods": (u32, [vp, vp, u32]),
        "lama_random_set_seed": (None, [u32]), "lama_random_uniform": (d, []),
        "lama_lo_create": (vp, [d, u32, i32, vp, i32]), "lama_lo_destroy": (None, [vp]), "lama_lo_last_error": (C.c_char_p, [vp]),
        "lama_lo_engine_origin": (C.c_char_p, [vp]), "lama_lo_update": (i32, [vp, vp, u32, vp, vp, d]),
        "lama_lo_get_odom": (i32, [vp, vp]), "lama_lo_iterations": (u32, [vp]), "lama_lo_deleted_patches": (u32, [vp]),
        "lama_lo_device_context": (vp, [vp]),
        "lama_sdm_write": (i32, [C.c_char_p, i32, d, u32, u32, vp, vp, vp]),
        "lama_sdm_read": (i32, [C.c_char_p, vp, vp, vp, u32, vp, vp, vp, vp]),
        "lama_sdm_image": (i32, [i32, d, u32, u32, vp, vp, vp, vp, vp, vp, C.c_uint64]),
        "lama_sdm_export_png": (i32, [i32, d, u32, u32, vp, vp, vp, C.c_char_p]),
        "lama_dm_build": (C.c_int64, [vp, C.c_uint64, u32, vp]), "lama_dm_build_fetch": (i32, [vp, vp, vp]),
        "lama_pgo_optimize": (i32, [vp, u32, vp, vp, vp, u32, vp, vp, u32, i32, vp, vp, vp, u32, vp, i32]),
        "lama_pgo_optimize_with": (i32, [vp, u32, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, u32, vp, i32]),
        "lama_pose_graph_optimize": (i32, [vp, u32, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, vp, i32]),
        "lama_mapbuilder_default_options": (None, [vp]), "lama_mapbuilder_create": (vp, [vp, vp, i32]), "lama_mapbuilder_destroy": (None, [vp]),
        "lama_mapbuilder_last_error": (C.c_char_p, [vp]), "lama_mapbuilder_engine_origin": (C.c_char_p, [vp]),
        "lama_mapbuilder_device_context": (vp, [vp]), "lama_mapbuilder_add": (C.c_int64, [vp, vp, u32, vp, vp, vp]),
        "lama_mapbuilder_set_pose": (i32, [vp, C.c_uint64, vp]), "lama_mapbuilder_set_poses": (i32, [vp, vp, C.c_uint64]),
        "lama_mapbuilder_build": (i32, [vp]), "lama_mapbuilder_reset": (i32, [vp]),
        "lama_mapbuilder_occupied_cells": (C.c_int64, [vp, vp, C.c_uint64]), "lama_mapbuilder_timing": (i32, [vp, vp]),
        "lama_mapbuilder_view_cells": (C.c_int64, [vp, i32, vp, C.c_uint64]),
        "lama_mapbuilder_match_solve": (i32, [vp, vp, u32, vp, vp, vp, u32, vp]),
        "lama_grid_default_options": (None, [vp]), "lama_grid_fetch": (C.c_int64, [vp, C.c_uint64]),
        "lama_slam_occupancy_grid": (i32, [vp, vp, vp]), "lama_slam_distance_grid": (i32, [vp, vp, vp]),
        "lama_pf_occupancy_grid": (i32, [vp, C.c_int64, vp, vp]), "lama_pf_distance_grid": (i32, [vp, C.c_int64, vp, vp]),
        "lama_mapbuilder_occupancy_grid": (i32, [vp, vp, vp]), "lama_mapbuilder_distance_grid": (i32, [vp, vp, vp]),
        "lama_lo_occupancy_grid": (i32, [vp, vp, vp]), "lama_lo_distance_grid": (i32, [vp, vp, vp]),
        "lama_loc_distance_grid": (i32, [vp, vp, vp]),
        "lama_ray_default_options": (None, [vp]),
        "lama_frontier_default_options": (None, [vp]), "lama_frontiers_fetch": (C.c_int64, [vp, C.c_uint64, vp, C.c_uint64]),
        "lama_slam_frontiers": (i32, [vp, vp, vp]), "lama_pf_frontiers": (i32, [vp, C.c_int64, vp, vp]),
        "lama_mapbuilder_frontiers": (i32, [vp, vp, vp]), "lama_lo_frontiers": (i32, [vp, vp, vp]),
        "lama_travel_default_options": (None, [vp]), "lama_routes_fetch": (C.c_int64, [vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64]),
        "lama_slam_plan_routes": (i32, [vp, vp, u32, vp, u32, vp, vp]), "lama_pf_plan_routes": (i32, [vp, C.c_int64, vp, u32, vp, u32, vp, vp]),
        "lama_mapbuilder_plan_routes": (i32, [vp, vp, u32, vp, u32, vp, vp]), "lama_lo_plan_routes": (i32, [vp, vp, u32, vp, u32, vp, vp]),
        "lama_loc_plan_routes": (i32, [vp, vp, u32, vp, u32, vp, vp]),
        "lama_slam_cast_rays": (i32, [vp, vp, u32, vp, u32, vp, vp, vp, vp]), "lama_pf_cast_rays": (i32, [vp, C.c_int64, vp, u32, vp, u32, vp, vp, vp, vp]),
        "lama_mapbuilder_cast_rays": (i32, [vp, vp, u32, vp, u32, vp, vp, vp, vp]), "lama_lo_cast_rays": (i32, [vp, vp, u32, vp, u32, vp, vp, vp, vp]),
        "lama_loc_cast_rays": (i32, [vp, vp, u32, vp, u32, vp, vp, vp, vp]),
        "lama_loc_check_scan": (C.c_int64, [vp, vp, u32, vp, vp, i32, vp]),
        "lama_slam_view_cast_rays": (i32, [vp, vp, u32, vp, u32, vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args


_host_bound = False


def _hostlib():
    global _host_bound
    L = host_lib()
    if not _host_bound:
        _bind_host(L)
        _host_bound = True
    return L


def use_host_library(path=None):
    """Load the host C-ABI (include/lama_host.h) from `path` instead of iris_lama_amd/lib/liblama_host.so (None = back to the
    product library).  The product never calls this; the test-suite loads its own -DLAMA_TESTING build of the same sources
    (tests/_testhost.py), the only build that can bind anything but liblama_hip.so.  Objects created before the switch keep
    working only as long as no call is made through them afterwards: switch between, not during, uses."""
    global _host, _host_bound, HOST_LIB
    HOST_LIB = path or _PRODUCT_HOST_LIB
    _host = None
    _host_bound = False


def pf_options(**kw):
    o = PFOptions()
    _hostlib().lama_pf_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def pose_from_xyr(x, y, yaw):
    out = np.zeros(4)
    _hostlib().lama_pose_from_xyr(float(x), float(y), float(yaw), _p(out))
    return out


class PFSlam2D(_Handle):
    """ctypes view of the host-side lama::PFSlam2D (include/lama/pf_slam2d.h)."""
    _destroy, _last_error, _context = "lama_pf_destroy", "lama_pf_last_error", "lama_pf_device_context"
    _grid_prefix = "lama_pf"

    def occupancy_grid(self, stride=1, probability=False, world_box=None, particle=None):
        """getOccupancyGrid (the best particle's) / getParticleOccupancyGrid(particle) -> Grid, or None (no map yet, or the
        particle lives in another process)."""
        return self._grid("occupancy", (-1 if particle is None else int(particle),), stride, probability, world_box)

    def distance_grid(self, stride=1, world_box=None, particle=None):
        return self._grid("distance", (-1 if particle is None else int(particle),), stride, False, world_box)

    def frontiers(self, particle=None, **kw):
        """getFrontiers (the best particle's) / getParticleFrontiers(particle) -> FrontierSet, or None"""
        return _Handle.frontiers(self, _args=(-1 if particle is None else int(particle),), **kw)

    def routes(self, from_xy, goals_xy, particle=None, **kw):
        """planRoutes (the best particle's maps) / planParticleRoutes(particle) -> RouteSet, or None"""
        return _Handle.routes(self, from_xy, goals_xy, _args=(-1 if particle is None else int(particle),), **kw)

    def cast_rays(self, poses4, pts, origin=None, quat=None, particle=None, **kw):
        """castRays (the best particle's maps) / castParticleRays(particle) -> RayCast, or None (no map yet, or the particle lives
        in another process)."""
        return _Handle.cast_rays(self, poses4, pts, origin, quat, _args=(-1 if particle is None else int(particle),), **kw)

    def __init__(self, opts):
        self.L = _hostlib()
        self.opts = opts
        self.P = opts.particles
        err = C.create_string_buffer(512)
        h = self.L.lama_pf_create(C.byref(opts), err, 512)
        if not h:
            raise LamaError(err.value.decode())
        self.h = C.c_void_p(h)
        lo, hi = C.c_uint32(0), C.c_uint32(0)
        self.L.lama_pf_local_range(self.h, C.byref(lo), C.byref(hi))
        self.lo, self.hi = lo.value, hi.value
        self._ctx_P = self.hi - self.lo                       # hip_context() views the local shard

    def engine_origin(self):
        return self.L.lama_pf_engine_origin(self.h).decode()

    def set_prior(self, x, y, yaw):
        self.L.lama_pf_set_prior(self.h, float(x), float(y), float(yaw))

    def update(self, pts, odom_xyr, ts=0.0, origin=None, quat=None):
        pts, origin, quat = self._scan(pts, origin, quat)
        od = np.ascontiguousarray(odom_xyr, dtype=np.float64)
        return bool(self._chk(self.L.lama_pf_update(self.h, _p(pts), len(pts), _p(origin), _p(quat), _p(od), float(ts))))

    def update_begin(self, pts, odom_xyr, ts=0.0, origin=None, quat=None):
        pts, origin, quat = self._scan(pts, origin, quat)
        od = np.ascontiguousarray(odom_xyr, dtype=np.float64)
        return self._chk(self.L.lama_pf_update_begin(self.h, _p(pts), len(pts), _p(origin), _p(quat), _p(od), float(ts)))

    def local_loglik(self):
        out = np.zeros(self.hi - self.lo)
        self.L.lama_pf_local_loglik(self.h, _p(out))
        return out

    def plan_resample(self, all_loglik):
        all_loglik = np.ascontiguousarray(all_loglik, dtype=np.float64)
        assert all_loglik.shape == (self.P,)
        idx = np.zeros(self.P, dtype=np.int32)
        r = self._chk(self.L.lama_pf_plan_resample(self.h, _p(all_loglik), _p(idx)))
        return idx if r else None

    def apply_resample(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        self._chk(self.L.lama_pf_apply_resample(self.h, _p(idx)))

    def update_maps(self):
        self._chk(self.L.lama_pf_update_maps(self.h))

    def device_context(self):
        return self.L.lama_pf_device_context(self.h)

    def poses(self):
        out = np.zeros((self.P, 4))
        self.L.lama_pf_get_poses(self.h, _p(out))
        return out

    def set_pose(self, i, pose4):
        self._chk(self.L.lama_pf_set_pose(self.h, i, _p(np.ascontiguousarray(pose4, dtype=np.float64))))

    def weights(self):
        w, nw, ws = np.zeros(self.P), np.zeros(self.P), np.zeros(self.P)
        self.L.lama_pf_get_weights(self.h, _p(w), _p(nw), _p(ws))
        return w, nw, ws

    def set_weights(self, w=None, ws=None):
        self.L.lama_pf_set_weights(self.h, _p(np.ascontiguousarray(w)) if w is not None else None,
                                   _p(np.ascontiguousarray(ws)) if ws is not None else None)

    def neff(self):
        return self.L.lama_pf_neff(self.h)

    def best(self):
        return self.L.lama_pf_best(self.h)

    def best_pose_xyr(self):
        out = np.zeros(3)
        self.L.lama_pf_best_pose_xyr(self.h, _p(out))
        return out

    def num_resamples(self):
        return self.L.lama_pf_num_resamples(self.h)

    def exchange_times(self):
        """Options::gpus > 1: what the last update spent exchanging (seconds) and shipped between shards."""
        t = np.zeros(8)
        n = self.L.lama_pf_exchange_times(self.h, _p(t))
        return dict(shards=n, gather_s=t[0], ship_s=t[1], import_s=t[2], shipped_particles=int(t[3]), shipped_bytes=int(t[4]),
                    local_copies_s=t[5], phase_begin_s=t[6], phase_maps_s=t[7])

    def shard_context(self, r):
        """HipContext view of shard r's device context (Options::gpus > 1), None when out of range."""
        h = self.L.lama_pf_shard_context(self.h, r)
        if not h:
            return None
        ctx = self.hip_context()
        ctx.h = C.c_void_p(h)
        G = self.opts.gpus
        ctx.P = ((r + 1) * self.P + G - 1) // G - (r * self.P + G - 1) // G
        return ctx

    def memory_usage(self):
        return self.L.lama_pf_memory_usage(self.h)

    def summary(self):
        n = self.L.lama_pf_summary(self.h, None, 0)
        if n <= 0:
            return ""
        buf = C.create_string_buffer(n)
        self.L.lama_pf_summary(self.h, buf, n)
        return buf.value.decode()

    def last_times(self):
        t = np.zeros(5)
        self.L.lama_pf_last_times(self.h, _p(t))
        return dict(total=t[0], solving=t[1], normalizing=t[2], resampling=t[3], mapping=t[4])

    def draw_from_motion(self, delta4, pose4):
        pose = np.array(pose4, dtype=np.float64)
        self._chk(self.L.lama_pf_draw_from_motion(self.h, _p(np.ascontiguousarray(delta4, dtype=np.float64)), _p(pose)))
        return pose

    def normalize(self):
        return self.L.lama_pf_normalize(self.h)

    def resample_indices(self, u):
        out = np.zeros(self.P, dtype=np.int32)
        self.L.lama_pf_resample_indices(self.h, float(u), _p(out))
        return out


class SlamOptions(C.Structure):
    _fields_ = [("trans_thresh", C.c_double), ("rot_thresh", C.c_double), ("l2_max", C.c_double),
                ("truncated_ray", C.c_double), ("truncated_range", C.c_double), ("resolution", C.c_double),
                ("patch_size", C.c_uint32), ("max_iter", C.c_uint32), ("gpu_device", C.c_int32), ("transient_map", C.c_int32),
                ("lm", C.c_int32)]


class Slam2D(_Handle):
    """ctypes view of the host-side lama::Slam2D (include/lama/slam2d.h): online SLAM, one pose + one map pair."""
    _destroy, _last_error, _context = "lama_slam_destroy", "lama_slam_last_error", "lama_slam_device_context"
    _grid_prefix = "lama_slam"

    def __init__(self, **kw):
        self.L = _hostlib()
        o = SlamOptions()
        self.L.lama_slam_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        err = C.create_string_buffer(512)
        h = self.L.lama_slam_create(C.byref(o), err, 512)
        if not h:
            raise LamaError(err.value.decode())
        self.h = C.c_void_p(h)

    def deleted_patches(self):
        return self.L.lama_slam_deleted_patches(self.h)

    def engine_origin(self):
        return self.L.lama_slam_engine_origin(self.h).decode()

    def set_pose(self, x, y, yaw):
        self.L.lama_slam_set_pose(self.h, float(x), float(y), float(yaw))

    def pose(self):
        out = np.zeros(4)
        self.L.lama_slam_get_pose(self.h, _p(out))
        return out

    def update(self, pts, odom_xyr, ts=0.0, origin=None, quat=None):
        pts, origin, quat = self._scan(pts, origin, quat)
        od = np.ascontiguousarray(odom_xyr, dtype=np.float64)
        rc = self.L.lama_slam_update(self.h, _p(pts), len(pts), _p(origin), _p(quat), _p(od), float(ts))
        if rc < 0:
            raise LamaError(self._error())
        return bool(rc)

    def enough_motion(self, odom_xyr):
        return bool(self.L.lama_slam_enough_motion(self.h, _p(np.ascontiguousarray(odom_xyr, dtype=np.float64))))

    def processed_cells(self):
        return self.L.lama_slam_processed_cells(self.h)

    def iterations(self):
        return self.L.lama_slam_iterations(self.h)

    # ---- Slam2D::getOccupancyMap() / getDistanceMap(): host snapshots with the reference's const map API (lama/sdm_maps.h)
    def view_bounds(self, which):
        mn, mx = np.zeros(3, dtype=np.uint32), np.zeros(3, dtype=np.uint32)
        wmn, wmx = np.zeros(3), np.zeros(3)
        if self.L.lama_slam_view_bounds(self.h, int(which), _p(mn), _p(mx), _p(wmn), _p(wmx)) < 0:
            return None
        return mn, mx, wmn, wmx

    def view_cells(self, which):
        n = self.L.lama_slam_view_cells(self.h, int(which), None, 0)
        if n < 0:
            return None
        out = np.zeros((n, 2), dtype=np.uint32)
        self.L.lama_slam_view_cells(self.h, int(which), _p(out), n)
        return out

    def view_occupancy(self, cells_xy):
        c = np.ascontiguousarray(cells_xy, dtype=np.uint32)
        n = len(c)
        fr, oc, un = (np.zeros(n, dtype=np.uint8) for _ in range(3))
        pr = np.zeros(n)
        if self.L.lama_slam_view_occupancy(self.h, n, _p(c), _p(fr), _p(oc), _p(un), _p(pr)) < 0:
            return None
        return fr.astype(bool), oc.astype(bool), un.astype(bool), pr

    def view_cast_rays(self, poses4, pts):
        """the host loop over getOccupancyMap()'s snapshot that castRays replaces (lama_slam_view_cast_rays) -> step (K, n), -1: none"""
        poses4 = np.ascontiguousarray(poses4, dtype=np.float64).reshape(-1, 4)
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        out = np.zeros((len(poses4), len(pts)), dtype=np.int32)
        return out if self.L.lama_slam_view_cast_rays(self.h, _p(poses4), len(poses4), _p(pts), len(pts), _p(out)) >= 0 else None

    def view_distance_cells(self, cells_xy):
        c = np.ascontiguousarray(cells_xy, dtype=np.uint32)
        out = np.zeros(len(c))
        return out if self.L.lama_slam_view_distance_cells(self.h, len(c), _p(c), _p(out)) >= 0 else None

    def view_distance_points(self, pts_xy):
        q = np.ascontiguousarray(pts_xy, dtype=np.float64)
        out = np.zeros((len(q), 3))
        return out if self.L.lama_slam_view_distance_points(self.h, len(q), _p(q), _p(out)) >= 0 else None

    # ---- lama::MatchSurface2D / lama::Solve on Slam2D::getDistanceMap() (include/lama/match_surface_2d.h, nlls/solver.h)
    def match_eval(self, pts, pose4, origin=None, quat=None, jac=True):
        pts, origin, quat = self._scan(pts, origin, quat)
        n = len(pts)
        r, J, rmse = np.zeros(n), (np.zeros((3, n)) if jac else None), C.c_double(0)
        rc = self.L.lama_slam_match_eval(self.h, _p(pts), n, _p(origin), _p(quat), _p(np.ascontiguousarray(pose4, dtype=np.float64)),
                                         _p(r), _p(J), C.byref(rmse))
        if rc < 0:
            raise LamaError(self._error())
        return r, (J.T.copy() if jac else None), rmse.value

    def match_solve(self, pts, pose4, strategy="gn", weight="cauchy", weight_param=0.15, max_iterations=100, origin=None, quat=None):
        pts, origin, quat = self._scan(pts, origin, quat)
        pose = np.array(pose4, dtype=np.float64)
        cov, it = np.zeros(9), C.c_uint32(0)
        rc = self.L.lama_slam_match_solve(self.h, _p(pts), len(pts), _p(origin), _p(quat), _p(pose), strategy.encode(), weight.encode(),
                                          float(weight_param), int(max_iterations), _p(cov), C.byref(it))
        if rc < 0:
            raise LamaError(self._error())
        return pose, cov.reshape(3, 3), it.value

    def match_solve_generic(self, pts, pose4, strategy="gn", weight="cauchy", weight_param=0.15, max_iterations=100, origin=None, quat=None):
        """The same problem through lama::Solver's generic host loop (per-beam evaluation on the device, everything else on the
        host): any of "unit", "tukey", "tdist", "cauchy", "huber" -> (pose, covariance, iterations)"""
        pts, origin, quat = self._scan(pts, origin, quat)
        pose = np.array(pose4, dtype=np.float64)
        cov, it = np.zeros(9), C.c_uint32(0)
        rc = self.L.lama_slam_match_solve_generic(self.h, _p(pts), len(pts), _p(origin), _p(quat), _p(pose), strategy.encode(), weight.encode(),
                                                  float(weight_param), int(max_iterations), _p(cov), C.byref(it))
        if rc < 0:
            raise LamaError(self._error())
        return pose, cov.reshape(3, 3), it.value

    def solve_batch(self, scans, poses4, strategy="gn", weight="huber", weight_param=0.15, max_iterations=None, origins=None, quats=None,
                    other=None, eps1=0.0):
        """lama::SolveBatch over MatchSurface2D problems on getDistanceMap() (odd problems on `other`'s map when given)
        -> (poses (B, 4), covariances (B, 3, 3), iterations (B,), errors (B,))"""
        pts, offs = pack_scans(scans)
        B = len(offs) - 1
        poses = np.array(poses4, dtype=np.float64).reshape(B, 4)
        mi = None if max_iterations is None else np.ascontiguousarray(np.broadcast_to(np.asarray(max_iterations, dtype=np.uint32), (B,)))
        origins = None if origins is None else np.ascontiguousarray(origins, dtype=np.float64).reshape(B, 3)
        quats = None if quats is None else np.ascontiguousarray(quats, dtype=np.float64).reshape(B, 4)
        cov, it, err = np.zeros((B, 9)), np.zeros(B, dtype=np.uint32), np.zeros(B)
        rc = self.L.lama_slam_solve_batch(self.h, other.h if other is not None else None, B, _p(pts), _p(offs), _p(origins), _p(quats), _p(poses),
                                          _p(mi), strategy.encode(), float(eps1), weight.encode(), float(weight_param), _p(cov), _p(it), _p(err))
        if rc < 0:
            raise LamaError(self._error())
        return poses, cov.reshape(B, 3, 3), it, err

    def correlative_search(self, pts, box_min, box_max, linear_step=0.2, angular_step=math.radians(5.0), point_step=0, tile=8, max_candidates=16,
                           refine=True, refine_iterations=100, origin=None, quat=None):
        """lama::CorrelativeSearch2D::search on getDistanceMap() over the box -> (dict of the candidates' arrays, sorted by rmse:
        coarse (B, 4), score (B,), pose (B, 4), rmse (B,), iterations (B,); dict of the lattice: cell_step, nx, ny, headings,
        point_step, tile)"""
        pts, origin, quat = self._scan(pts, origin, quat)
        box = np.array([box_min[0], box_min[1], box_max[0], box_max[1]], dtype=np.float64)
        cap = int(max_candidates)
        coarse, poses = np.zeros((cap, 4)), np.zeros((cap, 4))
        score, it, rmse = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32), np.zeros(cap)
        lat, num = np.zeros(6, dtype=np.uint32), C.c_uint32(0)
        rc = self.L.lama_slam_correlative_search(self.h, _p(pts), len(pts), _p(origin), _p(quat), _p(box), float(linear_step), float(angular_step),
                                                 int(point_step), int(tile), cap, 1 if refine else 0, int(refine_iterations), cap, _p(coarse), _p(score),
                                                 _p(poses), _p(rmse), _p(it), _p(lat), C.byref(num))
        if rc < 0:
            raise LamaError(self._error())
        B = min(num.value, cap)
        return (dict(coarse=coarse[:B], score=score[:B], pose=poses[:B], rmse=rmse[:B], iterations=it[:B]),
                dict(zip(("cell_step", "nx", "ny", "headings", "point_step", "tile"), (int(v) for v in lat))))


class Loc2D(_Handle):
    """ctypes view of the host-side lama::Loc2D (include/lama/loc2d.h): localisation on a fixed distance map."""
    _destroy, _last_error, _context = "lama_loc_destroy", "lama_loc_last_error", "lama_loc_device_context"
    _grid_prefix = "lama_loc"

    def occupancy_grid(self, *a, **kw):
        raise LamaError("lama::Loc2D has no device occupancy map: occupancy_map is a host map (distance_grid() is available)")

    def frontiers(self, *a, **kw):
        raise LamaError("lama::Loc2D has no device occupancy map: occupancy_map is a host map, frontiers are made from a device map")

    def check_scan(self, pts, origin=None, quat=None, tolerance_cells=2):
        """Loc2D::checkScan: one label per point at the current pose on the distance map (RAY_AGREES: it ends within
        tolerance_cells of a mapped obstacle; RAY_BLOCKED: it passes through one; RAY_NOVEL: it ends where the map has
        nothing) -> uint8 (n,), or None while there is no device map."""
        pts, origin, quat = self._scan(pts, origin, quat)
        out = np.zeros(len(pts), dtype=np.uint8)
        n = self.L.lama_loc_check_scan(self.h, _p(pts), len(pts), _p(origin), _p(quat), int(tolerance_cells), _p(out))
        if n < 0:
            raise LamaError(self._error())
        return out if n else None

    def __init__(self, trans_thresh=0.5, rot_thresh=0.5, l2_max=1.0, resolution=0.05, max_iter=100, gpu_device=0,
                 gloc_particles=3000, gloc_iters=10, gloc_thresh=0.15, cov_blend=0.0, strategy="gn"):
        self.L = _hostlib()
        err = C.create_string_buffer(512)
        h = self.L.lama_loc_create3(trans_thresh, rot_thresh, l2_max, resolution, max_iter, gloc_particles, gloc_iters,
                                    gloc_thresh, cov_blend, strategy.encode(), gpu_device, err, 512)
        if not h:
            raise LamaError(err.value.decode())
        self.h = C.c_void_p(h)

    def engine_origin(self):
        return self.L.lama_loc_engine_origin(self.h).decode()

    def set_obstacles_world(self, xy):
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        self._chk(self.L.lama_loc_set_obstacles_world(self.h, _p(xy), len(xy)))

    def write_distance_map(self, filename):
        self._chk(self.L.lama_loc_write_distance_map(self.h, str(filename).encode()))

    def read_distance_map(self, filename):
        """distance_map->read(file): the file's patches replace the device map (no addObstacle / update() replay)."""
        self._chk(self.L.lama_loc_read_distance_map(self.h, str(filename).encode()))

    def set_pose(self, x, y, yaw):
        self.L.lama_loc_set_pose(self.h, float(x), float(y), float(yaw))

    def pose(self):
        out = np.zeros(4)
        self.L.lama_loc_get_pose(self.h, _p(out))
        return out

    def update(self, pts, odom_xyr, ts=0.0, force=False, origin=None, quat=None):
        pts, origin, quat = self._scan(pts, origin, quat)
        od = np.ascontiguousarray(odom_xyr, dtype=np.float64)
        return bool(self._chk(self.L.lama_loc_update(self.h, _p(pts), len(pts), _p(origin), _p(quat), _p(od), float(ts), 1 if force else 0)))

    def covar(self):
        out = np.zeros(9)
        self.L.lama_loc_covar(self.h, _p(out))
        return out.reshape(3, 3)

    def rmse(self):
        return self.L.lama_loc_rmse(self.h)

    def iterations(self):
        return self.L.lama_loc_iterations(self.h)

    # ---- global localisation / sampling covariance (src/loc2d.cpp:194-286)
    def occ_set_cells(self, cells_xy, state):
        """occupancy_map->setFree (-1) / setUnknown (0) / setOccupied (1) on map cells."""
        cells = np.ascontiguousarray(cells_xy, dtype=np.uint32).reshape(-1, 2)
        self._chk(self.L.lama_loc_occ_set_cells(self.h, _p(cells), len(cells), int(state)))

    def occ_bounds(self):
        out = np.zeros(6)
        self.L.lama_loc_occ_bounds(self.h, _p(out))
        return out[:3].copy(), out[3:].copy()

    def trigger_global_localization(self):
        self.L.lama_loc_trigger_global_localization(self.h)

    def global_localization_active(self):
        return bool(self.L.lama_loc_global_localization_active(self.h))

    def relocalize(self, pts, linear_step=0.2, angular_step=math.radians(5.0), point_step=0, tile=8, max_candidates=16, refine_iterations=100,
                   origin=None, quat=None):
        """Loc2D::relocalize: lattice search over the occupancy map's bounds, free nodes only -> True when the pose was set"""
        pts, origin, quat = self._scan(pts, origin, quat)
        return bool(self._chk(self.L.lama_loc_relocalize(self.h, _p(pts), len(pts), _p(origin), _p(quat), float(linear_step), float(angular_step),
                                                         int(point_step), int(tile), int(max_candidates), int(refine_iterations))))

    def relocalize_candidates(self):
        """the candidates of the last relocalize(), best first: dict of coarse (B, 4), score, pose (B, 4), rmse, iterations"""
        B = self.L.lama_loc_relocalize_candidates(self.h, 0, None, None, None, None, None)
        coarse, poses = np.zeros((B, 4)), np.zeros((B, 4))
        score, it, rmse = np.zeros(B, dtype=np.uint32), np.zeros(B, dtype=np.uint32), np.zeros(B)
        if B:
            self.L.lama_loc_relocalize_candidates(self.h, B, _p(coarse), _p(score), _p(poses), _p(rmse), _p(it))
        return dict(coarse=coarse, score=score, pose=poses, rmse=rmse, iterations=it)

    def gloc_candidates(self):
        n = self.L.lama_loc_gloc_candidates(self.h, None, None, 0)
        poses, err = np.zeros((n, 4)), np.zeros(n)
        if n:
            self.L.lama_loc_gloc_candidates(self.h, _p(poses), _p(err), n)
        return poses, err

    def sampling_likelihoods(self):
        n = self.L.lama_loc_sampling_likelihoods(self.h, None, 0)
        out = np.zeros(n)
        if n:
            self.L.lama_loc_sampling_likelihoods(self.h, _p(out), n)
        return out


def random_set_seed(seed):
    """lama::random::setSeed (process-wide generator used by Loc2D::globalLocalization)."""
    _hostlib().lama_random_set_seed(int(seed))


# ---------------------------------------------------------------------------------------------------------------
# lama::sdm map formats (include/lama/sdm_io.h) on downloaded maps: {patch id: (cells, mask)} as HipContext.download_map returns
# ---------------------------------------------------------------------------------------------------------------
SDM_CELL_BYTES = {MAP_DISTANCE: 10, MAP_OCCUPANCY: 4, 2: 1, 3: 4}      # 3 = ProbabilisticOccupancyMap (float log-odds)


def _sdm_arrays(patches, kind):
    ids = np.array(sorted(patches), dtype=np.uint64)
    cb = SDM_CELL_BYTES[kind] * 1024
    cells = np.zeros((len(ids), cb), dtype=np.uint8)
    masks = np.zeros((len(ids), 16), dtype=np.uint64)
    for k, i in enumerate(ids):
        c, m = patches[int(i)]
        cells[k] = np.ascontiguousarray(c).view(np.uint8).reshape(-1)
        masks[k] = m
    return ids, cells, masks


def sdm_write(filename, patches, kind, resolution=0.05, max_sqdist=100):
    ids, cells, masks = _sdm_arrays(patches, kind)
    if _hostlib().lama_sdm_write(filename.encode(), kind, resolution, max_sqdist, len(ids), _p(ids), _p(cells), _p(masks)) != 0:
        raise LamaError(f"cannot write {filename}")


def sdm_read(filename):
    """-> (kind, resolution, max_sqdist, {patch id: (cells bytes, mask)})"""
    L = _hostlib()
    kind, n, msq, res = C.c_int32(0), C.c_uint32(0), C.c_uint32(0), C.c_double(0)
    if L.lama_sdm_read(filename.encode(), C.byref(kind), C.byref(res), C.byref(msq), 0, None, None, None, C.byref(n)) != 0:
        raise LamaError(f"cannot read {filename}")
    cb = SDM_CELL_BYTES[kind.value] * 1024
    ids = np.zeros(n.value, dtype=np.uint64)
    cells = np.zeros((n.value, cb), dtype=np.uint8)
    masks = np.zeros((n.value, 16), dtype=np.uint64)
    L.lama_sdm_read(filename.encode(), None, None, None, n.value, _p(ids), _p(cells), _p(masks), None)
    return kind.value, res.value, msq.value, {int(ids[k]): (cells[k], masks[k]) for k in range(n.value)}


def dm_build(cells_xy, max_sqdist):
    """The first build of Loc2D's distance map as the host facade does it (iris_lama_amd/host/dm_builder.hpp): addObstacle for the
    cells in order on an empty map + one update().  -> (cells processed, {patch id: (distance_t[1024] structured, mask[16])}),
    or None when the host does not build it (the facade then uses the device chain)."""
    L = _hostlib()
    cells_xy = np.ascontiguousarray(cells_xy, dtype=np.uint32)
    done = C.c_uint32(0)
    n = L.lama_dm_build(_p(cells_xy), len(cells_xy), int(max_sqdist), C.byref(done))
    if n < 0:
        return None
    ids = np.zeros(n, dtype=np.uint64)
    cells = np.zeros((n, 10240), dtype=np.uint8)
    masks = np.zeros((n, 16), dtype=np.uint64)
    if n:
        L.lama_dm_build_fetch(_p(ids), _p(cells), _p(masks))
    dist_t = np.dtype([("obstacle", "<i2", (3,)), ("sqdist", "<u2"), ("valid", "u1"), ("queued", "u1")])
    return done.value, {int(ids[k]): (cells[k].view(dist_t), masks[k]) for k in range(n)}


def sdm_image(patches, kind, resolution=0.05, max_sqdist=100):
    ids, cells, masks = _sdm_arrays(patches, kind)
    w, h = C.c_uint32(0), C.c_uint32(0)
    L = _hostlib()
    L.lama_sdm_image(kind, resolution, max_sqdist, len(ids), _p(ids), _p(cells), _p(masks), C.byref(w), C.byref(h), None, 0)
    out = np.zeros((h.value, w.value), dtype=np.uint8)
    L.lama_sdm_image(kind, resolution, max_sqdist, len(ids), _p(ids), _p(cells), _p(masks), C.byref(w), C.byref(h), _p(out), out.size)
    return out


def sdm_export_png(filename, patches, kind, resolution=0.05, max_sqdist=100):
    ids, cells, masks = _sdm_arrays(patches, kind)
    if _hostlib().lama_sdm_export_png(kind, resolution, max_sqdist, len(ids), _p(ids), _p(cells), _p(masks), filename.encode()) != 0:
        raise LamaError(f"cannot write {filename}")


# ---------------------------------------------------------------------------------------------------------------
# SE2 pose-graph linearisation on the device (include/lama_hip.h, lama_hip_pgo_*)
# ---------------------------------------------------------------------------------------------------------------
class PoseGraph:
    """Factors: fi, fj (fj = -1: prior on fi), meas [F,4] = {c, s, tx, ty}, sqrt_info [F,3] (DiagonalLoss: 1 / sigma).
    loss_kind [F] (PGO_LOSS_*) and loss_param [F]: a robust loss per factor, applied after the whitening
    (lama_hip_pgo_create_robust); both None: lama_hip_pgo_create."""

    def __init__(self, num_poses, fi, fj, meas, sqrt_info, device=0, loss_kind=None, loss_param=None):
        self.L = hip_lib()
        self.N = int(num_poses)
        self.fi = np.ascontiguousarray(fi, dtype=np.int32)
        self.fj = np.ascontiguousarray(fj, dtype=np.int32)
        self.meas = np.ascontiguousarray(meas, dtype=np.float64).reshape(-1, 4)
        self.sqrt_info = np.ascontiguousarray(sqrt_info, dtype=np.float64).reshape(-1, 3)
        self.F = len(self.fi)
        h = C.c_void_p()
        if loss_kind is None and loss_param is None:
            rc = self.L.lama_hip_pgo_create(device, self.N, _p(self.fi), _p(self.fj), _p(self.meas), _p(self.sqrt_info), self.F, C.byref(h))
        else:
            self.loss_kind = None if loss_kind is None else np.ascontiguousarray(loss_kind, dtype=np.int32)
            self.loss_param = None if loss_param is None else np.ascontiguousarray(loss_param, dtype=np.float64)
            for a in (self.loss_kind, self.loss_param):
                if a is not None and a.shape != (self.F,):
                    raise ValueError(f"loss_kind / loss_param must have one entry per factor ({self.F}), not shape {a.shape}")
            rc = self.L.lama_hip_pgo_create_robust(device, self.N, _p(self.fi), _p(self.fj), _p(self.meas), _p(self.sqrt_info),
                                                   _p(self.loss_kind), _p(self.loss_param), self.F, C.byref(h))
            why = self.L.lama_hip_pgo_last_error(None).decode()
            if rc != 0 and why != "null handle":
                raise LamaError(why)
        if rc != 0 or not h:
            raise LamaError(f"lama_hip_pgo_create failed (status {rc}): no usable MI355X / HIP device or invalid graph; there is no CPU fallback")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.lama_hip_pgo_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def linearize(self, poses, want_err=True, want_off=True):
        """-> dict(err [F,3], Hdiag [N,3,3], Hoff [F,3,3], b [N,3], chi2, kernel_ms)"""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(self.N, 4)
        err = np.zeros((self.F, 3)) if want_err else None
        hoff = np.zeros((self.F, 3, 3)) if want_off else None
        hd, b = np.zeros((self.N, 3, 3)), np.zeros((self.N, 3))
        chi2, ms = C.c_double(0), C.c_double(0)
        rc = self.L.lama_hip_pgo_linearize(self.h, _p(poses), _p(err), _p(hd), _p(hoff), _p(b), C.byref(chi2), C.byref(ms))
        if rc != 0:
            raise LamaError(self.L.lama_hip_pgo_last_error(self.h).decode())
        return {"err": err, "Hdiag": hd, "Hoff": hoff, "b": b, "chi2": chi2.value, "kernel_ms": ms.value}

    def _check(self, rc):
        if rc != 0:
            raise LamaError(self.L.lama_hip_pgo_last_error(self.h).decode())

    def pattern(self):
        """-> (row_ptr [N+1], cols [nnzb]): the lower block-CSR pattern of the Hessian (diagonal block first in each row)."""
        n = C.c_uint32(0)
        self._check(self.L.lama_hip_pgo_pattern(self.h, None, None, C.byref(n)))
        row_ptr, cols = np.zeros(self.N + 1, dtype=np.int32), np.zeros(n.value, dtype=np.int32)
        self._check(self.L.lama_hip_pgo_pattern(self.h, _p(row_ptr), _p(cols), C.byref(n)))
        return row_ptr, cols

    def set_poses(self, poses):
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(self.N, 4)
        self._check(self.L.lama_hip_pgo_set_poses(self.h, _p(poses)))

    def get_poses(self):
        out = np.zeros((self.N, 4))
        self._check(self.L.lama_hip_pgo_get_poses(self.h, _p(out)))
        return out

    def linearize_system(self):
        """At the current poses -> dict(blocks [nnzb,3,3], b [N,3], diag [N,3], half_chi2, kernel_ms)"""
        nnzb = C.c_uint32(0)
        self._check(self.L.lama_hip_pgo_pattern(self.h, None, None, C.byref(nnzb)))
        blocks, b, diag = np.zeros((nnzb.value, 3, 3)), np.zeros((self.N, 3)), np.zeros((self.N, 3))
        half, ms = C.c_double(0), C.c_double(0)
        self._check(self.L.lama_hip_pgo_linearize_system(self.h, _p(blocks), _p(b), _p(diag), C.byref(half), C.byref(ms)))
        return {"blocks": blocks, "b": b, "diag": diag, "half_chi2": half.value, "kernel_ms": ms.value}

    def try_step(self, dx):
        """Candidate = current * exp(dx) per pose -> (0.5 * chi2 at the candidate, kernel_ms)."""
        dx = np.ascontiguousarray(dx, dtype=np.float64).reshape(self.N, 3)
        half, ms = C.c_double(0), C.c_double(0)
        self._check(self.L.lama_hip_pgo_try_step(self.h, _p(dx), C.byref(half), C.byref(ms)))
        return half.value, ms.value

    def accept(self):
        """The candidate of the last try_step becomes the current state; LamaError when none is pending."""
        self._check(self.L.lama_hip_pgo_accept(self.h))

    def factor_weights(self):
        """-> w [F] of every factor's loss in the last linearize / linearize_system (1 without a loss); LamaError before the first."""
        w = np.zeros(self.F)
        self._check(self.L.lama_hip_pgo_factor_weights(self.h, _p(w)))
        return w

    def solve_pcg(self, lam, rel_tol=1e-10, max_iterations=None, batch=0, want_dx=True):
        """(H + lam diag(H)) dx = b of the last linearize_system, solved on the device by block-Jacobi PCG (lama_hip_pgo_solve_pcg).
        max_iterations None: max(100, 6 N).  -> dict(dx [N,3] or None, iterations, rel_residual_sq, outcome (PCG_CONVERGED / PCG_CAP /
        PCG_BREAKDOWN), model_decrease, kernel_ms); the solution stays on the device for try_solved_step."""
        dx = np.zeros((self.N, 3)) if want_dx else None
        it, oc = C.c_uint32(0), C.c_int32(-1)
        rel, model, ms = C.c_double(0), C.c_double(0), C.c_double(0)
        cap = max(100, 6 * self.N) if max_iterations is None else int(max_iterations)
        self._check(self.L.lama_hip_pgo_solve_pcg(self.h, float(lam), float(rel_tol), cap, int(batch), _p(dx), C.byref(it), C.byref(rel),
                                                  C.byref(oc), C.byref(model), C.byref(ms)))
        return {"dx": dx, "iterations": it.value, "rel_residual_sq": rel.value, "outcome": oc.value, "model_decrease": model.value,
                "kernel_ms": ms.value}

    def try_solved_step(self):
        """try_step with the solution solve_pcg left on the device -> (0.5 * chi2 at the candidate, kernel_ms)."""
        half, ms = C.c_double(0), C.c_double(0)
        self._check(self.L.lama_hip_pgo_try_solved_step(self.h, C.byref(half), C.byref(ms)))
        return half.value, ms.value


PCG_CONVERGED, PCG_CAP, PCG_BREAKDOWN = 0, 1, 2          # include/lama_hip.h, LAMA_HIP_PCG_*
PGO_LOSS_NONE, PGO_LOSS_HUBER, PGO_LOSS_CAUCHY, PGO_LOSS_DCS = 0, 1, 2, 3      # include/lama_hip.h, LAMA_HIP_PGO_LOSS_*
PGO_LOSSES = {None: PGO_LOSS_NONE, "none": PGO_LOSS_NONE, "huber": PGO_LOSS_HUBER, "cauchy": PGO_LOSS_CAUCHY, "dcs": PGO_LOSS_DCS}


class PgoReport(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_uint32), ("tries", C.c_uint32),
                ("initial_error", C.c_double), ("final_error", C.c_double), ("nnz_L", C.c_uint64),
                ("ms_device_linearize", C.c_double), ("ms_device_try", C.c_double), ("ms_analyze", C.c_double),
                ("ms_factorize", C.c_double), ("ms_total", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class PgoOptions(C.Structure):
    """lama_pgo_options (include/lama_host.h)"""
    _fields_ = [("struct_bytes", C.c_uint32), ("device", C.c_int32), ("linear_solver", C.c_int32), ("pcg_max_iterations", C.c_uint32),
                ("pcg_rel_tol", C.c_double)]


class PgoReport2(C.Structure):
    """lama_pgo_report2 (include/lama_host.h): lama_pgo_report behind its own size, then the device solver's counters"""
    _fields_ = [("struct_bytes", C.c_uint32), ("status", C.c_int32), ("iterations", C.c_uint32), ("tries", C.c_uint32),
                ("initial_error", C.c_double), ("final_error", C.c_double), ("nnz_L", C.c_uint64),
                ("ms_device_linearize", C.c_double), ("ms_device_try", C.c_double), ("ms_analyze", C.c_double),
                ("ms_factorize", C.c_double), ("ms_total", C.c_double),
                ("pcg_iterations", C.c_uint64), ("pcg_max_iterations_seen", C.c_uint32), ("pcg_fallbacks", C.c_uint32),
                ("ms_device_solve", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "struct_bytes"}


PGO_SOLVERS = {"ldlt": 0, "pcg": 1}                      # lama::SimplePGO::LinearSolver
PGO_STATUS = {0: "SUCCESS", 1: "MAX_ITERATION", 2: "ERROR_INCREASE", 3: "RANK_DEFICIENCY", 4: "INVALID", -1: "NOT_RUN"}


def simple_pgo(nodes, edges=(), fixed=(), device=0, solver=None, pcg_rel_tol=1e-10, pcg_max_iterations=0):
    """lama::SimplePGO::optimize (include/lama/simple_pgo.h) on the device.  nodes [n,4] {c, s, tx, ty} (node_list); edges: iterable of
    (from, to, pose4) (edge_list); fixed: iterable of (index, pose4) (fixed_list).  solver: "ldlt" (the default: the sparse LDL^T on
    the host) or "pcg" (the damped system solved on the device, lama_hip_pgo_solve_pcg; pcg_max_iterations 0: max(100, 6 n)).
    -> (ok, poses [n,4], report dict with the try trace under "trace": 1 accepted, 0 rejected, 2 rank deficient; with "pcg" also
    pcg_iterations, pcg_max_iterations_seen, pcg_fallbacks and ms_device_solve)."""
    nodes = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1, 4)
    n = len(nodes)
    edges, fixed = list(edges), list(fixed)
    ef = np.array([e[0] for e in edges], dtype=np.int32)
    et = np.array([e[1] for e in edges], dtype=np.int32)
    e4 = np.ascontiguousarray(np.array([e[2] for e in edges], dtype=np.float64).reshape(-1, 4))
    fx = np.array([f[0] for f in fixed], dtype=np.int32)
    f4 = np.ascontiguousarray(np.array([f[1] for f in fixed], dtype=np.float64).reshape(-1, 4))
    out = np.zeros((n, 4))
    cap = 1 << 16
    trace = np.zeros(cap, dtype=np.int8)
    err = C.create_string_buffer(512)
    if solver is None or solver == "ldlt":
        rep = PgoReport()
        rc = _hostlib().lama_pgo_optimize(_p(nodes) if n else None, n, _p(ef), _p(et), _p(e4), len(edges), _p(fx), _p(f4), len(fixed),
                                         device, _p(out) if n else None, C.byref(rep), _p(trace), cap, err, 512)
    else:
        if solver not in PGO_SOLVERS:
            raise ValueError(f"solver must be one of {sorted(PGO_SOLVERS)}, not {solver!r}")
        opt = PgoOptions(C.sizeof(PgoOptions), device, PGO_SOLVERS[solver], int(pcg_max_iterations), float(pcg_rel_tol))
        rep = PgoReport2()
        rep.struct_bytes = C.sizeof(PgoReport2)
        rc = _hostlib().lama_pgo_optimize_with(_p(nodes) if n else None, n, _p(ef), _p(et), _p(e4), len(edges), _p(fx), _p(f4), len(fixed),
                                              C.byref(opt), _p(out) if n else None, C.byref(rep), _p(trace), cap, err, 512)
    if rc < 0:
        raise LamaError(err.value.decode())
    r = rep.as_dict()
    r["status_name"] = PGO_STATUS.get(r["status"], str(r["status"]))
    r["trace"] = trace[:min(rep.tries, cap)].copy()
    return rc == 1, out, r


def pose_graph_optimize(nodes, factors, device=0, solver=None, pcg_rel_tol=1e-10, pcg_max_iterations=0):
    """lama::PoseGraph2D::optimize (include/lama/pose_graph_2d.h) on the device.  nodes [n,4] {c, s, tx, ty}; factors: iterable of
    (from, to, pose4, sigmas3) or (from, to, pose4, sigmas3, loss) with to = -1 for a prior on `from` and loss None or a pair
    (name, parameter), name one of "huber", "cauchy", "dcs".  solver, pcg_*: as simple_pgo.
    -> (ok, poses [n,4], report dict as simple_pgo's with "pcg", plus "weights" [F]: every factor's loss weight at the state the
    run ended in; empty when the graph was refused, status -1)."""
    nodes = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1, 4)
    n = len(nodes)
    factors = list(factors)
    nf = len(factors)
    fi = np.array([f[0] for f in factors], dtype=np.int32)
    fj = np.array([f[1] for f in factors], dtype=np.int32)
    m4 = np.ascontiguousarray(np.array([f[2] for f in factors], dtype=np.float64).reshape(-1, 4))
    s3 = np.ascontiguousarray(np.array([f[3] for f in factors], dtype=np.float64).reshape(-1, 3))
    losses = [f[4] if len(f) > 4 and f[4] is not None else (None, 0.0) for f in factors]
    for name, _ in losses:
        if name not in PGO_LOSSES:
            raise ValueError(f"loss must be None or (name, parameter) with name one of 'huber', 'cauchy', 'dcs', not {name!r}")
    kind = np.array([PGO_LOSSES[l[0]] for l in losses], dtype=np.int32)
    param = np.array([l[1] for l in losses], dtype=np.float64)
    if (solver or "ldlt") not in PGO_SOLVERS:
        raise ValueError(f"solver must be one of {sorted(PGO_SOLVERS)}, not {solver!r}")
    opt = PgoOptions(C.sizeof(PgoOptions), device, PGO_SOLVERS[solver or "ldlt"], int(pcg_max_iterations), float(pcg_rel_tol))
    rep = PgoReport2()
    rep.struct_bytes = C.sizeof(PgoReport2)
    out, weights = np.zeros((n, 4)), np.ones(nf)
    cap = 1 << 16
    trace = np.zeros(cap, dtype=np.int8)
    err = C.create_string_buffer(512)
    rc = _hostlib().lama_pose_graph_optimize(_p(nodes) if n else None, n, _p(fi), _p(fj), _p(m4), _p(s3), _p(kind), _p(param), nf, C.byref(opt),
                                            _p(out) if n else None, _p(weights), C.byref(rep), _p(trace), cap, err, 512)
    if rc < 0:
        raise LamaError(err.value.decode())
    r = rep.as_dict()
    r["status_name"] = PGO_STATUS.get(r["status"], str(r["status"]))
    r["trace"] = trace[:min(rep.tries, cap)].copy()
    r["weights"] = weights if r["status"] != -1 else np.zeros(0)
    return rc == 1, out, r


class LidarOdometry2D(_Handle):
    """ctypes view of the host-side lama::LidarOdometry2D (include/lama/lidar_odometry_2d.h)."""
    _destroy, _last_error, _context = "lama_lo_destroy", "lama_lo_last_error", "lama_lo_device_context"
    _grid_prefix = "lama_lo"

    def __init__(self, resolution=0.05, max_iter=100, gpu_device=0):
        self.L = _hostlib()
        err = C.create_string_buffer(512)
        h = self.L.lama_lo_create(resolution, max_iter, gpu_device, err, 512)
        if not h:
            raise LamaError(err.value.decode())
        self.h = C.c_void_p(h)

    def engine_origin(self):
        return self.L.lama_lo_engine_origin(self.h).decode()

    def update(self, pts, ts=0.0, origin=None, quat=None):
        pts, origin, quat = self._scan(pts, origin, quat)
        return bool(self._chk(self.L.lama_lo_update(self.h, _p(pts), len(pts), _p(origin), _p(quat), float(ts))))

    def odom(self):
        out = np.zeros(4)
        self.L.lama_lo_get_odom(self.h, _p(out))
        return out

    def iterations(self):
        return self.L.lama_lo_iterations(self.h)

    def deleted_patches(self):
        return self.L.lama_lo_deleted_patches(self.h)


class MapBuilderOptions(C.Structure):
    _fields_ = [("resolution", C.c_double), ("l2_max", C.c_double), ("patch_size", C.c_uint32), ("full", C.c_int32), ("prune", C.c_int32),
                ("gpu_device", C.c_int32), ("window_patches", C.c_uint32), ("occ_patch_capacity", C.c_uint32), ("dm_patch_capacity", C.c_uint32)]


class MapBuilder2D(_Handle):
    """ctypes view of the host-side lama::MapBuilder2D (include/lama/map_builder_2d.h): a map rebuilt from posed key scans."""
    _destroy, _last_error, _context = "lama_mapbuilder_destroy", "lama_mapbuilder_last_error", "lama_mapbuilder_device_context"
    _grid_prefix = "lama_mapbuilder"

    def __init__(self, **kw):
        self.L = _hostlib()
        o = MapBuilderOptions()
        self.L.lama_mapbuilder_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        err = C.create_string_buffer(512)
        h = self.L.lama_mapbuilder_create(C.byref(o), err, 512)
        if not h:
            raise LamaError(err.value.decode())
        self.h = C.c_void_p(h)

    def engine_origin(self):
        return self.L.lama_mapbuilder_engine_origin(self.h).decode()

    def add(self, pts, pose4, origin=None, quat=None):
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        origin = np.ascontiguousarray(origin if origin is not None else _Z3, dtype=np.float64)
        quat = np.ascontiguousarray(quat if quat is not None else _IDQ, dtype=np.float64)
        pose4 = np.ascontiguousarray(pose4, dtype=np.float64)
        return self._chk(self.L.lama_mapbuilder_add(self.h, _p(pts), len(pts), _p(origin), _p(quat), _p(pose4)))

    def set_pose(self, key, pose4):
        self._chk(self.L.lama_mapbuilder_set_pose(self.h, int(key), _p(np.ascontiguousarray(pose4, dtype=np.float64))))

    def set_poses(self, poses4):
        poses4 = np.ascontiguousarray(poses4, dtype=np.float64).reshape(-1, 4)
        self._chk(self.L.lama_mapbuilder_set_poses(self.h, _p(poses4), len(poses4)))

    def build(self):
        self._chk(self.L.lama_mapbuilder_build(self.h))

    def reset(self):
        self._chk(self.L.lama_mapbuilder_reset(self.h))

    def occupied_cells(self):
        n = self.L.lama_mapbuilder_occupied_cells(self.h, None, 0)
        out = np.zeros((n, 2), dtype=np.uint32)
        self.L.lama_mapbuilder_occupied_cells(self.h, _p(out), n)
        return out

    def timing(self):
        """wall-clock milliseconds of the last build(): integrate, occupied list, distance map"""
        ms = np.zeros(3)
        self.L.lama_mapbuilder_timing(self.h, _p(ms))
        return {"integrate_ms": ms[0], "occupied_ms": ms[1], "distance_ms": ms[2]}

    def view_cells(self, which):
        """visit_all_cells of getOccupancyMap() (0) / getDistanceMap() (1), or None when there is no such map"""
        n = self.L.lama_mapbuilder_view_cells(self.h, which, None, 0)
        if n < 0:
            return None
        out = np.zeros((n, 2), dtype=np.uint32)
        self._chk(self.L.lama_mapbuilder_view_cells(self.h, which, _p(out), n))
        return out

    def match_solve(self, pts, pose4, max_iterations=100, origin=None, quat=None):
        """lama::Solve(GaussNewton + Cauchy(0.15)) of MatchSurface2D on getDistanceMap() -> (pose4, iterations)"""
        pts, origin, quat = self._scan(pts, origin, quat)
        pose = np.ascontiguousarray(pose4, dtype=np.float64).copy()
        it = C.c_uint32(0)
        rc = self.L.lama_mapbuilder_match_solve(self.h, _p(pts), len(pts), _p(origin), _p(quat), _p(pose), int(max_iterations), C.byref(it))
        if rc != 0:
            raise LamaError(self._error() or "no distance map")
        return pose, it.value
