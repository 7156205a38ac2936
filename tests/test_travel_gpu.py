"""lama_hip_map_travel (iris_lama_amd/csrc/lama_travel.h) on the device, and planRoutes of the host classes over it.  The cases are
in tests/_travel_checks.py, the expected fields, routes and paths in tests/_travel.py (numpy / heapq, from download_map)."""
import math

import numpy as np
import pytest

import _travel as TR
import _travel_checks as TC
import iris_lama_amd.ffi as F

pytestmark = pytest.mark.gpu


@pytest.fixture()
def Fwide():
    """the module bound to the wide build (a 4-byte distance plane) in place of the default one"""
    saved = F.HIP_LIB, F._hip
    F.HIP_LIB, F._hip = F.HIP_LIB_WIDE, None
    yield F
    F.HIP_LIB, F._hip = saved


def test_open_floor_in_one_tile():
    TC.check_open_floor(F)


def test_the_move_rules():
    TC.check_move_rules(F)


def test_clearance_and_preference_from_the_distance_layer():
    TC.check_clearance_and_preference(F)


def test_clearance_and_preference_in_the_wide_build(Fwide):
    TC.check_clearance_and_preference(Fwide)


def test_tiles():
    TC.check_tiles(F)


def test_many_sources():
    TC.check_many_sources(F)


def test_goals():
    TC.check_goals(F)


def test_strides_and_boxes_beside_and_beyond_the_map():
    TC.check_strides_and_boxes(F)


def test_refusals_leave_every_output_untouched():
    TC.check_refusals(F)


def test_a_map_without_patches():
    TC.check_empty_map(F)


def test_random_pictures():
    TC.check_random_pictures(F)


OPTS = dict(robot_radius=0.1, preferred_clearance=0.3, near_factor=3, goal_reach=2, max_path_points=16)


def _open_spot(obj, stride=1, **kw):
    """a place for the robot to stand, in world metres: the centre of the first pixel of the largest 4-connected region the robot of
    OPTS can move in, as the restatement finds it on the two grids.  (The odometry of the log is not the map's frame, and a start on a
    wall cell or in a speck of free cells reaches nothing.)"""
    occ = obj.occupancy_grid(stride=stride, **kw)
    res, s = occ.resolution, occ.stride
    box = (occ.origin[0], occ.origin[1], occ.origin[0] + (occ.width * s - 1) * res, occ.origin[1] + (occ.height * s - 1) * res)
    dist = obj.distance_grid(stride=stride, world_box=box, **kw)
    clear = math.ceil(OPTS["robot_radius"] * (1.0 / res))
    trav, _ = TR.classify(occ.data, dist.data, clear, clear)
    (i, j), size = TR.largest_component_source(trav)
    assert size >= 500
    half = (float(s) - 1.0) / 2.0
    return [occ.origin[0] + res * (float(s) * float(i) + half), occ.origin[1] + res * (float(s) * float(j) + half)]


def _check_routes(obj, here, what, stride=1, **kw):
    """planRoutes from the world point `here` to every frontier seed, against the restatement on occupancy_grid() and distance_grid()
    of the same box, and the world points of the paths against the formula of include/lama/sdm/travel.h"""
    import _oracle as O                                              # w2m, the host's
    fs = obj.frontiers(stride=stride, **kw)
    assert fs is not None and len(fs.frontiers) >= 2, what
    goals = [f["seed"].tolist() for f in fs.frontiers] + [[here[0] + 500.0, here[1]]]
    rs = obj.routes([here], goals, stride=stride, field=True, **OPTS, **kw)
    occ = obj.occupancy_grid(stride=stride, **kw)
    res, s = occ.resolution, occ.stride
    box = (occ.origin[0], occ.origin[1], occ.origin[0] + (occ.width * s - 1) * res, occ.origin[1] + (occ.height * s - 1) * res)
    dist = obj.distance_grid(stride=stride, world_box=box, **kw)
    for g in (occ, dist):
        assert (rs.x0, rs.y0, rs.width, rs.height, rs.stride) == (g.x0, g.y0, g.width, g.height, g.stride), what
        assert rs.resolution == g.resolution and rs.cell_size == g.cell_size and np.array_equal(rs.origin, g.origin), what
    inv = 1.0 / res
    clear = math.ceil(OPTS["robot_radius"] * inv)
    prefer = max(clear, math.ceil(OPTS["preferred_clearance"] * inv))

    def pixel(p):
        c = O.w2m([p[0], p[1], 0.0], res=res)
        i, j = (int(c[0]) - rs.x0) // s, (int(c[1]) - rs.y0) // s
        return (i, j) if 0 <= i < rs.width and 0 <= j < rs.height else None
    Fx, routes, paths = TR.expect(occ.data, dist.data, clear, prefer, OPTS["near_factor"], [pixel(here)], [pixel(g) for g in goals], OPTS["goal_reach"],
                                  OPTS["max_path_points"])
    assert np.array_equal(rs.field, Fx), what
    for name in TR.ROUTE_T.names:
        assert np.array_equal(rs.routes[name], routes[name]), (what, name)
    assert routes[-1]["status"] == TR.OUTSIDE and (routes["status"] == TR.REACHED).sum() >= 2, what
    half = (float(s) - 1.0) / 2.0
    for g, r in enumerate(routes):
        n = min(OPTS["max_path_points"], int(r["steps"]) + 1) if r["status"] == TR.REACHED else 0
        assert rs.routes[g]["path_points"] == n == len(rs.paths[g]), what
        want = [[rs.origin[0] + res * (float(s) * float(int(p) % rs.width) + half), rs.origin[1] + res * (float(s) * float(int(p) // rs.width) + half)] for p in paths[g][:n]]
        assert rs.paths[g].tolist() == want, (what, g)
        if n:
            assert rs.routes[g]["length_m"] == float(r["cost"]) * rs.cell_size / 5.0 and pixel(rs.paths[g][0]) == pixel(here)
    assert (routes["steps"] + 1 > OPTS["max_path_points"]).any(), what     # some path is cut by the cap
    return rs


def test_host_classes_plan_routes_through_their_device_maps():
    pts, odom, _ = F.corridor_log(8, 120)
    s = F.Slam2D(trans_thresh=0.01, rot_thresh=0.01)
    assert s.routes([odom[0][:2]], [odom[0][:2]]) is None                      # before the first scan
    for k in range(8):
        s.update(pts[k], odom[k])
    s.view_bounds(0)                                                           # getOccupancyMap(): downloads the snapshot
    cells_before = s.view_cells(0)
    for stride in (1, 2):
        _check_routes(s, _open_spot(s, stride), f"Slam2D, stride {stride}", stride=stride)
    here = _open_spot(s)
    assert np.array_equal(s.view_cells(0), cells_before)                       # the snapshot is neither remade nor dropped
    bare = s.routes([here], [here], max_path_points=0)
    assert bare.field is None and tuple(bare.routes[["status", "cost", "steps", "path_points"]][0]) == (TR.REACHED, 0, 0, 0) and len(bare.paths[0]) == 0
    with pytest.raises(F.LamaError) as e:                                      # a start point outside the map's box
        s.routes([[here[0] + 500.0, here[1]]], [here])
    assert "lama_hip_map_travel" in str(e.value) and "source" in str(e.value)
    s.close()

    pf = F.PFSlam2D(F.pf_options(particles=4, seed=3, trans_thresh=0.01, rot_thresh=0.01))
    pf.set_prior(*odom[0])
    for k in range(8):
        pf.update(pts[k], odom[k])
    i = (pf.best() + 1) % 4
    _check_routes(pf, _open_spot(pf, particle=i), "PFSlam2D, another particle", particle=i)
    here = _open_spot(pf)
    there = [[here[0] + 1.0, here[1]], here]
    a, b = pf.routes([here], there, goal_reach=8), pf.routes([here], there, goal_reach=8, particle=pf.best())
    assert a.routes[1]["status"] == TR.REACHED and np.array_equal(a.routes, b.routes) and pf.routes([here], there, particle=4) is None
    pf.close()

    mb = F.MapBuilder2D()
    for k in range(8):
        mb.add(pts[k], F.pose_from_xyr(*odom[k]))
    assert mb.routes([odom[7][:2]], [odom[5][:2]]) is None                     # before the first build
    mb.build()
    _check_routes(mb, _open_spot(mb), "MapBuilder2D")
    mb.close()
