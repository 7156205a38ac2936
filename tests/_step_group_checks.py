"""Checks of the grouped step schedule (lama_hip_pf_match_and_map: particle groups on streams of their own, the status of a group's
map update collected with its next scan match) through the C-ABI, shared by tests/test_step_groups_gpu.py and the lane-simulator
tests (tests/test_step_groups_sim.py).

The reference is the CPU oracle's particle filter, teacher-forced: a step hands the device the start poses, the oracle's particles
are set to the poses the DEVICE matched (they differ from the oracle's own solve in the last bits) and integrate the scan there, so
both maps of every particle compare bit for bit (device-side checksums against the oracle's) after EVERY step.  The scan match itself
is compared with the oracle's solve from the same start poses within POSE_TOL.

World and scanner: the pillar hall of tests/_window_checks.py (180 beams, returns within 3 m).  Which path a case took is read from
the context's counters; a case that stops exercising its path fails."""
import math

import numpy as np

import _oracle as O
import _window_checks as W
from _worlds import segment_world_scan

POSE_TOL = W.POSE_TOL
LL_RTOL = 1e-9             # = test_gpu_parity.LL_RTOL


def device_step(F, ctx, pf, start, scan, what, dm_kind=0, check_maps=True):
    """One whole device step from `start`; -> the matched poses.  check_maps=False: nothing is asked of the context afterwards, so
    the status of this step's map update is collected by the NEXT step, with its scan match, and not by a call that drains."""
    P = len(start)
    pf.set_poses(start); pf.set_weights(w=np.zeros(P), ws=np.zeros(P)); pf.stage_set_scan(scan); pf.stage_scan_match()
    o_poses, o_ll = pf.poses().copy(), pf.weights()[0].copy()
    g_poses, g_ll, g_it = ctx.match_and_map(scan, start)
    assert np.abs(g_poses - o_poses).max() <= POSE_TOL, (what, np.abs(g_poses - o_poses).max())
    assert np.allclose(g_ll, o_ll, rtol=LL_RTOL), (what, g_ll, o_ll)
    pf.set_poses(g_poses); pf.stage_update_maps()
    if not check_maps:
        return g_poses
    assert np.array_equal(ctx.get_poses(), g_poses), what
    assert np.array_equal(ctx.map_checksums(F.MAP_DISTANCE), pf.map_checksums(dm_kind)), f"{what}: distance maps"
    assert np.array_equal(ctx.map_checksums(F.MAP_OCCUPANCY), pf.map_checksums(1)), f"{what}: occupancy maps"
    return g_poses


def _start_poses(pr, x, y, yaw):
    """every particle a few centimetres off its own consistent world: the scan match has work to do"""
    return np.stack([O.se2(x + W.OFFSETS[i % 3][0] + 0.02, y + W.OFFSETS[i % 3][1] - 0.015, yaw + 0.004 * (i + 1)) for i in range(pr.P)])


def check_window_moves_and_grows(F, groups, P=3, window=16, stops=(4.0, 8.0, 12.0, 16.0, 20.0), l2_max=None, every_scan=True, must_grow=True):
    """The robot drives along -x until the mapped area outgrows the window: shifts first, then a growth, each found by whichever
    group's results arrive first while the other groups' work is queued or running.  every_scan: the maps are compared after every
    scan (which drains the groups); else the steps follow each other as in a running filter and the maps are compared at the end.
    must_grow=False: a shorter drive that only shifts the window.  -> the counters"""
    pr = W.Pair(F, P, W._w(window, l2_max), W.START[0], W.START[1], math.pi)
    ctx = pr.ctx
    c0 = ctx.counters()
    for t in stops:
        x, y = W.START[0] - t, W.START[1]
        device_step(F, ctx, pr.pf, _start_poses(pr, x, y, math.pi), W.scan_at(x, y, math.pi), f"-x t = {t}", check_maps=every_scan or t == stops[-1])
    assert ctx.step_groups() == groups
    c = ctx.counters()
    assert c["window_shifts"] > c0["window_shifts"], c
    if must_grow:
        assert c["window_growths"] > c0["window_growths"] and c["window_patches"] > window, c
    pr.assert_maps("after the drive")
    pr.close()
    return c


ROOM = np.array([(-1.2, -1.2, 38.8, -1.2), (38.8, -1.2, 38.8, 38.8), (38.8, 38.8, -1.2, 38.8), (-1.2, 38.8, -1.2, -1.2)])     # 40 m square


def check_clean_abort_grows_the_arenas(F, groups, P=3, l2_max=None, every_scan=True):
    """The smallest arenas a context accepts and an empty room of 40 m, the robot 2 m from a corner and facing it.  The first scan's
    returns are cut at 3 m (the corner: a dozen patches); the next scan, from almost the same place, sees the far walls as well and
    its rays cross a hundred patches and more: the update's allocation phase asks for far more than the particles' regions have free,
    aborts before a cell is modified, and is found aborted only afterwards.  every_scan: by the call that drains the groups to compare
    the maps after the scan; else with the group's NEXT scan match -- the regions grow, the update is repeated, and that scan match,
    which has run on the map as it was before, runs again on the updated one (its poses are compared with the oracle's solve on the
    updated map).  -> the counters"""
    yaw = 1.25 * math.pi

    def scan(x, y, max_range):
        pts = segment_world_scan(ROOM, x, y, yaw, beams=W.BEAMS, max_range=max_range)
        assert len(pts) >= 60
        return pts
    cfg = dict(W._w(32, l2_max), dm_patch_capacity=8, occ_patch_capacity=8)
    pr = W.Pair(F, P, cfg, 0.8, 0.8, yaw, scan=scan(0.8, 0.8, 3.0))
    ctx = pr.ctx
    c0 = ctx.counters()
    stops = ((0.9, 0.85), (1.1, 1.0), (1.3, 1.1))
    for k, (x, y) in enumerate(stops):
        device_step(F, ctx, pr.pf, _start_poses(pr, x, y, yaw), scan(x, y, 60.0), f"stop {k}", check_maps=every_scan or k == len(stops) - 1)
    assert ctx.step_groups() == groups
    c = ctx.counters()
    # a region that has just grown for `count` patches holds round_up32(count + max(32, count / 4)): 64 after the first scan's dozen
    assert c0["occ_patches"] <= 16 * P and c["occ_patches"] - c0["occ_patches"] > 80 * P, (c0, c)      # ... so the update cannot have fitted
    assert c["arena_growths"] + c["pool_growths"] > c0["arena_growths"] + c0["pool_growths"], (c0, c)
    pr.assert_maps("after the last scan")
    pr.close()
    return c
