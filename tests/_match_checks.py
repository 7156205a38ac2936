"""Checks of the single-map matching kernels (k_match_eval and its cell mode, k_match_solve_batch on a batch of one, k_eval_batch,
k_sample_likelihood) against the CPU oracle, shared by tests/test_match_kernels_gpu.py and the lane-simulator tests.

Tolerances (each derived, none tuned):
  * per-beam outputs (residual, Jacobian row, cell distance) involve no reduction, and device and oracle evaluate the same
    fp64 expressions in the same order (-ffp-contract=off on both sides).  The one input computed by different code is
    the pose's rotation: cos / sin of atan2(s, c), from OCML on the device and from libm in the oracle.  So they are
    BIT-EQUAL where both agree: always in the lane simulator (it links the host's libm) and on the device for poses with
    s = 0, c = 1 (atan2 and sincos of 0 are exact).  Elsewhere a one-ulp difference of the rotation can move the map
    coordinate scale * x + off (about 4.2e7 cells, ulp 7.5e-9) by one ulp: residuals then agree within 1e-9 m and
    Jacobian rows within 1e-6, the tolerances of test_gpu_parity.py (check_match_surface_and_solver);
  * a summed output is compared with math.fsum of the per-beam terms (the exactly rounded sum):
    |dev - fsum| <= n * eps * sum|term|.  Every summation order of n terms stays within that bound, so it holds for the
    kernels' DPP trees and their +0.0 tail lanes, whatever the grouping.  The terms are the oracle's where the per-beam
    values are bit-equal (above); at a solution with an arbitrary heading they are the device's own per-beam values at
    that pose, themselves checked against the oracle in the same call;
  * k_sample_likelihood sums in point order like the reference, so only its exp can differ: OCML's exp is within one ulp
    of libm's, which the cube triples, and the same-order sum of positive terms adds at most nterms * eps / 2 on top:
    relative (nterms + 3) * eps on the device, bit-equal in the simulator (test_gpu_parity.py allows 1e-12);
  * solved poses: POSE_TOL of test_gpu_parity.py (the GN step's exp map goes through sincos; the normal equations are
    summed in a different order), identical iteration counts.
"""
import math

import numpy as np

import _oracle as O
from _cmp import DM_FIELDS, assert_maps_equal
from _worlds import open_corridor, open_corridor_scan

EPS = float(np.finfo(np.float64).eps)
POSE_TOL = 1e-8          # = test_gpu_parity.POSE_TOL
R_TOL, J_TOL = 1e-9, 1e-6  # = check_match_surface_and_solver(exact=False), used only where the rotations may differ
MEAS_SIGMA = 0.05        # lama_hip_default_cfg().meas_sigma = the oracle's calculateLikelihood sigma
CAUCHY_C = 1.0 / (0.15 * 0.15)   # cauchy015 (lama_dev.h)
BLOB = (2.5, 7.5)        # centre of an isolated 0.35 m blob, 3.5 m beyond the corridor's upper wall
SCAN_POSE = (1.3, 1.7, 0.12)


def world_obstacles(half_len=40.0):
    """open_corridor() plus an isolated blob: patches that touch neither wall, and cells between them with no patch"""
    bx, by = BLOB
    blob = [(bx + 0.05 * i, by + 0.05 * j) for i in range(-3, 4) for j in range(-3, 4)]
    return np.concatenate([open_corridor(half_len=half_len), np.array(blob)])


def build_world(F, l2_max, half_len=40.0, **cfg):
    """-> (context, oracle map): one particle whose distance map comes from lama_hip_map_add_obstacles, and the oracle's map
    from DynamicDistanceMap add + update.  The maps are asserted bit-equal first, so every later difference is the kernel's.
    cfg: further members of the context's configuration."""
    cells = np.array([[int(c[0]), int(c[1])] for c in (O.w2m([x, y, 0.0]) for x, y in world_obstacles(half_len))], dtype=np.uint32)
    dm = O.DM.new(l2_max=l2_max)
    for x, y in cells:
        dm.add(int(x), int(y))
    dm.update()
    assert dm.max_sqdist() == math.ceil(l2_max * (1.0 / 0.05)) ** 2
    ctx = F.HipContext(F.default_cfg(particles=1, l2_max=l2_max, **cfg))
    ctx.add_obstacles(0, cells)
    assert_maps_equal(ctx.download_map(0, F.MAP_DISTANCE), dm.dump(), DM_FIELDS, f"world distance map, l2_max {l2_max}")
    return ctx, dm


def scan_of(n, x=SCAN_POSE[0], y=SCAN_POSE[1], yaw=SCAN_POSE[2]):
    """Exactly n sensor-frame points of a scanner at (x, y, yaw) in open_corridor().  open_corridor_scan drops beams without
    a return, so the beam count is searched; tiny n take evenly spaced points of a larger scan."""
    if n >= 8:
        for beams in range(n, 2 * n + 64):
            pts = open_corridor_scan(x, y, yaw, beams=beams)
            if len(pts) == n:
                return pts
    pts = open_corridor_scan(x, y, yaw, beams=max(4 * n, 16))
    return pts[np.linspace(0, len(pts) - 1, n).round().astype(int)]


def edge_scan():
    """(points, pose): hits that sit exactly on cell edges.  Pose (0.5, 1.0, yaw 0) and every point coordinate a multiple of
    0.25 m make every hit coordinate x exactly representable with scale * x + off an integer: the bilinear weights mu are 0."""
    xs = 0.25 * np.arange(-20, 21)
    pts = [(x, -1.0, 0.0) for x in xs] + [(x, 3.0, 0.0) for x in xs] + [(x, 0.5, 0.0) for x in xs[::4]]
    return np.array(pts), O.se2(0.5, 1.0, 0.0)


def _quat_mul(p, q):
    w1, x1, y1, z1 = p
    w2, x2, y2, z2 = q
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


# sensor mounts (origin x, y, z, yaw offset, upside down)
MOUNTS = {"offset": (0.15, -0.05, 0.3, 0.0, False), "yawed": (0.0, 0.0, 0.0, 0.3, False), "upside_down": (0.1, 0.02, 0.0, 0.0, True)}


def mounted_scan(n, mount, x=SCAN_POSE[0], y=SCAN_POSE[1], yaw=SCAN_POSE[2]):
    """-> (points, origin, quat): n points as a sensor mounted by `mount` on a robot at (x, y, yaw) sees open_corridor()"""
    ox, oy, oz, a, flip = mount
    sx = x + math.cos(yaw) * ox - math.sin(yaw) * oy
    sy = y + math.sin(yaw) * ox + math.cos(yaw) * oy
    pts = scan_of(n, sx, sy, yaw + a).copy()
    quat = np.array([math.cos(a / 2), 0.0, 0.0, math.sin(a / 2)])
    if flip:                                   # roll pi: the sensor's y and z axes point the other way
        pts[:, 1] = -pts[:, 1]
        quat = _quat_mul(quat, np.array([math.cos(math.pi / 2), math.sin(math.pi / 2), 0.0, 0.0]))
    return pts, np.array([ox, oy, oz]), quat


def batch_poses(rng, B, x=SCAN_POSE[0], y=SCAN_POSE[1]):
    """B poses with c = 1, s = 0 (so the oracle's per-beam values are the device's, bit for bit): near the scan pose, shifted
    so that hits land where no patch exists (the blob's neighbourhood included), straddling the corridor's end, and so far
    away that every hit falls outside the device's map window"""
    out = np.zeros((B, 4))
    out[:, 0] = 1.0
    for b in range(B):
        k = b % 4
        if k == 0:
            out[b, 2:] = (x + rng.normal(0, 0.05), y + rng.normal(0, 0.05))
        elif k == 1:
            out[b, 2:] = (rng.uniform(-3.0, 6.0), rng.uniform(4.5, 9.0))
        elif k == 2:
            out[b, 2:] = (rng.uniform(33.0, 39.5), rng.uniform(0.5, 3.5))
        else:
            out[b, 2:] = (rng.uniform(300.0, 400.0), rng.uniform(-400.0, -300.0))
    return out


def eval_poses(n_rotated=1):
    """poses for the per-beam checks: at the scan's own heading shift (yaw 0, bit-equal on the device), off the patches,
    far outside the window, and `n_rotated` at an arbitrary heading"""
    x, y, yaw = SCAN_POSE
    poses = [O.se2(x + 0.03, y - 0.02, 0.0), O.se2(2.0, 6.5, 0.0), O.se2(37.0, 2.0, 0.0), O.se2(350.0, -350.0, 0.0)]
    poses += [O.se2(x - 0.01, y + 0.02, yaw + 0.01 + 0.4 * k) for k in range(n_rotated)]
    return poses


def _bit_equal_pose(pose, same_libm):
    return same_libm or (pose[0] == 1.0 and pose[1] == 0.0)


def assert_sum(dev, terms, what):
    """|dev - fsum(terms)| <= n * eps * sum|terms|: any summation order of the n terms stays inside"""
    terms = np.asarray(terms, dtype=np.float64)
    ref = math.fsum(terms)
    bound = len(terms) * EPS * math.fsum(np.abs(terms))
    assert abs(dev - ref) <= bound, (what, dev, ref, abs(dev - ref), bound)


def check_eval(ctx, dm, pts, pose, origin=O.ZERO3, quat=O.IDENT_Q, same_libm=False, what="", particle=0):
    """k_match_eval: residuals and Jacobian rows of MatchSurface2D::eval; cell mode: distance(w2m(hit)) of every beam.
    -> the device's (residuals, Jacobian)"""
    r, J = ctx.match_eval(particle, pts, pose, origin, quat)
    orr, oJ = O.eval_(dm, pts, pose, origin, quat)
    if _bit_equal_pose(pose, same_libm):
        assert np.array_equal(r, orr), (what, np.abs(r - orr).max())
        assert np.array_equal(J, oJ), (what, np.abs(J - oJ).max())
    else:
        assert np.abs(r - orr).max() <= R_TOL, (what, np.abs(r - orr).max())
        assert np.abs(J - oJ).max() <= J_TOL, (what, np.abs(J - oJ).max())
    d = ctx.cell_distances(particle, pts, pose, origin, quat)
    od = O.cell_distances(dm, pts, pose, origin, quat)
    assert np.array_equal(d, od), (what, np.flatnonzero(d != od)[:8])
    return r, J


def check_batch(ctx, dm, pts, poses, origin=O.ZERO3, quat=O.IDENT_Q, what=""):
    """k_eval_batch (squared norm, log-likelihood; lama_hip_match_batch is its log-likelihood alone) on poses with c = 1, s = 0,
    against fsum of the oracle's per-beam terms"""
    assert np.all(poses[:, 0] == 1.0) and np.all(poses[:, 1] == 0.0)
    sq, ll = ctx.eval_batch(0, pts, poses, origin, quat)
    ll2 = ctx.match_batch(0, pts, poses, origin, quat)
    # the same kernel with and without its squared-norm output: bit-equal (test_eval_batch_matches_oracle_and_match_batch)
    assert np.array_equal(ll, ll2), what
    for b, q in enumerate(poses):
        r = O.eval_(dm, pts, q, origin, quat, jac=False)
        rr = r * r
        assert_sum(sq[b], rr, (what, "sqnorm", b))
        assert_sum(ll[b], -rr / MEAS_SIGMA, (what, "loglik", b))
    return sq, ll


def check_solve(ctx, dm, pts, start, origin=O.ZERO3, quat=O.IDENT_Q, same_libm=False, what=""):
    """lama_hip_match_solve (k_match_solve_batch, one problem): pose and iteration count of Solve(GN, Cauchy(0.15)); J^T J lower triangle (weighted J) and the sum of
    squared unweighted residuals at the returned pose against fsum of the per-beam terms there"""
    pose, jtj, sr2, it = ctx.match_solve(0, pts, start, origin, quat)
    opose, oit, _ = O.solve_full(dm, pts, start, origin=origin, quat=quat)
    assert it == oit, (what, it, oit)
    assert np.abs(pose - opose).max() <= POSE_TOL, (what, np.abs(pose - opose).max())
    _check_out7(ctx, dm, pts, pose, jtj, sr2, origin, quat, same_libm, what)
    if _bit_equal_pose(start, same_libm):      # evaluation only (do_solve = 0) at a pose the oracle reproduces bit for bit
        p0, jtj0, sr20, it0 = ctx.match_solve(0, pts, start, origin, quat, solve=False)
        assert it0 == 0 and np.array_equal(p0, start)
        _check_out7(ctx, dm, pts, start, jtj0, sr20, origin, quat, same_libm, (what, "no solve"), oracle_terms=True)
    return pose, it


def _check_out7(ctx, dm, pts, pose, jtj, sr2, origin, quat, same_libm, what, oracle_terms=False):
    r, J = check_eval(ctx, dm, pts, pose, origin, quat, same_libm, what)
    if oracle_terms:
        r, J = O.eval_(dm, pts, pose, origin, quat)
    w = np.sqrt(1.0 / (1.0 + r * r * CAUCHY_C))
    j0, j1, j2 = J[:, 0] * w, J[:, 1] * w, J[:, 2] * w
    for k, t in enumerate((j0 * j0, j1 * j0, j1 * j1, j2 * j0, j2 * j1, j2 * j2)):
        assert_sum(jtj[k], t, (what, "JtJ", k))
    assert_sum(sr2, r * r, (what, "sum r^2"))


def sampling_ref(dm, pts, yaw, xy, step):
    """Loc2D::addSamplingCovariance's sum for an unmounted sensor, in point order: hit = (R(yaw) p) + (0 + xy) with the
    device's operation order (the host composes AngleAxis(yaw) with the identity mount), then distance_cell(w2m(hit))"""
    cs, sn = math.cos(yaw), math.sin(yaw)
    out = []
    for x, y in xy:
        l = 0.0
        for i in range(0, len(pts), step):
            px, py, pz = (float(v) for v in pts[i])
            hx = ((cs * px + (0.0 - sn) * py) + 0.0 * pz) + (0.0 + float(x))
            hy = ((sn * px + cs * py) + 0.0 * pz) + (0.0 + float(y))
            c = O.w2m([hx, hy, 0.0])
            d = dm.distance_cell(int(c[0]), int(c[1]))
            e = math.exp(-(d * d) / 0.01)
            l += e * e * e
        out.append(l)
    return np.array(out)


def check_sampling(ctx, dm, pts, yaw, xy, same_libm=False, what=""):
    """k_sample_likelihood with Loc2D's step = max(n // 100, 1)"""
    n = len(pts)
    step = max(n // 100, 1)
    nterms = (n + step - 1) // step
    got = ctx.sample_likelihood(0, pts, yaw, xy, step)
    want = sampling_ref(dm, pts, yaw, xy, step)
    tol = 0.0 if same_libm else (nterms + 3) * EPS
    assert np.all(np.abs(got - want) <= tol * want), (what, n, nterms, got, want)
    return nterms
