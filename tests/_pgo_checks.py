"""Checks of the six pose-graph kernels of iris_lama_amd/csrc/lama_pgo.h (k_pgo_factors, k_pgo_reduce, k_pgo_assemble,
k_pgo_retract, k_pgo_error, k_pgo_sum) through lama_hip_pgo_* at their branches, block edges and hubs, shared by
tests/test_pgo_sim.py (the lane simulator of tests/sim, no GPU) and tests/test_pgo_kernels_gpu.py.

The reference is always the CPU oracle: O.pgo_linearize, O.se2_exp / O.se2_mul (LM.retract) and the numpy Levenberg-Marquardt of
tests/_pgo_lm.py, which tests/test_oracle_vs_reference.py pins to the compiled minisam.  Every check takes the ffi module and
`same_libm`:

  same_libm = True   (the simulator: the kernel sources compiled for the host with -ffp-contract=off, glibc's atan2 / sin / cos as
                     in the oracle): err, Hoff, Hdiag, b, the assembled blocks and the retracted poses are BIT-EQUAL to the oracle.
  same_libm = False  (the device: OCML's atan2 / sin / cos may differ from glibc's in the last bits, nothing else may):
    * Hoff, Hdiag and the assembled blocks hold no such call -- products, sums, one sqrt and two divisions per so2_normalize of
      the poses the host uploaded; a prior adds its sqrt_info^2, also exactly -- and stay BIT-EQUAL;
    * err, b and the retracted poses are within K_LIBM * eps * scale of the oracle, scale being the sum of the magnitudes of the
      terms that make the value:
          err row r of a factor      w_r * (2 (|tx| + |ty|) + |theta|) of its relative pose z^-1 x_i^-1 x_j   (err_scale)
          b of a vertex              sum |J_v^T| |e| over its factors                                        (b_scale)
          a retracted pose           |x| + |dx| per component: |t| + |dx_x| + |dx_y| for tx, ty; 1 + |dx_theta| for c, s
      (retract_scale).  A wrong series coefficient or a wrong branch shows as a ratio of 1e3 and more.
  chi2 / half_chi2 in both modes: all terms are non-negative and only the order of the sum differs (wave shuffles, per-block
  partials, the strided k_pgo_sum), so |dev - oracle| <= 3 F eps chi2; without the host's libm the terms themselves move by
  2 |e| K_LIBM eps scale each, which is added (it is far below the summation bound once F reaches a few hundred).
"""
import math

import numpy as np

import _oracle as O
import _pgo_lm as LM
from _posegraph import make_graph

EPS = float(np.finfo(np.float64).eps)
# max |dev - oracle| / (eps * scale) over err, b and the retracted poses of every check below.
# MEASURED on an MI355X (ROCm's OCML against glibc): err 1.00, b 2.13, retracted poses 0 (bit-equal).  Asserted: 4 x 2.13 rounded
# up to a power of two = 16; the factor 4 leaves room for another libm, a wrong coefficient or branch shows as 1e3 and more.
K_LIBM = 16.0
MEASURED = {}                # name -> the largest ratio seen (printed by the device run that measures K_LIBM)
LAMA_HIP_E_STATE = -5        # include/lama_hip.h
W = (2.0, 2.0, 10.0)         # sqrt_info of SimplePGO's between factors (sigmas 0.5, 0.5, 0.1)
PI_NEAR = math.pi - 1e-9


# ------------------------------------------------------------------------------------------------------------------
# scales and comparisons
# ------------------------------------------------------------------------------------------------------------------
def rel_poses(poses, fi, fj, meas):
    """[F,4]: z^-1 (x_i^-1 x_j) of a between factor, z^-1 x_i of a prior -- what pgo_log is applied to (oracle products)"""
    out = np.zeros((len(fi), 4))
    for k in range(len(fi)):
        x = poses[fi[k]] if fj[k] < 0 else O.se2_mul(O.se2_inverse(poses[fi[k]]), poses[fj[k]])
        out[k] = O.se2_mul(O.se2_inverse(meas[k]), x)
    return out


def err_scale(rel, sq):
    mag = 2.0 * (np.abs(rel[:, 2]) + np.abs(rel[:, 3])) + np.abs(np.arctan2(rel[:, 1], rel[:, 0]))
    return np.asarray(sq, dtype=np.float64).reshape(-1, 3) * mag[:, None]


def _adj(g):
    return np.array([[g[0], -g[1], g[3]], [g[1], g[0], -g[2]], [0.0, 0.0, 1.0]])


def jacobians(poses, fi, fj, sq):
    """Whitened J_i, J_j [F,3,3] (BetweenFactor.h:59-67: J_i = Adj(x_j^-1) * -Adj(x_i), J_j = I; PriorFactor: J_i = I).  Used for
    the scale of b only; check_hub pins it to the oracle's Hoff."""
    Fn = len(fi)
    Ji, Jj = np.zeros((Fn, 3, 3)), np.zeros((Fn, 3, 3))
    for k in range(Fn):
        w = np.asarray(sq[k], dtype=np.float64)[:, None]
        if fj[k] < 0:
            Ji[k] = w * np.eye(3)
        else:
            Ji[k] = w * (_adj(O.se2_inverse(poses[fj[k]])) @ -_adj(poses[fi[k]]))
            Jj[k] = w * np.eye(3)
    return Ji, Jj


def b_scale(N, fi, fj, Ji, Jj, err):
    s = np.zeros((N, 3))
    for k in range(len(fi)):
        s[fi[k]] += np.abs(Ji[k]).T @ np.abs(err[k])
        if fj[k] >= 0:
            s[fj[k]] += np.abs(Jj[k]).T @ np.abs(err[k])
    return s


def retract_scale(x, dx):
    t = np.abs(dx[:, 0]) + np.abs(dx[:, 1])
    r = 1.0 + np.abs(dx[:, 2])
    return np.stack([r, r, np.abs(x[:, 2]) + t, np.abs(x[:, 3]) + t], axis=1)


def assert_close(name, dev, orc, scale, same_libm, what=""):
    """bit-equal with the host's libm; within K_LIBM * eps * scale without (the largest ratio goes to MEASURED[name])"""
    dev, orc = np.asarray(dev), np.asarray(orc)
    if same_libm:
        assert np.array_equal(dev, orc), (name, what, float(np.abs(dev - orc).max()))
        return
    diff = np.abs(dev - orc)
    scale = np.broadcast_to(scale, diff.shape)
    assert np.all(diff[scale == 0] == 0), (name, what, "a difference where the value is made of zeros")
    ratio = float((diff[scale > 0] / (EPS * scale[scale > 0])).max()) if np.any(scale > 0) else 0.0
    MEASURED[name] = max(MEASURED.get(name, 0.0), ratio)
    assert ratio <= K_LIBM, (name, what, ratio)


def chi2_allowance(Fn, chi2, same_libm, err=None, escale=None):
    tol = 3.0 * Fn * EPS * chi2
    if not same_libm and err is not None:
        tol += 2.0 * K_LIBM * EPS * float((np.abs(err) * escale).sum())
    return tol


def compare_linearisation(F, N, fi, fj, meas, sq, poses, same_libm, what="", graph=None):
    """linearize and linearize_system of one graph at `poses` against the oracle: err, Hoff, Hdiag, b, chi2; blocks, b, diag,
    half_chi2.  -> (dev, orc, sys)"""
    fi, fj = np.asarray(fi, dtype=np.int32), np.asarray(fj, dtype=np.int32)
    meas, sq = np.asarray(meas, dtype=np.float64).reshape(-1, 4), np.asarray(sq, dtype=np.float64).reshape(-1, 3)
    poses = np.asarray(poses, dtype=np.float64).reshape(N, 4)
    g = graph or F.PoseGraph(N, fi, fj, meas, sq)
    try:
        dev = g.linearize(poses)
        sys = g.linearize_system()
    finally:
        if graph is None:
            g.close()
    orc = O.pgo_linearize(poses, fi, fj, meas, sq)
    escale = err_scale(rel_poses(poses, fi, fj, meas), sq)
    assert np.array_equal(dev["Hoff"], orc["Hoff"]), (what, "Hoff", float(np.abs(dev["Hoff"] - orc["Hoff"]).max()))
    assert np.array_equal(dev["Hdiag"], orc["Hdiag"]), (what, "Hdiag", float(np.abs(dev["Hdiag"] - orc["Hdiag"]).max()))
    assert_close("err", dev["err"], orc["err"], escale, same_libm, what)
    bs = None if same_libm else b_scale(N, fi, fj, *jacobians(poses, fi, fj, sq), orc["err"])
    assert_close("b", dev["b"], orc["b"], bs, same_libm, what)
    tol = chi2_allowance(len(fi), orc["chi2"], same_libm, orc["err"], escale)
    assert abs(dev["chi2"] - orc["chi2"]) <= tol, (what, "chi2", dev["chi2"], orc["chi2"], tol)
    assert abs(sys["half_chi2"] - 0.5 * orc["chi2"]) <= 0.5 * tol, (what, "half_chi2", sys["half_chi2"], 0.5 * orc["chi2"], tol)
    row_ptr, cols, contrib = LM.lower_pattern(N, fi, fj)
    assert np.array_equal(sys["blocks"], LM.scatter_blocks(orc, cols, contrib, row_ptr)), (what, "blocks")
    assert np.array_equal(sys["b"], dev["b"]) and np.array_equal(sys["diag"], np.stack([np.diag(h) for h in orc["Hdiag"]])), what
    return dev, orc, sys


def compare_try_step(g, Fn, fi, fj, meas, sq, poses, dx, same_libm, what=""):
    """try_step's return against the oracle's 0.5 chi2 at LM.retract(poses, dx); the current state is `poses` already"""
    half, _ = g.try_step(dx)
    cand = LM.retract(poses, dx)
    orc = O.pgo_linearize(cand, fi, fj, meas, sq)
    tol = chi2_allowance(Fn, orc["chi2"], same_libm, orc["err"], err_scale(rel_poses(cand, fi, fj, meas), sq))
    assert abs(half - 0.5 * orc["chi2"]) <= 0.5 * tol, (what, "try_step", half, 0.5 * orc["chi2"], tol)
    return cand


# ------------------------------------------------------------------------------------------------------------------
# 1. the small-angle branch of pgo_log
# ------------------------------------------------------------------------------------------------------------------
LOG_THETAS = (0.0, 1e-12, 1.40e-5, -1.40e-5, 1.4142e-5, 1.4143e-5, 1.43e-5, -1.43e-5)   # c - 1 from 0 over -9.8e-11 to -1.02e-10
LOG_TRANSLATIONS = ((0.3, -0.2), (1e3, -1e3), (1e-6, 1e-6))


def log_branch_graph():
    """A star around the identity pose: vertex v = (t, theta) for every translation and theta of the lists, one between factor to or
    from vertex 0 (directions alternate: the relative pose is x_v or its inverse) and one prior each, all measuring the identity --
    the error is the log of the relative pose."""
    ident = O.se2(0, 0, 0)
    poses, fi, fj = [ident], [], []
    for tx, ty in LOG_TRANSLATIONS:
        for th in LOG_THETAS:
            v = len(poses)
            poses.append(O.se2(tx, ty, th))
            a, b = (0, v) if v % 2 else (v, 0)
            fi += [a, v]; fj += [b, -1]
    Fn = len(fi)
    return len(poses), np.array(fi, dtype=np.int32), np.array(fj, dtype=np.int32), np.tile(ident, (Fn, 1)), np.tile(W, (Fn, 1)), np.array(poses)


def check_log_branch(F, same_libm):
    N, fi, fj, meas, sq, poses = log_branch_graph()
    rel = rel_poses(poses, fi, fj, meas)
    small = np.abs(rel[:, 0] - 1.0) < 1e-10               # (c - 1 has no libm call: the device takes the same branch)
    per_t = len(fi) // len(LOG_TRANSLATIONS)
    for t in range(len(LOG_TRANSLATIONS)):
        s = small[t * per_t:(t + 1) * per_t]
        nz = np.abs(rel[t * per_t:(t + 1) * per_t, 1]) > 0          # (theta = 0 gives h = 1 on both branches: it does not count)
        assert (s & nz).sum() >= 2 and (~s).sum() >= 2, (t, s)
    mid = np.abs(rel[:, 0] - 1.0)
    assert mid[small].max() > 9.7e-11 and mid[~small].min() < 1.03e-10          # both sides within 3 % of the threshold
    compare_linearisation(F, N, fi, fj, meas, sq, poses, same_libm, "log branch")


# ------------------------------------------------------------------------------------------------------------------
# 2. rotation errors near the cut of atan2
# ------------------------------------------------------------------------------------------------------------------
CUT_ERRORS = tuple(s * e for e in (PI_NEAR, math.pi - 1e-6, 3.0, 0.5 * math.pi) for s in (1.0, -1.0))


def rotation_cut_graph():
    """-> N, fi, fj, meas, sq, poses, expected rotation error per factor.  Vertex pairs (a, b = a * z * d) and priors (x = z * d):
    d carries the rotation error; headings of a and z vary, identity measurements included.  Then pairs whose own headings are
    +-(pi - 1e-9), on either side of the cut, with a measurement that leaves an error of +-0.1 rad."""
    poses, fi, fj, meas, want = [], [], [], [], []
    headings = (0.0, 0.7, -2.9, PI_NEAR, -PI_NEAR)
    for n, e in enumerate(CUT_ERRORS):
        a = O.se2(1.5 - n, 0.25 * n, headings[n % 5])
        z = O.se2(0, 0, 0) if n % 2 == 0 else O.se2(0.8, -0.3, headings[(n + 2) % 5])
        d = O.se2(0.05, -0.02 * n, e)
        b = O.se2_mul(a, O.se2_mul(z, d))
        v = len(poses)
        poses += [a, b]
        fi += [v, v + 1, v + 1]; fj += [v + 1, v, -1]
        meas += [z, O.se2_inverse(z), O.se2_mul(b, O.se2_inverse(d))]          # the reversed factor's error is log(z d^-1 z^-1)
        want += [e, -e, e]
    for n, (ha, e) in enumerate(((PI_NEAR, 0.1), (-PI_NEAR, 0.1), (PI_NEAR, -0.1), (-PI_NEAR, -0.1))):
        a = O.se2(-3.0, 2.0 + n, ha)
        z = O.se2(0.4, 0.1, 2e-9 * (1 if ha < 0 else -1))                      # a * z lies on the other side of the cut
        b = O.se2_mul(a, O.se2_mul(z, O.se2(0.01, 0.02, e)))
        v = len(poses)
        poses += [a, b]
        fi += [v, v, v + 1]; fj += [v + 1, -1, -1]
        meas += [z, O.se2_mul(a, O.se2_inverse(O.se2(0.02, 0.0, e))), O.se2(b[2], b[3], math.atan2(b[1], b[0]) - e)]
        want += [e, e, e]
    Fn = len(fi)
    return len(poses), np.array(fi, dtype=np.int32), np.array(fj, dtype=np.int32), np.array(meas), np.tile(W, (Fn, 1)), np.array(poses), np.array(want)


def check_rotation_cut(F, same_libm):
    N, fi, fj, meas, sq, poses, want = rotation_cut_graph()
    orc = O.pgo_linearize(poses, fi, fj, meas, sq)
    theta = orc["err"][:, 2] / sq[:, 2]
    # the cases are what they claim: the sign at the cut is decided by the data (1e-9 away), not by the last bit
    assert np.abs(theta - want).max() < 1e-12, np.abs(theta - want).max()
    assert (np.abs(theta) > math.pi - 2e-9).sum() >= 4 and (theta > 3.0).any() and (theta < -3.0).any()
    compare_linearisation(F, N, fi, fj, meas, sq, poses, same_libm, "rotation cut")


# ------------------------------------------------------------------------------------------------------------------
# 3. block edges of PGO_BLOCK = 256 in F and N
# ------------------------------------------------------------------------------------------------------------------
def block_edge_graphs():
    """name -> (N, fi, fj, meas, sq, poses)"""
    out = {}
    node = O.se2(1.5, -0.5, 0.3)
    out["N1 F1"] = (1, np.array([0], np.int32), np.array([-1], np.int32), O.se2(1.4, -0.45, 0.25)[None], np.array([W]), node[None])
    for N, loops in ((256, 0), (256, 1), (256, 256), (256, 257), (257, 0), (257, 256)):
        fi, fj, meas, sq, truth, init = make_graph(N, loops, seed=N + loops)
        out[f"N{N} F{len(fi)}"] = (N, fi, fj, meas, sq, init)
    fi, fj, meas, sq, truth, init = make_graph(256, 0, seed=77)
    # F = 255: the last odometry factor dropped, the last vertex is isolated
    out["N256 F255 isolated"] = (256, fi[:-1], fj[:-1], meas[:-1], sq[:-1], init)
    # the last vertex carries only a prior
    fj2, meas2 = fj.copy(), meas.copy()
    fi2 = fi.copy(); fi2[-1] = 255; fj2[-1] = -1; meas2[-1] = truth[255]
    out["N256 F256 last prior"] = (256, fi2, fj2, meas2, sq, init)
    return out


def check_block_edges(F, same_libm):
    graphs = block_edge_graphs()
    assert sorted({len(g[1]) for g in graphs.values()}) == [1, 255, 256, 257, 512, 513] and {g[0] for g in graphs.values()} == {1, 256, 257}
    rng = np.random.default_rng(5)
    for name, (N, fi, fj, meas, sq, poses) in graphs.items():
        g = F.PoseGraph(N, fi, fj, meas, sq)
        try:
            dev, orc, sys = compare_linearisation(F, N, fi, fj, meas, sq, poses, same_libm, name, graph=g)
            if "isolated" in name:
                assert not np.any(dev["Hdiag"][N - 1]) and not np.any(dev["b"][N - 1]) and not np.any(sys["blocks"][-1])
            if "last prior" in name:
                assert np.array_equal(dev["Hdiag"][N - 1], np.diag(np.square(sq[-1]))) and np.any(dev["b"][N - 1])
            dx = rng.normal(0, [0.05, 0.05, 0.02], size=(N, 3))
            cand = compare_try_step(g, len(fi), fi, fj, meas, sq, poses, dx, same_libm, name)
            # the last factor counts (k_pgo_error's bound): without it the error is visibly another
            last = O.pgo_linearize(cand, fi[-1:], fj[-1:], meas[-1:], sq[-1:])["chi2"]
            assert last > 1e3 * chi2_allowance(len(fi), O.pgo_linearize(cand, fi, fj, meas, sq)["chi2"], False), name
        finally:
            g.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. more than 64 partial sums: the strided loop of k_pgo_sum runs twice
# ------------------------------------------------------------------------------------------------------------------
def check_many_partials(F, same_libm):
    for loops in (16100, 16384 + 256 - 300):
        N = 300
        fi, fj, meas, sq, truth, init = make_graph(N, loops, seed=loops)
        Fn = len(fi)
        assert Fn == N + loops and (Fn + 255) // 256 >= 65
        g = F.PoseGraph(N, fi, fj, meas, sq)
        try:
            dev = g.linearize(init)
            sys = g.linearize_system()
            orc = O.pgo_linearize(init, fi, fj, meas, sq)
            tol = 3.0 * Fn * EPS * orc["chi2"]                    # the summation bound alone, with or without the host's libm
            print(f"F = {Fn}: chi2 dev - oracle = {dev['chi2'] - orc['chi2']:.3e}, half_chi2 {sys['half_chi2'] - 0.5 * orc['chi2']:.3e}, allowed {tol:.3e}")
            assert abs(dev["chi2"] - orc["chi2"]) <= tol, (dev["chi2"], orc["chi2"], tol)
            assert abs(sys["half_chi2"] - 0.5 * orc["chi2"]) <= 0.5 * tol, (sys["half_chi2"], 0.5 * orc["chi2"], tol)
            assert np.array_equal(dev["Hoff"], orc["Hoff"]) and np.array_equal(dev["Hdiag"], orc["Hdiag"])
            assert_close("err", dev["err"], orc["err"], err_scale(rel_poses(init, fi, fj, meas), sq), same_libm, Fn)
            dx = np.random.default_rng(Fn).normal(0, [0.05, 0.05, 0.02], size=(N, 3))
            half, _ = g.try_step(dx)
            co = O.pgo_linearize(LM.retract(init, dx), fi, fj, meas, sq)
            tol = 3.0 * Fn * EPS * co["chi2"]
            print(f"F = {Fn}: try_step dev - oracle = {half - 0.5 * co['chi2']:.3e}, allowed {0.5 * tol:.3e}")
            assert abs(half - 0.5 * co["chi2"]) <= 0.5 * tol, (half, 0.5 * co["chi2"], tol)
        finally:
            g.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. a hub and a pair carried by many factors: the factor order of k_pgo_reduce and k_pgo_assemble
# ------------------------------------------------------------------------------------------------------------------
HUB_W = (2.0, 2.0, 8.0)      # powers of two: J_i = Hoff^T / w exactly, so the per-factor terms can be rebuilt from Hoff and err


def hub_graph():
    """600 poses; vertex 0 shares a factor with every other one, as i of one factor and j of the next; 40 factors on the pair
    (5, 17) in mixed direction; a prior on vertex 0.  Noisy measurements, so no term vanishes."""
    N = 600
    rng = np.random.default_rng(600)
    th = rng.uniform(-3.0, 3.0, N)
    xy = rng.uniform(-20.0, 20.0, (N, 2))
    poses = np.stack([O.se2(xy[v, 0], xy[v, 1], th[v]) for v in range(N)])
    fi, fj = [0], [-1]
    for v in range(1, N):
        a, b = (0, v) if v % 2 else (v, 0)
        fi.append(a); fj.append(b)
    for q in range(40):
        a, b = (5, 17) if q % 3 else (17, 5)
        fi.append(a); fj.append(b)
    meas = [O.se2_mul(poses[0], O.se2(0.1, -0.2, 0.05))]
    for k in range(1, len(fi)):
        d = O.se2_mul(O.se2_inverse(poses[fi[k]]), poses[fj[k]])
        meas.append(O.se2_mul(d, O.se2(*rng.normal(0, [0.05, 0.05, 0.01]))))
    return N, np.array(fi, dtype=np.int32), np.array(fj, dtype=np.int32), np.array(meas), np.tile(HUB_W, (len(fi), 1)), poses


def own_terms(lin, fi, fj, k, v):
    """J_v^T J_v and J_v^T e of factor k from a linearisation's OWN Hoff and err, operation by operation as k_pgo_factors makes
    them (w is a power of two: Hoff[a][c] = J_i[c][a] * w_c exactly)"""
    w = np.array(HUB_W)
    e = lin["err"][k]
    if fj[k] < 0 or fj[k] == v:                      # identity Jacobian, whitened
        J = np.diag(w)
    else:
        J = lin["Hoff"][k].T / w[:, None]
    D, G = np.zeros((3, 3)), np.zeros(3)
    for a in range(3):
        G[a] = (J[0][a] * e[0] + J[1][a] * e[1]) + J[2][a] * e[2]
        for c in range(3):
            D[a][c] = (J[0][a] * J[0][c] + J[1][a] * J[1][c]) + J[2][a] * J[2][c]
    return D, G


def sequential_vertex_sum(lin, fi, fj, v):
    H, b = np.zeros((3, 3)), np.zeros(3)
    for k in range(len(fi)):
        if fi[k] == v or fj[k] == v:
            D, G = own_terms(lin, fi, fj, k, v)
            H = H + D
            b = b - G
    return H, b


def check_hub(F, same_libm):
    N, fi, fj, meas, sq, poses = hub_graph()
    assert (fi == 0).sum() >= 299 and (fj == 0).sum() >= 299
    dev, orc, sys = compare_linearisation(F, N, fi, fj, meas, sq, poses, same_libm, "hub")
    row_ptr, cols, contrib = LM.lower_pattern(N, fi, fj)
    q175 = [q for q in range(row_ptr[17], row_ptr[18]) if cols[q] == 5][0]
    assert len(contrib[q175]) == 40 and len({tr for _, tr in contrib[q175]}) == 2
    # the rebuilt per-factor terms are the oracle's: one factor linearised alone, bit for bit
    Ji, Jj = jacobians(poses, fi, fj, sq)
    for k, v in ((0, 0), (1, 0), (2, 0), (600, 5), (601, 17), (602, 17)):
        one = O.pgo_linearize(poses, fi[k:k + 1], fj[k:k + 1], meas[k:k + 1], sq[k:k + 1])
        D, G = own_terms(orc, fi, fj, k, v)
        assert np.array_equal(D, one["Hdiag"][v]) and np.array_equal(-G, one["b"][v]), (k, v)
        if fj[k] >= 0:
            assert np.allclose(Ji[k].T @ Jj[k], orc["Hoff"][k], rtol=1e-12, atol=1e-12), k
    for v in (0, 5, 17):
        # the oracle's hub rows ARE the sequential factor-order sums of its per-factor terms
        H, b = sequential_vertex_sum(orc, fi, fj, v)
        assert np.array_equal(H, orc["Hdiag"][v]) and np.array_equal(b, orc["b"][v]), v
        # and the device's are those of ITS per-factor terms, whatever its libm: the order of k_pgo_reduce
        H, b = sequential_vertex_sum(dev, fi, fj, v)
        assert np.array_equal(H, dev["Hdiag"][v]), ("Hdiag in factor order", v)
        assert np.array_equal(b, dev["b"][v]), ("b in factor order", v, dev["b"][v] - b)
    # the order and the transposes of k_pgo_assemble: the device's own Hoff, scattered sequentially
    own = LM.scatter_blocks(dev, cols, contrib, row_ptr)
    assert np.array_equal(sys["blocks"][q175], own[q175]) and np.array_equal(sys["blocks"], own)
    acc = np.zeros((3, 3))
    for k, tr in contrib[q175]:
        acc = acc + (orc["Hoff"][k].T if tr else orc["Hoff"][k])
    assert np.array_equal(sys["blocks"][q175], acc)
    assert not np.array_equal(acc, acc.T)            # (a transpose ignored would show)


# ------------------------------------------------------------------------------------------------------------------
# 6. retract: pgo_exp at its branch, the renormalising product, accept
# ------------------------------------------------------------------------------------------------------------------
RETRACT_THETAS = (0.0,) + tuple(s * t for t in (3e-11, 0.9999e-10, 1.0001e-10, 1e-5, 3.0, PI_NEAR) for s in (1.0, -1.0))
RETRACT_T = (1e-9, 1.0, 1e3)
RETRACT_HEADINGS = (0.3, PI_NEAR, -PI_NEAR, -2.0)


def retract_graph():
    """One pose per (dx theta, translation magnitude, current heading), chained by between factors behind a prior.
    -> N, fi, fj, meas, sq, poses, dx"""
    poses, dx = [], []
    for n, (th, t, h) in enumerate((th, t, h) for th in RETRACT_THETAS for t in RETRACT_T for h in RETRACT_HEADINGS):
        poses.append(O.se2(0.5 * n, -0.25 * n, h))
        dx.append((t, -0.5 * t if n % 2 else 0.75 * t, th))
    poses, dx = np.array(poses), np.array(dx)
    N = len(poses)
    fi = np.array([0] + list(range(N - 1)), dtype=np.int32)
    fj = np.array([-1] + list(range(1, N)), dtype=np.int32)
    meas = np.array([poses[0]] + [O.se2_mul(O.se2_mul(O.se2_inverse(poses[v]), poses[v + 1]), O.se2(0.01, -0.01, 0.002)) for v in range(N - 1)])
    return N, fi, fj, meas, np.tile(W, (N, 1)), poses, dx


def check_retract(F, same_libm):
    N, fi, fj, meas, sq, poses, dx = retract_graph()
    th = np.abs(dx[:, 2])
    assert ((th > 0) & (th < 1e-10)).sum() >= 4 and ((th >= 1e-10) & (th < 1.1e-10)).sum() >= 2      # both sides of pgo_exp's branch
    g = F.PoseGraph(N, fi, fj, meas, sq)
    g2 = F.PoseGraph(N, fi, fj, meas, sq)
    try:
        g.set_poses(poses)
        assert np.array_equal(g.get_poses(), poses)
        compare_try_step(g, N, fi, fj, meas, sq, poses, dx, same_libm, "retract")
        assert np.array_equal(g.get_poses(), poses), "a try alone moved the current state"
        g.accept()
        got = g.get_poses()
        expect = LM.retract(poses, dx)
        assert_close("retract", got, expect, retract_scale(poses, dx), same_libm, "retract")
        # a rejected try leaves the state as it is, bit for bit
        g.try_step(np.full((N, 3), 0.3))
        assert np.array_equal(g.get_poses(), got)
        # the system after accept is the system at get_poses()
        sys = g.linearize_system()
        lin = g2.linearize(got)
        row_ptr, cols, contrib = LM.lower_pattern(N, fi, fj)
        assert np.array_equal(sys["blocks"], LM.scatter_blocks(lin, cols, contrib, row_ptr)) and np.array_equal(sys["b"], lin["b"])
        assert np.array_equal(sys["diag"], np.stack([np.diag(h) for h in lin["Hdiag"]]))
        orc = O.pgo_linearize(got, fi, fj, meas, sq)
        assert np.array_equal(lin["Hoff"], orc["Hoff"]) and np.array_equal(lin["Hdiag"], orc["Hdiag"])
        assert_close("err", lin["err"], orc["err"], err_scale(rel_poses(got, fi, fj, meas), sq), same_libm, "after accept")
        # 50 chained accepts of one dx: the renormalising product keeps (c, s) on the unit circle.  so2_normalize divides by
        # n = sqrt(c^2 + s^2) computed within one eps (two products, a sum, a root: 4 roundings of eps / 2, the root halves three of
        # them) and each quotient adds eps / 2, so the norm is within 1.5 eps of 1 after every step, not 50 times that.
        step = np.tile([0.01, -0.02, 0.37], (N, 1))
        step[1::2, 2] = -2.9
        cur = got
        for _ in range(50):
            g.try_step(step)
            g.accept()
            if same_libm:
                cur = LM.retract(cur, step)
        end = g.get_poses()
        norm = np.sqrt(end[:, 0].astype(np.longdouble) ** 2 + end[:, 1].astype(np.longdouble) ** 2)
        assert np.finfo(np.longdouble).eps < EPS / 100, "the norm check needs extended precision"
        assert float(np.abs(norm - 1).max()) <= 2 * EPS, float(np.abs(norm - 1).max())
        if same_libm:
            assert np.array_equal(end, cur)
    finally:
        g.close()
        g2.close()


# ------------------------------------------------------------------------------------------------------------------
# 7. state handling
# ------------------------------------------------------------------------------------------------------------------
def _refused_accept(g, expect_poses, what):
    rc = g.L.lama_hip_pgo_accept(g.h)
    assert rc == LAMA_HIP_E_STATE, (what, rc)
    msg = g.L.lama_hip_pgo_last_error(g.h).decode()
    assert "no candidate pending" in msg, (what, msg)
    assert np.array_equal(g.get_poses(), expect_poses), (what, "the refused accept changed the current poses")


def check_accept_needs_a_candidate(F):
    N = 50
    fi, fj, meas, sq, truth, init = make_graph(N, 30, seed=8)
    dx = np.random.default_rng(3).normal(0, [0.05, 0.05, 0.02], size=(N, 3))
    g = F.PoseGraph(N, fi, fj, meas, sq)
    try:
        g.set_poses(init)
        _refused_accept(g, init, "fresh graph")
        g.try_step(dx)
        g.accept()
        moved = g.get_poses()
        assert not np.array_equal(moved, init)
        _refused_accept(g, moved, "second accept")
        _refused_accept(g, moved, "third accept")
        g.try_step(dx)
        g.set_poses(truth)
        _refused_accept(g, truth, "accept after set_poses")
        g.try_step(dx)
        g.linearize(init)
        _refused_accept(g, init, "accept after linearize")
        with np.testing.assert_raises(F.LamaError):
            g.accept()
        # and the regular sequence still works afterwards
        g.try_step(dx)
        g.accept()
        assert np.array_equal(g.get_poses(), moved)
    finally:
        g.close()


def _script(g, poses, dx):
    """the calls of one Levenberg-Marquardt iteration; everything they return"""
    out = []
    lin = g.linearize(poses)
    out += [lin[k] for k in ("err", "Hdiag", "Hoff", "b")] + [np.float64(lin["chi2"])]
    yield out
    sys = g.linearize_system()
    out += [sys["blocks"], sys["b"], sys["diag"], np.float64(sys["half_chi2"])]
    yield out
    out.append(np.float64(g.try_step(dx)[0]))
    yield out
    g.accept()
    out.append(g.get_poses())
    yield out
    sys = g.linearize_system()
    out += [sys["blocks"], sys["b"], np.float64(sys["half_chi2"])]
    yield out


def check_two_graphs_do_not_disturb_each_other(F):
    specs = []
    for N, loops, seed in ((50, 30, 1), (257, 300, 2)):
        fi, fj, meas, sq, truth, init = make_graph(N, loops, seed=seed)
        specs.append((N, fi, fj, meas, sq, init, np.random.default_rng(seed).normal(0, [0.05, 0.05, 0.02], size=(N, 3))))
    alone = []
    for N, fi, fj, meas, sq, init, dx in specs:
        g = F.PoseGraph(N, fi, fj, meas, sq)
        try:
            alone.append(list(_script(g, init, dx))[-1])
        finally:
            g.close()
    graphs = [F.PoseGraph(s[0], *s[1:5]) for s in specs]
    try:
        runs = [_script(g, s[5], s[6]) for g, s in zip(graphs, specs)]
        both = [None, None]
        for _ in range(5):                               # one call of the first, one of the second, ...
            for n in (0, 1):
                both[n] = next(runs[n])
    finally:
        for g in graphs:
            g.close()
    for n in (0, 1):
        assert len(both[n]) == len(alone[n]) == 14
        for a, b in zip(both[n], alone[n]):
            assert np.array_equal(a, b), n


# ------------------------------------------------------------------------------------------------------------------
# 8. the whole loop (lama::SimplePGO::optimize over whichever device library the host library is bound to)
# ------------------------------------------------------------------------------------------------------------------
def loop_inputs(N, loops, with_fixed, push=0.0):
    """SimplePGO's three lists from a make_graph trajectory.  push: the dead reckoning turns by that angle more at every second
    step, so the start curls away from what the loop closures say: Gauss-Newton steps out of such a start overshoot, the tries that
    are rejected are rejected by a wide margin, in the middle of the run (not at the optimum, where accept or reject is rounding)"""
    fi, fj, meas, sq, truth, init = make_graph(N, loops, seed=N + 7)
    edges = [(int(fi[k]), int(fj[k]), meas[k]) for k in range(N, len(fi))]
    nodes = init.copy()
    if push:
        for v in range(N - 1):
            nodes[v + 1] = O.se2_mul(nodes[v], O.se2_mul(meas[1 + v], O.se2(0, 0, push if v % 2 == 0 else 0.0)))
    fixed = [(0, nodes[0]), (N // 2, truth[N // 2]), (N - 1, truth[N - 1])] if with_fixed else []
    return nodes, edges, fixed


def check_loop(F, nodes, edges, fixed, need_rejection=False):
    ok, poses, rep = F.simple_pgo(nodes, edges, fixed)
    fi, fj, meas, sq = LM.build_graph(nodes, edges, fixed)
    ref = LM.levenberg_marquardt(fi, fj, meas, sq, nodes)
    assert ok == (ref["status"] == LM.SUCCESS)
    LM.assert_same_run(rep, ref)
    if need_rejection:                        # a rejected try with accepted iterations after it
        its = LM.iterations_of(rep["trace"])
        assert ok and any(LM.REJECTED in it for it in its[:-2]) and its[-1] == [LM.ACCEPTED], its
    assert abs(rep["initial_error"] - ref["initial_error"]) <= 1e-10 * ref["initial_error"]
    assert abs(rep["final_error"] - ref["final_error"]) <= 1e-10 * max(ref["final_error"], 1e-12)
    if ok:
        assert np.abs(poses - ref["poses"]).max() < 1e-8 * max(1.0, np.abs(ref["poses"]).max())
        assert rep["final_error"] < rep["initial_error"]
    else:
        assert np.array_equal(poses, nodes)
    return ok, rep, ref
