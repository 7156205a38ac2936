"""Checks of the per-factor robust losses of the device pose graph (k_pgo_factors_robust, k_pgo_error_robust of
iris_lama_amd/csrc/lama_pgo.h through lama_hip_pgo_create_robust / _factor_weights, and lama::PoseGraph2D on top), shared by
tests/test_robust_pgo_sim.py (the lane simulator, no GPU) and tests/test_robust_pgo_gpu.py.

The reference is always tests/_pgo_robust.py, the scalar restatement that tests/test_robust_pgo_golden.py pins to minisam's own
loss functions and linearisation.  Every check takes the ffi module and `same_libm`, as in tests/_pgo_checks.py:

  same_libm = True   (the simulator, glibc's atan2 as in the restatement): err, Hoff, Hdiag, b, the assembled blocks, diag and the
                     factor weights are BIT-EQUAL to the restatement.
  same_libm = False  (the device, OCML's atan2):
    * a loss-free factor keeps the rule of tests/_pgo_checks.py: its Hoff, and every Hdiag row and assembled block made of
      loss-free factors only, are BIT-EQUAL; its err is within K_LIBM eps err_scale.
    * a robust factor: OCML's atan2 moves the whitened error e in its last bits, and with it n = ||e|| and sqrt(w(n)).  With
      s_r = err_scale of row r (the existing bound on |d e_r|, in units of eps), |d n| <= sum_r s_r =: S (the norm is 1-Lipschitz
      in every component).  The relative sensitivity |d ln sqrt(w) / d ln n| is at most sigma = 1/2 (Huber: sqrt(k / n)), 1 (Cauchy:
      n^2 / (k^2 + n^2) < 1), 2 (DCS: 2 n^2 / (c + n^2) < 2), so sqrt(w) moves by at most rho = sigma S / n relative, plus the
      roundings of the few operations that make it (the `1 +` below).  Hence, per value:
          w                         w * 2 (1 + rho)
          err row r                 sqrt(w) (s_r + |e_r| (1 + rho))
          an entry of J_a^T J_b     w * sum_t |J_a[t][.] J_b[t][.]| * 2 (1 + rho)        (the unweighted products hold no libm call;
                                                                                          J^T J carries sqrt(w) twice)
          b of a vertex             sum over its factors of |J_v^T| |e| (the b_scale of tests/_pgo_checks.py, of the weighted
                                    values) + for the robust ones |J_v^T| (err scale above) + |J_v^T| |e| (1 + rho)
      Hdiag and the assembled blocks add the scales of the robust factors they are made of; a scale of 0 demands equality.
      Asserted: |dev - restatement| <= K_ROBUST eps scale.
  chi2 / half_chi2 / try_step: tests/_pgo_checks.chi2_allowance with the err scale above.

K_ROBUST: the largest ratio |dev - restatement| / (eps scale) MEASURED on an MI355X (ROCm's OCML against glibc) over every check of
this module, times four, rounded up to a power of two (how K_LIBM of tests/_pgo_checks.py was set: room for another libm, while a
wrong formula or branch shows as 1e3 and more).
MEASURED on an MI355X, over the golden cases, the block-edge graphs and the hub: w 0.245, err 0.206, Hoff 0.378, Hdiag 0.490, the
assembled blocks 0.490, b 2.474.  Asserted: 4 x 2.474 rounded up to a power of two = 16.
"""
import os

import numpy as np

import _oracle as O
import _pgo_checks as P
import _pgo_robust as R
from _pgo_lm import scatter_blocks
from _posegraph import make_graph

EPS = P.EPS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robust_pgo_golden.npz")
K_ROBUST = 16.0
MEASURED = {}                # name -> the largest ratio seen in this process (printed per check by assert_close)
LAMA_HIP_E_INVALID, LAMA_HIP_E_STATE = -1, -5      # include/lama_hip.h
ROBUST_PARAM = {R.HUBER: 0.1, R.CAUCHY: 0.3, R.DCS: 0.5}


def load_cases():
    """tests/golden/robust_pgo_golden.npz (tests/golden/make_robust_pgo_golden.py) -> name -> dict(poses, fi, fj, meas, sigmas, sq,
    kind, param, composed, outlier, H, b, werr, esn)"""
    z = np.load(GOLDEN)
    out, at = {}, {}
    width = {"poses": ("N", 4), "fi": ("F", 1), "fj": ("F", 1), "meas": ("F", 4), "sigmas": ("F", 3), "kind": ("F", 1), "param": ("F", 1),
             "composed": ("F", 1), "outlier": ("F", 1), "b": ("N", 3), "werr": ("F", 3)}
    for n, name in enumerate(z["names"]):
        N, F = int(z["num_poses"][n]), int(z["num_factors"][n])
        c = {}
        for field, (per, w) in width.items():
            cnt = (N if per == "N" else F) * w
            a = z[field][at.get(field, 0):at.get(field, 0) + cnt]
            at[field] = at.get(field, 0) + cnt
            c[field] = a.reshape(-1, w) if w > 1 else a
        c["H"] = z["H"][at.get("H", 0):at.get("H", 0) + 9 * N * N].reshape(3 * N, 3 * N)
        at["H"] = at.get("H", 0) + 9 * N * N
        c["esn"] = float(z["esn"][n])
        c["sq"] = 1.0 / c["sigmas"]                     # DiagonalLoss::Sigmas: cwiseInverse
        out[str(name)] = c
    return out


# ------------------------------------------------------------------------------------------------------------------
# scales and the comparison
# ------------------------------------------------------------------------------------------------------------------
def robust_scales(N, fi, fj, meas, sq, kind, poses, ref):
    """-> dict(err [F,3], w [F], Hoff [F,3,3], Hdiag [N,3,3], b [N,3]) as the module's header derives them"""
    F = len(fi)
    s = P.err_scale(P.rel_poses(poses, fi, fj, meas), sq)             # of the whitened error, before the robust loss
    n = np.sqrt((ref["white"] ** 2).sum(axis=1))
    sigma = np.array([R.SENSITIVITY[int(k)] for k in kind])
    rob = np.asarray(kind) != R.NONE
    rho1 = np.where(rob, 1.0 + sigma * s.sum(axis=1) / np.where(n > 0, n, 1.0), 0.0)          # 1 + rho; 0 for a loss-free factor
    sqrtw = np.sqrt(ref["w"])
    err = np.where(rob[:, None], sqrtw[:, None] * (s + np.abs(ref["white"]) * rho1[:, None]), s)
    Ji, Jj, e = np.abs(ref["Ji"]), np.abs(ref["Jj"]), np.abs(ref["err"])
    Hoff = np.einsum("kta,ktc->kac", Ji, Jj) * (2.0 * rho1)[:, None, None]          # (Ji, Jj are the weighted ones: w is inside)
    Hdiag, b = np.zeros((N, 3, 3)), np.zeros((N, 3))
    for k in range(F):
        for v, J in ((fi[k], Ji[k]), (fj[k], Jj[k])):
            if v < 0:
                continue
            Hdiag[v] += (J.T @ J) * 2.0 * rho1[k]
            b[v] += J.T @ e[k]
            if rob[k]:
                b[v] += J.T @ err[k] + (J.T @ e[k]) * rho1[k]
    return {"err": err, "w": ref["w"] * 2.0 * rho1, "Hoff": Hoff, "Hdiag": Hdiag, "b": b, "robust": rob}


def block_scales(sc, cols, contrib, row_ptr):
    out = np.zeros((len(cols), 3, 3))
    for r in range(len(row_ptr) - 1):
        for q in range(row_ptr[r], row_ptr[r + 1]):
            if contrib[q] is None:
                out[q] = sc["Hdiag"][r]
            else:
                for k, tr in contrib[q]:
                    out[q] += sc["Hoff"][k].T if tr else sc["Hoff"][k]
    return out


def assert_close(name, dev, ref, scale, same_libm, what="", K=None):
    """bit-equal with the host's libm; within K eps scale without, and equal wherever the scale is 0"""
    dev, ref = np.asarray(dev), np.asarray(ref)
    if same_libm:
        assert np.array_equal(dev, ref), (name, what, float(np.abs(dev - ref).max()))
        return
    K = K_ROBUST if K is None else K
    diff = np.abs(dev - ref)
    scale = np.broadcast_to(scale, diff.shape)
    assert np.all(diff[scale == 0] == 0), (name, what, "a difference where nothing may move")
    ratio = float((diff[scale > 0] / (EPS * scale[scale > 0])).max()) if np.any(scale > 0) else 0.0
    MEASURED[name] = max(MEASURED.get(name, 0.0), ratio)
    print(f"    [{what}] {name}: max |dev - restatement| / (eps scale) = {ratio:.3f}")
    assert ratio <= K, (name, what, ratio)


def chi2_tol(Fn, chi2, same_libm, err, escale):
    return P.chi2_allowance(Fn, chi2, same_libm, err, escale * max(1.0, K_ROBUST / P.K_LIBM))


def compare(F, N, fi, fj, meas, sq, kind, param, poses, same_libm, what="", graph=None):
    """linearize, linearize_system and factor_weights of one graph at `poses` against the restatement -> (dev, ref, sys, w)"""
    fi, fj = np.asarray(fi, dtype=np.int32), np.asarray(fj, dtype=np.int32)
    meas, sq = np.asarray(meas, dtype=np.float64).reshape(-1, 4), np.asarray(sq, dtype=np.float64).reshape(-1, 3)
    kind, param = np.asarray(kind, dtype=np.int32), np.asarray(param, dtype=np.float64)
    poses = np.asarray(poses, dtype=np.float64).reshape(N, 4)
    g = graph or F.PoseGraph(N, fi, fj, meas, sq, loss_kind=kind, loss_param=param)
    try:
        dev = g.linearize(poses)
        w = g.factor_weights()
        sys = g.linearize_system()
        w2 = g.factor_weights()
    finally:
        if graph is None:
            g.close()
    ref = R.linearize(poses, fi, fj, meas, sq, kind, param)
    sc = robust_scales(N, fi, fj, meas, sq, kind, poses, ref)
    free = ~sc["robust"]
    assert np.array_equal(w, w2) and np.all(w[free] == 1.0), what
    assert_close("w", w, ref["w"], np.where(free, 0.0, sc["w"]), same_libm, what)
    # loss-free factors: today's rule
    assert np.array_equal(dev["Hoff"][free], ref["Hoff"][free]), (what, "Hoff of the loss-free factors")
    P.assert_close("err", dev["err"][free], ref["err"][free], sc["err"][free], same_libm, what)
    # robust factors (and, with a scale of 0 where no robust factor contributes, everything else once more)
    assert_close("err", dev["err"][~free], ref["err"][~free], sc["err"][~free], same_libm, what)
    assert_close("Hoff", dev["Hoff"], ref["Hoff"], sc["Hoff"], same_libm, what)
    assert_close("Hdiag", dev["Hdiag"], ref["Hdiag"], sc["Hdiag"], same_libm, what)
    assert_close("b", dev["b"], ref["b"], sc["b"], same_libm, what)
    tol = chi2_tol(len(fi), ref["chi2"], same_libm, ref["err"], sc["err"])
    assert abs(dev["chi2"] - ref["chi2"]) <= tol, (what, "chi2", dev["chi2"], ref["chi2"], tol)
    assert abs(sys["half_chi2"] - 0.5 * ref["chi2"]) <= 0.5 * tol, (what, "half_chi2", sys["half_chi2"], 0.5 * ref["chi2"], tol)
    row_ptr, cols, contrib = R.lower_pattern(N, fi, fj)
    # the system is the scatter of the device's OWN per-factor outputs, bit for bit, and close to the restatement's
    assert np.array_equal(sys["blocks"], scatter_blocks(dev, cols, contrib, row_ptr)), (what, "blocks")
    assert np.array_equal(sys["b"], dev["b"]) and np.array_equal(sys["diag"], np.stack([np.diag(h) for h in dev["Hdiag"]])), what
    assert_close("blocks", sys["blocks"], scatter_blocks(ref, cols, contrib, row_ptr), block_scales(sc, cols, contrib, row_ptr), same_libm, what)
    return dev, ref, sys, w


def compare_try_step(g, fi, fj, meas, sq, kind, param, poses, dx, same_libm, what=""):
    """try_step's return against the restatement's 0.5 chi2 at retract(poses, dx): the error kernel carries the factor kernel's weight"""
    half, _ = g.try_step(dx)
    cand = R.retract(poses, dx)
    ref = R.linearize(cand, fi, fj, meas, sq, kind, param)
    sc = robust_scales(len(poses), fi, fj, meas, sq, kind, cand, ref)
    tol = chi2_tol(len(fi), ref["chi2"], same_libm, ref["err"], sc["err"])
    assert abs(half - 0.5 * ref["chi2"]) <= 0.5 * tol, (what, "try_step", half, 0.5 * ref["chi2"], tol)
    return cand, ref


# ------------------------------------------------------------------------------------------------------------------
# 1. the golden cases
# ------------------------------------------------------------------------------------------------------------------
def check_golden_cases(F, same_libm):
    cases = load_cases()
    assert len(cases) == 7
    for name, c in cases.items():
        dev, ref, sys, w = compare(F, len(c["poses"]), c["fi"], c["fj"], c["meas"], c["sq"], c["kind"], c["param"], c["poses"], same_libm, name)
        if same_libm:                                  # and with it minisam's own numbers
            assert np.array_equal(dev["err"], c["werr"]) and np.array_equal(dev["b"], c["b"]), name
            assert np.array_equal(R.dense(len(c["poses"]), c["fi"], c["fj"], dev), c["H"]), name
    # the thresholds: error (t, 0, 0) holds no rounding on either libm (atan2(0, 1) = 0), so the weights are the golden ones exactly
    for name, expect_one in (("huber_below", True), ("huber_at", False), ("huber_above", False), ("dcs_below", True), ("dcs_at", True), ("dcs_above", False)):
        c = cases[name]
        g = F.PoseGraph(1, c["fi"], c["fj"], c["meas"], c["sq"], loss_kind=c["kind"], loss_param=c["param"])
        try:
            lin = g.linearize(c["poses"])
            w = g.factor_weights()
        finally:
            g.close()
        assert np.array_equal(lin["err"], c["werr"]), name
        assert (w[0] == 1.0) == (expect_one or name == "huber_at"), (name, w)         # (Huber at n = k: the other branch, k / n = 1)
        assert np.array_equal(w, R.linearize(c["poses"], c["fi"], c["fj"], c["meas"], c["sq"], c["kind"], c["param"])["w"]), name


# ------------------------------------------------------------------------------------------------------------------
# 2. 255, 256, 257 factors: robust factors on both sides of the block edge, the four kinds mixed inside every wave
# ------------------------------------------------------------------------------------------------------------------
def mixed_graph(N, loops, seed, outlier_every=5):
    """make_graph's trajectory with sqrt_info of its own per factor, kinds cycling 0, 1, 2, 3 in factor order, and every
    `outlier_every`-th loop closure measured metres off -> N, fi, fj, meas, sq, kind, param, init"""
    fi, fj, meas, sq, truth, init = make_graph(N, loops, seed=seed)
    Fn = len(fi)
    rng = np.random.default_rng(seed + 1000)
    meas = meas.copy()
    for k in range(N, Fn, outlier_every):
        meas[k] = O.se2_mul(meas[k], O.se2(*rng.uniform(1.0, 3.0, 2), rng.uniform(0.5, 2.0)))
    kind = ((np.arange(Fn) + 2) % 4).astype(np.int32)            # (factors 255 and 256, either side of the block edge, are robust)
    param = np.array([ROBUST_PARAM.get(int(k), 0.0) for k in kind])
    # a robust factor alone (sqrt_info 1) or composed (the sigmas of the reference's chain), alternating
    sq = np.where(((np.arange(Fn) // 4) % 2 == 0)[:, None] & (kind != 0)[:, None], 1.0, 1.0 / np.array([0.25, 0.25, 0.15]))
    return N, fi, fj, meas, sq, kind, param, init


def check_block_edges(F, same_libm):
    rng = np.random.default_rng(11)
    for N, loops, drop in ((200, 56, 1), (200, 56, 0), (200, 57, 0)):
        N, fi, fj, meas, sq, kind, param, init = mixed_graph(N, loops, seed=N + loops)
        if drop:
            fi, fj, meas, sq, kind, param = fi[:-1], fj[:-1], meas[:-1], sq[:-1], kind[:-1], param[:-1]
        Fn = len(fi)
        what = f"F{Fn}"
        assert all({int(k) for k in kind[q:q + 64]} == {0, 1, 2, 3} for q in range(0, 256, 64))          # mixed inside every wave
        assert kind[253] != 0 and (Fn < 256 or kind[255] != 0) and (Fn < 257 or kind[256] != 0)           # robust on both sides of the edge
        g = F.PoseGraph(N, fi, fj, meas, sq, loss_kind=kind, loss_param=param)
        try:
            dev, ref, sys, w = compare(F, N, fi, fj, meas, sq, kind, param, init, same_libm, what, graph=g)
            rob = kind != 0
            assert (w[rob] < 1.0).sum() >= 20 and (w[kind == R.HUBER] == 1.0).any() and (w[kind == R.DCS] == 1.0).any(), what
            # the last factor counts in both kernels: robust or not, it is in the weights and in the error of a step
            dx = rng.normal(0, [0.05, 0.05, 0.02], size=(N, 3))
            cand, cref = compare_try_step(g, fi, fj, meas, sq, kind, param, init, dx, same_libm, what)
            last = float((cref["err"][-1] ** 2).sum())
            assert last > 1e3 * chi2_tol(Fn, cref["chi2"], False, cref["err"], robust_scales(N, fi, fj, meas, sq, kind, cand, cref)["err"]), what
        finally:
            g.close()
    return True


# ------------------------------------------------------------------------------------------------------------------
# 3. a hub: 70 factors on one vertex, robust and plain alternating -- the factor-order sums
# ------------------------------------------------------------------------------------------------------------------
def hub_graph():
    N = 71
    rng = np.random.default_rng(71)
    poses = np.stack([O.se2(*rng.uniform(-10, 10, 2), rng.uniform(-3, 3)) for _ in range(N)])
    fi, fj, meas, kind = [], [], [], []
    for v in range(1, N):
        a, b = (0, v) if v % 2 else (v, 0)
        fi.append(a); fj.append(b)
        d = O.se2_mul(O.se2_inverse(poses[a]), poses[b])
        meas.append(O.se2_mul(d, O.se2(*rng.normal(0, [0.3, 0.3, 0.1]))))
        kind.append(0 if v % 2 else 1 + (v // 2) % 3)
    kind = np.array(kind, dtype=np.int32)
    param = np.array([ROBUST_PARAM.get(int(k), 0.0) for k in kind])
    return N, np.array(fi, dtype=np.int32), np.array(fj, dtype=np.int32), np.array(meas), np.tile(P.HUB_W, (N - 1, 1)), kind, param, poses


def check_hub(F, same_libm):
    N, fi, fj, meas, sq, kind, param, poses = hub_graph()
    assert len(fi) == 70 and ((fi == 0) | (fj == 0)).all() and (kind != 0).sum() == 35
    dev, ref, sys, w = compare(F, N, fi, fj, meas, sq, kind, param, poses, same_libm, "hub")
    assert (w[kind != 0] < 1.0).sum() >= 30
    # the restatement's hub row IS the sequential factor-order sum of its per-factor terms (it is written that way); the device's is
    # that of ITS per-factor terms, whatever its libm, rebuilt exactly from its own err, Hoff and weights: where the hub is a
    # factor's j (the robust ones) its Jacobian is sq sqrt(w) I, sq a power of two and the root correctly rounded on both sides;
    # where it is the i (the loss-free ones) J_i = Hoff^T / sq_c exactly, as in tests/_pgo_checks.own_terms.
    H, b = np.zeros((3, 3)), np.zeros(3)
    sqv = np.array(P.HUB_W)
    for k in range(len(fi)):
        e = dev["err"][k]
        sqrtw = np.sqrt(w[k])
        assert (fj[k] == 0) == (kind[k] != 0)
        J = np.diag(sqv * sqrtw) if fj[k] == 0 else dev["Hoff"][k].T / sqv[:, None]
        D, G = np.zeros((3, 3)), np.zeros(3)
        for a in range(3):
            G[a] = (J[0][a] * e[0] + J[1][a] * e[1]) + J[2][a] * e[2]
            for c in range(3):
                D[a][c] = (J[0][a] * J[0][c] + J[1][a] * J[1][c]) + J[2][a] * J[2][c]
        H, b = H + D, b - G
    assert np.array_equal(H, dev["Hdiag"][0]) and np.array_equal(b, dev["b"][0]), "hub row in factor order"


# ------------------------------------------------------------------------------------------------------------------
# 4. try_step at a retracted state: the error kernel against the factor kernel
# ------------------------------------------------------------------------------------------------------------------
def check_try_step_equals_the_factor_kernel(F, same_libm):
    N, fi, fj, meas, sq, kind, param, init = mixed_graph(120, 150, seed=4)
    dx = np.random.default_rng(9).normal(0, [0.05, 0.05, 0.02], size=(N, 3))
    g = F.PoseGraph(N, fi, fj, meas, sq, loss_kind=kind, loss_param=param)
    g2 = F.PoseGraph(N, fi, fj, meas, sq, loss_kind=kind, loss_param=param)
    try:
        g.set_poses(init)
        sys0 = g.linearize_system()
        w0 = g.factor_weights()
        cand, ref = compare_try_step(g, fi, fj, meas, sq, kind, param, init, dx, same_libm, "try_step")
        half, _ = g.try_step(dx)
        assert np.array_equal(g.factor_weights(), w0), "a try changed the weights of the last linearisation"
        g.accept()
        moved = g.get_poses()
        # the factor kernel at the accepted state reports the error the error kernel judged the step by: same terms, same order
        sys1 = g.linearize_system()
        assert sys1["half_chi2"] == half, (sys1["half_chi2"], half)
        lin = g2.linearize(moved)
        assert 0.5 * lin["chi2"] == half or abs(0.5 * lin["chi2"] - half) <= 3 * len(fi) * EPS * half
        assert not np.array_equal(g.factor_weights(), w0) and np.array_equal(g.factor_weights(), g2.factor_weights())
        assert sys0["half_chi2"] != half
        # the same with the device solver's step (try_solved_step shares the kernel)
        g.set_poses(init)
        g.linearize_system()
        sol = g.solve_pcg(1e-3)
        assert sol["outcome"] == F.PCG_CONVERGED
        h1, _ = g.try_solved_step()
        h2, _ = g.try_step(sol["dx"])
        assert h1 == h2
    finally:
        g.close()
        g2.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. create_robust without a robust factor is create; refusals; factor_weights before a linearisation
# ------------------------------------------------------------------------------------------------------------------
def _everything(g, poses, dx):
    lin = g.linearize(poses)
    sys = g.linearize_system()
    half, _ = g.try_step(dx)
    g.accept()
    sys2 = g.linearize_system()
    return [lin[k] for k in ("err", "Hdiag", "Hoff", "b")] + [np.float64(lin["chi2"]), sys["blocks"], sys["b"], sys["diag"],
            np.float64(sys["half_chi2"]), np.float64(half), g.get_poses(), sys2["blocks"], sys2["b"], np.float64(sys2["half_chi2"]), g.factor_weights()]


def check_no_robust_factor_is_create(F):
    N = 257
    fi, fj, meas, sq, truth, init = make_graph(N, 300, seed=2)
    Fn = len(fi)
    dx = np.random.default_rng(2).normal(0, [0.05, 0.05, 0.02], size=(N, 3))
    outs = []
    for kw in ({}, {"loss_kind": None, "loss_param": np.full(Fn, 0.1)}, {"loss_kind": np.zeros(Fn, np.int32), "loss_param": None},
               {"loss_kind": np.zeros(Fn, np.int32), "loss_param": np.full(Fn, np.nan)}):
        g = F.PoseGraph(N, fi, fj, meas, sq, **kw)
        try:
            outs.append(_everything(g, init, dx))
        finally:
            g.close()
    for o in outs[1:]:
        assert len(o) == len(outs[0]) == 15
        for a, b in zip(o, outs[0]):
            assert np.array_equal(a, b)
    assert np.all(outs[0][-1] == 1.0)


def check_refusals(F):
    N = 20
    fi, fj, meas, sq, truth, init = make_graph(N, 10, seed=3)
    Fn = len(fi)
    good_kind = (np.arange(Fn) % 4).astype(np.int32)
    good_param = np.full(Fn, 0.2)
    for k, kd, pv, word in ((7, 4, 0.2, "unknown loss kind"), (7, -1, 0.2, "unknown loss kind"), (5, 1, 0.0, "not finite and > 0"),
                            (6, 2, -1.0, "not finite and > 0"), (7, 3, float("nan"), "not finite and > 0"), (9, 1, float("inf"), "not finite and > 0")):
        kind, param = good_kind.copy(), good_param.copy()
        kind[k], param[k] = kd, pv
        h = F.C.c_void_p(123)
        L = F.hip_lib()
        rc = L.lama_hip_pgo_create_robust(0, N, F._p(fi), F._p(fj), F._p(meas), F._p(sq), F._p(kind), F._p(param), Fn, F.C.byref(h))
        assert rc == LAMA_HIP_E_INVALID and not h.value, (k, kd, pv, rc)
        msg = L.lama_hip_pgo_last_error(None).decode()
        assert f"factor {k} " in msg and word in msg, msg
        with np.testing.assert_raises(F.LamaError):
            F.PoseGraph(N, fi, fj, meas, sq, loss_kind=kind, loss_param=param)
    # robust kinds without parameters at all
    h = F.C.c_void_p()
    assert F.hip_lib().lama_hip_pgo_create_robust(0, N, F._p(fi), F._p(fj), F._p(meas), F._p(sq), F._p(good_kind), None, Fn, F.C.byref(h)) == LAMA_HIP_E_INVALID
    # a parameter of a loss-free factor is not looked at
    param = good_param.copy()
    param[good_kind == 0] = np.nan
    for kw in ({"loss_kind": good_kind, "loss_param": param}, {}):
        g = F.PoseGraph(N, fi, fj, meas, sq, **kw)
        try:
            w = np.zeros(Fn)
            rc = g.L.lama_hip_pgo_factor_weights(g.h, F._p(w))
            assert rc == LAMA_HIP_E_STATE and "nothing linearised yet" in g.L.lama_hip_pgo_last_error(g.h).decode(), rc
            with np.testing.assert_raises(F.LamaError):
                g.factor_weights()
            g.set_poses(init)
            g.linearize_system()
            assert g.factor_weights().shape == (Fn,)
        finally:
            g.close()


# ------------------------------------------------------------------------------------------------------------------
# 6. lama::PoseGraph2D::optimize on a ring with false closures
# ------------------------------------------------------------------------------------------------------------------
# The seed of the ring: the smallest for which the numpy Levenberg-Marquardt ALONE (tests/_pgo_robust.py, no device code) returns
# SUCCESS with Huber on the closures, leaves every false closure at a weight < 1 and every true one at exactly 1, and ends closer
# to the ground truth than the same loop on the same graph without a loss.  (Seed 0 does; ring_meets_the_input_condition() checks it
# on the CPU, tests/test_robust_pgo_sim.py::test_ring_seed_meets_the_input_condition.)
# The loss-free graph is all but quadratic: its loop converges in two iterations and the third compares error changes of 1e-12,
# so whether it ends with SUCCESS or ERROR_INCREASE -- whether optimize() writes poses at all -- is rounding, in the numpy loop and
# on the device alike.  The loss-free end state the device's result is compared with is therefore the numpy loop's (the state after
# its accepted steps, whatever the status of its last iteration).
RING_SEED = 0
RING_N, RING_TRUE, RING_FALSE = 40, 6, 2
PRIOR_SIGMAS, CHAIN_SIGMAS, UNIT = (0.01, 0.01, 0.01), (0.25, 0.25, 0.15), (1.0, 1.0, 1.0)      # graph_slam2d.cpp:214,224,266


def ring_graph(seed=None):
    """The reference's GraphSlam2D graph on a ring of 40 poses (radius 5 m): prior 0.01 on node 0, chain factors (0.25, 0.25, 0.15)
    from noisy odometry, 6 true closures across the ring and 2 gross false ones (metres off), all closures with unit sigmas.
    -> truth, nodes (dead reckoning), factors [(i, j, pose, sigmas)], closure indices true / false"""
    rng = np.random.default_rng(RING_SEED if seed is None else seed)
    N = RING_N
    ang = 2 * np.pi * np.arange(N) / N
    truth = np.stack([O.se2(5 * np.cos(a), 5 * np.sin(a), a + np.pi / 2) for a in ang])
    odo = [O.se2_mul(O.se2_mul(O.se2_inverse(truth[v]), truth[v + 1]), O.se2(*rng.normal(0, [0.03, 0.03, 0.02]))) for v in range(N - 1)]
    nodes = [truth[0]]
    for v in range(N - 1):
        nodes.append(O.se2_mul(nodes[v], odo[v]))
    nodes = np.stack(nodes)
    factors = [(0, -1, truth[0], PRIOR_SIGMAS)] + [(v, v + 1, odo[v], CHAIN_SIGMAS) for v in range(N - 1)]
    true_idx, false_idx = [], []
    for q in range(RING_TRUE):
        a, b = N - 1 - 3 * q, 2 * q                     # the end of the ring seen from its start
        rel = O.se2_mul(O.se2_inverse(truth[a]), truth[b])
        true_idx.append(len(factors))
        factors.append((a, b, O.se2_mul(rel, O.se2(*rng.normal(0, [0.01, 0.01, 0.005]))), UNIT))
    for q in range(RING_FALSE):
        a, b = 10 + 15 * q, 30 - 12 * q
        rel = O.se2_mul(O.se2_inverse(truth[a]), truth[b])
        false_idx.append(len(factors))
        factors.append((a, b, O.se2_mul(rel, O.se2(3.0 + q, -2.5, 0.8)), UNIT))
    return truth, nodes, factors, true_idx, false_idx


def ring_arrays(factors, huber):
    fi = np.array([f[0] for f in factors], dtype=np.int32)
    fj = np.array([f[1] for f in factors], dtype=np.int32)
    meas = np.array([f[2] for f in factors])
    sq = 1.0 / np.array([f[3] for f in factors])
    closure = np.arange(len(factors)) >= RING_N
    kind = np.where(closure & huber, R.HUBER, R.NONE).astype(np.int32)
    return fi, fj, meas, sq, kind, np.where(kind != 0, 0.1, 0.0)


_ring_cache = {}


def ring_reference(seed=None):
    """The numpy Levenberg-Marquardt on the ring, with Huber(0.1) on the closures and without any loss; computed once per process.
    -> dict(huber=run, plain=run, w=final weights, err_huber / err_plain = largest position error against the truth)"""
    key = RING_SEED if seed is None else seed
    if key in _ring_cache:
        return _ring_cache[key]
    truth, nodes, factors, true_idx, false_idx = ring_graph(seed)
    out = {}
    for name, huber in (("huber", True), ("plain", False)):
        fi, fj, meas, sq, kind, param = ring_arrays(factors, huber)
        out[name] = R.levenberg_marquardt(lambda p: R.linearize(p, fi, fj, meas, sq, kind, param), fi, fj, nodes)
        out["err_" + name] = float(np.hypot(*(out[name]["poses"][:, 2:] - truth[:, 2:]).T).max())
        if huber:
            end = R.linearize(out[name]["poses"], fi, fj, meas, sq, kind, param)
            out["w"] = end["w"]
            out["grad1"] = float(sum((np.abs(J[k]).T @ np.abs(end["err"][k])).sum() for J in (end["Ji"], end["Jj"]) for k in range(len(fi))))
    _ring_cache[key] = out
    return out


def ring_meets_the_input_condition(seed=None):
    truth, nodes, factors, true_idx, false_idx = ring_graph(seed)
    ref = ring_reference(seed)
    return (ref["huber"]["status"] == R.SUCCESS and bool(np.all(ref["w"][false_idx] < 1.0)) and bool(np.all(ref["w"][true_idx] == 1.0))
            and ref["err_huber"] < ref["err_plain"] and ref["plain"]["iterations"] >= 2 and ref["plain"]["trace"][:2] == [R.ACCEPTED, R.ACCEPTED])


def check_ring(F, solver):
    truth, nodes, factors, true_idx, false_idx = ring_graph()
    ref = ring_reference()
    assert ring_meets_the_input_condition()
    with_loss = [f + (("huber", 0.1),) if k >= RING_N else f for k, f in enumerate(factors)]
    ok, poses, rep = F.pose_graph_optimize(nodes, with_loss, solver=solver)
    run = ref["huber"]
    assert ok and rep["status"] == R.SUCCESS
    R.assert_same_run(rep, run)
    assert abs(rep["initial_error"] - run["initial_error"]) <= 1e-10 * run["initial_error"]
    dpose = np.abs(poses - run["poses"]).max()
    assert dpose < 1e-8 * max(1.0, np.abs(run["poses"]).max())
    # two end states dpose apart differ in error by its derivative times that, to first order.  The derivative does not vanish at
    # the end: minisam's loop minimises 0.5 sum w n^2 by steps that hold w fixed, so where it stops b = -J^T e is zero but the
    # error's own slope is not (a Huber outlier contributes 0.5 k n, whose slope is half of its term of b).  Per factor that slope is
    # at most |J^T| |e| for all three losses (d(0.5 w n^2)/dn <= w n), summed here without cancellation (grad1, at the numpy run's
    # end; doubled for the higher orders), on top of the rounding of the sum.
    assert abs(rep["final_error"] - run["final_error"]) <= 2.0 * ref["grad1"] * dpose + 1e-10 * run["final_error"]
    w = rep["weights"]
    assert w.shape == (len(factors),) and np.all(w[:RING_N] == 1.0)
    assert np.all(w[false_idx] < 1.0) and np.all(w[true_idx] == 1.0), (w[false_idx], w[true_idx])
    e_huber = float(np.hypot(*(poses[:, 2:] - truth[:, 2:]).T).max())
    print(f"    ring [{solver}]: largest position error {e_huber:.4f} m under Huber, {ref['err_plain']:.4f} m without a loss (numpy loop)")
    assert e_huber < ref["err_plain"], (e_huber, ref["err_plain"])
    # the same graph without a loss through the same class: every weight is 1, and its first two iterations are the numpy loop's
    ok2, plain, rep2 = F.pose_graph_optimize(nodes, factors, solver=solver)
    assert np.all(rep2["weights"] == 1.0) and list(rep2["trace"][:2]) == [R.ACCEPTED, R.ACCEPTED]
    assert abs(rep2["initial_error"] - ref["plain"]["initial_error"]) <= 1e-10 * ref["plain"]["initial_error"]
    return poses, rep


def check_host_class_refusals(F):
    """invalid indices, a self edge, an empty graph, a bad loss parameter or sigma: false, status -1, nothing written"""
    truth, nodes, factors, _, _ = ring_graph()
    bad = [[(0, 0, nodes[0], UNIT)], [(0, RING_N, nodes[0], UNIT)], [(-1, 1, nodes[0], UNIT)], [(0, -2, nodes[0], UNIT)], [],
           [(0, 1, nodes[0], UNIT, ("huber", 0.0))], [(0, 1, nodes[0], UNIT, ("dcs", float("nan")))], [(0, 1, nodes[0], (1.0, 0.0, 1.0))]]
    for extra in bad:
        fs = (factors + extra) if extra else []
        ok, poses, rep = F.pose_graph_optimize(nodes, fs)
        assert not ok and rep["status"] == -1 and rep["tries"] == 0 and np.array_equal(poses, nodes) and len(rep["weights"]) == 0, extra
    ok, poses, rep = F.pose_graph_optimize(np.zeros((0, 4)), [])
    assert not ok and rep["status"] == -1
