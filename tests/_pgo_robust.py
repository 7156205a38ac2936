"""Test infrastructure: the pose-graph linearisation with per-factor robust losses, restated in explicit scalar operations in the
reference's order, and minisam's Levenberg-Marquardt (as in tests/_pgo_lm.py) over any linearisation.

What is restated (vendor/minisam/minisam/): PriorFactor<SE2d> / BetweenFactor<SE2d> (slam/PriorFactor.h:50-62,
slam/BetweenFactor.h:50-68), DiagonalLoss (core/LossFunction.cpp:95-113), then per factor HuberLoss, CauchyLoss or DCSLoss
(core/LossFunction.h:173,200-202,230-238; weightInPlace core/LossFunction.cpp:164-228) in ComposedLoss's order, the accumulation of
linearzationLowerHessian in factor order, FactorGraph::errorSquaredNorm (core/FactorGraph.cpp:88-90).  The group operations
(product, inverse, exp) are the CPU oracle's, pinned to the reference elsewhere; everything after them is Python floats: IEEE
doubles, one rounding per operation, no contraction, math.atan2 / math.sqrt of the host's libm.
tests/test_robust_pgo_golden.py pins this module to minisam's own code, bit for bit, through tests/golden/robust_pgo_golden.npz."""
import math

import numpy as np

import _oracle as O
from _pgo_lm import ACCEPTED, ERROR_INCREASE, MAX_ITERATION, RANK_DEFICIENT, REJECTED, SUCCESS  # noqa: F401
from _pgo_lm import assert_same_run, lower_pattern, retract  # noqa: F401

NONE, HUBER, CAUCHY, DCS = 0, 1, 2, 3                 # LAMA_HIP_PGO_LOSS_* (include/lama_hip.h)
SENSITIVITY = {NONE: 0.0, HUBER: 0.5, CAUCHY: 1.0, DCS: 2.0}      # sup |d ln sqrt(w) / d ln n| of each loss


def weight(kind, param, n):
    """w(n) of LossFunction.h; param: Huber k, Cauchy k (k2 = k * k is formed here, as the constructor does), DCS c"""
    if kind == NONE:
        return 1.0
    if kind == HUBER:
        return 1.0 if n < param else param / math.fabs(n)
    if kind == CAUCHY:
        k2 = param * param
        return k2 / (k2 + n * n)
    if kind == DCS:
        e2 = n * n
        if e2 > param:
            w = 2.0 * param / (param + e2)
            return w * w
        return 1.0
    raise ValueError(kind)


def se2_log(g):
    """include/lama/sophus/se2.hpp:519-542"""
    c, s, tx, ty = (float(v) for v in g)
    theta = math.atan2(s, c)
    halftheta = 0.5 * theta
    real_minus_one = c - 1.0
    if math.fabs(real_minus_one) < 1e-10:
        h = 1.0 - (1.0 / 12) * theta * theta
    else:
        h = -(halftheta * s) / real_minus_one
    return [h * tx + halftheta * ty, -halftheta * tx + h * ty, theta]


def _adj(g):
    c, s, tx, ty = (float(v) for v in g)
    return [[c, -s, ty], [s, c, -tx], [0.0, 0.0, 1.0]]


def factor_terms(poses, i, j, z, sq, kind, param):
    """-> e [3], Ji, Jj [3][3] (weighted), w, and the whitened error before the robust loss"""
    ident = [[1.0 if r == c else 0.0 for c in range(3)] for r in range(3)]
    if j < 0:
        e = se2_log(O.se2_mul(O.se2_inverse(z), poses[i]))
        Ji, Jj = ident, [[0.0] * 3 for _ in range(3)]
    else:
        e = se2_log(O.se2_mul(O.se2_inverse(z), O.se2_mul(O.se2_inverse(poses[i]), poses[j])))
        Hinv, Hc = _adj(poses[i]), _adj(O.se2_inverse(poses[j]))
        Ji = [[(Hc[r][0] * -Hinv[0][c] + Hc[r][1] * -Hinv[1][c]) + Hc[r][2] * -Hinv[2][c] for c in range(3)] for r in range(3)]
        Jj = ident
    e = [e[r] * float(sq[r]) for r in range(3)]                                   # DiagonalLoss::weightInPlace
    Ji = [[Ji[r][c] * float(sq[r]) for c in range(3)] for r in range(3)]
    Jj = [[Jj[r][c] * float(sq[r]) for c in range(3)] for r in range(3)]
    white = list(e)
    w = 1.0
    if kind != NONE:                                                              # the robust loss after it
        n = math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        w = weight(kind, float(param), n)
        sqrtw = math.sqrt(w)
        e = [v * sqrtw for v in e]
        Ji = [[v * sqrtw for v in row] for row in Ji]
        Jj = [[v * sqrtw for v in row] for row in Jj]
    return e, Ji, Jj, w, white


def linearize(poses, fi, fj, meas, sq, kind=None, param=None):
    """-> dict(err [F,3], Hdiag [N,3,3], Hoff [F,3,3], b [N,3], chi2 (the oracle's running sum), esn (errorSquaredNorm: per-factor
    squared norms, summed), w [F], white [F,3] (the error before the robust loss), Ji, Jj [F,3,3])"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4)
    meas = np.asarray(meas, dtype=np.float64).reshape(-1, 4)
    sq = np.asarray(sq, dtype=np.float64).reshape(-1, 3)
    N, F = len(poses), len(fi)
    kind = np.zeros(F, dtype=np.int32) if kind is None else np.asarray(kind)
    param = np.zeros(F) if param is None else np.asarray(param, dtype=np.float64)
    err, white, w = np.zeros((F, 3)), np.zeros((F, 3)), np.ones(F)
    Hd = [[[0.0] * 3 for _ in range(3)] for _ in range(N)]
    bb = [[0.0] * 3 for _ in range(N)]
    Hoff, JI, JJ = np.zeros((F, 3, 3)), np.zeros((F, 3, 3)), np.zeros((F, 3, 3))
    chi2, esn = 0.0, 0.0
    for k in range(F):
        i, j = int(fi[k]), int(fj[k])
        e, Ji, Jj, w[k], white[k] = factor_terms(poses, i, j, meas[k], sq[k], int(kind[k]), param[k])
        err[k], JI[k], JJ[k] = e, Ji, Jj
        for r in range(3):
            chi2 += e[r] * e[r]
        esn += (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        for a in range(3):
            bb[i][a] -= (Ji[0][a] * e[0] + Ji[1][a] * e[1]) + Ji[2][a] * e[2]
            for c in range(3):
                Hd[i][a][c] += (Ji[0][a] * Ji[0][c] + Ji[1][a] * Ji[1][c]) + Ji[2][a] * Ji[2][c]
        if j >= 0:
            for a in range(3):
                bb[j][a] -= (Jj[0][a] * e[0] + Jj[1][a] * e[1]) + Jj[2][a] * e[2]
                for c in range(3):
                    Hd[j][a][c] += (Jj[0][a] * Jj[0][c] + Jj[1][a] * Jj[1][c]) + Jj[2][a] * Jj[2][c]
                    Hoff[k][a][c] = (Ji[0][a] * Jj[0][c] + Ji[1][a] * Jj[1][c]) + Ji[2][a] * Jj[2][c]
    return {"err": err, "Hdiag": np.array(Hd).reshape(N, 3, 3), "Hoff": Hoff, "b": np.array(bb).reshape(N, 3), "chi2": chi2, "esn": esn,
            "w": w, "white": white, "Ji": JI, "Jj": JJ}


def dense(N, fi, fj, lin):
    """The full symmetric Hessian [3N,3N]: the factors on one pair add up in factor order, as the reference's loop does"""
    H = np.zeros((3 * N, 3 * N))
    for v in range(N):
        H[3 * v:3 * v + 3, 3 * v:3 * v + 3] = lin["Hdiag"][v]
    for k in range(len(fi)):
        if fj[k] >= 0:
            i, j = int(fi[k]), int(fj[k])
            H[3 * i:3 * i + 3, 3 * j:3 * j + 3] += lin["Hoff"][k]
            H[3 * j:3 * j + 3, 3 * i:3 * i + 3] += lin["Hoff"][k].T
    return H


def levenberg_marquardt(lin_at, fi, fj, init, max_iterations=100):
    """tests/_pgo_lm.levenberg_marquardt with the linearisation pluggable: lin_at(poses) -> dict(Hdiag, Hoff, b, chi2).
    -> dict(status, iterations, trace, poses, initial_error, final_error)."""
    x = np.array(init, dtype=np.float64).reshape(-1, 4)
    N = len(x)
    lam, inc = 1e-5, 2.0
    err = lambda p: 0.5 * lin_at(p)["chi2"]
    last_err = err(x)
    out = {"initial_error": last_err, "trace": [], "iterations": 0}
    while out["iterations"] < max_iterations:
        lin = lin_at(x)
        H = dense(N, fi, fj, lin)
        g = lin["b"].reshape(-1)
        diag = np.diag(H).copy()
        curr = last_err
        last_lam, status, new_err = 0.0, ERROR_INCREASE, None
        while lam < 1e10:
            H[np.diag_indices_from(H)] += (lam - last_lam) * diag
            last_lam = lam
            try:
                dx = np.linalg.solve(H, g)
                ok = bool(np.all(np.isfinite(dx)))
            except np.linalg.LinAlgError:
                ok = False
            accepted = False
            if ok:
                cand = retract(x, dx.reshape(N, 3))
                e_new = err(cand)
                with np.errstate(invalid="ignore", divide="ignore"):
                    ratio = (curr - e_new) / (0.5 * dx.dot(lam * diag * dx + g))
                if ratio > 1e-3:
                    x, new_err, accepted = cand, e_new, True
                    lam *= max(1.0 / 3.0, 1.0 - (2.0 * ratio - 1.0) ** 3)
                    lam = max(1e-20, lam)
                    inc = 2.0
            out["trace"].append(ACCEPTED if accepted else (REJECTED if ok else RANK_DEFICIENT))
            if accepted:
                status = SUCCESS
                break
            lam *= inc
            inc *= 2.0
        out["iterations"] += 1
        if status != SUCCESS:
            out.update(status=status, poses=x, final_error=last_err)
            return out
        out["final_error"] = new_err
        if new_err - last_err > 1e-20:
            out.update(status=ERROR_INCREASE, poses=x)
            return out
        if (last_err - new_err) < 1e-5 or (last_err - new_err) / last_err < 1e-5:
            out.update(status=SUCCESS, poses=x)
            return out
        last_err = new_err
    out.update(status=MAX_ITERATION, poses=x)
    return out
