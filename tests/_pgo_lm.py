"""Test infrastructure: lama::SimplePGO restated in numpy -- the reference's graph (src/simple_pgo.cpp:48-105) and minisam's
Levenberg-Marquardt with its default parameters, dense.  The linear system comes from the CPU oracle (O.pgo_linearize, pinned to
minisam's own linearisation by tests/test_oracle_vs_reference.py).  Lines cited are under vendor/minisam/minisam/nonlinear/."""
import numpy as np

import _oracle as O

SUCCESS, MAX_ITERATION, ERROR_INCREASE, RANK_DEFICIENCY = 0, 1, 2, 3
REJECTED, ACCEPTED, RANK_DEFICIENT = 0, 1, 2


def build_graph(nodes, edges=(), fixed=()):
    """simple_pgo.cpp:48-105: fi, fj (-1: prior), meas [F,4], sqrt_info [F,3] = 1 / sigma (DiagonalLoss::Sigmas)."""
    nodes = np.asarray(nodes, dtype=np.float64).reshape(-1, 4)
    fi, fj, meas, sq = [], [], [], []
    if len(fixed) == 0:
        fi.append(0); fj.append(-1); meas.append(nodes[0]); sq.append(1.0 / np.array([1.0, 1.0, 1.0]))
    else:
        for idx, pose in fixed:
            fi.append(idx); fj.append(-1); meas.append(np.asarray(pose, dtype=np.float64)); sq.append(1.0 / np.array([0.1, 0.1, 0.1]))
    for i in range(len(nodes) - 1):                      # node_list[i] - node_list[i+1] = x_i^-1 x_{i+1} (Pose2D::operator-)
        fi.append(i); fj.append(i + 1); meas.append(O.se2_mul(O.se2_inverse(nodes[i]), nodes[i + 1]))
        sq.append(1.0 / np.array([0.5, 0.5, 0.1]))
    for a, b, pose in edges:
        fi.append(a); fj.append(b); meas.append(np.asarray(pose, dtype=np.float64)); sq.append(1.0 / np.array([0.5, 0.5, 0.1]))
    return (np.array(fi, dtype=np.int32), np.array(fj, dtype=np.int32), np.array(meas).reshape(-1, 4), np.array(sq).reshape(-1, 3))


def lower_pattern(N, fi, fj):
    """The lower block-CSR pattern of the device (include/lama_hip.h, lama_hip_pgo_pattern): row r = diagonal, then the distinct
    c < r sharing a between factor, ascending.  -> row_ptr, cols, contributions (per block: [(factor, transposed)] in factor order)."""
    rows = [dict() for _ in range(N)]
    for k in range(len(fi)):
        if fj[k] >= 0:
            i, j = int(fi[k]), int(fj[k])
            rows[max(i, j)].setdefault(min(i, j), []).append((k, i < j))
    row_ptr, cols, contrib = [0], [], []
    for r in range(N):
        cols.append(r); contrib.append(None)
        for c in sorted(rows[r]):
            cols.append(c); contrib.append(rows[r][c])
        row_ptr.append(len(cols))
    return np.array(row_ptr, dtype=np.int32), np.array(cols, dtype=np.int32), contrib


def scatter_blocks(lin, cols, contrib, row_ptr):
    """The blocks of the lower pattern from the per-variable / per-factor outputs of a linearisation, in factor order."""
    blocks = np.zeros((len(cols), 3, 3))
    for r in range(len(row_ptr) - 1):
        for q in range(row_ptr[r], row_ptr[r + 1]):
            if contrib[q] is None:
                blocks[q] = lin["Hdiag"][r]
            else:
                acc = np.zeros((3, 3))
                for k, tr in contrib[q]:
                    acc = acc + (lin["Hoff"][k].T if tr else lin["Hoff"][k])
                blocks[q] = acc
    return blocks


def _dense(N, fi, fj, lin):
    H = np.zeros((3 * N, 3 * N))
    for v in range(N):
        H[3 * v:3 * v + 3, 3 * v:3 * v + 3] += lin["Hdiag"][v]
    for k in range(len(fi)):
        if fj[k] >= 0:
            i, j = int(fi[k]), int(fj[k])
            H[3 * i:3 * i + 3, 3 * j:3 * j + 3] += lin["Hoff"][k]
            H[3 * j:3 * j + 3, 3 * i:3 * i + 3] += lin["Hoff"][k].T
    return H


def retract(x, dx):
    """x_v * exp(dx_v) (geometry/Sophus.h:52-56)."""
    return np.stack([O.se2_mul(x[v], O.se2_exp(dx[v])) for v in range(len(x))])


def levenberg_marquardt(fi, fj, meas, sq, init, max_iterations=100):
    """-> dict(status, iterations, trace, poses, initial_error, final_error).  Defaults: NonlinearOptimizer.h:54-60,
    LevenbergMarquardtOptimizer.h:20-36; reset() LevenbergMarquardtOptimizer.cpp:35-44."""
    x = np.array(init, dtype=np.float64).reshape(-1, 4)
    N = len(x)
    lam, inc = 1e-5, 2.0
    err = lambda p: 0.5 * O.pgo_linearize(p, fi, fj, meas, sq)["chi2"]
    last_err = err(x)                                                   # NonlinearOptimizer.cpp:180
    out = {"initial_error": last_err, "trace": [], "iterations": 0, "ratios": []}
    while out["iterations"] < max_iterations:                           # NonlinearOptimizer.cpp:189
        lin = O.pgo_linearize(x, fi, fj, meas, sq)                      # iterate(): linearise once (LM.cpp:56-80)
        H = _dense(N, fi, fj, lin)
        g = lin["b"].reshape(-1)
        diag = np.diag(H).copy()                                        # undamped hessian_diag (LM.cpp:83-85)
        curr = last_err
        last_lam, status, new_err = 0.0, ERROR_INCREASE, None
        while lam < 1e10:                                               # LM.cpp:117
            H[np.diag_indices_from(H)] += (lam - last_lam) * diag       # dumpLinearSystem_ (LM.cpp:265-318, 369-374)
            last_lam = lam
            try:                                                        # (SimplicialLDLT NumericalIssue -> RANK_DEFICIENCY)
                dx = np.linalg.solve(H, g)
                ok = bool(np.all(np.isfinite(dx)))
            except np.linalg.LinAlgError:
                ok = False
            accepted = False
            if ok:
                cand = retract(x, dx.reshape(N, 3))
                e_new = err(cand)
                with np.errstate(invalid="ignore", divide="ignore"):   # (0 / 0 at the optimum: NaN, a rejection)
                    ratio = (curr - e_new) / (0.5 * dx.dot(lam * diag * dx + g))   # tryLambda_ (LM.cpp:219-236)
                out["ratios"].append((lam, curr - e_new, ratio))
                if ratio > 1e-3:
                    x, new_err, accepted = cand, e_new, True
                    lam *= max(1.0 / 3.0, 1.0 - (2.0 * ratio - 1.0) ** 3)     # decreaseLambda_ (LM.cpp:327-333)
                    lam = max(1e-20, lam)
                    inc = 2.0
            out["trace"].append(ACCEPTED if accepted else (REJECTED if ok else RANK_DEFICIENT))
            if accepted:
                status = SUCCESS
                break
            lam *= inc                                                  # increaseLambda_ (LM.cpp:321-324)
            inc *= 2.0
        out["iterations"] += 1
        if status != SUCCESS:
            out.update(status=status, poses=x, final_error=last_err)
            return out
        out["final_error"] = new_err
        if new_err - last_err > 1e-20:                                  # NonlinearOptimizer.cpp:217
            out.update(status=ERROR_INCREASE, poses=x)
            return out
        if (last_err - new_err) < 1e-5 or (last_err - new_err) / last_err < 1e-5:   # errorStopCondition_ (:237-240)
            out.update(status=SUCCESS, poses=x)
            return out
        last_err = new_err
    out.update(status=MAX_ITERATION, poses=x)
    return out


def iterations_of(trace):
    """The trace split into LM iterations: each ends with its accepted try (the last one may end without)."""
    its, cur = [], []
    for t in trace:
        cur.append(int(t))
        if t == ACCEPTED:
            its.append(cur)
            cur = []
    if cur:
        its.append(cur)
    return its


def assert_same_run(got, ref):
    """Same status, iteration count and accept/reject sequence.  The one allowance: the tries of the LAST iteration may differ in
    number when it ends with an accepted step.  By then the state is at the optimum to the solver's rounding, the tries compare error
    changes of ~1e-9 made of that rounding (the sparse LDL^T and the dense solve round differently), and which large lambda first
    shows a gain is noise; either way that iteration accepts and the stop test ends the run."""
    assert got["status"] == ref["status"] and got["iterations"] == ref["iterations"], (got["status"], ref["status"], got["iterations"], ref["iterations"])
    a, b = iterations_of(got["trace"]), iterations_of(ref["trace"])
    assert len(a) == len(b) and a[:-1] == b[:-1], (a, b)
    assert a[-1] == b[-1] or (a[-1][-1] == b[-1][-1] == ACCEPTED and got["status"] == SUCCESS), (a[-1], b[-1])
