"""Test infrastructure: the block-Jacobi preconditioned conjugate gradient of iris_lama_amd/csrc/lama_pgo_pcg.h restated in numpy with
the SAME order of every sum, so that dx, the iteration count, r.r and the model decrease of lama_hip_pgo_solve_pcg can be compared
for bit-equality (only +, -, *, / are involved and the library is built with -ffp-contract=off).  The order is the one written in
that file's header comment:

  * a 3x3 product:  y[a] = (B[a][0] p[0] + B[a][1] p[1]) + B[a][2] p[2]
  * a row of the product: terms t = 0 diagonal (damped: B[c][c] + lam * d[c]), then the lower blocks by ascending column, then the
    transposed blocks by ascending row; lane g of the row's 8 lanes adds the terms g, g + 8, ... from 0; xor tree 4, 2, 1
  * a dot product: per-workgroup partials (xor tree 32 .. 1 over each wave of 64, then the 4 waves in order), then the partials as
    k_pgo_sum adds them (lane l: l, l + 64, ... in order; xor tree 32 .. 1).  p.q has one workgroup per 32 rows (256 threads, lane 0 of
    each row's 8 carries the row's value), everything else one per 256 poses.
"""
import numpy as np

CONVERGED, CAP, BREAKDOWN = 0, 1, 2
GROUP = 8
DBL_MAX = float(np.finfo(np.float64).max)
_LANES = np.arange(64)


def _butterfly(v, offsets):
    """v[..., 64]: v += shfl_xor(v, o) for every offset in turn"""
    for o in offsets:
        v = v + v[..., _LANES ^ o]
    return v


def block_partials(per_thread):
    """per_thread: one value per thread of consecutive workgroups of 256 (padded with 0) -> one partial per workgroup"""
    n = len(per_thread)
    nb = max(1, (n + 255) // 256)
    v = np.zeros(nb * 256)
    v[:n] = per_thread
    red = _butterfly(v.reshape(nb, 4, 64), (32, 16, 8, 4, 2, 1))[:, :, 0]
    t = np.zeros(nb)
    for w in range(4):
        t = t + red[:, w]
    return t


def sum_partials(part):
    """k_pgo_sum without its factor 0.5 / pcg_sum"""
    t = np.zeros(64)
    for start in range(0, len(part), 64):
        chunk = part[start:start + 64]
        t[:len(chunk)] = t[:len(chunk)] + chunk
    return float(_butterfly(t, (32, 16, 8, 4, 2, 1))[0])


def _dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _matvec(M, p):
    """M [n,3,3], p [n,3] -> [n,3]"""
    return (M[:, :, 0] * p[:, 0:1] + M[:, :, 1] * p[:, 1:2]) + M[:, :, 2] * p[:, 2:3]


def _positive_finite(v):
    return bool(v > 0.0 and v <= DBL_MAX)


class Structure:
    """The term lists of the product for one lower pattern (row_ptr, cols): per term its row, lane, step, block, kind and source pose"""

    def __init__(self, row_ptr, cols):
        row_ptr, cols = np.asarray(row_ptr), np.asarray(cols)
        N = len(row_ptr) - 1
        self.N = N
        brow = np.repeat(np.arange(N), np.diff(row_ptr))
        trans = [[] for _ in range(N)]
        for q in range(len(cols)):                       # (ascending q = ascending row)
            if cols[q] != brow[q]:
                trans[cols[q]].append(q)
        rows, lanes, steps, blocks, kinds, srcs = [], [], [], [], [], []
        for r in range(N):
            terms = [(row_ptr[r], 0, r)] + [(q, 1, cols[q]) for q in range(row_ptr[r] + 1, row_ptr[r + 1])] + [(q, 2, brow[q]) for q in trans[r]]
            for t, (q, kind, src) in enumerate(terms):
                rows.append(r); lanes.append(t % GROUP); steps.append(t // GROUP); blocks.append(q); kinds.append(kind); srcs.append(src)
        self.rows, self.lanes, self.steps = np.array(rows), np.array(lanes), np.array(steps)
        self.blocks, self.kinds, self.srcs = np.array(blocks), np.array(kinds), np.array(srcs)
        self.by_step = [np.nonzero(self.steps == s)[0] for s in range(int(self.steps.max()) + 1)]
        self.diag_block = row_ptr[:-1]
        self.transposed = [len(t) for t in trans]


def pcg(row_ptr, cols, blocks, b, diag, lam, rel_tol=1e-10, max_iterations=None, structure=None):
    """-> dict(dx [N,3], iterations, rr, bb, rel_residual_sq, outcome, model_decrease)"""
    S = structure or Structure(row_ptr, cols)
    N = S.N
    blocks = np.asarray(blocks, dtype=np.float64).reshape(-1, 3, 3)
    b = np.asarray(b, dtype=np.float64).reshape(N, 3)
    d = np.asarray(diag, dtype=np.float64).reshape(N, 3)
    lam = float(lam)
    if max_iterations is None:
        max_iterations = max(100, 6 * N)
    # ---- k_pgo_pcg_setup
    M = blocks[S.diag_block].copy()
    for c in range(3):
        M[:, c, c] = M[:, c, c] + lam * d[:, c]
    m00, m11, m22, m10, m20, m21 = M[:, 0, 0], M[:, 1, 1], M[:, 2, 2], M[:, 1, 0], M[:, 2, 0], M[:, 2, 1]
    with np.errstate(all="ignore"):
        c00, c10, c20 = m11 * m22 - m21 * m21, m20 * m21 - m10 * m22, m10 * m21 - m20 * m11
        c11, c21, c22 = m00 * m22 - m20 * m20, m10 * m20 - m00 * m21, m00 * m11 - m10 * m10
        det = (m00 * c00 + m10 * c10) + m20 * c20
        pd = (m00 > 0) & (m00 <= DBL_MAX) & (c22 > 0) & (c22 <= DBL_MAX) & (det > 0) & (det <= DBL_MAX)
        safe = np.where(pd, det, 1.0)
        I = np.stack([c00, c10, c11, c20, c21, c22], axis=1) / safe[:, None]
    I[~pd] = 0.0
    fine = (I[:, 0] > 0.0) & np.all((I >= -DBL_MAX) & (I <= DBL_MAX), axis=1)
    I[~fine] = 0.0
    done = None if bool(np.all(fine)) else BREAKDOWN
    W = np.zeros((N, 3, 3))
    W[:, 0, 0], W[:, 0, 1], W[:, 0, 2] = I[:, 0], I[:, 1], I[:, 3]
    W[:, 1, 0], W[:, 1, 1], W[:, 1, 2] = I[:, 1], I[:, 2], I[:, 4]
    W[:, 2, 0], W[:, 2, 1], W[:, 2, 2] = I[:, 3], I[:, 4], I[:, 5]
    x = np.zeros((N, 3))
    r = b.copy()
    z = _matvec(W, r)
    p = z.copy()
    # ---- k_pgo_pcg_begin
    rho = sum_partials(block_partials(_dot3(r, z)))
    bb = sum_partials(block_partials(_dot3(b, b)))
    thresh = (rel_tol * rel_tol) * bb
    rr, iters = bb, 0
    if done is None:
        if bb == 0.0:
            done = CONVERGED
        elif not _positive_finite(bb) or not _positive_finite(rho):
            done = BREAKDOWN
    # the matrices of the terms (the blocks and lam are fixed for the solve)
    T = blocks[S.blocks].copy()
    T[S.kinds == 0] = M
    T[S.kinds == 2] = np.transpose(T[S.kinds == 2], (0, 2, 1))
    k = 0
    while done is None and k < max_iterations:
        # ---- k_pgo_pcg_spmv
        acc = np.zeros((N, GROUP, 3))
        for idx in S.by_step:
            acc[S.rows[idx], S.lanes[idx]] = acc[S.rows[idx], S.lanes[idx]] + _matvec(T[idx], p[S.srcs[idx]])
        for o in (4, 2, 1):
            acc = acc + acc[:, np.arange(GROUP) ^ o]
        q = acc[:, 0]
        per_thread = np.zeros((N, GROUP))
        per_thread[:, 0] = _dot3(p, q)
        pq = sum_partials(block_partials(per_thread.reshape(-1)))
        # ---- k_pgo_pcg_step / k_pgo_pcg_dir
        if not _positive_finite(pq):
            done = BREAKDOWN
            break
        alpha = rho / pq
        x = x + alpha * p
        r = r - alpha * q
        z = _matvec(W, r)
        rr = sum_partials(block_partials(_dot3(r, r)))
        rz = sum_partials(block_partials(_dot3(r, z)))
        iters = k + 1
        if rr <= thresh:
            done = CONVERGED
            break
        beta = rz / rho
        p = z + beta * p
        rho = rz
        k += 1
    # ---- k_pgo_pcg_model, k_pgo_sum
    t = x * ((lam * d) * x + b)
    model = 0.5 * sum_partials(block_partials((t[:, 0] + t[:, 1]) + t[:, 2]))
    return {"dx": x, "iterations": iters, "rr": rr, "bb": bb, "rel_residual_sq": 0.0 if bb == 0.0 else rr / bb,
            "outcome": CAP if done is None else done, "model_decrease": model}


def apply_system(row_ptr, cols, blocks, diag, lam, x):
    """(H + lam D) x from the lower blocks, in any order (the residual checks)"""
    row_ptr, cols = np.asarray(row_ptr), np.asarray(cols)
    N = len(row_ptr) - 1
    blocks = np.asarray(blocks).reshape(-1, 3, 3)
    x = np.asarray(x).reshape(N, 3)
    brow = np.repeat(np.arange(N), np.diff(row_ptr))
    y = lam * np.asarray(diag).reshape(N, 3) * x
    np.add.at(y, brow, np.einsum("qab,qb->qa", blocks, x[cols]))
    off = brow != cols
    np.add.at(y, cols[off], np.einsum("qba,qb->qa", blocks[off], x[brow[off]]))
    return y
