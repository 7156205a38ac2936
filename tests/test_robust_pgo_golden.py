"""tests/_pgo_robust.py -- the scalar restatement of the pose-graph linearisation with per-factor robust losses, which the device
kernels are checked with (tests/_pgo_robust_checks.py) -- against minisam's own code: tests/golden/robust_pgo_golden.npz holds what
the reference's HuberLoss / CauchyLoss / DCSLoss, alone and composed after DiagonalLoss, its lower-Hessian linearisation and its
errorSquaredNorm return (tests/golden/make_robust_pgo_golden.py).  No device, no reference tree."""
import numpy as np
import pytest

import _oracle as O
import _pgo_robust as R
import _pgo_robust_checks as RC
from _posegraph import make_graph


@pytest.fixture(scope="module")
def cases():
    return RC.load_cases()


def test_golden_holds_every_kind_alone_composed_inlier_outlier_and_the_thresholds(cases):
    g = cases["graph6"]
    assert len(g["poses"]) == 6
    seen = {(int(k), int(c), int(o)) for k, c, o in zip(g["kind"], g["composed"], g["outlier"]) if k}
    assert seen == {(k, c, o) for k in (1, 2, 3) for c in (0, 1) for o in (0, 1)}
    assert ((g["fj"] < 0) & (g["kind"] != 0)).sum() == 3 and ((g["fj"] < 0) & (g["kind"] == 0)).sum() == 1
    assert np.all(g["sigmas"][(g["kind"] != 0) & (g["composed"] == 0)] == 1.0) and (g["kind"] == 0).sum() >= 10
    k = cases["huber_at"]["param"][0]
    assert [cases["huber_" + n]["poses"][0, 2] for n in ("below", "at", "above")] == [np.nextafter(k, 0), k, np.nextafter(k, 1)]
    c = cases["dcs_at"]["param"][0]
    t = [cases["dcs_" + n]["poses"][0, 2] for n in ("below", "at", "above")]
    assert t[0] * t[0] < c == t[1] * t[1] < t[2] * t[2] and t[0] == np.nextafter(t[1], 0) and t[2] == np.nextafter(t[1], 1)


def test_restatement_reproduces_minisam_bit_for_bit(cases):
    for name, c in cases.items():
        lin = R.linearize(c["poses"], c["fi"], c["fj"], c["meas"], c["sq"], c["kind"], c["param"])
        assert np.array_equal(lin["err"], c["werr"]), (name, "weighted errors")
        assert np.array_equal(R.dense(len(c["poses"]), c["fi"], c["fj"], lin), c["H"]), (name, "H")
        assert np.array_equal(lin["b"], c["b"]), (name, "b")
        assert lin["esn"] == c["esn"], (name, "errorSquaredNorm", lin["esn"], c["esn"])


def test_thresholds_fall_on_the_references_side(cases):
    w = {n: R.linearize(c["poses"], c["fi"], c["fj"], c["meas"], c["sq"], c["kind"], c["param"])["w"][0] for n, c in cases.items() if n != "graph6"}
    assert w["huber_below"] == 1.0 and w["huber_at"] == 1.0 and w["huber_above"] < 1.0      # (at n = k: k / n, which is 1)
    assert w["dcs_below"] == 1.0 and w["dcs_at"] == 1.0 and w["dcs_above"] < 1.0
    # and the reference's errors say the same: scaled by sqrt(w) only above the threshold
    for n, c in cases.items():
        if n != "graph6":
            assert (c["werr"][0, 0] == c["poses"][0, 2]) == (not n.endswith("above")), n


def test_without_losses_the_restatement_is_the_oracle_bit_for_bit():
    fi, fj, meas, sq, truth, init = make_graph(60, 80, seed=12)
    orc = O.pgo_linearize(init, fi, fj, meas, sq)
    for kw in ({}, {"kind": np.zeros(len(fi), np.int32), "param": np.full(len(fi), 0.1)}):
        lin = R.linearize(init, fi, fj, meas, sq, **kw)
        for k in ("err", "Hdiag", "Hoff", "b"):
            assert np.array_equal(lin[k], orc[k]), k
        assert lin["chi2"] == orc["chi2"] and np.all(lin["w"] == 1.0)
