#!/usr/bin/env python
"""Generates tests/golden/robust_pgo_golden.npz by RUNNING MINISAM'S OWN loss functions and linearisation: small SE2 pose graphs of
PriorFactor<SE2d> / BetweenFactor<SE2d> whose factors carry HuberLoss, CauchyLoss or DCSLoss alone, each of them composed after
DiagonalLoss::Sigmas (ComposedLoss), or the plain DiagonalLoss; for each graph the lower-Hessian linearisation (H, b), every
factor's weightedError and FactorGraph::errorSquaredNorm.  tests/_pgo_robust.py -- the restatement the device kernels are checked
with -- must reproduce every value bit for bit (tests/test_robust_pgo_golden.py).

The cases:
  graph6      6 poses, 27 factors: every robust kind alone and composed, as an inlier (w = 1, or close to 1 for Cauchy) and as an
              outlier, priors with and without a loss among them, plain DiagonalLoss factors between.
  huber_*     one prior, unit sigmas, rotation 0, error (t, 0, 0) -- the norm is t exactly -- with t one ulp below k, k, one ulp
              above k: Huber's `n < k`.
  dcs_*       the same with t * t one step below c, equal to c, one step above c: DCS's `e2 > c`.

The throw-away driver below is written, compiled with the minisam sources oracle/Makefile.ref lists as MINISAM_SRC (against the
Eigen stand-in of oracle/ref_shim: Eigen3 is not installed here) and run in a temporary directory OUTSIDE the repository; only the
numbers come back, as hexadecimal floating point.  Needs /root/reference and the CPU oracle (tests/_oracle.py) for the group
operations that build the inputs.
Run from the repository root:  python tests/golden/make_robust_pgo_golden.py
"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import _oracle as O  # noqa: E402
import _pgo_robust as R  # noqa: E402

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>
#include <minisam/core/FactorGraph.h>
#include <minisam/core/LossFunction.h>
#include <minisam/core/VariableOrdering.h>
#include <minisam/core/Variables.h>
#include <minisam/geometry/Sophus.h>
#include <minisam/nonlinear/SparsityPattern.h>
#include <minisam/nonlinear/linearization.h>
#include <minisam/slam/BetweenFactor.h>
#include <minisam/slam/PriorFactor.h>
#include "lama/pose2d.h"
namespace sam = minisam;
using lama::SE2d;
static double rd() { char t[64]; if (std::scanf("%63s", t) != 1) std::exit(2); return std::strtod(t, nullptr); }
static int ri() { int v; if (std::scanf("%d", &v) != 1) std::exit(2); return v; }
static SE2d pose()      // the state as given, bit for bit (no renormalisation)
{
    SE2d g;
    const double c = rd(), s = rd(), x = rd(), y = rd();
    g.so2().data()[0] = c; g.so2().data()[1] = s;
    g.translation() = Eigen::Vector2d(x, y);
    return g;
}
int main()
{
    const int N = ri(), F = ri();
    sam::Variables values;
    for (int i = 0; i < N; ++i) values.add(sam::key('x', (size_t)i), pose());
    sam::FactorGraph graph;
    for (int k = 0; k < F; ++k) {
        const int i = ri(), j = ri();
        const SE2d z = pose();
        Eigen::VectorXd sig(3);
        sig << 0, 0, 0;
        for (int r = 0; r < 3; ++r) sig(r) = rd();
        const int kind = ri();
        const double p = rd();
        const int composed = ri();
        std::shared_ptr<sam::LossFunction> robust, loss;
        if (kind == 1) robust = sam::HuberLoss::Huber(p);
        if (kind == 2) robust = sam::CauchyLoss::Cauchy(p);
        if (kind == 3) robust = sam::DCSLoss::DCS(p);
        if (!robust) loss = sam::DiagonalLoss::Sigmas(sig);
        else if (composed) loss = sam::ComposedLoss::Compose(sam::DiagonalLoss::Sigmas(sig), robust);
        else loss = robust;
        if (j < 0) graph.add(sam::PriorFactor<SE2d>(sam::key('x', (size_t)i), z, loss));
        else graph.add(sam::BetweenFactor<SE2d>(sam::key('x', (size_t)i), sam::key('x', (size_t)j), z, loss));
    }
    const sam::VariableOrdering ordering = values.defaultVariableOrdering();
    const sam::internal::LowerHessianSparsityPattern sparsity = sam::internal::constructLowerHessianSparsity(graph, values, ordering);
    Eigen::SparseMatrix<double> AtA;
    Eigen::VectorXd Atb;
    sam::internal::linearzationLowerHessian(graph, values, sparsity, AtA, Atb);
    std::vector<int> col((size_t)N), pose_of((size_t)3 * N), comp_of((size_t)3 * N);
    for (int i = 0; i < N; ++i) col[i] = sparsity.var_col[ordering.searchKey(sam::key('x', (size_t)i))];
    for (int i = 0; i < N; ++i) for (int a = 0; a < 3; ++a) { pose_of[(size_t)col[i] + a] = i; comp_of[(size_t)col[i] + a] = a; }
    const size_t n3 = (size_t)3 * N;
    std::vector<double> H(n3 * n3, 0.0);
    const int* outer = AtA.outerIndexPtr(); const int* inner = AtA.innerIndexPtr(); const double* val = AtA.valuePtr();
    for (int j = 0; j < (int)n3; ++j)
        for (int q = outer[j]; q < outer[j + 1]; ++q) {
            const int i = inner[q];
            const size_t r = (size_t)3 * pose_of[(size_t)i] + comp_of[(size_t)i], c = (size_t)3 * pose_of[(size_t)j] + comp_of[(size_t)j];
            H[r * n3 + c] = val[q];
            H[c * n3 + r] = val[q];
        }
    for (size_t q = 0; q < n3 * n3; ++q) std::printf("%a\n", H[q]);
    for (int i = 0; i < N; ++i) for (int a = 0; a < 3; ++a) std::printf("%a\n", Atb((size_t)col[i] + a));
    for (int k = 0; k < F; ++k) {
        const Eigen::VectorXd e = graph.factors()[k]->weightedError(values);
        for (int a = 0; a < 3; ++a) std::printf("%a\n", e(a));
    }
    std::printf("%a\n", graph.errorSquaredNorm(values));
    return 0;
}
"""


def minisam_sources():
    text = open(os.path.join(ROOT, "oracle", "Makefile.ref")).read().replace("\\\n", " ")
    m = re.search(r"^MINISAM_SRC\s*:=\s*(.*)$", text, re.M)
    return [os.path.join(REF, "vendor", "minisam", "minisam", s) for s in m.group(1).split()]


def graph6():
    """-> dict of inputs.  sigmas of a factor whose robust loss stands alone are 1 (sqrt_info = 1: the bare loss, exactly)."""
    rng = np.random.default_rng(66)
    N = 6
    truth = np.stack([O.se2(*rng.uniform(-4, 4, 2), rng.uniform(-3, 3)) for _ in range(N)])
    poses = np.stack([O.se2_mul(truth[v], O.se2(*rng.normal(0, [0.001, 0.001, 0.0003]))) for v in range(N)])
    K = {R.HUBER: 0.1, R.CAUCHY: 0.3, R.DCS: 0.5}
    spec = []                                       # (i, j, kind, composed, outlier, sigmas)
    pairs = [(a, b) for a in range(N) for b in range(N) if a != b]
    rng.shuffle(pairs)
    pairs = [tuple(int(v) for v in p) for p in pairs]
    q = 0
    for kind in (R.HUBER, R.CAUCHY, R.DCS):
        for composed in (0, 1):
            for outlier in (0, 1):
                i, j = pairs[q]; q += 1
                spec.append((i, j, kind, composed, outlier, (0.25, 0.25, 0.15) if composed else (1.0, 1.0, 1.0)))
    for kind, composed, outlier in ((R.HUBER, 0, 1), (R.CAUCHY, 1, 0), (R.DCS, 1, 1)):          # priors with a loss
        spec.append((len(spec) % N, -1, kind, composed, outlier, (0.1, 0.1, 0.1) if composed else (1.0, 1.0, 1.0)))
    spec.append((0, -1, R.NONE, 0, 0, (0.01, 0.01, 0.01)))                                        # plain DiagonalLoss
    for v in range(N - 1):
        spec.append((v, v + 1, R.NONE, 0, 0, (0.25, 0.25, 0.15)))
    for _ in range(6):
        i, j = pairs[q]; q += 1
        spec.append((i, j, R.NONE, 0, 0, (0.5, 0.5, 0.1)))
    order = rng.permutation(len(spec))              # the kinds interleave in factor order
    spec = [spec[k] for k in order]
    fi = np.array([s[0] for s in spec], dtype=np.int32)
    fj = np.array([s[1] for s in spec], dtype=np.int32)
    kind = np.array([s[2] for s in spec], dtype=np.int32)
    composed = np.array([s[3] for s in spec], dtype=np.int32)
    sig = np.array([s[5] for s in spec], dtype=np.float64)
    param = np.array([K.get(s[2], 0.0) for s in spec])
    meas = []
    for (i, j, kd, cp, outlier, sg) in spec:
        rel = truth[i] if j < 0 else O.se2_mul(O.se2_inverse(truth[i]), truth[j])
        # an inlier measures the truth to a hundredth of its sigmas; an outlier is metres and a large angle off
        off = O.se2(*(rng.normal(0, 1, 3) * np.array(sg) * 0.01)) if not outlier else O.se2(1.5, -2.0, 0.9)
        meas.append(O.se2_mul(rel, off))
    return dict(poses=poses, fi=fi, fj=fj, meas=np.array(meas), sigmas=sig, kind=kind, param=param, composed=composed,
                outlier=np.array([s[4] for s in spec], dtype=np.int32))


def threshold_case(kind, param, t):
    return dict(poses=np.array([[1.0, 0.0, t, 0.0]]), fi=np.array([0], dtype=np.int32), fj=np.array([-1], dtype=np.int32),
                meas=np.array([[1.0, 0.0, 0.0, 0.0]]), sigmas=np.ones((1, 3)), kind=np.array([kind], dtype=np.int32),
                param=np.array([param]), composed=np.array([0], dtype=np.int32), outlier=np.array([0], dtype=np.int32))


def cases():
    out = {"graph6": graph6()}
    k = np.float64(0.1)
    for name, t in (("below", np.nextafter(k, 0.0)), ("at", k), ("above", np.nextafter(k, 1.0))):
        out["huber_" + name] = threshold_case(R.HUBER, float(k), float(t))
    t0 = np.float64(0.7)
    c = float(t0 * t0)
    for name, t in (("below", np.nextafter(t0, 0.0)), ("at", t0), ("above", np.nextafter(t0, 1.0))):
        out["dcs_" + name] = threshold_case(R.DCS, c, float(t))
    assert float(np.nextafter(t0, 0.0)) ** 2 < c < float(np.nextafter(t0, 1.0)) ** 2
    return out


def run(exe, c):
    N, F = len(c["poses"]), len(c["fi"])
    hx = lambda a: " ".join(float(v).hex() for v in np.ravel(a))
    lines = [f"{N} {F}"] + [hx(p) for p in c["poses"]]
    for k in range(F):
        lines.append(f"{c['fi'][k]} {c['fj'][k]} {hx(c['meas'][k])} {hx(c['sigmas'][k])} {c['kind'][k]} {float(c['param'][k]).hex()} {c['composed'][k]}")
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    v = np.array([float.fromhex(s) for s in r.stdout.split()])
    n3 = 3 * N
    assert len(v) == n3 * n3 + n3 + 3 * F + 1, (len(v), N, F)
    return dict(H=v[:n3 * n3].reshape(n3, n3), b=v[n3 * n3:n3 * n3 + n3].reshape(N, 3), werr=v[n3 * n3 + n3:-1].reshape(F, 3), esn=v[-1])


def main():
    all_cases = cases()
    names = sorted(all_cases)
    results = {}
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        open(src, "w").write(DRIVER)
        subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-w", "-pthread", "-I" + os.path.join(ROOT, "oracle", "ref_shim"),
                        "-I" + os.path.join(REF, "include"), "-I" + os.path.join(REF, "vendor", "minisam"), src] + minisam_sources() +
                       ["-o", exe], check=True)
        for name in names:
            results[name] = run(exe, all_cases[name])
    # one array per field, the cases one after the other in the order of `names` (load_cases in tests/_pgo_robust_checks.py
    # splits them again by num_poses / num_factors): a few kilobytes instead of a zip member per case and field
    out = {"names": np.array(names), "num_poses": np.array([len(all_cases[n]["poses"]) for n in names], dtype=np.int32),
           "num_factors": np.array([len(all_cases[n]["fi"]) for n in names], dtype=np.int32)}
    for field in ("poses", "fi", "fj", "meas", "sigmas", "kind", "param", "composed", "outlier"):
        out[field] = np.concatenate([np.ravel(all_cases[n][field]) for n in names])
    for field in ("H", "b", "werr"):
        out[field] = np.concatenate([np.ravel(results[n][field]) for n in names])
    out["esn"] = np.array([results[n]["esn"] for n in names])
    # the cases are what they claim (by the restatement, which the golden test pins to the numbers above)
    g = all_cases["graph6"]
    lin = R.linearize(g["poses"], g["fi"], g["fj"], g["meas"], 1.0 / g["sigmas"], g["kind"], g["param"])
    rob = g["kind"] != R.NONE
    assert np.all(lin["w"][rob & (g["outlier"] == 1)] < 0.5), lin["w"]
    assert np.all(lin["w"][rob & (g["outlier"] == 0) & (g["kind"] != R.CAUCHY)] == 1.0), lin["w"]
    assert np.all(lin["w"][rob & (g["outlier"] == 0) & (g["kind"] == R.CAUCHY)] > 0.95), lin["w"]
    np.savez_compressed(os.path.join(HERE, "robust_pgo_golden.npz"), **out)
    print("wrote robust_pgo_golden.npz:", {n: len(all_cases[n]["fi"]) for n in sorted(all_cases)},
          os.path.getsize(os.path.join(HERE, "robust_pgo_golden.npz")), "bytes")


if __name__ == "__main__":
    sys.exit(main())
