#!/usr/bin/env python
"""Generates tests/golden/robust_weights_golden.npz by RUNNING THE REFERENCE'S OWN src/nlls/robust_cost.cpp: for each of the five
RobustCost classes, a list of arguments x and what its value(x) returns.  tests/_match_batch_checks.robust_value -- the numpy
restatement the batched solver's sums are checked with -- must reproduce every value bit for bit
(tests/test_match_batch_sim.py).

The arguments: 0, a logarithmic sweep of 1e-9 .. 1e3 (the distances of a scan matcher are 0 .. l2_max metres), seeded uniform
samples of [0, 6], and for Huber(0.15) / Tukey(4.6851) the kink itself, one ulp below and one ulp above it.

The throw-away binding -- a driver of a dozen lines that prints value(x) in hexadecimal floating point -- is written, compiled
against the reference's sources (with the Eigen stand-in of oracle/ref_shim: Eigen3 is not installed here) and run in a temporary
directory OUTSIDE the repository; only the numbers come back.  Needs /root/reference.
Run from the repository root:  python tests/golden/make_robust_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
KINDS = [("unit", "UnitWeight", None), ("tukey", "TukeyWeight", 4.6851), ("tdist", "TDistributionWeight", 3.0),
         ("cauchy", "CauchyWeight", 0.3), ("huber", "HuberWeight", 0.15)]

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "lama/nlls/robust_cost.h"
int main(int argc, char** argv)
{
    const std::string kind(argv[1]);
    const double p = std::strtod(argv[2], nullptr);
    std::unique_ptr<lama::RobustCost> w;
    if (kind == "unit") w.reset(new lama::UnitWeight);
    else if (kind == "tukey") w.reset(new lama::TukeyWeight(p));
    else if (kind == "tdist") w.reset(new lama::TDistributionWeight(p));
    else if (kind == "cauchy") w.reset(new lama::CauchyWeight(p));
    else w.reset(new lama::HuberWeight(p));
    char line[128];
    while (std::fgets(line, sizeof line, stdin)) std::printf("%a\n", w->value(std::strtod(line, nullptr)));
    return 0;
}
"""


def arguments(kind, param):
    rng = np.random.default_rng(20)
    x = [np.array([0.0]), np.logspace(-9, 3, 97), rng.uniform(0.0, 6.0, 160)]
    if kind in ("huber", "tukey"):
        k = np.float64(param)
        x.append(np.array([np.nextafter(k, 0.0), k, np.nextafter(k, 9.0)]))
    return np.concatenate(x)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        open(src, "w").write(DRIVER)
        subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-I" + os.path.join(REF, "include"), "-I" + os.path.join(ROOT, "oracle", "ref_shim"),
                        src, os.path.join(REF, "src", "nlls", "robust_cost.cpp"), "-o", exe], check=True)
        for kind, _, param in KINDS:
            x = arguments(kind, param)
            r = subprocess.run([exe, kind, float(param or 0.0).hex()], input="".join(float(v).hex() + "\n" for v in x), capture_output=True, text=True, check=True)
            v = np.array([float.fromhex(s) for s in r.stdout.split()])
            assert len(v) == len(x)
            out[kind + "_x"], out[kind + "_value"], out[kind + "_param"] = x, v, np.float64(param or 0.0)
    np.savez_compressed(os.path.join(HERE, "robust_weights_golden.npz"), **out)
    print("wrote robust_weights_golden.npz:", {k: len(out[k + "_x"]) for k, _, _ in KINDS})


if __name__ == "__main__":
    sys.exit(main())
