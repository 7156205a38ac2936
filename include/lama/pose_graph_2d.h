// lama/pose_graph_2d.h -- lama::PoseGraph2D: a general SE2 pose graph with lama::SimplePGO's optimizer (not in the reference).
//
// Where SimplePGO builds the one graph of src/simple_pgo.cpp with its fixed sigmas, here every factor carries its own: a prior on
// a node or a relative pose between two nodes, three sigmas (x, y, theta of the factor's error, DiagonalLoss::Sigmas) and
// optionally a robust loss applied after that whitening -- minisam's ComposedLoss(DiagonalLoss, robust).  With sigmas of 1 it is the
// bare robust loss, exactly: the graph GraphSlam2D::optimizePoseGraph (src/graph_slam2d.cpp:214,224,266,394-430 of the reference)
// optimises is
//
//     lama::PoseGraph2D g;
//     for (const Pose2D& p : key_poses) g.addNode(p);
//     g.addPrior(0, key_poses[0], Vector3d(0.01, 0.01, 0.01));
//     for (int i = 0; i + 1 < n; ++i) g.addBetween(i, i + 1, key_poses[i] - key_poses[i + 1], Vector3d(0.25, 0.25, 0.15));
//     for (const Closure& c : closures)
//         g.addBetween(c.from, c.to, c.relative_pose, Vector3d(1, 1, 1), lama::PoseGraph2D::Loss::Huber(0.1));
//     if (g.optimize()) { /* g.nodes are the corrected poses; g.weights[k] < 1 marks a closure the loss held back */ }
//
// The error of addBetween(from, to, z) is log(z^-1 (x_from^-1 x_to)) (BetweenFactor<SE2d>), that of addPrior(node, z) is
// log(z^-1 x_node) (PriorFactor<SE2d>).
//
// optimize() has SimplePGO::optimize's contract: minisam's Levenberg-Marquardt with its default parameters, every residual,
// Jacobian, Hessian block and trial step computed by the device library (lama_hip_pgo_*, include/lama_hip.h); it returns true and
// writes `nodes` only when the optimizer reports SUCCESS, and returns false with report.status = -1 and nothing run for an empty
// graph (no node or no factor), a factor index outside `nodes`, a factor between a node and itself, a sigma that is not finite and
// > 0, an unknown loss kind or a robust loss whose parameter is not finite and > 0.  There is no CPU fallback: optimize() throws
// std::runtime_error when the device library or a HIP device is missing.
#pragma once

#include <cstdint>

#include "lama/pose2d.h"
#include "lama/simple_pgo.h"
#include "lama/types.h"

namespace lama {

struct PoseGraph2D {

    // A robust loss on the norm n of a factor's whitened error (vendor/minisam/minisam/core/LossFunction.h): the factor's error and
    // Jacobians are scaled by sqrt(w(n)).
    struct Loss {
        enum Kind : int32_t { KIND_NONE = 0, KIND_HUBER = 1, KIND_CAUCHY = 2, KIND_DCS = 3 };    // LAMA_HIP_PGO_LOSS_* (include/lama_hip.h)
        int32_t kind;
        double param;
        Loss() : kind(KIND_NONE), param(0.0) {}
        static Loss None() { return Loss(); }
        static Loss Huber(double k) { Loss l; l.kind = KIND_HUBER; l.param = k; return l; }      // w = n < k ? 1 : k / n
        static Loss Cauchy(double k) { Loss l; l.kind = KIND_CAUCHY; l.param = k; return l; }    // w = k^2 / (k^2 + n^2)
        static Loss DCS(double c) { Loss l; l.kind = KIND_DCS; l.param = c; return l; }         // w = n^2 > c ? (2c / (c + n^2))^2 : 1
    };

    struct Factor {
        int from = 0;
        int to = -1;                 // -1: a prior on `from`
        Pose2D measurement;
        Vector3d sigmas;
        Loss loss;
    };

    //>> Variables
    using NodeList = List<Pose2D>;
    using FactorList = List<Factor>;

    NodeList nodes;
    FactorList factors;

    // -> the new node's index
    int addNode(const Pose2D& pose);
    void addPrior(int node, const Pose2D& measurement, const Vector3d& sigmas, Loss loss = Loss());
    void addBetween(int from, int to, const Pose2D& measurement, const Vector3d& sigmas, Loss loss = Loss());

    bool optimize();

    int device = 0;                  // HIP device the graph lives on

    // what the last optimize() did, and how it solves its damped systems: as in lama::SimplePGO (include/lama/simple_pgo.h)
    using Report = SimplePGO::Report;
    Report report;
    enum LinearSolver { HostLDLT = 0, DevicePCG = 1 };
    LinearSolver linear_solver = HostLDLT;
    double pcg_rel_tol = 1e-10;        // stop at ||r|| <= pcg_rel_tol ||b||
    uint32_t pcg_max_iterations = 0;   // 0: max(100, 6 * nodes.size())

    // per factor, the weight w of its loss at the state the last optimize() ended in (whatever its status): 1 for a factor without
    // a loss or inside its loss's quadratic region.  Empty when optimize() did not run.
    DynamicArray<double> weights;
};

} // namespace lama
