// lama/simple_pgo.h -- lama::SimplePGO: the reference's pose-graph optimizer (include/lama/simple_pgo.h, src/simple_pgo.cpp:48-105).
//
// Given a list of nodes, edges and fixed nodes it calculates the nodes' poses that minimise the graph error: a prior on node 0
// (sigmas 1, 1, 1) -- or one prior per fixed node (sigmas 0.1) --, odometry between consecutive nodes and the loop closures of
// edge_list (sigmas 0.5, 0.5, 0.1), solved by minisam's Levenberg-Marquardt with its default parameters.  Here the poses stay on the
// GPU for the whole optimize(): the residuals, the Jacobians, the assembled Hessian blocks and every trial step are computed by the
// device library (lama_hip_pgo_*, include/lama_hip.h); the sparse LDL^T factorisation runs on the host unless linear_solver (below)
// asks for the device's conjugate gradient in its place.  There is no CPU fallback:
// optimize() throws std::runtime_error when the device library or a HIP device is missing.
//
// optimize() returns true and writes the result into node_list only when the optimizer reports SUCCESS; any other status
// (MAX_ITERATION after 100 iterations, ERROR_INCREASE -- also for a graph already at its optimum --, RANK_DEFICIENCY) returns false
// and leaves node_list untouched.  So do an empty node_list and an edge or fixed index outside node_list (undefined behaviour in the
// reference), and an edge from a node to itself.
#pragma once

#include <cstdint>
#include <utility>

#include "lama/pose2d.h"
#include "lama/types.h"

namespace lama {

struct SimplePGO {

    //>> Variables
    using NodeList = List<Pose2D>;
    using EdgeList = List<std::pair<int, std::pair<int, Pose2D>>>;
    using FixedList = List<std::pair<int, Pose2D>>;

    NodeList node_list;
    EdgeList edge_list;
    FixedList fixed_list;

    bool optimize();

    // ---- additions (not in the reference)
    int device = 0;                  // HIP device the graph lives on

    // what the last optimize() did
    struct Report {
        int32_t status = -1;         // minisam's NonlinearOptimizationStatus: 0 SUCCESS, 1 MAX_ITERATION, 2 ERROR_INCREASE,
                                     // 3 RANK_DEFICIENCY, 4 INVALID; -1: not run (invalid input)
        uint32_t iterations = 0;
        uint32_t tries = 0;          // damped linear solves (LM lambda tries) over all iterations
        double initial_error = 0.0;  // 0.5 * sum of squared whitened errors
        double final_error = 0.0;
        uint64_t nnz_L = 0;          // scalar nonzeros of the strictly lower factor under the fill-reducing ordering
        double ms_device_linearize = 0.0;   // device: residuals, Jacobians, Hessian assembly (kernel time, summed)
        double ms_device_try = 0.0;         // device: retract + error of the trial steps (kernel time, summed)
        double ms_analyze = 0.0;            // host: ordering and symbolic factorisation (once)
        double ms_factorize = 0.0;          // host: numeric factorisation and solve (every try)
        double ms_total = 0.0;
        DynamicArray<int8_t> trace;         // per try: 1 accepted, 0 rejected (no gain), 2 rank deficient
        // linear_solver = DevicePCG (all zero otherwise)
        uint64_t pcg_iterations = 0;        // conjugate-gradient iterations, summed over the tries
        uint32_t pcg_max_iterations_seen = 0;   // the longest solve
        uint32_t pcg_fallbacks = 0;         // tries that reached the iteration cap and went to the host LDL^T instead
        double ms_device_solve = 0.0;       // device: the solves (summed)
    };
    Report report;

    // How the damped system (H + lambda diag(H)) dx = b of every Levenberg-Marquardt try is solved.
    //   HostLDLT  : the sparse LDL^T on the host (the default; what the lines above describe).
    //   DevicePCG : a conjugate gradient preconditioned by the damped 3x3 diagonal blocks, on the device (lama_hip_pgo_solve_pcg):
    //               nothing is factorised, the system and the step never leave the device.  The right choice for graphs with many
    //               loop closures, whose factor fills in; a chain with few closures needs thousands of iterations and has no fill --
    //               leave those to HostLDLT.  A try whose solve reaches pcg_max_iterations is solved by the host LDL^T instead
    //               (report.pcg_fallbacks counts them); optimize() throws std::runtime_error when the device library lacks the solver.
    enum LinearSolver { HostLDLT = 0, DevicePCG = 1 };
    LinearSolver linear_solver = HostLDLT;
    double pcg_rel_tol = 1e-10;        // stop at ||r|| <= pcg_rel_tol ||b||
    uint32_t pcg_max_iterations = 0;   // 0: max(100, 6 * node_list.size())
};

} // namespace lama
