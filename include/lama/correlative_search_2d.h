// lama/correlative_search_2d.h -- lama::CorrelativeSearch2D: exhaustive search of a pose lattice against a distance map on the device
// (correlative scan matching, Olson 2009), the stage that PRODUCES the start pose the Gauss-Newton registration needs.
//
// An addition: the reference has no such class.  Its global search is Loc2D::globalLocalization (src/loc2d.cpp:249-286: 3000 random
// poses) and GraphSlam2D::coarseSearchAndCorrelateCandidateScan; both hope that one sample lands within the solver's basin.  Here
// EVERY pose of a regular lattice over a box is scored in one launch (lama_hip_match_search_lattice, include/lama_hip.h: the sum of
// the squared cell distances at the scan's end points, exact integer arithmetic), the best few are kept and refined together in one
// launch of lama_hip_match_solve_batch -- GaussNewton with CauchyWeight(0.15), what every class of the reference solves with.
#pragma once

#include <cstdint>
#include <vector>

#include "pose2d.h"
#include "sdm/dynamic_distance_map.h"

namespace lama {

struct CorrelativeSearch2D {
    struct Options {
        double linear_step = 0.2;                       // metres between lattice nodes: max(1, round(linear_step / resolution)) whole cells
        double angular_step = 5.0 * M_PI / 180.0;       // H = max(1, round(2 pi / angular_step)) headings -pi + h * 2 pi / H
        uint32_t point_step = 0;                        // every point_step-th point is scored; 0: max(n / 256, 1)
        uint32_t tile = 8;                              // the device keeps the best node of every tile x tile nodes (at most 8)
        uint32_t max_candidates = 16;
        bool refine = true;                             // false: pose = coarse, rmse evaluated there
        uint32_t refine_iterations = 100;
    };
    struct Candidate {
        Pose2D coarse;          // the lattice node
        uint32_t score;         // its sum of squared cell distances (cells^2) over the scored points
        Pose2D pose;            // refined
        double rmse;            // MatchSurface2D::error() at `pose`, over ALL points of the scan
        uint32_t iterations;
    };
    // the lattice `search` lays over a box for a scan of n points on a map of this resolution
    struct Lattice {
        uint32_t cell_step = 1, nx = 1, ny = 1, num_headings = 1, point_step = 1, tile = 8;
        double heading(uint32_t h) const { return -M_PI + (double)h * (2.0 * M_PI / (double)num_headings); }
    };

    Options options;
    CorrelativeSearch2D() {}
    explicit CorrelativeSearch2D(const Options& o) : options(o) {}

    Lattice lattice(double resolution, size_t num_points, const Vector2d& box_min, const Vector2d& box_max) const;

    // `surface`: a map handed out by Slam2D, PFSlam2D (any particle) or MapBuilder2D -- it is searched on the device it lives on, as
    // MatchSurface2D evaluates it.  Node (0, 0) of the lattice is box_min, the nodes cover the box.  Of every tile the best node is a
    // candidate (a tile keeps ONE node); walking them from the best score, one is taken unless an already taken one lies within one
    // tile in x and in y and within one heading (circularly) -- so both ends of a symmetric corridor stay in the list -- until
    // max_candidates are taken.  They are refined in one launch and come back sorted by rmse.
    // Throws std::invalid_argument for a null / unbound map, an empty scan or box, and what the device entry refuses;
    // std::runtime_error when the bound device library has no lama_hip_match_search_lattice.
    std::vector<Candidate> search(const DynamicDistanceMap* surface, const PointCloudXYZ::Ptr& scan, const Vector2d& box_min,
                                  const Vector2d& box_max) const;
};

} // namespace lama
