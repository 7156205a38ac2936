// lama/sdm/travel.h -- ROUTES through a device map: can the robot get from where it is to each of a list of goals, how far is it, and
// along which pixels -- what an exploring robot asks about its frontier seeds (frontier.h) and a localised one about a place on its
// floor plan.  An addition (the reference has nothing of the kind; a caller downloaded two dense grids, inflated the obstacles and ran
// Dijkstra on one core): the host classes' planRoutes() relax a travel-cost field on the device (lama_hip_map_travel,
// iris_lama_amd/csrc/lama_travel.h) and bring down the routes only.
//
// The pixels, the stride and the box are those of grid.h.  A pixel is traversable when it is FREE in the trinary occupancy grid and its
// squared distance (the distance grid) is at least clearance^2 cells; lama::Loc2D, whose only device map is the distance map, applies
// the distance rule alone (that map knows no "unknown").  Entering a pixel costs 5 by an edge, 7 by a diagonal, near_factor times as
// much where the pixel is closer than the preferred clearance; a diagonal needs both pixels beside it traversable (no corner is cut).
// Exact, in integers: include/lama_hip.h has the whole definition.
#pragma once

#include <cstdint>
#include <vector>

#include "../types.h"
#include "grid.h"

namespace lama { namespace sdm {

struct TravelOptions {
    uint32_t stride = 1;                // 1, 2, 4, 8, 16 or 32 cells per pixel side
    bool whole_map = true;              // Map::bounds of the device map; false: the box [world_min, world_max] (metres), as GridOptions
    Vector2d world_min, world_max;
    double robot_radius = 0.0;          // metres; clearance_cells = ceil(robot_radius / resolution), computed on the host
    double preferred_clearance = 0.0;   // metres, in cells likewise; raised to the robot's radius where it is smaller
    uint32_t near_factor = 1;           // 1 .. 64: what a pixel closer than preferred_clearance costs more
    uint32_t goal_reach = 0;            // 0 .. 16 pixels: a goal is answered by the best pixel within this Chebyshev distance of it
    uint32_t max_path_points = 1024;    // per route, counted from the source; 0: no paths
    bool field = false;                 // also the travel-cost field
};

enum RouteStatus : uint32_t { kRouteReached = 0, kRouteUnreached = 1, kRouteOutside = 2 };

// pixel: the answer pixel j * width + i; cost: 5 per edge step, 7 per diagonal step, near_factor times that close to obstacles;
// steps: the moves of the whole path.  length_m = cost * cell_size / 5 (the length of the path where near_factor is 1, diagonals
// counted as 1.4).  path: world metres, SOURCE FIRST, the first min(max_path_points, steps + 1) pixel centres by the formula of
// frontier.h: origin.xy + resolution * (stride * (i, j) + (stride - 1) / 2.0).
struct Route {
    uint32_t status = kRouteUnreached, pixel = 0xFFFFFFFFu, cost = 0xFFFFFFFFu, steps = 0;
    double length_m = 0.0;
    std::vector<Vector2d> path;
};

// The box as GridHeader describes it; routes[g] answers goals[g].
struct RouteSet : GridHeader {
    std::vector<Route> routes;
    std::vector<uint32_t> field;        // TravelOptions::field: [height][width], 0xFFFFFFFF where no route leads
    uint32_t rounds = 0;                // relaxation rounds the device ran (a diagnostic)
};

}} // namespace lama::sdm
