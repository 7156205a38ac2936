// lama/sdm/frontier.h -- the FRONTIERS of a device occupancy map: where mapped free space ends and unknown space begins, grouped into
// connected clusters with a size, a box, a centroid and a place to drive to -- what an exploring robot asks its map after every update.
// An addition (the reference has nothing of the kind; a caller walked the dense grid on the host): the host classes' getFrontiers()
// label the clusters on the device (lama_hip_map_frontiers, iris_lama_amd/csrc/lama_frontier.h) and bring down the cluster list only.
//
// A frontier pixel is a FREE pixel of the trinary occupancy grid (grid.h, same box and stride rules) with at least one UNKNOWN pixel
// among its four edge neighbours; pixels around the box count as the map has them.  Clusters are 8-connected.  Exact, in integers.
#pragma once

#include <cstdint>
#include <vector>

#include "../types.h"
#include "grid.h"

namespace lama { namespace sdm {

struct FrontierOptions {
    uint32_t stride = 1;           // 1, 2, 4, 8, 16 or 32 cells per pixel side
    bool whole_map = true;         // Map::bounds of the device map; false: the box [world_min, world_max] (metres), as GridOptions
    Vector2d world_min, world_max;
    uint32_t min_pixels = 1;       // clusters of fewer frontier pixels are not reported (they still count in frontier_pixels)
    uint32_t max_frontiers = 0;    // the largest this many; 0: all
    bool labels = false;           // also the label grid
};

// label: the smallest pixel index j * width + i of the cluster; sums of the pixel indices; the box in pixels.
// centroid / seed in world metres: Map::m2w gives cell CENTRES (the reference's w2m rounds), so with origin as in GridHeader
//   centroid = origin.xy + resolution * (stride * (sum / pixels) + (stride - 1) / 2.0)      (sum / pixels in double)
//   seed     = the same expression at the label's pixel (label % width, label / width): always a free pixel of the cluster, which
//              the centroid of a bent frontier need not be.
struct Frontier {
    uint32_t label = 0, pixels = 0, min_i = 0, min_j = 0, max_i = 0, max_j = 0;
    uint64_t sum_i = 0, sum_j = 0;
    Vector2d centroid, seed;
};

// The box as GridHeader describes it, except that a side of the whole-map box is clipped to 32,766 pixels (the labelling keeps a
// pixel of margin on either side within the raster's 32,768).  frontiers: by pixels descending, then label ascending.
struct FrontierSet : GridHeader {
    std::vector<Frontier> frontiers;
    uint64_t frontier_pixels = 0;  // all frontier pixels of the box, those of clusters below min_pixels included
    uint64_t clusters = 0;         // clusters with pixels >= min_pixels (frontiers.size() unless max_frontiers cut the list)
    std::vector<uint32_t> labels;  // FrontierOptions::labels: [height][width], the cluster's label at a frontier pixel, 0xFFFFFFFF elsewhere
};

}} // namespace lama::sdm
