// lama/sdm/grid.h -- DENSE grids of a device map: what a nav_msgs/OccupancyGrid carries, a planner's costmap eats and a viewer draws.
// An addition (the reference hands out its sparse maps and lets the caller walk bounds() cell by cell): the host classes'
// getOccupancyGrid() / getDistanceGrid() classify and write the cells out on the device (lama_hip_map_rasterize,
// iris_lama_amd/csrc/lama_raster.h), for the whole map or a world box, one element per stride x stride block of cells.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "../types.h"

namespace lama { namespace sdm {

struct GridOptions {
    uint32_t stride = 1;           // 1, 2, 4, 8, 16 or 32 cells per pixel side
    bool probability = false;      // occupancy: 0 .. 100 = round-half-up(100 * occupied / visited) instead of the trinary 0 / 100 / -1
    bool whole_map = true;         // Map::bounds of the device map; false: the box [world_min, world_max] (metres)
    Vector2d world_min, world_max;
};

// Pixel (i, j) is at data[j * width + i] and covers the map cells [x0 + i * stride, x0 + (i + 1) * stride) x [y0 + j * stride, ...).
// A side is clipped to 32,768 pixels; x0 and y0 are multiples of the stride (a world box is widened outwards to them).
struct GridHeader {
    uint32_t x0 = 0, y0 = 0, width = 0, height = 0, stride = 1;
    double resolution = 0.0;       // of the map
    double cell_size = 0.0;        // stride * resolution: the side of a pixel in metres
    Vector3d origin;               // Map::m2w of cell (x0, y0), z = 0 -- what iris_lama_ros puts into info.origin.position
};

// int8, the values of nav_msgs/OccupancyGrid: 0 free, 100 occupied, -1 unknown (GridOptions::probability: 0 .. 100, -1 unknown).
// A block is occupied if any of its cells is, else free if any is, else unknown; with probability, the largest of its visited cells.
struct OccupancyGrid : GridHeader {
    std::vector<int8_t> data;
};

// uint16 squared distances in cells: the stored sqdist where the cell has a valid obstacle, else the map's largest (max_distance);
// a block holds the smallest of its cells.
struct DistanceGrid : GridHeader {
    double max_distance = 0.0;     // DynamicDistanceMap::maxDistance(), metres
    std::vector<uint16_t> sqdist;
    // DynamicDistanceMap::distance(cell) of (the nearest cell of) pixel (i, j): sqrt(sqdist) * resolution
    double metres(uint32_t i, uint32_t j) const { return std::sqrt((double)sqdist[(size_t)j * width + i]) * resolution; }
};

}} // namespace lama::sdm
