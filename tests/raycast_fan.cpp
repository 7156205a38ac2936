// TEST INFRASTRUCTURE (tests/test_raycast_query_cpu.py): the host-side helpers of include/lama/sdm/ray_cast.h from a C++ caller.
// argv: n angle_min angle_increment max_range -> the fan's points, one "x y z" line each, as hexadecimal floats; then the ranges
// of a few stopping cells (rayRange, fillRayRanges).
#include <cstdio>
#include <cstdlib>

#include "lama/sdm/ray_cast.h"

int main(int argc, char** argv)
{
    if (argc != 5) return 2;
    const lama::PointCloudXYZ::Ptr fan = lama::sdm::makeFan((uint32_t)std::atoi(argv[1]), std::atof(argv[2]), std::atof(argv[3]), std::atof(argv[4]));
    for (const lama::Vector3d& p : fan->points) std::printf("%a %a %a\n", p[0], p[1], p[2]);
    lama::sdm::RayCastResult r;
    r.num_poses = 2; r.n = 3; r.resolution = 0.05;
    r.start_xy = {100u, 200u, 4000000000u, 7u};
    r.status = {1, 0, 2, 1, 1, 0};
    r.cell_xy = {103u, 204u, 0u, 0u, 100u, 200u, 4000000000u - 8191u, 7u + 4096u, 4000000001u, 7u, 5u, 5u};
    lama::sdm::fillRayRanges(r);
    for (double v : r.range) std::printf("%a\n", v);
    return 0;
}
