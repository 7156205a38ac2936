// A consumer of lama::MapBuilder2D (include/lama/map_builder_2d.h) written against the public headers only: key scans with
// poses (as lama::SimplePGO hands them back) -> occupancy map + distance map -> MatchSurface2D on the rebuilt map.
// Without a device the constructor throws (no CPU fallback): the program reports that and exits 0.
#include <cmath>
#include <cstdio>
#include <exception>

#include "lama/map_builder_2d.h"
#include "lama/match_surface_2d.h"
#include "lama/nlls/solver.h"

int main()
{
    try {
        lama::MapBuilder2D::Options o;
        o.l2_max = 1.0;
        lama::MapBuilder2D builder(o);
        for (int k = 0; k < 4; ++k) {
            lama::PointCloudXYZ::Ptr cloud(new lama::PointCloudXYZ);
            for (int i = 0; i < 360; ++i) {        // a round room of 4 m radius seen from x = 0.3 k
                const double a = i * 3.14159265358979 / 180.0, x = 0.3 * k;
                const double bq = x * std::cos(a), r = -bq + std::sqrt(bq * bq + 16.0 - x * x);
                cloud->points.push_back(lama::Vector3d(r * std::cos(a), r * std::sin(a), 0.0));
            }
            builder.add(cloud, lama::Pose2D(0.3 * k, 0.0, 0.0));
        }
        builder.add(lama::PointCloudXYZ::Ptr(new lama::PointCloudXYZ), lama::Pose2D(9.0, 9.0, 1.0));      // an empty cloud contributes nothing
        builder.build();
        const lama::FrequencyOccupancyMap* occ = builder.getOccupancyMap();
        const lama::DynamicDistanceMap* dm = builder.getDistanceMap();
        if (!occ || !dm) { std::printf("no map\n"); return 1; }
        size_t cells = 0;
        occ->visit_all_cells([&](const lama::Vector3ui&) { ++cells; });
        const bool wall = occ->isOccupied(lama::Vector3d(4.0, 0.0, 0.0)), inside = occ->isFree(lama::Vector3d(1.0, 1.0, 0.0));
        builder.setPose(1, lama::Pose2D(0.3, 0.0, 0.0));
        builder.build();
        std::printf("device path ran: keys %zu cells %zu occupied %zu wall %d inside %d patches %zu\n", builder.size(), cells,
                    builder.occupiedCells().size() / 2, (int)wall, (int)inside, dm->patches());
        return (wall && inside && cells > 1000) ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("no device: %s\n", e.what());
        return 0;
    }
}
