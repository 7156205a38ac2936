// host_lifecycle.cpp -- TEST PROGRAM: the life cycle of the host classes' device context (lama::DeviceContext) on the engine test
// double, as a stand-alone executable built with -fsanitize=address,undefined (Makefile: _build/host_lifecycle; run by
// tests/test_device_context_cpu.py with the double's path as its argument).  One object of each of the five classes is constructed,
// updated and destroyed; Loc2D::Init runs twice; a DeviceContext is moved.  The double counts the contexts it creates and destroys.
#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "hip_engine.hpp"
#include "lama/device_context.h"
#include "lama/lidar_odometry_2d.h"
#include "lama/loc2d.h"
#include "lama/map_builder_2d.h"
#include "lama/pf_slam2d.h"
#include "lama/slam2d.h"

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; }             \
    } while (0)

namespace {

struct Counts { uint64_t created, destroyed, zero_cap_downloads; };
void (*g_counts)(uint64_t*) = nullptr;
Counts counts()
{
    uint64_t v[3];
    g_counts(v);
    return Counts{v[0], v[1], v[2]};
}

lama::PointCloudXYZ::Ptr ring(double radius)                      // a round room seen from its middle
{
    lama::PointCloudXYZ::Ptr cloud(new lama::PointCloudXYZ);
    for (int k = 0; k < 180; ++k) {
        const double a = k * M_PI / 90.0;
        cloud->points.push_back(lama::Vector3d(radius * std::cos(a), radius * std::sin(a), 0.0));
    }
    return cloud;
}

void fill_room(lama::Loc2D& loc, double side)                     // the walls of a square room into both public maps
{
    const double res = loc.distance_map->resolution;
    const int n = (int)(side / res);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            const lama::Vector3d p(res * i, res * j, 0.0);
            if (i == 0 || j == 0 || i == n - 1 || j == n - 1) { loc.occupancy_map->setOccupied(p); loc.distance_map->addObstacle(loc.distance_map->w2m(p)); }
            else loc.occupancy_map->setFree(p);
        }
}

} // namespace

int main(int argc, char** argv)
{
    CHECK(argc == 2);
    std::shared_ptr<lama::HipEngine> engine = lama::loadHipEngine(argv[1]);
    g_counts = reinterpret_cast<void (*)(uint64_t*)>(dlsym(engine->dl, "lama_cpu_engine_call_counts"));
    CHECK(g_counts);
    lama::setEngineOverride(engine);
    const lama::PointCloudXYZ::Ptr cloud = ring(3.0);
    const lama::Pose2D start(1.0, 2.0, 0.25), turned = start + lama::Pose2D(0.0, 0.0, 0.6);

    {
        lama::Slam2D slam;
        slam.setPose(start);
        CHECK(slam.update(cloud, start, 0.0) && slam.update(cloud, turned, 1.0));
        CHECK(slam.getDistanceMap() && slam.getDistanceMap()->device().ctx == slam.deviceContext());     // a view that holds the raw handle
        CHECK(slam.getOccupancyMap() && slam.getOccupancyMap()->patches() > 0);
        // a refused call: "<class>: <call> failed (status <rc>): <last error>"
        lama::PointCloudXYZ::Ptr bad(new lama::PointCloudXYZ(*cloud));
        bad->points[7] = lama::Vector3d(std::nan(""), 0.0, 0.0);
        try {
            slam.update(bad, start + lama::Pose2D(1.0, 0.0, 0.0), 2.0);
            CHECK(!"a scan with a NaN point was accepted");
        } catch (const std::runtime_error& e) {
            CHECK(std::strstr(e.what(), "lama::Slam2D: lama_hip_pf_scan_match failed (status -1): the scan holds a non-finite point"));
        }
    }
    {
        lama::PFSlam2D::Options o;
        o.particles = 4; o.seed = 7;
        lama::PFSlam2D pf(o);
        pf.setPrior(start);
        CHECK(pf.update(cloud, start, 0.0) && pf.update(cloud, turned, 1.0));
        CHECK(pf.getDistanceMap() && pf.getDistanceMap()->device().ctx == pf.deviceContext());
        o.gpus = 2;                                                  // two shard objects, each with a context of its own
        lama::PFSlam2D group(o);
        group.setPrior(start);
        CHECK(group.update(cloud, start, 0.0) && group.update(cloud, turned, 1.0));
        CHECK(group.numShards() == 2 && group.deviceContext() == group.shard(0)->deviceContext() && group.engine() != nullptr);
        CHECK(group.getDistanceMap() != nullptr);
    }
    {
        lama::LidarOdometry2D lo;
        CHECK(lo.update(cloud, 0.0) && lo.update(cloud, 1.0));
        lama::sdm::HostMap m;
        CHECK(lo.downloadDistanceMap(m) && !m.ids.empty() && m.cells.size() == m.ids.size() * 10240 && m.masks.size() == m.ids.size() * 16);
        CHECK(lo.downloadOccupancyMap(m) && !m.ids.empty() && m.cells.size() == m.ids.size() * 4096);
    }
    {
        lama::MapBuilder2D mb;
        mb.add(cloud, start);
        mb.add(cloud, turned);
        mb.build();
        CHECK(!mb.occupiedCells().empty() && mb.getOccupancyMap() && mb.getDistanceMap());
        CHECK(mb.getDistanceMap()->device().ctx == mb.deviceContext());
        // a builder whose only key is an empty cloud has a map without patches: success, empty arrays, no download of capacity 0
        lama::MapBuilder2D empty;
        empty.add(lama::PointCloudXYZ::Ptr(new lama::PointCloudXYZ), start);
        empty.build();
        const Counts before = counts();
        lama::sdm::HostMap m;
        m.ids.assign(3, 1u);
        CHECK(empty.downloadOccupancyMap(m) && m.ids.empty() && m.cells.empty() && m.masks.empty());
        CHECK(counts().zero_cap_downloads == before.zero_cap_downloads);
    }
    {
        const Counts c0 = counts();
        lama::Loc2D loc;
        lama::Loc2D::Options o;
        loc.Init(o);
        CHECK(!loc.deviceContext() && counts().created == c0.created);                 // the context comes with the first device call
        fill_room(loc, 4.0);
        CHECK(loc.distance_map->update() > 0 && loc.deviceContext());
        CHECK(counts().created == c0.created + 1 && counts().destroyed == c0.destroyed);
        o.resolution = 0.1;                                                            // a second Init: fresh maps, a fresh context
        loc.Init(o);
        CHECK(!loc.deviceContext() && counts().created == c0.created + 1 && counts().destroyed == c0.destroyed + 1);
        fill_room(loc, 4.0);
        CHECK(loc.distance_map->update() > 0 && loc.distance_map->resolution == 0.1);
        CHECK(counts().created == c0.created + 2 && counts().destroyed == c0.destroyed + 1);
        CHECK(loc.distance_map->distance(lama::Vector3d(2.0, 2.0, 0.0)) > 0.9);         // (reach 1 m: the room's middle is beyond it)
        loc.setPose(lama::Pose2D(2.0, 2.0, 0.0));
        CHECK(loc.update(ring(1.9), lama::Pose2D(0.0, 0.0, 0.0), 0.0, true) && std::isfinite(loc.getRMSE()));
    }
    {
        const Counts c0 = counts();
        lama_hip_cfg cfg;
        engine->default_cfg(&cfg);
        cfg.particles = 2;
        lama::DeviceContext a("lama::Test");
        CHECK(!a);
        a.create(engine, cfg);
        lama_hip_ctx* raw = a.get();
        CHECK(a && raw && counts().created == c0.created + 1);
        lama::DeviceContext b(std::move(a));
        CHECK(!a && !a.get() && b && b.get() == raw);
        std::vector<uint64_t> ids(2, 5u), masks(1, 1u);
        std::vector<uint8_t> cells(9, 1u);
        CHECK(b.download(1, LAMA_HIP_MAP_DISTANCE, ids, cells, masks) && ids.empty() && cells.empty() && masks.empty());    // no scan yet: no patch
        CHECK(!a.download(0, LAMA_HIP_MAP_DISTANCE, ids, cells, masks));                                                     // no context
        CHECK(counts().zero_cap_downloads == c0.zero_cap_downloads);
        try {
            b.check(-5, "lama_hip_something");
            CHECK(!"check(-5) did not throw");
        } catch (const std::runtime_error& e) {
            CHECK(std::string(e.what()) == "lama::Test: lama_hip_something failed (status -5): ");
        }
        b.check(0, "lama_hip_something");
        lama::DeviceContext c("lama::Other");
        c = std::move(b);
        CHECK(!b && c.get() == raw && counts().destroyed == c0.destroyed);
        c.reset();
        c.reset();
        CHECK(!c && counts().destroyed == c0.destroyed + 1);
    }   // a, b, c destroyed: nothing left to destroy
    const Counts end = counts();
    CHECK(end.created == end.destroyed && end.created == 10);
    lama::setEngineOverride(nullptr);
    std::printf("host life cycle OK: %llu contexts created and destroyed\n", (unsigned long long)end.created);
    return 0;
}
