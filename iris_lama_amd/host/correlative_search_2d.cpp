// correlative_search_2d.cpp -- lama::CorrelativeSearch2D (include/lama/correlative_search_2d.h): lattice, candidate selection and
// refinement around lama_hip_match_search_lattice / lama_hip_match_solve_batch.
#include "lama/correlative_search_2d.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

#include "correlative_impl.hpp"
#include "scan_arrays.hpp"

namespace lama {

CorrelativeSearch2D::Lattice CorrelativeSearch2D::lattice(double resolution, size_t num_points, const Vector2d& box_min, const Vector2d& box_max) const
{
    if (!(resolution > 0.0)) throw std::invalid_argument("lama::CorrelativeSearch2D: the map's resolution is not positive");
    if (!(options.linear_step > 0.0) || !(options.angular_step > 0.0)) throw std::invalid_argument("lama::CorrelativeSearch2D: linear_step and angular_step are positive");
    if (!(box_max.x() >= box_min.x()) || !(box_max.y() >= box_min.y())) throw std::invalid_argument("lama::CorrelativeSearch2D: the box is empty (or not finite)");
    Lattice l;
    l.cell_step = (uint32_t)std::max(1.0, std::round(options.linear_step / resolution));
    l.num_headings = (uint32_t)std::max(1.0, std::round(2.0 * M_PI / options.angular_step));
    const double node = (double)l.cell_step * resolution;                // metres between nodes
    const double fx = std::floor((box_max.x() - box_min.x()) / node), fy = std::floor((box_max.y() - box_min.y()) / node);
    if (!(fx < 4294967295.0) || !(fy < 4294967295.0)) throw std::invalid_argument("lama::CorrelativeSearch2D: the box holds more than 2^32 nodes a side");
    l.nx = (uint32_t)fx + 1u; l.ny = (uint32_t)fy + 1u;
    l.point_step = options.point_step ? options.point_step : (uint32_t)std::max<size_t>(num_points / 256, 1);
    l.tile = options.tile;
    return l;
}

namespace detail {

std::vector<CorrelativeSearch2D::Candidate> correlative_search(const CorrelativeSearch2D& cs, const CorrelativeDevice& dev, const PointCloudXYZ& scan,
                                                               const Vector2d& box_min, const Vector2d& box_max,
                                                               const std::function<bool(double, double)>& keep)
{
    typedef CorrelativeSearch2D::Candidate Candidate;
    const CorrelativeSearch2D::Options& opt = cs.options;
    if (scan.points.empty()) throw std::invalid_argument("lama::CorrelativeSearch2D: empty scan");
    if (!dev.engine->match_search_lattice)
        throw std::runtime_error("lama::CorrelativeSearch2D: the device library " + dev.engine->origin + " has no lama_hip_match_search_lattice (missing "
                                 "entry: it is older than this host library, or not a device library); rebuild it");
    if (!dev.engine->match_solve_batch)
        throw std::runtime_error("lama::CorrelativeSearch2D: the device library " + dev.engine->origin + " has no lama_hip_match_solve_batch (missing entry)");
    const uint32_t n = (uint32_t)scan.points.size();
    const CorrelativeSearch2D::Lattice L = cs.lattice(dev.resolution, n, box_min, box_max);
    const uint32_t H = L.num_headings, tile = L.tile;
    if (tile == 0) throw std::invalid_argument("lama::CorrelativeSearch2D: tile is at least 1");
    auto refuse = [&](int32_t rc, const char* what) {
        const std::string text = deviceFailure(*dev.engine, dev.ctx, "lama::CorrelativeSearch2D", what, rc);
        if (rc == LAMA_HIP_E_INVALID) throw std::invalid_argument(text);
        throw std::runtime_error(text);
    };
    std::vector<double> hcs(2 * (size_t)H);
    for (uint32_t h = 0; h < H; ++h) { const double a = L.heading(h); hcs[2 * h] = std::cos(a); hcs[2 * h + 1] = std::sin(a); }
    const uint32_t tiles_x = (L.nx - 1u) / tile + 1u, tiles_y = (L.ny - 1u) / tile + 1u;
    std::vector<uint64_t> keys((size_t)tiles_x * tiles_y * H);
    const ScanArrays a(scan);
    int32_t rc = dev.engine->match_search_lattice(dev.ctx, dev.particle, a.pts.data(), n, a.o, a.q, L.point_step, hcs.data(), H, box_min.x(), box_min.y(),
                                                  L.cell_step, L.nx, L.ny, tile, keys.data(), nullptr);
    if (rc) refuse(rc, "lama_hip_match_search_lattice");

    // ---- selection: ascending keys; one is taken unless a taken one is within one tile in x and y and one heading (circularly)
    struct Node { uint32_t score, h, ix, iy; };
    auto node_of = [&](uint64_t key) {
        const uint32_t index = (uint32_t)key;
        return Node{(uint32_t)(key >> 32), index / (L.nx * L.ny), index % L.nx, (index / L.nx) % L.ny};
    };
    const double node_m = (double)L.cell_step * dev.resolution;
    auto node_x = [&](const Node& k) { return box_min.x() + (double)k.ix * node_m; };
    auto node_y = [&](const Node& k) { return box_min.y() + (double)k.iy * node_m; };
    std::sort(keys.begin(), keys.end());
    std::vector<Node> taken;
    for (size_t i = 0; i < keys.size() && taken.size() < opt.max_candidates; ++i) {
        const Node k = node_of(keys[i]);
        if (keep && !keep(node_x(k), node_y(k))) continue;
        bool near = false;
        for (const Node& t : taken) {
            const uint32_t dtx = k.ix / tile > t.ix / tile ? k.ix / tile - t.ix / tile : t.ix / tile - k.ix / tile;
            const uint32_t dty = k.iy / tile > t.iy / tile ? k.iy / tile - t.iy / tile : t.iy / tile - k.iy / tile;
            const uint32_t dh = k.h > t.h ? k.h - t.h : t.h - k.h;
            if (dtx <= 1u && dty <= 1u && std::min(dh, H - dh) <= 1u) { near = true; break; }
        }
        if (!near) taken.push_back(k);
    }
    std::vector<Candidate> out;
    const size_t B = taken.size();
    if (B == 0) return out;

    // ---- refinement: one batch, GaussNewton + CauchyWeight(0.15); the whole scan for every candidate
    std::vector<uint32_t> particles(B, dev.particle), offs(B + 1, 0u), limits(B, opt.refine ? opt.refine_iterations : 0u), status(B, 0u);
    std::vector<double> pts, origins(3 * B), quats(4 * B), poses(4 * B), out8(8 * B);
    std::vector<int32_t> iters(B, 0);
    pts.reserve(a.pts.size() * B);
    out.resize(B);
    for (size_t b = 0; b < B; ++b) {
        pts.insert(pts.end(), a.pts.begin(), a.pts.end());
        offs[b + 1] = (uint32_t)(pts.size() / 3);
        for (int k = 0; k < 3; ++k) origins[3 * b + k] = a.o[k];
        for (int k = 0; k < 4; ++k) quats[4 * b + k] = a.q[k];
        const double p4[4] = {hcs[2 * taken[b].h], hcs[2 * taken[b].h + 1], node_x(taken[b]), node_y(taken[b])};
        for (int k = 0; k < 4; ++k) poses[4 * b + k] = p4[k];
        out[b].coarse = Pose2D(SE2d::fromArray(p4));
        out[b].score = taken[b].score;
    }
    rc = dev.engine->match_solve_batch(dev.ctx, (uint32_t)B, particles.data(), pts.data(), offs.data(), origins.data(), quats.data(), poses.data(),
                                       limits.data(), 0 /* GaussNewton */, LAMA_HIP_ROBUST_CAUCHY, 0.15, out8.data(), iters.data(), status.data());
    if (rc && rc != LAMA_HIP_E_NUMERIC) refuse(rc, "lama_hip_match_solve_batch");
    std::vector<Candidate> good;
    for (size_t b = 0; b < B; ++b) {
        if (status[b]) continue;                                     // (a zero-norm unit complex on the way: the reference would have thrown)
        out[b].pose = Pose2D(SE2d::fromArray(&poses[4 * b]));
        out[b].rmse = std::sqrt(out8[8 * b + 7] / (double)n);
        out[b].iterations = (uint32_t)iters[b];
        good.push_back(out[b]);
    }
    std::stable_sort(good.begin(), good.end(), [](const Candidate& x, const Candidate& y) { return x.rmse < y.rmse; });
    return good;
}

} // namespace detail

std::vector<CorrelativeSearch2D::Candidate> CorrelativeSearch2D::search(const DynamicDistanceMap* surface, const PointCloudXYZ::Ptr& scan,
                                                                        const Vector2d& box_min, const Vector2d& box_max) const
{
    if (!surface) throw std::invalid_argument("lama::CorrelativeSearch2D: null surface");
    if (!scan) throw std::invalid_argument("lama::CorrelativeSearch2D: null scan");
    const DynamicDistanceMap::DeviceBinding& d = surface->device();
    if (!d.engine || !d.ctx)
        throw std::invalid_argument("lama::CorrelativeSearch2D: the distance map does not live on the device (obtain it from Slam2D / PFSlam2D / "
                                    "MapBuilder2D::getDistanceMap()); there is no CPU search path");
    detail::CorrelativeDevice dev;
    dev.engine = d.engine.get(); dev.ctx = d.ctx; dev.particle = d.particle; dev.resolution = surface->resolution;
    return detail::correlative_search(*this, dev, *scan, box_min, box_max, std::function<bool(double, double)>());
}

} // namespace lama
