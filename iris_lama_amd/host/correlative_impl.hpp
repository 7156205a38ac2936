// correlative_impl.hpp -- the search of lama::CorrelativeSearch2D on a given device context: shared by the class (a map bound through
// DynamicDistanceMap::device()) and Loc2D::relocalize (the object's own context).
#pragma once

#include <functional>
#include <vector>

#include "hip_engine.hpp"
#include "lama/correlative_search_2d.h"

namespace lama {
namespace detail {

struct CorrelativeDevice {
    const HipEngine* engine = nullptr;
    lama_hip_ctx* ctx = nullptr;
    uint32_t particle = 0;
    double resolution = 0.05;
};

// keep (may be empty): a tile winner whose node position it rejects is dropped before the selection
std::vector<CorrelativeSearch2D::Candidate> correlative_search(const CorrelativeSearch2D& cs, const CorrelativeDevice& dev, const PointCloudXYZ& scan,
                                                               const Vector2d& box_min, const Vector2d& box_max,
                                                               const std::function<bool(double, double)>& keep);

} // namespace detail
} // namespace lama
