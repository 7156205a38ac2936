// scan_arrays.hpp -- a PointCloudXYZ as the device C-ABI (include/lama_hip.h) takes a scan: xyz triples, the sensor origin and the
// sensor orientation as a (w, x, y, z) quaternion.
#pragma once

#include <vector>

#include "lama/types.h"

namespace lama {
namespace detail {

struct ScanArrays {
    std::vector<double> pts;
    double o[3], q[4];
    explicit ScanArrays(const PointCloudXYZ& s) : pts(s.points.size() * 3)
    {
        for (size_t i = 0; i < s.points.size(); ++i) { pts[3 * i] = s.points[i].x(); pts[3 * i + 1] = s.points[i].y(); pts[3 * i + 2] = s.points[i].z(); }
        o[0] = s.sensor_origin_.x(); o[1] = s.sensor_origin_.y(); o[2] = s.sensor_origin_.z();
        q[0] = s.sensor_orientation_.w(); q[1] = s.sensor_orientation_.x(); q[2] = s.sensor_orientation_.y(); q[3] = s.sensor_orientation_.z();
    }
};

} // namespace detail
} // namespace lama
