// pgo_pattern.hpp -- the lower block-CSR pattern of an SE2 pose graph's Hessian (3x3 blocks), shared by the device library
// (lama_hip_pgo_create builds it once per graph) and the host tests that restate the device's assembly.
//   row r : its diagonal block first, then the distinct columns c < r that share a between factor with r, ascending.
//   The factors on one pair contribute in factor order: code = 2 k + 1 when the block is the transpose of factor k's J_i^T J_j
//   (its i is the smaller index), 2 k otherwise.  A diagonal block has no contribution list (it is the per-variable sum).
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <vector>

namespace lama {
namespace pgo {

struct BlockPattern {
    std::vector<int32_t> row_ptr;   // [N+1]
    std::vector<int32_t> rows;      // [nnzb]
    std::vector<int32_t> cols;      // [nnzb]
    std::vector<int32_t> cptr;      // [nnzb+1] into contrib
    std::vector<int32_t> contrib;
};

inline BlockPattern lowerBlockPattern(uint32_t N, const int32_t* fi, const int32_t* fj, uint32_t F)
{
    std::vector<std::array<int32_t, 3>> pr;             // (row, col, code) in factor order
    for (uint32_t k = 0; k < F; ++k)
        if (fj[k] >= 0) pr.push_back({{std::max(fi[k], fj[k]), std::min(fi[k], fj[k]), (int32_t)(2 * k + (fi[k] < fj[k] ? 1 : 0))}});
    std::stable_sort(pr.begin(), pr.end(), [](const std::array<int32_t, 3>& a, const std::array<int32_t, 3>& b) {
        return a[0] != b[0] ? a[0] < b[0] : a[1] < b[1];
    });
    BlockPattern p;
    p.row_ptr.assign(N + 1, 0);
    size_t q = 0;
    for (uint32_t r = 0; r < N; ++r) {
        p.row_ptr[r] = (int32_t)p.cols.size();
        p.rows.push_back((int32_t)r); p.cols.push_back((int32_t)r); p.cptr.push_back((int32_t)p.contrib.size());
        for (; q < pr.size() && pr[q][0] == (int32_t)r; ++q) {
            if (p.cols.back() != pr[q][1]) {            // (the diagonal block's column r is above every c)
                p.rows.push_back((int32_t)r); p.cols.push_back(pr[q][1]); p.cptr.push_back((int32_t)p.contrib.size());
            }
            p.contrib.push_back(pr[q][2]);
        }
    }
    p.row_ptr[N] = (int32_t)p.cols.size();
    p.cptr.push_back((int32_t)p.contrib.size());
    return p;
}

} // namespace pgo
} // namespace lama
