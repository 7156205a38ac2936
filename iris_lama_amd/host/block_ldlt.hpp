// block_ldlt.hpp -- sparse LDL^T of a symmetric matrix made of 3x3 blocks: the host-side linear solver of lama::SimplePGO.
//
// minisam's SimplePGO path solves with Eigen's SimplicialLDLT under an AMD ordering (vendor/minisam/minisam/linear/
// SparseCholesky.{h,cpp}): the pattern is analysed once per optimize(), the numeric factorisation runs on every damped try, and a
// NumericalIssue (a zero pivot) is reported as RANK_DEFICIENCY.  This is the same split on the block graph of a pose graph:
//   analyze   : minimum-degree ordering of the block graph (the family AMD belongs to), elimination tree and column counts of L
//               (the up-looking algorithm of Davis' LDL, one 3x3 block per entry).
//   factorize : A = L D L^T with unit block-lower L and block-diagonal D, each D_k factorised as a scalar 3x3 LDL^T -- the same
//               pivots as a scalar LDL^T of the permuted matrix.  A zero or non-finite pivot returns false (rank deficiency).
//   solve     : x = A^-1 b.
// Input: the lower block-CSR pattern of pgo_pattern.hpp (row r: diagonal block first, then columns c < r), blocks row-major.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <set>
#include <utility>
#include <vector>

namespace lama {
namespace pgo {

// Minimum-degree ordering of the graph of a lower block pattern, on the explicit elimination graph: repeatedly eliminate the
// vertex of least current degree (ties: the lowest index) and join its neighbours into a clique.  Returns perm, perm[k] = the
// vertex eliminated k-th.
inline std::vector<int32_t> minimumDegreeOrder(int32_t N, const int32_t* row_ptr, const int32_t* cols)
{
    std::vector<std::vector<int32_t>> adj(N);
    for (int32_t r = 0; r < N; ++r)
        for (int32_t q = row_ptr[r]; q < row_ptr[r + 1]; ++q)
            if (cols[q] != r) { adj[r].push_back(cols[q]); adj[cols[q]].push_back(r); }
    std::set<std::pair<int32_t, int32_t>> queue;
    for (int32_t v = 0; v < N; ++v) {
        std::sort(adj[v].begin(), adj[v].end());
        adj[v].erase(std::unique(adj[v].begin(), adj[v].end()), adj[v].end());
        queue.insert({(int32_t)adj[v].size(), v});
    }
    std::vector<int32_t> perm;
    perm.reserve(N);
    std::vector<int32_t> merged;
    while (!queue.empty()) {
        const int32_t v = queue.begin()->second;
        queue.erase(queue.begin());
        perm.push_back(v);
        const std::vector<int32_t> nb = std::move(adj[v]);
        adj[v].clear();
        for (int32_t u : nb) {
            queue.erase({(int32_t)adj[u].size(), u});
            merged.clear();
            std::set_union(adj[u].begin(), adj[u].end(), nb.begin(), nb.end(), std::back_inserter(merged));
            adj[u].clear();
            for (int32_t w : merged)
                if (w != u && w != v) adj[u].push_back(w);
            queue.insert({(int32_t)adj[u].size(), u});
        }
    }
    return perm;
}

class BlockLDLT {
public:
    // natural = true keeps the given order (for comparisons); the product uses the minimum-degree ordering
    void analyze(int32_t N, const int32_t* row_ptr, const int32_t* cols, bool natural = false)
    {
        N_ = N;
        perm_.resize(N);
        if (natural) for (int32_t k = 0; k < N; ++k) perm_[k] = k;
        else perm_ = minimumDegreeOrder(N, row_ptr, cols);
        iperm_.assign(N, 0);
        for (int32_t k = 0; k < N; ++k) iperm_[perm_[k]] = k;
        // the strictly upper part of the permuted matrix by columns: entry (j, k), j < k, is input block src (transposed if tr)
        Ap_.assign(N + 1, 0);
        diag_src_.assign(N, -1);
        for (int32_t r = 0; r < N; ++r)
            for (int32_t q = row_ptr[r]; q < row_ptr[r + 1]; ++q) {
                if (cols[q] == r) { diag_src_[iperm_[r]] = q; continue; }
                ++Ap_[std::max(iperm_[r], iperm_[cols[q]]) + 1];
            }
        for (int32_t k = 0; k < N; ++k) Ap_[k + 1] += Ap_[k];
        Ai_.assign(Ap_[N], 0); Asrc_.assign(Ap_[N], 0);
        std::vector<int32_t> fill(Ap_.begin(), Ap_.end() - 1);
        for (int32_t r = 0; r < N; ++r)
            for (int32_t q = row_ptr[r]; q < row_ptr[r + 1]; ++q) {
                if (cols[q] == r) continue;
                const int32_t pr = iperm_[r], pc = iperm_[cols[q]];
                const int32_t k = std::max(pr, pc), at = fill[k]++;
                Ai_[at] = std::min(pr, pc);
                Asrc_[at] = 2 * q + (pr > pc ? 1 : 0);          // A(j, k) = B(r, c) when r's position is j, else B^T
            }
        // elimination tree and column counts (ldl_symbolic)
        parent_.assign(N, -1);
        std::vector<int32_t> flag(N, -1), lnz(N, 0);
        for (int32_t k = 0; k < N; ++k) {
            flag[k] = k;
            for (int32_t p = Ap_[k]; p < Ap_[k + 1]; ++p)
                for (int32_t i = Ai_[p]; flag[i] != k; i = parent_[i]) {
                    if (parent_[i] == -1) parent_[i] = k;
                    ++lnz[i];
                    flag[i] = k;
                }
        }
        Lp_.assign(N + 1, 0);
        for (int32_t k = 0; k < N; ++k) Lp_[k + 1] = Lp_[k] + lnz[k];
        Li_.assign(Lp_[N], 0);
        Lx_.assign(9 * (size_t)Lp_[N], 0.0);
        Dinv_.assign(9 * (size_t)N, 0.0);
        Y_.assign(9 * (size_t)N, 0.0);
        flag_.assign(N, -1); pattern_.assign(N, 0); lnz_.assign(N, 0);
    }

    // scalar nonzeros of the strictly lower triangle of L (the 3 inside every diagonal block included)
    uint64_t nnzL() const { return 9 * (uint64_t)(Lp_.empty() ? 0 : Lp_[N_]) + 3 * (uint64_t)N_; }
    const std::vector<int32_t>& permutation() const { return perm_; }

    // blocks: [nnzb][9] in the pattern given to analyze().  false: a zero or non-finite pivot (rank deficiency)
    bool factorize(const double* blocks)
    {
        const int32_t N = N_;
        std::fill(flag_.begin(), flag_.end(), -1);
        std::fill(lnz_.begin(), lnz_.end(), 0);
        for (int32_t k = 0; k < N; ++k) {
            int32_t top = N;
            flag_[k] = k;
            for (int32_t p = Ap_[k]; p < Ap_[k + 1]; ++p) {     // scatter column k of the upper part, find the pattern of row k of L
                const int32_t j = Ai_[p];
                const double* B = blocks + 9 * (size_t)(Asrc_[p] >> 1);
                double* Y = &Y_[9 * (size_t)j];
                if (Asrc_[p] & 1) { for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) Y[3 * a + b] = B[3 * b + a]; }
                else { for (int t = 0; t < 9; ++t) Y[t] = B[t]; }
                int32_t len = 0;
                for (int32_t i = j; flag_[i] != k; i = parent_[i]) { pattern_[len++] = i; flag_[i] = k; }
                while (len > 0) pattern_[--top] = pattern_[--len];
            }
            double D[9];
            const double* Akk = blocks + 9 * (size_t)diag_src_[k];
            for (int t = 0; t < 9; ++t) D[t] = Akk[t];
            for (int32_t t = top; t < N; ++t) {
                const int32_t i = pattern_[t];
                double y[9];
                double* Yi = &Y_[9 * (size_t)i];
                for (int s = 0; s < 9; ++s) { y[s] = Yi[s]; Yi[s] = 0.0; }
                const int32_t p2 = Lp_[i] + lnz_[i];
                for (int32_t p = Lp_[i]; p < p2; ++p) {            // Y_m -= L_mi y_i
                    const double* L = &Lx_[9 * (size_t)p];
                    double* Ym = &Y_[9 * (size_t)Li_[p]];
                    for (int a = 0; a < 3; ++a)
                        for (int b = 0; b < 3; ++b) Ym[3 * a + b] -= (L[3 * a] * y[b] + L[3 * a + 1] * y[3 + b]) + L[3 * a + 2] * y[6 + b];
                }
                double* Lk = &Lx_[9 * (size_t)p2];                  // L_ki = y_i^T D_i^-1
                const double* Di = &Dinv_[9 * (size_t)i];
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) Lk[3 * a + b] = (y[a] * Di[b] + y[3 + a] * Di[3 + b]) + y[6 + a] * Di[6 + b];
                for (int a = 0; a < 3; ++a)                          // D_k -= L_ki y_i
                    for (int b = 0; b < 3; ++b) D[3 * a + b] -= (Lk[3 * a] * y[b] + Lk[3 * a + 1] * y[3 + b]) + Lk[3 * a + 2] * y[6 + b];
                Li_[p2] = k;
                ++lnz_[i];
            }
            if (!invert3(D, &Dinv_[9 * (size_t)k])) return false;
        }
        return true;
    }

    void solve(const double* b, double* x) const
    {
        const int32_t N = N_;
        std::vector<double> z(3 * (size_t)N);
        for (int32_t k = 0; k < N; ++k) for (int t = 0; t < 3; ++t) z[3 * k + t] = b[3 * (size_t)perm_[k] + t];
        for (int32_t k = 0; k < N; ++k)                              // L z = P b
            for (int32_t p = Lp_[k]; p < Lp_[k + 1]; ++p) {
                const double* L = &Lx_[9 * (size_t)p];
                double* zi = &z[3 * (size_t)Li_[p]];
                const double* zk = &z[3 * (size_t)k];
                for (int a = 0; a < 3; ++a) zi[a] -= (L[3 * a] * zk[0] + L[3 * a + 1] * zk[1]) + L[3 * a + 2] * zk[2];
            }
        for (int32_t k = 0; k < N; ++k) {                            // D^-1
            const double* Di = &Dinv_[9 * (size_t)k];
            double* zk = &z[3 * (size_t)k];
            const double v0 = zk[0], v1 = zk[1], v2 = zk[2];
            for (int a = 0; a < 3; ++a) zk[a] = (Di[3 * a] * v0 + Di[3 * a + 1] * v1) + Di[3 * a + 2] * v2;
        }
        for (int32_t k = N - 1; k >= 0; --k)                         // L^T
            for (int32_t p = Lp_[k]; p < Lp_[k + 1]; ++p) {
                const double* L = &Lx_[9 * (size_t)p];
                const double* zi = &z[3 * (size_t)Li_[p]];
                double* zk = &z[3 * (size_t)k];
                for (int a = 0; a < 3; ++a) zk[a] -= (L[a] * zi[0] + L[3 + a] * zi[1]) + L[6 + a] * zi[2];
            }
        for (int32_t k = 0; k < N; ++k) for (int t = 0; t < 3; ++t) x[3 * (size_t)perm_[k] + t] = z[3 * k + t];
    }

private:
    // D = l d l^T (scalar LDL^T of the lower triangle, no pivoting); Dinv = D^-1.  false on a zero or non-finite pivot
    static bool invert3(const double* D, double* Dinv)
    {
        const double d0 = D[0];
        if (!(d0 != 0.0) || !std::isfinite(d0)) return false;
        const double l10 = D[3] / d0, l20 = D[6] / d0;
        const double d1 = D[4] - l10 * l10 * d0;
        if (!(d1 != 0.0) || !std::isfinite(d1)) return false;
        const double l21 = (D[7] - l20 * l10 * d0) / d1;
        const double d2 = D[8] - l20 * l20 * d0 - l21 * l21 * d1;
        if (!(d2 != 0.0) || !std::isfinite(d2)) return false;
        for (int c = 0; c < 3; ++c) {                                // column c of D^-1: l^-T d^-1 l^-1 e_c
            double v0 = c == 0 ? 1.0 : 0.0, v1 = c == 1 ? 1.0 : 0.0, v2 = c == 2 ? 1.0 : 0.0;
            v1 -= l10 * v0;
            v2 -= l20 * v0 + l21 * v1;
            v0 /= d0; v1 /= d1; v2 /= d2;
            v1 -= l21 * v2;
            v0 -= l10 * v1 + l20 * v2;
            Dinv[c] = v0; Dinv[3 + c] = v1; Dinv[6 + c] = v2;
        }
        for (int t = 0; t < 9; ++t) if (!std::isfinite(Dinv[t])) return false;
        return true;
    }

    int32_t N_ = 0;
    std::vector<int32_t> perm_, iperm_, Ap_, Ai_, Asrc_, diag_src_, parent_, Lp_, Li_;
    std::vector<double> Lx_, Dinv_;
    mutable std::vector<double> Y_;
    std::vector<int32_t> flag_, pattern_, lnz_;
};

} // namespace pgo
} // namespace lama
