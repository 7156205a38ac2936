// Test shim (tests/test_simple_pgo_cpu.py): the host parts of lama::SimplePGO -- the block LDL^T (iris_lama_amd/host/block_ldlt.hpp),
// the Levenberg-Marquardt loop (pgo_lm.hpp) and the graph construction (pgo_graph.hpp) -- compiled without the device.  The loop is
// driven through the same System interface as the product, with the CPU oracle's linearisation (oracle/lama_oracle.hpp) in place of
// the device's, scattered into the device's pattern (pgo_pattern.hpp).
#include <cstring>

#include "../iris_lama_amd/host/block_ldlt.hpp"
#include "../iris_lama_amd/host/pgo_graph.hpp"
#include "../iris_lama_amd/host/pgo_lm.hpp"
#include "../iris_lama_amd/host/pgo_pattern.hpp"
#include "../oracle/lama_oracle.hpp"

namespace {

orc::SE2 se2_of(const double* p) { orc::SE2 s; s.c = p[0]; s.s = p[1]; s.tx = p[2]; s.ty = p[3]; return s; }

class OracleSystem : public lama::pgo::System {
public:
    OracleSystem(uint32_t N, const int32_t* fi, const int32_t* fj, const double* meas4, const double* sq3, uint32_t F, const double* init4)
        : pat_(lama::pgo::lowerBlockPattern(N, fi, fj, F)), x_(N), cand_(N), fs_(F)
    {
        for (uint32_t v = 0; v < N; ++v) x_[v] = se2_of(init4 + 4 * v);
        for (uint32_t k = 0; k < F; ++k) {
            fs_[k].i = fi[k]; fs_[k].j = fj[k]; fs_[k].meas = se2_of(meas4 + 4 * k);
            for (int r = 0; r < 3; ++r) fs_[k].sqrt_info[r] = sq3[3 * k + r];
        }
    }
    uint32_t numPoses() const override { return (uint32_t)x_.size(); }
    void pattern(std::vector<int32_t>& row_ptr, std::vector<int32_t>& cols) override { row_ptr = pat_.row_ptr; cols = pat_.cols; }
    double linearize(double* blocks, double* b, double* diag, double*) override
    {
        std::vector<double> e, hd, ho, bb;
        double c2 = 0.0;
        orc::pgo_linearize(x_, fs_, e, hd, ho, bb, c2);
        for (size_t q = 0; q < pat_.cols.size(); ++q) {
            double* B = blocks + 9 * q;
            if (pat_.rows[q] == pat_.cols[q]) {
                std::memcpy(B, &hd[9 * (size_t)pat_.rows[q]], 9 * sizeof(double));
                for (int t = 0; t < 3; ++t) diag[3 * (size_t)pat_.rows[q] + t] = B[4 * t];
                continue;
            }
            for (int t = 0; t < 9; ++t) B[t] = 0.0;
            for (int32_t p = pat_.cptr[q]; p < pat_.cptr[q + 1]; ++p) {
                const double* H = &ho[9 * (size_t)(pat_.contrib[p] >> 1)];
                if (pat_.contrib[p] & 1) { for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) B[3 * a + c] += H[3 * c + a]; }
                else { for (int t = 0; t < 9; ++t) B[t] += H[t]; }
            }
        }
        std::memcpy(b, bb.data(), bb.size() * sizeof(double));
        return 0.5 * c2;
    }
    double tryStep(const double* dx, double*) override
    {
        for (size_t v = 0; v < x_.size(); ++v) cand_[v] = orc::se2_mul(x_[v], orc::se2_exp(dx[3 * v], dx[3 * v + 1], dx[3 * v + 2]));
        std::vector<double> e, hd, ho, bb;
        double c2 = 0.0;
        orc::pgo_linearize(cand_, fs_, e, hd, ho, bb, c2);
        return 0.5 * c2;
    }
    void accept() override { x_.swap(cand_); }
    const std::vector<orc::SE2>& poses() const { return x_; }

private:
    lama::pgo::BlockPattern pat_;
    std::vector<orc::SE2> x_, cand_;
    std::vector<orc::PgoFactor> fs_;
};

} // namespace

extern "C" {

// analyze + factorize + solve; returns 1 (solved), 0 (rank deficient)
int shim_ldlt_solve(int32_t N, const int32_t* row_ptr, const int32_t* cols, const double* blocks, const double* b, double* x,
                    int32_t natural, uint64_t* nnzL, double* ms_analyze)
{
    lama::pgo::BlockLDLT f;
    const auto t0 = std::chrono::steady_clock::now();
    f.analyze(N, row_ptr, cols, natural != 0);
    if (ms_analyze) *ms_analyze = lama::pgo::msSince(t0);
    if (nnzL) *nnzL = f.nnzL();
    if (!f.factorize(blocks)) return 0;
    f.solve(b, x);
    return 1;
}

int shim_lm(uint32_t N, const int32_t* fi, const int32_t* fj, const double* meas4, const double* sq3, uint32_t F, const double* init4,
            double* out4, int32_t* status, uint32_t* iterations, int8_t* trace, uint32_t cap, uint32_t* tries, double* errs2)
{
    OracleSystem sys(N, fi, fj, meas4, sq3, F, init4);
    const lama::pgo::LmResult r = lama::pgo::levenbergMarquardt(sys);
    *status = r.status; *iterations = r.iterations; *tries = r.tries;
    for (size_t q = 0; q < r.trace.size() && q < cap; ++q) trace[q] = r.trace[q];
    errs2[0] = r.initial_error; errs2[1] = r.final_error;
    for (uint32_t v = 0; v < N; ++v) {
        const orc::SE2& p = sys.poses()[v];
        out4[4 * v] = p.c; out4[4 * v + 1] = p.s; out4[4 * v + 2] = p.tx; out4[4 * v + 3] = p.ty;
    }
    return 0;
}

// SimplePGO's graph (pgo_graph.hpp) from flat lists; returns the number of factors (-1: buildGraph refused the lists)
int shim_build_graph(const double* nodes4, uint32_t n, const int32_t* ef, const int32_t* et, const double* e4, uint32_t ne,
                     const int32_t* fx, const double* f4, uint32_t nf, int32_t* fi, int32_t* fj, double* meas4, double* sq3, uint32_t cap)
{
    lama::SimplePGO p;
    for (uint32_t i = 0; i < n; ++i) p.node_list.push_back(lama::Pose2D(lama::SE2d::fromArray(nodes4 + 4 * i)));
    for (uint32_t k = 0; k < ne; ++k) p.edge_list.push_back({ef[k], {et[k], lama::Pose2D(lama::SE2d::fromArray(e4 + 4 * k))}});
    for (uint32_t k = 0; k < nf; ++k) p.fixed_list.push_back({fx[k], lama::Pose2D(lama::SE2d::fromArray(f4 + 4 * k))});
    lama::pgo::Graph g;
    if (!lama::pgo::buildGraph(p, g)) return -1;
    for (size_t k = 0; k < g.fi.size() && k < cap; ++k) {
        fi[k] = g.fi[k]; fj[k] = g.fj[k];
        for (int t = 0; t < 4; ++t) meas4[4 * k + t] = g.meas4[4 * k + t];
        for (int t = 0; t < 3; ++t) sq3[3 * k + t] = g.sqrt_info3[3 * k + t];
    }
    return (int)g.fi.size();
}

} // extern "C"
