// lama_hip.hip -- C-ABI implementation (include/lama_hip.h) of the MI355X scan-matching path.
// gfx950 only.  No CPU fallback: every entry point needs a HIP device and fails loudly without one.
#include "../../include/lama_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "lama_kernels.h"
#include "lama_pgo.h"
#include "lama_pgo_pcg.h"
#include "lama_map_build.h"
#include "lama_raster.h"
#include "lama_frontier.h"
#include "lama_travel.h"
#include "lama_raycast_query.h"
#include "lama_match_batch.h"
#include "lama_correlative.h"
#include "../host/pgo_pattern.hpp"

using namespace lama_dev;

namespace {

// Device array that frees itself: n elements at p (none after a failed allocation).  Nothing is zeroed implicitly.
template <class T>
struct DevBuf {
    T* p = nullptr; size_t n = 0;
    DevBuf() {}
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&&) = delete;
    ~DevBuf() { reset(); }
    void reset() { (void)hipFree(p); p = nullptr; n = 0; }
    hipError_t alloc(size_t m)                                      // (on an empty buffer)
    {
        const hipError_t e = hipMalloc(&p, m * sizeof(T));
        if (e == hipSuccess) n = m; else p = nullptr;
        return e;
    }
    // at least `need` elements: a smaller buffer is freed BEFORE the new one (of max(need, floor) elements) is allocated
    hipError_t grow(size_t need, size_t floor = 0)
    {
        if (need <= n) return hipSuccess;
        reset();
        return alloc(std::max(need, floor));
    }
    size_t bytes() const { return n * sizeof(T); }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(n, o.n); }
    operator T*() const { return p; }
};

// A stream or an event that destroys itself.
template <class H, hipError_t (*Destroy)(H)>
struct HipHandle {
    H h = nullptr;
    HipHandle() {}
    HipHandle(HipHandle&& o) noexcept : h(o.h) { o.h = nullptr; }
    HipHandle& operator=(HipHandle&&) = delete;
    ~HipHandle() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
};
using Stream = HipHandle<hipStream_t, hipStreamDestroy>;
using Event = HipHandle<hipEvent_t, hipEventDestroy>;
// the deleter of the handles' unique_ptrs (a type of this file: those instantiations stay out of the library's exported symbols)
struct Delete { template <class T> void operator()(T* q) const { delete q; } };

// The maps of all particles of a context: two directories per HOME (P homes), pooled planes in which every particle owns one
// contiguous region per map kind (lama_dev.h).  A pool is a list of CHUNKS: it grows by another chunk (never by copying), a region
// lies inside one chunk.  The reference's patches are heap objects shared through cow_ptr (include/lama/cow_ptr.h:86-118); here
// memory follows use through per-particle region capacities, and a resample moves nothing that survives.
struct RegionAlloc;
struct PoolChunk {
    DevBuf<uint8_t> plane[4];                                       // dm: sv, obs, mask, - ; occ: occ, occ_mask, occ_hit, rev
    uint32_t patches = 0;
};
struct MapStore {
    DevBuf<int16_t> dm_dir, occ_dir;                                // [P homes][W*W]
    int32_t* counts = nullptr;                                      // [P][2] logical particle (a view into lama_hip_ctx::d_results)
    std::vector<PoolChunk> dm_chunks, occ_chunks;
};
constexpr size_t DM_PLANE_B[3] = {SV_PATCH_BYTES, 4096, 128};                 // dm_sv, dm_obs, dm_mask bytes per patch
constexpr size_t OCC_PLANE_B[4] = {4096, 128, 128, 4};              // occ, occ_mask, occ_hit, rev
// the host's record of a particle: home + region (chunk, offset, capacity) per map kind; the device gets PartRec (addresses)
struct HostPart { uint32_t home, dm_chunk, dm_off, dm_cap, occ_chunk, occ_off, occ_cap; };

// First-fit allocator of contiguous regions (in patches) over a pool; neighbouring free blocks coalesce.  Host side only: the device
// sees the result as the plane addresses in PartRec.  Free space is always all-zero on the device (k_zero_regions).
struct RegionAlloc {
    std::map<uint32_t, uint32_t> free_;        // offset -> length
    uint32_t cap = 0, used = 0;
    void reset(uint32_t c) { free_.clear(); cap = c; used = 0; if (c) free_[0] = c; }
    bool alloc(uint32_t n, uint32_t& off)
    {
        if (n == 0) { off = 0; return true; }
        for (auto it = free_.begin(); it != free_.end(); ++it) {
            if (it->second < n) continue;
            off = it->first;
            const uint32_t rest = it->second - n;
            free_.erase(it);
            if (rest) free_[off + n] = rest;
            used += n;
            return true;
        }
        return false;
    }
    void release(uint32_t off, uint32_t n)
    {
        if (n == 0) return;
        used -= n;
        auto nx = free_.lower_bound(off);
        if (nx != free_.begin()) {
            auto pv = std::prev(nx);
            if (pv->first + pv->second == off) { off = pv->first; n += pv->second; free_.erase(pv); }
        }
        if (nx != free_.end() && off + n == nx->first) { n += nx->second; free_.erase(nx); }
        free_[off] = n;
    }
    void extend(uint32_t newcap) { if (newcap > cap) { const uint32_t o = cap, n = newcap - cap; cap = newcap; used += n; release(o, n); } }
    uint32_t largest_free() const { uint32_t m = 0; for (auto& kv : free_) m = std::max(m, kv.second); return m; }
};

} // namespace

// Page-locked host array with the part of std::vector's interface the context uses: the per-call transfers (poses, counts,
// statistics, transforms, scan points) then are real DMA transfers that overlap with kernel launches instead of staged,
// blocking pageable copies.
template <class T>
struct PinVec {
    T* p = nullptr; size_t n = 0, cap = 0; bool pinned = false;
    PinVec() {}
    PinVec(const PinVec&) = delete;
    PinVec& operator=(const PinVec&) = delete;
    ~PinVec() { release(); }
    void release() { if (p) { if (pinned) (void)hipHostFree(p); else std::free(p); } p = nullptr; }
    void reserve(size_t m)
    {
        if (m <= cap) return;
        m = std::max(m, 2 * cap);                                   // geometric: a list built element by element re-pins O(log n) times
        T* q = nullptr;
        bool pin = hipHostMalloc((void**)&q, m * sizeof(T), hipHostMallocDefault) == hipSuccess && q;
        if (!pin) { (void)hipGetLastError(); q = (T*)std::malloc(m * sizeof(T)); }       // pageable memory still works, only slower
        if (!q) std::abort();                                                           // out of host memory
        if (p) std::memcpy(q, p, n * sizeof(T));
        release();
        p = q; cap = m; pinned = pin;
    }
    void resize(size_t m) { reserve(m); if (m > n) std::memset(p + n, 0, (m - n) * sizeof(T)); n = m; }
    void assign(size_t m, T v) { reserve(m); n = m; for (size_t i = 0; i < m; ++i) p[i] = v; }
    T* data() { return p; }
    const T* data() const { return p; }
    size_t size() const { return n; }
    T& operator[](size_t i) { return p[i]; }
    const T& operator[](size_t i) const { return p[i]; }
};

// One particle group of the grouped step schedule (lama_hip_pf_match_and_map): a contiguous block of the pool with a stream of its
// own and its own copy of everything that is a pool-wide scalar or list of an update.  Arrays indexed by particle stay the context's.
// Three groups by default: the context's three streams of the routed / early lanes, idle in small pools.  With the runtime's default
// of four hardware queues per process they get a queue each; a fourth stream shares one with the third, and the two groups' brushfire
// kernels then run one after the other (measured: a 30-particle step takes 2.65 ms with four groups, 1.39 ms with three, 1.47 ms with
// one; profiles/r07_step_groups.md).  Four can be asked for (LAMA_HIP_STEP_GROUPS) where the process has more queues.
constexpr uint32_t MAX_STEP_GROUPS = 4;
constexpr uint32_t DEFAULT_STEP_GROUPS = 3;
struct StepGroup {
    hipStream_t s = nullptr;          // one of the context's streams (not owned)
    uint32_t first = 0, count = 0;
    DevBuf<uint32_t> d_words;         // [0]: error word, [2..9]: hand-over counts (DevParams::slow_n)
    DevBuf<uint32_t> d_slow_list;     // [4][P] hand-over lists (DevParams::slow_list)
    DevBuf<double> d_pts;             // the group's own copy of the scan, uploaded on its stream
    DevBuf<uint8_t> d_pack; PinVec<uint8_t> h_pack;      // k_pack_group's block and its page-locked destination
    Event ev_match;                   // the block has arrived
    Event tev[6];                     // cfg.profile: brackets of scan match, ray-cast, brushfire
    uint32_t timed = 0;               // ... which of them have been recorded and not read yet (bit per bracket)
    bool maps_queued = false;         // a map update whose status has not been collected yet
    // what that update was asked to do (a clean abort repeats it after the arenas grew): poses, mount, scan slot, beams, reach
    std::vector<double> upd_poses; Affine upd_mtf; uint32_t upd_slot = 0, upd_n = 0; double upd_reach = 0.0;
};
// byte offsets inside a group's block for `n` particles (k_pack_group writes it)
struct GroupPack {
    size_t poses, loglik, stats, guard, counts, iters, words, bytes;
    explicit GroupPack(size_t n) : poses(0), loglik(32 * n), stats(40 * n), guard(72 * n), counts(76 * n), iters(84 * n), words(88 * n), bytes(88 * n + 64) {}
};

struct lama_hip_ctx {
    lama_hip_cfg cfg;
    std::string error;
    Stream stream;
    Event ev0, ev1;
    struct PendingTimer { hipEvent_t a, b; double* acc; uint64_t* launches; };
    std::vector<Event> ev_pool;                 // pairs handed out by Timer, resolved after the call's final sync
    std::vector<PendingTimer> pending;
    size_t ev_used = 0;
    bool initialised = false;   // first scan done
    bool poisoned = false;      // a resample ran out of device memory half-way: every later call fails (LAMA_HIP_E_STATE)
    bool dm_deleted = false;    // lama_hip_pf_delete_patches has removed a distance-map patch: obstacle offsets of the cells around it may
                                // dangle from now on (DevParams::ghosts; sticky: the offsets outlive any number of updates)

    uint32_t P = 0, W = 0, WC = 0, wx0 = 0, wy0 = 0;
    uint32_t max_sqdist = 0;
    double scale = 0, off = 0;

    MapStore ms;
    std::vector<RegionAlloc> ra_dm, ra_occ;     // one allocator per chunk
    std::vector<HostPart> h_part;     // logical particle -> home / regions (host truth) ...
    DevBuf<PartRec> d_part;           // ... and its device copy
    PinVec<PartRec> h_part_stage;     // (page-locked staging of the upload)
    PinVec<CloneJob> h_jobs; DevBuf<CloneJob> d_jobs;
    PinVec<ZeroJob> h_zjobs; DevBuf<ZeroJob> d_zjobs;
    uint32_t floor_dm = 128, floor_occ = 128;      // smallest region a particle gets (cfg.dm_patch_capacity / occ_patch_capacity)
    PinVec<uint32_t> h_guard;         // the guard's per-particle bound of the last map update
    uint64_t clone_bytes = 0;         // bytes the particle copies of the last resample moved (counters)
    double* d_poses = nullptr;        // (a view into d_results)
    DevBuf<uint64_t> d_qlower, d_qraise;
    uint64_t* d_stats = nullptr;      // (a view into d_results)
    DevBuf<uint32_t> d_qsizes;
    DevBuf<uint64_t> d_dbg;
    DevBuf<uint32_t> d_slow;
    DevBuf<uint32_t> d_slow_list; uint32_t* d_slow_n = nullptr;      // hand-over list of the brushfire's first stage (d_slow_n: a view into d_results)
    // routing of the long brushfire chains (k_bf_route): second stream + events for the big-queue stage that runs beside the first one
    DevBuf<uint8_t> d_heavy;
    // early lane: the particles routed in the previous update (d_heavy still holds them; valid while the particle set is unchanged)
    DevBuf<uint8_t> d_early; DevBuf<uint32_t> d_elist;
    Stream stream3; Event ev_alloc, ev_go, ev_early;
    bool early_ok = false;            // the last map update routed over the whole pool and nothing has permuted the particles since
    uint32_t early_candidates = 0;    // routed + early-lane particles of the last map update (none: the early lane is not even launched)
    std::vector<double> h_ll; bool ll_valid = false;   // log-likelihoods of the last scan match, in the current particle order
    PinVec<uint32_t> h_hlist; DevBuf<uint32_t> d_hlist;   // the worst-fitting particles of that scan match (early lane)
    uint32_t early_on = 1;            // LAMA_HIP_BF_ROUTE's fifth number (0: no early lane)
    uint32_t early_min_count = 1024;  // below ~4 workgroups per CU everybody else's ray-cast is too short to be worth overtaking (an override sets 0)
    Stream stream2; Event ev_route, ev_heavy;
    uint32_t route_min_count = 64, route_min_events = 48, route_percent = 150, route_cap = 64;     // LAMA_HIP_BF_ROUTE overrides (tests)
    bool route_forced = false; uint32_t num_cus = 256;
    bool debug_tail = false, debug_window = false;      // LAMA_HIP_DEBUG_TAIL / LAMA_HIP_DEBUG_WINDOW, read at creation
    uint32_t big_stage_pad = 0;                         // dynamic LDS added to the early lane's big-queue workgroups (a FULL chip) so that a long chain has its CU to itself
    DevBuf<uint64_t> d_act; DevBuf<uint32_t> d_act_count;
    // patch-centric ray-cast (lama_raycast_patch.h): ray records / bounding boxes of the scan's beams, arena slot -> directory position
    // (the three grow together: d_rrec's count is their capacity, in beams of the whole pool)
    DevBuf<lama_dev::RayRec> d_rrec; DevBuf<uint64_t> d_rbbox; DevBuf<lama_dev::RayChunk> d_rchunk;
    int32_t* d_err = nullptr;         // (a view into d_results)
    DevBuf<double> d_pts; uint32_t last_n = 0;
    PinVec<uint64_t> h_stats;
    PinVec<double> h_tfs, h_pts;
    PinVec<int32_t> h_err;
    PinVec<uint32_t> h_slow_n;        // hand-over counts of the last map update (brushfire, ordered replay)
    DevBuf<double> d_tfs;
    double* d_loglik = nullptr; int32_t* d_iters = nullptr;
    // d_poses | d_loglik | d_iters | d_err are carved out of ONE allocation so that a scan match brings all of its results
    // (and the error word) back with a single device-to-host copy; those pointers (and d_slow_n, d_stats, d_guard, ms.counts) are
    // views into it, not owners
    DevBuf<uint8_t> d_results;
    size_t results_bytes = 0, status_off = 0, status_bytes = 0;
    PinVec<uint8_t> h_status;
    PinVec<uint8_t> h_results;
    DevBuf<int32_t> d_oldcounts;
    // lama_hip_map_integrate_scans / lama_hip_map_occupied_cells (lama_map_build.h): inputs, ray records, the bin table over the call's
    // box, offsets, touched-patch list and slots, bins; all grow-only
    DevBuf<double> d_mb_pts, d_mb_tfs; DevBuf<uint32_t> d_mb_offs; DevBuf<lama_dev::MbRay> d_mb_rays;
    DevBuf<uint32_t> d_mb_table, d_mb_off, d_mb_list, d_mb_bins; DevBuf<int32_t> d_mb_slot; DevBuf<uint64_t> d_mb_meta;
    PinVec<double> h_mb_tfs; PinVec<uint32_t> h_mb_offs; PinVec<uint64_t> h_mb_meta;
    // lama_hip_map_rasterize / lama_hip_map_bounds (lama_raster.h): the dense grid and its page-locked staging copy, grow-only
    DevBuf<uint8_t> d_raster; PinVec<uint8_t> h_raster;
    // lama_hip_map_frontiers (lama_frontier.h): the compacted records, 40 bytes a reported cluster, grow-only (the rest is in d_raster)
    DevBuf<lama_dev::FrontierRec> d_frontier_rec;
    // lama_hip_map_travel (lama_travel.h): rasters, classes, field, tile flags and lists, sources, goals, routes and paths in one
    // grow-only buffer; what the last call's host loop did (lama_hip_map_travel_stats)
    DevBuf<uint8_t> d_travel;
    uint32_t travel_rounds = 0, travel_max_tiles = 0, travel_readbacks = 0; uint64_t travel_tiles = 0;
    // lama_hip_map_cast_rays (lama_raycast_query.h), grow-only: [points 3n | pose transforms 12K] and the outputs, 22 bytes a beam
    DevBuf<double> d_rq_in; DevBuf<uint8_t> d_rq_out; PinVec<double> h_rq_tfs;
    DevBuf<double> d_bposes, d_bout;  // batch evaluations: four pose doubles per entry, one output double (ensure_batch)
    // lama_hip_match_solve_batch (lama_match_batch.h), grow-only: [out8 8B | poses 4B | mounts 12B | points 3N] and
    // [iterations B | status B | problems 4B], with their page-locked staging copies
    DevBuf<double> d_msb_f64; DevBuf<uint32_t> d_msb_u32;
    PinVec<double> h_msb_f64; PinVec<uint32_t> h_msb_u32;
    // lama_hip_match_search_lattice (lama_correlative.h), grow-only: the headings' transforms [H][12] and the tile keys
    DevBuf<double> d_cs_tfs; DevBuf<uint64_t> d_cs_best;
    PinVec<double> h_cs_tfs;

    double scan_reach = 0.0;          // largest point distance of the resident scan (sensor frame, metres)
    uint32_t visit_bound = 0;         // upper bound of the largest `visited` counter of any frequency cell (see k_occ_max_visited)
    DevBuf<uint32_t> d_scalar;
    // particle shipping: descriptors / gathered blob heads of one batch
    DevBuf<lama_dev::ShipDesc> d_ship_desc; DevBuf<uint8_t> d_ship_heads;
    PinVec<lama_dev::ShipDesc> h_ship_desc; PinVec<uint8_t> h_ship_heads;
    uint32_t* d_guard = nullptr;      // (a view into d_results) [P][2] bound on the distance-map patches an update may still allocate + block ticket (k_occ_reverse_dir)
    // what the last run_update_maps was asked to do: a cleanly aborted update (ERR_CLEAN_ABORT) is run again after the arenas grew
    Affine last_mtf; uint32_t last_first = 0, last_count = 0;
    bool last_guarded = false;        // the update went through the parallel ray-cast (its allocation phase precedes every modification)
    int recover_depth = 0;
    // the box of everything that can be mapped so far, absolute patch coordinates (ensure_window)
    int64_t mbx0 = 0, mbx1 = 0, mby0 = 0, mby1 = 0; bool mb_valid = false;
    bool unguarded_retry = false;     // the arenas are at their hard limit and the guard's bound did not fit: run the update without it
    // host-side effects of a map update that a repeated pass (recover_update) must not apply twice
    uint32_t saved_visit_bound = 0; lama_hip_counters saved_ctr;
    bool pending_maps = false;        // lama_hip_pf_update_maps_begin queued work whose status has not been collected yet
    // grouped step schedule (lama_hip_pf_match_and_map): pools below route_min_count are split into step_groups contiguous blocks
    StepGroup grp[MAX_STEP_GROUPS];
    Stream stream4;
    uint32_t step_groups = 1;         // 1: the single-stream schedule (LAMA_HIP_STEP_GROUPS overrides, read at creation)
    uint32_t groups_ran = 0;          // how many groups the last lama_hip_pf_match_and_map really ran (lama_hip_pf_step_groups)
    std::vector<int32_t> deferred_idx; bool resample_deferred = false;      // lama_hip_pf_resample while the groups were busy: made by the next call
    bool groups_busy = false;         // group streams may hold work: whoever touches shared state on the main stream waits for them first
    PinVec<double> h_pts2; uint32_t scan_slot = 0;       // second scan staging buffer: a step's scan outlives the step (repeat after a clean abort)
    std::vector<uint64_t> h_chain;    // per-particle brushfire cell counts of the map update whose status is being collected
    bool chain_dirty = false;
    double step_ms[3] = {0, 0, 0}; bool step_ms_any[3] = {false, false, false};     // longest group bracket of the update being collected
    PinVec<double> h_poses;           // host mirror of the particle poses (source of truth between calls)
    PinVec<int32_t> h_counts;         // host mirror of counts of the current set (refreshed after map updates)
    lama_hip_counters ctr;

    // nothing may still run on the stream when the members release themselves
    ~lama_hip_ctx()
    {
        (void)hipSetDevice(cfg.device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (StepGroup& g : grp) if (g.s) (void)hipStreamSynchronize(g.s);
    }
};

namespace {

// A failed HIP call: the error is recorded, and the call returns only once the stream has finished what it queued (copies from host
// memory that is released on the way out -- staging vectors, the caller's buffers, page-locked job lists -- may still be in flight).
int32_t hip_fail(lama_hip_ctx* ctx, hipError_t e, const char* what)
{
    ctx->error = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->groups_busy) for (StepGroup& g : ctx->grp) if (g.s) (void)hipStreamSynchronize(g.s);
    return LAMA_HIP_E_HIP;
}
#define HIPCHK(ctx, call)                                                                              \
    do {                                                                                               \
        const hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) return hip_fail((ctx), e_, #call);                                       \
    } while (0)

int32_t fail(lama_hip_ctx* ctx, int32_t code, const std::string& msg)
{
    ctx->error = msg;
    return code;
}

// Eigen Quaternion::toRotationMatrix restated (moving_tf = Translation(origin) * q,
// src/match_surface_2d.cpp:49, src/pf_slam2d.cpp:397,444)
Affine moving_tf(const double* origin3, const double* q)
{
    Affine a;
    const double w = q ? q[0] : 1.0, x = q ? q[1] : 0.0, y = q ? q[2] : 0.0, z = q ? q[3] : 0.0;
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    a.R[0][0] = 1.0 - (tyy + tzz); a.R[0][1] = txy - twz;         a.R[0][2] = txz + twy;
    a.R[1][0] = txy + twz;         a.R[1][1] = 1.0 - (txx + tzz); a.R[1][2] = tyz - twx;
    a.R[2][0] = txz - twy;         a.R[2][1] = tyz + twx;         a.R[2][2] = 1.0 - (txx + tyy);
    for (int i = 0; i < 3; ++i) a.t[i] = origin3 ? origin3[i] : 0.0;
    return a;
}

// fixed_tf(pose) * moving_tf on the HOST (libm), 12 doubles [R row-major | t]
// (src/pf_slam2d.cpp:444-451 ; Eigen AngleAxis(theta, UnitZ) restated)
void host_scan_tf(const double* pose4, const Affine& m, double* out12)
{
    const double theta = std::atan2(pose4[1], pose4[0]);
    const double sn = std::sin(theta), cs = std::cos(theta);
    const double F[3][3] = {{cs, 0.0 - sn, 0.0}, {sn, cs, 0.0}, {0.0, 0.0, (1.0 - cs) + cs}};
    const double ft[3] = {pose4[2], pose4[3], 0.0};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) out12[3 * i + j] = (F[i][0] * m.R[0][j] + F[i][1] * m.R[1][j]) + F[i][2] * m.R[2][j];
        out12[9 + i] = ((F[i][0] * m.t[0] + F[i][1] * m.t[1]) + F[i][2] * m.t[2]) + ft[i];
    }
}

// how many patches beyond an obstacle's own the brushfire can reach (and allocate): ceil(l2_max / resolution) + 1 cells.  After a
// deletion it can also re-create the patch of an obstacle cell that a cell in that reach still points at: as many cells again.
uint32_t guard_radius(const lama_hip_ctx* c)
{
    const uint32_t r = (uint32_t)std::ceil(std::sqrt((double)c->max_sqdist));
    return ((c->dm_deleted ? 2u * r + 1u : r) + 1u + 31u) / 32u;
}

DevParams make_params(const lama_hip_ctx* c)
{
    DevParams p;
    p.P = c->P; p.W = c->W; p.WC = c->WC; p.wx0 = c->wx0; p.wy0 = c->wy0;
    p.qcap = c->cfg.queue_capacity; p.part = c->d_part;
    p.max_sqdist = c->max_sqdist; p.max_iter = c->cfg.max_iter;
    p.scale = c->scale; p.off = c->off; p.resolution = c->cfg.resolution;
    p.maxdist = std::sqrt((double)c->max_sqdist) * c->cfg.resolution;
    p.meas_sigma = c->cfg.meas_sigma;
    p.trunc_ray = c->cfg.truncated_ray; p.trunc_range = c->cfg.truncated_range;
    const MapStore& s = c->ms;
    p.dm_dir = s.dm_dir; p.occ_dir = s.occ_dir; p.counts = s.counts;
    p.guard = c->d_guard;
    p.guard_r = guard_radius(c);
    p.poses = c->d_poses; p.q_lower = c->d_qlower; p.q_raise = c->d_qraise; p.stats = c->d_stats; p.qsizes = c->d_qsizes; p.err = c->d_err; p.dbg = c->d_dbg; p.slow = c->d_slow; p.slow_list = c->d_slow_list; p.slow_n = c->d_slow_n; p.heavy = nullptr; p.elist = nullptr; p.elist_n = nullptr; p.early = nullptr; p.lane = 0;
    p.act = c->d_act; p.act_count = c->d_act_count; p.act_cap = c->cfg.active_capacity;
    p.occ_policy = c->cfg.occupancy_policy; p.ray_rule = c->cfg.ray_rule; p.strategy = c->cfg.solver_strategy;
    // ProbabilisticOccupancyMap's parameters (probabilistic_occupancy_map.cpp:43-59): logods(p) = float(log(p / (1 - p))) of a
    // float argument, stored in double members
    auto logods = [](float prob) { return (double)(float)std::log(prob / (1.0 - prob)); };
    p.lo_miss = logods(0.4f); p.lo_hit = logods(0.7f); p.lo_min = logods(0.12f); p.lo_max = logods(0.97f);
    p.ghosts = c->dm_deleted ? 1u : 0u;
    return p;
}

// the kernels of one particle group: the context's parameters with the group's own error word and hand-over lists
DevParams group_params(const lama_hip_ctx* c, const StepGroup& g)
{
    DevParams p = make_params(c);
    p.err = reinterpret_cast<int32_t*>(g.d_words.p); p.slow_n = g.d_words.p + 2; p.slow_list = g.d_slow_list;
    return p;
}

// Nothing runs on the group streams any more when this returns.  Whoever touches, on the main stream, state that all particles
// share -- the window directories, the particle table and the regions behind it, the pools -- calls it first (the grouped step
// schedule's rare paths are drained, not made clever).
int32_t wait_for_groups(lama_hip_ctx* c)
{
    if (!c->groups_busy) return LAMA_HIP_OK;
    for (StepGroup& g : c->grp)
        if (g.count) { const hipError_t e = hipStreamSynchronize(g.s); if (e != hipSuccess) { c->error = std::string("hipStreamSynchronize(group stream): ") + hipGetErrorString(e); return LAMA_HIP_E_HIP; } }
    return LAMA_HIP_OK;
}

// The largest squared point distance of a scan.  False when a coordinate is infinite: no cell (the reference's w2m casts it to an integer:
// undefined behaviour, include/lama/sdm/map.h:125-128); strict: or a NaN (std::max drops it, the sum of products with zero keeps it)
bool scan_reach2(const double* pts, size_t n, bool strict, double& r2)
{
    double nan_acc = r2 = 0.0;
    for (size_t i = 0; i < n; ++i) { const double d2 = pts[3 * i] * pts[3 * i] + pts[3 * i + 1] * pts[3 * i + 1] + pts[3 * i + 2] * pts[3 * i + 2]; r2 = std::max(r2, d2); nan_acc += d2 * 0.0; }
    return std::isfinite(r2) && (!strict || nan_acc == 0.0);
}

int32_t upload_scan(lama_hip_ctx* c, const double* pts, uint32_t n)
{
    if (!pts) {      // reuse the scan uploaded by the previous call (same scan for scan_match and update_maps)
        if (c->last_n == 0 || n != c->last_n) return fail(c, LAMA_HIP_E_INVALID, "pts == NULL but no matching scan is resident");
        return LAMA_HIP_OK;
    }
    c->last_n = n;
    HIPCHK(c, c->d_pts.grow((size_t)3 * n, (size_t)3 * 2048));
    c->h_pts.resize((size_t)3 * n);                       // the caller's buffer is only borrowed for the call
    std::memcpy(c->h_pts.data(), pts, sizeof(double) * 3 * n);
    double r2 = 0.0;
    if (!scan_reach2(pts, n, false, r2)) { c->last_n = 0; return fail(c, LAMA_HIP_E_INVALID, "the scan holds a non-finite point (filter NaN / inf ranges before the update, as iris_lama_ros does)"); }
    c->scan_reach = std::sqrt(r2);
    HIPCHK(c, hipMemcpyAsync(c->d_pts, c->h_pts.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
    return LAMA_HIP_OK;
}

// the batch buffers hold at least `entries` results (d_bout, whose count is their capacity) and four pose doubles per entry
// (d_bposes); both are freed before the larger pair is allocated
int32_t ensure_batch(lama_hip_ctx* c, size_t entries, size_t floor = 0)
{
    if (entries <= c->d_bout.n) return LAMA_HIP_OK;
    c->d_bposes.reset(); c->d_bout.reset();
    const size_t cap = std::max(entries, floor);
    HIPCHK(c, c->d_bposes.alloc(4 * cap));
    HIPCHK(c, c->d_bout.alloc(cap));
    return LAMA_HIP_OK;
}

void resolve_timers(lama_hip_ctx* c);
int32_t grow_arenas(lama_hip_ctx* c, uint32_t first, uint32_t count);
int32_t recover_update(lama_hip_ctx* c, int32_t e);
int32_t run_update_maps(lama_hip_ctx* c, uint32_t n, const Affine& mtf, uint32_t first, uint32_t count);
int32_t permute_particles(lama_hip_ctx* c, const int32_t* idx);

// A failed allocation keeps counting (dir_alloc_one: the counts then say what a particle WANTED, which the clean-abort path
// uses).  When the error is final, the counts go back into the regions: every later copy (resample, export, a region move)
// is sized from them and must not run into a neighbour's region.
int32_t clamp_counts(lama_hip_ctx* c, bool fetch)
{
    if (fetch) HIPCHK(c, hipMemcpyAsync(c->h_counts.data(), c->ms.counts, sizeof(int32_t) * 2 * c->P, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    bool clamped = false;
    for (uint32_t p = 0; p < c->P; ++p) {
        const HostPart& hp = c->h_part[p];
        if ((uint32_t)c->h_counts[2 * p] > hp.dm_cap) { c->h_counts[2 * p] = (int32_t)hp.dm_cap; clamped = true; }
        if ((uint32_t)c->h_counts[2 * p + 1] > hp.occ_cap) { c->h_counts[2 * p + 1] = (int32_t)hp.occ_cap; clamped = true; }
    }
    if (clamped) {
        HIPCHK(c, hipMemcpyAsync(c->ms.counts, c->h_counts.data(), sizeof(int32_t) * 2 * c->P, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return LAMA_HIP_OK;
}

// what a non-zero device error word means to the caller
int32_t device_error_result(lama_hip_ctx* c, int32_t e)
{
    if (e & ERR_WINDOW) return fail(c, LAMA_HIP_E_WINDOW, "a map cell fell outside the device window (the mapped area is wider than 1016 patches)");
    if (e & ERR_DM_CAP) return fail(c, LAMA_HIP_E_CAPACITY, "a particle's distance map exceeds 32767 patches (or the device is out of memory)");
    if (e & ERR_OCC_CAP) return fail(c, LAMA_HIP_E_CAPACITY, "a particle's occupancy map exceeds 32767 patches (or the device is out of memory)");
    if (e & ERR_QUEUE) return fail(c, LAMA_HIP_E_CAPACITY, "brushfire queue full (raise cfg.queue_capacity)");
    return fail(c, LAMA_HIP_E_NUMERIC, "unit complex number is (near) zero (SophusException in the reference)");
}

// A map update's status in the fetched bytes of the pool's packed block or of a group's k_pack_group block (read with memcpy): error word,
// 5 hand-over counts, and for the particles base .. base + n their [n][4] statistics words, [n] guard bounds and [n][2] patch counts.
struct StatusView {
    const uint8_t *err, *slow_n, *stats, *guard, *counts; uint32_t base, n;
    int32_t error() const { int32_t e; std::memcpy(&e, err, sizeof(e)); return e; }
};

// an update's status goes into the counters and host mirrors; of one that succeeded (particles [first, first + count)) also the cell statistics and, if given, the chains
void apply_update_status(lama_hip_ctx* c, const StatusView& v, uint32_t first, uint32_t count, uint64_t* chain)
{
    uint32_t sn[5]; std::memcpy(sn, v.slow_n, sizeof(sn));
    c->ctr.brushfire_handovers += sn[0]; c->ctr.replay_handovers += sn[1] + sn[3]; c->ctr.brushfire_routed += sn[2] + sn[4]; c->ctr.brushfire_early += sn[4];
    c->early_candidates = sn[2] + sn[4];
    c->h_guard.resize(c->P);
    std::memcpy(&c->h_guard[v.base], v.guard, sizeof(uint32_t) * v.n);
    std::memcpy(&c->h_counts[2 * (size_t)v.base], v.counts, sizeof(int32_t) * 2 * v.n);
    if (v.error() != 0) return;
    for (uint32_t p = first; p < first + count; ++p) {
        uint64_t st[4]; std::memcpy(st, v.stats + sizeof(st) * (p - v.base), sizeof(st));
        c->ctr.ray_cells += st[2]; c->ctr.bf_cells += st[3]; if (chain) chain[p] = st[3];
    }
}

void refresh_patch_totals(lama_hip_ctx* c)
{
    c->ctr.dm_patches = c->ctr.occ_patches = 0;
    for (uint32_t p = 0; p < c->P; ++p) { c->ctr.dm_patches += c->h_counts[2 * p]; c->ctr.occ_patches += c->h_counts[2 * p + 1]; }
}

// End of an API call: one stream synchronisation that brings back the device error word and, when asked, a map update's packed
// status (maps) or a scan match's statistics (match; err_in_results: its error word has come with its results): one round trip.
int32_t check_device_errors(lama_hip_ctx* c, bool maps = false, bool match = false, bool err_in_results = false)
{
    c->h_err.resize(1);
    int32_t& e = c->h_err[0] = 0;
    if (maps || match) c->h_stats.resize((size_t)c->P * 4);
    if (maps) {
        c->h_status.resize(c->status_bytes); c->h_slow_n.resize(5);
        HIPCHK(c, hipMemcpyAsync(c->h_status.data(), c->d_results + c->status_off, c->status_bytes, hipMemcpyDeviceToHost, c->stream));
    } else {
        if (match) {
            HIPCHK(c, hipMemcpyAsync(c->h_counts.data(), c->ms.counts, sizeof(int32_t) * 2 * c->P, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->h_stats.data(), c->d_stats, sizeof(uint64_t) * c->h_stats.size(), hipMemcpyDeviceToHost, c->stream));
        }
        if (!err_in_results) HIPCHK(c, hipMemcpyAsync(&e, c->d_err, sizeof(e), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (maps) {
        const uint8_t* const b = c->h_status.data(), * const sn = b + ((const uint8_t*)c->d_slow_n - (c->d_results + c->status_off));
        const StatusView v{b, sn, sn + 32, sn + 32 + 32 * (size_t)c->P, sn + 32 + 40 * (size_t)c->P, 0u, c->P};
        e = v.error();
        std::memcpy(c->h_slow_n.data(), v.slow_n, 5 * sizeof(uint32_t));                 // (mirrors: the longest chain below, recover_group)
        std::memcpy(c->h_stats.data(), v.stats, sizeof(uint64_t) * 4 * c->P);
        apply_update_status(c, v, c->last_first, c->last_count, nullptr);      // (a block's update leaves the others' statistics alone)
    }
    if (err_in_results) std::memcpy(&e, c->h_results.data() + ((const uint8_t*)c->d_err - c->d_results), sizeof(e));
    resolve_timers(c);
    if (e != 0) {
        HIPCHK(c, hipMemsetAsync(c->d_err, 0, sizeof(int32_t), c->stream));
        // The allocation phase of a map update ran out of patches before any cell was modified: grow and run the update again.
        if (maps && (e & ERR_CLEAN_ABORT) && (e & (ERR_DM_CAP | ERR_OCC_CAP)) && !(e & ERR_WINDOW) && c->last_guarded && c->recover_depth < 10) {
            const int32_t rr = recover_update(c, e);
            if (rr != LAMA_HIP_E_CAPACITY) return rr;      // done (or another error); E_CAPACITY: the arenas are at their limit
        }
        if (e & (ERR_DM_CAP | ERR_OCC_CAP)) { const int32_t rcl = clamp_counts(c, !(maps || match)); if (rcl) return rcl; }
        return device_error_result(c, e);
    }
    if (match) for (uint32_t p = 0; p < c->P; ++p) { c->ctr.gn_iterations += c->h_stats[4 * p]; c->ctr.gn_evals += c->h_stats[4 * p + 1]; }
    if (maps || match) refresh_patch_totals(c);
    if (!maps) return LAMA_HIP_OK;
    uint64_t mx = 0, sum = 0; uint32_t arg = 0;                     // the update lasted as long as its longest chain
    for (uint32_t p = c->last_first; p < c->last_first + c->last_count; ++p) { const uint64_t v = c->h_stats[4 * p + 3]; sum += v; if (v > mx) { mx = v; arg = p; } }
    c->ctr.bf_longest_chain_sum += mx; c->ctr.bf_longest_chain_last = mx;
    if (c->debug_tail) {
        // (how well would the scan match's log-likelihood have predicted the longest chain? its rank among the pool, 0 = lowest)
        uint32_t rank = 0; double ll = 0, mean_ll = 0;
        if (c->h_results.size() >= c->results_bytes && c->P > 1) {
            const double* L = reinterpret_cast<const double*>(c->h_results.data() + sizeof(double) * 4 * c->P);
            ll = L[arg];
            for (uint32_t p = 0; p < c->P; ++p) { rank += L[p] < ll ? 1u : 0u; mean_ll += L[p]; }
            mean_ll /= c->P;
        }
        std::fprintf(stderr, "brushfire pops: mean %.0f max %llu (particle %u) handovers %u brushfire %.3f ms; log-lik of that particle %.1f (pool mean %.1f), rank %u of %u\n", (double)sum / c->P, (unsigned long long)mx, arg, c->h_slow_n[0], c->ctr.ms_brushfire, ll, mean_ll, rank, c->P);
    }
    return grow_arenas(c, 0, c->P);
}

// ------------------------------------------------------------------------------------------------
// Memory that follows the maps.  The reference's maps allocate patches on demand without bound (src/sdm/map.cpp:400-411) and share
// them between particles copy-on-write (include/lama/cow_ptr.h:86-118).  Here every particle owns one contiguous region of each
// pool; a region has the capacity ITS particle needs (counts are on the host after every map update) and is moved to a larger one
// -- that particle alone -- when it runs short; the pools themselves grow geometrically when the allocator finds no room.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t MAX_PATCHES = 32767u;      // directory entries are int16

static uint32_t round_up32(uint32_t v) { return (v + 31u) / 32u * 32u; }

// the region capacity a particle with `count` used slots should have so that the next update normally fits (`extra`: head room
// asked for explicitly, e.g. the allocation guard's bound)
static uint32_t want_capacity(uint32_t floor_cap, uint32_t count, uint32_t extra)
{
    const uint32_t head = std::max<uint32_t>(std::max<uint32_t>(32u, count / 4u), extra);
    return std::min<uint32_t>(MAX_PATCHES, std::max<uint32_t>(floor_cap, round_up32(count + head)));
}

static PartRec dev_part(const lama_hip_ctx* c, const HostPart& h)
{
    PartRec r{};
    r.home = h.home; r.dm_cap = h.dm_cap; r.occ_cap = h.occ_cap;
    const PoolChunk& d = c->ms.dm_chunks[h.dm_chunk];
    const PoolChunk& o = c->ms.occ_chunks[h.occ_chunk];
    r.dm_sv = (sv_t*)(d.plane[0] + (size_t)h.dm_off * DM_PLANE_B[0]);
    r.dm_obs = (uint32_t*)(d.plane[1] + (size_t)h.dm_off * DM_PLANE_B[1]);
    r.dm_mask = (uint64_t*)(d.plane[2] + (size_t)h.dm_off * DM_PLANE_B[2]);
    r.occ = (uint32_t*)(o.plane[0] + (size_t)h.occ_off * OCC_PLANE_B[0]);
    r.occ_mask = (uint64_t*)(o.plane[1] + (size_t)h.occ_off * OCC_PLANE_B[1]);
    r.occ_hit = (uint64_t*)(o.plane[2] + (size_t)h.occ_off * OCC_PLANE_B[2]);
    r.rev = (int32_t*)(o.plane[3] + (size_t)h.occ_off * OCC_PLANE_B[3]);
    return r;
}

int32_t upload_part(lama_hip_ctx* c)
{
    c->h_part_stage.resize(c->P);
    for (uint32_t p = 0; p < c->P; ++p) c->h_part_stage[p] = dev_part(c, c->h_part[p]);
    HIPCHK(c, hipMemcpyAsync(c->d_part, c->h_part_stage.data(), sizeof(PartRec) * c->P, hipMemcpyHostToDevice, c->stream));
    return LAMA_HIP_OK;
}

// one more chunk for a pool, of at least `min_patches` (free pool space is all-zero: the chunk is zeroed here).  Nothing that
// exists is copied or moved: a pool grows to whatever the device holds without a second copy of itself.
int32_t add_chunk(lama_hip_ctx* c, bool dm, uint32_t min_patches)
{
    std::vector<PoolChunk>& chunks = dm ? c->ms.dm_chunks : c->ms.occ_chunks;
    uint64_t total = 0;
    for (const PoolChunk& k : chunks) total += k.patches;
    uint64_t want = std::max<uint64_t>(std::max<uint64_t>(min_patches, total / 4u), 1024u);      // geometric: the number of chunks stays small, the last one mostly used
    want = (want + 1023u) / 1024u * 1024u;
    const uint64_t per_patch = dm ? (SV_PATCH_BYTES + 4096 + 128) : (4096 + 128 + 128 + 4);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const uint64_t room = free_b > (1ull << 30) ? free_b - (1ull << 30) : 0;       // leave 1 GB for everything else
        if (want * per_patch > room) want = room / per_patch / 32u * 32u;
        if (want < min_patches)
            return fail(c, LAMA_HIP_E_CAPACITY, std::string(dm ? "distance-map" : "occupancy") + " pool: the device has no room for " + std::to_string(min_patches) + " more patches");
    }
    if (want > 0xFFFFFFF0ull) want = 0xFFFFFFF0ull;
    PoolChunk k;                                                    // (its planes free themselves if a later one fails)
    k.patches = (uint32_t)want;
    const int nplanes = dm ? 3 : 4;
    for (int i = 0; i < nplanes; ++i) {
        const size_t bytes = (size_t)k.patches * (dm ? DM_PLANE_B[i] : OCC_PLANE_B[i]);
        hipError_t e = k.plane[i].alloc(bytes);
        if (e == hipSuccess && !(!dm && i == 3)) e = hipMemsetAsync(k.plane[i], 0, bytes, c->stream);     // (rev is rebuilt per scan)
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, LAMA_HIP_E_CAPACITY, std::string(dm ? "distance-map" : "occupancy") + " pool: " + hipGetErrorString(e));
        }
    }
    chunks.push_back(std::move(k));
    (dm ? c->ra_dm : c->ra_occ).emplace_back();
    (dm ? c->ra_dm : c->ra_occ).back().reset(chunks.back().patches);
    c->ctr.pool_growths += 1;
    return LAMA_HIP_OK;
}

int32_t region_alloc(lama_hip_ctx* c, bool dm, uint32_t n, uint32_t& chunk, uint32_t& off)
{
    std::vector<RegionAlloc>& ras = dm ? c->ra_dm : c->ra_occ;
    for (uint32_t k = 0; k < ras.size(); ++k)
        if (ras[k].alloc(n, off)) { chunk = k; return LAMA_HIP_OK; }
    const int32_t rc = add_chunk(c, dm, n);
    if (rc) return rc;
    chunk = (uint32_t)ras.size() - 1;
    if (!ras[chunk].alloc(n, off)) return fail(c, LAMA_HIP_E_CAPACITY, "patch pool exhausted");
    return LAMA_HIP_OK;
}
static void region_release(lama_hip_ctx* c, bool dm, uint32_t chunk, uint32_t off, uint32_t n) { (dm ? c->ra_dm : c->ra_occ)[chunk].release(off, n); }

// addresses of a region's planes (dm: sv, obs, mask -> [0..2]; occ: occ, occ_mask -> [3..4]) for the clone / zero jobs
static void region_ptrs(const lama_hip_ctx* c, const HostPart& h, void* out[5])
{
    const PartRec r = dev_part(c, h);
    out[0] = r.dm_sv; out[1] = r.dm_obs; out[2] = r.dm_mask; out[3] = r.occ; out[4] = r.occ_mask;
}

// run the jobs in c->h_jobs / c->h_zjobs: `zero_first` = the zero jobs free regions no job reads (resample); else they free the jobs'
// own sources (growth) and run behind the copies
// (j0 / z0: the jobs from these positions of the staging lists on -- set_capacities queues group after group without a host round
// trip in between, so a group's slice of the page-locked lists must stay untouched until the stream has consumed it)
static int32_t run_jobs(lama_hip_ctx* c, bool zero_first, size_t j0 = 0, size_t z0 = 0)
{
    const uint32_t nj = (uint32_t)(c->h_jobs.size() - j0), nz = (uint32_t)(c->h_zjobs.size() - z0);
    if (nj == 0 && nz == 0) return LAMA_HIP_OK;
    HIPCHK(c, c->d_jobs.grow(nj, 256));
    HIPCHK(c, c->d_zjobs.grow(nz, 256));
    const DevParams prm = make_params(c);
    if (nj) HIPCHK(c, hipMemcpyAsync(c->d_jobs, c->h_jobs.data() + j0, sizeof(CloneJob) * nj, hipMemcpyHostToDevice, c->stream));
    if (nz) HIPCHK(c, hipMemcpyAsync(c->d_zjobs, c->h_zjobs.data() + z0, sizeof(ZeroJob) * nz, hipMemcpyHostToDevice, c->stream));
    if (nz && zero_first) hipLaunchKernelGGL(k_zero_regions, dim3(nz, 5, CLONE_SPLIT), dim3(256), 0, c->stream, (const ZeroJob*)c->d_zjobs);
    if (nj) hipLaunchKernelGGL(k_clone_particles, dim3(nj, 7, CLONE_SPLIT), dim3(256), 0, c->stream, prm, (const CloneJob*)c->d_jobs);
    if (nz && !zero_first) hipLaunchKernelGGL(k_zero_regions, dim3(nz, 5, CLONE_SPLIT), dim3(256), 0, c->stream, (const ZeroJob*)c->d_zjobs);
    HIPCHK(c, hipGetLastError());
    return LAMA_HIP_OK;
}

// Give the listed particles regions of (at least) the capacities asked for; a particle whose region is large enough keeps it.  The
// used slots move with one launch for all of them, the old regions go back to the allocator zeroed.  Synchronises the stream.
struct CapRequest { uint32_t p, dm_cap, occ_cap; };
int32_t set_capacities(lama_hip_ctx* c, const std::vector<CapRequest>& reqs)
{
    // The particles of one filter map the same world and outgrow their regions together.  Moved all at once, every new region would
    // have to exist beside every old one (a second copy of the maps, and a pool that never gets its first half back: the freed
    // regions are all smaller than the next request).  So the movers go in groups: a group's old regions are zeroed and released
    // before the next group allocates -- first fit from the lowest address then places the next new regions into the space the
    // previous groups left (neighbouring free regions coalesce), and the pool stays at live data + head room + one group.
    // The groups are ordered by the STREAM, not by the host (one host round trip per group was ~48 of them for one growth
    // event at 3000 particles): group g+1's copies run behind group g's copies and zero jobs, so a region released on the host right
    // after group g was queued may be handed to group g+1.  Every group has its own slice of the page-locked job lists (reserved up
    // front: the lists must not be re-allocated while a transfer is pending) and of nothing else -- the device-side lists are read by
    // a group's kernels before the next group's upload overwrites them, in stream order.
    constexpr size_t GROUP = 64;
    { const int32_t rw = wait_for_groups(c); if (rw) return rw; }      // regions move, the particle table is rewritten: on an idle device only
    struct Old { bool dm; uint32_t chunk, off, cap; };
    bool any = false;
    int32_t err = LAMA_HIP_OK;                                     // a failed allocation: what was planned so far is still carried out (the table,
                                                                   // the regions and their contents stay consistent), then the error is returned
    c->h_jobs.resize(0); c->h_zjobs.resize(0);
    c->h_jobs.reserve(reqs.size()); c->h_zjobs.reserve(reqs.size());
    for (size_t g0 = 0; g0 < reqs.size() && err == LAMA_HIP_OK; g0 += GROUP) {
        std::vector<Old> released;
        const size_t j0 = c->h_jobs.size(), z0 = c->h_zjobs.size();
        for (size_t q = g0; q < std::min(reqs.size(), g0 + GROUP); ++q) {
            const CapRequest& r = reqs[q];
            HostPart& hp = c->h_part[r.p];
            const bool gd = r.dm_cap > hp.dm_cap, go = r.occ_cap > hp.occ_cap;
            if (!gd && !go) continue;
            if (r.dm_cap > MAX_PATCHES || r.occ_cap > MAX_PATCHES) { err = fail(c, LAMA_HIP_E_CAPACITY, "a particle's map exceeds 32767 patches"); break; }
            const HostPart before = hp;
            uint32_t dch = 0, doff = 0, och = 0, ooff = 0;
            if (gd) { err = region_alloc(c, true, r.dm_cap, dch, doff); if (err) break; }
            if (go) { err = region_alloc(c, false, r.occ_cap, och, ooff); if (err) { if (gd) region_release(c, true, dch, doff, r.dm_cap); break; } }
            if (gd) {
                released.push_back(Old{true, hp.dm_chunk, hp.dm_off, hp.dm_cap});
                hp.dm_chunk = dch; hp.dm_off = doff; hp.dm_cap = r.dm_cap;
            }
            if (go) {
                released.push_back(Old{false, hp.occ_chunk, hp.occ_off, hp.occ_cap});
                hp.occ_chunk = och; hp.occ_off = ooff; hp.occ_cap = r.occ_cap;
            }
            CloneJob j{};
            j.src_home = j.dst_home = hp.home;
            j.sdm = c->h_counts[2 * r.p]; j.socc = c->h_counts[2 * r.p + 1];
            void* sp[5]; void* dp[5];
            region_ptrs(c, before, sp); region_ptrs(c, hp, dp);
            ZeroJob z{};
            for (int k = 0; k < 5; ++k) { j.s[k] = sp[k]; j.d[k] = dp[k]; z.d[k] = (sp[k] != dp[k]) ? sp[k] : nullptr; }
            z.ndm = j.sdm; z.nocc = j.socc;
            c->h_jobs.resize(c->h_jobs.size() + 1); c->h_jobs[c->h_jobs.size() - 1] = j;
            c->h_zjobs.resize(c->h_zjobs.size() + 1); c->h_zjobs[c->h_zjobs.size() - 1] = z;
        }
        if (released.empty()) continue;
        any = true;
        const int32_t rc = run_jobs(c, false, j0, z0);
        if (rc) return rc;
        for (const Old& o : released) region_release(c, o.dm, o.chunk, o.off, o.cap);     // (only now: no job of THIS group may land in a region another one of it still reads)
    }
    if (!any) return err;
    const std::string msg = c->error;
    const int32_t rc = upload_part(c);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ctr.arena_growths += 1;
    if (err) c->error = msg;
    return err;
}

// after a map update (counts on the host, stream idle): every particle keeps head room for the next one
int32_t grow_arenas(lama_hip_ctx* c, uint32_t first, uint32_t count)
{
    std::vector<CapRequest> reqs;
    // the guard's bound of the last update says what the next one will ask for (open space: many occupancy patches without a
    // distance-map patch nearby)
    for (uint32_t p = first; p < first + count; ++p) {
        const HostPart& pr = c->h_part[p];
        const uint32_t dmc = (uint32_t)c->h_counts[2 * p], occ = (uint32_t)c->h_counts[2 * p + 1];
        if (dmc > pr.dm_cap || occ > pr.occ_cap) continue;      // a cleanly aborted update of another particle group: its own repeat grows it
        const uint32_t gh = p < c->h_guard.size() ? c->h_guard[p] : 0u;
        uint32_t nd = pr.dm_cap, no = pr.occ_cap;
        if (dmc + std::max<uint32_t>(std::max<uint32_t>(16u, dmc / 16u), gh) > pr.dm_cap) nd = want_capacity(c->floor_dm, dmc, gh + gh / 4u);
        if (occ + std::max<uint32_t>(16u, occ / 16u) > pr.occ_cap) no = want_capacity(c->floor_occ, occ, 0u);
        if (nd > pr.dm_cap || no > pr.occ_cap) reqs.push_back(CapRequest{p, std::max(nd, pr.dm_cap), std::max(no, pr.occ_cap)});
    }
    if (reqs.empty()) return LAMA_HIP_OK;
    return set_capacities(c, reqs);
}

// A map update whose allocation phase failed (ERR_CLEAN_ABORT: no cell was modified): clear what the phase left behind, give the
// particles that ran short what they asked for and run the same update again.  The reference's maps simply allocate
// (src/sdm/map.cpp:400-411).  What a particle asked for: the occupancy allocations count on past the capacity (dir_alloc_one), the
// distance-map bound is the guard's (k_occ_reverse_dir -> guard[2p]).
int32_t recover_update(lama_hip_ctx* c, int32_t e)
{
    ++c->recover_depth;
    // the aborted pass changed nothing on the device; undo what it did on the host (wrap-guard bound, scan / launch counters)
    c->visit_bound = c->saved_visit_bound;
    {
        const lama_hip_counters now = c->ctr;
        c->ctr = c->saved_ctr;
        c->ctr.arena_growths = now.arena_growths; c->ctr.pool_growths = now.pool_growths; c->ctr.dm_patches = now.dm_patches; c->ctr.occ_patches = now.occ_patches;
    }
    DevParams prm = make_params(c);
    const size_t WW = (size_t)c->W * c->W;
    hipLaunchKernelGGL(k_update_cleanup, dim3(c->P, (unsigned)((WW + 255) / 256)), dim3(256), 0, c->stream, prm);
    for (const PoolChunk& k : c->ms.occ_chunks) HIPCHK(c, hipMemsetAsync(k.plane[2], 0, (size_t)k.patches * 128, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_act_count, 0, (size_t)c->P * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_err, 0, sizeof(int32_t), c->stream));
    // the counts hold what every particle WANTED (allocations count on past the capacity); the guard its distance-map bound
    c->h_guard.resize(c->P);
    HIPCHK(c, hipMemcpyAsync(c->h_counts.data(), c->ms.counts, sizeof(int32_t) * 2 * c->P, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_guard.data(), c->d_guard, sizeof(uint32_t) * c->P, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<CapRequest> reqs;
    bool at_limit = false, fixed_counts = false;
    for (uint32_t p = c->last_first; p < c->last_first + c->last_count; ++p) {      // (the particles of the aborted update)
        HostPart& pr = c->h_part[p];
        uint32_t wdm = (uint32_t)c->h_counts[2 * p], wocc = (uint32_t)c->h_counts[2 * p + 1];
        uint32_t nd = pr.dm_cap, no = pr.occ_cap;
        if (wocc > pr.occ_cap) { no = want_capacity(c->floor_occ, wocc, 0u); c->h_counts[2 * p + 1] = (int32_t)pr.occ_cap; fixed_counts = true; }
        if (wdm > pr.dm_cap) { c->h_counts[2 * p] = (int32_t)pr.dm_cap; wdm = pr.dm_cap; fixed_counts = true; nd = want_capacity(c->floor_dm, wdm, 64u); }
        const uint32_t gh = c->h_guard[p];
        if ((e & ERR_DM_CAP) && !c->unguarded_retry && (uint64_t)wdm + gh > pr.dm_cap) {
            if ((uint64_t)wdm + gh > MAX_PATCHES) at_limit = true;      // the guard's bound does not fit the hard limit: run this update unguarded
            nd = std::max(nd, std::min<uint32_t>(MAX_PATCHES, round_up32(wdm + gh + gh / 8u + 16u)));
        }
        if (nd > pr.dm_cap || no > pr.occ_cap) {
            if (no > MAX_PATCHES || (wocc > MAX_PATCHES)) { --c->recover_depth; return LAMA_HIP_E_CAPACITY; }
            reqs.push_back(CapRequest{p, std::max(nd, pr.dm_cap), std::max(no, pr.occ_cap)});
        }
    }
    if (fixed_counts) HIPCHK(c, hipMemcpyAsync(c->ms.counts, c->h_counts.data(), sizeof(int32_t) * 2 * c->P, hipMemcpyHostToDevice, c->stream));
    if (reqs.empty() && !at_limit) { --c->recover_depth; return LAMA_HIP_E_CAPACITY; }     // nothing to grow: a real limit
    if (at_limit && c->unguarded_retry) { --c->recover_depth; return LAMA_HIP_E_CAPACITY; }
    int32_t rc = set_capacities(c, reqs);
    const bool saved_unguarded = c->unguarded_retry;
    c->unguarded_retry = at_limit;
    if (rc == LAMA_HIP_OK) rc = run_update_maps(c, c->last_n, c->last_mtf, c->last_first, c->last_count);
    if (rc == LAMA_HIP_OK) rc = check_device_errors(c, true, false);
    --c->recover_depth;
    c->unguarded_retry = saved_unguarded;
    return rc;
}

int32_t drain_groups(lama_hip_ctx* c);
int32_t apply_resample(lama_hip_ctx* c, const int32_t* idx);
// Collects the status of a map update queued by lama_hip_pf_update_maps_begin (one synchronisation); called at the start of
// every other entry point, so a deferred error surfaces in the next call on the context.
int32_t finish_pending(lama_hip_ctx* c)
{
    if (c->groups_busy) { (void)hipSetDevice(c->cfg.device); const int32_t rg = drain_groups(c); if (rg) { c->resample_deferred = false; return rg; } }
    if (c->pending_maps) {
        c->pending_maps = false;
        (void)hipSetDevice(c->cfg.device);
        const int32_t rc = check_device_errors(c, true, false);
        if (rc) { c->error = "deferred from lama_hip_pf_update_maps_begin: " + c->error; c->resample_deferred = false; return rc; }
    }
    if (c->resample_deferred) {                                     // (lama_hip_pf_resample while the groups were still running)
        c->resample_deferred = false;
        (void)hipSetDevice(c->cfg.device);
        const int32_t rc = apply_resample(c, c->deferred_idx.data());
        if (rc) c->error = "deferred from lama_hip_pf_resample: " + c->error;
        return rc;
    }
    return LAMA_HIP_OK;
}
int32_t refuse_poisoned(lama_hip_ctx* c) { return fail(c, LAMA_HIP_E_STATE, "the context ran out of device memory in the middle of a resample and cannot continue"); }
#define ENTER(c) do { if ((c)->poisoned) return refuse_poisoned(c); const int32_t rc_enter_ = finish_pending(c); if (rc_enter_) return rc_enter_; } while (0)

// hipEvent bracket around a kernel group; resolved (elapsed time read) by resolve_timers() after the API call's final
// stream synchronisation, so profiling adds no host round trips.
struct Timer {
    lama_hip_ctx* c; double* acc; uint64_t* launches; hipEvent_t a = nullptr, b = nullptr;
    StepGroup* g = nullptr; int kind = 0;
    // a particle group's bracket (kind 0: scan match, 1: ray-cast, 2: brushfire): the group's own events on its own stream; read by
    // take_group_timers once the group's next block has arrived
    Timer(lama_hip_ctx* c_, StepGroup* g_, int kind_) : c(c_), acc(nullptr), launches(nullptr), g(g_), kind(kind_)
    {
        if (!c->cfg.profile) return;
        a = g->tev[2 * kind]; b = g->tev[2 * kind + 1];
        (void)hipEventRecord(a, g->s);
    }
    Timer(lama_hip_ctx* c_, double* acc_, uint64_t* l_) : c(c_), acc(acc_), launches(l_)
    {
        if (!c->cfg.profile) return;
        if (c->ev_used + 2 > c->ev_pool.size())
            for (int i = 0; i < 2; ++i) { c->ev_pool.emplace_back(); (void)hipEventCreate(&c->ev_pool.back().h); }
        a = c->ev_pool[c->ev_used++]; b = c->ev_pool[c->ev_used++];
        (void)hipEventRecord(a, c->stream);
    }
    // the ray-cast (ray: kind 1) or brushfire (kind 2) bracket of a map update: its group's, else the context's
    static Timer of_update(lama_hip_ctx* c, StepGroup* g, int kind) { return g ? Timer(c, g, kind) : kind == 1 ? Timer(c, &c->ctr.ms_raycast, &c->ctr.launches_raycast) : Timer(c, &c->ctr.ms_brushfire, &c->ctr.launches_brushfire); }
    void stop()
    {
        if (!c->cfg.profile) return;
        if (g) { (void)hipEventRecord(b, g->s); g->timed |= 1u << kind; return; }
        (void)hipEventRecord(b, c->stream);
        c->pending.push_back({a, b, acc, launches});
    }
};

// the brackets of a group whose stream has passed them: the step's figure is the LONGEST group's (flush_step_timers adds it)
void take_group_timers(lama_hip_ctx* c, StepGroup& g)
{
    for (int k = 0; k < 3; ++k) {
        if (!(g.timed & (1u << k))) continue;
        float ms = 0;
        if (hipEventElapsedTime(&ms, g.tev[2 * k], g.tev[2 * k + 1]) == hipSuccess) { c->step_ms[k] = std::max(c->step_ms[k], (double)ms); c->step_ms_any[k] = true; }
    }
    g.timed = 0;
}

// end of a grouped step (or of a drain): ms_* accumulate the longest group's bracket, launches_* count updates; the longest chain of the
// update whose statuses have just been collected keeps its pool-wide meaning
void flush_step_figures(lama_hip_ctx* c)
{
    double* acc[3] = {&c->ctr.ms_scan_match, &c->ctr.ms_raycast, &c->ctr.ms_brushfire};
    uint64_t* cnt[3] = {&c->ctr.launches_scan_match, &c->ctr.launches_raycast, &c->ctr.launches_brushfire};
    for (int k = 0; k < 3; ++k) {
        if (c->step_ms_any[k]) { *acc[k] += c->step_ms[k]; *cnt[k] += 1; }
        c->step_ms[k] = 0; c->step_ms_any[k] = false;
    }
    c->ctr.ms_update_maps = c->ctr.ms_raycast + c->ctr.ms_brushfire;
    c->ctr.launches_update_maps = c->ctr.launches_raycast;
    if (c->chain_dirty) {
        uint64_t mx = 0;
        for (uint64_t v : c->h_chain) mx = std::max(mx, v);
        c->ctr.bf_longest_chain_sum += mx; c->ctr.bf_longest_chain_last = mx;
        std::fill(c->h_chain.begin(), c->h_chain.end(), 0);
        c->chain_dirty = false;
    }
}

void resolve_timers(lama_hip_ctx* c)      // call after the stream has been synchronised
{
    for (auto& t : c->pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) { *t.acc += ms; *t.launches += 1; }
    }
    c->pending.clear();
    c->ev_used = 0;
    c->ctr.ms_update_maps = c->ctr.ms_raycast + c->ctr.ms_brushfire;
    c->ctr.launches_update_maps = c->ctr.launches_raycast;
}

// The reference's maps have no extent (src/sdm/map.cpp:400-411); the device window has one, but it MOVES and (round 4) GROWS.  The
// host keeps the box of everything that can be mapped so far -- the union, over all updates, of pose +- scan reach of every
// particle, in absolute patch coordinates (a superset of the mapped area; imported particles bring their sender's).  Before a map
// update (and before an import) the window must hold that box:
//   * it fits the window side: the window is moved by the smallest patch-granular step that holds it (plus a little slack in the
//     direction of the move) -- a permutation of the two directories of every particle (k_shift_window; the other particle set's
//     directories are the scratch destination, then the pointers are swapped);
//   * it does not: the directories are re-allocated with a larger side (at least half as large again, a multiple of 8, at most
//     LAMA_HIP_MAX_WINDOW = 1016 patches = 1.6 km at 0.05 m) and re-tiled by the same kernel; arenas, cells and slots are untouched.
// Only a map wider than 1016 patches remains LAMA_HIP_E_WINDOW (the kernels report what really falls outside).
constexpr int64_t LAMA_HIP_MAX_WINDOW = 1016;

int32_t regrid_window(lama_hip_ctx* c, uint32_t newW, int64_t nox, int64_t noy)
{
    const int64_t ox = c->wx0 >> 5, oy = c->wy0 >> 5;
    const int dx = (int)(nox - ox), dy = (int)(noy - oy);
    const size_t WW = (size_t)c->W * c->W, nWW = (size_t)newW * newW, P = c->P;
    if (!c->initialised && newW == c->W) { c->wx0 = (uint32_t)(nox * 32); c->wy0 = (uint32_t)(noy * 32); return LAMA_HIP_OK; }   // nothing mapped yet
    { const int32_t rw = wait_for_groups(c); if (rw) return rw; }      // the directories are every particle's
    // both directories of every home are re-tiled into fresh arrays (same side: a permutation; larger side: the window grew), then the
    // old arrays are released.  A failed allocation leaves the window as it was (nothing leaks).
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && 2 * P * nWW * 2 + (1ull << 28) > free_b)
            return fail(c, LAMA_HIP_E_WINDOW, "not enough device memory to re-tile the window directories (" + std::to_string(2 * P * nWW * 2 >> 20) + " MB for a " + std::to_string(newW) + "-patch window)");
    }
    DevBuf<int16_t> nd[2];
    for (int k = 0; k < 2; ++k) {
        hipError_t e = nd[k].alloc(P * nWW);
        if (e == hipSuccess && newW != c->W) e = hipMemsetAsync(nd[k], 0xFF, P * nWW * 2, c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "window directories");
    }
    const dim3 grid((unsigned)P, (unsigned)((std::max(WW, nWW) + 255) / 256));
    int16_t* const to_dm = nd[0]; int16_t* const to_occ = nd[1];   // (launch arguments are plain pointers: the owners are not copied)
    hipLaunchKernelGGL(k_shift_window, grid, dim3(256), 0, c->stream, c->ms.dm_dir, to_dm, c->W, newW, dx, dy, WW, nWW, c->d_err);
    hipLaunchKernelGGL(k_shift_window, grid, dim3(256), 0, c->stream, c->ms.occ_dir, to_occ, c->W, newW, dx, dy, WW, nWW, c->d_err);
    {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "k_shift_window");
    }
    c->ms.dm_dir.swap(nd[0]); c->ms.occ_dir.swap(nd[1]);           // (the old directories are released with nd)
    if (newW != c->W) {
        c->W = newW; c->WC = newW * 32; c->cfg.window_patches = newW;
        c->ctr.window_growths += 1;
    }
    c->wx0 = (uint32_t)(nox * 32); c->wy0 = (uint32_t)(noy * 32);
    c->ctr.window_shifts += 1;
    c->ctr.window_patches = c->W;
    return LAMA_HIP_OK;
}

// the window must hold the box [x0, x1] x [y0, y1] (absolute patches): union it into the mapped box, then move / grow the window
int32_t ensure_window(lama_hip_ctx* c, int64_t x0, int64_t x1, int64_t y0, int64_t y1)
{
    if (!c->mb_valid) { c->mbx0 = x0; c->mbx1 = x1; c->mby0 = y0; c->mby1 = y1; c->mb_valid = true; }
    else { c->mbx0 = std::min(c->mbx0, x0); c->mbx1 = std::max(c->mbx1, x1); c->mby0 = std::min(c->mby0, y0); c->mby1 = std::max(c->mby1, y1); }
    const int64_t ox = c->wx0 >> 5, oy = c->wy0 >> 5, W = c->W;
    if (c->debug_window) std::fprintf(stderr, "ensure_window: box x [%ld, %ld] y [%ld, %ld] mapped x [%ld, %ld] y [%ld, %ld] window x [%ld, %ld) y [%ld, %ld)\n", (long)x0, (long)x1, (long)y0, (long)y1, (long)c->mbx0, (long)c->mbx1, (long)c->mby0, (long)c->mby1, (long)ox, (long)(ox + W), (long)oy, (long)(oy + W));
    if (c->mbx0 >= ox && c->mbx1 < ox + W && c->mby0 >= oy && c->mby1 < oy + W) return LAMA_HIP_OK;
    const int64_t span = std::max(c->mbx1 - c->mbx0 + 1, c->mby1 - c->mby0 + 1);
    int64_t newW = W;
    if (span > W) newW = std::min<int64_t>(LAMA_HIP_MAX_WINDOW, std::max<int64_t>((span + 8 + 7) / 8 * 8, (W + W / 2 + 7) / 8 * 8));
    // what the (new) window must hold: the whole mapped box when it fits, else at least this call's box (the kernels then report
    // what really falls outside: LAMA_HIP_E_WINDOW)
    int64_t hx0 = c->mbx0, hx1 = c->mbx1, hy0 = c->mby0, hy1 = c->mby1;
    if (span > newW) { hx0 = x0; hx1 = x1; hy0 = y0; hy1 = y1; if (x1 - x0 + 1 > newW || y1 - y0 + 1 > newW) return LAMA_HIP_OK; }
    auto place = [&](int64_t o, int64_t lo, int64_t hi) {
        const int64_t a = hi - newW + 1, b = lo;              // admissible origins: a <= origin <= b
        int64_t no = std::min(std::max(o, a), b);
        if (no > o) no = std::min(no + 4, b); else if (no < o) no = std::max(no - 4, a);
        return no;
    };
    const int64_t nox = c->initialised ? place(ox, hx0, hx1) : (hx0 + hx1 + 1) / 2 - newW / 2;
    const int64_t noy = c->initialised ? place(oy, hy0, hy1) : (hy0 + hy1 + 1) / 2 - newW / 2;
    return regrid_window(c, (uint32_t)newW, nox, noy);
}

// a context whose map is placed by something else than a first scan (an uploaded map, a list of obstacles, integrated key scans):
// identity poses, and the window has been placed by the caller
int32_t start_without_first_scan(lama_hip_ctx* c)
{
    if (c->initialised) return LAMA_HIP_OK;
    for (uint32_t p = 0; p < c->P; ++p) { c->h_poses[4 * p] = 1.0; c->h_poses[4 * p + 1] = 0.0; c->h_poses[4 * p + 2] = 0.0; c->h_poses[4 * p + 3] = 0.0; }
    HIPCHK(c, hipMemcpyAsync(c->d_poses, c->h_poses.data(), sizeof(double) * 4 * c->P, hipMemcpyHostToDevice, c->stream));
    c->initialised = true;
    return LAMA_HIP_OK;
}

int32_t fit_window(lama_hip_ctx* c, const Affine& mtf, uint32_t first, uint32_t count)
{
    // no cell further than truncated_range from the sensor is touched (src/pf_slam2d.cpp:470-476): "no return" readings far
    // beyond it must not push mapped patches out of the window
    double far = c->scan_reach;
    if (c->cfg.ray_rule == 0 && c->cfg.truncated_range > 0.0) far = std::min(far, c->cfg.truncated_range);
    // padding: the brushfire allocates distance-map patches up to guard_r patches beyond a hit (make_params: ceil(l2_max / resolution)
    // + 1 cells), plus one patch for the rounding of the box.  permute_particles copies only the directory rows inside this box, so a
    // patch outside it would be lost by a clone (a fixed 2 patches were too few for l2_max above 64 cells).
    const uint32_t guard_r = guard_radius(c);
    const double reach = far + std::sqrt(mtf.t[0] * mtf.t[0] + mtf.t[1] * mtf.t[1]) + (double)(guard_r + 1u) * 32.0 * c->cfg.resolution;
    double xlo = 1e300, xhi = -1e300, ylo = 1e300, yhi = -1e300;
    for (uint32_t p = first; p < first + count; ++p) {
        const double x = c->h_poses[4 * p + 2], y = c->h_poses[4 * p + 3];
        xlo = std::min(xlo, x - reach); xhi = std::max(xhi, x + reach);
        ylo = std::min(ylo, y - reach); yhi = std::max(yhi, y + reach);
    }
    auto patch = [&](double w) { return (int64_t)std::floor((c->scale * w + c->off) / 32.0); };
    return ensure_window(c, patch(xlo), patch(xhi), patch(ylo), patch(yhi));
}

// how many particles may go to the big-queue stage beside the first one: an 84 KB workgroup takes the LDS of seven first-stage
// workgroups, and a first stage that no longer fits the chip in one round (12 per CU) costs far more than the routing saves
static uint32_t route_places(const lama_hip_ctx* c, uint32_t count)
{
    const uint32_t slots = c->num_cus * 12u;
    if (c->route_forced || count >= slots) return c->route_cap;                 // (several rounds anyway)
    return std::min<uint32_t>(c->route_cap, std::max<uint32_t>(8u, (slots - count) / 7u));
}

// A map update is decided (plan_update), noted (note_update_begin) and launched (launch_update).  The plan's defaults are the plain parallel update: all a particle group ever runs (step_can_group); the rest is decided for the main stream only.
struct UpdatePlan {
    hipStream_t s = nullptr; const double* d_pts = nullptr; uint32_t n = 0, first = 0, count = 0;      // the main lane's stream, the scan as uploaded on it
    DevParams prm;                                                    // (error word and hand-over lists: the context's or a group's)
    lama_dev::TfTable tab = lama_dev::TfTable(); bool tf_by_value = false;     // the scan transforms travel with the launches, d_tfs is not read
    StepGroup* timers = nullptr;                                      // whose brackets time the update: the group's own, else the context's
    bool sequential = false, guarded = true, canon = false, two_waves = false, route = false, early_lane = false;
    bool prev_routed = false; uint32_t host_n = 0;                    // early lane: d_heavy holds the previous update's routed particles; entries of h_hlist
    uint32_t route_places = 0; unsigned gy = 0, resume_grid = 0; bool replay_large = true;
};

// the parallel kernels implement the frequency counters and the PF ray rule only; every hit is an order-sensitive visit (the list holds
// active_capacity of them), the visit key carries the beam index in 13 bits (act_key) and k_ray_patches keeps one 64-beam chunk per lane
static bool parallel_raycast_ruled_out(const lama_hip_ctx* c, uint32_t n)
{
    return c->cfg.sequential_raycast == 1 || c->cfg.occupancy_policy == 1 || c->cfg.ray_rule == 1 || n > 4096u || (uint64_t)n + 4096u > c->cfg.active_capacity;
}

// every decision of the map update of particles [first, first + count); g: of that particle group, on its stream; wrap_sequential: wrap_guard_probe's answer
UpdatePlan plan_update(lama_hip_ctx* c, uint32_t n, uint32_t first, uint32_t count, bool wrap_sequential, StepGroup* g = nullptr)
{
    UpdatePlan u;
    u.n = n; u.first = first; u.count = count; u.timers = g; u.tf_by_value = g && count <= (uint32_t)lama_dev::ARG_BLOCK;
    u.s = g ? g->s : (hipStream_t)c->stream; u.d_pts = g ? (const double*)g->d_pts : (const double*)c->d_pts; u.prm = g ? group_params(c, *g) : make_params(c);
    u.two_waves = c->cfg.brushfire_waves == 2 || (c->cfg.brushfire_waves == 0 && count <= BF_TW_MAX_PARTICLES);
    u.gy = count <= 64 ? 128u : (count >= 1024 ? 8u : 32u);      // workgroups per particle; a full chip needs fewer
#ifdef LAMA_WAVE_SIM
    u.gy = 4u;                                   // (tests/sim runs every thread as a fiber: 128 mostly idle workgroups per particle cost it minutes)
#endif
    u.replay_large = count <= 512; u.resume_grid = std::min<unsigned>(count, 256u);      // (workgroups that walk the usually empty hand-over lists)
    if (g) return u;
    u.sequential = parallel_raycast_ruled_out(c, n) || wrap_sequential;      // both ray-casts are bit-exact; the parallel one wins while the chip is not full
    u.guarded = c->cfg.ray_rule == 0;            // the allocation walk uses the PF ray rule (else: pregrow_unguarded)
    u.canon = c->cfg.brushfire_mode == 1;        // opt-in parallel variant; whatever it leaves (qsizes != 0) falls through to the exact stages
    u.route = u.two_waves && count >= c->route_min_count && c->route_cap > 0; u.route_places = route_places(c, count);
    // early lane: the particles the previous update routed (long chains, usually long again) ...
    if (u.sequential || !(c->early_on && u.two_waves && !u.canon && first == 0 && count == c->P &&
                          count >= std::max<uint32_t>(c->route_min_count, c->early_min_count) && c->route_cap > 0)) return u;
    if (c->ll_valid) {
        // ... and those whose scan match of this step fitted far worse than the pool's (log-likelihood below 2.5 times the mean, both negative)
        double mean = 0; for (uint32_t p = 0; p < c->P; ++p) mean += c->h_ll[p]; mean /= c->P;
        const double lim = 2.5 * std::min(mean, 0.0) - 5.0;
        std::vector<std::pair<double, uint32_t>> cand;
        for (uint32_t p = 0; p < c->P; ++p) if (c->h_ll[p] < lim) cand.emplace_back(c->h_ll[p], p);
        if (cand.size() > u.route_places) { std::partial_sort(cand.begin(), cand.begin() + u.route_places, cand.end()); cand.resize(u.route_places); }
        c->h_hlist.resize(256);
        for (auto& e : cand) c->h_hlist[u.host_n++] = e.second;
    }
    u.prev_routed = c->early_ok && c->early_candidates > 0; u.early_lane = u.host_n > 0 || u.prev_routed;
    return u;
}

// A uint16 `visited` counter that wraps INSIDE a scan makes the order of the visits matter (k_occ_max_visited): where the host's bound
// cannot rule that out, the device is asked for the largest counter (`bound`, else left at -1).  note_update_begin takes the answer.
int32_t wrap_guard_probe(lama_hip_ctx* c, uint32_t n, int64_t& bound)
{
    if (parallel_raycast_ruled_out(c, n) || (uint64_t)c->visit_bound + n < 65536u) return LAMA_HIP_OK;
    uint32_t m = 0;
    if (c->initialised) {
        const DevParams prm = make_params(c);
        (void)hipMemsetAsync(c->d_scalar, 0, sizeof(uint32_t), c->stream);
        hipLaunchKernelGGL(k_occ_max_visited, dim3(c->P), dim3(256), 0, c->stream, prm, c->d_scalar);
        HIPCHK(c, hipMemcpyAsync(&m, c->d_scalar, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    bound = m;
    return LAMA_HIP_OK;
}

// the allocation phase walks by the PF ray rule: under LidarOdometry's rule the particles get every patch a scan of this reach can touch beforehand
int32_t pregrow_unguarded(lama_hip_ctx* c, uint32_t first, uint32_t count)
{
    if (c->cfg.ray_rule == 0) return LAMA_HIP_OK;
    const double rp = c->scan_reach / (32.0 * c->cfg.resolution) + 2.5;
    const uint32_t bound = (uint32_t)std::min(32767.0, std::ceil(3.1416 * rp * rp));
    std::vector<CapRequest> reqs;
    for (uint32_t p = first; p < first + count; ++p) {
        const HostPart& pr = c->h_part[p];
        const uint32_t nd = std::min<uint32_t>(MAX_PATCHES, round_up32((uint32_t)c->h_counts[2 * p] + bound)), no = std::min<uint32_t>(MAX_PATCHES, round_up32((uint32_t)c->h_counts[2 * p + 1] + bound));
        if (nd > pr.dm_cap || no > pr.occ_cap) reqs.push_back(CapRequest{p, std::max(nd, pr.dm_cap), std::max(no, pr.occ_cap)});
    }
    return reqs.empty() ? LAMA_HIP_OK : set_capacities(c, reqs);
}

// the host-side effects of beginning an update (a grouped step: once, for the pool); saved_*: what a repeat must not apply twice
void note_update_begin(lama_hip_ctx* c, const Affine& mtf, const UpdatePlan& u, int64_t probed)
{
    c->last_mtf = mtf; c->last_first = u.first; c->last_count = u.count; c->last_guarded = u.guarded;
    if (c->recover_depth == 0) { c->saved_visit_bound = c->visit_bound; c->saved_ctr = c->ctr; }
    if (probed >= 0) { c->visit_bound = (uint32_t)probed; if (u.sequential) c->ctr.wrap_guard_scans += 1; }
    c->visit_bound = (uint32_t)std::min<uint64_t>((uint64_t)c->visit_bound + u.n, 65535u);
    if (u.sequential) c->ctr.sequential_raycast_scans += 1; else c->ctr.parallel_raycast_scans += 1;
    c->early_ok = u.route && u.first == 0 && u.count == c->P;      // (early lane included; a resample takes it back)
}

// the scan transforms of particles [first, first + count): into `tab` (launch arguments) or to d_tfs on stream s
int32_t stage_scan_tfs(lama_hip_ctx* c, const Affine& mtf, uint32_t first, uint32_t count, hipStream_t s, lama_dev::TfTable* tab)
{
    PinVec<double>& tfs = c->h_tfs; tfs.resize((size_t)c->P * 12);
    for (uint32_t p = first; p < first + count; ++p) host_scan_tf(&c->h_poses[4 * p], mtf, &tfs[12 * (size_t)p]);
    if (tab) std::memcpy(tab->v, &tfs[12 * (size_t)first], sizeof(double) * 12 * count);
    else HIPCHK(c, hipMemcpyAsync(c->d_tfs + 12 * (size_t)first, &tfs[12 * (size_t)first], sizeof(double) * 12 * count, hipMemcpyHostToDevice, s));
    return LAMA_HIP_OK;
}

// Workgroup b of a launch goes to XCD b mod 8, each with its own L2: a two-dimensional launch (particle, something) keeps a particle's
// workgroups on the XCD of its one-dimensional launches only when its particle dimension is a multiple of 8 (else the brushfire finds
// none of its cells in the L2 its ray-cast wrote them through).  The whole pool, or its last block, rounds up (the kernels skip
// particles >= P); the blocks in front cannot -- the next particle is another group's -- and are multiples of 8 where the split allows.
static unsigned xcd_grid(const lama_hip_ctx* c, uint32_t first, uint32_t count)
{
    return first + count == c->P ? (count + 7u) / 8u * 8u : count;
}

// allocation phase of a map update (ray records, hit cells' patches, the patches the rays cross, the bound on the distance-map patches
// still to come): afterwards either every patch the update needs exists or an error bit is set and no map cell has been modified
// (tab: k_ray_hits and k_occ_reverse_dir take the scan transforms as a launch argument, the plan's TfTable, or read d_tfs: NoTable)
template <class Tab>
int32_t launch_allocation_phase(lama_hip_ctx* c, const UpdatePlan& u, int alloc_only, const Tab& tab)
{
    const uint32_t n = u.n, first = u.first, count = u.count;
    const double* const d_tfs = u.tf_by_value ? nullptr : (const double*)c->d_tfs;
    const size_t need = (size_t)c->P * n;
    if (need > c->d_rrec.n) {                                       // all three are freed before any is allocated
        c->d_rrec.reset(); c->d_rbbox.reset(); c->d_rchunk.reset();
        hipError_t e = c->d_rrec.alloc(need);
        if (e == hipSuccess) e = c->d_rbbox.alloc(need);
        if (e == hipSuccess) e = c->d_rchunk.alloc((size_t)c->P * ((n + 63) / 64));     // per 64 beams of a particle
        if (e != hipSuccess) { c->d_rrec.reset(); return hip_fail(c, e, "ray buffers"); }
    }
    const dim3 hits_grid(xcd_grid(c, first, count), (n + 255) / 256);
    hipLaunchKernelGGL(k_ray_hits<Tab>, hits_grid, dim3(256), 0, u.s, u.prm, u.d_pts, (int)n, d_tfs, (int)first,
                       (lama_dev::RayRec*)c->d_rrec, (uint64_t*)c->d_rbbox, alloc_only, (lama_dev::RayChunk*)c->d_rchunk, tab);
    const int rw_seg = count <= 64 ? 4 : 1;
    hipLaunchKernelGGL(k_ray_alloc_walk, dim3(xcd_grid(c, first, count), (n * rw_seg + 255) / 256), dim3(256), 0, u.s, u.prm, (const lama_dev::RayRec*)c->d_rrec, (int)n, (int)first, rw_seg);
    double far = c->scan_reach;                                   // no cell further than truncated_range from the sensor is touched
    if (c->cfg.truncated_range > 0.0) far = std::min(far, c->cfg.truncated_range);
    const int reach_cells = (int)std::ceil(far * c->scale) + 2;
    // the directory rows that can hold a patch at all: the mapped box (ensure_window; what permute_particles copies)
    uint32_t row0 = 0, row1 = c->W - 1;
    if (c->mb_valid) {
        const int64_t oy = c->wy0 >> 5, W = c->W;
        const int64_t lo = std::min(std::max(c->mby0 - oy, (int64_t)0), W - 1), hi = std::min(std::max(c->mby1 - oy, (int64_t)0), W - 1);
        if (hi >= lo) { row0 = (uint32_t)lo; row1 = (uint32_t)hi; }
    }
    hipLaunchKernelGGL(k_occ_reverse_dir<Tab>, dim3(count), dim3(256), 0, u.s, u.prm, (int)first, d_tfs, reach_cells, c->unguarded_retry ? 1 : 0, row0, row1, tab);
    return LAMA_HIP_OK;
}
int32_t launch_allocation_phase(lama_hip_ctx* c, const UpdatePlan& u, int alloc_only) { return u.tf_by_value ? launch_allocation_phase(c, u, alloc_only, u.tab) : launch_allocation_phase(c, u, alloc_only, lama_dev::NoTable()); }

// The early lane's ray-cast kernels run HERE, on an idle chip, its brushfire on a stream of its own; the main lane waits for an event
// recorded directly in front of that brushfire, so that its big-queue workgroups are placed first (order of dispatch: DESIGN.md section 4)
int32_t launch_early_lane(lama_hip_ctx* c, const UpdatePlan& u)
{
    DevParams pe = u.prm; pe.elist = c->d_elist; pe.elist_n = c->d_slow_n + 4; pe.lane = 1;
    hipLaunchKernelGGL(k_ray_patches, dim3(u.route_places, 128u), dim3(256), 0, c->stream, pe, (const lama_dev::RayRec*)c->d_rrec,
                       (const uint64_t*)c->d_rbbox, (const lama_dev::RayChunk*)c->d_rchunk, (int)u.n, 0);
    hipLaunchKernelGGL((k_ray_replay<RP_SORT_SMALL, RP_SORT_SMALL, false, RP_BLOCK_LARGE>), dim3(u.route_places), dim3(RP_BLOCK_LARGE), 0, c->stream, pe, 0);
    hipLaunchKernelGGL((k_ray_replay<8192, 8192, true, RP_BLOCK_LARGE>), dim3(u.route_places), dim3(RP_BLOCK_LARGE), 0, c->stream, pe, 0);
    HIPCHK(c, hipEventRecord(c->ev_alloc, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream3, c->ev_alloc, 0));
    hipLaunchKernelGGL(k_mark_early, dim3(1), dim3(64), 0, c->stream3, pe);
    HIPCHK(c, hipEventRecord(c->ev_go, c->stream3));
    hipLaunchKernelGGL((k_brushfire<LQ_BIG, RQ_BIG, true, true>), dim3(u.route_places), dim3(2 * UM_BLOCK), c->big_stage_pad, c->stream3, pe, 0, 2);
    HIPCHK(c, hipEventRecord(c->ev_early, c->stream3));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_go, 0));
    return LAMA_HIP_OK;
}

// patch-centric visits: a workgroup owns one occupancy patch of one particle, no global atomics on the counters
int32_t launch_parallel_raycast(lama_hip_ctx* c, const UpdatePlan& u)
{
    const int first = (int)u.first; const uint32_t host_n = u.host_n;
    if (u.early_lane) {                                             // the early list, before anything is queued
        if (host_n) HIPCHK(c, hipMemcpyAsync(c->d_hlist, c->h_hlist.data(), sizeof(uint32_t) * host_n, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_early_list, dim3(1), dim3(256), 0, c->stream, u.prev_routed ? (const uint8_t*)c->d_heavy : (const uint8_t*)nullptr,
                           (const uint32_t*)c->d_hlist, host_n, c->d_early, c->d_elist, c->d_slow_n + 4, (int)c->P, u.route_places);
    }
    { const int32_t ra = launch_allocation_phase(c, u, 0); if (ra) return ra; }
    DevParams prm = u.prm;
    if (u.early_lane) { const int32_t re = launch_early_lane(c, u); if (re) return re; prm.early = c->d_early; }     // everybody else: the main lane skips them
    hipLaunchKernelGGL(k_ray_patches, dim3(xcd_grid(c, u.first, u.count), u.gy), dim3(256), 0, u.s, prm, (const lama_dev::RayRec*)c->d_rrec,
                       (const uint64_t*)c->d_rbbox, (const lama_dev::RayChunk*)c->d_rchunk, (int)u.n, first);
    if (u.replay_large) {
        hipLaunchKernelGGL((k_ray_replay<RP_SORT_SMALL, RP_SORT_SMALL, false, RP_BLOCK_LARGE>), dim3(u.count), dim3(RP_BLOCK_LARGE), 0, u.s, prm, first);
        hipLaunchKernelGGL((k_ray_replay<8192, 8192, true, RP_BLOCK_LARGE>), dim3(u.resume_grid), dim3(RP_BLOCK_LARGE), 0, u.s, prm, first);
    } else {
        hipLaunchKernelGGL((k_ray_replay<RP_SORT_SMALL, RP_SORT_SMALL, false, RP_BLOCK_SMALL>), dim3(u.count), dim3(RP_BLOCK_SMALL), 0, u.s, prm, first);
        hipLaunchKernelGGL((k_ray_replay<8192, 8192, true, RP_BLOCK_SMALL>), dim3(u.resume_grid), dim3(RP_BLOCK_SMALL), 0, u.s, prm, first);
    }
    return LAMA_HIP_OK;
}

// stage 1: small LDS window, every particle; 2: big window, resumes particles whose queue outgrew stage 1; 3: HBM queue for anything larger
int32_t launch_brushfire(lama_hip_ctx* c, const UpdatePlan& u)
{
    const int first = (int)u.first;
    DevParams prm = u.prm; if (u.early_lane) prm.early = c->d_early;
    if (u.canon) hipLaunchKernelGGL(k_brushfire_canon, dim3(u.count), dim3(CN_BLOCK), 0, u.s, prm, first);
    if (u.route) {
        // the big-queue workgroups (84 KB of LDS) must be placed BEFORE the first stage, which skips them, fills every CU's LDS: it goes to stream2 behind an event
        prm.heavy = c->d_heavy;
        hipLaunchKernelGGL(k_bf_route, dim3(1), dim3(256), 0, c->stream, prm, first, (int)u.count, c->route_min_events, c->route_percent, u.route_places);
        HIPCHK(c, hipEventRecord(c->ev_route, c->stream));
        hipLaunchKernelGGL((k_brushfire<LQ_BIG, RQ_BIG, true, true>), dim3(u.route_places), dim3(2 * UM_BLOCK), 0, c->stream, prm, first, 1);
        HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_route, 0));
        hipLaunchKernelGGL((k_brushfire<LQ_SMALL, RQ_SMALL, false, true>), dim3(u.count), dim3(2 * UM_BLOCK), 0, c->stream2, prm, first, 0);
        HIPCHK(c, hipEventRecord(c->ev_heavy, c->stream2));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_heavy, 0));
    } else if (u.two_waves) hipLaunchKernelGGL((k_brushfire<LQ_SMALL, RQ_SMALL, false, true>), dim3(u.count), dim3(2 * UM_BLOCK), 0, u.s, prm, first, 0);
    else hipLaunchKernelGGL((k_brushfire<LQ_SMALL, RQ_SMALL, false, false>), dim3(u.count), dim3(UM_BLOCK), 0, u.s, prm, first, 0);
    if (u.two_waves) hipLaunchKernelGGL((k_brushfire<LQ_BIG, RQ_BIG, true, true>), dim3(u.resume_grid), dim3(2 * UM_BLOCK), 0, u.s, prm, first, 0);
    else hipLaunchKernelGGL((k_brushfire<LQ_BIG, RQ_BIG, true, false>), dim3(u.resume_grid), dim3(UM_BLOCK), 0, u.s, prm, first, 0);
    if (u.early_lane) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_early, 0));
    hipLaunchKernelGGL(k_brushfire_slow, dim3(u.count), dim3(UM_BLOCK), 0, u.s, prm, first);
    return LAMA_HIP_OK;
}

// ray_timer: the ray-cast bracket, which the caller has opened (the pool's: in front of its fills)
int32_t launch_update(lama_hip_ctx* c, const UpdatePlan& u, Timer& ray_timer)
{
    int32_t rc = !u.sequential ? launch_parallel_raycast(c, u) : u.guarded ? launch_allocation_phase(c, u, 1) : LAMA_HIP_OK;
    if (rc) return rc;
    if (u.sequential) hipLaunchKernelGGL(k_raycast, dim3(u.count), dim3(UM_BLOCK), 0, u.s, u.prm, u.d_pts, (int)u.n, c->d_tfs, (int)u.first);      // beam by beam
    ray_timer.stop();
    HIPCHK(c, hipGetLastError());
    Timer t = Timer::of_update(c, u.timers, 2);
    c->ctr.brushfire_mode = c->cfg.brushfire_mode; c->ctr.brushfire_waves = u.two_waves ? 2u : 1u;
    rc = launch_brushfire(c, u);
    if (rc) return rc;
    t.stop();
    HIPCHK(c, hipGetLastError());
    return LAMA_HIP_OK;
}

int32_t run_update_maps(lama_hip_ctx* c, uint32_t n, const Affine& mtf, uint32_t first, uint32_t count)
{
    int32_t rc = fit_window(c, mtf, first, count);
    if (rc == LAMA_HIP_OK) rc = stage_scan_tfs(c, mtf, first, count, c->stream, nullptr);
    if (rc) return rc;
    Timer t = Timer::of_update(c, nullptr, 1);
    const bool whole = first == 0 && count == c->P;      // hand-over counts and statistics are adjacent (ctx_create); a block leaves the others' statistics alone
    (void)hipMemsetAsync(c->d_slow_n, 0, whole ? 32 + sizeof(uint64_t) * 4 * c->P : 32, c->stream);
    if (!whole) (void)hipMemsetAsync(c->d_stats + 4 * (size_t)first, 0, sizeof(uint64_t) * 4 * count, c->stream);
    int64_t probed = -1; rc = wrap_guard_probe(c, n, probed);
    if (rc == LAMA_HIP_OK) rc = pregrow_unguarded(c, first, count);
    if (rc) return rc;
    const UpdatePlan u = plan_update(c, n, first, count, probed >= 0 && (uint64_t)probed + n >= 65536u);
    note_update_begin(c, mtf, u, probed);
    return launch_update(c, u, t);
}


// new particle i := old particle idx[i] (pose + both maps), IN PLACE (resample(), src/pf_slam2d.cpp:558-574; the first scan's
// copies, :204-216).  The first new particle that draws an old one takes over its home and regions -- nothing moves --, every further
// copy of it goes to the home of a particle nobody drew; its regions are reused when they have the source's capacities, else they
// go back to the allocator (zeroed where used) and fresh ones are taken.  What the device copies is exactly the clones.
int32_t permute_particles(lama_hip_ctx* c, const int32_t* idx)
{
    const uint32_t P = c->P;
    std::vector<uint8_t> taken(P, 0);
    std::vector<HostPart> np(P);
    std::vector<int32_t> nc(2 * (size_t)P);
    std::vector<double> npose(4 * (size_t)P);
    std::vector<uint32_t> clones;                                   // new particles that need a copy
    for (uint32_t i = 0; i < P; ++i) {
        const uint32_t j = (uint32_t)idx[i];
        std::memcpy(&npose[4 * i], &c->h_poses[4 * j], sizeof(double) * 4);
        nc[2 * i] = c->h_counts[2 * j]; nc[2 * i + 1] = c->h_counts[2 * j + 1];
        if (!taken[j]) { taken[j] = 1; np[i] = c->h_part[j]; } else clones.push_back(i);
    }
    std::vector<uint32_t> dead;                                     // old particles nobody drew: their homes / regions are free
    for (uint32_t j = 0; j < P; ++j) if (!taken[j]) dead.push_back(j);
    c->h_jobs.resize(0); c->h_zjobs.resize(0);
    c->clone_bytes = 0;
    const size_t WW = (size_t)c->W * c->W;
    // the directory rows that can hold a patch at all: the mapped box of the context (a superset of every particle's map, ensure_window);
    // W is a multiple of 8, so a row is a whole number of 16-byte units
    uint32_t dir_off16 = 0, dir_n16 = (uint32_t)(WW * 2 / 16);
    {
        const int64_t oy = c->wy0 >> 5, W = c->W;                   // (the rows of mapped_box_rel(c, 1))
        if (c->mb_valid) {
            const int64_t lo = std::min(std::max(c->mby0 - oy, (int64_t)0), W - 1), hi = std::min(std::max(c->mby1 - oy, (int64_t)0), W - 1);
            if (hi >= lo) { dir_off16 = (uint32_t)(lo * W * 2 / 16); dir_n16 = (uint32_t)((hi - lo + 1) * W * 2 / 16); }
        }
    }
    // first pass: dead particles whose regions cannot be reused as they are go back to the allocator (so that the clones can have them)
    // -- a dead particle is matched with the clone of the same rank; capacities are mostly equal (particles of one filter map the
    // same world), so the common case is a plain overwrite
    struct Slot { bool keep_dm, keep_occ; HostPart rec; int32_t odm, oocc; };
    std::vector<Slot> slots(dead.size());
    for (size_t k = 0; k < dead.size(); ++k) {
        const uint32_t d = dead[k], i = clones[k], j = (uint32_t)idx[i];
        const HostPart& dr = c->h_part[d];
        const HostPart& sr = c->h_part[j];
        Slot sl{dr.dm_cap == sr.dm_cap, dr.occ_cap == sr.occ_cap, dr, c->h_counts[2 * d], c->h_counts[2 * d + 1]};
        void* dp[5];
        region_ptrs(c, dr, dp);
        ZeroJob z{};
        if (!sl.keep_dm) { z.ndm = sl.odm; z.d[0] = dp[0]; z.d[1] = dp[1]; z.d[2] = dp[2]; region_release(c, true, dr.dm_chunk, dr.dm_off, dr.dm_cap); }
        if (!sl.keep_occ) { z.nocc = sl.oocc; z.d[3] = dp[3]; z.d[4] = dp[4]; region_release(c, false, dr.occ_chunk, dr.occ_off, dr.occ_cap); }
        if (z.ndm || z.nocc) { c->h_zjobs.resize(c->h_zjobs.size() + 1); c->h_zjobs[c->h_zjobs.size() - 1] = z; }
        slots[k] = sl;
    }
    for (size_t k = 0; k < dead.size(); ++k) {
        const uint32_t i = clones[k], j = (uint32_t)idx[i];
        const HostPart sr = c->h_part[j];
        Slot& sl = slots[k];
        HostPart r = sl.rec;                                        // the dead particle's home; its regions where they are kept
        r.dm_cap = sr.dm_cap; r.occ_cap = sr.occ_cap;
        CloneJob job{};
        job.src_home = sr.home; job.dst_home = r.home;
        job.sdm = c->h_counts[2 * j]; job.socc = c->h_counts[2 * j + 1];
        // (a region of the capacity a dead particle of another size has just given back: this can only fail when the device is out of
        // memory for another chunk.  The particle table is then half permuted: the context refuses further work.)
        if (sl.keep_dm) job.odm = sl.odm;
        else { const int32_t rc = region_alloc(c, true, sr.dm_cap, r.dm_chunk, r.dm_off); if (rc) { c->poisoned = true; return rc; } job.odm = 0; }
        if (sl.keep_occ) job.oocc = sl.oocc;
        else { const int32_t rc = region_alloc(c, false, sr.occ_cap, r.occ_chunk, r.occ_off); if (rc) { c->poisoned = true; return rc; } job.oocc = 0; }
        void* sp[5]; void* dp[5];
        region_ptrs(c, sr, sp); region_ptrs(c, r, dp);
        for (int q = 0; q < 5; ++q) { job.s[q] = sp[q]; job.d[q] = dp[q]; }
        job.dir_off16 = dir_off16; job.dir_n16 = dir_n16;
        np[i] = r;
        c->h_jobs.resize(c->h_jobs.size() + 1); c->h_jobs[c->h_jobs.size() - 1] = job;
        c->clone_bytes += 2 * (uint64_t)dir_n16 * 16 + (uint64_t)job.sdm * (SV_PATCH_BYTES + 4096 + 128) + (uint64_t)job.socc * (4096 + 128);
    }
    c->h_part = np;
    std::memcpy(c->h_poses.data(), npose.data(), npose.size() * sizeof(double));
    std::memcpy(c->h_counts.data(), nc.data(), nc.size() * sizeof(int32_t));
    int32_t rc = upload_part(c);                                    // (the jobs carry absolute bases; the table is for everybody after them)
    if (rc) return rc;
    {
        Timer t(c, &c->ctr.ms_resample, &c->ctr.launches_resample);
        rc = run_jobs(c, true);
        t.stop();
    }
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->ms.counts, c->h_counts.data(), sizeof(int32_t) * 2 * P, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_poses, c->h_poses.data(), sizeof(double) * 4 * P, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_timers(c);
    c->ctr.resample_clones += clones.size();
    c->ctr.resample_bytes += c->clone_bytes;
    return LAMA_HIP_OK;
}

// ------------------------------------------------------------------------------------------------
// Grouped step schedule (lama_hip_pf_match_and_map).  A particle's map update is a function of its own pose, its own maps and the
// scan, and its scan match reads its own distance map only: nothing but the host's resample decision couples the particles of a step.
// So every group runs scan match -> (host: window, transforms) -> ray-cast -> brushfire on its own stream, nobody waits for a map
// update, and the status of a group's update travels with the results of its NEXT scan match (k_pack_group: one copy per group).
// All ordering is stream order, events and host decisions; no kernel waits for anything.
// ------------------------------------------------------------------------------------------------
int32_t apply_resample(lama_hip_ctx* c, const int32_t* idx)
{
    c->early_ok = false;                                            // particle indices change meaning
    if (c->ll_valid) { std::vector<double> nl(c->P); for (uint32_t i = 0; i < c->P; ++i) nl[i] = c->h_ll[idx[i]]; c->h_ll.swap(nl); }
    return permute_particles(c, idx);
}

bool step_can_group(const lama_hip_ctx* c, uint32_t n)
{
    // (the plain parallel update only: everything else -- beam-sequential ray-cast, the wrap-guard probe, LidarOdometry's ray rule, the
    // opt-in parallel brushfire, routing -- runs as it always did, on the main stream, after the groups have drained)
    return c->step_groups > 1 && c->P < c->route_min_count && c->cfg.brushfire_mode == 0 && c->cfg.sequential_raycast != 1 &&
           c->cfg.occupancy_policy != 1 && c->cfg.ray_rule == 0 && n <= 4096u && (uint64_t)n + 4096u <= c->cfg.active_capacity &&
           (uint64_t)c->visit_bound + n < 65536u;
}

// k_scan_match with the distance look-up that max_sqdist asks for; start poses as a launch argument (ptab, at most ARG_BLOCK) or from d_poses
void launch_scan_match(lama_hip_ctx* c, const DevParams& prm, hipStream_t s, const double* d_pts, uint32_t n, const Affine& mtf, uint32_t first, uint32_t count, const lama_dev::PoseTable* ptab)
{
    const bool big = c->max_sqdist > (uint32_t)SM_LUT; const lama_dev::NoTable none;
    if (ptab && big) hipLaunchKernelGGL((k_scan_match<true, lama_dev::PoseTable>), dim3(count), dim3(SM_BLOCK), 0, s, prm, d_pts, (int)n, mtf, c->d_loglik, c->d_iters, (int)first, *ptab);
    else if (ptab) hipLaunchKernelGGL((k_scan_match<false, lama_dev::PoseTable>), dim3(count), dim3(SM_BLOCK), 0, s, prm, d_pts, (int)n, mtf, c->d_loglik, c->d_iters, (int)first, *ptab);
    else if (big) hipLaunchKernelGGL((k_scan_match<true, lama_dev::NoTable>), dim3(count), dim3(SM_BLOCK), 0, s, prm, d_pts, (int)n, mtf, c->d_loglik, c->d_iters, (int)first, none);
    else hipLaunchKernelGGL((k_scan_match<false, lama_dev::NoTable>), dim3(count), dim3(SM_BLOCK), 0, s, prm, d_pts, (int)n, mtf, c->d_loglik, c->d_iters, (int)first, none);
}

// scan match of the group's block from the poses in c->h_poses, then its block (results + status of its previous map update) on the
// way to g.h_pack; g.ev_match says when it has arrived.  status_only: no scan match (drain_groups)
int32_t queue_group_match(lama_hip_ctx* c, StepGroup& g, uint32_t n, const Affine& mtf, bool status_only)
{
    const DevParams prm = group_params(c, g);
    // (launch arguments are plain values: the owners are not copied)
    hipStream_t s = g.s;
    uint32_t* const d_words = g.d_words; uint8_t* const d_pack = g.d_pack;
    const int first = (int)g.first, count = (int)g.count;
    // The step path: the predicted poses of a block of at most ARG_BLOCK particles are launch arguments -- no upload of the poses --, and
    // k_pack_group clears what it has packed -- a group's update needs no fills in front of its ray-cast.
    if (!status_only) {
        const bool by_value = g.count <= (uint32_t)lama_dev::ARG_BLOCK;
        lama_dev::PoseTable ptab = lama_dev::PoseTable();
        if (by_value) std::memcpy(ptab.v, &c->h_poses[4 * (size_t)g.first], sizeof(double) * 4 * g.count);
        else HIPCHK(c, hipMemcpyAsync(c->d_poses + 4 * (size_t)g.first, &c->h_poses[4 * (size_t)g.first], sizeof(double) * 4 * g.count, hipMemcpyHostToDevice, s));
        Timer t(c, &g, 0);
        launch_scan_match(c, prm, s, g.d_pts, n, mtf, g.first, g.count, by_value ? &ptab : nullptr);
        t.stop();
    }
    hipLaunchKernelGGL(k_pack_group, dim3(1), dim3(64), 0, s, prm, (const double*)c->d_loglik, (const int32_t*)c->d_iters, d_words, first, count, d_pack, status_only ? 0 : 1);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(g.h_pack.data(), d_pack, GroupPack(g.count).bytes, hipMemcpyDeviceToHost, g.s));
    HIPCHK(c, hipEventRecord(g.ev_match, g.s));
    return LAMA_HIP_OK;
}

// A cleanly aborted map update of one group (its allocation phase ran out of patches before any cell was modified): today's code on
// the main stream, on an idle device, for the group's block -- grow, then the same update again from the poses and the scan it had.
int32_t recover_group(lama_hip_ctx* c, StepGroup& g, int32_t e)
{
    int32_t rc = wait_for_groups(c);
    if (rc) return rc;
    const size_t o = 4 * (size_t)g.first, m = 4 * (size_t)g.count;
    const std::vector<double> now(c->h_poses.data() + o, c->h_poses.data() + o + m);
    std::memcpy(c->h_poses.data() + o, g.upd_poses.data(), sizeof(double) * m);
    const PinVec<double>& scan = g.upd_slot ? c->h_pts2 : c->h_pts;
    HIPCHK(c, c->d_pts.grow((size_t)3 * g.upd_n, (size_t)3 * 2048));
    HIPCHK(c, hipMemcpyAsync(c->d_pts, scan.data(), sizeof(double) * 3 * g.upd_n, hipMemcpyHostToDevice, c->stream));
    const double reach_now = c->scan_reach;
    c->scan_reach = g.upd_reach; c->last_n = g.upd_n;
    c->last_mtf = g.upd_mtf; c->last_first = g.first; c->last_count = g.count; c->last_guarded = true;
    // what the repeat does on the host a second time (the scan's visits, launch counts and brackets, the longest chain) is taken back
    const uint32_t vb = c->visit_bound;
    const lama_hip_counters before = c->ctr;
    c->saved_visit_bound = vb; c->saved_ctr = c->ctr;               // (recover_update rolls back to these: nothing to roll back here)
    rc = recover_update(c, e);
    c->visit_bound = vb;
    c->ctr.parallel_raycast_scans = before.parallel_raycast_scans; c->ctr.sequential_raycast_scans = before.sequential_raycast_scans;
    c->ctr.ms_raycast = before.ms_raycast; c->ctr.launches_raycast = before.launches_raycast;
    c->ctr.ms_brushfire = before.ms_brushfire; c->ctr.launches_brushfire = before.launches_brushfire;
    c->ctr.bf_longest_chain_sum = before.bf_longest_chain_sum; c->ctr.bf_longest_chain_last = before.bf_longest_chain_last;
    if (rc == LAMA_HIP_OK) { for (uint32_t p = g.first; p < g.first + g.count; ++p) c->h_chain[p] = c->h_stats[4 * (size_t)p + 3]; c->chain_dirty = true; }
    c->scan_reach = reach_now; c->last_n = 0;                       // (the main stream's scan buffer holds no scan a later call may reuse)
    std::memcpy(c->h_poses.data() + o, now.data(), sizeof(double) * m);
    return rc;
}

// The block of group g has arrived: the status of its previous map update, if one was queued (returned; no longer queued then), goes
// into the host mirrors and the counters.  The group's error word through `e`.
bool collect_group_status(lama_hip_ctx* c, StepGroup& g, int32_t& e)
{
    const GroupPack L(g.count); const uint8_t* const b = g.h_pack.data();
    const StatusView v{b + L.words, b + L.words + 2 * sizeof(uint32_t), b + L.stats, b + L.guard, b + L.counts, g.first, g.count};
    e = v.error();
    take_group_timers(c, g);
    if (!g.maps_queued) return false;
    apply_update_status(c, v, g.first, g.count, c->h_chain.data());     // (the step's longest chain is pool-wide: flush_step_figures)
    if (e == 0) c->chain_dirty = true;
    g.maps_queued = false;
    return true;
}

// a non-zero error word of group g (of its previous map update when one was queued, else of its scan match): what
// check_device_errors does, for the group
int32_t handle_group_error(lama_hip_ctx* c, StepGroup& g, int32_t e, bool of_maps)
{
    HIPCHK(c, hipMemsetAsync(g.d_words, 0, sizeof(int32_t), g.s));
    if (of_maps && (e & ERR_CLEAN_ABORT) && (e & (ERR_DM_CAP | ERR_OCC_CAP)) && !(e & ERR_WINDOW)) {
        const int32_t rr = recover_group(c, g, e);
        if (rr != LAMA_HIP_E_CAPACITY) return rr;                   // done (or another error); E_CAPACITY: the arenas are at their limit
    }
    int32_t rc = wait_for_groups(c);
    if (rc) return rc;
    if (e & (ERR_DM_CAP | ERR_OCC_CAP)) { rc = clamp_counts(c, true); if (rc) return rc; }
    return device_error_result(c, e);
}

// Collects the status of every group's queued map update (one more block per group, one wait per stream) and leaves the device idle:
// called, through ENTER, at the start of every entry point but lama_hip_pf_match_and_map -- a deferred error surfaces there.
int32_t drain_groups(lama_hip_ctx* c)
{
    if (!c->groups_busy) return LAMA_HIP_OK;
    int32_t rc = LAMA_HIP_OK;
    for (uint32_t k = 0; k < c->step_groups && rc == LAMA_HIP_OK; ++k)
        if (c->grp[k].count && c->grp[k].maps_queued) rc = queue_group_match(c, c->grp[k], 0, Affine(), true);
    const int32_t rw = wait_for_groups(c);
    if (rc == LAMA_HIP_OK) rc = rw;
    c->groups_busy = false;
    if (rc) { for (StepGroup& g : c->grp) g.maps_queued = false; return rc; }
    std::string first_msg;
    for (uint32_t k = 0; k < c->step_groups; ++k) {
        StepGroup& g = c->grp[k];
        if (!g.count || !g.maps_queued) continue;
        int32_t e = 0;
        (void)collect_group_status(c, g, e);
        if (e == 0) continue;
        const int32_t re = handle_group_error(c, g, e, true);
        if (re && rc == LAMA_HIP_OK) { rc = re; first_msg = c->error; }
    }
    for (uint32_t k = 0; k < c->step_groups; ++k) if (c->grp[k].count) (void)hipStreamSynchronize(c->grp[k].s);     // (error words cleared)
    flush_step_figures(c);
    refresh_patch_totals(c);
    if (rc) { c->error = "deferred from the previous map update: " + first_msg; return rc; }
    return grow_arenas(c, 0, c->P);
}

// one group of a grouped step, its block has arrived: status, results, window, map update
int32_t finish_group_step(lama_hip_ctx* c, StepGroup& g, uint32_t n, const Affine& mtf, double* poses_out, double* loglik_out, int32_t* iters_out)
{
    const size_t o = 4 * (size_t)g.first, m = 4 * (size_t)g.count;
    int32_t e = 0;
    const bool had_maps = collect_group_status(c, g, e);
    if (e != 0) {
        int32_t rc = handle_group_error(c, g, e, had_maps);
        if (rc) { if (had_maps) c->error = "deferred from the previous map update: " + c->error; return rc; }
        // the update has been repeated: this step's scan match ran on the map as it was before -- once more, on the updated one
        // (h_poses still holds the block's predicted poses)
        rc = queue_group_match(c, g, n, mtf, false);
        if (rc) return rc;
        HIPCHK(c, hipStreamSynchronize(g.s));
        (void)collect_group_status(c, g, e);
        if (e != 0) { HIPCHK(c, hipMemsetAsync(g.d_words, 0, sizeof(int32_t), g.s)); return device_error_result(c, e); }
    } else if (had_maps) {
        const int32_t rc = grow_arenas(c, g.first, g.count);         // head room for the next update (waits for the groups only when a region moves)
        if (rc) return rc;
    }
    const GroupPack L(g.count);
    const uint8_t* b = g.h_pack.data();
    std::memcpy(c->h_poses.data() + o, b + L.poses, sizeof(double) * m);
    std::memcpy(&c->h_ll[g.first], b + L.loglik, sizeof(double) * g.count);
    if (poses_out) std::memcpy(poses_out + o, b + L.poses, sizeof(double) * m);
    if (loglik_out) std::memcpy(loglik_out + g.first, b + L.loglik, sizeof(double) * g.count);
    if (iters_out) std::memcpy(iters_out + g.first, b + L.iters, sizeof(int32_t) * g.count);
    if (c->cfg.profile) {
        const uint64_t* st = reinterpret_cast<const uint64_t*>(b + L.stats);
        for (uint32_t i = 0; i < g.count; ++i) { c->ctr.gn_iterations += st[4 * i]; c->ctr.gn_evals += st[4 * i + 1]; }
    }
    int32_t rc = fit_window(c, mtf, g.first, g.count);              // (a move or a re-tiling waits for the groups first)
    if (rc) return rc;
    g.upd_poses.assign(c->h_poses.data() + o, c->h_poses.data() + o + m);
    g.upd_mtf = mtf; g.upd_slot = c->scan_slot; g.upd_n = n; g.upd_reach = c->scan_reach;
    UpdatePlan u = plan_update(c, n, g.first, g.count, false, &g);
    rc = stage_scan_tfs(c, mtf, g.first, g.count, g.s, u.tf_by_value ? &u.tab : nullptr);
    if (rc) return rc;
    Timer t = Timer::of_update(c, &g, 1);
    rc = launch_update(c, u, t);
    g.maps_queued = rc == LAMA_HIP_OK;
    return rc;
}

} // namespace

extern "C" {

void lama_hip_default_cfg(lama_hip_cfg* cfg)
{
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->particles = 30;
    cfg->resolution = 0.05;
    cfg->patch_size = 32;
    cfg->l2_max = 0.5;
    cfg->meas_sigma = 0.05;
    cfg->max_iter = 100;
    cfg->device = 0;
    cfg->window_patches = 128;
    cfg->dm_patch_capacity = 128;
    cfg->occ_patch_capacity = 128;
    cfg->queue_capacity = 32768;
    cfg->active_capacity = 8192;
}

int32_t lama_hip_device_count(int32_t* count)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (count) *count = (e == hipSuccess) ? n : 0;
    return e == hipSuccess ? LAMA_HIP_OK : LAMA_HIP_E_HIP;
}

const char* lama_hip_last_error(const lama_hip_ctx* ctx) { return ctx ? ctx->error.c_str() : "null context"; }

int32_t lama_hip_ctx_create(const lama_hip_cfg* cfg_in, lama_hip_ctx** out)
{
    if (!cfg_in || !out) return LAMA_HIP_E_INVALID;
    *out = nullptr;
    lama_hip_cfg cfg = *cfg_in;
    if (cfg.window_patches == 0) cfg.window_patches = 128;
    if (cfg.dm_patch_capacity == 0) cfg.dm_patch_capacity = 128;
    if (cfg.occ_patch_capacity == 0) cfg.occ_patch_capacity = 128;
    if (cfg.queue_capacity == 0) cfg.queue_capacity = 32768;
    if (cfg.active_capacity == 0) cfg.active_capacity = 8192;
    if (cfg.active_capacity > 8192) cfg.active_capacity = 8192;      // largest k_ray_replay stage
    // No environment variable changes what a context computes or which kernels it runs: the variants are chosen through the
    // configuration only (cfg.brushfire_mode = 1, the one variant that is NOT bit-identical to the reference, must be asked for
    // by the caller), and lama_hip_get_counters reports what actually ran.
    if (cfg.brushfire_mode > 1 || cfg.brushfire_waves > 2) return LAMA_HIP_E_INVALID;
    if (cfg.particles == 0 || cfg.patch_size != 32 || !(cfg.resolution > 0) || cfg.window_patches > (uint32_t)LAMA_HIP_MAX_WINDOW ||
        (cfg.window_patches & 7) || cfg.dm_patch_capacity > 32767 || cfg.occ_patch_capacity > 32767 ||
        cfg.queue_capacity < (uint32_t)LQ_BIG)
        return LAMA_HIP_E_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg.device < 0 || cfg.device >= ndev) return LAMA_HIP_E_HIP;

    std::unique_ptr<lama_hip_ctx, Delete> owner(new lama_hip_ctx());       // (released into *out on success only)
    lama_hip_ctx* c = owner.get();
    c->cfg = cfg;
    std::memset(&c->ctr, 0, sizeof(c->ctr));
    c->P = cfg.particles; c->W = cfg.window_patches; c->WC = c->W * 32;
    c->ctr.window_patches = c->W;
    // developer switches, read ONCE here (never on the path of an update): LAMA_HIP_DEBUG_TAIL / LAMA_HIP_DEBUG_WINDOW print what the
    // longest chain / the window did; LAMA_HIP_BF_ROUTE overrides the routing thresholds (tests, experiments)
    c->debug_tail = std::getenv("LAMA_HIP_DEBUG_TAIL") != nullptr;
    c->debug_window = std::getenv("LAMA_HIP_DEBUG_WINDOW") != nullptr;
    {   // A long chain that shares its CU with six first-stage workgroups runs at 0.79 us per pop, alone at 0.75 (and 0.65 on an idle
        // chip): the routed / early big-queue workgroups of a full chip ask for the REST of the CU's LDS as dynamic shared memory, so
        // nothing else is placed beside them (workgroups of that launch without a list entry exit at once and free their CU).
        // 3000 particles: brushfire 4.31 -> 4.10 ms, step 6.36 -> 6.17 ms (round 6); 120 KB instead of the whole CU: no gain.  Only the
        // EARLY lane's launch is padded -- the chains predicted to be the longest; padding the routed launch as well (up to 64 places
        // when many particles re-draw their walls, e.g. after every resample) takes more LDS than the first stage can spare and
        // measured 0.5 - 1 % slower.
        constexpr uint32_t CU_LDS = 160u * 1024u, GRAN = 1280u;
        const uint32_t used = (uint32_t)((sizeof(lama_dev::BfLds<LQ_BIG, RQ_BIG>) + GRAN - 1) / GRAN * GRAN);
        c->big_stage_pad = CU_LDS > used + 2u * GRAN ? CU_LDS - used - 2u * GRAN : 0u;
    }
    if (const char* rr = std::getenv("LAMA_HIP_BF_ROUTE")) {      // "min particles,min events,percent of the mean,places" (tests, experiments; places 0: off)
        unsigned a = 0, b = 0, pc = 0, d = 0, e = 1;
        if (std::sscanf(rr, "%u,%u,%u,%u,%u", &a, &b, &pc, &d, &e) >= 4) { c->route_min_count = a; c->route_min_events = b; c->route_percent = pc; c->route_cap = std::min(d, 256u); c->early_on = e; c->early_min_count = 0; c->route_forced = true; }
    }
    c->scale = 1.0 / cfg.resolution;
    c->off = double(2642244ull >> 1) * 32.0;                      // src/sdm/map.cpp:55-58
    // DynamicDistanceMap::setMaxDistance (src/sdm/dynamic_distance_map.cpp:149-153)
    uint32_t md = (uint32_t)std::ceil(cfg.l2_max * c->scale);
    c->max_sqdist = md * md;
    // this build's queue entries carry obstacle offsets up to MAX_OFFSET_CELLS and its distance plane that range squared: 127 cells
    // in liblama_hip.so, 255 -- all that the reference's uint16_t sqdist can hold -- in liblama_hip_wide.so (lama_dev.h)
    if (c->max_sqdist == 0 || md > MAX_OFFSET_CELLS) return LAMA_HIP_E_INVALID;

    // (hipSuccess is 0: each condition below stops at its first failing call)
    if (hipSetDevice(cfg.device)) return LAMA_HIP_E_HIP;
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, cfg.device) == hipSuccess && prop.multiProcessorCount > 0) c->num_cus = (uint32_t)prop.multiProcessorCount; }
    if (hipStreamCreate(&c->stream.h) || hipEventCreate(&c->ev0.h) || hipEventCreate(&c->ev1.h)) return LAMA_HIP_E_HIP;
    const size_t P = c->P, WW = (size_t)c->W * c->W, dc = cfg.dm_patch_capacity, oc = cfg.occ_patch_capacity;
    {
        // one particle set: directories per home, pooled planes with one region per particle and map kind (lama_dev.h).  The pools
        // start at P x the configured capacities and grow with the maps.
        MapStore& m = c->ms;
        c->floor_dm = (uint32_t)dc; c->floor_occ = (uint32_t)oc;
        if (P * dc > 0xFFFFFFF0ull || P * oc > 0xFFFFFFF0ull) return LAMA_HIP_E_INVALID;
        if (m.dm_dir.alloc(P * WW) || hipMemset(m.dm_dir, 0xFF, P * WW * 2)) return LAMA_HIP_E_HIP;
        if (m.occ_dir.alloc(P * WW) || hipMemset(m.occ_dir, 0xFF, P * WW * 2)) return LAMA_HIP_E_HIP;
        // (m.counts lives in the results / status block below: one copy brings a map update's counters back)
        // first chunk of each pool: P regions of the configured capacity
        if (add_chunk(c, true, (uint32_t)(P * dc)) != LAMA_HIP_OK || add_chunk(c, false, (uint32_t)(P * oc)) != LAMA_HIP_OK) return LAMA_HIP_E_HIP;
        c->ctr.pool_growths = 0;
        c->h_part.resize(P);
        for (size_t p = 0; p < P; ++p) {
            HostPart r{};
            r.home = (uint32_t)p; r.dm_cap = (uint32_t)dc; r.occ_cap = (uint32_t)oc;
            if (region_alloc(c, true, (uint32_t)dc, r.dm_chunk, r.dm_off) != LAMA_HIP_OK || region_alloc(c, false, (uint32_t)oc, r.occ_chunk, r.occ_off) != LAMA_HIP_OK) return LAMA_HIP_E_HIP;
            c->h_part[p] = r;
        }
        if (c->d_part.alloc(P)) return LAMA_HIP_E_HIP;
        if (upload_part(c) != LAMA_HIP_OK) return LAMA_HIP_E_HIP;
        if (hipStreamSynchronize(c->stream)) return LAMA_HIP_E_HIP;
    }
    // ONE allocation: [poses | loglik | iters | err]   what a scan match brings back (results_bytes, one copy) ...
    //                 [err | slow_n | stats | guard | counts]   ... and what a map update brings back (status_bytes from status_off, one
    // copy: round 6 -- the five copies it used to take were 23 us at the end of every 1.8 ms update); slow_n and stats are adjacent:
    // one memset clears both when an update starts.
    c->results_bytes = P * 4 * 8 + P * 8 + P * 4 + 8;
    c->status_off = P * 4 * 8 + P * 8 + P * 4;                                  // the error word: last of the results, first of the status
    const size_t slow_off = (c->results_bytes + 7) / 8 * 8;
    c->status_bytes = (slow_off - c->status_off) + 32 + P * 4 * 8 + P * 2 * 4 + P * 2 * 4;
    if (c->d_results.alloc(c->status_off + c->status_bytes) || hipMemset(c->d_results, 0, c->status_off + c->status_bytes)) return LAMA_HIP_E_HIP;
    c->d_poses = reinterpret_cast<double*>(c->d_results.p);
    c->d_loglik = c->d_poses + P * 4;
    c->d_iters = reinterpret_cast<int32_t*>(c->d_loglik + P);
    c->d_err = c->d_iters + P;
    c->d_slow_n = reinterpret_cast<uint32_t*>(c->d_results + slow_off);
    c->d_stats = reinterpret_cast<uint64_t*>(c->d_results + slow_off + 32);
    c->d_guard = reinterpret_cast<uint32_t*>(c->d_stats + P * 4);
    c->ms.counts = reinterpret_cast<int32_t*>(c->d_guard + P * 2);
    if (c->d_qlower.alloc(P * (size_t)cfg.queue_capacity) || c->d_qraise.alloc(P * (size_t)cfg.queue_capacity)) return LAMA_HIP_E_HIP;
    if (c->d_qsizes.alloc(P * 2) || hipMemset(c->d_qsizes, 0, P * 2 * 4)) return LAMA_HIP_E_HIP;
    if (c->d_dbg.alloc(P * 16 + (1u << 20) / 8) || hipMemset(c->d_dbg, 0, P * 16 * 8 + (1u << 20))) return LAMA_HIP_E_HIP;   // + 1 MiB developer event log
    if (c->d_slow.alloc(P) || hipMemset(c->d_slow, 0, P * 4)) return LAMA_HIP_E_HIP;
    if (c->d_slow_list.alloc(4 * P) || hipMemset(c->d_slow_list, 0, 4 * P * 4)) return LAMA_HIP_E_HIP;
    if (c->d_heavy.alloc(P) || hipMemset(c->d_heavy, 0, P)) return LAMA_HIP_E_HIP;
    if (c->d_early.alloc(P) || hipMemset(c->d_early, 0, P)) return LAMA_HIP_E_HIP;
    if (c->d_elist.alloc(256) || hipMemset(c->d_elist, 0, 256 * 4)) return LAMA_HIP_E_HIP;
    if (c->d_hlist.alloc(256) || hipMemset(c->d_hlist, 0, 256 * 4)) return LAMA_HIP_E_HIP;
    if (hipStreamCreate(&c->stream2.h) || hipStreamCreate(&c->stream3.h)) return LAMA_HIP_E_HIP;
    {
        // Grouped step schedule (lama_hip_pf_match_and_map): a pool too small for routing and the early lane -- whose streams are
        // therefore idle -- is split into contiguous blocks, each with a stream of its own, so that a block whose brushfire chains are
        // short this step goes on with the next scan match while another block's longest chain still runs.
        // THE RULE of these streams: nothing that one group's stream wrote, by kernel or by copy, is read on another group's stream.
        // What all groups read and the host rewrites per step (the scan) is uploaded once per group, into the group's own buffer, on
        // the group's stream; per-update scalars and lists (error word, hand-over counts and lists) exist once per group; arrays
        // indexed by particle are touched by the owning group only.  Everything else (window, particle table, regions, resample,
        // export / import, downloads) runs on the main stream after wait_for_groups / drain_groups, i.e. on an idle device.
        uint32_t G = c->P < c->route_min_count ? DEFAULT_STEP_GROUPS : 1u;
        if (const char* sg = std::getenv("LAMA_HIP_STEP_GROUPS")) {      // tests, measurements: 1 = the single-stream schedule
            unsigned v = 0;
            if (std::sscanf(sg, "%u", &v) == 1 && v >= 1) G = std::min<uint32_t>(v, MAX_STEP_GROUPS);
        }
        if (c->P >= c->route_min_count) G = 1;
        c->step_groups = G;
        if (G > 1) {
            if (G > 3 && hipStreamCreate(&c->stream4.h)) return LAMA_HIP_E_HIP;      // (only an override asks for a fourth group)
            const hipStream_t ss[MAX_STEP_GROUPS] = {c->stream, c->stream2, c->stream3, c->stream4};
            // contiguous blocks of ceil(P / G) particles -- of the next multiple of 8 where that still makes G blocks (30 particles in
            // 4 groups: 8, 8, 8, 6), so that a block's two-dimensional launches keep a particle on the XCD its one-dimensional ones
            // put it on (xcd_grid)
            uint32_t per = (uint32_t)((P + G - 1) / G);
            const uint32_t per8 = (per + 7u) / 8u * 8u;
            if ((P + per8 - 1) / per8 == G) per = per8;
            for (uint32_t k = 0; k < G; ++k) {
                StepGroup& g = c->grp[k];
                g.s = ss[k];
                g.first = (uint32_t)std::min<size_t>(P, (size_t)k * per); g.count = (uint32_t)std::min<size_t>(P, (size_t)(k + 1) * per) - g.first;
                if (g.count == 0) continue;
                const GroupPack L(g.count);
                if (g.d_words.alloc(16) || hipMemset(g.d_words, 0, 64) || g.d_slow_list.alloc(4 * P) || hipMemset(g.d_slow_list, 0, 4 * P * 4) ||
                    g.d_pack.alloc(L.bytes) || hipEventCreateWithFlags(&g.ev_match.h, hipEventDisableTiming))
                    return LAMA_HIP_E_HIP;
                g.h_pack.resize(L.bytes);
                if (cfg.profile) for (Event& e : g.tev) if (hipEventCreate(&e.h)) return LAMA_HIP_E_HIP;
            }
            c->h_chain.assign(P, 0);
        }
    }
    if (hipEventCreateWithFlags(&c->ev_alloc.h, hipEventDisableTiming) || hipEventCreateWithFlags(&c->ev_early.h, hipEventDisableTiming) ||
        hipEventCreateWithFlags(&c->ev_go.h, hipEventDisableTiming) ||
        hipEventCreateWithFlags(&c->ev_route.h, hipEventDisableTiming) || hipEventCreateWithFlags(&c->ev_heavy.h, hipEventDisableTiming))
        return LAMA_HIP_E_HIP;
    if (c->d_scalar.alloc(4) || hipMemset(c->d_scalar, 0, 16)) return LAMA_HIP_E_HIP;
    if (c->d_act.alloc(P * (size_t)cfg.active_capacity)) return LAMA_HIP_E_HIP;
    if (c->d_act_count.alloc(P) || hipMemset(c->d_act_count, 0, P * 4)) return LAMA_HIP_E_HIP;
    if (c->d_tfs.alloc(P * 12) || c->d_oldcounts.alloc(P * 2)) return LAMA_HIP_E_HIP;
    if (hipDeviceSynchronize()) return LAMA_HIP_E_HIP;
    c->h_poses.assign(P * 4, 0.0);
    c->h_counts.assign(P * 2, 0);
    *out = owner.release();
    return LAMA_HIP_OK;
}

void lama_hip_ctx_destroy(lama_hip_ctx* c) { delete c; }

int32_t lama_hip_pf_set_poses(lama_hip_ctx* c, const double* poses)
{
    if (!c || !poses) return LAMA_HIP_E_INVALID;
    ENTER(c);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    std::memcpy(c->h_poses.data(), poses, sizeof(double) * 4 * c->P);
    // asynchronous: the source is the context's own host mirror, which stays valid; later calls are stream ordered
    HIPCHK(c, hipMemcpyAsync(c->d_poses, c->h_poses.data(), sizeof(double) * 4 * c->P, hipMemcpyHostToDevice, c->stream));
    return LAMA_HIP_OK;
}

int32_t lama_hip_pf_get_poses(lama_hip_ctx* c, double* poses)
{
    if (!c || !poses) return LAMA_HIP_E_INVALID;
    ENTER(c);
    std::memcpy(poses, c->h_poses.data(), sizeof(double) * 4 * c->P);
    return LAMA_HIP_OK;
}

int32_t lama_hip_pf_init(lama_hip_ctx* c, const double* pts, uint32_t n, const double* origin3, const double* quat,
                         const double* pose0)
{
    if (!c || !pts || !pose0 || n == 0) return LAMA_HIP_E_INVALID;
    ENTER(c);
    if (c->initialised) return fail(c, LAMA_HIP_E_STATE, "lama_hip_pf_init called twice");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // centre the map window on the first pose (patch aligned)
    const double mx = c->scale * pose0[2] + c->off, my = c->scale * pose0[3] + c->off;
    const uint32_t px = ((uint32_t)mx) >> 5, py = ((uint32_t)my) >> 5;
    c->wx0 = (px - c->W / 2) * 32;
    c->wy0 = (py - c->W / 2) * 32;
    for (uint32_t p = 0; p < c->P; ++p) std::memcpy(&c->h_poses[4 * p], pose0, sizeof(double) * 4);
    HIPCHK(c, hipMemcpyAsync(c->d_poses, c->h_poses.data(), sizeof(double) * 4 * c->P, hipMemcpyHostToDevice, c->stream));
    int32_t rc = upload_scan(c, pts, n);
    if (rc) return rc;
    const Affine mtf = moving_tf(origin3, quat);
    rc = run_update_maps(c, n, mtf, 0, 1);                          // particle 0 only (pf_slam2d.cpp:204)
    if (rc) return rc;
    rc = check_device_errors(c, true, false);                        // (grows the arenas and repeats the update if it ran out of patches)
    if (rc) return rc;
    if (c->P > 1) {                                                 // copy-construct the others (:206-216)
        std::vector<int32_t> idx(c->P, 0);
        rc = permute_particles(c, idx.data());
        if (rc) return rc;
    }
    rc = check_device_errors(c, true, false);
    if (rc) return rc;
    c->initialised = true;
    return LAMA_HIP_OK;
}

int32_t lama_hip_pf_scan_match(lama_hip_ctx* c, const double* pts, uint32_t n, const double* origin3, const double* quat,
                               double* poses_out, double* loglik_out, int32_t* iters_out)
{
    if (!c || !pts || n == 0) return LAMA_HIP_E_INVALID;
    ENTER(c);
    if (!c->initialised) return fail(c, LAMA_HIP_E_STATE, "lama_hip_pf_scan_match before lama_hip_pf_init");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int32_t rc = upload_scan(c, pts, n);
    if (rc) return rc;
    const Affine mtf = moving_tf(origin3, quat);
    DevParams prm = make_params(c);
    {
        Timer t(c, &c->ctr.ms_scan_match, &c->ctr.launches_scan_match);
        launch_scan_match(c, prm, c->stream, c->d_pts, n, mtf, 0, c->P, nullptr);      // (the poses are in d_poses)
        t.stop();
    }
    HIPCHK(c, hipGetLastError());
    // poses, log-likelihoods, iteration counts and the error word: one copy (they share an allocation)
    c->h_results.resize(c->results_bytes);
    HIPCHK(c, hipMemcpyAsync(c->h_results.data(), c->d_results, c->results_bytes, hipMemcpyDeviceToHost, c->stream));
    rc = check_device_errors(c, false, c->cfg.profile != 0, true);   // synchronises
    if (rc) return rc;
    const uint8_t* r = c->h_results.data();
    std::memcpy(c->h_poses.data(), r, sizeof(double) * 4 * c->P);
    if (poses_out) std::memcpy(poses_out, r, sizeof(double) * 4 * c->P);
    if (loglik_out) std::memcpy(loglik_out, r + sizeof(double) * 4 * c->P, sizeof(double) * c->P);
    if (iters_out) std::memcpy(iters_out, r + sizeof(double) * 5 * c->P, sizeof(int32_t) * c->P);
    c->h_ll.resize(c->P); std::memcpy(c->h_ll.data(), r + sizeof(double) * 4 * c->P, sizeof(double) * c->P); c->ll_valid = true;
    return LAMA_HIP_OK;
}

int32_t lama_hip_pf_resample(lama_hip_ctx* c, const int32_t* sample_idx)
{
    if (!c || !sample_idx) return LAMA_HIP_E_INVALID;
    if (c->poisoned) return refuse_poisoned(c);
    if (!c->initialised) return fail(c, LAMA_HIP_E_STATE, "lama_hip_pf_resample before lama_hip_pf_init");
    for (uint32_t i = 0; i < c->P; ++i)
        if (sample_idx[i] < 0 || (uint32_t)sample_idx[i] >= c->P) return fail(c, LAMA_HIP_E_INVALID, "sample_idx out of range");
    // The groups of a grouped step are still updating their maps: the copy waits for all of them, so it is made by the NEXT call on the
    // context, whatever that is (finish_pending) -- until then the host is free, and a filter's prediction of the next step runs
    // beside the map kernels as it does when no resample is due.  An error of the copy is then that call's ("deferred from ...").
    if (c->groups_busy && !c->resample_deferred) {
        c->deferred_idx.assign(sample_idx, sample_idx + c->P);
        c->resample_deferred = true;
        return LAMA_HIP_OK;
    }
    ENTER(c);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return apply_resample(c, sample_idx);
}

int32_t lama_hip_pf_update_maps_begin(lama_hip_ctx* c, const double* pts, uint32_t n, const double* origin3, const double* quat)
{
    if (!c || n == 0) return LAMA_HIP_E_INVALID;
    ENTER(c);
    if (!c->initialised) return fail(c, LAMA_HIP_E_STATE, "lama_hip_pf_update_maps before lama_hip_pf_init");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int32_t rc = upload_scan(c, pts, n);
    if (rc) return rc;
    const Affine mtf = moving_tf(origin3, quat);
    rc = run_update_maps(c, n, mtf, 0, c->P);
    if (rc) return rc;
    c->pending_maps = true;
    return LAMA_HIP_OK;
}

int32_t lama_hip_ctx_device(const lama_hip_ctx* c) { return c ? c->cfg.device : -1; }

int32_t lama_hip_sync(lama_hip_ctx* c)
{
    if (!c) return LAMA_HIP_E_INVALID;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return finish_pending(c);
}

int32_t lama_hip_pf_update_maps(lama_hip_ctx* c, const double* pts, uint32_t n, const double* origin3, const double* quat)
{
    const int32_t rc = lama_hip_pf_update_maps_begin(c, pts, n, origin3, quat);
    if (rc) return rc;
    return lama_hip_sync(c);
}

int32_t lama_hip_pf_match_and_map(lama_hip_ctx* c, const double* pts, uint32_t n, const double* origin3, const double* quat,
                                  const double* poses_in, double* poses_out, double* loglik_out, int32_t* iters_out)
{
    if (!c || !pts || !poses_in || n == 0) return LAMA_HIP_E_INVALID;
    if (c->poisoned) return refuse_poisoned(c);
    if (!c->initialised) return fail(c, LAMA_HIP_E_STATE, "lama_hip_pf_match_and_map before lama_hip_pf_init");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // A step that could not be grouped (below) has left its map update queued on the main stream: its status is collected here, and the
    // schedule is chosen for THIS step alone -- one ungroupable scan (the wrap-guard probe is due every 65536 / n scans) must not
    // keep the context on one stream.
    if (c->pending_maps || c->resample_deferred) { const int32_t rp = finish_pending(c); if (rp) return rp; }
    if (!step_can_group(c, n)) {
        // the single-stream schedule (each of the three calls drains whatever the groups still hold)
        int32_t rc = lama_hip_pf_set_poses(c, poses_in);
        if (rc == LAMA_HIP_OK) rc = lama_hip_pf_scan_match(c, pts, n, origin3, quat, poses_out, loglik_out, iters_out);
        if (rc == LAMA_HIP_OK) rc = lama_hip_pf_update_maps_begin(c, nullptr, n, origin3, quat);
        if (rc == LAMA_HIP_OK) c->groups_ran = 1;
        return rc;
    }
    // the scan: page-locked staging (two buffers by turns: the previous step's scan may be needed once more, recover_group), reach
    c->scan_slot ^= 1u;
    PinVec<double>& hp = c->scan_slot ? c->h_pts2 : c->h_pts;
    hp.resize((size_t)3 * n);
    std::memcpy(hp.data(), pts, sizeof(double) * 3 * n);
    double r2 = 0.0;
    if (!scan_reach2(pts, n, false, r2)) { c->scan_slot ^= 1u; return fail(c, LAMA_HIP_E_INVALID, "the scan holds a non-finite point (filter NaN / inf ranges before the update, as iris_lama_ros does)"); }
    c->scan_reach = std::sqrt(r2);
    c->last_n = 0;                                                  // (the main stream's scan buffer is not this scan)
    const Affine mtf = moving_tf(origin3, quat);
    std::memcpy(c->h_poses.data(), poses_in, sizeof(double) * 4 * c->P);
    c->h_ll.resize(c->P);
    c->groups_busy = true;
    c->early_ok = false;
    uint32_t left = 0;
    for (uint32_t k = 0; k < c->step_groups; ++k) {
        StepGroup& g = c->grp[k];
        if (!g.count) continue;
        HIPCHK(c, g.d_pts.grow((size_t)3 * n, (size_t)3 * 2048));
        HIPCHK(c, hipMemcpyAsync(g.d_pts, hp.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, g.s));
        const int32_t rc = queue_group_match(c, g, n, mtf, false);
        if (rc) return rc;
        left |= 1u << k;
    }
    UpdatePlan step; step.n = n; step.count = c->P;                // (once for the pool; the plan's defaults are what every group's plan says)
    note_update_begin(c, mtf, step, -1);
    // the groups are taken as their blocks arrive, not in a fixed order: the one whose chains were short goes on first
    while (left) {
        for (uint32_t k = 0; k < c->step_groups; ++k) {
            if (!(left & (1u << k))) continue;
            StepGroup& g = c->grp[k];
#ifndef LAMA_WAVE_SIM
            const hipError_t q = hipEventQuery(g.ev_match);
            if (q == hipErrorNotReady) continue;
            if (q != hipSuccess) return hip_fail(c, q, "hipEventQuery");
#endif
            left &= ~(1u << k);
            const int32_t rc = finish_group_step(c, g, n, mtf, poses_out, loglik_out, iters_out);
            if (rc) {
                // The step fails as a whole, once: the groups not taken yet hand in the status of the same update (their scan match
                // results are dropped), so that the next call starts clean -- as it does after the single-stream schedule's one error.
                const std::string msg = c->error;
                (void)wait_for_groups(c);
                for (uint32_t j = 0; j < c->step_groups; ++j) {
                    if (!(left & (1u << j))) continue;
                    StepGroup& o = c->grp[j];
                    int32_t e = 0;
                    const bool had_maps = collect_group_status(c, o, e);
                    if (e != 0) (void)handle_group_error(c, o, e, had_maps);
                }
                flush_step_figures(c);
                c->error = msg;
                return rc;
            }
        }
    }
    c->ll_valid = true;
    flush_step_figures(c);
    refresh_patch_totals(c);
    c->ctr.brushfire_mode = c->cfg.brushfire_mode;
    c->groups_ran = 0;
    for (uint32_t k = 0; k < c->step_groups; ++k) c->groups_ran += c->grp[k].count ? 1u : 0u;      // (more groups than particles: the empty ones did not run)
    return LAMA_HIP_OK;
}

int32_t lama_hip_pf_step_groups(lama_hip_ctx* c, uint32_t* ran, uint32_t* configured)
{
    if (!c || (!ran && !configured)) return LAMA_HIP_E_INVALID;
    if (configured) {                                               // (fixed at creation: no need to wait for anything)
        uint32_t n = 0;
        for (uint32_t k = 0; k < c->step_groups; ++k) n += c->grp[k].count ? 1u : 0u;
        *configured = c->step_groups > 1 ? n : 0u;
    }
    if (!ran) return LAMA_HIP_OK;
    ENTER(c);
    *ran = c->groups_ran;
    return LAMA_HIP_OK;
}

int32_t lama_hip_pf_map_patches(lama_hip_ctx* c, uint32_t particle, int32_t kind, uint32_t* num)
{
    if (!c || !num || particle >= c->P || (kind != LAMA_HIP_MAP_DISTANCE && kind != LAMA_HIP_MAP_OCCUPANCY)) return LAMA_HIP_E_INVALID;
    ENTER(c);
    *num = (uint32_t)c->h_counts[2 * particle + (kind == LAMA_HIP_MAP_OCCUPANCY ? 1 : 0)];
    return LAMA_HIP_OK;
}

int32_t lama_hip_pf_patch_ids(lama_hip_ctx* c, uint32_t particle, int32_t kind, uint32_t cap, uint64_t* patch_ids, uint32_t* num_patches)
{
    if (!c || particle >= c->P || (kind != LAMA_HIP_MAP_DISTANCE && kind != LAMA_HIP_MAP_OCCUPANCY)) return LAMA_HIP_E_INVALID;
    ENTER(c);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const MapStore& s = c->ms;
    const size_t WW = (size_t)c->W * c->W;
    const bool dm = kind == LAMA_HIP_MAP_DISTANCE;
    std::vector<int16_t> dir(WW);
    HIPCHK(c, hipMemcpy(dir.data(), (dm ? s.dm_dir : s.occ_dir) + c->h_part[particle].home * WW, WW * 2, hipMemcpyDeviceToHost));
    std::vector<uint64_t> ids;
    for (uint32_t wy = 0; wy < c->W; ++wy)
        for (uint32_t wx = 0; wx < c->W; ++wx)
            if (dir[wy * c->W + wx] >= 0) ids.push_back(((uint64_t)(c->wx0 >> 5) + wx) * 2642244ull + ((uint64_t)(c->wy0 >> 5) + wy));
    std::sort(ids.begin(), ids.end());
    if (num_patches) *num_patches = (uint32_t)ids.size();
    if (patch_ids) for (size_t k = 0; k < ids.size() && k < cap; ++k) patch_ids[k] = ids[k];
    return LAMA_HIP_OK;
}

int32_t lama_hip_pf_map_checksums(lama_hip_ctx* c, int32_t kind, uint64_t* out)
{
    if (!c || !out || (kind != LAMA_HIP_MAP_DISTANCE && kind != LAMA_HIP_MAP_OCCUPANCY)) return LAMA_HIP_E_INVALID;
    ENTER(c);
    if (c->cfg.occupancy_policy != 0 && kind == LAMA_HIP_MAP_OCCUPANCY) return fail(c, LAMA_HIP_E_INVALID, "map checksums cover the frequency occupancy policy");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    DevBuf<uint64_t> sums;
    HIPCHK(c, sums.alloc(c->P));
    uint64_t* const d_out = sums;                                   // (launch arguments are plain pointers: the owners are not copied)
    DevParams prm = make_params(c);
    hipLaunchKernelGGL(k_map_checksum, dim3(c->P), dim3(256), 0, c->stream, prm, kind == LAMA_HIP_MAP_DISTANCE ? 0 : 1, d_out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, d_out, sizeof(uint64_t) * c->P, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LAMA_HIP_OK;
}

// Map::deletePatchAt on both maps.  The arenas are bump allocated (slot = count++), so a deleted slot is refilled with the
// last used slot and the directory entry of that patch is redirected: the arena stays dense.  Host driven (a handful of
// patches per scan at most): device-to-device copies + memsets on the context's stream.
int32_t lama_hip_pf_delete_patches(lama_hip_ctx* c, uint32_t particle, const uint64_t* patch_ids, uint32_t n, uint32_t* deleted)
{
    if (!c || particle >= c->P || (!patch_ids && n)) return LAMA_HIP_E_INVALID;
    ENTER(c);
    if (deleted) *deleted = 0;
    if (n == 0) return LAMA_HIP_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    MapStore& s = c->ms;
    const size_t WW = (size_t)c->W * c->W;
    const HostPart hp = c->h_part[particle];
    const PartRec pr = dev_part(c, hp);                             // the particle's regions (plane addresses)
    for (int kind = 0; kind < 2; ++kind) {
        const bool dm = kind == 0;
        int16_t* d_dir = (dm ? s.dm_dir : s.occ_dir) + hp.home * WW;
        std::vector<int16_t> dir(WW);
        HIPCHK(c, hipMemcpy(dir.data(), d_dir, WW * 2, hipMemcpyDeviceToHost));
        int count = c->h_counts[2 * particle + (dm ? 0 : 1)];
        bool touched = false;
        for (uint32_t k = 0; k < n; ++k) {
            const uint64_t px = patch_ids[k] / 2642244ull, py = patch_ids[k] % 2642244ull;
            const int64_t wx = (int64_t)px - (int64_t)(c->wx0 >> 5), wy = (int64_t)py - (int64_t)(c->wy0 >> 5);
            if (wx < 0 || wy < 0 || wx >= (int64_t)c->W || wy >= (int64_t)c->W) continue;
            const size_t pidx = (size_t)wy * c->W + (size_t)wx;
            const int slot = dir[pidx];
            if (slot < 0) continue;
            const int last = count - 1;
            auto plane_move = [&](void* plane, size_t bytes_per_slot) -> hipError_t {
                char* b = (char*)plane;
                if (slot != last) {
                    hipError_t e = hipMemcpyAsync(b + (size_t)slot * bytes_per_slot, b + (size_t)last * bytes_per_slot, bytes_per_slot, hipMemcpyDeviceToDevice, c->stream);
                    if (e != hipSuccess) return e;
                }
                return hipMemsetAsync(b + (size_t)last * bytes_per_slot, 0, bytes_per_slot, c->stream);
            };
            if (dm) {
                HIPCHK(c, plane_move(pr.dm_sv, SV_PATCH_BYTES)); HIPCHK(c, plane_move(pr.dm_obs, 4096)); HIPCHK(c, plane_move(pr.dm_mask, 128));
            } else {
                HIPCHK(c, plane_move(pr.occ, 4096)); HIPCHK(c, plane_move(pr.occ_mask, 128));
                HIPCHK(c, plane_move(pr.occ_hit, 128));
            }
            if (slot != last)
                for (size_t q = 0; q < WW; ++q) if (dir[q] == last) { dir[q] = (int16_t)slot; break; }
            dir[pidx] = -1;
            --count;
            touched = true;
            if (dm && deleted) ++*deleted;
            if (dm) c->dm_deleted = true;
        }
        if (touched) {
            HIPCHK(c, hipMemcpyAsync(d_dir, dir.data(), WW * 2, hipMemcpyHostToDevice, c->stream));
            c->h_counts[2 * particle + (dm ? 0 : 1)] = count;
            HIPCHK(c, hipMemcpyAsync(s.counts + 2 * particle + (dm ? 0 : 1), &c->h_counts[2 * particle + (dm ? 0 : 1)], sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));          // `dir` and h_counts are read by the copies above
        }
    }
    return LAMA_HIP_OK;
}

int32_t lama_hip_pf_download_map(lama_hip_ctx* c, uint32_t particle, int32_t kind, uint32_t cap,
                                 uint64_t* patch_ids, uint8_t* cells, uint64_t* masks, uint32_t* num_patches)
{
    if (!c || particle >= c->P || (kind != LAMA_HIP_MAP_DISTANCE && kind != LAMA_HIP_MAP_OCCUPANCY)) return LAMA_HIP_E_INVALID;
    ENTER(c);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const MapStore& s = c->ms;
    const size_t WW = (size_t)c->W * c->W;
    const bool dm = kind == LAMA_HIP_MAP_DISTANCE;
    const HostPart hp = c->h_part[particle];
    const PartRec pr = dev_part(c, hp);
    const uint32_t count = (uint32_t)c->h_counts[2 * particle + (dm ? 0 : 1)];
    if (num_patches) *num_patches = count;
    if (count == 0 || cap == 0) return LAMA_HIP_OK;
    std::vector<int16_t> dir(WW);
    HIPCHK(c, hipMemcpy(dir.data(), (dm ? s.dm_dir : s.occ_dir) + hp.home * WW, WW * 2, hipMemcpyDeviceToHost));
    // (reference patch id, slot), ascending id
    std::vector<std::pair<uint64_t, int>> order;
    for (uint32_t wy = 0; wy < c->W; ++wy)
        for (uint32_t wx = 0; wx < c->W; ++wx) {
            int slot = dir[wy * c->W + wx];
            if (slot < 0) continue;
            const uint64_t px = (c->wx0 >> 5) + wx, py = (c->wy0 >> 5) + wy;
            order.emplace_back(px * 2642244ull + py, slot);                   // Map::m2p
        }
    std::sort(order.begin(), order.end());
    if (order.size() != count) return fail(c, LAMA_HIP_E_STATE, "directory / count mismatch");
    std::vector<uint64_t> hmask((size_t)count * 16);
    HIPCHK(c, hipMemcpy(hmask.data(), dm ? pr.dm_mask : pr.occ_mask,
                        hmask.size() * 8, hipMemcpyDeviceToHost));
    std::vector<sv_t> hsv; std::vector<uint32_t> hobs, hocc;
    if (dm) {
        hsv.resize((size_t)count * 1024); hobs.resize((size_t)count * 1024);
        HIPCHK(c, hipMemcpy(hsv.data(), pr.dm_sv, hsv.size() * SV_BYTES, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(hobs.data(), pr.dm_obs, hobs.size() * 4, hipMemcpyDeviceToHost));
    } else {
        hocc.resize((size_t)count * 1024);
        HIPCHK(c, hipMemcpy(hocc.data(), pr.occ, hocc.size() * 4, hipMemcpyDeviceToHost));
    }
    const uint32_t nout = std::min<uint32_t>(cap, count);
    for (uint32_t k = 0; k < nout; ++k) {
        const int slot = order[k].second;
        if (patch_ids) patch_ids[k] = order[k].first;
        if (masks) std::memcpy(masks + (size_t)k * 16, &hmask[(size_t)slot * 16], 128);
        if (!cells) continue;
        if (dm) {
            uint8_t* o = cells + (size_t)k * 10240;
            for (int ci = 0; ci < 1024; ++ci) {
                const sv_t sv = hsv[(size_t)slot * 1024 + ci];
                const uint32_t ob = hobs[(size_t)slot * 1024 + ci];
                const int16_t ox = (int16_t)(ob & 0xFFFF), oy = (int16_t)(ob >> 16), oz = 0;
                const uint16_t sq = (uint16_t)(sv & SV_SQMASK);
                std::memcpy(o + 10 * ci + 0, &ox, 2); std::memcpy(o + 10 * ci + 2, &oy, 2); std::memcpy(o + 10 * ci + 4, &oz, 2);
                std::memcpy(o + 10 * ci + 6, &sq, 2);
                o[10 * ci + 8] = (sv & SV_VALID) ? 1 : 0;
                o[10 * ci + 9] = (sv & SV_QUEUED) ? 1 : 0;
            }
        } else {
            std::memcpy(cells + (size_t)k * 4096, &hocc[(size_t)slot * 1024], 4096);   // {u16 occupied, u16 visited} little endian
            if (masks && c->cfg.occupancy_policy == 0) {   // Container mask of a frequency cell = "visited != 0" (plus the plane bits set on uint16 wrap)
                uint64_t* mk = masks + (size_t)k * 16;
                for (int ci = 0; ci < 1024; ++ci)
                    if (hocc[(size_t)slot * 1024 + ci] >> 16) mk[ci >> 6] |= 1ull << (ci & 63);
            }
        }
    }
    return LAMA_HIP_OK;
}

int32_t lama_hip_pf_upload_map(lama_hip_ctx* c, uint32_t particle, int32_t kind, uint32_t n, const uint64_t* patch_ids, const uint8_t* cells,
                               const uint64_t* masks)
{
    if (!c || particle >= c->P || (kind != LAMA_HIP_MAP_DISTANCE && kind != LAMA_HIP_MAP_OCCUPANCY) || (n && (!patch_ids || !cells || !masks))) return LAMA_HIP_E_INVALID;
    ENTER(c);
    if (n > MAX_PATCHES) return fail(c, LAMA_HIP_E_CAPACITY, "a particle's map exceeds 32767 patches");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const bool dm = kind == LAMA_HIP_MAP_DISTANCE;
    // Convert and validate everything FIRST: a rejected upload must leave the particle's previous map as it was (the old
    // slots were zeroed and the window / region possibly moved before a squared distance beyond the plane's 14 bits was noticed).
    std::vector<sv_t> hsv; std::vector<uint32_t> hobs;
    if (n && dm) {     // distance_t (10 B: int16 obstacle[3], uint16 sqdist, bool valid_obstacle, bool is_queued) -> the two planes
        hsv.resize((size_t)n * 1024); hobs.resize((size_t)n * 1024);
        for (size_t k = 0; k < n; ++k)
            for (int ci = 0; ci < 1024; ++ci) {
                const uint8_t* o = cells + k * 10240 + 10 * (size_t)ci;
                int16_t ox, oy; uint16_t sq;
                std::memcpy(&ox, o, 2); std::memcpy(&oy, o + 2, 2); std::memcpy(&sq, o + 6, 2);
                if ((uint32_t)sq > (uint32_t)SV_SQMASK) return fail(c, LAMA_HIP_E_INVALID, "the uploaded distance map holds a squared distance beyond 16383 cells^2 (l2_max above 127 cells)");
                hsv[k * 1024 + ci] = (sv_t)((sv_t)sq | (o[8] ? SV_VALID : (sv_t)0) | (o[9] ? SV_QUEUED : (sv_t)0));
                hobs[k * 1024 + ci] = ((uint32_t)(uint16_t)ox) | (((uint32_t)(uint16_t)oy) << 16);      // (pack_obs)
            }
    }
    if (n) {           // a patch given twice is an error (checked on the ids: the window may still move below)
        std::vector<uint64_t> ids(patch_ids, patch_ids + n);
        std::sort(ids.begin(), ids.end());
        if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return fail(c, LAMA_HIP_E_INVALID, "a patch index appears twice in the uploaded map");
    }
    if (n) {   // the window must hold the patches (it is centred / moved / grown for them)
        int64_t x0 = INT64_MAX, x1 = INT64_MIN, y0 = INT64_MAX, y1 = INT64_MIN;
        for (uint32_t k = 0; k < n; ++k) {
            const int64_t px = (int64_t)(patch_ids[k] / 2642244ull), py = (int64_t)(patch_ids[k] % 2642244ull);
            x0 = std::min(x0, px); x1 = std::max(x1, px); y0 = std::min(y0, py); y1 = std::max(y1, py);
        }
        if (x1 - x0 + 1 > LAMA_HIP_MAX_WINDOW || y1 - y0 + 1 > LAMA_HIP_MAX_WINDOW) return fail(c, LAMA_HIP_E_WINDOW, "the map is wider than the largest device window (1016 patches)");
        const int32_t rw = ensure_window(c, x0, x1, y0, y1);
        if (rw) return rw;
    }
    { const int32_t rf = start_without_first_scan(c); if (rf) return rf; }
    {   // room for the patches (the particle's region moves if it must; what it held is replaced below)
        const HostPart& hp = c->h_part[particle];
        const uint32_t cap = dm ? hp.dm_cap : hp.occ_cap;
        if (n > cap) {
            const uint32_t want = want_capacity(dm ? c->floor_dm : c->floor_occ, n, 0u);
            const int32_t rg = set_capacities(c, {CapRequest{particle, dm ? want : hp.dm_cap, dm ? hp.occ_cap : want}});
            if (rg) return rg;
        }
    }
    const HostPart hp = c->h_part[particle];
    const PartRec pr = dev_part(c, hp);
    const size_t WW = (size_t)c->W * c->W;
    const int32_t old = c->h_counts[2 * particle + (dm ? 0 : 1)];
    // directory: slot k = the k-th given patch; a patch given twice is an error
    std::vector<int16_t> dir(WW, (int16_t)-1);
    for (uint32_t k = 0; k < n; ++k) {
        const int64_t wx = (int64_t)(patch_ids[k] / 2642244ull) - (int64_t)(c->wx0 >> 5), wy = (int64_t)(patch_ids[k] % 2642244ull) - (int64_t)(c->wy0 >> 5);
        if (wx < 0 || wy < 0 || wx >= (int64_t)c->W || wy >= (int64_t)c->W) return fail(c, LAMA_HIP_E_WINDOW, "a patch of the uploaded map fell outside the device window");
        int16_t& e = dir[(size_t)wy * c->W + (size_t)wx];
        if (e >= 0) return fail(c, LAMA_HIP_E_INVALID, "a patch index appears twice in the uploaded map");
        e = (int16_t)k;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // what the particle held before: zero the slots the new map does not overwrite ("unused slot == calloc'd")
    if (old > (int32_t)n) {
        const size_t keep = n, gone = (size_t)old - n;
        if (dm) {
            HIPCHK(c, hipMemsetAsync((char*)pr.dm_sv + keep * SV_PATCH_BYTES, 0, gone * SV_PATCH_BYTES, c->stream));
            HIPCHK(c, hipMemsetAsync((char*)pr.dm_obs + keep * 4096, 0, gone * 4096, c->stream));
            HIPCHK(c, hipMemsetAsync((char*)pr.dm_mask + keep * 128, 0, gone * 128, c->stream));
        } else {
            HIPCHK(c, hipMemsetAsync((char*)pr.occ + keep * 4096, 0, gone * 4096, c->stream));
            HIPCHK(c, hipMemsetAsync((char*)pr.occ_mask + keep * 128, 0, gone * 128, c->stream));
        }
    }
    // The copies go through the context's OWN stream, the one whose kernels read these planes afterwards with plain loads: a copy that
    // another stream carries out (a synchronous hipMemcpy runs on the null stream) into memory this context's kernels have read before
    // can leave them looking at cached lines of the old content -- the import of particle blobs taught that.
    if (n) {
        if (dm) {
            HIPCHK(c, hipMemcpyAsync(pr.dm_sv, hsv.data(), hsv.size() * SV_BYTES, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(pr.dm_obs, hobs.data(), hobs.size() * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(pr.dm_mask, masks, (size_t)n * 128, hipMemcpyHostToDevice, c->stream));
        } else {       // frequency {u16 occupied, u16 visited} / float log-odds: 4 B cells as they are
            HIPCHK(c, hipMemcpyAsync(pr.occ, cells, (size_t)n * 4096, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(pr.occ_mask, masks, (size_t)n * 128, hipMemcpyHostToDevice, c->stream));
        }
    }
    HIPCHK(c, hipMemcpyAsync((dm ? c->ms.dm_dir : c->ms.occ_dir) + hp.home * WW, dir.data(), WW * 2, hipMemcpyHostToDevice, c->stream));
    c->h_counts[2 * particle + (dm ? 0 : 1)] = (int32_t)n;
    HIPCHK(c, hipMemcpyAsync(c->ms.counts + 2 * particle + (dm ? 0 : 1), &c->h_counts[2 * particle + (dm ? 0 : 1)], sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                   // (the caller's buffers and the staging vectors are free again)
    if (!dm) c->visit_bound = 65535u;                             // unknown counters: let the wrap guard look before the next parallel ray-cast
    c->early_ok = false;
    return LAMA_HIP_OK;
}

// k_eval_batch for B poses; `timed`: the launch counts into ms_eval_batch / launches_eval_batch
static int32_t eval_batch_impl(lama_hip_ctx* c, uint32_t particle, const double* pts, uint32_t n, const double* origin3, const double* quat,
                               const double* poses, uint32_t B, double* sqnorm_out, double* loglik_out, bool timed)
{
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int32_t rc = upload_scan(c, pts, n);
    if (rc) return rc;
    rc = ensure_batch(c, 2 * (size_t)B);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_bposes, poses, sizeof(double) * 4 * B, hipMemcpyHostToDevice, c->stream));
    const Affine mtf = moving_tf(origin3, quat);
    DevParams prm = make_params(c);
    double* const d_sq = sqnorm_out ? (double*)c->d_bout : nullptr;
    double* const d_ll = loglik_out ? c->d_bout + B : nullptr;
    const auto launch = [&] { hipLaunchKernelGGL(k_eval_batch, dim3(B), dim3(SM_BLOCK), 0, c->stream, prm, (int)particle, c->d_pts, (int)n, mtf, c->d_bposes, d_sq, d_ll); };
    if (timed) {
        Timer t(c, &c->ctr.ms_eval_batch, &c->ctr.launches_eval_batch);
        launch();
        t.stop();
    } else launch();
    HIPCHK(c, hipGetLastError());
    if (sqnorm_out) HIPCHK(c, hipMemcpyAsync(sqnorm_out, d_sq, sizeof(double) * B, hipMemcpyDeviceToHost, c->stream));
    if (loglik_out) HIPCHK(c, hipMemcpyAsync(loglik_out, d_ll, sizeof(double) * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_timers(c);
    return LAMA_HIP_OK;
}

int32_t lama_hip_match_batch(lama_hip_ctx* c, uint32_t particle, const double* pts, uint32_t n, const double* origin3,
                             const double* quat, const double* poses, uint32_t B, double* out)
{
    if (!c || !pts || !poses || !out || n == 0 || B == 0 || particle >= c->P) return LAMA_HIP_E_INVALID;
    ENTER(c);
    if (!c->initialised) return fail(c, LAMA_HIP_E_STATE, "lama_hip_match_batch before lama_hip_pf_init");
    return eval_batch_impl(c, particle, pts, n, origin3, quat, poses, B, nullptr, out, false);
}

int32_t lama_hip_eval_batch(lama_hip_ctx* c, uint32_t particle, const double* pts, uint32_t n, const double* origin3,
                            const double* quat, const double* poses, uint32_t B, double* sqnorm_out, double* loglik_out)
{
    if (!c || !poses || (!sqnorm_out && !loglik_out) || n == 0 || B == 0 || particle >= c->P) return LAMA_HIP_E_INVALID;
    ENTER(c);
    if (!c->initialised) return fail(c, LAMA_HIP_E_STATE, "lama_hip_eval_batch before the map exists");
    return eval_batch_impl(c, particle, pts, n, origin3, quat, poses, B, sqnorm_out, loglik_out, true);
}

int32_t lama_hip_map_sample_likelihood(lama_hip_ctx* c, uint32_t particle, const double* pts, uint32_t n, const double* origin3,
                                       const double* quat, double yaw, const double* xy, uint32_t K, uint32_t point_step, double* l_out)
{
    if (!c || !xy || !l_out || n == 0 || K == 0 || point_step == 0 || particle >= c->P) return LAMA_HIP_E_INVALID;
    ENTER(c);
    if (!c->initialised) return fail(c, LAMA_HIP_E_STATE, "lama_hip_map_sample_likelihood before the map exists");
    if ((n + point_step - 1) / point_step > (uint32_t)SL_MAX_TERMS)
        return fail(c, LAMA_HIP_E_INVALID, "more than " + std::to_string(SL_MAX_TERMS) + " sampled points per pose");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int32_t rc = upload_scan(c, pts, n);
    if (rc) return rc;
    rc = ensure_batch(c, 2 * (size_t)K);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_bposes, xy, sizeof(double) * 2 * K, hipMemcpyHostToDevice, c->stream));
    // (Translation(x, y, 0) * AngleAxis(yaw, Z)) * moving_tf without the per-sample translation (src/loc2d.cpp:211-224)
    const Affine mtf = moving_tf(origin3, quat);
    const double sn = std::sin(yaw), cs = std::cos(yaw);          // Eigen AngleAxis(yaw, UnitZ), as in host_scan_tf
    Affine fixed;
    const double F[3][3] = {{cs, 0.0 - sn, 0.0}, {sn, cs, 0.0}, {0.0, 0.0, (1.0 - cs) + cs}};
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) fixed.R[i][j] = F[i][j]; fixed.t[i] = 0.0; }
    Affine base;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) base.R[i][j] = (fixed.R[i][0] * mtf.R[0][j] + fixed.R[i][1] * mtf.R[1][j]) + fixed.R[i][2] * mtf.R[2][j];
        base.t[i] = (fixed.R[i][0] * mtf.t[0] + fixed.R[i][1] * mtf.t[1]) + fixed.R[i][2] * mtf.t[2];
    }
    DevParams prm = make_params(c);
    hipLaunchKernelGGL(k_sample_likelihood, dim3(K), dim3(64), 0, c->stream, prm, (int)particle, c->d_pts, (int)n, (int)point_step, base,
                       c->d_bposes, c->d_bout);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(l_out, c->d_bout, sizeof(double) * K, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LAMA_HIP_OK;
}

// ------------------------------------------------------------------------------------------------
// SE2 pose-graph linearisation (lama_pgo.h)
// ------------------------------------------------------------------------------------------------
struct lama_hip_pgo {
    int32_t device = 0;
    uint32_t N = 0, F = 0, blocksF = 0;
    Stream stream;
    Event ev0, ev1;
    DevBuf<double> d_poses, d_meas, d_sqrt, d_err, d_hoff, d_fdi, d_fdj, d_fg, d_hdiag, d_b, d_chi;
    DevBuf<int32_t> d_fi, d_fj, d_incptr, d_inc;
    std::vector<double> h_chi;
    std::string error;
    // the Levenberg-Marquardt loop (lama_hip_pgo_set_poses .. _accept): d_poses is the current state, d_cand the candidate
    uint32_t nnzb = 0;
    std::vector<int32_t> h_rowptr, h_cols;
    DevBuf<double> d_cand, d_dx, d_blocks, d_diag, d_half;
    DevBuf<int32_t> d_brow, d_bcol, d_cptr, d_contrib;
    bool candidate_pending = false;        // d_cand holds the candidate of a try_step that no accept / set_poses / linearize followed
    // the device solver of the damped system (lama_pgo_pcg.h; lama_hip_pgo_solve_pcg, _try_solved_step)
    uint32_t parts_pq = 0, parts_v = 0;    // partials per dot product: one per PCG_ROWS rows (p.q), one per PGO_BLOCK poses (the others)
    DevBuf<int32_t> d_rowptr, d_tptr, d_tidx;
    DevBuf<double> d_minv, d_px, d_pr, d_pz, d_pp, d_pq, d_part_pq, d_part_rr, d_part_rz;
    DevBuf<PcgState> d_pcg;
    bool system_valid = false;             // d_blocks / d_b / d_diag are the system at d_poses (linearize_system since the state last changed)
    bool solution_valid = false;           // d_px solves that system (solve_pcg since)
    // per-factor robust losses (lama_hip_pgo_create_robust): allocated only when a factor has one; without, the graph launches
    // k_pgo_factors / k_pgo_error as lama_hip_pgo_create's does
    bool robust = false;
    bool linearized = false;               // a linearize / linearize_system has run: lama_hip_pgo_factor_weights has something to return
    DevBuf<int32_t> d_loss_kind;
    DevBuf<double> d_loss_param, d_weight;

    __attribute__((visibility("hidden"))) ~lama_hip_pgo() { (void)hipSetDevice(device); }     // (not exported: the C-ABI is)
};

#define PGOCHK(g, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { (g)->error = std::string(#call) + ": " + hipGetErrorString(e_); return LAMA_HIP_E_HIP; } } while (0)

static thread_local std::string g_pgo_create_error;     // why the last lama_hip_pgo_create_robust of this thread refused its losses

// loss_kind / loss_param: NULL, or validated by the caller ([F] each)
static int32_t pgo_create(int32_t device, uint32_t N, const int32_t* fi, const int32_t* fj, const double* meas4, const double* sqrt_info3,
                          const int32_t* loss_kind, const double* loss_param, uint32_t F, lama_hip_pgo** out)
{
    if (!out || !fi || !fj || !meas4 || !sqrt_info3 || N == 0 || F == 0) return LAMA_HIP_E_INVALID;
    *out = nullptr;
    for (uint32_t k = 0; k < F; ++k)
        if (fi[k] < 0 || (uint32_t)fi[k] >= N || fj[k] >= (int32_t)N || fj[k] == fi[k]) return LAMA_HIP_E_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= device || device < 0) return LAMA_HIP_E_HIP;
    if (hipSetDevice(device) != hipSuccess) return LAMA_HIP_E_HIP;
    std::unique_ptr<lama_hip_pgo, Delete> p(new lama_hip_pgo);             // (released into *out on success only)
    p->device = device; p->N = N; p->F = F; p->blocksF = (F + PGO_BLOCK - 1) / PGO_BLOCK;
    // incidence lists in factor order (counting sort): what the reference's sequential loop over the factors adds to a variable
    std::vector<int32_t> ptr(N + 1, 0), inc;
    for (uint32_t k = 0; k < F; ++k) { ++ptr[fi[k] + 1]; if (fj[k] >= 0) ++ptr[fj[k] + 1]; }
    for (uint32_t v = 0; v < N; ++v) ptr[v + 1] += ptr[v];
    inc.resize(ptr[N]);
    std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
    for (uint32_t k = 0; k < F; ++k) { inc[fill[fi[k]]++] = (int32_t)(2 * k); if (fj[k] >= 0) inc[fill[fj[k]]++] = (int32_t)(2 * k + 1); }
    // (hipSuccess is 0: each condition below stops at its first failing call)
    if (hipStreamCreate(&p->stream.h) || hipEventCreate(&p->ev0.h) || hipEventCreate(&p->ev1.h)) return LAMA_HIP_E_HIP;
    if (p->d_poses.alloc(4 * (size_t)N) || p->d_meas.alloc(4 * (size_t)F) || p->d_sqrt.alloc(3 * (size_t)F) || p->d_err.alloc(3 * (size_t)F) ||
        p->d_hoff.alloc(9 * (size_t)F) || p->d_fdi.alloc(9 * (size_t)F) || p->d_fdj.alloc(9 * (size_t)F) || p->d_fg.alloc(6 * (size_t)F) ||
        p->d_hdiag.alloc(9 * (size_t)N) || p->d_b.alloc(3 * (size_t)N) || p->d_chi.alloc(p->blocksF) ||
        p->d_fi.alloc(F) || p->d_fj.alloc(F) || p->d_incptr.alloc((size_t)N + 1) || p->d_inc.alloc(std::max<size_t>(inc.size(), 1)))
        return LAMA_HIP_E_HIP;
    if (hipMemcpy(p->d_fi, fi, sizeof(int32_t) * F, hipMemcpyHostToDevice) || hipMemcpy(p->d_fj, fj, sizeof(int32_t) * F, hipMemcpyHostToDevice) ||
        hipMemcpy(p->d_meas, meas4, sizeof(double) * 4 * F, hipMemcpyHostToDevice) ||
        hipMemcpy(p->d_sqrt, sqrt_info3, sizeof(double) * 3 * F, hipMemcpyHostToDevice) ||
        hipMemcpy(p->d_incptr, ptr.data(), sizeof(int32_t) * (N + 1), hipMemcpyHostToDevice) ||
        hipMemcpy(p->d_inc, inc.data(), sizeof(int32_t) * inc.size(), hipMemcpyHostToDevice))
        return LAMA_HIP_E_HIP;
    p->h_chi.resize(p->blocksF);
    const lama::pgo::BlockPattern bp = lama::pgo::lowerBlockPattern(N, fi, fj, F);    // (host/pgo_pattern.hpp)
    const std::vector<int32_t>&brow = bp.rows, &bcol = bp.cols, &cptr = bp.cptr, &contrib = bp.contrib;
    p->nnzb = (uint32_t)bcol.size();
    p->h_rowptr = bp.row_ptr;
    p->h_cols = bcol;
    if (p->d_cand.alloc(4 * (size_t)N) || p->d_dx.alloc(3 * (size_t)N) || p->d_blocks.alloc(9 * (size_t)p->nnzb) ||
        p->d_diag.alloc(3 * (size_t)N) || p->d_half.alloc(1) || p->d_brow.alloc(p->nnzb) || p->d_bcol.alloc(p->nnzb) ||
        p->d_cptr.alloc((size_t)p->nnzb + 1) || p->d_contrib.alloc(std::max<size_t>(contrib.size(), 1)))
        return LAMA_HIP_E_HIP;
    if (hipMemcpy(p->d_brow, brow.data(), sizeof(int32_t) * p->nnzb, hipMemcpyHostToDevice) ||
        hipMemcpy(p->d_bcol, bcol.data(), sizeof(int32_t) * p->nnzb, hipMemcpyHostToDevice) ||
        hipMemcpy(p->d_cptr, cptr.data(), sizeof(int32_t) * cptr.size(), hipMemcpyHostToDevice) ||
        (!contrib.empty() && hipMemcpy(p->d_contrib, contrib.data(), sizeof(int32_t) * contrib.size(), hipMemcpyHostToDevice)))
        return LAMA_HIP_E_HIP;
    // the transpose index of the lower pattern (lama_pgo_pcg.h): for every row r the off-diagonal blocks whose COLUMN is r, ascending
    // in their row (the blocks are stored by ascending row, so a counting sort by column keeps that order)
    std::vector<int32_t> tptr(N + 1, 0), tidx;
    for (uint32_t q = 0; q < p->nnzb; ++q) if (brow[q] != bcol[q]) ++tptr[bcol[q] + 1];
    for (uint32_t v = 0; v < N; ++v) tptr[v + 1] += tptr[v];
    tidx.resize(tptr[N]);
    { std::vector<int32_t> at(tptr.begin(), tptr.end() - 1);
      for (uint32_t q = 0; q < p->nnzb; ++q) if (brow[q] != bcol[q]) tidx[at[bcol[q]]++] = (int32_t)q; }
    p->parts_pq = (N + PCG_ROWS - 1) / PCG_ROWS;
    p->parts_v = (N + PGO_BLOCK - 1) / PGO_BLOCK;
    if (p->d_rowptr.alloc((size_t)N + 1) || p->d_tptr.alloc((size_t)N + 1) || p->d_tidx.alloc(std::max<size_t>(tidx.size(), 1)) ||
        p->d_minv.alloc(9 * (size_t)N) || p->d_px.alloc(3 * (size_t)N) || p->d_pr.alloc(3 * (size_t)N) || p->d_pz.alloc(3 * (size_t)N) ||
        p->d_pp.alloc(3 * (size_t)N) || p->d_pq.alloc(3 * (size_t)N) || p->d_part_pq.alloc(p->parts_pq) || p->d_part_rr.alloc(p->parts_v) ||
        p->d_part_rz.alloc(p->parts_v) || p->d_pcg.alloc(1))
        return LAMA_HIP_E_HIP;
    if (hipMemcpy(p->d_rowptr, bp.row_ptr.data(), sizeof(int32_t) * (N + 1), hipMemcpyHostToDevice) ||
        hipMemcpy(p->d_tptr, tptr.data(), sizeof(int32_t) * (N + 1), hipMemcpyHostToDevice) ||
        (!tidx.empty() && hipMemcpy(p->d_tidx, tidx.data(), sizeof(int32_t) * tidx.size(), hipMemcpyHostToDevice)))
        return LAMA_HIP_E_HIP;
    for (uint32_t k = 0; loss_kind && k < F; ++k) p->robust = p->robust || loss_kind[k] != LAMA_HIP_PGO_LOSS_NONE;
    if (p->robust) {
        std::vector<double> prm(F, 0.0);                                   // Cauchy: k2_ = k * k, formed once (LossFunction.h:162)
        for (uint32_t k = 0; k < F; ++k)
            if (loss_kind[k] != LAMA_HIP_PGO_LOSS_NONE) prm[k] = loss_kind[k] == LAMA_HIP_PGO_LOSS_CAUCHY ? loss_param[k] * loss_param[k] : loss_param[k];
        if (p->d_loss_kind.alloc(F) || p->d_loss_param.alloc(F) || p->d_weight.alloc(F)) return LAMA_HIP_E_HIP;
        if (hipMemcpy(p->d_loss_kind, loss_kind, sizeof(int32_t) * F, hipMemcpyHostToDevice) ||
            hipMemcpy(p->d_loss_param, prm.data(), sizeof(double) * F, hipMemcpyHostToDevice))
            return LAMA_HIP_E_HIP;
    }
    *out = p.release();
    return LAMA_HIP_OK;
}

int32_t lama_hip_pgo_create(int32_t device, uint32_t N, const int32_t* fi, const int32_t* fj, const double* meas4, const double* sqrt_info3,
                            uint32_t F, lama_hip_pgo** out)
{
    return pgo_create(device, N, fi, fj, meas4, sqrt_info3, nullptr, nullptr, F, out);
}

int32_t lama_hip_pgo_create_robust(int32_t device, uint32_t N, const int32_t* fi, const int32_t* fj, const double* meas4,
                                   const double* sqrt_info3, const int32_t* loss_kind, const double* loss_param, uint32_t F, lama_hip_pgo** out)
{
    g_pgo_create_error.clear();
    if (out) *out = nullptr;
    for (uint32_t k = 0; loss_kind && k < F; ++k) {
        const int32_t kind = loss_kind[k];
        if (kind < LAMA_HIP_PGO_LOSS_NONE || kind > LAMA_HIP_PGO_LOSS_DCS) {
            g_pgo_create_error = "lama_hip_pgo_create_robust: factor " + std::to_string(k) + " has the unknown loss kind " + std::to_string(kind);
            return LAMA_HIP_E_INVALID;
        }
        if (kind == LAMA_HIP_PGO_LOSS_NONE) continue;
        if (!loss_param || !std::isfinite(loss_param[k]) || !(loss_param[k] > 0.0)) {
            g_pgo_create_error = "lama_hip_pgo_create_robust: factor " + std::to_string(k) + " has a robust loss whose parameter is not finite and > 0";
            return LAMA_HIP_E_INVALID;
        }
    }
    return pgo_create(device, N, fi, fj, meas4, sqrt_info3, loss_kind, loss_param, F, out);
}

void lama_hip_pgo_destroy(lama_hip_pgo* g) { delete g; }

const char* lama_hip_pgo_last_error(const lama_hip_pgo* g)
{
    if (g) return g->error.c_str();
    return g_pgo_create_error.empty() ? "null handle" : g_pgo_create_error.c_str();     // (a refused create_robust left no handle to ask)
}

static PgoLossPtrs pgo_loss_ptrs(lama_hip_pgo* g) { return PgoLossPtrs{g->d_loss_kind, g->d_loss_param, g->d_weight}; }

int32_t lama_hip_pgo_factor_weights(lama_hip_pgo* g, double* w)
{
    if (!g || !w) return LAMA_HIP_E_INVALID;
    if (!g->linearized) {
        g->error = "lama_hip_pgo_factor_weights: nothing linearised yet (call lama_hip_pgo_linearize or lama_hip_pgo_linearize_system first)";
        return LAMA_HIP_E_STATE;
    }
    if (!g->robust) { std::fill(w, w + g->F, 1.0); return LAMA_HIP_OK; }
    PGOCHK(g, hipSetDevice(g->device));
    PGOCHK(g, hipMemcpyAsync(w, g->d_weight, sizeof(double) * g->F, hipMemcpyDeviceToHost, g->stream));
    PGOCHK(g, hipStreamSynchronize(g->stream));
    return LAMA_HIP_OK;
}

int32_t lama_hip_pgo_linearize(lama_hip_pgo* g, const double* poses4, double* err, double* Hdiag, double* Hoff, double* b, double* chi2,
                               double* kernel_ms)
{
    if (!g || !poses4) return LAMA_HIP_E_INVALID;
    g->candidate_pending = false;
    g->system_valid = g->solution_valid = false;
    PGOCHK(g, hipSetDevice(g->device));
    PGOCHK(g, hipMemcpyAsync(g->d_poses, poses4, sizeof(double) * 4 * g->N, hipMemcpyHostToDevice, g->stream));
    PgoPtrs p{g->d_poses, g->d_fi, g->d_fj, g->d_meas, g->d_sqrt, g->d_err, g->d_hoff, g->d_fdi, g->d_fdj, g->d_fg, g->d_incptr, g->d_inc,
              g->d_hdiag, g->d_b, g->d_chi};
    PGOCHK(g, hipEventRecord(g->ev0, g->stream));
    if (g->robust) hipLaunchKernelGGL(k_pgo_factors_robust, dim3(g->blocksF), dim3(PGO_BLOCK), 0, g->stream, p, pgo_loss_ptrs(g), g->F);
    else hipLaunchKernelGGL(k_pgo_factors, dim3(g->blocksF), dim3(PGO_BLOCK), 0, g->stream, p, g->F);
    hipLaunchKernelGGL(k_pgo_reduce, dim3((g->N + PGO_BLOCK - 1) / PGO_BLOCK), dim3(PGO_BLOCK), 0, g->stream, p, g->N);
    PGOCHK(g, hipEventRecord(g->ev1, g->stream));
    PGOCHK(g, hipGetLastError());
    if (err) PGOCHK(g, hipMemcpyAsync(err, g->d_err, sizeof(double) * 3 * g->F, hipMemcpyDeviceToHost, g->stream));
    if (Hoff) PGOCHK(g, hipMemcpyAsync(Hoff, g->d_hoff, sizeof(double) * 9 * g->F, hipMemcpyDeviceToHost, g->stream));
    if (Hdiag) PGOCHK(g, hipMemcpyAsync(Hdiag, g->d_hdiag, sizeof(double) * 9 * g->N, hipMemcpyDeviceToHost, g->stream));
    if (b) PGOCHK(g, hipMemcpyAsync(b, g->d_b, sizeof(double) * 3 * g->N, hipMemcpyDeviceToHost, g->stream));
    PGOCHK(g, hipMemcpyAsync(g->h_chi.data(), g->d_chi, sizeof(double) * g->blocksF, hipMemcpyDeviceToHost, g->stream));
    PGOCHK(g, hipStreamSynchronize(g->stream));
    g->linearized = true;
    if (chi2) { double t = 0; for (double x : g->h_chi) t += x; *chi2 = t; }
    if (kernel_ms) { float ms = 0; PGOCHK(g, hipEventElapsedTime(&ms, g->ev0, g->ev1)); *kernel_ms = ms; }
    return LAMA_HIP_OK;
}

int32_t lama_hip_pgo_pattern(const lama_hip_pgo* g, int32_t* row_ptr, int32_t* cols, uint32_t* nnzb)
{
    if (!g || !nnzb) return LAMA_HIP_E_INVALID;
    *nnzb = g->nnzb;
    if (row_ptr) std::copy(g->h_rowptr.begin(), g->h_rowptr.end(), row_ptr);
    if (cols) std::copy(g->h_cols.begin(), g->h_cols.end(), cols);
    return LAMA_HIP_OK;
}

int32_t lama_hip_pgo_set_poses(lama_hip_pgo* g, const double* poses4)
{
    if (!g || !poses4) return LAMA_HIP_E_INVALID;
    g->candidate_pending = false;
    g->system_valid = g->solution_valid = false;
    PGOCHK(g, hipSetDevice(g->device));
    PGOCHK(g, hipMemcpyAsync(g->d_poses, poses4, sizeof(double) * 4 * g->N, hipMemcpyHostToDevice, g->stream));
    PGOCHK(g, hipStreamSynchronize(g->stream));
    return LAMA_HIP_OK;
}

int32_t lama_hip_pgo_get_poses(lama_hip_pgo* g, double* poses4)
{
    if (!g || !poses4) return LAMA_HIP_E_INVALID;
    PGOCHK(g, hipSetDevice(g->device));
    PGOCHK(g, hipMemcpyAsync(poses4, g->d_poses, sizeof(double) * 4 * g->N, hipMemcpyDeviceToHost, g->stream));
    PGOCHK(g, hipStreamSynchronize(g->stream));
    return LAMA_HIP_OK;
}

int32_t lama_hip_pgo_linearize_system(lama_hip_pgo* g, double* blocks, double* b, double* diag, double* half_chi2, double* kernel_ms)
{
    if (!g) return LAMA_HIP_E_INVALID;
    g->system_valid = g->solution_valid = false;   // (set again once the system is complete)
    PGOCHK(g, hipSetDevice(g->device));
    PgoPtrs p{g->d_poses, g->d_fi, g->d_fj, g->d_meas, g->d_sqrt, g->d_err, g->d_hoff, g->d_fdi, g->d_fdj, g->d_fg, g->d_incptr, g->d_inc,
              g->d_hdiag, g->d_b, g->d_chi};
    PgoSysPtrs s{g->d_hdiag, g->d_hoff, g->d_brow, g->d_bcol, g->d_cptr, g->d_contrib, g->d_blocks, g->d_diag};
    PGOCHK(g, hipEventRecord(g->ev0, g->stream));
    if (g->robust) hipLaunchKernelGGL(k_pgo_factors_robust, dim3(g->blocksF), dim3(PGO_BLOCK), 0, g->stream, p, pgo_loss_ptrs(g), g->F);
    else hipLaunchKernelGGL(k_pgo_factors, dim3(g->blocksF), dim3(PGO_BLOCK), 0, g->stream, p, g->F);
    hipLaunchKernelGGL(k_pgo_reduce, dim3((g->N + PGO_BLOCK - 1) / PGO_BLOCK), dim3(PGO_BLOCK), 0, g->stream, p, g->N);
    hipLaunchKernelGGL(k_pgo_assemble, dim3((g->nnzb + PGO_BLOCK - 1) / PGO_BLOCK), dim3(PGO_BLOCK), 0, g->stream, s, g->nnzb);
    hipLaunchKernelGGL(k_pgo_sum, dim3(1), dim3(64), 0, g->stream, (const double*)g->d_chi, g->blocksF, (double*)g->d_half);
    PGOCHK(g, hipEventRecord(g->ev1, g->stream));
    PGOCHK(g, hipGetLastError());
    if (blocks) PGOCHK(g, hipMemcpyAsync(blocks, g->d_blocks, sizeof(double) * 9 * g->nnzb, hipMemcpyDeviceToHost, g->stream));
    if (b) PGOCHK(g, hipMemcpyAsync(b, g->d_b, sizeof(double) * 3 * g->N, hipMemcpyDeviceToHost, g->stream));
    if (diag) PGOCHK(g, hipMemcpyAsync(diag, g->d_diag, sizeof(double) * 3 * g->N, hipMemcpyDeviceToHost, g->stream));
    double h = 0.0;
    PGOCHK(g, hipMemcpyAsync(&h, g->d_half, sizeof(double), hipMemcpyDeviceToHost, g->stream));
    PGOCHK(g, hipStreamSynchronize(g->stream));
    g->system_valid = true;
    g->linearized = true;
    if (half_chi2) *half_chi2 = h;
    if (kernel_ms) { float ms = 0; PGOCHK(g, hipEventElapsedTime(&ms, g->ev0, g->ev1)); *kernel_ms = ms; }
    return LAMA_HIP_OK;
}

int32_t lama_hip_pgo_try_step(lama_hip_pgo* g, const double* dx, double* half_chi2, double* kernel_ms)
{
    if (!g || !dx || !half_chi2) return LAMA_HIP_E_INVALID;
    g->candidate_pending = false;          // (set again once the candidate is complete)
    PGOCHK(g, hipSetDevice(g->device));
    PgoPtrs p{g->d_cand, g->d_fi, g->d_fj, g->d_meas, g->d_sqrt, g->d_err, g->d_hoff, g->d_fdi, g->d_fdj, g->d_fg, g->d_incptr, g->d_inc,
              g->d_hdiag, g->d_b, g->d_chi};
    PGOCHK(g, hipMemcpyAsync(g->d_dx, dx, sizeof(double) * 3 * g->N, hipMemcpyHostToDevice, g->stream));
    PGOCHK(g, hipEventRecord(g->ev0, g->stream));
    hipLaunchKernelGGL(k_pgo_retract, dim3((g->N + PGO_BLOCK - 1) / PGO_BLOCK), dim3(PGO_BLOCK), 0, g->stream, (const double*)g->d_poses,
                       (const double*)g->d_dx, (double*)g->d_cand, g->N);
    if (g->robust) hipLaunchKernelGGL(k_pgo_error_robust, dim3(g->blocksF), dim3(PGO_BLOCK), 0, g->stream, p, pgo_loss_ptrs(g), (const double*)g->d_cand, g->F);
    else hipLaunchKernelGGL(k_pgo_error, dim3(g->blocksF), dim3(PGO_BLOCK), 0, g->stream, p, (const double*)g->d_cand, g->F);
    hipLaunchKernelGGL(k_pgo_sum, dim3(1), dim3(64), 0, g->stream, (const double*)g->d_chi, g->blocksF, (double*)g->d_half);
    PGOCHK(g, hipEventRecord(g->ev1, g->stream));
    PGOCHK(g, hipGetLastError());
    double h = 0.0;
    PGOCHK(g, hipMemcpyAsync(&h, g->d_half, sizeof(double), hipMemcpyDeviceToHost, g->stream));
    PGOCHK(g, hipStreamSynchronize(g->stream));
    *half_chi2 = h;
    g->candidate_pending = true;
    if (kernel_ms) { float ms = 0; PGOCHK(g, hipEventElapsedTime(&ms, g->ev0, g->ev1)); *kernel_ms = ms; }
    return LAMA_HIP_OK;
}

int32_t lama_hip_pgo_accept(lama_hip_pgo* g)
{
    if (!g) return LAMA_HIP_E_INVALID;
    if (!g->candidate_pending) {           // (the swap would bring back whatever the candidate buffer held before)
        g->error = "lama_hip_pgo_accept: no candidate pending (call lama_hip_pgo_try_step first)";
        return LAMA_HIP_E_STATE;
    }
    g->candidate_pending = false;
    g->system_valid = g->solution_valid = false;
    g->d_poses.swap(g->d_cand);            // (the stream is idle: try_step synchronised it)
    return LAMA_HIP_OK;
}

// ---- the damped system solved on the device (lama_pgo_pcg.h)
static PcgPtrs pcg_ptrs(lama_hip_pgo* g)
{
    return PcgPtrs{g->d_blocks, g->d_diag, g->d_b, g->d_rowptr, g->d_bcol, g->d_brow, g->d_tptr, g->d_tidx, g->d_minv, g->d_px, g->d_pr,
                   g->d_pz, g->d_pp, g->d_pq, g->d_part_pq, g->d_part_rr, g->d_part_rz, g->d_pcg};
}

int32_t lama_hip_pgo_solve_pcg(lama_hip_pgo* g, double lambda, double rel_tol, uint32_t max_iterations, uint32_t batch, double* dx,
                               uint32_t* iterations, double* rel_residual_sq, int32_t* outcome, double* model_decrease, double* kernel_ms)
{
    if (!g) return LAMA_HIP_E_INVALID;
    if (!(lambda >= 0.0) || !std::isfinite(lambda) || !(rel_tol > 0.0 && rel_tol < 1.0) || max_iterations == 0) {
        g->error = "lama_hip_pgo_solve_pcg: lambda must be finite and >= 0, rel_tol in (0, 1), max_iterations > 0";
        return LAMA_HIP_E_INVALID;
    }
    if (!g->system_valid) {
        g->error = "lama_hip_pgo_solve_pcg: no linear system at the current state (call lama_hip_pgo_linearize_system first)";
        return LAMA_HIP_E_STATE;
    }
    if (batch == 0) batch = LAMA_HIP_PCG_DEFAULT_BATCH;
    g->solution_valid = false;
    PGOCHK(g, hipSetDevice(g->device));
    const PcgPtrs s = pcg_ptrs(g);
    const uint32_t N = g->N;
    const dim3 grid_v(g->parts_v), grid_pq(g->parts_pq), block(PGO_BLOCK);
    PcgState st;
    PGOCHK(g, hipMemsetAsync(g->d_pcg, 0, sizeof(PcgState), g->stream));
    PGOCHK(g, hipEventRecord(g->ev0, g->stream));
    hipLaunchKernelGGL(k_pgo_pcg_setup, grid_v, block, 0, g->stream, s, lambda, N);
    hipLaunchKernelGGL(k_pgo_pcg_begin, dim3(1), dim3(64), 0, g->stream, s, rel_tol * rel_tol, g->parts_v);
    PGOCHK(g, hipGetLastError());
    PGOCHK(g, hipMemcpyAsync(&st, g->d_pcg, sizeof(PcgState), hipMemcpyDeviceToHost, g->stream));
    PGOCHK(g, hipStreamSynchronize(g->stream));
    uint32_t enqueued = 0;
    while (st.done == 0 && enqueued < max_iterations) {
        const uint32_t n = std::min(batch, max_iterations - enqueued);
        for (uint32_t k = enqueued; k < enqueued + n; ++k) {
            hipLaunchKernelGGL(k_pgo_pcg_spmv, grid_pq, block, 0, g->stream, s, lambda, N);
            hipLaunchKernelGGL(k_pgo_pcg_step, grid_v, block, 0, g->stream, s, k & 1u, g->parts_pq, N);
            hipLaunchKernelGGL(k_pgo_pcg_dir, grid_v, block, 0, g->stream, s, k, g->parts_pq, g->parts_v, N);
        }
        enqueued += n;
        PGOCHK(g, hipGetLastError());
        PGOCHK(g, hipMemcpyAsync(&st, g->d_pcg, sizeof(PcgState), hipMemcpyDeviceToHost, g->stream));
        PGOCHK(g, hipStreamSynchronize(g->stream));
    }
    hipLaunchKernelGGL(k_pgo_pcg_model, grid_v, block, 0, g->stream, s, lambda, N);
    hipLaunchKernelGGL(k_pgo_sum, dim3(1), dim3(64), 0, g->stream, (const double*)g->d_part_rr, g->parts_v, &((PcgState*)g->d_pcg)->model);
    PGOCHK(g, hipEventRecord(g->ev1, g->stream));
    PGOCHK(g, hipGetLastError());
    PGOCHK(g, hipMemcpyAsync(&st, g->d_pcg, sizeof(PcgState), hipMemcpyDeviceToHost, g->stream));
    if (dx) PGOCHK(g, hipMemcpyAsync(dx, g->d_px, sizeof(double) * 3 * N, hipMemcpyDeviceToHost, g->stream));
    PGOCHK(g, hipStreamSynchronize(g->stream));
    const int32_t oc = st.done == PCG_CONVERGED ? LAMA_HIP_PCG_CONVERGED : st.done == PCG_BREAKDOWN ? LAMA_HIP_PCG_BREAKDOWN : LAMA_HIP_PCG_CAP;
    g->solution_valid = oc != LAMA_HIP_PCG_BREAKDOWN;
    if (iterations) *iterations = st.iters;
    if (rel_residual_sq) *rel_residual_sq = st.bb == 0.0 ? 0.0 : st.rr / st.bb;
    if (outcome) *outcome = oc;
    if (model_decrease) *model_decrease = st.model;
    if (kernel_ms) { float ms = 0; PGOCHK(g, hipEventElapsedTime(&ms, g->ev0, g->ev1)); *kernel_ms = ms; }
    return LAMA_HIP_OK;
}

int32_t lama_hip_pgo_try_solved_step(lama_hip_pgo* g, double* half_chi2, double* kernel_ms)
{
    if (!g || !half_chi2) return LAMA_HIP_E_INVALID;
    if (!g->solution_valid) {
        g->error = "lama_hip_pgo_try_solved_step: no solution of the system at the current state (call lama_hip_pgo_solve_pcg first)";
        return LAMA_HIP_E_STATE;
    }
    g->candidate_pending = false;          // (set again once the candidate is complete)
    PGOCHK(g, hipSetDevice(g->device));
    PgoPtrs p{g->d_cand, g->d_fi, g->d_fj, g->d_meas, g->d_sqrt, g->d_err, g->d_hoff, g->d_fdi, g->d_fdj, g->d_fg, g->d_incptr, g->d_inc,
              g->d_hdiag, g->d_b, g->d_chi};
    PGOCHK(g, hipEventRecord(g->ev0, g->stream));
    hipLaunchKernelGGL(k_pgo_retract, dim3((g->N + PGO_BLOCK - 1) / PGO_BLOCK), dim3(PGO_BLOCK), 0, g->stream, (const double*)g->d_poses,
                       (const double*)g->d_px, (double*)g->d_cand, g->N);
    if (g->robust) hipLaunchKernelGGL(k_pgo_error_robust, dim3(g->blocksF), dim3(PGO_BLOCK), 0, g->stream, p, pgo_loss_ptrs(g), (const double*)g->d_cand, g->F);
    else hipLaunchKernelGGL(k_pgo_error, dim3(g->blocksF), dim3(PGO_BLOCK), 0, g->stream, p, (const double*)g->d_cand, g->F);
    hipLaunchKernelGGL(k_pgo_sum, dim3(1), dim3(64), 0, g->stream, (const double*)g->d_chi, g->blocksF, (double*)g->d_half);
    PGOCHK(g, hipEventRecord(g->ev1, g->stream));
    PGOCHK(g, hipGetLastError());
    double h = 0.0;
    PGOCHK(g, hipMemcpyAsync(&h, g->d_half, sizeof(double), hipMemcpyDeviceToHost, g->stream));
    PGOCHK(g, hipStreamSynchronize(g->stream));
    *half_chi2 = h;
    g->candidate_pending = true;
    if (kernel_ms) { float ms = 0; PGOCHK(g, hipEventElapsedTime(&ms, g->ev0, g->ev1)); *kernel_ms = ms; }
    return LAMA_HIP_OK;
}

int32_t lama_hip_map_add_obstacles(lama_hip_ctx* c, uint32_t particle, const uint32_t* cells_xy, uint32_t n)
{
    if (!c || !cells_xy || n == 0 || particle >= c->P) return LAMA_HIP_E_INVALID;
    ENTER(c);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    {   // the window must hold the listed cells and what the brushfire reaches from them (it is centred / moved / grown for that)
        const int64_t r = (int64_t)guard_radius(c);
        int64_t x0 = INT64_MAX, x1 = INT64_MIN, y0 = INT64_MAX, y1 = INT64_MIN;
        for (uint32_t i = 0; i < n; ++i) {
            const int64_t px = cells_xy[2 * i] >> 5, py = cells_xy[2 * i + 1] >> 5;
            x0 = std::min(x0, px); x1 = std::max(x1, px); y0 = std::min(y0, py); y1 = std::max(y1, py);
        }
        const int32_t rw = ensure_window(c, x0 - r, x1 + r, y0 - r, y1 + r);
        if (rw) return rw;
    }
    { const int32_t rf = start_without_first_scan(c); if (rf) return rf; }
    {   // every distance-map patch this call can allocate lies within guard_r patches of a listed cell's patch: make room first
        const int r = (int)guard_radius(c);
        std::vector<uint64_t> keys;
        keys.reserve((size_t)n);
        uint64_t last = ~0ull;
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t k = ((uint64_t)(cells_xy[2 * i + 1] >> 5) << 32) | (uint64_t)(cells_xy[2 * i] >> 5);
            if (k != last) { keys.push_back(k); last = k; }
        }
        std::sort(keys.begin(), keys.end());
        keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
        std::vector<uint64_t> dil;
        dil.reserve(keys.size() * (size_t)((2 * r + 1) * (2 * r + 1)));
        for (uint64_t k : keys)
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) dil.push_back((((k >> 32) + (uint64_t)(int64_t)dy) << 32) | (uint32_t)((uint32_t)k + (uint32_t)dx));
        std::sort(dil.begin(), dil.end());
        dil.erase(std::unique(dil.begin(), dil.end()), dil.end());
        const uint64_t want = (uint64_t)c->h_counts[2 * particle] + dil.size();
        if (want > c->h_part[particle].dm_cap) {
            const int32_t rg = set_capacities(c, {CapRequest{particle, (uint32_t)std::min<uint64_t>(MAX_PATCHES, (want + 31u) / 32u * 32u), c->h_part[particle].occ_cap}});
            if (rg) return rg;
        }
        c->last_guarded = false;
    }
    DevBuf<uint32_t> cells;
    HIPCHK(c, cells.alloc(2 * (size_t)n));
    uint32_t* const d_cells = cells;                                // (launch arguments are plain pointers: the owners are not copied)
    HIPCHK(c, hipMemcpyAsync(d_cells, cells_xy, sizeof(uint32_t) * 2 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    DevParams prm = make_params(c);
    // queue capacity bounds one batch of additions; larger lists go in slices (each followed by dm->update(): adding
    // obstacles then updating in slices yields the same distance map only if no slice boundary matters -- so a list
    // longer than the queue is rejected instead)
    if (n > c->cfg.queue_capacity) return fail(c, LAMA_HIP_E_CAPACITY, "more obstacle cells than cfg.queue_capacity");
    HIPCHK(c, hipMemsetAsync(c->d_slow_n, 0, 5 * sizeof(uint32_t), c->stream));    // all five: check_device_errors(maps) adds every word to the counters
    hipLaunchKernelGGL(k_dm_add_obstacles, dim3(1), dim3(UM_BLOCK), 0, c->stream, prm, (int)particle, d_cells, n);
    hipLaunchKernelGGL((k_brushfire<LQ_SMALL, RQ_SMALL, false, true>), dim3(1), dim3(2 * UM_BLOCK), 0, c->stream, prm, (int)particle, 0);
    hipLaunchKernelGGL((k_brushfire<LQ_BIG, RQ_BIG, true, true>), dim3(1), dim3(2 * UM_BLOCK), 0, c->stream, prm, (int)particle, 0);
    hipLaunchKernelGGL(k_brushfire_slow, dim3(1), dim3(UM_BLOCK), 0, c->stream, prm, (int)particle);
    HIPCHK(c, hipGetLastError());
    c->last_first = 0; c->last_count = c->P;                        // (whose statistics check_device_errors reads)
    return check_device_errors(c, true, false);
}

// ---- lama_map_build.h: K posed key scans into one occupancy map, and the occupied cells of a map -----------------------------------
int32_t lama_hip_map_integrate_scans(lama_hip_ctx* c, uint32_t particle, uint32_t K, const double* poses4, const double* pts, const uint32_t* offs,
                                     const double* origins, const double* quats, uint32_t flags)
{
    if (!c || particle >= c->P || (flags & ~3u)) return LAMA_HIP_E_INVALID;
    ENTER(c);
    if (c->cfg.occupancy_policy != 0) return fail(c, LAMA_HIP_E_INVALID, "key scans are integrated into a frequency occupancy map (cfg.occupancy_policy 0)");
    if (K == 0) return LAMA_HIP_OK;
    if (!poses4 || !offs) return fail(c, LAMA_HIP_E_INVALID, "poses4 / scan_offsets missing");
    for (uint32_t k = 0; k < K; ++k)
        if (offs[k + 1] < offs[k]) return fail(c, LAMA_HIP_E_INVALID, "scan_offsets must not decrease");
    const uint64_t total64 = (uint64_t)offs[K] - offs[0];
    if (total64 == 0) return LAMA_HIP_OK;                           // nothing but empty scans: the reference's loop bodies never run
    if (!pts || total64 >= (uint64_t)MB_HIT) return fail(c, LAMA_HIP_E_INVALID, "pts_xyz missing, or more than 2^31 - 1 points");
    const uint32_t total = (uint32_t)total64;
    const bool full = flags & 1u, prune = flags & 2u;
    // tf = T(pose) * T(sensor origin) * R(sensor orientation) per scan, on the host like every map update's (host_scan_tf)
    c->h_mb_tfs.resize((size_t)12 * K); c->h_mb_offs.resize((size_t)K + 1);
    for (uint32_t k = 0; k < K; ++k) {
        host_scan_tf(poses4 + 4 * (size_t)k, moving_tf(origins ? origins + 3 * (size_t)k : nullptr, quats ? quats + 4 * (size_t)k : nullptr), &c->h_mb_tfs[12 * (size_t)k]);
        for (int j = 0; j < 12; ++j)
            if (!std::isfinite(c->h_mb_tfs[12 * (size_t)k + j])) return fail(c, LAMA_HIP_E_INVALID, "a key pose or sensor transform is not finite");
    }
    for (uint32_t k = 0; k <= K; ++k) c->h_mb_offs[k] = offs[k] - offs[0];
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, c->d_mb_pts.grow((size_t)3 * total)); HIPCHK(c, c->d_mb_tfs.grow((size_t)12 * K)); HIPCHK(c, c->d_mb_offs.grow((size_t)K + 1));
    HIPCHK(c, c->d_mb_rays.grow(total)); HIPCHK(c, c->d_mb_meta.grow(8));
    c->h_mb_meta.resize(8);
    MbBounds* const d_bounds = reinterpret_cast<MbBounds*>(c->d_mb_meta.p);
    MbMeta* const d_meta = reinterpret_cast<MbMeta*>(c->d_mb_meta.p + 4);
    {
        MbBounds b0{0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0u, 0u, 0ull};
        std::memcpy(c->h_mb_meta.data(), &b0, sizeof(b0));
    }
    // (all copies on the context's own stream, the one whose kernels read the buffers: DESIGN.md section 8)
    HIPCHK(c, hipMemcpyAsync(c->d_mb_meta, c->h_mb_meta.data(), sizeof(MbBounds), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_mb_pts, pts + 3 * (size_t)offs[0], sizeof(double) * 3 * total, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_mb_tfs, c->h_mb_tfs.data(), sizeof(double) * 12 * K, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_mb_offs, c->h_mb_offs.data(), sizeof(uint32_t) * ((size_t)K + 1), hipMemcpyHostToDevice, c->stream));
    auto untruncated_params = [c]() { DevParams p = make_params(c); p.trunc_ray = 0.0; p.trunc_range = 0.0; return p; };      // generateOccupancyMap truncates nothing
    DevParams prm = untruncated_params();
    const unsigned ray_blocks = (total + 255u) / 256u;
    MbRay* const d_rays = c->d_mb_rays;
    {
        Timer t(c, &c->ctr.ms_raycast, &c->ctr.launches_raycast);
        hipLaunchKernelGGL(k_mb_geom, dim3(ray_blocks), dim3(256), 0, c->stream, prm, (const double*)c->d_mb_pts, (const uint32_t*)c->d_mb_offs,
                           (const double*)c->d_mb_tfs, K, total, full ? 1 : 0, d_rays, d_bounds);
        t.stop();
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_mb_meta.data(), c->d_mb_meta, sizeof(MbBounds), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    MbBounds bnd;
    std::memcpy(&bnd, c->h_mb_meta.data(), sizeof(bnd));
    // ---- everything that can refuse the call comes before anything of the map changes ----
    if (bnd.flags & MB_NONFINITE) { resolve_timers(c); return fail(c, LAMA_HIP_E_INVALID, "a key scan holds a non-finite point (filter NaN / inf ranges first, as iris_lama_ros does)"); }
    if (bnd.flags & MB_TOO_LONG) { resolve_timers(c); return fail(c, LAMA_HIP_E_WINDOW, "a ray is longer than 8191 cells"); }
    {
        const int64_t x0 = bnd.x0, x1 = bnd.x1, y0 = bnd.y0, y1 = bnd.y1;
        const int64_t ux0 = c->mb_valid ? std::min(c->mbx0, x0) : x0, ux1 = c->mb_valid ? std::max(c->mbx1, x1) : x1;
        const int64_t uy0 = c->mb_valid ? std::min(c->mby0, y0) : y0, uy1 = c->mb_valid ? std::max(c->mby1, y1) : y1;
        if (ux1 - ux0 + 1 > LAMA_HIP_MAX_WINDOW || uy1 - uy0 + 1 > LAMA_HIP_MAX_WINDOW) {
            resolve_timers(c);
            return fail(c, LAMA_HIP_E_WINDOW, "the key scans and the map so far are wider than the largest device window (1016 patches)");
        }
        const int32_t rw = ensure_window(c, x0, x1, y0, y1);
        if (rw) { resolve_timers(c); return rw; }
    }
    { const int32_t rf = start_without_first_scan(c); if (rf) return rf; }
    const uint32_t bx0 = bnd.x0 - (c->wx0 >> 5), by0 = bnd.y0 - (c->wy0 >> 5), bw = bnd.x1 - bnd.x0 + 1u, bh = bnd.y1 - bnd.y0 + 1u, nb = bw * bh;
    if (bx0 + bw > c->W || by0 + bh > c->W) { resolve_timers(c); return fail(c, LAMA_HIP_E_WINDOW, "the key scans fell outside the device window"); }
    HIPCHK(c, c->d_mb_table.grow(nb)); HIPCHK(c, c->d_mb_off.grow((size_t)nb + 1)); HIPCHK(c, c->d_mb_list.grow(nb)); HIPCHK(c, c->d_mb_slot.grow(nb));
    prm = untruncated_params();
    uint32_t* const d_table = c->d_mb_table; uint32_t* const d_off = c->d_mb_off; uint32_t* const d_list = c->d_mb_list; int32_t* const d_slot = c->d_mb_slot;
    HIPCHK(c, hipMemsetAsync(d_table, 0, sizeof(uint32_t) * nb, c->stream));
    {
        Timer t(c, &c->ctr.ms_raycast, &c->ctr.launches_raycast);
        hipLaunchKernelGGL(k_mb_bin, dim3(ray_blocks), dim3(256), 0, c->stream, prm, (const MbRay*)d_rays, total, bx0, by0, bw, bh, d_table, (const uint32_t*)nullptr, (uint32_t*)nullptr);
        hipLaunchKernelGGL(k_mb_scan, dim3(1), dim3(MB_SCAN_BLOCK), 0, c->stream, prm, (int)particle, bx0, by0, bw, nb, d_table, d_off, d_list, d_meta);
        t.stop();
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_mb_meta.data() + 4, d_meta, sizeof(MbMeta), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    MbMeta meta;
    std::memcpy(&meta, c->h_mb_meta.data() + 4, sizeof(meta));
    const uint64_t want = (uint64_t)c->h_counts[2 * particle + 1] + meta.need;
    if (want > MAX_PATCHES) { resolve_timers(c); return fail(c, LAMA_HIP_E_CAPACITY, "the particle's occupancy map would exceed 32767 patches"); }
    if (want > c->h_part[particle].occ_cap) {
        const int32_t rg = set_capacities(c, {CapRequest{particle, c->h_part[particle].dm_cap, want_capacity(c->floor_occ, (uint32_t)want, 0u)}});
        if (rg) { resolve_timers(c); return rg; }
        prm = untruncated_params();
    }
    HIPCHK(c, c->d_mb_bins.grow(meta.items, (size_t)1 << 16));
    uint32_t* const d_bins = c->d_mb_bins;
    {
        Timer t(c, &c->ctr.ms_raycast, &c->ctr.launches_raycast);
        hipLaunchKernelGGL(k_mb_alloc, dim3((meta.touched + 255u) / 256u), dim3(256), 0, c->stream, prm, (int)particle, bx0, by0, bw, (const uint32_t*)d_list, meta.touched, d_slot);
        hipLaunchKernelGGL(k_mb_bin, dim3(ray_blocks), dim3(256), 0, c->stream, prm, (const MbRay*)d_rays, total, bx0, by0, bw, bh, d_table, (const uint32_t*)d_off, d_bins);
        hipLaunchKernelGGL(k_mb_patches, dim3(meta.touched), dim3(256), 0, c->stream, prm, (int)particle, bx0, by0, bw, (const uint32_t*)d_list, (const int32_t*)d_slot,
                           (const uint32_t*)d_off, (const uint32_t*)d_bins, (const MbRay*)d_rays);
        if (prune) hipLaunchKernelGGL(k_mb_prune, dim3((unsigned)std::min<uint64_t>(std::max<uint64_t>(want, 1), 4096)), dim3(256), 0, c->stream, prm, (int)particle);
        t.stop();
    }
    HIPCHK(c, hipGetLastError());
    c->h_err.resize(1);
    HIPCHK(c, hipMemcpyAsync(&c->h_counts[2 * particle], c->ms.counts + 2 * particle, sizeof(int32_t) * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&c->h_err[0], c->d_err, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_timers(c);
    c->ctr.ray_cells += bnd.visits;
    { uint64_t oc = 0; for (uint32_t p = 0; p < c->P; ++p) oc += (uint64_t)c->h_counts[2 * p + 1]; c->ctr.occ_patches = oc; }
    c->visit_bound = 65535u;                                      // unknown counters: the wrap guard looks before the next parallel ray-cast
    if (c->h_err[0] != 0) {                                       // (room was made for every patch: not expected)
        HIPCHK(c, hipMemsetAsync(c->d_err, 0, sizeof(int32_t), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return fail(c, LAMA_HIP_E_CAPACITY, "an occupancy patch could not be allocated while integrating key scans");
    }
    return LAMA_HIP_OK;
}

int32_t lama_hip_map_occupied_cells(lama_hip_ctx* c, uint32_t particle, uint32_t cap, uint32_t* cells_xy, uint32_t* n_out)
{
    if (!c || !n_out || particle >= c->P) return LAMA_HIP_E_INVALID;
    ENTER(c);
    if (c->cfg.occupancy_policy != 0) return fail(c, LAMA_HIP_E_INVALID, "occupied cells are listed for a frequency occupancy map (cfg.occupancy_policy 0)");
    *n_out = 0;
    const uint32_t count = (uint32_t)c->h_counts[2 * particle + 1];
    if (count == 0) return LAMA_HIP_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, c->d_mb_table.grow(count)); HIPCHK(c, c->d_mb_off.grow((size_t)count + 1)); HIPCHK(c, c->d_mb_list.grow(count)); HIPCHK(c, c->d_mb_slot.grow(count));
    uint32_t* const d_cnt = c->d_mb_table; uint32_t* const d_off = c->d_mb_off; uint32_t* const d_pos = c->d_mb_list; int32_t* const d_slot = c->d_mb_slot;
    const DevParams prm = make_params(c);
    hipLaunchKernelGGL(k_mb_order, dim3(1), dim3(MB_SCAN_BLOCK), 0, c->stream, prm, (int)particle, d_slot, d_pos);
    hipLaunchKernelGGL(k_mb_occupied, dim3(count), dim3(256), 0, c->stream, prm, (int)particle, (const int32_t*)d_slot, (const uint32_t*)d_pos, d_cnt, (const uint32_t*)nullptr, 0u, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_mb_exscan, dim3(1), dim3(MB_SCAN_BLOCK), 0, c->stream, (const uint32_t*)d_cnt, count, d_off);
    HIPCHK(c, hipGetLastError());
    uint32_t total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, d_off + count, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_out = total;
    const uint32_t m = std::min(cap, total);
    if (!cells_xy || m == 0) return LAMA_HIP_OK;
    HIPCHK(c, c->d_mb_bins.grow(2 * (size_t)m, (size_t)1 << 16));
    uint32_t* const d_out = c->d_mb_bins;
    hipLaunchKernelGGL(k_mb_occupied, dim3(count), dim3(256), 0, c->stream, prm, (int)particle, (const int32_t*)d_slot, (const uint32_t*)d_pos, d_cnt, (const uint32_t*)d_off, m, d_out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(cells_xy, d_out, sizeof(uint32_t) * 2 * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LAMA_HIP_OK;
}

// ---- lama_raster.h: the box of a map's patches, and a map written out as a dense grid ----------------------------------------------
int32_t lama_hip_map_bounds(lama_hip_ctx* c, uint32_t particle, int32_t kind, uint32_t min_xy[2], uint32_t max_xy[2], uint32_t* num_patches)
{
    if (!c || particle >= c->P || (kind != LAMA_HIP_MAP_DISTANCE && kind != LAMA_HIP_MAP_OCCUPANCY)) return LAMA_HIP_E_INVALID;
    ENTER(c);
    // Map::bounds of a map without patches (src/sdm/map.cpp:139-157): min stays at its start value, max is 0 + patch_length
    uint32_t lo[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, hi[2] = {32u, 32u}, n = 0;
    if (c->h_counts[2 * particle + (kind == LAMA_HIP_MAP_DISTANCE ? 0 : 1)] != 0) {
        HIPCHK(c, hipSetDevice(c->cfg.device));
        HIPCHK(c, c->d_raster.grow(sizeof(MapBoundsRec), (size_t)1 << 16));
        c->h_raster.reserve(sizeof(MapBoundsRec));
        MapBoundsRec* const d_rec = reinterpret_cast<MapBoundsRec*>(c->d_raster.p);
        hipLaunchKernelGGL(k_map_bounds, dim3(1), dim3(MB_SCAN_BLOCK), 0, c->stream, make_params(c), (int)particle, kind == LAMA_HIP_MAP_DISTANCE ? 0 : 1, d_rec);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(c->h_raster.data(), d_rec, sizeof(MapBoundsRec), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        MapBoundsRec r;
        std::memcpy(&r, c->h_raster.data(), sizeof(r));
        n = r.n;
        if (n) { lo[0] = c->wx0 + 32u * r.x0; lo[1] = c->wy0 + 32u * r.y0; hi[0] = c->wx0 + 32u * r.x1 + 32u; hi[1] = c->wy0 + 32u * r.y1 + 32u; }
    }
    if (min_xy) { min_xy[0] = lo[0]; min_xy[1] = lo[1]; }
    if (max_xy) { max_xy[0] = hi[0]; max_xy[1] = hi[1]; }
    if (num_patches) *num_patches = n;
    return LAMA_HIP_OK;
}

int32_t lama_hip_map_rasterize(lama_hip_ctx* c, uint32_t particle, int32_t layer, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
                               uint32_t stride, void* out, uint64_t out_bytes)
{
    if (!c || !out || particle >= c->P) return LAMA_HIP_E_INVALID;
    ENTER(c);
    // ---- everything that can refuse the call comes before anything is written ----
    if (layer != LAMA_HIP_RASTER_TRINARY && layer != LAMA_HIP_RASTER_PROBABILITY && layer != LAMA_HIP_RASTER_SQDIST) return fail(c, LAMA_HIP_E_INVALID, "unknown raster layer");
    if (layer == LAMA_HIP_RASTER_PROBABILITY && c->cfg.occupancy_policy != 0)
        return fail(c, LAMA_HIP_E_INVALID, "the probability layer is exact for the frequency occupancy policy only (cfg.occupancy_policy 0)");
    uint32_t log2s = 0;
    while (log2s < 6u && (1u << log2s) != stride) ++log2s;
    if (log2s > 5u) return fail(c, LAMA_HIP_E_INVALID, "the raster stride must be 1, 2, 4, 8, 16 or 32");
    if ((x0 & (stride - 1u)) || (y0 & (stride - 1u))) return fail(c, LAMA_HIP_E_INVALID, "the raster origin must be a multiple of the stride");
    if (width < 1u || height < 1u || width > 32768u || height > 32768u) return fail(c, LAMA_HIP_E_INVALID, "raster width and height must be 1 .. 32768 pixels");
    const size_t esize = layer == LAMA_HIP_RASTER_SQDIST ? 2 : 1, bytes = (size_t)width * height * esize;
    if (out_bytes != (uint64_t)bytes) return fail(c, LAMA_HIP_E_INVALID, "out_bytes is not width * height * element size");
    const bool dm = layer == LAMA_HIP_RASTER_SQDIST;
    if (c->h_counts[2 * particle + (dm ? 0 : 1)] == 0) {            // no patch at all (a context before its first scan has no window yet): every cell is absent
        if (dm) std::fill_n(static_cast<uint16_t*>(out), (size_t)width * height, (uint16_t)c->max_sqdist);
        else std::memset(out, 0xFF, bytes);
        return LAMA_HIP_OK;
    }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, c->d_raster.grow(bytes, (size_t)1 << 16));
    c->h_raster.reserve(bytes);
    const RasterBox box{x0, y0, width, height, stride, log2s};
    // the patch positions the box touches (its last cell may lie past 2^32 - 1: 64 bits)
    const uint64_t xe = (uint64_t)x0 + (uint64_t)width * stride - 1u, ye = (uint64_t)y0 + (uint64_t)height * stride - 1u;
    const dim3 grid((unsigned)((xe >> 5) - (x0 >> 5) + 1u), (unsigned)((ye >> 5) - (y0 >> 5) + 1u));
    const DevParams prm = make_params(c);
    uint8_t* const d_out = c->d_raster;
    if (layer == LAMA_HIP_RASTER_TRINARY) hipLaunchKernelGGL(k_raster<RASTER_TRINARY>, grid, dim3(256), 0, c->stream, prm, (int)particle, box, reinterpret_cast<int8_t*>(d_out));
    else if (layer == LAMA_HIP_RASTER_PROBABILITY) hipLaunchKernelGGL(k_raster<RASTER_PROBABILITY>, grid, dim3(256), 0, c->stream, prm, (int)particle, box, reinterpret_cast<int8_t*>(d_out));
    else hipLaunchKernelGGL(k_raster<RASTER_SQDIST>, grid, dim3(256), 0, c->stream, prm, (int)particle, box, reinterpret_cast<uint16_t*>(d_out));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_raster.data(), d_out, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(out, c->h_raster.data(), bytes);
    return LAMA_HIP_OK;
}

// ---- lama_frontier.h: the frontier clusters of a box of the occupancy map ----------------------------------------------------------
static_assert(sizeof(lama_hip_frontier) == 40 && sizeof(FrontierRec) == 40 && offsetof(lama_hip_frontier, sum_i) == offsetof(FrontierRec, sum_i) &&
              offsetof(lama_hip_frontier, max_j) == offsetof(FrontierRec, max_j), "FrontierRec is lama_hip_frontier");
int32_t lama_hip_map_frontiers(lama_hip_ctx* c, uint32_t particle, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, uint32_t stride,
                               uint32_t min_pixels, uint32_t cap, lama_hip_frontier* out, uint32_t* n, uint64_t* frontier_pixels, uint32_t* labels_out,
                               double* kernel_ms)
{
    if (!c) return LAMA_HIP_E_INVALID;
    ENTER(c);
    // ---- everything that can refuse the call comes before anything is written ----
    const char* const me = "lama_hip_map_frontiers: ";
    if (!n) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "n is NULL");
    if (!out && cap != 0u) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "out is NULL with cap != 0");
    if (particle >= c->P) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "particle out of range");
    uint32_t log2s = 0;
    while (log2s < 6u && (1u << log2s) != stride) ++log2s;
    if (log2s > 5u) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "the stride must be 1, 2, 4, 8, 16 or 32");
    if ((x0 & (stride - 1u)) || (y0 & (stride - 1u))) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "the origin must be a multiple of the stride");
    if (width < 1u || height < 1u || width > 32766u || height > 32766u) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "width and height must be 1 .. 32766 pixels");
    if ((uint64_t)width * height > (1ull << 28)) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "width * height must not exceed 2^28 pixels");
    if (min_pixels == 0u) min_pixels = 1u;
    const size_t npix = (size_t)width * height;
    if (c->h_counts[2 * particle + 1] == 0) {                       // no occupancy patch: nothing is free, so nothing is a frontier
        *n = 0;
        if (frontier_pixels) *frontier_pixels = 0;
        if (labels_out) std::memset(labels_out, 0xFF, npix * sizeof(uint32_t));
        if (kernel_ms) *kernel_ms = 0.0;
        return LAMA_HIP_OK;
    }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // the box widened by one pixel per side; a halo column / row whose cells would lie below 0 or above 2^32 - 1 does not exist
    // (x0 is a multiple of the stride, so x0 < stride means x0 == 0)
    FrontierBox fb;
    fb.width = width; fb.height = height;
    fb.ox = x0 >= stride ? 1u : 0u; fb.oy = y0 >= stride ? 1u : 0u;
    fb.has_right = (uint64_t)x0 + (uint64_t)width * stride <= 0xFFFFFFFFull ? 1u : 0u;
    fb.has_down = (uint64_t)y0 + (uint64_t)height * stride <= 0xFFFFFFFFull ? 1u : 0u;
    fb.rw = width + fb.ox + 1u; fb.rh = height + fb.oy + 1u;
    fb.sw = (width + 1u) >> 1; fb.nslots = fb.sw * ((height + 1u) >> 1);
    // [head 16 | widened raster, later the compacted slot list | sums and boxes 24 a slot | counts 4 a slot | L 4 a pixel]: 28 bytes per
    // 2 x 2 block, 4 per pixel and 1 per pixel of the widened box -- below 12 bytes per pixel of the widened box
    const size_t ras_bytes = ((size_t)fb.rw * fb.rh + 7u) & ~(size_t)7u;                       // (>= 4 * nslots: (w + 1)(h + 1) >= 4 ceil(w / 2) ceil(h / 2))
    const size_t o_ras = sizeof(FrontierHead), o_sums = o_ras + ras_bytes, o_cnt = o_sums + 24u * (size_t)fb.nslots, o_L = o_cnt + 4u * (size_t)fb.nslots;
    const size_t bytes = o_L + 4u * npix;
    HIPCHK(c, c->d_raster.grow(bytes, (size_t)1 << 16));
    uint8_t* const base = c->d_raster;
    FrontierHead* const d_head = reinterpret_cast<FrontierHead*>(base);
    int8_t* const d_ras = reinterpret_cast<int8_t*>(base + o_ras);
    uint32_t* const d_ids = reinterpret_cast<uint32_t*>(base + o_ras);
    unsigned long long* const d_sums = reinterpret_cast<unsigned long long*>(base + o_sums);
    const FrontierSlots st{d_sums, d_sums + fb.nslots, d_sums + 2u * (size_t)fb.nslots, reinterpret_cast<uint32_t*>(base + o_cnt)};
    uint32_t* const d_L = reinterpret_cast<uint32_t*>(base + o_L);
    const RasterBox box{x0 - fb.ox * stride, y0 - fb.oy * stride, fb.rw, fb.rh, stride, log2s};
    const uint64_t xe = (uint64_t)box.x0 + (uint64_t)box.width * stride - 1u, ye = (uint64_t)box.y0 + (uint64_t)box.height * stride - 1u;
    const dim3 rgrid((unsigned)((xe >> 5) - (box.x0 >> 5) + 1u), (unsigned)((ye >> 5) - (box.y0 >> 5) + 1u));
    const dim3 pgrid((unsigned)((npix + 255u) / 256u)), sgrid((fb.nslots + 255u) / 256u);
    const DevParams prm = make_params(c);
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, hipMemsetAsync(d_head, 0, sizeof(FrontierHead), c->stream));
    hipLaunchKernelGGL(k_raster<RASTER_TRINARY>, rgrid, dim3(256), 0, c->stream, prm, (int)particle, box, d_ras);
    hipLaunchKernelGGL(k_frontier_mark, pgrid, dim3(256), 0, c->stream, fb, (const int8_t*)d_ras, d_L, st, d_head);
    hipLaunchKernelGGL(k_frontier_merge, pgrid, dim3(256), 0, c->stream, fb, d_L);
    hipLaunchKernelGGL(k_frontier_reduce, pgrid, dim3(256), 0, c->stream, fb, d_L, st);
    hipLaunchKernelGGL(k_frontier_compact, sgrid, dim3(256), 0, c->stream, fb, st, min_pixels, d_head, d_ids);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->h_raster.reserve(sizeof(FrontierHead));
    HIPCHK(c, hipMemcpyAsync(c->h_raster.data(), d_head, sizeof(FrontierHead), hipMemcpyDeviceToHost, c->stream));
    if (labels_out) HIPCHK(c, hipMemcpyAsync(labels_out, d_L, 4u * npix, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    FrontierHead head;
    std::memcpy(&head, c->h_raster.data(), sizeof(head));
    float ms = 0, ms2 = 0;
    if (kernel_ms) HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    // the records of the kept clusters: a dense array sized by their number, sorted here (pixels descending, then label ascending)
    std::vector<FrontierRec> recs(head.n);
    if (head.n) {
        HIPCHK(c, c->d_frontier_rec.grow(head.n, 1024));
        FrontierRec* const d_rec = c->d_frontier_rec;
        HIPCHK(c, hipEventRecord(c->ev0, c->stream));
        hipLaunchKernelGGL(k_frontier_gather, dim3((head.n + 255u) / 256u), dim3(256), 0, c->stream, fb, (const uint32_t*)d_L, st, (const uint32_t*)d_ids, head.n, d_rec);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->ev1, c->stream));
        HIPCHK(c, hipMemcpyAsync(recs.data(), d_rec, sizeof(FrontierRec) * (size_t)head.n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (kernel_ms) HIPCHK(c, hipEventElapsedTime(&ms2, c->ev0, c->ev1));
        std::sort(recs.begin(), recs.end(), [](const FrontierRec& a, const FrontierRec& b) { return a.pixels != b.pixels ? a.pixels > b.pixels : a.label < b.label; });
    }
    *n = head.n;
    if (frontier_pixels) *frontier_pixels = head.pixels;
    if (kernel_ms) *kernel_ms = (double)ms + (double)ms2;
    if (out && head.n) std::memcpy(out, recs.data(), sizeof(FrontierRec) * (size_t)std::min(cap, head.n));
    return LAMA_HIP_OK;
}

// ---- lama_travel.h: the travel-cost field of a box, the best pixel near every goal and the path to it ------------------------------
static_assert(sizeof(lama_hip_route) == 16 && sizeof(TravelRoute) == 16 && offsetof(lama_hip_route, steps) == offsetof(TravelRoute, steps), "TravelRoute is lama_hip_route");
int32_t lama_hip_map_travel(lama_hip_ctx* c, uint32_t particle, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, uint32_t stride,
                            uint32_t clearance_cells, uint32_t prefer_cells, uint32_t near_factor, uint32_t num_sources, const uint32_t* sources_xy,
                            uint32_t num_goals, const uint32_t* goals_xy, uint32_t goal_reach, lama_hip_route* routes, uint32_t path_cap,
                            uint32_t* paths, uint32_t* field_out, uint32_t* rounds_out, double* kernel_ms)
{
    if (!c) return LAMA_HIP_E_INVALID;
    ENTER(c);
    // ---- everything that can refuse the call comes before anything is written ----
    const std::string me = "lama_hip_map_travel: ";
    if (particle >= c->P) return fail(c, LAMA_HIP_E_INVALID, me + "particle out of range");
    uint32_t log2s = 0;
    while (log2s < 6u && (1u << log2s) != stride) ++log2s;
    if (log2s > 5u) return fail(c, LAMA_HIP_E_INVALID, me + "the stride must be 1, 2, 4, 8, 16 or 32");
    if ((x0 & (stride - 1u)) || (y0 & (stride - 1u))) return fail(c, LAMA_HIP_E_INVALID, me + "the origin must be a multiple of the stride");
    if (width < 1u || height < 1u || width > 32768u || height > 32768u) return fail(c, LAMA_HIP_E_INVALID, me + "width and height must be 1 .. 32768 pixels");
    if (near_factor < 1u || near_factor > 64u) return fail(c, LAMA_HIP_E_INVALID, me + "near_factor must be 1 .. 64");
    if ((uint64_t)width * height * 7u * near_factor >= (1ull << 32)) return fail(c, LAMA_HIP_E_INVALID, me + "width * height * 7 * near_factor must stay below 2^32");
    if ((uint64_t)clearance_cells * clearance_cells > (uint64_t)c->max_sqdist)
        return fail(c, LAMA_HIP_E_INVALID, me + "clearance_cells^2 exceeds the distance map's max_sqdist: no pixel could be traversable");
    if (prefer_cells < clearance_cells || prefer_cells > 65535u) return fail(c, LAMA_HIP_E_INVALID, me + "prefer_cells must be clearance_cells .. 65535");
    if (goal_reach > 16u) return fail(c, LAMA_HIP_E_INVALID, me + "goal_reach must be 0 .. 16");
    if (num_sources == 0u || !sources_xy) return fail(c, LAMA_HIP_E_INVALID, me + "at least one source is needed");
    if (num_goals != 0u && (!goals_xy || !routes)) return fail(c, LAMA_HIP_E_INVALID, me + "goals_xy or routes is NULL with num_goals != 0");
    if (path_cap != 0u && num_goals != 0u && !paths) return fail(c, LAMA_HIP_E_INVALID, me + "paths is NULL with path_cap != 0");
    if ((uint64_t)num_goals * path_cap > (1ull << 28)) return fail(c, LAMA_HIP_E_INVALID, me + "num_goals * path_cap must not exceed 2^28");
    for (uint32_t k = 0; k < num_sources; ++k) {
        const uint32_t sx = sources_xy[2 * k], sy = sources_xy[2 * k + 1];
        if (sx < x0 || sy < y0 || ((sx - x0) >> log2s) >= width || ((sy - y0) >> log2s) >= height) return fail(c, LAMA_HIP_E_INVALID, me + "a source lies outside the box");
    }
    const bool has_dm = c->h_counts[2 * particle] != 0, has_occ = c->h_counts[2 * particle + 1] != 0, nothing = !has_dm && !has_occ;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    TravelBox tb;
    tb.x0 = x0; tb.y0 = y0; tb.width = width; tb.height = height; tb.log2s = log2s; tb.near_factor = near_factor;
    tb.tw = (width + 31u) >> 5; tb.th = (height + 31u) >> 5; tb.ntiles = tb.tw * tb.th;
    const size_t npix = (size_t)width * height, cap_all = (size_t)num_goals * path_cap;
    constexpr uint32_t HIST = 256;                                  // the rounds of one batch: their list lengths are read back together
    auto up16 = [](size_t v) { return (v + 15u) & ~(size_t)15u; };
    // [field 4 npix | sq raster 2 npix | occ raster npix | class npix | two flag arrays and the list 12 ntiles | list lengths | sources |
    //  goals | routes | ring | paths]
    const size_t o_F = 0, o_sq = o_F + up16(4u * npix), o_occ = o_sq + up16(2u * npix), o_cls = o_occ + up16(npix), o_flags = o_cls + up16(npix);
    const size_t o_list = o_flags + up16(8u * (size_t)tb.ntiles), o_hist = o_list + up16(4u * (size_t)tb.ntiles), o_src = o_hist + 4u * HIST;
    const size_t o_goal = o_src + up16(8u * (size_t)num_sources), o_route = o_goal + up16(8u * (size_t)num_goals), o_ring = o_route + up16(16u * (size_t)num_goals);
    const size_t o_path = o_ring + up16(4u * cap_all), bytes = o_path + up16(4u * cap_all);
    HIPCHK(c, c->d_travel.grow(bytes, (size_t)1 << 16));
    uint8_t* const base = c->d_travel;
    uint32_t* const d_F = reinterpret_cast<uint32_t*>(base + o_F);
    uint16_t* const d_sq = reinterpret_cast<uint16_t*>(base + o_sq);
    int8_t* const d_occ = reinterpret_cast<int8_t*>(base + o_occ);
    uint8_t* const d_cls = base + o_cls;
    uint32_t* const d_flags = reinterpret_cast<uint32_t*>(base + o_flags);
    uint32_t* const d_list = reinterpret_cast<uint32_t*>(base + o_list);
    uint32_t* const d_hist = reinterpret_cast<uint32_t*>(base + o_hist);
    uint32_t* const d_src = reinterpret_cast<uint32_t*>(base + o_src);
    uint32_t* const d_goal = reinterpret_cast<uint32_t*>(base + o_goal);
    TravelRoute* const d_route = reinterpret_cast<TravelRoute*>(base + o_route);
    uint32_t* const d_ring = reinterpret_cast<uint32_t*>(base + o_ring);
    uint32_t* const d_path = reinterpret_cast<uint32_t*>(base + o_path);
    // page-locked staging: [list lengths | sources, later routes | goals | paths]
    const size_t s_hist = 0, s_src = 4u * HIST, s_goal = s_src + std::max(up16(8u * (size_t)num_sources), up16(16u * (size_t)num_goals));
    const size_t s_path = s_goal + up16(8u * (size_t)num_goals);
    c->h_raster.reserve(s_path + 4u * cap_all);
    uint8_t* const hs = c->h_raster.data();
    std::memcpy(hs + s_src, sources_xy, 8u * (size_t)num_sources);
    if (num_goals) std::memcpy(hs + s_goal, goals_xy, 8u * (size_t)num_goals);
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_src, hs + s_src, 8u * (size_t)num_sources, hipMemcpyHostToDevice, c->stream));
    if (num_goals) HIPCHK(c, hipMemcpyAsync(d_goal, hs + s_goal, 8u * (size_t)num_goals, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_flags, 0, 8u * (size_t)tb.ntiles, c->stream));
    if (!nothing) {
        const RasterBox box{x0, y0, width, height, stride, log2s};
        const uint64_t xe = (uint64_t)x0 + (uint64_t)width * stride - 1u, ye = (uint64_t)y0 + (uint64_t)height * stride - 1u;
        const dim3 rgrid((unsigned)((xe >> 5) - (x0 >> 5) + 1u), (unsigned)((ye >> 5) - (y0 >> 5) + 1u));
        const DevParams prm = make_params(c);
        if (has_occ) hipLaunchKernelGGL(k_raster<RASTER_TRINARY>, rgrid, dim3(256), 0, c->stream, prm, (int)particle, box, d_occ);
        if (has_dm) hipLaunchKernelGGL(k_raster<RASTER_SQDIST>, rgrid, dim3(256), 0, c->stream, prm, (int)particle, box, d_sq);
    }
    hipLaunchKernelGGL(k_travel_classify, dim3((unsigned)((npix + 255u) / 256u)), dim3(256), 0, c->stream, tb, has_occ ? (const int8_t*)d_occ : (const int8_t*)nullptr,
                       has_dm ? (const uint16_t*)d_sq : (const uint16_t*)nullptr, (uint32_t)c->max_sqdist, clearance_cells * clearance_cells, prefer_cells * prefer_cells,
                       nothing ? 1 : 0, d_cls, d_F);
    hipLaunchKernelGGL(k_travel_seed, dim3((num_sources + 255u) / 256u), dim3(256), 0, c->stream, tb, num_sources, (const uint32_t*)d_src, d_F, d_flags);
    HIPCHK(c, hipGetLastError());
    // Rounds: compact the marked tiles, relax them; the marks for the next round go into the other flag array.  The host does not
    // know a round's list length when it launches it (the relax grid is sized for the box and workgroups beyond the list leave at
    // once), and learns only in batches whether the field has settled: a blocking read-back costs several launches' worth of time,
    // a round without a tile two nearly empty launches.  Batches double from 8 to 256 rounds, so at most as many empty rounds are
    // launched as rounds had run before, with log2 as many read-backs.  After round k every pixel whose best path crosses at most k
    // tile rims is final, so width * height + 1 rounds are the hard bound.
    c->travel_rounds = 0; c->travel_max_tiles = 0; c->travel_readbacks = 0; c->travel_tiles = 0;
    if (!nothing) {
        const uint64_t max_rounds = (uint64_t)npix + 1u;
        const dim3 cgrid((tb.ntiles + 255u) / 256u), xgrid(std::min(tb.ntiles, 2048u));
        uint64_t launched = 0;
        uint32_t batch = 8, cur = 0;
        for (bool settled = false; !settled;) {
            if (launched >= max_rounds) return fail(c, LAMA_HIP_E_STATE, me + "internal error: the field did not settle within width * height + 1 rounds");
            const uint32_t b = (uint32_t)std::min<uint64_t>(batch, max_rounds - launched);
            HIPCHK(c, hipMemsetAsync(d_hist, 0, 4u * (size_t)b, c->stream));
            for (uint32_t r = 0; r < b; ++r, cur ^= 1u) {
                hipLaunchKernelGGL(k_travel_compact, cgrid, dim3(256), 0, c->stream, tb.ntiles, d_flags + (size_t)cur * tb.ntiles, d_list, d_hist + r);
                hipLaunchKernelGGL(k_travel_relax, xgrid, dim3(256), 0, c->stream, tb, (const uint8_t*)d_cls, d_F, (const uint32_t*)d_list, (const uint32_t*)(d_hist + r),
                                   d_flags + (size_t)(cur ^ 1u) * tb.ntiles);
            }
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(hs + s_hist, d_hist, 4u * (size_t)b, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            ++c->travel_readbacks;
            const uint32_t* const hist = reinterpret_cast<const uint32_t*>(hs + s_hist);
            for (uint32_t r = 0; r < b && !settled; ++r) {
                if (hist[r] == 0u) { settled = true; break; }       // nothing was marked: every later round of the batch was empty too
                ++c->travel_rounds; c->travel_tiles += hist[r]; c->travel_max_tiles = std::max(c->travel_max_tiles, hist[r]);
            }
            launched += b;
            batch = std::min(batch * 2u, HIST);
        }
    }
    if (num_goals) {
        hipLaunchKernelGGL(k_travel_answer, dim3(num_goals), dim3(64), 0, c->stream, tb, num_goals, (const uint32_t*)d_goal, goal_reach, (const uint32_t*)d_F, d_route);
        hipLaunchKernelGGL(k_travel_trace, dim3(num_goals), dim3(64), 0, c->stream, tb, num_goals, (const uint8_t*)d_cls, (const uint32_t*)d_F, d_route, path_cap, d_ring, d_path);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    if (num_goals) HIPCHK(c, hipMemcpyAsync(hs + s_src, d_route, 16u * (size_t)num_goals, hipMemcpyDeviceToHost, c->stream));
    if (cap_all) HIPCHK(c, hipMemcpyAsync(hs + s_path, d_path, 4u * cap_all, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const TravelRoute* const got = reinterpret_cast<const TravelRoute*>(hs + s_src);
    for (uint32_t g = 0; g < num_goals; ++g)
        if (got[g].status == TRAVEL_BROKEN) return fail(c, LAMA_HIP_E_STATE, me + "internal error: a path left the field");
    // ---- nothing can fail the call any more except the field's copy: the outputs
    if (field_out) {
        HIPCHK(c, hipMemcpyAsync(field_out, d_F, 4u * npix, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    float ms = 0;
    if (kernel_ms) { HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1)); *kernel_ms = (double)ms; }
    if (rounds_out) *rounds_out = c->travel_rounds;
    if (num_goals) std::memcpy(routes, got, 16u * (size_t)num_goals);
    if (cap_all)
        for (uint32_t g = 0; g < num_goals; ++g)
            if (got[g].status == TRAVEL_REACHED)
                std::memcpy(paths + (size_t)g * path_cap, hs + s_path + 4u * (size_t)g * path_cap, 4u * (size_t)std::min<uint64_t>(path_cap, (uint64_t)got[g].steps + 1u));
    return LAMA_HIP_OK;
}

int32_t lama_hip_map_travel_stats(lama_hip_ctx* c, uint32_t* rounds, uint64_t* tiles_run, uint32_t* max_tiles, uint32_t* readbacks)
{
    if (!c) return LAMA_HIP_E_INVALID;
    if (rounds) *rounds = c->travel_rounds;
    if (tiles_run) *tiles_run = c->travel_tiles;
    if (max_tiles) *max_tiles = c->travel_max_tiles;
    if (readbacks) *readbacks = c->travel_readbacks;
    return LAMA_HIP_OK;
}

// ---- lama_raycast_query.h: the first cell of every beam that stops the ray ---------------------------------------------------------
namespace {
// One beam's start and hit cell as beam_geometry forms them without truncation, in double BEFORE the cast (Map::w2m casts: a value
// outside [0, 2^32) is undefined behaviour there) -> 0, or 1: a cell leaves the 32-bit range, 2: more than 8191 steps
int cast_beam_check(const lama_hip_ctx* c, const double* T, const double* pt)
{
    const double h[3] = {((T[0] * pt[0] + T[1] * pt[1]) + T[2] * pt[2]) + T[9], ((T[3] * pt[0] + T[4] * pt[1]) + T[5] * pt[2]) + T[10],
                         ((T[6] * pt[0] + T[7] * pt[1]) + T[8] * pt[2]) + T[11]};
    int64_t nn = 0;
    for (int a = 0; a < 3; ++a) {
        const double mh = (c->scale * h[a] + c->off) + 0.5, ms = (c->scale * T[9 + a] + c->off) + 0.5;
        if (!(mh >= 0.0) || !(mh < 4294967296.0) || !(ms >= 0.0) || !(ms < 4294967296.0)) return 1;
        const int64_t d = (int64_t)(uint32_t)mh - (int64_t)(uint32_t)ms;
        nn = std::max(nn, d < 0 ? -d : d);
    }
    return nn > 8191 ? 2 : 0;
}
} // namespace

int32_t lama_hip_map_cast_rays(lama_hip_ctx* c, uint32_t particle, int32_t kind, uint32_t num_poses, const double* poses4, const double* pts, uint32_t n,
                               const double* origin3, const double* quat, uint32_t flags, int32_t tolerance_cells, uint8_t* status, int32_t* step,
                               uint32_t* nn_out, uint32_t* cell_xy, uint32_t* end_sqdist, uint8_t* label, uint32_t* start_xy, double* kernel_ms)
{
    if (!c) return LAMA_HIP_E_INVALID;
    ENTER(c);
    // ---- everything that can refuse the call, before anything is uploaded or written
    const char* const me = "lama_hip_map_cast_rays: ";
    if (!status || !poses4 || !pts) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "status, poses4 or pts_xyz is NULL");
    if (n == 0 || num_poses == 0) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "no beam or no pose");
    if (particle >= c->P) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "particle out of range");
    if (kind != LAMA_HIP_MAP_DISTANCE && kind != LAMA_HIP_MAP_OCCUPANCY) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "unknown map kind");
    if (flags & ~(uint32_t)LAMA_HIP_RAY_STOP_UNKNOWN) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "unknown flag");
    if (kind == LAMA_HIP_MAP_DISTANCE && (flags & LAMA_HIP_RAY_STOP_UNKNOWN))
        return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "LAMA_HIP_RAY_STOP_UNKNOWN has no meaning on the distance map (a cell without a valid obstacle is not unknown)");
    const uint64_t total = (uint64_t)num_poses * n;
    if (total >= (1ull << 31)) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "num_poses * n must stay below 2^31");
    for (int k = 0; origin3 && k < 3; ++k) if (!std::isfinite(origin3[k])) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "the sensor origin is not finite");
    for (int k = 0; quat && k < 4; ++k) if (!std::isfinite(quat[k])) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "the sensor orientation is not finite");
    double r2 = 0.0;
    if (!scan_reach2(pts, n, true, r2)) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "the scan holds a non-finite point (filter NaN / inf ranges first, as iris_lama_ros does)");
    const Affine mtf = moving_tf(origin3, quat);
    const double reach = std::sqrt(r2);
    c->h_rq_tfs.resize(12 * (size_t)num_poses);
    for (uint32_t k = 0; k < num_poses; ++k) {
        double* const t = &c->h_rq_tfs[12 * (size_t)k];
        for (int j = 0; j < 4; ++j) if (!std::isfinite(poses4[4 * (size_t)k + j])) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "a pose is not finite");
        host_scan_tf(poses4 + 4 * (size_t)k, mtf, t);
        for (int j = 0; j < 12; ++j) if (!std::isfinite(t[j])) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "a pose or sensor transform is not finite");
        // Every hit lies within |row of R| * reach of the transform's translation on each axis: where that bound keeps all cells inside
        // the 32-bit range and below the step limit with two cells to spare, no beam of the pose needs a look; else each gets one.
        bool sure = true;
        for (int a = 0; a < 3; ++a) {
            const double row = std::sqrt(t[3 * a] * t[3 * a] + t[3 * a + 1] * t[3 * a + 1] + t[3 * a + 2] * t[3 * a + 2]) * reach;
            const double lo = c->scale * (t[9 + a] - row) + c->off, hi = c->scale * (t[9 + a] + row) + c->off;
            sure = sure && lo >= 2.0 && hi < 4294967290.0 && c->scale * row + 2.0 < 8191.0;
        }
        if (sure) continue;
        for (uint32_t i = 0; i < n; ++i) {
            const int bad = cast_beam_check(c, t, pts + 3 * (size_t)i);
            if (bad == 1) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "a start or hit cell leaves the 32-bit range of map cell coordinates");
            if (bad == 2) return fail(c, LAMA_HIP_E_WINDOW, std::string(me) + "a beam is longer than 8191 cells");
        }
    }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const size_t n_in = 3 * (size_t)n + 12 * (size_t)num_poses;
    // outputs, the widest first so that every array is aligned: cell_xy 8 | step 4 | nn 4 | end_sqdist 4 | status 1 | label 1 bytes a beam
    const size_t T64 = (size_t)total, o_cell = 0, o_step = 8 * T64, o_nn = 12 * T64, o_end = 16 * T64, o_status = 20 * T64, o_label = 21 * T64;
    HIPCHK(c, c->d_rq_in.grow(n_in, (size_t)1 << 14));
    HIPCHK(c, c->d_rq_out.grow(22 * T64, (size_t)1 << 16));
    double* const d_pts = c->d_rq_in; double* const d_tfs = d_pts + 3 * (size_t)n;
    uint8_t* const d_out = c->d_rq_out;
    HIPCHK(c, hipMemcpyAsync(d_pts, pts, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_tfs, c->h_rq_tfs.data(), sizeof(double) * 12 * (size_t)num_poses, hipMemcpyHostToDevice, c->stream));
    DevParams prm = make_params(c);
    prm.trunc_ray = 0.0; prm.trunc_range = 0.0;                    // the whole beam, as the map rebuild takes it
    const bool want_label = label && tolerance_cells >= 0;
    const CastOut out{d_out + o_status, step ? reinterpret_cast<int32_t*>(d_out + o_step) : nullptr, nn_out ? reinterpret_cast<uint32_t*>(d_out + o_nn) : nullptr,
                      cell_xy ? reinterpret_cast<uint32_t*>(d_out + o_cell) : nullptr, (end_sqdist || want_label) ? reinterpret_cast<uint32_t*>(d_out + o_end) : nullptr,
                      want_label ? d_out + o_label : nullptr};
    const dim3 grid((n + 255u) / 256u, std::min<uint32_t>(num_poses, 65535u));
    if (kernel_ms) HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    if (kind == LAMA_HIP_MAP_DISTANCE) hipLaunchKernelGGL(k_cast_rays<true>, grid, dim3(256), 0, c->stream, prm, (int)particle, (const double*)d_pts, n, (const double*)d_tfs, num_poses, flags, tolerance_cells, out);
    else hipLaunchKernelGGL(k_cast_rays<false>, grid, dim3(256), 0, c->stream, prm, (int)particle, (const double*)d_pts, n, (const double*)d_tfs, num_poses, flags, tolerance_cells, out);
    HIPCHK(c, hipGetLastError());
    if (kernel_ms) HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipMemcpyAsync(status, d_out + o_status, T64, hipMemcpyDeviceToHost, c->stream));
    if (step) HIPCHK(c, hipMemcpyAsync(step, d_out + o_step, 4 * T64, hipMemcpyDeviceToHost, c->stream));
    if (nn_out) HIPCHK(c, hipMemcpyAsync(nn_out, d_out + o_nn, 4 * T64, hipMemcpyDeviceToHost, c->stream));
    if (cell_xy) HIPCHK(c, hipMemcpyAsync(cell_xy, d_out + o_cell, 8 * T64, hipMemcpyDeviceToHost, c->stream));
    if (end_sqdist) HIPCHK(c, hipMemcpyAsync(end_sqdist, d_out + o_end, 4 * T64, hipMemcpyDeviceToHost, c->stream));
    if (want_label) HIPCHK(c, hipMemcpyAsync(label, d_out + o_label, T64, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (kernel_ms) { float ms = 0; HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1)); *kernel_ms = ms; }
    // the start cell of a pose's beams, w2m(tf.translation()): the same arithmetic as the device's w2m (checked above to be in range)
    for (uint32_t k = 0; start_xy && k < num_poses; ++k)
        for (int a = 0; a < 2; ++a) start_xy[2 * (size_t)k + a] = (uint32_t)((c->scale * c->h_rq_tfs[12 * (size_t)k + 9 + a] + c->off) + 0.5);
    return LAMA_HIP_OK;
}

static int32_t match_eval_impl(lama_hip_ctx* c, uint32_t particle, const double* pts, uint32_t n, const double* origin3, const double* quat,
                               const double* pose, double* residuals, double* jacobian, int cell_mode);
int32_t lama_hip_match_eval(lama_hip_ctx* c, uint32_t particle, const double* pts, uint32_t n, const double* origin3, const double* quat,
                            const double* pose, double* residuals, double* jacobian)
{
    return match_eval_impl(c, particle, pts, n, origin3, quat, pose, residuals, jacobian, 0);
}
int32_t lama_hip_match_cell_distances(lama_hip_ctx* c, uint32_t particle, const double* pts, uint32_t n, const double* origin3, const double* quat,
                                      const double* pose, double* distances)
{
    return match_eval_impl(c, particle, pts, n, origin3, quat, pose, distances, nullptr, 1);
}
static int32_t match_eval_impl(lama_hip_ctx* c, uint32_t particle, const double* pts, uint32_t n, const double* origin3, const double* quat,
                               const double* pose, double* residuals, double* jacobian, int cell_mode)
{
    if (!c || !pts || !pose || !residuals || n == 0 || particle >= c->P) return LAMA_HIP_E_INVALID;
    ENTER(c);
    if (!c->initialised) return fail(c, LAMA_HIP_E_STATE, "lama_hip_match_eval before a map exists");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int32_t rc = upload_scan(c, pts, n);
    if (rc) return rc;
    DevBuf<double> out, pose_in;                                    // (released in this order: pose_in, then out)
    HIPCHK(c, pose_in.alloc(4));
    HIPCHK(c, out.alloc(4 * (size_t)n));
    double* const d_pose = pose_in; double* const d_out = out;      // (launch arguments are plain pointers: the owners are not copied)
    HIPCHK(c, hipMemcpyAsync(d_pose, pose, sizeof(double) * 4, hipMemcpyHostToDevice, c->stream));
    const Affine mtf = moving_tf(origin3, quat);
    DevParams prm = make_params(c);
    hipLaunchKernelGGL(k_match_eval, dim3((n + 255) / 256), dim3(256), 0, c->stream, prm, (int)particle, c->d_pts, (int)n, mtf, d_pose, d_out,
                       jacobian ? d_out + n : nullptr, cell_mode);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(residuals, d_out, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    if (jacobian) HIPCHK(c, hipMemcpyAsync(jacobian, d_out + n, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LAMA_HIP_OK;
}

// ---- registration (lama_match_batch.h): B independent (map, scan, start pose) problems in one launch of k_match_solve_batch;
// lama_hip_match_solve / lama_hip_match_solve_with are a batch of one with the compile-time CauchyWeight(0.15)
constexpr int32_t MSB_CAUCHY015 = -1;      // (beside the LAMA_HIP_ROBUST_* kinds)

// the staging arrays of B problems (layout at lama_hip_ctx), in elements
struct MsbLayout {
    size_t out = 0, pose, mtf, pts, it = 0, st, prob, n_u32;
    explicit MsbLayout(size_t B) : pose(8 * B), mtf(12 * B), pts(24 * B), st(B), prob(2 * B), n_u32(6 * B) {}
};

static void stage_problem(lama_hip_ctx* c, const MsbLayout& L, size_t b, const double* pose4, const Affine& m, const MsbProblem& pb)
{
    std::memcpy(c->h_msb_f64.data() + L.pose + 4 * b, pose4, sizeof(double) * 4);
    double* q = c->h_msb_f64.data() + L.mtf + 12 * b;
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) q[3 * i + j] = m.R[i][j]; q[9 + i] = m.t[i]; }
    std::memcpy(c->h_msb_u32.data() + L.prob + 4 * b, &pb, sizeof(pb));
}

extern "C++" {
template <class WT>
static void launch_match_solve_batch(lama_hip_ctx* c, const DevParams& prm, uint32_t B, const MsbProblem* d_prob,
                                     const double* d_pts, const double* d_mtf, double* d_pose, double* d_out, int32_t* d_iters, uint32_t* d_status, WT wt)
{
    if (c->max_sqdist > (uint32_t)SM_LUT)
        hipLaunchKernelGGL((k_match_solve_batch<true, WT>), dim3(B), dim3(SM_BLOCK), 0, c->stream, prm, d_prob, d_pts, d_mtf, d_pose, d_out, d_iters, d_status, wt);
    else
        hipLaunchKernelGGL((k_match_solve_batch<false, WT>), dim3(B), dim3(SM_BLOCK), 0, c->stream, prm, d_prob, d_pts, d_mtf, d_pose, d_out, d_iters, d_status, wt);
}
}   // extern "C++"

// Uploads the first n_f64 staged doubles from the poses on (poses, mounts and, when the call staged them, its points) and the problem
// records, runs the BIGSQ x policy instantiation on the points at d_pts (NULL: the staged ones) and fetches {out8, poses} and
// {iterations, status} into the staging arrays.  A status word that is set makes the call LAMA_HIP_E_NUMERIC -- with `one_msg`, or,
// without one, with the count of such problems; the results are in the staging arrays either way.
static int32_t match_solve_staged(lama_hip_ctx* c, const DevParams& prm, uint32_t B, size_t n_f64, const double* d_pts, int32_t robust_kind,
                                  double wparam, const char* one_msg)
{
    const MsbLayout L(B);
    double* const hf = c->h_msb_f64.data(); uint32_t* const hu = c->h_msb_u32.data();
    HIPCHK(c, c->d_msb_f64.grow(n_f64, (size_t)1 << 14)); HIPCHK(c, c->d_msb_u32.grow(L.n_u32, (size_t)1 << 10));
    double* const df = c->d_msb_f64; uint32_t* const du = c->d_msb_u32;
    HIPCHK(c, hipMemcpyAsync(df + L.pose, hf + L.pose, sizeof(double) * (n_f64 - L.pose), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(du + L.prob, hu + L.prob, sizeof(uint32_t) * (L.n_u32 - L.prob), hipMemcpyHostToDevice, c->stream));
    const MsbProblem* const d_prob = reinterpret_cast<const MsbProblem*>(du + L.prob);
    int32_t* const d_it = reinterpret_cast<int32_t*>(du + L.it);
#define LAMA_MSB_LAUNCH(...) launch_match_solve_batch(c, prm, B, d_prob, d_pts ? d_pts : df + L.pts, df + L.mtf, df + L.pose, df + L.out, d_it, du + L.st, __VA_ARGS__)
    switch (robust_kind) {
    case MSB_CAUCHY015: LAMA_MSB_LAUNCH(WCauchy015{}); break;
    case LAMA_HIP_ROBUST_UNIT: LAMA_MSB_LAUNCH(WUnit{wparam}); break;
    case LAMA_HIP_ROBUST_TUKEY: LAMA_MSB_LAUNCH(WTukey{wparam}); break;
    case LAMA_HIP_ROBUST_TDIST: LAMA_MSB_LAUNCH(WTDist{wparam}); break;
    case LAMA_HIP_ROBUST_CAUCHY: LAMA_MSB_LAUNCH(WCauchy{wparam}); break;
    default: LAMA_MSB_LAUNCH(WHuber{wparam}); break;
    }
#undef LAMA_MSB_LAUNCH
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hf + L.out, df + L.out, sizeof(double) * 12 * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hu + L.it, du + L.it, sizeof(uint32_t) * 2 * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint32_t bad = 0, first_bad = 0;
    for (uint32_t b = B; b-- > 0;) if (hu[L.st + b]) { ++bad; first_bad = b; }
    if (bad && one_msg) return fail(c, LAMA_HIP_E_NUMERIC, one_msg);
    if (bad)
        return fail(c, LAMA_HIP_E_NUMERIC, "lama_hip_match_solve_batch: " + std::to_string(bad) + " of " + std::to_string(B) + " problems met a zero-norm unit complex (the first is problem " +
                                               std::to_string(first_bad) + "; status_out marks them); the other problems' results stand");
    return LAMA_HIP_OK;
}

// one problem on the resident scan (upload_scan).  strategy < 0, max_iterations == 0: the context's; do_solve == 0: evaluate only, the
// pose comes back as it went in
static int32_t match_solve_one(lama_hip_ctx* c, uint32_t particle, const double* pts, uint32_t n, const double* origin3, const double* quat,
                               double* pose_inout, double* out7, int32_t* iters_out, int32_t do_solve, int32_t strategy, uint32_t max_iterations)
{
    if (!c || !pts || !pose_inout || n == 0 || particle >= c->P) return LAMA_HIP_E_INVALID;
    ENTER(c);
    if (!c->initialised) return fail(c, LAMA_HIP_E_STATE, "lama_hip_match_solve before a map exists");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int32_t rc = upload_scan(c, pts, n);
    if (rc) return rc;
    const MsbLayout L(1);
    c->h_msb_f64.resize(L.pts); c->h_msb_u32.resize(L.n_u32);
    DevParams prm = make_params(c);
    if (strategy >= 0) prm.strategy = strategy;
    stage_problem(c, L, 0, pose_inout, moving_tf(origin3, quat), MsbProblem{particle, 0u, n, !do_solve ? 0u : max_iterations ? max_iterations : prm.max_iter});
    rc = match_solve_staged(c, prm, 1, L.pts, c->d_pts, MSB_CAUCHY015, 0.0, "unit complex number is (near) zero (SophusException in the reference)");
    if (rc == LAMA_HIP_OK || rc == LAMA_HIP_E_NUMERIC) std::memcpy(pose_inout, c->h_msb_f64.data() + L.pose, sizeof(double) * 4);
    if (rc) return rc;
    if (out7) std::memcpy(out7, c->h_msb_f64.data() + L.out, sizeof(double) * 7);
    if (iters_out) std::memcpy(iters_out, c->h_msb_u32.data() + L.it, sizeof(int32_t));
    return LAMA_HIP_OK;
}

int32_t lama_hip_match_solve(lama_hip_ctx* c, uint32_t particle, const double* pts, uint32_t n, const double* origin3, const double* quat,
                             double* pose_inout, double* out7, int32_t* iters_out, int32_t do_solve)
{
    return match_solve_one(c, particle, pts, n, origin3, quat, pose_inout, out7, iters_out, do_solve, -1, 0);
}

int32_t lama_hip_match_solve_with(lama_hip_ctx* c, uint32_t particle, const double* pts, uint32_t n, const double* origin3, const double* quat,
                                  double* pose_inout, double* out7, int32_t* iters_out, int32_t strategy, uint32_t max_iterations)
{
    if (strategy != 0 && strategy != 1) return LAMA_HIP_E_INVALID;
    return match_solve_one(c, particle, pts, n, origin3, quat, pose_inout, out7, iters_out, 1, strategy, max_iterations);
}

int32_t lama_hip_match_solve_batch(lama_hip_ctx* c, uint32_t B, const uint32_t* particles, const double* pts, const uint32_t* offs,
                                   const double* origins, const double* quats, double* poses, const uint32_t* max_iterations,
                                   int32_t strategy, int32_t robust_kind, double robust_param, double* out8, int32_t* iters_out, uint32_t* status_out)
{
    if (!c) return LAMA_HIP_E_INVALID;
    if (B == 0) return LAMA_HIP_OK;
    ENTER(c);
    // ---- everything that can refuse the call, before anything is uploaded
    if (!particles || !pts || !offs || !poses || !max_iterations || !out8 || !iters_out) return fail(c, LAMA_HIP_E_INVALID, "lama_hip_match_solve_batch: a required array is NULL");
    if (strategy != 0 && strategy != 1) return fail(c, LAMA_HIP_E_INVALID, "lama_hip_match_solve_batch: strategy is 0 (GaussNewton) or 1 (LevenbergMarquard)");
    if (!std::isfinite(robust_param))                     // (whichever form it comes in: the stored c_ of CauchyWeight(0) is an infinity)
        return fail(c, LAMA_HIP_E_INVALID, "lama_hip_match_solve_batch: the robust cost's parameter is not finite");
    // the constant the kernel's policy takes is the one the reference's class stores: formed here as its constructor forms it, or
    // (LAMA_HIP_ROBUST_STORED) handed over already formed
    const bool stored = (robust_kind & LAMA_HIP_ROBUST_STORED) != 0;
    robust_kind &= ~LAMA_HIP_ROBUST_STORED;
    double wparam = robust_param;
    switch (robust_kind) {
    case LAMA_HIP_ROBUST_UNIT: break;
    case LAMA_HIP_ROBUST_TUKEY:      // 1 - x^2 / b^2
        if (!stored) wparam = robust_param * robust_param;
        if (!(wparam > 0.0) || !std::isfinite(wparam)) return fail(c, LAMA_HIP_E_INVALID, "lama_hip_match_solve_batch: TukeyWeight(b) divides by b * b, which is zero (or overflows)");
        break;
    case LAMA_HIP_ROBUST_TDIST:      // (dof + 1) / (dof + x^2): zero divides at x = 0, a negative one at x^2 = -dof (and weighs negatively)
        if (!(robust_param > 0.0)) return fail(c, LAMA_HIP_E_INVALID, "lama_hip_match_solve_batch: TDistributionWeight(dof) needs dof > 0");
        break;
    case LAMA_HIP_ROBUST_CAUCHY:     // c_ = 1 / (param * param)
        if (!stored) wparam = 1.0 / (robust_param * robust_param);
        if (!std::isfinite(wparam) || wparam < 0.0) return fail(c, LAMA_HIP_E_INVALID, "lama_hip_match_solve_batch: CauchyWeight(param) divides by param * param, which is zero");
        break;
    case LAMA_HIP_ROBUST_HUBER:      // k / |x| for x >= k: zero gives 0 / 0 at x = 0, a negative one a negative weight everywhere
        if (!(robust_param > 0.0)) return fail(c, LAMA_HIP_E_INVALID, "lama_hip_match_solve_batch: HuberWeight(k) needs k > 0");
        break;
    default: return fail(c, LAMA_HIP_E_INVALID, "lama_hip_match_solve_batch: unknown robust cost");
    }
    for (uint32_t b = 0; b < B; ++b) {
        if (offs[b + 1] <= offs[b]) return fail(c, LAMA_HIP_E_INVALID, "lama_hip_match_solve_batch: problem " + std::to_string(b) + " has an empty (or decreasing) point slice");
        if (offs[b + 1] - offs[b] > 0x7FFFFFFFu) return fail(c, LAMA_HIP_E_INVALID, "lama_hip_match_solve_batch: more than 2^31 - 1 points in one problem");
        if (particles[b] >= c->P) return fail(c, LAMA_HIP_E_INVALID, "lama_hip_match_solve_batch: problem " + std::to_string(b) + " names a particle out of range");
        for (int k = 0; k < 4; ++k)
            if (!std::isfinite(poses[4 * (size_t)b + k])) return fail(c, LAMA_HIP_E_INVALID, "lama_hip_match_solve_batch: the start pose of problem " + std::to_string(b) + " is not finite");
        for (int k = 0; origins && k < 3; ++k)
            if (!std::isfinite(origins[3 * (size_t)b + k])) return fail(c, LAMA_HIP_E_INVALID, "lama_hip_match_solve_batch: the sensor origin of problem " + std::to_string(b) + " is not finite");
        for (int k = 0; quats && k < 4; ++k)
            if (!std::isfinite(quats[4 * (size_t)b + k])) return fail(c, LAMA_HIP_E_INVALID, "lama_hip_match_solve_batch: the sensor orientation of problem " + std::to_string(b) + " is not finite");
    }
    const size_t N = (size_t)offs[B] - offs[0];
    {
        const double* q = pts + 3 * (size_t)offs[0];
        double acc = 0.0;                                            // (a NaN or an infinity anywhere makes the sum of products with zero a NaN)
        for (size_t i = 0; i < 3 * N; ++i) acc += q[i] * 0.0;
        if (!(acc == 0.0)) return fail(c, LAMA_HIP_E_INVALID, "lama_hip_match_solve_batch: a scan holds a non-finite point (filter NaN / inf ranges first, as iris_lama_ros does)");
    }
    if (!c->initialised) return fail(c, LAMA_HIP_E_STATE, "lama_hip_match_solve_batch before a map exists");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // ---- staging: one array of doubles, one of words (layout at lama_hip_ctx)
    const MsbLayout L(B);
    const size_t n_f64 = L.pts + 3 * N;
    c->h_msb_f64.resize(n_f64); c->h_msb_u32.resize(L.n_u32);
    std::memcpy(c->h_msb_f64.data() + L.pts, pts + 3 * (size_t)offs[0], sizeof(double) * 3 * N);
    for (uint32_t b = 0; b < B; ++b)
        stage_problem(c, L, b, poses + 4 * (size_t)b, moving_tf(origins ? origins + 3 * (size_t)b : nullptr, quats ? quats + 4 * (size_t)b : nullptr),
                      MsbProblem{particles[b], offs[b] - offs[0], offs[b + 1] - offs[b], max_iterations[b]});
    DevParams prm = make_params(c);
    prm.strategy = strategy;
    const int32_t rc = match_solve_staged(c, prm, B, n_f64, nullptr, robust_kind, wparam, nullptr);
    if (rc && rc != LAMA_HIP_E_NUMERIC) return rc;
    const double* const hf = c->h_msb_f64.data(); const uint32_t* const hu = c->h_msb_u32.data();
    std::memcpy(out8, hf + L.out, sizeof(double) * 8 * B);
    std::memcpy(poses, hf + L.pose, sizeof(double) * 4 * B);
    std::memcpy(iters_out, hu + L.it, sizeof(int32_t) * B);
    if (status_out) std::memcpy(status_out, hu + L.st, sizeof(uint32_t) * B);
    return rc;
}

// ---- exhaustive pose-lattice search (lama_correlative.h): every heading's transform is formed HERE (libm, like every map update's),
// the kernel turns points into cells and sums stored squared distances
int32_t lama_hip_match_search_lattice(lama_hip_ctx* c, uint32_t particle, const double* pts, uint32_t n, const double* origin3, const double* quat,
                                      uint32_t point_step, const double* headings_cs, uint32_t H, double wx0, double wy0,
                                      uint32_t cell_step, uint32_t nx, uint32_t ny, uint32_t tile, uint64_t* best_out, uint32_t* scores_out)
{
    if (!c) return LAMA_HIP_E_INVALID;
    ENTER(c);
    // ---- everything that can refuse the call, before anything is uploaded
    const char* const me = "lama_hip_match_search_lattice: ";
    if (!pts || !headings_cs || !best_out) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "a required array is NULL");
    if (n == 0 || point_step == 0 || H == 0) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "no point, no heading, or a point step of 0");
    if (nx == 0 || ny == 0 || cell_step == 0 || tile == 0) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "nx, ny, cell_step and tile are at least 1");
    if (tile > 8u || tile * tile > (uint32_t)CS_NODES)
        return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "a tile holds at most " + std::to_string(CS_NODES) + " nodes (tile <= 8)");
    if (particle >= c->P) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "particle out of range");
    const uint64_t nodes = (uint64_t)nx * ny;
    if (nodes >= (1ull << 32) || nodes * H >= (1ull << 32)) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "the lattice has 2^32 nodes or more (a key carries a 32-bit index)");
    const uint32_t n_used = (n - 1u) / point_step + 1u;
    if ((uint64_t)n_used * c->max_sqdist >= (1ull << 32)) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "a score could exceed 32 bits (points used x max_sqdist); raise point_step");
    for (int k = 0; origin3 && k < 3; ++k) if (!std::isfinite(origin3[k])) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "the sensor origin is not finite");
    for (int k = 0; quat && k < 4; ++k) if (!std::isfinite(quat[k])) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "the sensor orientation is not finite");
    if (!std::isfinite(wx0) || !std::isfinite(wy0)) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "the lattice origin is not finite");
    for (size_t k = 0; k < 2 * (size_t)H; ++k) if (!std::isfinite(headings_cs[k])) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "a heading entry is not finite");
    double r2 = 0.0;
    if (!scan_reach2(pts, n, true, r2)) return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "the scan holds a non-finite point (filter NaN / inf ranges first, as iris_lama_ros does)");
    // no cell coordinate of any node may leave [0, 2^32): per heading, the hits lie within |row of R| * reach of the transform's
    // translation, and the far corner adds cell_step * (nx - 1, ny - 1) cells
    const Affine mtf = moving_tf(origin3, quat);
    const double reach = std::sqrt(r2);
    c->h_cs_tfs.resize(12 * (size_t)H);
    for (uint32_t h = 0; h < H; ++h) {
        const double pose4[4] = {headings_cs[2 * (size_t)h], headings_cs[2 * (size_t)h + 1], wx0, wy0};
        double* const t = &c->h_cs_tfs[12 * (size_t)h];
        host_scan_tf(pose4, mtf, t);
        for (int a = 0; a < 2; ++a) {
            const double row = std::sqrt(t[3 * a] * t[3 * a] + t[3 * a + 1] * t[3 * a + 1] + t[3 * a + 2] * t[3 * a + 2]) * reach;
            const double lo = c->scale * (t[9 + a] - row) + c->off, hi = c->scale * (t[9 + a] + row) + c->off + 1.0 + (double)cell_step * (double)((a == 0 ? nx : ny) - 1u);
            if (!(lo >= 0.0) || !(hi < 4294967295.0))
                return fail(c, LAMA_HIP_E_INVALID, std::string(me) + "the lattice, with the scan's reach around it, leaves the 32-bit range of map cell coordinates");
        }
    }
    if (!c->initialised) return fail(c, LAMA_HIP_E_STATE, "lama_hip_match_search_lattice before a map exists");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const int32_t rc = upload_scan(c, pts, n);
    if (rc) return rc;
    const uint32_t tiles_x = (nx - 1u) / tile + 1u, tiles_y = (ny - 1u) / tile + 1u;
    const uint64_t total = (uint64_t)tiles_x * tiles_y * H;
    HIPCHK(c, c->d_cs_tfs.grow(12 * (size_t)H, 12 * 128));
    HIPCHK(c, c->d_cs_best.grow(total, (size_t)1 << 12));
    DevBuf<uint32_t> scores;                                        // (only a caller who asks for every score pays for them)
    if (scores_out) HIPCHK(c, scores.alloc(nodes * H));
    double* const d_tfs = c->d_cs_tfs; uint64_t* const d_best = c->d_cs_best; uint32_t* const d_scores = scores;
    HIPCHK(c, hipMemcpyAsync(d_tfs, c->h_cs_tfs.data(), sizeof(double) * 12 * (size_t)H, hipMemcpyHostToDevice, c->stream));
    const DevParams prm = make_params(c);
    hipLaunchKernelGGL(k_search_lattice, dim3((unsigned)std::min<uint64_t>(total, (uint64_t)1 << 20)), dim3(CS_BLOCK), 0, c->stream, prm, (int)particle,
                       (const double*)c->d_pts, n_used, point_step, (const double*)d_tfs, cell_step, nx, ny, tile, tiles_x, tiles_y, total, d_best, d_scores);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(best_out, d_best, sizeof(uint64_t) * total, hipMemcpyDeviceToHost, c->stream));
    if (scores_out) HIPCHK(c, hipMemcpyAsync(scores_out, d_scores, sizeof(uint32_t) * nodes * H, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LAMA_HIP_OK;
}

// Particle blob layout: [pose 4 f64][header 8 i32][dm_dir][occ_dir][dm_sv used][dm_obs used][dm_mask used][occ used][occ_mask used]
// (the directories in the SENDER's window side W: windows grow independently, the header carries the side)
static uint64_t blob_bytes_w(uint64_t W, int dmc, int occ)
{
    return 32 + 32 + 2 * W * W * 2 + (uint64_t)dmc * (SV_PATCH_BYTES + 4096 + 128) + (uint64_t)occ * (4096 + 128);
}
static uint64_t blob_bytes(const lama_hip_ctx* c, int dmc, int occ) { return blob_bytes_w(c->W, dmc, occ); }

// the extent of this context's mapped box inside its window (lo | hi << 16 in patches; the whole window when nothing is known)
static int32_t mapped_box_rel(const lama_hip_ctx* c, int axis)
{
    const int64_t o = (axis == 0 ? c->wx0 : c->wy0) >> 5, W = c->W;
    int64_t lo = 0, hi = W - 1;
    if (c->mb_valid) { lo = std::min(std::max((axis == 0 ? c->mbx0 : c->mby0) - o, (int64_t)0), W - 1); hi = std::min(std::max((axis == 0 ? c->mbx1 : c->mby1) - o, (int64_t)0), W - 1); }
    return (int32_t)((uint32_t)lo | ((uint32_t)hi << 16));
}

// ---- particle shipping: all outgoing / incoming particles of a resample in one launch each (k_export_particles / k_import_particles)
static int32_t upload_ship_desc(lama_hip_ctx* c, uint32_t n)
{
    if ((size_t)BLOB_HEAD * n > c->d_ship_heads.n) {               // (allocated last: its count is the capacity of both)
        c->d_ship_desc.reset(); c->d_ship_heads.reset();
        const size_t cap = std::max<uint32_t>(n, 64u);
        HIPCHK(c, c->d_ship_desc.alloc(cap));
        HIPCHK(c, c->d_ship_heads.alloc((size_t)BLOB_HEAD * cap));
    }
    HIPCHK(c, hipMemcpyAsync(c->d_ship_desc, c->h_ship_desc.data(), sizeof(ShipDesc) * n, hipMemcpyHostToDevice, c->stream));
    return LAMA_HIP_OK;
}

int32_t lama_hip_pf_export_particles(lama_hip_ctx* c, uint32_t n, const uint32_t* particles, void* const* bufs, const uint64_t* caps, uint64_t* bytes)
{
    if (!c || (n && !particles)) return LAMA_HIP_E_INVALID;
    ENTER(c);
    if (!c->initialised) return fail(c, LAMA_HIP_E_STATE, "export before init");
    bool sizes_only = bufs == nullptr;
    for (uint32_t k = 0; k < n; ++k) {
        if (particles[k] >= c->P) return LAMA_HIP_E_INVALID;
        const uint64_t need = blob_bytes(c, c->h_counts[2 * particles[k]], c->h_counts[2 * particles[k] + 1]);
        if (bytes) bytes[k] = need;
        if (!sizes_only && (!bufs[k] || !caps || caps[k] < need)) return fail(c, LAMA_HIP_E_INVALID, "export buffer missing or too small");
    }
    if (sizes_only || n == 0) return LAMA_HIP_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    c->h_ship_desc.resize(n);
    for (uint32_t k = 0; k < n; ++k) c->h_ship_desc[k] = ShipDesc{(uint8_t*)bufs[k], particles[k], 0, 0, 0};
    const int32_t rc = upload_ship_desc(c, n);
    if (rc) return rc;
    hipLaunchKernelGGL(k_export_particles, dim3(n, 7, SHIP_SPLIT), dim3(256), 0, c->stream, make_params(c), (const ShipDesc*)c->d_ship_desc,
                       (const double*)c->d_poses, (int32_t)(c->wx0 >> 5), (int32_t)(c->wy0 >> 5),
                       (int32_t)c->visit_bound, mapped_box_rel(c, 0), mapped_box_rel(c, 1));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LAMA_HIP_OK;
}

int32_t lama_hip_pf_export_particle(lama_hip_ctx* c, uint32_t particle, void* buf, uint64_t cap, uint64_t* bytes)
{
    if (!buf) return lama_hip_pf_export_particles(c, 1, &particle, nullptr, nullptr, bytes);
    void* b1 = buf;
    return lama_hip_pf_export_particles(c, 1, &particle, &b1, &cap, bytes);
}

int32_t lama_hip_pf_import_particles(lama_hip_ctx* c, uint32_t n, const uint32_t* particles, const void* const* bufs, const uint64_t* bytes)
{
    if (!c || (n && (!particles || !bufs || !bytes))) return LAMA_HIP_E_INVALID;
    ENTER(c);
    if (!c->initialised) return fail(c, LAMA_HIP_E_STATE, "import before init");
    if (n == 0) return LAMA_HIP_OK;
    for (uint32_t k = 0; k < n; ++k) if (particles[k] >= c->P || !bufs[k] || bytes[k] < (uint64_t)BLOB_HEAD) return LAMA_HIP_E_INVALID;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    c->early_ok = false; c->ll_valid = false;                       // other particles sit in these slots now
    // 1. what is coming: the blobs' heads in one copy
    c->h_ship_desc.resize(n);
    for (uint32_t k = 0; k < n; ++k) c->h_ship_desc[k] = ShipDesc{(uint8_t*)const_cast<void*>(bufs[k]), particles[k], 0, 0, 0};
    int32_t rc = upload_ship_desc(c, n);
    if (rc) return rc;
    hipLaunchKernelGGL(k_gather_blob_heads, dim3(n), dim3(64), 0, c->stream, (const ShipDesc*)c->d_ship_desc, n, c->d_ship_heads);
    c->h_ship_heads.resize((size_t)BLOB_HEAD * n);
    HIPCHK(c, hipMemcpyAsync(c->h_ship_heads.data(), c->d_ship_heads, (size_t)BLOB_HEAD * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint32_t max_dm = 0, max_occ = 0;
    for (uint32_t k = 0; k < n; ++k) {
        int32_t hdr[8];
        std::memcpy(hdr, c->h_ship_heads.data() + (size_t)BLOB_HEAD * k + 32, 32);
        if (hdr[0] < 0 || hdr[1] < 0 || hdr[0] > 32767 || hdr[1] > 32767 || hdr[5] < 8 || hdr[5] > (int32_t)LAMA_HIP_MAX_WINDOW || (hdr[5] & 7) ||
            blob_bytes_w((uint64_t)hdr[5], hdr[0], hdr[1]) != bytes[k])
            return fail(c, LAMA_HIP_E_INVALID, "particle blob does not match this context's geometry");
        max_dm = std::max<uint32_t>(max_dm, (uint32_t)hdr[0]); max_occ = std::max<uint32_t>(max_occ, (uint32_t)hdr[1]);
        // every shard's window follows (and grows with) its own particles: this one must hold what the sender has mapped
        const int64_t sx = hdr[2], sy = hdr[3];
        rc = ensure_window(c, sx + (hdr[6] & 0xFFFF), sx + ((uint32_t)hdr[6] >> 16), sy + (hdr[7] & 0xFFFF), sy + ((uint32_t)hdr[7] >> 16));
        if (rc) return rc;
    }
    for (uint32_t k = 0; k < n; ++k) {
        int32_t hdr[8];
        std::memcpy(hdr, c->h_ship_heads.data() + (size_t)BLOB_HEAD * k + 32, 32);
        // the sender's window sits elsewhere: the kernel translates the directories
        c->h_ship_desc[k].wdx = (int32_t)((int64_t)(c->wx0 >> 5) - (int64_t)hdr[2]);
        c->h_ship_desc[k].wdy = (int32_t)((int64_t)(c->wy0 >> 5) - (int64_t)hdr[3]);
    }
    {   // every destination region must hold what its incoming particle brings (the sender's maps may have grown before ours)
        std::vector<CapRequest> reqs;
        for (uint32_t k = 0; k < n; ++k) {
            int32_t hdr[8];
            std::memcpy(hdr, c->h_ship_heads.data() + (size_t)BLOB_HEAD * k + 32, 32);
            const HostPart& pr = c->h_part[particles[k]];
            const uint32_t nd = want_capacity(c->floor_dm, (uint32_t)hdr[0], 0u), no = want_capacity(c->floor_occ, (uint32_t)hdr[1], 0u);
            if ((uint32_t)hdr[0] > pr.dm_cap || (uint32_t)hdr[1] > pr.occ_cap) reqs.push_back(CapRequest{particles[k], std::max(nd, pr.dm_cap), std::max(no, pr.occ_cap)});
        }
        (void)max_dm; (void)max_occ;
        if (!reqs.empty()) { rc = set_capacities(c, reqs); if (rc) return rc; }
    }
    // 2. the copies
    rc = upload_ship_desc(c, n);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_oldcounts, c->ms.counts, sizeof(int32_t) * 2 * c->P, hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(k_import_particles, dim3(n, 7, SHIP_SPLIT), dim3(256), 0, c->stream, make_params(c), (const ShipDesc*)c->d_ship_desc, (const int32_t*)c->d_oldcounts,
                       c->d_poses, c->d_err);
    HIPCHK(c, hipGetLastError());
    // the import itself reports what it could not place (a patch of the sender's window outside this one: ERR_WINDOW) -- not the
    // next, unrelated call on the context
    { const int32_t ri = check_device_errors(c); if (ri) return ri; }
    // 3. host mirrors
    for (uint32_t k = 0; k < n; ++k) {
        const uint8_t* head = c->h_ship_heads.data() + (size_t)BLOB_HEAD * k;
        int32_t hdr[8];
        std::memcpy(hdr, head + 32, 32);
        const uint32_t i = particles[k];
        std::memcpy(&c->h_poses[4 * i], head, 32);
        c->h_counts[2 * i] = hdr[0]; c->h_counts[2 * i + 1] = hdr[1];
        // the wrap guard's bound must hold for the counters this particle brings (they may be far above this context's own)
        c->visit_bound = std::max<uint32_t>(c->visit_bound, (uint32_t)std::min<int32_t>(std::max<int32_t>(hdr[4], 0), 65535));
    }
    return LAMA_HIP_OK;
}

int32_t lama_hip_pf_import_particle(lama_hip_ctx* c, uint32_t particle, const void* buf, uint64_t bytes)
{
    const void* b1 = buf;
    return lama_hip_pf_import_particles(c, 1, &particle, &b1, &bytes);
}

int32_t lama_hip_blob_alloc(lama_hip_ctx* c, uint64_t bytes, void** buf)
{
    if (!c || !buf || bytes == 0) return LAMA_HIP_E_INVALID;
    *buf = nullptr;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipMalloc(buf, bytes));
    return LAMA_HIP_OK;
}

int32_t lama_hip_blob_free(lama_hip_ctx* c, void* buf)
{
    if (!c) return LAMA_HIP_E_INVALID;
    if (!buf) return LAMA_HIP_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipFree(buf));
    return LAMA_HIP_OK;
}

// Peer access between two devices, enabled once per ordered pair and process: without it hipMemcpyPeerAsync is
// staged through host memory by the runtime instead of going GPU to GPU over xGMI.  Returns 1 when BOTH directions are enabled.
static int peer_access_between(int a, int b)
{
    // (the shards of a multi-GPU object copy concurrently, a host thread each: the table is shared by all of them)
    static std::mutex mu;
    static std::map<std::pair<int, int>, int> state;
    std::lock_guard<std::mutex> lock(mu);
    int prev_dev = -1;
    (void)hipGetDevice(&prev_dev);
    auto one_way = [&](int from, int to) -> int {
        const auto key = std::make_pair(from, to);
        auto it = state.find(key);
        if (it != state.end()) return it->second;
        int can = 0, ok = 0;
        if (hipDeviceCanAccessPeer(&can, from, to) == hipSuccess && can) {
            if (hipSetDevice(from) == hipSuccess) {
                const hipError_t e = hipDeviceEnablePeerAccess(to, 0);
                ok = (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) ? 1 : 0;
                if (!ok) (void)hipGetLastError();
            }
        } else (void)hipGetLastError();
        state[key] = ok;
        return ok;
    };
    const int ab = one_way(a, b), ba = one_way(b, a);
    if (prev_dev >= 0) (void)hipSetDevice(prev_dev);              // enabling access switches the calling thread's device
    return ab && ba;
}

int32_t lama_hip_blob_copy(lama_hip_ctx* dc, void* dst, lama_hip_ctx* sc, const void* src, uint64_t bytes)
{
    if (!dc || !sc || !dst || !src) return LAMA_HIP_E_INVALID;
    if (bytes == 0) return LAMA_HIP_OK;
    if (dc->cfg.device == sc->cfg.device) {
        HIPCHK(dc, hipSetDevice(dc->cfg.device));
        HIPCHK(dc, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, dc->stream));
        HIPCHK(dc, hipStreamSynchronize(dc->stream));
        return LAMA_HIP_OK;
    }
    // two devices: peer access first (queried and enabled once per pair), then the copy on the destination's stream; without peer
    // access the same call still works -- the runtime stages it -- and the counters say so (peer_access = 0)
    const int peer = peer_access_between(dc->cfg.device, sc->cfg.device);
    dc->ctr.peer_access = (uint32_t)peer;      // (the destination's own counter only: its thread is the caller; the source learns the value when it is a destination)
    HIPCHK(dc, hipSetDevice(dc->cfg.device));
    hipEvent_t e0 = dc->ev0, e1 = dc->ev1;
    HIPCHK(dc, hipEventRecord(e0, dc->stream));
    HIPCHK(dc, hipMemcpyPeerAsync(dst, dc->cfg.device, src, sc->cfg.device, bytes, dc->stream));      // GPU to GPU over xGMI
    HIPCHK(dc, hipEventRecord(e1, dc->stream));
    HIPCHK(dc, hipStreamSynchronize(dc->stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) { dc->ctr.peer_copy_ms += ms; dc->ctr.peer_copy_bytes += bytes; }
    return LAMA_HIP_OK;
}

// profiling builds only (-DLAMA_PROFILE_BF): per-particle cycle counters of the last k_brushfire launch
int32_t lama_hip_debug_cycles(lama_hip_ctx* c, uint64_t* out /* P x 8 */)
{
    if (!c || !out) return LAMA_HIP_E_INVALID;
    ENTER(c);
    HIPCHK(c, hipMemcpy(out, c->d_dbg, sizeof(uint64_t) * 8 * c->P, hipMemcpyDeviceToHost));
    return LAMA_HIP_OK;
}

// second block of developer counters (-DLAMA_PROFILE_LSE): kernel-level timestamps of k_brushfire per particle
int32_t lama_hip_debug_cycles2(lama_hip_ctx* c, uint64_t* out /* P x 8 */)
{
    if (!c || !out) return LAMA_HIP_E_INVALID;
    ENTER(c);
    HIPCHK(c, hipMemcpy(out, c->d_dbg + 8 * (size_t)c->P, sizeof(uint64_t) * 8 * c->P, hipMemcpyDeviceToHost));
    return LAMA_HIP_OK;
}

// developer event log of particle 0 (-DLAMA_PROFILE_LSE): out[0] = number of words, then (event << 56 | timestamp) words
int32_t lama_hip_debug_log(lama_hip_ctx* c, uint64_t* out /* 131072 words */)
{
    if (!c || !out) return LAMA_HIP_E_INVALID;
    ENTER(c);
    HIPCHK(c, hipMemcpy(out, c->d_dbg + 16 * (size_t)c->P, 1u << 20, hipMemcpyDeviceToHost));
    return LAMA_HIP_OK;
}

#if defined(LAMA_KC_PROBE) || (defined(LAMA_KC_OLD) && LAMA_KC_OLD == 4)
// experiment build only (tools/kc_probe.py): out[0] = number of mismatches logged by kc_probe (lama_dev.h), then 64 x 8 words; clears the log
int32_t lama_hip_debug_kc_probe(uint64_t* out /* 1 + 512 words */)
{
    uint32_t n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(lama_dev::g_kc_n), sizeof(n)) != hipSuccess) return LAMA_HIP_E_HIP;
    out[0] = n;
    if (hipMemcpyFromSymbol(out + 1, HIP_SYMBOL(lama_dev::g_kc_ev), sizeof(uint64_t) * 512) != hipSuccess) return LAMA_HIP_E_HIP;
    n = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(lama_dev::g_kc_n), &n, sizeof(n)) != hipSuccess) return LAMA_HIP_E_HIP;
    return LAMA_HIP_OK;
}
#endif

// device memory the context holds: the maps (pools + directories), of which used, and everything
static void memory_figures(const lama_hip_ctx* c, lama_hip_counters* o)
{
    const MapStore& m = c->ms;
    const uint64_t P = c->P, WW = (uint64_t)c->W * c->W;
    const uint64_t dirs = 2 * P * WW * 2;
    uint64_t dm_used = 0, occ_used = 0;
    for (uint32_t p = 0; p < c->P; ++p) { dm_used += (uint64_t)c->h_counts[2 * p]; occ_used += (uint64_t)c->h_counts[2 * p + 1]; }
    uint64_t dm_pool = 0, occ_pool = 0;
    for (const PoolChunk& k : m.dm_chunks) dm_pool += k.patches;
    for (const PoolChunk& k : m.occ_chunks) occ_pool += k.patches;
    o->hbm_bytes_allocated = dirs + dm_pool * (SV_PATCH_BYTES + 4096 + 128) + occ_pool * (4096 + 128 + 128 + 4);
    o->hbm_bytes_used = dirs + dm_used * (SV_PATCH_BYTES + 4096 + 128) + occ_used * (4096 + 128 + 128 + 4);
    const uint64_t other = 2 * P * (uint64_t)c->cfg.queue_capacity * 8 + P * (uint64_t)c->cfg.active_capacity * 8 + (uint64_t)c->d_rrec.n * (sizeof(lama_dev::RayRec) + 8) +
                           P * (16 * 8 + 12 * 8 + 4 * 8 + 64) + (1u << 20) + (uint64_t)c->d_pts.bytes();
    o->hbm_bytes_total = o->hbm_bytes_allocated + other;
}

int32_t lama_hip_get_counters(lama_hip_ctx* c, lama_hip_counters* out)
{
    if (!c || !out) return LAMA_HIP_E_INVALID;
    ENTER(c);
    *out = c->ctr;
    memory_figures(c, out);
    out->struct_bytes = (uint32_t)sizeof(lama_hip_counters);
    return LAMA_HIP_OK;
}

uint32_t lama_hip_counters_bytes(void) { return (uint32_t)sizeof(lama_hip_counters); }

int32_t lama_hip_get_counters_sized(lama_hip_ctx* c, void* out, uint32_t bytes)
{
    if (!c || !out) return LAMA_HIP_E_INVALID;
    lama_hip_counters full;
    const int32_t rc = lama_hip_get_counters(c, &full);
    if (rc) return rc;
    std::memcpy(out, &full, std::min<size_t>(bytes, sizeof(full)));
    return LAMA_HIP_OK;
}

int32_t lama_hip_reset_counters(lama_hip_ctx* c)
{
    if (!c) return LAMA_HIP_E_INVALID;
    ENTER(c);
    const lama_hip_counters old = c->ctr;
    std::memset(&c->ctr, 0, sizeof(c->ctr));
    c->ctr.dm_patches = old.dm_patches; c->ctr.occ_patches = old.occ_patches;
    c->ctr.brushfire_mode = old.brushfire_mode; c->ctr.brushfire_waves = old.brushfire_waves;
    c->ctr.window_patches = c->W; c->ctr.peer_access = old.peer_access;
    return LAMA_HIP_OK;
}

} // extern "C"
