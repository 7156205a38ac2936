// travel_host_path.cpp -- the HOST path tools/travel_bench.py compares lama_hip_map_travel with: what a caller had before the entry
// point existed, once the two dense grids are down -- classify the pixels, run Dijkstra with a binary heap over the move rules of
// include/lama_hip.h on one core, pick every goal's answer and walk its path back.  Plain C++, no device code; built by the tool
// (g++ -O2 -shared) and used by nothing else.
#include <cstdint>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

namespace {
constexpr uint32_t NONE = 0xFFFFFFFFu;
const int DI[8] = {-1, 0, 1, -1, 1, -1, 0, 1}, DJ[8] = {-1, -1, -1, 0, 0, 1, 1, 1};      // ascending pixel index
}

// occ: int8 trinary grid or NULL (a distance-only map); sq: uint16 squared distances; src / goal: pixel indices (goal NONE: outside).
// field [h][w] and routes [ng][4] {status, pixel, cost, steps} are written; the return value is the number of heap pops.
extern "C" uint64_t travel_host_path(const int8_t* occ, const uint16_t* sq, uint32_t w, uint32_t h, uint32_t clearance, uint32_t prefer, uint32_t near_factor,
                                     uint32_t ns, const uint32_t* src, uint32_t ng, const uint32_t* goal, uint32_t reach, uint32_t* field, uint32_t* routes)
{
    const size_t n = (size_t)w * h;
    std::vector<uint8_t> pass(n), near(n);
    for (size_t k = 0; k < n; ++k) {
        pass[k] = (!occ || occ[k] == 0) && (uint32_t)sq[k] >= clearance * clearance;
        near[k] = (uint32_t)sq[k] < prefer * prefer;
    }
    for (size_t k = 0; k < n; ++k) field[k] = NONE;
    typedef std::pair<uint32_t, uint32_t> Item;                     // cost, pixel
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    for (uint32_t k = 0; k < ns; ++k) { field[src[k]] = 0; heap.push(Item(0u, src[k])); }
    auto legal = [&](int pi, int pj, int qi, int qj) {
        if (!pass[(size_t)qj * w + qi]) return false;
        return pi == qi || pj == qj || (pass[(size_t)pj * w + qi] && pass[(size_t)qj * w + pi]);
    };
    uint64_t pops = 0;
    while (!heap.empty()) {
        const Item it = heap.top();
        heap.pop();
        ++pops;
        if (it.first > field[it.second]) continue;
        const int i = (int)(it.second % w), j = (int)(it.second / w);
        for (int d = 0; d < 8; ++d) {
            const int a = i + DI[d], b = j + DJ[d];
            if (a < 0 || b < 0 || a >= (int)w || b >= (int)h || !legal(i, j, a, b)) continue;
            const size_t q = (size_t)b * w + a;
            const uint32_t nd = it.first + ((DI[d] && DJ[d]) ? 7u : 5u) * (near[q] ? near_factor : 1u);
            if (nd < field[q]) { field[q] = nd; heap.push(Item(nd, (uint32_t)q)); }
        }
    }
    for (uint32_t g = 0; g < ng; ++g) {
        uint32_t* r = routes + 4 * g;
        r[0] = 2; r[1] = NONE; r[2] = NONE; r[3] = 0;
        if (goal[g] == NONE) continue;
        const int gi = (int)(goal[g] % w), gj = (int)(goal[g] / w);
        uint32_t best = NONE, at = NONE;
        for (int b = gj - (int)reach < 0 ? 0 : gj - (int)reach; b <= gj + (int)reach && b < (int)h; ++b)
            for (int a = gi - (int)reach < 0 ? 0 : gi - (int)reach; a <= gi + (int)reach && a < (int)w; ++a)
                if (field[(size_t)b * w + a] < best) { best = field[(size_t)b * w + a]; at = (uint32_t)((size_t)b * w + a); }
        r[0] = best == NONE ? 1u : 0u;
        if (best == NONE) continue;
        r[1] = at; r[2] = best;
        uint32_t p = at, steps = 0;
        while (field[p] != 0) {
            const int i = (int)(p % w), j = (int)(p / w);
            const uint32_t m = near[p] ? near_factor : 1u;
            uint32_t next = NONE;
            for (int d = 0; d < 8 && next == NONE; ++d) {
                const int a = i + DI[d], b = j + DJ[d];
                if (a < 0 || b < 0 || a >= (int)w || b >= (int)h) continue;
                const size_t q = (size_t)b * w + a;
                if (field[q] != NONE && legal(a, b, i, j) && field[q] + ((DI[d] && DJ[d]) ? 7u : 5u) * m == field[p]) next = (uint32_t)q;
            }
            if (next == NONE) break;
            p = next;
            ++steps;
        }
        r[3] = steps;
    }
    return pops;
}
