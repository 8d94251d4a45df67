// Host-side pieces of the LD heat map (capi.hip wld_run_heatmap; the kernel's
// epilogue in pair_heatmap.hip shares the float <-> key mapping and the grid
// size): the check of a site -> cell map, the order-preserving 32-bit key of
// an f32 (the device keeps a cell's max as the max of keys), the first and
// last cell of every 64-site block, the tile filter, the number of pairs a
// launch must consider, and how two heat maps of disjoint chunk ranges (or of
// a device group's members) combine.  Header-only and free of HIP types so the
// host test (tests/cpp/heatmap_plan_check.cpp) checks the same code.
//
// site_cell[s] is the cell of loaded site s: -1 (on no cell) or an id <
// n_cells, non-decreasing over the sites that have one.  A pair a < b is
// considered iff it is in the chunk range and the window and both sites have
// a cell; it then belongs to cell (site_cell[a], site_cell[b]), row <= column.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "tile_order.hpp"

#if defined(__HIPCC__)
#define WLD_HEAT_HD __host__ __device__
#else
#define WLD_HEAT_HD
#endif

namespace wld {
namespace heatmap_plan {

constexpr uint32_t kMaxCells = 4096;  // per side (= WLD_HEAT_MAX_CELLS)
constexpr uint32_t kTileSide = 64, kChunkSide = 256;
// G: the cells of a tile's rectangle the kernel reduces in LDS (16 bytes
// each); a larger rectangle (cells under two sites wide) goes to global
// memory from the lanes
constexpr uint32_t kGridCells = 1024;

// ---- the key of an f32: key(x) < key(y) iff x < y for all non-NaN x, y
// (-0 below +0), so an unsigned max of keys is the float max, negative values
// included.  Every finite value's key is >= 0x00800000: key 0, what a zeroed
// buffer holds, lies below them all and stands for "no value".
WLD_HEAT_HD inline uint32_t float_key(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
WLD_HEAT_HD inline float key_float(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}
constexpr uint32_t kNoKey = 0;

// ---- validation: the first index that breaks the map's rules, or L
enum : int { kMapOk = 0, kMapTooLarge = 1, kMapNegative = 2, kMapDescends = 3 };
struct MapCheck {
    int what;
    uint32_t index;  // the first offending site (kMapOk: L)
    uint32_t prev;   // kMapDescends: the site before it that has a cell
};
inline MapCheck validate(const int32_t *site_cell, uint32_t L, uint32_t n_cells) {
    bool have = false;
    uint32_t prev = 0;
    for (uint32_t s = 0; s < L; ++s) {
        const int32_t c = site_cell[s];
        if (c == -1) continue;
        if (c < -1) return {kMapNegative, s, 0};
        if ((uint32_t)c >= n_cells) return {kMapTooLarge, s, 0};
        if (have && c < site_cell[prev]) return {kMapDescends, s, prev};
        have = true;
        prev = s;
    }
    return {kMapOk, L, 0};
}

// ---- per 64-site block: the cells of its first and last site with a cell
// (lo > hi: the block has none).  O(L).
struct Blocks {
    std::vector<int32_t> lo, hi;
    bool mapped(uint32_t t) const { return t < lo.size() && lo[t] <= hi[t]; }
};
inline Blocks blocks(const int32_t *site_cell, uint32_t L, uint32_t n_blocks) {
    Blocks b;
    b.lo.assign(n_blocks, 0);
    b.hi.assign(n_blocks, -1);
    for (uint32_t s = 0; s < L && s / kTileSide < n_blocks; ++s) {
        const int32_t c = site_cell[s];
        if (c < 0) continue;
        const uint32_t t = s / kTileSide;
        if (b.lo[t] > b.hi[t]) b.lo[t] = c;
        b.hi[t] = c;
    }
    return b;
}

// ---- the tile filter: of a tile list (ta << 16 | tb), the tiles whose row
// block and column block both hold a site with a cell, in the list's order
inline std::vector<uint32_t> filter_tiles(const std::vector<uint32_t> &tiles, const Blocks &b) {
    std::vector<uint32_t> out;
    for (uint32_t t : tiles)
        if (t != tile_order::kNoTileEntry && b.mapped(t >> 16) && b.mapped(t & 0xFFFFu)) out.push_back(t);
    return out;
}

// ---- the considered pairs of the linear chunks [lb, le): a < b <= hi[a] (hi
// null: no window, every b < L), both with a cell, chunk (a / 256, b / 256)
// in the range.  A prefix count of the sites with a cell, and per site one
// step per chunk column its partners reach.
inline uint64_t considered_pairs(const int32_t *site_cell, const uint32_t *hi, uint32_t L, uint32_t lb, uint32_t le) {
    if (L < 2 || lb >= le) return 0;
    std::vector<uint32_t> pre((size_t)L + 1, 0);
    for (uint32_t s = 0; s < L; ++s) pre[s + 1] = pre[s] + (site_cell[s] >= 0 ? 1u : 0u);
    const uint32_t n = (L + kChunkSide - 1) / kChunkSide;
    uint64_t pairs = 0;
    for (uint32_t a = 0; a + 1 < L; ++a) {
        if (site_cell[a] < 0) continue;
        const uint32_t h = hi ? std::min(hi[a], L - 1) : L - 1, row = a / kChunkSide;
        for (uint32_t b = a + 1; b <= h;) {
            const uint32_t col = b / kChunkSide;
            const uint32_t e = std::min<uint32_t>(h, (col + 1) * kChunkSide - 1);
            const uint32_t li = tile_order::chunk_linear_host(n, row, col);
            if (li >= lb && li < le) pairs += pre[e + 1] - pre[b];
            b = e + 1;
        }
    }
    return pairs;
}

// ---- a heat map on the host: n_cells x n_cells row-major; max as keys
// (kNoKey where count == 0)
struct Heatmap {
    uint32_t n_cells = 0;
    uint64_t pairs = 0, none_pairs = 0, nonfinite_pairs = 0, counted_pairs = 0;
    uint64_t tiles = 0;
    double kernel_ms = 0.0;
    std::vector<uint64_t> count;
    std::vector<double> sum;
    std::vector<uint32_t> max_key;
};

// into (+)= from: counts and sums add, max is the larger key, tiles add,
// kernel_ms is the slower of the two (members of a device group run side by
// side).  An empty `into` takes from's shape.
inline void merge(Heatmap &into, const Heatmap &from) {
    into.pairs += from.pairs;
    into.none_pairs += from.none_pairs;
    into.nonfinite_pairs += from.nonfinite_pairs;
    into.counted_pairs += from.counted_pairs;
    into.tiles += from.tiles;
    if (from.kernel_ms > into.kernel_ms) into.kernel_ms = from.kernel_ms;
    if (into.n_cells < from.n_cells) into.n_cells = from.n_cells;
    if (into.count.size() < from.count.size()) into.count.resize(from.count.size(), 0);
    if (into.sum.size() < from.sum.size()) into.sum.resize(from.sum.size(), 0.0);
    if (into.max_key.size() < from.max_key.size()) into.max_key.resize(from.max_key.size(), kNoKey);
    for (size_t i = 0; i < from.count.size(); ++i) into.count[i] += from.count[i];
    for (size_t i = 0; i < from.sum.size(); ++i) into.sum[i] += from.sum[i];
    for (size_t i = 0; i < from.max_key.size(); ++i) into.max_key[i] = std::max(into.max_key[i], from.max_key[i]);
}

}  // namespace heatmap_plan
}  // namespace wld
