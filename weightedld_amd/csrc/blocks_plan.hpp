// Host-side pieces of the LD blocks (capi.hip wld_run_block_breaks,
// wld_blocks_partition, wld_blocks_from_breaks, wld_run_blocks; the two
// epilogues in pair_blocks.hip share the min key and the table size): the
// argument checks, how break arrays of disjoint chunk ranges (or of a device
// group's members) combine, the partition of the site axis from the break
// arrays, the tiles pass 2 launches and the per-64-site-block id limits its
// epilogue reduces over.  Header-only and free of HIP types so the host test
// (tests/cpp/blocks_plan_check.cpp) checks the same code.
//
// Breaks.  fwd[a] = the smallest b of the weak considered pairs (a, b),
// bwd[b] = the largest a of the weak considered pairs (a, b), kNone where
// there is none; last[a] = the last in-window partner of a (n - 1 without a
// window; non-decreasing, last[a] >= a).
//
// A run [s, e] (e <= last[s]) is valid under
//   kRuleAll    iff no pair of it is weak:        fwd[i] > e for every i in [s, e];
//   kRuleSpine  iff no pair (s, k), (k, e) is:    fwd[s] > e and bwd[e] < s.
// The partition starts at s = 0, takes the largest e in [s, last[s]] with
// [s, e] valid, and goes on at e + 1; runs of >= min_sites sites are blocks.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "heatmap_plan.hpp"

namespace wld {
namespace blocks_plan {

constexpr uint32_t kNone = 0xFFFFFFFFu;  // = WLD_BLOCKS_NONE
constexpr int kStatR2 = 0, kStatAbsDprime = 1;
constexpr int kRuleAll = 0, kRuleSpine = 1;
constexpr uint32_t kTileSide = 64;
// the block ids one tile's counted pairs can carry: a block has >= 2 sites, so
// a 64-site block meets at most 33 (32 inside it and one reaching in)
constexpr uint32_t kTableIds = 64;

// ---- the min of a block as an unsigned max: inv_key(x) = ~float_key(x), so
// the largest inv_key belongs to the smallest value under float_key's order.
// Every finite value's inv_key is >= 0x00800000: 0, what a zeroed buffer
// holds, stands for "no value".
WLD_HEAT_HD inline uint32_t inv_key(float x) { return ~heatmap_plan::float_key(x); }
WLD_HEAT_HD inline float inv_key_float(uint32_t k) { return heatmap_plan::key_float(~k); }
constexpr uint32_t kNoInvKey = 0;

// ---- the argument checks: 0, or which argument is wrong
enum : int { kArgOk = 0, kArgStat = 1, kArgStrongMin = 2, kArgRule = 3, kArgMinSites = 4 };
inline int check_stat(int stat, float strong_min) {
    if (stat != kStatR2 && stat != kStatAbsDprime) return kArgStat;
    if (!std::isfinite(strong_min)) return kArgStrongMin;
    return kArgOk;
}
inline int check_rule(int rule, uint32_t min_sites) {
    if (rule != kRuleAll && rule != kRuleSpine) return kArgRule;
    if (min_sites < 2) return kArgMinSites;
    return kArgOk;
}

// ---- the breaks of a range on the host
struct Breaks {
    uint32_t n_sites = 0;
    int stat = kStatR2;
    float strong_min = 0.0f;
    uint64_t pairs = 0, none_pairs = 0, nonfinite_pairs = 0, strong_pairs = 0, weak_pairs = 0;
    uint64_t tiles = 0;
    double kernel_ms = 0.0;
    std::vector<uint32_t> fwd, bwd, last;  // n_sites each
};

inline bool same_float(float a, float b) {
    uint32_t x, y;
    __builtin_memcpy(&x, &a, 4);
    __builtin_memcpy(&y, &b, 4);
    return x == y;
}
// whether two results may merge: the same set, statistic, threshold and window
inline bool mergeable(uint64_t n_a, int stat_a, float min_a, const uint32_t *last_a, uint64_t n_b, int stat_b,
                      float min_b, const uint32_t *last_b) {
    if (n_a != n_b || stat_a != stat_b || !same_float(min_a, min_b)) return false;
    for (uint64_t i = 0; i < n_a; ++i)
        if (last_a[i] != last_b[i]) return false;
    return true;
}
// into (+)= from over disjoint ranges: fwd by min, bwd by max (kNone below
// every index), totals and tiles add, kernel_ms is the slower of the two
// (members of a device group run side by side)
inline void merge_arrays(uint32_t *fwd, uint32_t *bwd, const uint32_t *ffwd, const uint32_t *fbwd, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) {
        fwd[i] = std::min(fwd[i], ffwd[i]);  // (kNone is the largest value)
        if (fbwd[i] != kNone && (bwd[i] == kNone || fbwd[i] > bwd[i])) bwd[i] = fbwd[i];
    }
}
inline void merge(Breaks &into, const Breaks &from) {
    into.pairs += from.pairs;
    into.none_pairs += from.none_pairs;
    into.nonfinite_pairs += from.nonfinite_pairs;
    into.strong_pairs += from.strong_pairs;
    into.weak_pairs += from.weak_pairs;
    into.tiles += from.tiles;
    into.kernel_ms = std::max(into.kernel_ms, from.kernel_ms);
    if (into.fwd.empty() && !into.n_sites) {
        into.n_sites = from.n_sites;
        into.stat = from.stat;
        into.strong_min = from.strong_min;
        into.fwd = from.fwd;
        into.bwd = from.bwd;
        into.last = from.last;
        return;
    }
    merge_arrays(into.fwd.data(), into.bwd.data(), from.fwd.data(), from.bwd.data(),
                 std::min(into.fwd.size(), from.fwd.size()));
}

// ---- the partition
struct Partition {
    std::vector<uint32_t> first, last;  // per block, in site order
    std::vector<int32_t> site_block;    // per site: its block, or -1
};
// the end of the run that starts at s
inline uint32_t run_end(const uint32_t *fwd, const uint32_t *bwd, const uint32_t *last, uint32_t n, uint32_t s,
                        int rule) {
    uint32_t bound = std::min(last[s], n - 1);
    if (bound < s) bound = s;
    if (rule == kRuleAll) {
        // the running minimum of fwd[i] - 1 while i stays inside it (fwd[i] > i)
        for (uint32_t i = s; i <= bound; ++i)
            if (fwd[i] != kNone && fwd[i] > i) bound = std::min(bound, fwd[i] - 1);
        return bound;
    }
    if (fwd[s] != kNone && fwd[s] > s) bound = std::min(bound, fwd[s] - 1);
    for (uint32_t e = bound; e > s; --e)
        if (bwd[e] == kNone || bwd[e] < s) return e;
    return s;
}
inline Partition partition(const uint32_t *fwd, const uint32_t *bwd, const uint32_t *last, uint32_t n, int rule,
                           uint32_t min_sites) {
    Partition p;
    p.site_block.assign(n, -1);
    for (uint32_t s = 0; s < n;) {
        const uint32_t e = run_end(fwd, bwd, last, n, s, rule);
        if (e - s + 1 >= min_sites) {
            const int32_t id = (int32_t)p.first.size();
            p.first.push_back(s);
            p.last.push_back(e);
            for (uint32_t i = s; i <= e; ++i) p.site_block[i] = id;
        }
        s = e + 1;
    }
    return p;
}

// ---- pass 2's tiles (ta << 16 | tb, ta <= tb), ascending: those some block
// intersects in both its row block and its column block
inline std::vector<uint32_t> stats_tiles(const Partition &p) {
    std::vector<uint32_t> t;
    for (size_t k = 0; k < p.first.size(); ++k) {
        const uint32_t lo = p.first[k] / kTileSide, hi = p.last[k] / kTileSide;
        for (uint32_t ta = lo; ta <= hi; ++ta)
            for (uint32_t tb = ta; tb <= hi; ++tb) t.push_back((ta << 16) | tb);
    }
    std::sort(t.begin(), t.end());
    t.erase(std::unique(t.begin(), t.end()), t.end());
    return t;
}
// ... and the pairs they must count: the pairs inside the blocks
inline uint64_t block_pairs(const Partition &p) {
    uint64_t s = 0;
    for (size_t k = 0; k < p.first.size(); ++k) {
        const uint64_t m = (uint64_t)p.last[k] - p.first[k] + 1;
        s += m * (m - 1) / 2;
    }
    return s;
}
// ---- per 64-site block the first and last block id of its sites (lo > hi:
// none): heatmap_plan::blocks on site_block.  Ids ascend over the sites and a
// block has >= 2 sites, so hi - lo < kTableIds.
inline heatmap_plan::Blocks id_limits(const Partition &p, uint32_t n_tile_blocks) {
    return heatmap_plan::blocks(p.site_block.data(), (uint32_t)p.site_block.size(), n_tile_blocks);
}

}  // namespace blocks_plan
}  // namespace wld
