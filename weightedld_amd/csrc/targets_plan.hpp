// Host-side plan of a target-site run (capi.hip wld_run_targets): the rows of
// a list of chosen sites against every in-window partner.  Validation of the
// list, each target's partner range under the window, the blocks of 16 targets
// the kernel takes on its A side, the work items (block x 64-site partner
// tile) and the batches the dense staging is cut into.  Header-only so the
// host test (tests/cpp/targets_plan_check.cpp) checks the same code.
//
// hi[a] is window_plan's limit (the last in-window partner of a, a itself:
// none; non-decreasing), or empty without a window.  A pair (a, b), a < b, is
// in the window iff b <= hi[a]; so the partners of t above it are t + 1 ..
// hi[t] and those below it the s < t with hi[s] >= t — hi non-decreasing makes
// them the contiguous range lo[t] .. t - 1, lo[t] = the first s with hi[s] >= t
// (hi[t] >= t: lo[t] <= t always).
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace wld {
namespace targets_plan {

constexpr uint32_t kBlock = 16;      // targets per block: the A rows of one 16x16 MFMA block
constexpr uint32_t kTileSide = 64;   // partner sites per work item
constexpr uint32_t kNoTarget = 0xFFFFFFFFu;  // an empty slot of the last block
// WLD_OPT_TARGET_BATCH_SLOTS' default: 2^26 pair slots (16 x blocks x padded
// sites) of three floats each, 768 MiB of staging per batch
constexpr uint64_t kDefaultBatchSlots = 1ull << 26;
constexpr uint64_t kMaxRows = 0xFFFFFFFFull;  // n_targets x (L - 1) of one call

enum BadKind { kFine = 0, kOutOfRange = 1, kRepeated = 2 };
struct Bad {
    BadKind kind = kFine;
    uint32_t pos = 0;    // the first offending list position
    uint32_t first = 0;  // kRepeated: the earlier position holding the same site
};

// The first list position whose target is >= L or repeats an earlier one.
inline Bad validate(const uint32_t *targets, uint32_t n, uint32_t L) {
    std::vector<uint32_t> seen(n ? L : 0, kNoTarget);  // site -> the position that listed it
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t t = targets[k];
        if (t >= L) return {kOutOfRange, k, 0};
        if (seen[t] != kNoTarget) return {kRepeated, k, seen[t]};
        seen[t] = k;
    }
    return {};
}

// lo[t] = the first s with hi[s] >= t, for every site (hi: L entries,
// non-decreasing, hi[s] >= s)
inline std::vector<uint32_t> lower_limits(const std::vector<uint32_t> &hi) {
    const uint32_t L = (uint32_t)hi.size();
    std::vector<uint32_t> lo(L);
    uint32_t s = 0;
    for (uint32_t t = 0; t < L; ++t) {
        while (hi[s] < t) ++s;  // (stops at s == t at the latest)
        lo[t] = s;
    }
    return lo;
}

struct Plan {
    uint32_t L = 0, n_targets = 0, n_blocks = 0;
    // slot 16 b + j: the j-th target of block b in loaded-index order, its list
    // position and its partner range [lo, hi] \ {site}; kNoTarget pads the last block
    std::vector<uint32_t> slot_site, slot_pos, slot_lo, slot_hi;
    // the work items, by block then tile: item_tile[item_begin[b] .. item_begin[b + 1])
    std::vector<uint32_t> item_tile;
    std::vector<uint64_t> item_begin;
    // batch k takes the blocks [batch_begin[k], batch_begin[k + 1])
    std::vector<uint32_t> batch_begin;
    uint64_t items() const { return item_tile.size(); }
    uint32_t batches() const { return batch_begin.empty() ? 0 : (uint32_t)batch_begin.size() - 1; }
};

// does tile hold a partner of the target (site, [lo, hi])?  (a tile whose only
// member in range is the target itself does not)
inline bool tile_has_partner(uint32_t site, uint32_t lo, uint32_t hi, uint32_t tile) {
    const uint64_t t0 = (uint64_t)tile * kTileSide, t1 = t0 + kTileSide - 1;
    if (t1 < lo || t0 > hi) return false;
    const uint64_t s0 = std::max<uint64_t>(t0, lo), s1 = std::min<uint64_t>(t1, hi);
    return s1 - s0 + 1 > ((site >= s0 && site <= s1) ? 1u : 0u);
}

// targets: a validated list (validate gave kFine); hi: the window's limits or
// empty; LP: the padded site count (a multiple of 64); slots: the batch cap
// (>= 1; a batch holds at least one block whatever it says).
inline Plan make(const uint32_t *targets, uint32_t n, uint32_t L, uint32_t LP, const std::vector<uint32_t> &hi,
                 uint64_t slots) {
    Plan p;
    p.L = L;
    p.n_targets = n;
    p.n_blocks = (n + kBlock - 1) / kBlock;
    std::vector<uint32_t> order(n);  // sorted position -> list position
    for (uint32_t k = 0; k < n; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return targets[x] < targets[y]; });
    const std::vector<uint32_t> lo = hi.empty() ? std::vector<uint32_t>() : lower_limits(hi);
    const size_t ns = (size_t)p.n_blocks * kBlock;
    p.slot_site.assign(ns, kNoTarget);
    p.slot_pos.assign(ns, kNoTarget);
    p.slot_lo.assign(ns, 0);
    p.slot_hi.assign(ns, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t t = targets[order[i]];
        p.slot_site[i] = t;
        p.slot_pos[i] = order[i];
        p.slot_lo[i] = hi.empty() ? 0u : lo[t];
        p.slot_hi[i] = hi.empty() ? L - 1 : hi[t];
    }
    // items: per block the union of its targets' tile ranges (a target's own
    // tile only where it holds another site of the range)
    p.item_begin.assign((size_t)p.n_blocks + 1, 0);
    std::vector<std::pair<uint32_t, uint32_t>> iv;
    for (uint32_t b = 0; b < p.n_blocks; ++b) {
        iv.clear();
        for (uint32_t j = 0; j < kBlock; ++j) {
            const size_t s = (size_t)b * kBlock + j;
            const uint32_t t = p.slot_site[s];
            if (t == kNoTarget) continue;
            uint32_t f = p.slot_lo[s] / kTileSide, l = p.slot_hi[s] / kTileSide;
            const uint32_t own = t / kTileSide;  // (f <= own <= l)
            if (tile_has_partner(t, p.slot_lo[s], p.slot_hi[s], own)) {
                iv.emplace_back(f, l);
            } else {  // the own tile drops out: it ends the range on one side or splits it
                if (own > f) iv.emplace_back(f, own - 1);
                if (own < l) iv.emplace_back(own + 1, l);
            }
        }
        std::sort(iv.begin(), iv.end());
        uint32_t next = 0;  // the first tile not yet emitted
        for (const auto &r : iv)
            for (uint32_t tile = std::max(next, r.first); tile <= r.second; ++tile) {
                p.item_tile.push_back(tile);
                next = tile + 1;
            }
        p.item_begin[b + 1] = p.item_tile.size();
    }
    // batches: consecutive blocks, 16 x blocks x LP slots within the cap
    const uint64_t per_block = (uint64_t)kBlock * std::max<uint32_t>(LP, 1);
    const uint64_t bb = std::max<uint64_t>(1, slots / per_block);
    p.batch_begin.push_back(0);
    for (uint64_t b = bb; b < p.n_blocks; b += bb) p.batch_begin.push_back((uint32_t)b);
    if (p.n_blocks) p.batch_begin.push_back(p.n_blocks);
    else p.batch_begin.clear();
    return p;
}

// The items of the blocks [b0, b1) as the launch takes them: tile-major (the
// workgroups of one partner tile run side by side and share its rows in the
// cache), the block local to the batch: {block - b0, tile} pairs.
inline std::vector<uint32_t> batch_items(const Plan &p, uint32_t b0, uint32_t b1) {
    std::vector<std::pair<uint32_t, uint32_t>> it;  // (tile, local block)
    for (uint32_t b = b0; b < b1; ++b)
        for (uint64_t i = p.item_begin[b]; i < p.item_begin[b + 1]; ++i) it.emplace_back(p.item_tile[i], b - b0);
    std::sort(it.begin(), it.end());
    std::vector<uint32_t> out;
    out.reserve(2 * it.size());
    for (const auto &e : it) {
        out.push_back(e.second);
        out.push_back(e.first);
    }
    return out;
}

}  // namespace targets_plan
}  // namespace wld
