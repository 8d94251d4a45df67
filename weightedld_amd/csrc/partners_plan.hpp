// Host-side pieces of the best-partner lists (capi.hip wld_run_partners; the
// selecting epilogue and the merge kernel in pair_partners.hip share the key
// packing and the staging layout): the 64-bit selection key and its inverse,
// the per-block CSR of the tile parts of a tile list, the cut of a tile list
// into staging batches, the staging size, the number of pairs a range must
// consider, and how two results over disjoint chunk ranges (or of a device
// group's members) combine.  Header-only and free of HIP types so the host
// test (tests/cpp/partners_plan_check.cpp) checks the same code.
//
// Order.  The candidates of a site are ordered by r2 descending under
// heatmap_plan::float_key's total order (-0 below +0), then by partner loaded
// index ascending.  key = float_key(r2) << 32 | (0xFFFFFFFF - partner): the
// unsigned maximum of the keys is the first candidate.  A site never meets the
// same partner twice (a pair lies in one tile of one chunk), so a site's keys
// are distinct and "the best k" is one set whatever order the parts arrive in.
// Key 0 lies below every candidate's key (a finite or infinite r2 has
// float_key >= 0x007FFFFF) and stands for "no entry".
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "heatmap_plan.hpp"
#include "tile_order.hpp"

#if defined(__HIPCC__)
#define WLD_PART_HD __host__ __device__
#else
#define WLD_PART_HD
#endif

namespace wld {
namespace partners_plan {

constexpr uint32_t kMaxK = 64;  // = WLD_PARTNERS_MAX_K, the tile side
constexpr uint32_t kTileSide = 64, kChunkSide = 256;
constexpr uint32_t kNoPartner = 0xFFFFFFFFu;
constexpr uint64_t kNoKey = 0;
constexpr uint64_t kDefaultBatchBytes = 1ull << 30;  // WLD_OPT_PARTNERS_BATCH_BYTES

// one staged or listed candidate: 16 bytes
struct Entry {
    uint64_t key;
    float d, dp;
};

WLD_PART_HD inline uint64_t pack_key(float r2, uint32_t partner) {
    return (uint64_t)heatmap_plan::float_key(r2) << 32 | (uint64_t)(kNoPartner - partner);
}
WLD_PART_HD inline float key_r2(uint64_t key) { return heatmap_plan::key_float((uint32_t)(key >> 32)); }
WLD_PART_HD inline uint32_t key_partner(uint64_t key) { return kNoPartner - (uint32_t)key; }

// ---- staging of a batch of n tiles at list length kp = min(k, 64): per tile
// two sides (0: its a rows, 1: its b columns) of 64 local sites, each a part of
// kp entries and one count.  Part index = (2 position + side) * 64 + local site.
inline uint64_t parts_of(uint64_t n_tiles) { return n_tiles * 2 * kTileSide; }
inline uint64_t tile_bytes(uint32_t kp) { return 2ull * kTileSide * ((uint64_t)kp * sizeof(Entry) + sizeof(uint32_t)); }
inline uint64_t staging_bytes(uint64_t n_tiles, uint32_t kp) { return n_tiles * tile_bytes(kp); }

// ---- the batch cut: tiles per batch under batch_bytes, at least one
inline uint64_t batch_tiles(uint64_t batch_bytes, uint32_t kp) {
    return std::max<uint64_t>(1, batch_bytes / tile_bytes(kp));
}
// [begin, end) of every batch of an n-entry list
inline std::vector<std::pair<uint64_t, uint64_t>> batches(uint64_t n, uint64_t batch_bytes, uint32_t kp) {
    std::vector<std::pair<uint64_t, uint64_t>> out;
    const uint64_t per = batch_tiles(batch_bytes, kp);
    for (uint64_t b = 0; b < n; b += per) out.emplace_back(b, std::min(n, b + per));
    return out;
}

// ---- per 64-site block, the (2 position + side) entries of the batch's tiles
// [begin, end) of a list (ta << 16 | tb; padding entries skipped) that hold
// parts of its sites: block ta the tile's side 0, block tb its side 1 (a
// diagonal tile both).  Positions count from the batch's first tile.  Entries
// of a block are in list order.
struct Csr {
    std::vector<uint32_t> off;  // n_blocks + 1
    std::vector<uint32_t> ent;
};
inline Csr build_csr(const uint32_t *tiles, uint64_t begin, uint64_t end, uint32_t n_blocks) {
    Csr c;
    c.off.assign((size_t)n_blocks + 1, 0);
    auto each = [&](auto &&f) {
        for (uint64_t p = begin; p < end; ++p) {
            const uint32_t t = tiles[p];
            if (t == tile_order::kNoTileEntry) continue;
            const uint32_t ta = t >> 16, tb = t & 0xFFFFu;
            if (ta >= n_blocks || tb >= n_blocks) continue;
            f(ta, (uint32_t)(2 * (p - begin)));
            f(tb, (uint32_t)(2 * (p - begin) + 1));
        }
    };
    each([&](uint32_t blk, uint32_t) { ++c.off[blk + 1]; });
    for (uint32_t b = 0; b < n_blocks; ++b) c.off[b + 1] += c.off[b];
    c.ent.assign(c.off[n_blocks], 0);
    std::vector<uint32_t> cur(c.off.begin(), c.off.end() - 1);
    each([&](uint32_t blk, uint32_t e) { c.ent[cur[blk]++] = e; });
    return c;
}

// ---- the considered pairs of the linear chunks [lb, le): a < b <= hi[a] (hi
// null: no window, every b < L) with chunk (a / 256, b / 256) in the range
inline uint64_t considered_pairs(const uint32_t *hi, uint32_t L, uint32_t lb, uint32_t le) {
    if (L < 2 || lb >= le) return 0;
    const uint32_t n = (L + kChunkSide - 1) / kChunkSide;
    uint64_t pairs = 0;
    for (uint32_t a = 0; a + 1 < L; ++a) {
        const uint32_t h = hi ? std::min(hi[a], L - 1) : L - 1, row = a / kChunkSide;
        for (uint32_t b = a + 1; b <= h;) {
            const uint32_t col = b / kChunkSide;
            const uint32_t e = std::min<uint32_t>(h, (col + 1) * kChunkSide - 1);
            const uint32_t li = tile_order::chunk_linear_host(n, row, col);
            if (li >= lb && li < le) pairs += e - b + 1;
            b = e + 1;
        }
    }
    return pairs;
}

// ---- a result on the host: per site k entries, best first, kNoKey past the
// site's count
struct Partners {
    uint32_t n_sites = 0, k = 0;
    uint64_t pairs = 0, none_pairs = 0, passing_pairs = 0, tiles = 0;
    double kernel_ms = 0.0, merge_ms = 0.0;
    std::vector<Entry> list;  // n_sites * k
};

// the best k of two lists (each best first, kNoKey padded) into out (may not
// alias either)
inline void merge_lists(const Entry *x, const Entry *y, uint32_t k, Entry *out) {
    uint32_t i = 0, j = 0;
    for (uint32_t n = 0; n < k; ++n) {
        const uint64_t kx = i < k ? x[i].key : kNoKey, ky = j < k ? y[j].key : kNoKey;
        if (kx == kNoKey && ky == kNoKey) out[n] = Entry{kNoKey, 0.0f, 0.0f};
        else if (kx >= ky) out[n] = x[i++];
        else out[n] = y[j++];
    }
}

// into (+)= from: lists merge under the order, counters and tiles add, the
// times are the slower of the two (members of a device group run side by
// side).  An empty `into` takes from's shape; the shapes must agree otherwise
// (the caller checks).
inline void merge(Partners &into, const Partners &from) {
    into.pairs += from.pairs;
    into.none_pairs += from.none_pairs;
    into.passing_pairs += from.passing_pairs;
    into.tiles += from.tiles;
    into.kernel_ms = std::max(into.kernel_ms, from.kernel_ms);
    into.merge_ms = std::max(into.merge_ms, from.merge_ms);
    if (into.list.empty() && !into.n_sites) {
        into.n_sites = from.n_sites;
        into.k = from.k;
        into.list = from.list;
        return;
    }
    const uint32_t k = into.k;
    std::vector<Entry> tmp(k);
    for (uint32_t s = 0; s < into.n_sites && s < from.n_sites; ++s) {
        merge_lists(&into.list[(size_t)s * k], &from.list[(size_t)s * k], k, tmp.data());
        std::copy(tmp.begin(), tmp.end(), into.list.begin() + (size_t)s * k);
    }
}

}  // namespace partners_plan
}  // namespace wld
