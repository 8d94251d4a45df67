// Host-side plan of a windowed run (capi.hip wld_set_window): which pairs of
// the loaded set lie in the window (max_distance D in parent coordinates,
// max_sites K in loaded sites; 0 = no limit), per site, per reference chunk
// and per 64x64 tile, and the shard partition balanced by in-window pairs.
// Header-only so the host test (tests/cpp/window_plan_check.cpp) checks the
// same code.
//
// pos[i] is the parent coordinate of loaded site i (null: pos[i] = i) and
// must be non-decreasing when D > 0 (first_descent).  A pair a < b is in the
// window iff (D == 0 || pos[b] - pos[a] <= D) && (K == 0 || b - a <= K); pos
// monotone makes a's partners the contiguous range a + 1 .. hi[a], and hi
// itself non-decreasing.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "tile_order.hpp"

namespace wld {
namespace window_plan {

constexpr uint32_t kChunkSide = 256, kTileSide = 64, kTilesPerChunkSide = 4;

// the first index i >= 1 with pos[i] < pos[i - 1], or L when there is none
inline uint32_t first_descent(const uint32_t *pos, uint32_t L) {
    for (uint32_t i = 1; i < L; ++i)
        if (pos[i] < pos[i - 1]) return i;
    return L;
}

// hi[a]: the last in-window partner of a (hi[a] == a: none).  The device's
// window_limits_kernel (order.hip) computes the same by the same search.
inline std::vector<uint32_t> limits(const uint32_t *pos, uint32_t L, uint64_t D, uint64_t K) {
    std::vector<uint32_t> hi(L);
    for (uint32_t a = 0; a < L; ++a) {
        uint32_t h = L - 1;
        if (K && K < (uint64_t)(h - a)) h = a + (uint32_t)K;
        if (D) {
            // (coordinates are 32-bit: a larger D admits as much as 2^32 - 1, and cannot wrap)
            const uint64_t lim = (uint64_t)(pos ? pos[a] : a) + std::min<uint64_t>(D, 0xFFFFFFFFull);
            // the largest b in [a, h] with pos[b] <= lim (pos[a] <= lim holds)
            uint32_t lo = a, up = h;
            while (lo < up) {
                const uint32_t mid = lo + (up - lo + 1) / 2;
                if ((uint64_t)(pos ? pos[mid] : mid) <= lim) lo = mid;
                else up = mid - 1;
            }
            h = lo;
        }
        hi[a] = h;
    }
    return hi;
}

inline uint32_t chunk_rows(uint32_t L) { return (L + kChunkSide - 1) / kChunkSide; }

// In-window pairs of every reference chunk as a prefix in linear chunk order:
// pre[i] = the pairs of linear chunks [0, i), n(n+1)/2 + 1 entries.
inline std::vector<uint64_t> chunk_prefix(const std::vector<uint32_t> &hi) {
    const uint32_t L = (uint32_t)hi.size(), n = chunk_rows(L);
    std::vector<uint64_t> pre((size_t)n * (n + 1) / 2 + 1, 0);
    for (uint32_t a = 0; a < L; ++a) {
        const uint32_t row = a / kChunkSide;
        for (uint32_t b = a + 1; b <= hi[a];) {  // a's partners, one chunk column at a time
            const uint32_t col = b / kChunkSide;
            const uint32_t e = std::min<uint32_t>(hi[a], (col + 1) * kChunkSide - 1);
            pre[(size_t)tile_order::chunk_linear_host(n, row, col) + 1] += e - b + 1;
            b = e + 1;
        }
    }
    for (size_t i = 1; i < pre.size(); ++i) pre[i] += pre[i - 1];
    return pre;
}

// does tile (ta, tb), tb >= ta, hold an in-window pair?
inline bool tile_in_window(const std::vector<uint32_t> &hi, uint32_t ta, uint32_t tb) {
    const uint32_t L = (uint32_t)hi.size();
    const uint32_t a0 = ta * kTileSide, a1 = std::min(L, a0 + kTileSide);  // the tile's a sites [a0, a1)
    if (a0 >= L) return false;
    if (tb > ta) return hi[a1 - 1] >= tb * kTileSide;  // (hi non-decreasing: the last a reaches furthest)
    for (uint32_t a = a0; a + 1 < a1; ++a)             // the diagonal tile: a partner inside it
        if (hi[a] > a) return true;
    return false;
}

// tile_order::range_tiles restricted to the tiles holding an in-window pair,
// in the same (ta, tb) order and packing
inline std::vector<uint32_t> range_tiles(uint32_t n, uint32_t T_used, uint32_t lb, uint32_t le,
                                         const std::vector<uint32_t> &hi) {
    const uint32_t L = (uint32_t)hi.size();
    std::vector<uint32_t> t;
    for (uint32_t ta = 0; ta < T_used && ta * kTileSide < L; ++ta) {
        const uint32_t row = ta / kTilesPerChunkSide;
        const uint32_t reach = hi[std::min(L, (ta + 1) * kTileSide) - 1] / kTileSide;  // the row's last b tile
        for (uint32_t col = row; col < n && col * kTilesPerChunkSide <= reach; ++col) {
            const uint32_t li = tile_order::chunk_linear_host(n, row, col);
            if (li < lb || li >= le) continue;
            for (uint32_t tb = std::max(ta, col * kTilesPerChunkSide);
                 tb < std::min<uint32_t>((col + 1) * kTilesPerChunkSide, T_used) && tb <= reach; ++tb)
                if (tile_in_window(hi, ta, tb)) t.push_back((ta << 16) | tb);
        }
    }
    return t;
}

// Shard `shard` of n_shards of the chunk sequence, balanced by in-window
// pairs: boundary j is the linear chunk whose prefix is closest to j/n_shards
// of the total, and shard k takes the k-th range from the END (the
// conventions of wld_shard_chunks).  Each boundary lies within half a chunk's
// count of its target, so no shard exceeds total / n_shards by more than the
// largest single chunk's count.
inline void shard_range(const std::vector<uint64_t> &pre, int n_shards, int shard, uint32_t *begin, uint32_t *end) {
    const uint32_t m = (uint32_t)pre.size() - 1;
    auto boundary = [&](int j) -> uint32_t {
        if (j <= 0) return 0;
        if (j >= n_shards) return m;
        const long double target = (long double)pre[m] * j / n_shards;
        uint32_t i = (uint32_t)(std::upper_bound(pre.begin(), pre.end(), (uint64_t)target) - pre.begin()) - 1;
        if (i < m && (long double)pre[i + 1] - target < target - (long double)pre[i]) ++i;
        return i;
    };
    *begin = boundary(n_shards - 1 - shard);
    *end = boundary(n_shards - shard);
    if (*end < *begin) *end = *begin;
}

}  // namespace window_plan
}  // namespace wld
