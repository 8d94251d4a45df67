// The step list of the banded Cholesky factorisation (banded_chol.hip;
// wld_banded_cholesky_device / wld_banded_solve_device).  Host only.
//
// The n x n matrix of bandwidth K is cut into block rows of 64 rows.  Block row
// I (rows i0 = 64 I .. i0 + rows - 1) takes three steps:
//   1. factor its 64x64 diagonal block;
//   2. solve its panel, the columns [panel_begin, panel_end) right of the
//      diagonal block that the band of its rows reaches: column j belongs to it
//      when some row i of the block row has j - i <= K, i.e. j <= i0 + 63 + K,
//      and j < n (the panel is a trapezoid: row i ends at i + K);
//   3. subtract the panel's products from the trailing window: the 64x64 blocks
//      (a, b), 1 <= a <= b <= blocks, of the panel's columns against themselves
//      (block m holds the columns i0 + 64 m .. i0 + 64 m + 63, clipped at
//      panel_end), upper part only.
// K = 0 and the last block row have an empty panel and no window; K >= n clips
// at n.  The triangular solves walk the same blocks: block row I reads `left`
// blocks of earlier block rows (forward) and `blocks` panel blocks (backward).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace wld {
namespace banded_chol_plan {

constexpr uint32_t kSide = 64;

inline uint32_t block_rows(uint32_t n) { return (uint32_t)(((uint64_t)n + kSide - 1) / kSide); }

// the 64-column blocks a band of width K reaches beyond the diagonal block
inline uint32_t reach(uint32_t K) { return (uint32_t)(((uint64_t)K + kSide - 1) / kSide); }

struct Step {
    uint32_t i0, rows;                // the block row's rows [i0, i0 + rows)
    uint32_t panel_begin, panel_end;  // its panel's columns (empty: both equal)
    uint32_t blocks;                  // 64-column blocks of the panel
    uint32_t left;                    // earlier block rows whose panel meets this block row's columns
};

inline Step step(uint32_t n, uint32_t K, uint32_t I) {
    const uint64_t i0 = (uint64_t)I * kSide;
    Step s;
    s.i0 = (uint32_t)i0;
    s.rows = (uint32_t)std::min<uint64_t>(kSide, n - i0);
    s.panel_begin = (uint32_t)std::min<uint64_t>(i0 + kSide, n);
    s.panel_end = (uint32_t)std::min<uint64_t>(i0 + kSide + K, n);
    s.blocks = (s.panel_end - s.panel_begin + kSide - 1) / kSide;
    s.left = std::min(I, reach(K));
    return s;
}

// one 64x64 block of a trailing window: the rows [r0, r1) x the columns
// [c0, c1) of the matrix, a <= b the panel blocks it multiplies
struct Block {
    uint32_t a, b, r0, r1, c0, c1;
};

inline std::vector<Block> window(const Step &s) {
    std::vector<Block> w;
    for (uint32_t b = 1; b <= s.blocks; ++b)
        for (uint32_t a = 1; a <= b; ++a) {
            const uint32_t r0 = s.i0 + a * kSide, c0 = s.i0 + b * kSide;
            w.push_back(Block{a, b, r0, (uint32_t)std::min<uint64_t>((uint64_t)r0 + kSide, s.panel_end), c0,
                              (uint32_t)std::min<uint64_t>((uint64_t)c0 + kSide, s.panel_end)});
        }
    return w;
}

// The window launch's grid is the list above in this order: workgroup t is the
// t-th pair (a, b), a <= b, counted by b first: t = b (b + 1) / 2 + a (both
// 0-based here: panel blocks a + 1 and b + 1).  Shared with the kernel.
#if defined(__HIPCC__)
#define WLD_CHOL_HD __host__ __device__
#else
#define WLD_CHOL_HD
#endif
WLD_CHOL_HD inline uint64_t tri_count(uint32_t blocks) { return (uint64_t)blocks * ((uint64_t)blocks + 1) / 2; }
WLD_CHOL_HD inline void tri_decode(uint64_t t, uint32_t *a, uint32_t *b) {
    uint64_t hi = (uint64_t)((__builtin_sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (hi * (hi + 1) / 2 > t) --hi;            // (the square root may be off by one either way)
    while ((hi + 1) * (hi + 2) / 2 <= t) ++hi;
    *b = (uint32_t)hi;
    *a = (uint32_t)(t - hi * (hi + 1) / 2);
}

// launches of one factorisation: the fill, then per block row the diagonal
// block's launch and, where the panel is not empty, the panel's and the window's
inline uint64_t launches(uint32_t n, uint32_t K) {
    uint64_t l = 1;
    for (uint32_t I = 0; I < block_rows(n); ++I) l += 1 + (step(n, K, I).blocks ? 2 : 0);
    return l;
}

}  // namespace banded_chol_plan
}  // namespace wld
