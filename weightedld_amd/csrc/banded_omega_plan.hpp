// The tiling of the pair-sum table of a band and the splits of a sweep scan
// (banded_omega.hip; wld_banded_pairsum_device, wld_banded_omega_device,
// wld_omega_splits).  Host only, except the clipping rules the kernels share.
//
// The table M[j][k] = sum of the band's entries (u, v) with j <= u < v <= j + k
// is built in two passes over band storage ([n][K + 1], element k of row j is
// entry (j, j + k)):
//
//   rows    P[j][k] = P[j][k-1] + b(j, k): n chains along the rows.  A row
//           block holds 64 rows; it walks the columns in tiles of 64 (col_tiles),
//           each tile loaded as 64 row segments and scanned by one lane per row.
//   chains  M[j][k] = M[j+1][k-1] + P[j][k]: one chain per end site i = j + k,
//           walked from k = 0 (row i) down to k = K (row i - K).  A chain block
//           holds the 64 chains i0 .. i0 + 63; in one step it takes ONE row j,
//           lane c the element k = i0 + c - j of it, so the 64 lanes read and
//           write one contiguous run of a row (row_segment).  Over 64 steps the
//           block covers a parallelogram: 64 chains x 64 steps (tile).  The
//           chains i >= n hold only the +0.0 tails (j + k >= n), so the blocks
//           cover i = 0 .. n + K - 1.
//
// Clipping: a chain starts at row min(i, n - 1) and ends at row max(0, i - K);
// K < 64 leaves most of a run's lanes past the band; K >= n ends every chain at
// row 0.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define WLD_OMEGA_HD __host__ __device__
#else
#define WLD_OMEGA_HD
#endif

namespace wld {
namespace banded_omega_plan {

constexpr uint32_t kSide = 64;

// the row pass: blocks of 64 rows, tiles of 64 columns k = 0 .. K
inline uint32_t row_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + kSide - 1) / kSide); }
WLD_OMEGA_HD inline uint32_t col_tiles(uint32_t K) { return (uint32_t)((uint64_t)K / kSide + 1); }

// the chain pass: blocks of 64 chains i = 0 .. n + K - 1 (n >= 1)
inline uint32_t chain_blocks(uint32_t n, uint32_t K) { return (uint32_t)(((uint64_t)n + K + kSide - 1) / kSide); }

// the rows a chain block walks, top (first) to bottom (last), both inclusive:
// from the first row that holds an element of one of its chains to the last
struct Rows {
    uint32_t top, bottom;
};
WLD_OMEGA_HD inline Rows rows(uint64_t i0, uint32_t n, uint32_t K) {
    Rows r;
    r.top = (uint32_t)(i0 + kSide - 1 < (uint64_t)n - 1 ? i0 + kSide - 1 : (uint64_t)n - 1);
    r.bottom = (uint32_t)(i0 > K ? i0 - K : 0);
    return r;
}

// the elements k of row j that belong to the chains i0 .. i0 + 63: [k_lo, k_hi]
// (false: none); lane c of the block holds k = i0 + c - j
WLD_OMEGA_HD inline bool row_segment(uint64_t i0, uint32_t j, uint32_t K, uint32_t *k_lo, uint32_t *k_hi) {
    if (i0 + kSide - 1 < j) return false;
    const uint64_t lo = i0 > j ? i0 - j : 0, hi = i0 + kSide - 1 - j;
    if (lo > K) return false;
    *k_lo = (uint32_t)lo;
    *k_hi = (uint32_t)(hi < K ? hi : K);
    return true;
}

// the 64-step tiles of a chain block: tile t walks the rows top - 64 t down to
// max(bottom, top - 64 t - 63).  The chain kernel does not consult these two: it
// walks rows() top down in groups of eight with the chain's value in a register,
// so a 64-step tile is only a way to state (and check) which rows and runs 64
// chains x 64 steps cover.
inline uint32_t step_tiles(uint64_t i0, uint32_t n, uint32_t K) {
    const Rows r = rows(i0, n, K);
    if (r.bottom > r.top) return 0;
    return (r.top - r.bottom) / kSide + 1;
}
inline Rows tile(uint64_t i0, uint32_t n, uint32_t K, uint32_t t) {
    const Rows r = rows(i0, n, K);
    Rows q;
    q.top = r.top - t * kSide;
    q.bottom = q.top - r.bottom >= kSide ? q.top - (kSide - 1) : r.bottom;
    return q;
}

// what a split of the scan must satisfy: lo <= c < hi < n and hi - lo <= K
WLD_OMEGA_HD inline bool split_ok(uint32_t c, uint32_t lo, uint32_t hi, uint32_t n, uint32_t K) {
    return lo <= c && c < hi && hi < n && hi - lo <= K;
}

// candidate border pairs of a split: left borders a = lo .. c + 1 - min_side,
// right borders b = c + min_side .. hi
WLD_OMEGA_HD inline void split_sides(uint32_t c, uint32_t lo, uint32_t hi, uint32_t min_side, uint32_t *n_left,
                                     uint32_t *n_right) {
    const uint64_t a_end = (uint64_t)c + 1, b_min = (uint64_t)c + min_side;
    *n_left = a_end >= (uint64_t)lo + min_side ? (uint32_t)(a_end - min_side - lo + 1) : 0;
    *n_right = b_min <= hi ? (uint32_t)(hi - b_min + 1) : 0;
}

// The splits of a scan from coordinates (wld_omega_splits).  pos: the sites'
// coordinates, non-decreasing (null: pos[i] = i).  n_grid 0: every split c = 0 ..
// n - 2 at x = pos[c]; n_grid >= 1: the equidistant positions x_g = pos[0] +
// floor(span g / (n_grid - 1)), span = pos[n - 1] - pos[0] (n_grid 1: the
// midpoint pos[0] + floor(span / 2)), c the last site with pos <= x_g, clamped
// to [0, n - 2].  lo = max(c + 1 - max_side, first site with pos >= x - D), at
// most c; hi = min(c + max_side, last site with pos <= x + D, n - 1), at least
// c + 1; D = max_distance, 0: no distance limit.  Needs n >= 2, max_side >= 1.
inline uint64_t n_splits(uint32_t n, uint32_t n_grid) { return n_grid ? n_grid : (uint64_t)n - 1; }

// the first index i >= 1 with pos[i] < pos[i - 1], or n when there is none (or no pos)
template <class Pos>
inline uint32_t first_descent(const Pos *pos, uint32_t n) {
    if (pos)
        for (uint32_t i = 1; i < n; ++i)
            if (pos[i] < pos[i - 1]) return i;
    return n;
}

// (Pos: uint64_t coordinates of the caller, or the context's 32-bit copy)
template <class Pos>
inline void splits(const Pos *pos, uint32_t n, uint32_t n_grid, uint32_t max_side, uint64_t max_distance,
                   uint64_t *position, uint32_t *split, uint32_t *lo, uint32_t *hi) {
    auto at = [&](uint32_t i) -> uint64_t { return pos ? pos[i] : i; };
    // the first site with pos >= x, in [0, n]
    auto first_ge = [&](uint64_t x) -> uint32_t {
        uint32_t b = 0, e = n;
        while (b < e) {
            const uint32_t mid = b + (e - b) / 2;
            if (at(mid) >= x) e = mid;
            else b = mid + 1;
        }
        return b;
    };
    // one past the last site with pos <= x, in [0, n]
    auto first_gt = [&](uint64_t x) -> uint32_t {
        uint32_t b = 0, e = n;
        while (b < e) {
            const uint32_t mid = b + (e - b) / 2;
            if (at(mid) > x) e = mid;
            else b = mid + 1;
        }
        return b;
    };
    const uint64_t p0 = at(0), span = at(n - 1) - p0, total = n_splits(n, n_grid);
    for (uint64_t g = 0; g < total; ++g) {
        uint64_t x;
        uint32_t c;
        if (!n_grid) {
            c = (uint32_t)g;
            x = at(c);
        } else {
            x = n_grid == 1 ? p0 + span / 2
                            : p0 + (uint64_t)((unsigned __int128)span * g / (uint64_t)(n_grid - 1));
            const uint32_t past = first_gt(x);  // (>= 1: pos[0] <= x)
            c = std::min<uint32_t>(past ? past - 1 : 0, n - 2);
        }
        uint32_t l = c + 1 > max_side ? c + 1 - max_side : 0;
        uint32_t h = (uint32_t)std::min<uint64_t>((uint64_t)c + max_side, n - 1);
        if (max_distance) {
            l = std::max(l, first_ge(x > max_distance ? x - max_distance : 0));
            const uint64_t top = x + max_distance < x ? ~0ull : x + max_distance;
            const uint32_t past = first_gt(top);
            h = std::min(h, past ? past - 1 : 0);
        }
        position[g] = x;
        split[g] = c;
        lo[g] = std::min(l, c);
        hi[g] = std::max(h, c + 1);
    }
}

}  // namespace banded_omega_plan
}  // namespace wld
