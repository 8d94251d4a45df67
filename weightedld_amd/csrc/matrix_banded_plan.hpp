// Host-side plan of the banded LD matrix (capi.hip wld_matrix_banded_width /
// wld_run_matrix_banded_device / wld_run_matrix_banded): the argument checks,
// the width a window needs, the tile list of a row range, the description of
// the elements no listed tile writes (the fill list), the strip split of the
// host call and the pair count of a row range.  Header-only and free of HIP
// types so that the host test (tests/cpp/matrix_banded_plan_check.cpp) checks
// the same code; covered() is also what the fill kernel evaluates
// (pair_matrix_banded.hip).
//
// ("band" in matrix_plan.hpp means the dense host call's row strips; the
// diagonal storage here is "banded", its host call's row ranges "strips".)
//
// Layout.  Upper band, row-major by site: for the rows u in [r0, r1) (loaded
// site indices) and k = 0..K, dst[(u - r0) * ld + k] is entry (u, u + k) of the
// LD matrix.  Pair (a, b), a < b, is computed once, by tile (ta, tb) =
// (a / 64, b / 64), ta <= tb, and lands in row a at k = b - a: a listed tile
// writes, in each of its rows u inside [r0, r1), the elements of the columns
// b = 64 tb .. 64 tb + 63 with u <= b and b - u <= K (one contiguous run of k;
// columns b >= L hold +0.0, the diagonal tile supplies k = 0 by the diagonal
// rule).  The listed tiles of row tile ta are those of the offsets tb - ta in
// [c0, c1) (Cover: the window's limits are non-decreasing, so the tiles that
// hold an in-window pair are consecutive but for the diagonal one), and
// element (u, k) is written by one of them iff 64 c0 <= (u - 64 ta) + k <
// 64 c1.  Every other element of the block gets +0.0 (k = 0: the diagonal
// rule) from the fill kernel, which takes the 64 x 64 blocks (row tile, k
// block) that hold such an element.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "matrix_plan.hpp"

namespace wld {
namespace matrix_banded_plan {

constexpr uint32_t kSide = 64;
constexpr uint64_t kMaxSites = 4194304;  // tile indices are 16-bit (ta << 16 | tb)
constexpr uint32_t kMinStripRows = 64;

struct Rows {
    uint32_t r0, r1;
};

// what validate() refuses (capi.hip words the message)
enum Refusal { kOk = 0, kEmpty, kRange, kStat, kDtype, kFlags, kLd, kNull, kWidth, kSites };

// max over a of hi[a] - a: the bandwidth below which an in-window pair would be
// dropped.  hi: the window's limits (window_plan::limits; null: no window).
inline uint32_t width(uint32_t L, const uint32_t *hi) {
    if (!L) return 0;
    if (!hi) return L - 1;
    uint32_t w = 0;
    for (uint32_t a = 0; a < L; ++a) w = std::max(w, hi[a] - a);
    return w;
}

// The caller's row range (an end of 0 = L), bandwidth and layout, checked;
// *out = the rows with their end resolved.  needed: width() of the window.
inline Refusal validate(uint64_t L, uint32_t rb, uint32_t re, uint32_t K, uint32_t needed, int stat, int dtype,
                        int flags, size_t ld, bool have_dst, Rows *out) {
    if (stat < matrix_plan::kStatR2 || stat > matrix_plan::kStatDPrime) return kStat;
    if (dtype != matrix_plan::kF32 && dtype != matrix_plan::kF16) return kDtype;
    if (flags & ~matrix_plan::kZeroMissing) return kFlags;
    if (!have_dst) return kNull;
    if (L > kMaxSites) return kSites;
    if (re > L || rb > L) return kRange;
    const uint32_t r1 = re ? re : (uint32_t)L;
    if (rb >= r1) return kEmpty;
    *out = Rows{rb, r1};
    if (K < needed) return kWidth;
    return (uint64_t)ld < (uint64_t)K + 1 ? kLd : kOk;
}

// The listed tiles of row tile ta: those of the offsets tb - ta in [c0, c1)
// (c1 <= c0: none).  c0 is 1 where the diagonal tile holds no in-window pair
// and a later one does.
struct Cover {
    uint32_t c0, c1;
};
inline Cover cover(uint32_t L, const uint32_t *hi, uint32_t ta) {
    const uint32_t a0 = ta * kSide;
    if (a0 >= L) return Cover{0, 0};
    const uint32_t a1 = std::min<uint64_t>(L, (uint64_t)a0 + kSide);
    const bool diag = matrix_plan::tile_has_pair(L, hi, ta, ta);
    const uint32_t reach = (hi ? hi[a1 - 1] : L - 1) / kSide;  // the last tile an a of the row tile reaches
    if (reach > ta) return Cover{diag ? 0u : 1u, reach - ta + 1};
    return Cover{0, diag ? 1u : 0u};
}
// is element k of the row at offset i (0..63) of its row tile written by a listed tile?
WLD_MATRIX_HD inline bool covered(uint32_t c0, uint32_t c1, uint32_t i, uint32_t k) {
    const uint64_t s = (uint64_t)i + k;  // (the column's offset from the row tile's first site)
    return s >= (uint64_t)c0 * kSide && s < (uint64_t)c1 * kSide;
}

// a 64 x 64 block of the band (rows 64 ta .., elements k = 64 kb ..) that holds
// an element no listed tile writes, with its row tile's cover
struct FillBlock {
    uint32_t ta, kb, c0, c1;
};
struct Plan {
    std::vector<uint32_t> tiles;  // ta << 16 | tb, (ta, tb) order: the tiles launched
    std::vector<FillBlock> fill;
};
// The tiles of the row tiles meeting `rows` that hold an in-window pair, and
// the blocks of rows x [0, K] with an element none of them writes.  Every
// element lies in exactly one listed tile's run or is uncovered in exactly one
// fill block.
inline Plan plan(uint32_t L, const uint32_t *hi, const Rows &rows, uint32_t K) {
    Plan p;
    for (uint32_t ta = rows.r0 / kSide; ta <= (rows.r1 - 1) / kSide; ++ta) {
        const Cover c = cover(L, hi, ta);
        for (uint32_t t = c.c0; t < c.c1; ++t) p.tiles.push_back((ta << 16) | (ta + t));
        const uint32_t imin = std::max(rows.r0, ta * kSide) - ta * kSide;
        const uint32_t imax = std::min(rows.r1, ta * kSide + kSide) - 1 - ta * kSide;
        for (uint64_t kb = 0; kb <= K / kSide; ++kb) {
            const uint64_t klo = kb * kSide, khi = std::min<uint64_t>(klo + kSide - 1, K);
            const bool whole = c.c1 > c.c0 && klo + imin >= (uint64_t)c.c0 * kSide && khi + imax < (uint64_t)c.c1 * kSide;
            if (!whole) p.fill.push_back(FillBlock{ta, (uint32_t)kb, c.c0, c.c1});
        }
    }
    return p;
}

// the in-window pairs a < b with a in rows: what the launches over rows count
inline uint64_t count_pairs(uint32_t L, const uint32_t *hi, const Rows &rows) {
    uint64_t n = 0;
    for (uint32_t a = rows.r0; a < rows.r1; ++a) n += (hi ? hi[a] : L - 1) - a;
    return n;
}

// The host call's strips: whole rows, as many per strip as batch_bytes holds
// (at least kMinStripRows, at most the range's).  A pair belongs to the strip
// of its row a.
inline uint32_t strip_rows(const Rows &q, uint32_t K, size_t elem_bytes, uint64_t batch_bytes) {
    const uint64_t row_bytes = ((uint64_t)K + 1) * elem_bytes;
    const uint64_t fit = std::max<uint64_t>(batch_bytes / row_bytes, kMinStripRows);
    return (uint32_t)std::min<uint64_t>(fit, q.r1 - q.r0);
}
inline std::vector<Rows> strips(const Rows &q, uint32_t K, size_t elem_bytes, uint64_t batch_bytes) {
    const uint32_t n = strip_rows(q, K, elem_bytes, batch_bytes);
    std::vector<Rows> s;
    for (uint64_t r = q.r0; r < q.r1; r += n) s.push_back(Rows{(uint32_t)r, (uint32_t)std::min<uint64_t>(r + n, q.r1)});
    return s;
}

}  // namespace matrix_banded_plan
}  // namespace wld
