// Host-side plan of the dense LD matrix (capi.hip wld_run_matrix_device /
// wld_run_matrix): the argument checks, the tile list of a site rectangle
// under the window with the images each tile writes, the 64x64 blocks of the
// rectangle that no listed tile writes (the fill list), the band split of the
// host call, and the rule that counts a pair with both orientations in the
// rectangle once.  Header-only and free of HIP types so that the host test
// (tests/cpp/matrix_plan_check.cpp) checks the same code; images() and
// counts_here() are also what the kernel evaluates (pair_matrix.hip).
//
// The rectangle holds entries (u, v), u in [r0, r1) (rows), v in [c0, c1)
// (columns), loaded site indices.  A pair a < b is computed once, by tile
// (ta, tb) = (a / 64, b / 64), ta <= tb.  The tile's direct image is the set
// of entries (a, b) — rows in block ta, columns in block tb — and its mirrored
// image the entries (b, a) — rows in block tb, columns in block ta.  A diagonal
// tile's two images are the same block: it writes it once (direct supplies
// a < b, mirror a > b, the diagonal rule a == b).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define WLD_MATRIX_HD __host__ __device__
#else
#define WLD_MATRIX_HD
#endif

namespace wld {
namespace matrix_plan {

constexpr uint32_t kSide = 64;
constexpr uint32_t kDirect = 1, kMirror = 2;  // images()
constexpr int kStatR2 = 0, kStatR = 1, kStatD = 2, kStatDPrime = 3;  // WLD_MATRIX_*
constexpr int kF32 = 0, kF16 = 1;
constexpr int kZeroMissing = 1;
constexpr uint64_t kDefaultBatchBytes = 1ull << 30;  // WLD_OPT_MATRIX_BATCH_BYTES
constexpr uint32_t kMinBandRows = 64;

struct Rect {
    uint32_t r0, r1, c0, c1;
};

// what validate() refuses (capi.hip words the message)
enum Refusal { kOk = 0, kEmpty, kRange, kStat, kDtype, kFlags, kLd, kNull };

// The caller's rectangle (an end of 0 = L) and layout, checked; *out = the
// rectangle with its ends resolved.
inline Refusal validate(uint64_t L, uint32_t rb, uint32_t re, uint32_t cb, uint32_t ce, int stat, int dtype, int flags,
                        size_t ld, bool have_dst, Rect *out) {
    if (stat < kStatR2 || stat > kStatDPrime) return kStat;
    if (dtype != kF32 && dtype != kF16) return kDtype;
    if (flags & ~kZeroMissing) return kFlags;
    if (!have_dst) return kNull;
    if (re > L || ce > L || rb > L || cb > L) return kRange;
    const uint32_t r1 = re ? re : (uint32_t)L, c1 = ce ? ce : (uint32_t)L;
    if (rb >= r1 || cb >= c1) return kEmpty;
    *out = Rect{rb, r1, cb, c1};
    return ld < (size_t)(c1 - cb) ? kLd : kOk;
}

WLD_MATRIX_HD inline bool block_meets(uint32_t t, uint32_t lo, uint32_t hi) {  // sites [64 t, 64 t + 64) and [lo, hi)
    return t * kSide < hi && t * kSide + kSide > lo;
}
// the images of tile (ta, tb), ta <= tb, that hold an entry of the rectangle
WLD_MATRIX_HD inline uint32_t images(const Rect &q, uint32_t ta, uint32_t tb) {
    uint32_t m = 0;
    if (block_meets(ta, q.r0, q.r1) && block_meets(tb, q.c0, q.c1)) m |= kDirect;
    if (block_meets(tb, q.r0, q.r1) && block_meets(ta, q.c0, q.c1)) m |= kMirror;
    return m;
}

// The counting rule.  A pair a < b has the entries (a, b) and (b, a) of the
// call's rectangle `full` at most; its canonical entry is (a, b) where that is
// inside, else (b, a).  A launch over `band` (full's columns, a sub-range of
// its rows; the device call: band == full) counts the pair iff the canonical
// entry lies in the band: every pair with an entry counts in exactly one band.
WLD_MATRIX_HD inline bool counts_here(const Rect &full, const Rect &band, uint32_t a, uint32_t b) {
    const bool a_col = a >= full.c0 && a < full.c1, b_col = b >= full.c0 && b < full.c1;
    if (a >= full.r0 && a < full.r1 && b_col) return a >= band.r0 && a < band.r1;
    if (b >= full.r0 && b < full.r1 && a_col) return b >= band.r0 && b < band.r1;
    return false;
}

// the in-window partners b of a (a < b <= hi_a) inside [lo, up)
inline uint64_t partners_in(uint32_t a, uint32_t hi_a, uint32_t lo, uint32_t up) {
    const uint64_t s = std::max<uint64_t>((uint64_t)a + 1, lo), e = std::min<uint64_t>((uint64_t)hi_a + 1, up);
    return e > s ? e - s : 0;
}
// The pairs the rule counts over the whole rectangle: those with an entry in
// it.  hi: the window's limits (window_plan::limits; null: no window).
inline uint64_t count_pairs(uint32_t L, const uint32_t *hi, const Rect &q) {
    const uint32_t i0 = std::max(q.r0, q.c0), i1 = std::min(q.r1, q.c1);  // sites that are a row and a column
    uint64_t n = 0;
    for (uint32_t a = 0; a < L; ++a) {
        const uint32_t h = hi ? hi[a] : L - 1;
        const bool row = a >= q.r0 && a < q.r1, col = a >= q.c0 && a < q.c1;
        if (row) n += partners_in(a, h, q.c0, q.c1);
        if (col) n += partners_in(a, h, q.r0, q.r1);
        if (row && col && i0 < i1) n -= partners_in(a, h, i0, i1);  // (both entries inside: once)
    }
    return n;
}

// does tile (ta, tb) hold an in-window pair? (window_plan::tile_in_window's rule)
inline bool tile_has_pair(uint32_t L, const uint32_t *hi, uint32_t ta, uint32_t tb) {
    const uint32_t a0 = ta * kSide, a1 = std::min(L, a0 + kSide);
    if (a0 >= L || (uint64_t)tb * kSide >= L) return false;
    if (tb > ta) return (hi ? hi[a1 - 1] : L - 1) >= tb * kSide;
    for (uint32_t a = a0; a + 1 < a1; ++a)
        if ((hi ? hi[a] : L - 1) > a) return true;
    return false;
}

struct Plan {
    std::vector<uint32_t> tiles;  // ta << 16 | tb, (ta, tb) order: the tiles launched
    std::vector<uint32_t> fill;   // bi << 16 | bj: blocks (rows 64 bi.., columns 64 bj..) no listed tile writes
};
// The tiles that hold an in-window pair and an image meeting `band`, and the
// blocks meeting the band that none of them writes.  Every entry of the band
// lies in exactly one written image or fill block.
inline Plan plan(uint32_t L, const uint32_t *hi, const Rect &band) {
    Plan p;
    const uint32_t bi0 = band.r0 / kSide, bi1 = (band.r1 - 1) / kSide, bj0 = band.c0 / kSide, bj1 = (band.c1 - 1) / kSide;
    for (uint32_t bi = bi0; bi <= bi1; ++bi)
        for (uint32_t bj = bj0; bj <= bj1; ++bj) {
            const uint32_t ta = std::min(bi, bj), tb = std::max(bi, bj);
            if (!tile_has_pair(L, hi, ta, tb)) p.fill.push_back((bi << 16) | bj);
            // (a tile whose two images both meet the band is listed once: at its direct block)
            else if (bi <= bj || !(images(band, ta, tb) & kDirect)) p.tiles.push_back((ta << 16) | tb);
        }
    std::sort(p.tiles.begin(), p.tiles.end());
    return p;
}

// The host call's bands: whole rows [r0 + k rows, ...), as many per band as
// batch_bytes holds (at least kMinBandRows, at most the rectangle's).
inline uint32_t band_rows(const Rect &q, size_t elem_bytes, uint64_t batch_bytes) {
    const uint64_t row_bytes = (uint64_t)(q.c1 - q.c0) * elem_bytes;
    const uint64_t fit = std::max<uint64_t>(batch_bytes / row_bytes, kMinBandRows);
    return (uint32_t)std::min<uint64_t>(fit, q.r1 - q.r0);
}
inline std::vector<Rect> bands(const Rect &q, size_t elem_bytes, uint64_t batch_bytes) {
    const uint32_t n = band_rows(q, elem_bytes, batch_bytes);
    std::vector<Rect> b;
    for (uint64_t r = q.r0; r < q.r1; r += n) b.push_back(Rect{(uint32_t)r, (uint32_t)std::min<uint64_t>(r + n, q.r1), q.c0, q.c1});
    return b;
}

}  // namespace matrix_plan
}  // namespace wld
