// Host-only check of weightedld_amd/csrc/matrix_banded_plan.hpp against brute
// force: the argument validation, the width a window needs, the tile list of a
// row range, the fill description (every element of the rows x [0, K] block
// written exactly once: by the listed tile of its column where there is one,
// else by a listed fill block), the pair count of a row range and the strip
// split of the host call (a pair counts in exactly one strip, that of its row
// a).  Prints "OK" and returns 0, or the first mismatch and 1.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "matrix_banded_plan.hpp"
#include "window_plan.hpp"

namespace bp = wld::matrix_banded_plan;
namespace wp = wld::window_plan;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);   \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
            return 1;                                     \
        }                                                 \
    } while (0)

static bool in_window(const std::vector<uint32_t> *hi, uint32_t a, uint32_t b) { return !hi || b <= (*hi)[a]; }

static int check_validate() {
    bp::Rows q{};
    CHECK(bp::validate(100, 0, 0, 99, 99, 1, 0, 0, 100, true, &q) == bp::kOk && q.r0 == 0 && q.r1 == 100, "all rows");
    CHECK(bp::validate(100, 3, 50, 20, 7, 3, 1, 1, 21, true, &q) == bp::kOk && q.r0 == 3 && q.r1 == 50, "a row range");
    CHECK(bp::validate(100, 3, 50, 20, 7, 0, 0, 0, 20, true, &q) == bp::kLd, "ld below K + 1");
    CHECK(bp::validate(100, 3, 50, 6, 7, 0, 0, 0, 100, true, &q) == bp::kWidth, "K below the needed width");
    CHECK(bp::validate(100, 0, 0, 0xFFFFFFFFu, 7, 0, 0, 0, 100, true, &q) == bp::kLd, "K + 1 does not wrap");
    CHECK(bp::validate(100, 3, 3, 9, 0, 0, 0, 0, 100, true, &q) == bp::kEmpty, "empty rows");
    CHECK(bp::validate(100, 5, 3, 9, 0, 0, 0, 0, 100, true, &q) == bp::kEmpty, "reversed rows");
    CHECK(bp::validate(100, 100, 0, 9, 0, 0, 0, 0, 100, true, &q) == bp::kEmpty, "rows begin at L");
    CHECK(bp::validate(100, 0, 101, 9, 0, 0, 0, 0, 100, true, &q) == bp::kRange, "row end past L");
    CHECK(bp::validate(100, 101, 0, 9, 0, 0, 0, 0, 100, true, &q) == bp::kRange, "row begin past L");
    CHECK(bp::validate(0, 0, 0, 0, 0, 0, 0, 0, 1, true, &q) == bp::kEmpty, "no site");
    CHECK(bp::validate(100, 0, 0, 99, 99, 4, 0, 0, 100, true, &q) == bp::kStat, "stat 4");
    CHECK(bp::validate(100, 0, 0, 99, 99, -1, 0, 0, 100, true, &q) == bp::kStat, "stat -1");
    CHECK(bp::validate(100, 0, 0, 99, 99, 0, 2, 0, 100, true, &q) == bp::kDtype, "dtype 2");
    CHECK(bp::validate(100, 0, 0, 99, 99, 0, 0, 2, 100, true, &q) == bp::kFlags, "flag bit 2");
    CHECK(bp::validate(100, 0, 0, 99, 99, 0, 0, 0, 100, false, &q) == bp::kNull, "null destination");
    CHECK(bp::validate(bp::kMaxSites, 0, 0, 9, 9, 0, 0, 0, 10, true, &q) == bp::kOk, "the most sites");
    CHECK(bp::validate(bp::kMaxSites + 1, 0, 0, 9, 9, 0, 0, 0, 10, true, &q) == bp::kSites, "too many sites");
    return 0;
}

// one row range under one window and bandwidth, split into strips
static int check_rows(uint32_t L, const std::vector<uint32_t> *hi, const bp::Rows &full, uint32_t K, size_t eb,
                      uint64_t batch) {
    const uint32_t *h = hi ? hi->data() : nullptr;
    const uint32_t T = (L + 63) / 64, W = K + 1;
    // brute force: the width, and the tiles holding an in-window pair
    uint32_t width = 0;
    std::vector<uint8_t> has((size_t)T * T, 0);
    for (uint32_t a = 0; a < L; ++a)
        for (uint32_t b = a + 1; b < L; ++b)
            if (in_window(hi, a, b)) {
                has[(size_t)(a / 64) * T + b / 64] = 1;
                width = std::max(width, b - a);
            }
    CHECK(bp::width(L, h) == width, "width %u; brute force %u (L %u)", bp::width(L, h), width, L);
    CHECK(K >= width, "the case's K %u is below the width %u", K, width);

    const std::vector<bp::Rows> strips = bp::strips(full, K, eb, batch);
    CHECK(!strips.empty() && strips.front().r0 == full.r0 && strips.back().r1 == full.r1, "strips' ends");
    const uint32_t rows = bp::strip_rows(full, K, eb, batch);
    for (size_t k = 0; k < strips.size(); ++k) {
        const bp::Rows &s = strips[k];
        CHECK(s.r0 < s.r1, "strip %zu is empty", k);
        CHECK(k == 0 || s.r0 == strips[k - 1].r1, "strip %zu does not follow its predecessor", k);
        CHECK(k + 1 == strips.size() || s.r1 - s.r0 == rows, "strip %zu has %u rows, not %u", k, s.r1 - s.r0, rows);
        CHECK(s.r1 - s.r0 <= rows, "strip %zu too tall", k);
    }
    const uint32_t H = full.r1 - full.r0;
    CHECK(rows == H || rows >= bp::kMinStripRows, "a strip of %u rows", rows);
    CHECK(rows == H || rows == bp::kMinStripRows || (uint64_t)rows * W * eb <= batch, "a strip of %u rows x %u exceeds %llu bytes",
          rows, W, (unsigned long long)batch);
    CHECK(rows == H || (uint64_t)(rows + 1) * W * eb > batch, "a strip of %u rows is not the largest", rows);

    uint64_t counted = 0, brute = 0;
    for (const bp::Rows &s : strips) {
        const bp::Plan p = bp::plan(L, h, s, K);
        const uint32_t SH = s.r1 - s.r0;
        std::vector<uint8_t> cover((size_t)SH * W, 0);
        std::set<uint32_t> seen;
        for (size_t i = 0; i < p.tiles.size(); ++i) {
            const uint32_t ta = p.tiles[i] >> 16, tb = p.tiles[i] & 0xFFFFu;
            CHECK(ta <= tb && tb < T, "tile (%u, %u) out of range", ta, tb);
            CHECK(i == 0 || p.tiles[i - 1] < p.tiles[i], "the tile list is not in (ta, tb) order");
            CHECK(seen.insert(p.tiles[i]).second, "tile (%u, %u) listed twice", ta, tb);
            CHECK(has[(size_t)ta * T + tb], "tile (%u, %u) holds no in-window pair", ta, tb);
            CHECK(ta * 64 < s.r1 && ta * 64 + 64 > s.r0, "tile (%u, %u) misses the rows", ta, tb);
            // the kernel's store rule: row u of the tile, the columns b of block tb with u <= b, b - u <= K
            for (uint32_t u = std::max(ta * 64, s.r0); u < std::min(ta * 64 + 64, s.r1); ++u)
                for (uint32_t b = tb * 64; b < tb * 64 + 64; ++b)
                    if (b >= u && b - u <= K) cover[(size_t)(u - s.r0) * W + (b - u)]++;
        }
        // every tile that holds a pair and meets the rows is listed
        for (uint32_t ta = s.r0 / 64; ta <= (s.r1 - 1) / 64; ++ta)
            for (uint32_t tb = ta; tb < T; ++tb)
                if (has[(size_t)ta * T + tb]) CHECK(seen.count((ta << 16) | tb), "tile (%u, %u) is missing", ta, tb);
        std::set<uint64_t> blocks;
        for (const bp::FillBlock &e : p.fill) {
            CHECK(e.ta * 64 < s.r1 && e.ta * 64 + 64 > s.r0 && (uint64_t)e.kb * 64 <= K, "fill block (%u, %u) misses the block", e.ta, e.kb);
            CHECK(blocks.insert(((uint64_t)e.ta << 32) | e.kb).second, "fill block (%u, %u) listed twice", e.ta, e.kb);
            const bp::Cover c = bp::cover(L, h, e.ta);
            CHECK(c.c0 == e.c0 && c.c1 == e.c1, "fill block (%u, %u) carries another cover", e.ta, e.kb);
            // the fill kernel's rule
            for (uint32_t row = 0; row < 64; ++row)
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const uint64_t k = (uint64_t)e.kb * 64 + lane;
                    const uint32_t u = e.ta * 64 + row;
                    if (k > K || u < s.r0 || u >= s.r1) continue;
                    if (!bp::covered(e.c0, e.c1, row, (uint32_t)k)) cover[(size_t)(u - s.r0) * W + k]++;
                }
        }
        for (uint32_t u = s.r0; u < s.r1; ++u)
            for (uint32_t k = 0; k <= K; ++k)
                CHECK(cover[(size_t)(u - s.r0) * W + k] == 1, "element (%u, k %u) written %u times (L %u, rows [%u, %u), K %u)", u, k,
                      cover[(size_t)(u - s.r0) * W + k], L, s.r0, s.r1, K);
        // covered() names exactly the elements a listed tile writes
        for (uint32_t u = s.r0; u < s.r1; ++u) {
            const bp::Cover c = bp::cover(L, h, u / 64);
            for (uint32_t k = 0; k <= K; ++k) {
                const uint64_t b = (uint64_t)u + k;
                const bool by_tile = b / 64 < T && seen.count(((u / 64) << 16) | (uint32_t)(b / 64));
                CHECK(bp::covered(c.c0, c.c1, u % 64, k) == by_tile, "covered(%u, k %u) is %d (L %u)", u, k, !by_tile, L);
            }
        }
        // the pairs the strip's launch counts: those of its rows, each through a listed tile
        uint64_t here = 0;
        for (uint32_t a = s.r0; a < s.r1; ++a)
            for (uint32_t b = a + 1; b < L; ++b)
                if (in_window(hi, a, b)) {
                    CHECK(seen.count(((a / 64) << 16) | (b / 64)), "pair (%u, %u) counts in a strip that does not list its tile", a, b);
                    CHECK(b - a <= K, "pair (%u, %u) lies beyond the bandwidth %u", a, b, K);
                    here++;
                }
        CHECK(bp::count_pairs(L, h, s) == here, "count_pairs of rows [%u, %u): %llu; brute force %llu", s.r0, s.r1,
              (unsigned long long)bp::count_pairs(L, h, s), (unsigned long long)here);
        counted += here;
    }
    for (uint32_t a = full.r0; a < full.r1; ++a)
        for (uint32_t b = a + 1; b < L; ++b) brute += in_window(hi, a, b);
    CHECK(counted == brute && bp::count_pairs(L, h, full) == brute, "the strips count %llu pairs, count_pairs %llu; brute force %llu",
          (unsigned long long)counted, (unsigned long long)bp::count_pairs(L, h, full), (unsigned long long)brute);
    return 0;
}

int main() {
    if (check_validate()) return 1;
    CHECK(bp::width(0, nullptr) == 0, "width of no site");
    const uint32_t Ls[] = {1, 2, 63, 64, 65, 130, 600};
    const uint64_t batches[] = {1ull << 30, 1ull, 70000ull};
    for (uint32_t L : Ls) {
        // a map with repeated positions and gaps, for the distance window
        std::vector<uint32_t> pos(L);
        uint32_t p = 5;
        for (uint32_t i = 0; i < L; ++i) pos[i] = (p += (i % 7 == 3) ? 0 : (i % 61 == 60) ? 90 : (i % 5 == 0) ? 0 : 2);
        struct Win { uint64_t D, K; } wins[] = {{0, 0}, {0, 1}, {0, 63}, {0, 64}, {0, 65}, {40, 0}, {1, 0}, {40, 20}};
        for (const Win &w : wins) {
            const bool windowed = w.D || w.K;
            const std::vector<uint32_t> hi = wp::limits(pos.data(), L, w.D, w.K);
            const uint32_t need = bp::width(L, windowed ? hi.data() : nullptr);
            // all rows and unaligned row ranges; the needed width and surplus ones
            std::vector<bp::Rows> ranges = {{0, L}};
            if (L > 2) ranges.push_back({1, L - 1});
            if (L >= 130) ranges.push_back({37, 101}), ranges.push_back({64, 128}), ranges.push_back({L - 1, L});
            if (L >= 600) ranges.push_back({37, 201}), ranges.push_back({250, 600});
            for (const bp::Rows &r : ranges)
                for (uint32_t extra : {0u, 7u, 64u, 150u})
                    for (uint64_t batch : batches) {
                        if (extra > 7 && batch != batches[0]) continue;
                        if (check_rows(L, windowed ? &hi : nullptr, r, need + extra, (extra & 1) ? 2 : 4, batch)) {
                            printf("  (L %u, D %llu, K %llu, rows [%u, %u), bandwidth %u, batch %llu)\n", L, (unsigned long long)w.D,
                                   (unsigned long long)w.K, r.r0, r.r1, need + extra, (unsigned long long)batch);
                            return 1;
                        }
                    }
        }
    }
    {
        // only the pair (63, 64) is in the window: the first row tile's diagonal
        // tile is not listed, its next one is (Cover::c0 == 1)
        const uint32_t L = 130;
        std::vector<uint32_t> pos(L);
        for (uint32_t i = 0; i < L; ++i) pos[i] = 10 * i;
        pos[64] = pos[63];
        const std::vector<uint32_t> hi = wp::limits(pos.data(), L, 1, 0);
        const bp::Cover c = bp::cover(L, hi.data(), 0);
        CHECK(c.c0 == 1 && c.c1 == 2, "cover of the lone cross-tile pair: [%u, %u)", c.c0, c.c1);
        for (uint32_t K : {1u, 70u})
            for (const bp::Rows &r : {bp::Rows{0, L}, bp::Rows{60, 70}, bp::Rows{63, 64}})
                if (check_rows(L, &hi, r, K, 4, 1)) return 1;
    }
    printf("OK\n");
    return 0;
}
