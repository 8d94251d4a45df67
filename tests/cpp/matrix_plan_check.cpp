// Host-only check of weightedld_amd/csrc/matrix_plan.hpp against brute force:
// the argument validation, the tile list with its images and the fill list
// (every entry of a band written exactly once, by the tile of its pair where
// that tile holds an in-window pair, else by a fill block), the counting rule
// (a pair with an entry counts in exactly one band, once) and the band split.
// Prints "OK" and returns 0, or the first mismatch and 1.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "matrix_plan.hpp"
#include "window_plan.hpp"

namespace mp = wld::matrix_plan;
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
    mp::Rect q{};
    CHECK(mp::validate(100, 0, 0, 0, 0, 1, 0, 0, 100, true, &q) == mp::kOk && q.r0 == 0 && q.r1 == 100 && q.c0 == 0 &&
              q.c1 == 100, "full square");
    CHECK(mp::validate(100, 3, 50, 61, 70, 3, 1, 1, 9, true, &q) == mp::kOk && q.r0 == 3 && q.r1 == 50 && q.c0 == 61 &&
              q.c1 == 70, "rectangle");
    CHECK(mp::validate(100, 3, 50, 61, 70, 0, 0, 0, 8, true, &q) == mp::kLd, "ld below the width");
    CHECK(mp::validate(100, 3, 3, 0, 0, 0, 0, 0, 100, true, &q) == mp::kEmpty, "empty rows");
    CHECK(mp::validate(100, 5, 3, 0, 0, 0, 0, 0, 100, true, &q) == mp::kEmpty, "reversed rows");
    CHECK(mp::validate(100, 0, 0, 100, 0, 0, 0, 0, 100, true, &q) == mp::kEmpty, "columns begin at L");
    CHECK(mp::validate(100, 0, 101, 0, 0, 0, 0, 0, 200, true, &q) == mp::kRange, "row end past L");
    CHECK(mp::validate(100, 0, 0, 101, 0, 0, 0, 0, 200, true, &q) == mp::kRange, "column begin past L");
    CHECK(mp::validate(0, 0, 0, 0, 0, 0, 0, 0, 1, true, &q) == mp::kEmpty, "no site");
    CHECK(mp::validate(100, 0, 0, 0, 0, 4, 0, 0, 100, true, &q) == mp::kStat, "stat 4");
    CHECK(mp::validate(100, 0, 0, 0, 0, -1, 0, 0, 100, true, &q) == mp::kStat, "stat -1");
    CHECK(mp::validate(100, 0, 0, 0, 0, 0, 2, 0, 100, true, &q) == mp::kDtype, "dtype 2");
    CHECK(mp::validate(100, 0, 0, 0, 0, 0, 0, 2, 100, true, &q) == mp::kFlags, "flag bit 2");
    CHECK(mp::validate(100, 0, 0, 0, 0, 0, 0, 0, 100, false, &q) == mp::kNull, "null destination");
    return 0;
}

// one rectangle split into bands: the plans, the counts and the counting rule
static int check_rect(uint32_t L, const std::vector<uint32_t> *hi, const mp::Rect &full, size_t eb, uint64_t batch) {
    const uint32_t *h = hi ? hi->data() : nullptr;
    const uint32_t W = full.c1 - full.c0, T = (L + 63) / 64;
    // brute force: the tiles holding an in-window pair
    std::vector<uint8_t> has((size_t)T * T, 0);
    for (uint32_t a = 0; a < L; ++a)
        for (uint32_t b = a + 1; b < L; ++b)
            if (in_window(hi, a, b)) has[(size_t)(a / 64) * T + b / 64] = 1;
    for (uint32_t ta = 0; ta < T; ++ta)
        for (uint32_t tb = ta; tb < T; ++tb)
            CHECK(mp::tile_has_pair(L, h, ta, tb) == (has[(size_t)ta * T + tb] != 0), "tile_has_pair(%u, %u) L %u", ta, tb, L);

    const std::vector<mp::Rect> bands = mp::bands(full, eb, batch);
    CHECK(!bands.empty() && bands.front().r0 == full.r0 && bands.back().r1 == full.r1, "bands' ends");
    const uint32_t rows = mp::band_rows(full, eb, batch);
    for (size_t k = 0; k < bands.size(); ++k) {
        const mp::Rect &b = bands[k];
        CHECK(b.c0 == full.c0 && b.c1 == full.c1 && b.r0 < b.r1, "band %zu's shape", k);
        CHECK(k == 0 || b.r0 == bands[k - 1].r1, "band %zu does not follow its predecessor", k);
        CHECK(k + 1 == bands.size() || b.r1 - b.r0 == rows, "band %zu has %u rows, not %u", k, b.r1 - b.r0, rows);
        CHECK(b.r1 - b.r0 <= rows, "band %zu too tall", k);
    }
    CHECK(rows == full.r1 - full.r0 || rows >= mp::kMinBandRows, "a band of %u rows", rows);
    CHECK(rows == full.r1 - full.r0 || rows == mp::kMinBandRows || (uint64_t)rows * W * eb <= batch,
          "a band of %u rows x %u exceeds %llu bytes", rows, W, (unsigned long long)batch);
    CHECK(rows == full.r1 - full.r0 || (uint64_t)(rows + 1) * W * eb > batch, "a band of %u rows is not the largest", rows);

    uint64_t counted = 0;
    std::vector<uint32_t> pair_bands((size_t)L * L, 0);  // bands that count pair (a, b)
    for (const mp::Rect &band : bands) {
        const mp::Plan p = mp::plan(L, h, band);
        const uint32_t H = band.r1 - band.r0;
        std::vector<uint8_t> cover((size_t)H * W, 0);
        auto mark = [&](uint32_t bi, uint32_t bj) {  // block (rows 64 bi.., columns 64 bj..) clipped to the band
            for (uint32_t u = bi * 64; u < bi * 64 + 64; ++u)
                for (uint32_t v = bj * 64; v < bj * 64 + 64; ++v)
                    if (u >= band.r0 && u < band.r1 && v >= band.c0 && v < band.c1) cover[(size_t)(u - band.r0) * W + v - band.c0]++;
        };
        std::set<uint32_t> seen;
        for (size_t i = 0; i < p.tiles.size(); ++i) {
            const uint32_t ta = p.tiles[i] >> 16, tb = p.tiles[i] & 0xFFFFu;
            CHECK(ta <= tb && tb < T, "tile (%u, %u) out of range", ta, tb);
            CHECK(i == 0 || p.tiles[i - 1] < p.tiles[i], "the tile list is not in (ta, tb) order");
            CHECK(seen.insert(p.tiles[i]).second, "tile (%u, %u) listed twice", ta, tb);
            CHECK(has[(size_t)ta * T + tb], "tile (%u, %u) holds no in-window pair", ta, tb);
            const uint32_t img = mp::images(band, ta, tb);
            CHECK(img != 0, "tile (%u, %u) has no image in the band", ta, tb);
            if (ta == tb) mark(ta, ta);
            else {
                if (img & mp::kDirect) mark(ta, tb);
                if (img & mp::kMirror) mark(tb, ta);
            }
        }
        for (uint32_t e : p.fill) {
            const uint32_t bi = e >> 16, bj = e & 0xFFFFu;
            CHECK(mp::block_meets(bi, band.r0, band.r1) && mp::block_meets(bj, band.c0, band.c1), "fill block (%u, %u) misses the band", bi, bj);
            CHECK(!has[(size_t)std::min(bi, bj) * T + std::max(bi, bj)], "fill block (%u, %u) belongs to a tile with a pair", bi, bj);
            mark(bi, bj);
        }
        for (uint32_t u = band.r0; u < band.r1; ++u)
            for (uint32_t v = band.c0; v < band.c1; ++v)
                CHECK(cover[(size_t)(u - band.r0) * W + v - band.c0] == 1, "entry (%u, %u) written %u times (L %u, band rows [%u, %u))", u,
                      v, cover[(size_t)(u - band.r0) * W + v - band.c0], L, band.r0, band.r1);
        // every tile that holds a pair and an image is listed
        for (uint32_t ta = 0; ta < T; ++ta)
            for (uint32_t tb = ta; tb < T; ++tb)
                if (has[(size_t)ta * T + tb] && mp::images(band, ta, tb))
                    CHECK(seen.count((ta << 16) | tb), "tile (%u, %u) is missing", ta, tb);
        // the pairs this band's launch counts: only through a listed tile
        for (uint32_t a = 0; a < L; ++a)
            for (uint32_t b = a + 1; b < L; ++b)
                if (in_window(hi, a, b) && mp::counts_here(full, band, a, b)) {
                    CHECK(seen.count(((a / 64) << 16) | (b / 64)), "pair (%u, %u) counts in a band that does not list its tile", a, b);
                    pair_bands[(size_t)a * L + b]++;
                    counted++;
                }
    }
    uint64_t brute = 0;
    for (uint32_t a = 0; a < L; ++a)
        for (uint32_t b = a + 1; b < L; ++b) {
            const bool e1 = a >= full.r0 && a < full.r1 && b >= full.c0 && b < full.c1;
            const bool e2 = b >= full.r0 && b < full.r1 && a >= full.c0 && a < full.c1;
            const bool entry = in_window(hi, a, b) && (e1 || e2);
            brute += entry;
            CHECK(pair_bands[(size_t)a * L + b] == (entry ? 1u : 0u), "pair (%u, %u) counted %u times", a, b, pair_bands[(size_t)a * L + b]);
        }
    CHECK(counted == brute, "the bands count %llu pairs; brute force %llu", (unsigned long long)counted, (unsigned long long)brute);
    CHECK(mp::count_pairs(L, h, full) == brute, "count_pairs %llu; brute force %llu", (unsigned long long)mp::count_pairs(L, h, full),
          (unsigned long long)brute);
    return 0;
}

int main() {
    if (check_validate()) return 1;
    std::mt19937_64 rng(0x4d41545249584cull);
    auto U = [&](uint32_t lo, uint32_t hi) { return (uint32_t)(lo + rng() % (hi - lo + 1)); };
    // the shapes of the GPU tests, then random ones
    struct Fixed { uint32_t L, r0, r1, c0, c1; } fixed[] = {
        {130, 0, 130, 0, 130}, {130, 3, 129, 61, 70}, {130, 70, 130, 0, 60}, {130, 50, 100, 60, 130},
        {130, 64, 65, 64, 65}, {130, 5, 6, 100, 101}, {600, 77, 78, 0, 600}, {600, 0, 600, 333, 334},
        {129, 0, 129, 0, 129}, {64, 0, 64, 0, 64}, {1, 0, 1, 0, 1}, {65, 64, 65, 0, 65}};
    for (const Fixed &f : fixed)
        for (uint64_t batch : {1ull << 30, 1ull, 40000ull})
            if (check_rect(f.L, nullptr, mp::Rect{f.r0, f.r1, f.c0, f.c1}, 4, batch)) return 1;
    for (int it = 0; it < 60; ++it) {
        const uint32_t L = it < 6 ? U(1, 70) : U(1, 420);
        std::vector<uint32_t> pos(L);
        uint32_t p = U(0, 5);
        for (uint32_t i = 0; i < L; ++i) pos[i] = (p += U(0, 3) * (U(0, 9) == 0 ? 40 : 1));
        const int mode = it % 4;  // no window, K, D, both
        const uint64_t K = (mode & 1) ? U(1, 150) : 0, D = (mode & 2) ? U(0, 1) ? U(1, 30) : U(30, 400) : 0;
        const std::vector<uint32_t> hi = wp::limits(pos.data(), L, D, K);
        uint32_t r0 = U(0, L - 1), r1 = U(r0 + 1, L), c0 = U(0, L - 1), c1 = U(c0 + 1, L);
        if (it % 5 == 0) r0 = c0 = 0, r1 = c1 = L;
        const size_t eb = (it & 1) ? 2 : 4;
        const uint64_t batch = it % 3 == 0 ? 1ull << 30 : it % 3 == 1 ? 1 : (uint64_t)U(64, 200) * (c1 - c0) * eb + U(0, 7);
        if (check_rect(L, mode ? &hi : nullptr, mp::Rect{r0, r1, c0, c1}, eb, batch)) {
            printf("  (case %d: L %u, D %llu, K %llu, rows [%u, %u), columns [%u, %u), batch %llu)\n", it, L,
                   (unsigned long long)D, (unsigned long long)K, r0, r1, c0, c1, (unsigned long long)batch);
            return 1;
        }
    }
    printf("OK\n");
    return 0;
}
