// Host-only check of weightedld_amd/csrc/banded_chol_plan.hpp against brute
// force: per block row of 64 rows the panel's column extent, its 64-column
// blocks, the trailing window's block list with its clipped extents and the
// count of earlier block rows the forward solve reads; that every in-band
// element of the upper triangle lies in exactly one diagonal block or panel;
// and the launch count.  Prints "OK" and returns 0, or the first mismatch and 1.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "banded_chol_plan.hpp"

namespace cp = wld::banded_chol_plan;

#define CHECK(cond, ...)                                \
    do {                                                \
        if (!(cond)) {                                  \
            printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                        \
            printf("\n");                               \
            return 1;                                   \
        }                                               \
    } while (0)

// the panel columns of the block row at i0 by enumeration
static std::vector<uint32_t> brute_panel(uint32_t n, uint32_t K, uint32_t i0) {
    std::vector<uint32_t> cols;
    for (uint64_t j = (uint64_t)i0 + 64; j < n; ++j) {
        bool hit = false;
        for (uint64_t i = i0; i < (uint64_t)i0 + 64 && i < n && !hit; ++i) hit = j - i <= K;
        if (hit) cols.push_back((uint32_t)j);
    }
    return cols;
}

static int check_shape(uint32_t n, uint32_t K) {
    const uint32_t R = cp::block_rows(n);
    CHECK((uint64_t)R * 64 >= n && (uint64_t)(R - 1) * 64 < n, "block rows of n %u", n);
    uint64_t launches = 1, covered = 0, in_band = 0;
    std::vector<std::vector<uint32_t>> panels;
    for (uint32_t I = 0; I < R; ++I) {
        const cp::Step s = cp::step(n, K, I);
        const std::vector<uint32_t> cols = brute_panel(n, K, I * 64);
        panels.push_back(cols);
        CHECK(s.i0 == I * 64 && s.rows == (n - s.i0 < 64 ? n - s.i0 : 64), "rows of block row %u (n %u K %u)", I, n, K);
        CHECK(s.panel_end - s.panel_begin == cols.size(), "panel size of block row %u (n %u K %u): %u, brute %zu", I, n, K,
              s.panel_end - s.panel_begin, cols.size());
        CHECK(s.panel_begin <= s.panel_end && s.panel_end <= n, "panel order of block row %u (n %u K %u)", I, n, K);
        if (!cols.empty())
            CHECK(s.panel_begin == cols.front() && s.panel_end == cols.back() + 1 && s.rows == 64,
                  "panel extent of block row %u (n %u K %u)", I, n, K);
        std::set<uint32_t> blocks;
        for (uint32_t j : cols) blocks.insert((j - s.i0) / 64);
        CHECK(s.blocks == blocks.size() && (blocks.empty() || (*blocks.begin() == 1 && *blocks.rbegin() == s.blocks)),
              "panel blocks of block row %u (n %u K %u)", I, n, K);
        // the window: every pair of panel blocks a <= b, clipped at the panel's end
        const std::vector<cp::Block> w = cp::window(s);
        std::set<std::pair<uint32_t, uint32_t>> want, got;
        for (uint32_t a : blocks)
            for (uint32_t b : blocks)
                if (a <= b) want.insert({a, b});
        for (const cp::Block &b : w) {
            CHECK(got.insert({b.a, b.b}).second, "a window block twice (n %u K %u)", n, K);
            uint32_t r0 = ~0u, r1 = 0, c0 = ~0u, c1 = 0;
            for (uint32_t j : cols) {
                if ((j - s.i0) / 64 == b.a) r0 = j < r0 ? j : r0, r1 = j + 1;
                if ((j - s.i0) / 64 == b.b) c0 = j < c0 ? j : c0, c1 = j + 1;
            }
            CHECK(b.r0 == r0 && b.r1 == r1 && b.c0 == c0 && b.c1 == c1, "window block (%u, %u) extents (n %u K %u)", b.a,
                  b.b, n, K);
        }
        CHECK(got == want, "window block set of block row %u (n %u K %u)", I, n, K);
        // the earlier block rows whose panel meets this block row's columns
        uint32_t left = 0;
        for (uint32_t J = 0; J < I; ++J) {
            bool meets = false;
            for (uint32_t j : panels[J]) meets = meets || (j >= s.i0 && j < s.i0 + s.rows);
            left += meets;
        }
        CHECK(s.left == left, "left blocks of block row %u (n %u K %u): %u, brute %u", I, n, K, s.left, left);
        // the contiguous run just before I: the forward solve walks I - left .. I - 1
        for (uint32_t J = 0; J < I; ++J) {
            bool meets = false;
            for (uint32_t j : panels[J]) meets = meets || (j >= s.i0 && j < s.i0 + s.rows);
            CHECK(meets == (J + s.left >= I), "left run of block row %u (n %u K %u)", I, n, K);
        }
        // the kernels' own rules (banded_chol.hip), restated: the solve kernel walks
        // min(I, reach) blocks forward and min(reach, (n - 1 - i0) / 64) backward;
        // workgroup t of the window launch decodes its pair with tri_decode, which
        // must give the list's t-th block
        {
            const uint32_t reach = (uint32_t)(((uint64_t)K + 63) / 64);
            CHECK(s.left == (I < reach ? I : reach), "the solve kernel's forward count (n %u K %u)", n, K);
            const uint32_t right = (n - 1 - s.i0) / 64;
            CHECK(s.blocks == (reach < right ? reach : right), "the solve kernel's backward count (n %u K %u)", n, K);
            CHECK(cp::tri_count(s.blocks) == w.size(), "the window grid's size (n %u K %u)", n, K);
            for (uint64_t t = 0; t < w.size(); ++t) {
                uint32_t a = 0, b = 0;
                cp::tri_decode(t, &a, &b);
                CHECK(a + 1 == w[t].a && b + 1 == w[t].b, "workgroup %llu of the window grid (n %u K %u)",
                      (unsigned long long)t, n, K);
            }
        }
        launches += 1 + (cols.empty() ? 0 : 2);
        // coverage of the in-band upper triangle of these rows
        for (uint64_t i = s.i0; i < (uint64_t)s.i0 + s.rows; ++i)
            for (uint64_t j = i; j < n && j - i <= K; ++j) {
                ++in_band;
                const bool diag = j < (uint64_t)s.i0 + 64, panel = j >= s.panel_begin && j < s.panel_end;
                CHECK(diag != panel, "element (%llu, %llu) of n %u K %u is in %d places", (unsigned long long)i,
                      (unsigned long long)j, n, K, (int)diag + (int)panel);
                ++covered;
            }
    }
    CHECK(covered == in_band, "coverage");
    CHECK(cp::launches(n, K) == launches, "launches of n %u K %u", n, K);
    return 0;
}

int main() {
    const uint32_t shapes[][2] = {{1, 0},    {63, 5},   {64, 63},  {65, 64},   {130, 129}, {130, 400}, {600, 65},
                                  {600, 200}, {5, 0},    {64, 0},   {128, 64},  {129, 1},   {1000, 1},  {700, 4000000000u},
                                  {2051, 1000}, {192, 128}, {193, 127}, {64, 64}, {65, 63}};
    for (const auto &s : shapes)
        if (check_shape(s[0], s[1])) return 1;
    CHECK(cp::reach(0) == 0 && cp::reach(1) == 1 && cp::reach(64) == 1 && cp::reach(65) == 2 &&
              cp::reach(0xFFFFFFFFu) == 67108864u,
          "reach");
    // the pair index at the sizes where the square root's rounding matters
    for (uint64_t b : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)46340, (uint64_t)65535, (uint64_t)67108864,
                       (uint64_t)94906265})
        for (uint64_t a : {(uint64_t)0, b / 2, b})
            if (a <= b) {
                uint32_t ga = 0, gb = 0;
                cp::tri_decode(b * (b + 1) / 2 + a, &ga, &gb);
                CHECK(ga == a && gb == b, "tri_decode at (%llu, %llu)", (unsigned long long)a, (unsigned long long)b);
            }
    // the last representable site count: no wrap
    const cp::Step s = cp::step(0xFFFFFFFFu, 0xFFFFFFFFu, cp::block_rows(0xFFFFFFFFu) - 1);
    CHECK(s.rows == 63 && s.blocks == 0 && s.panel_begin == s.panel_end, "the last block row of 2^32 - 1 sites");
    printf("OK\n");
    return 0;
}
