// Host-only check of weightedld_amd/csrc/banded_omega_plan.hpp against brute
// force, over every (n, K) with n <= 200 and K <= 140: the chain pass's
// parallelogram tiling (every element (j, k) of [n] x [K + 1] is visited exactly
// once, by the chain block of its end site i = j + k, in the lane i - i0, inside
// the block's row range, inside the row's run and inside exactly one 64-step
// tile; a chain's elements come in the order k = 0, 1, 2, ..., from k = i - (n - 1)
// for a chain i >= n, which holds only tails; nothing outside the band is
// touched), the row pass's block and tile counts, the candidate
// counts of a split, and the splits of a scan against a linear search.  Prints
// "OK" and returns 0, or the first mismatch and 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "banded_omega_plan.hpp"

namespace op = wld::banded_omega_plan;

#define CHECK(cond, ...)                                \
    do {                                                \
        if (!(cond)) {                                  \
            printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                        \
            printf("\n");                               \
            return 1;                                   \
        }                                               \
    } while (0)

static int check_shape(uint32_t n, uint32_t K) {
    CHECK((uint64_t)op::row_blocks(n) * 64 >= n && (uint64_t)(op::row_blocks(n) - 1) * 64 < n, "row blocks of n %u", n);
    CHECK((uint64_t)op::col_tiles(K) * 64 > K && (uint64_t)(op::col_tiles(K) - 1) * 64 <= K, "column tiles of K %u", K);
    const uint32_t blocks = op::chain_blocks(n, K);
    CHECK((uint64_t)blocks * 64 >= (uint64_t)n + K && (uint64_t)(blocks - 1) * 64 < (uint64_t)n + K,
          "chain blocks of n %u K %u", n, K);
    std::vector<uint32_t> seen((size_t)n * (K + 1), 0);
    for (uint32_t I = 0; I < blocks; ++I) {
        const uint64_t i0 = (uint64_t)I * 64;
        const op::Rows r = op::rows(i0, n, K);
        CHECK(r.bottom <= r.top && r.top < n, "rows of chain block %u (n %u K %u)", I, n, K);
        // brute force: the first and last row holding an element of the block's chains
        uint32_t top = 0, bottom = ~0u;
        bool any = false;
        for (uint32_t j = 0; j < n; ++j)
            for (uint32_t k = 0; k <= K; ++k)
                if ((uint64_t)j + k >= i0 && (uint64_t)j + k < i0 + 64) {
                    top = any && top > j ? top : j;
                    bottom = bottom < j ? bottom : j;
                    any = true;
                }
        CHECK(any && r.top == top && r.bottom == bottom, "row range of chain block %u (n %u K %u): %u..%u, brute %u..%u", I, n,
              K, r.top, r.bottom, top, bottom);
        const uint32_t tiles = op::step_tiles(i0, n, K);
        CHECK(tiles == (r.top - r.bottom) / 64 + 1, "step tiles of chain block %u (n %u K %u)", I, n, K);
        // the tiles partition the rows, top down, 64 at a time
        uint32_t next = r.top;
        for (uint32_t t = 0; t < tiles; ++t) {
            const op::Rows q = op::tile(i0, n, K, t);
            CHECK(q.top == next && q.bottom <= q.top && q.top - q.bottom < 64 && q.bottom >= r.bottom,
                  "tile %u of chain block %u (n %u K %u)", t, I, n, K);
            CHECK(t + 1 == tiles ? q.bottom == r.bottom : q.top - q.bottom == 63, "tile %u's height (n %u K %u)", t, n, K);
            next = q.bottom - 1;
        }
        // the walk the kernel does: rows top down, the row's run, lane = i - i0
        // (a chain i >= n, all tails, starts at row n - 1 with k = i - (n - 1))
        std::vector<int64_t> last_k(64, -1);
        for (uint64_t lane = 0; lane < 64; ++lane)
            if (i0 + lane > (uint64_t)n - 1) last_k[lane] = (int64_t)(i0 + lane - (n - 1)) - 1;
        for (uint32_t j = r.top + 1; j-- > r.bottom;) {
            uint32_t k_lo = 0, k_hi = 0;
            const bool has = op::row_segment(i0, j, K, &k_lo, &k_hi);
            uint32_t b_lo = ~0u, b_hi = 0;
            bool b_has = false;
            for (uint32_t k = 0; k <= K; ++k)
                if ((uint64_t)j + k >= i0 && (uint64_t)j + k < i0 + 64) {
                    b_lo = b_has ? b_lo : k;
                    b_hi = k;
                    b_has = true;
                }
            CHECK(has == b_has && (!has || (k_lo == b_lo && k_hi == b_hi)), "run of row %u in chain block %u (n %u K %u)", j, I,
                  n, K);
            if (!has) continue;
            for (uint32_t k = k_lo; k <= k_hi; ++k) {
                const uint64_t lane = (uint64_t)j + k - i0;
                CHECK(lane < 64, "lane of (%u, %u)", j, k);
                CHECK(last_k[lane] + 1 == (int64_t)k, "chain %llu visits k %u after %lld (n %u K %u)",
                      (unsigned long long)(i0 + lane), k, (long long)last_k[lane], n, K);
                last_k[lane] = k;
                ++seen[(size_t)j * (K + 1) + k];
            }
        }
        // rows outside the range hold nothing of this block
        for (uint32_t j = 0; j < n; ++j)
            if (j < r.bottom || j > r.top) {
                uint32_t k_lo, k_hi;
                if (op::row_segment(i0, j, K, &k_lo, &k_hi))
                    for (uint32_t k = k_lo; k <= k_hi; ++k)
                        CHECK(false, "row %u outside %u..%u holds k %u of chain block %u (n %u K %u)", j, r.bottom, r.top, k, I,
                              n, K);
            }
    }
    for (size_t e = 0; e < seen.size(); ++e)
        CHECK(seen[e] == 1, "element (%zu, %zu) of n %u K %u visited %u times", e / (K + 1), e % (K + 1), n, K, seen[e]);
    return 0;
}

static int check_splits(const std::vector<uint64_t> &pos, bool indices) {
    const uint32_t n = (uint32_t)pos.size();
    for (uint32_t n_grid : {0u, 1u, 2u, 7u, 3u * n})
        for (uint32_t max_side : {1u, 2u, 33u, 100000u})
            for (uint64_t D : {(uint64_t)0, (uint64_t)1, (uint64_t)5, (uint64_t)60, ~(uint64_t)0}) {
                const uint64_t G = op::n_splits(n, n_grid);
                CHECK(G == (n_grid ? n_grid : n - 1), "split count");
                std::vector<uint64_t> x(G);
                std::vector<uint32_t> c(G), lo(G), hi(G);
                op::splits(indices ? nullptr : pos.data(), n, n_grid, max_side, D, x.data(), c.data(), lo.data(), hi.data());
                const unsigned __int128 span = pos[n - 1] - pos[0];
                for (uint64_t g = 0; g < G; ++g) {
                    uint64_t wx;
                    uint32_t wc = 0;
                    if (!n_grid) {
                        wc = (uint32_t)g;
                        wx = pos[wc];
                    } else {
                        wx = n_grid == 1 ? pos[0] + (uint64_t)(span / 2) : pos[0] + (uint64_t)(span * g / (n_grid - 1));
                        for (uint32_t i = 0; i < n; ++i)
                            if (pos[i] <= wx) wc = i;
                        if (wc > n - 2) wc = n - 2;
                    }
                    int64_t wl = (int64_t)wc - (int64_t)max_side + 1, wh = (int64_t)wc + max_side;
                    if (wl < 0) wl = 0;
                    if (wh > (int64_t)n - 1) wh = n - 1;
                    if (D) {
                        int64_t first = n, last = -1;
                        for (uint32_t i = n; i-- > 0;)
                            if ((unsigned __int128)pos[i] + D >= wx) first = i;
                        for (uint32_t i = 0; i < n; ++i)
                            if ((unsigned __int128)pos[i] <= (unsigned __int128)wx + D) last = i;
                        if (first > wl) wl = first;
                        if (last < wh) wh = last;
                    }
                    if (wl > (int64_t)wc) wl = wc;
                    if (wh < (int64_t)wc + 1) wh = wc + 1;
                    CHECK(x[g] == wx && c[g] == wc && lo[g] == (uint32_t)wl && hi[g] == (uint32_t)wh,
                          "split %llu (n_grid %u max_side %u D %llu): x %llu c %u lo %u hi %u, brute x %llu c %u lo %lld hi %lld",
                          (unsigned long long)g, n_grid, max_side, (unsigned long long)D, (unsigned long long)x[g], c[g], lo[g],
                          hi[g], (unsigned long long)wx, wc, (long long)wl, (long long)wh);
                    CHECK(lo[g] <= c[g] && c[g] < hi[g] && hi[g] < n && (uint64_t)hi[g] - lo[g] <= 2ull * max_side - 1,
                          "split %llu's order", (unsigned long long)g);
                    CHECK(op::split_ok(c[g], lo[g], hi[g], n, hi[g] - lo[g]) && !op::split_ok(c[g], lo[g], hi[g], hi[g], n) &&
                              (hi[g] - lo[g] == 0 || !op::split_ok(c[g], lo[g], hi[g], n, hi[g] - lo[g] - 1)),
                          "split_ok");
                }
            }
    return 0;
}

int main() {
    for (uint32_t n = 1; n <= 200; ++n)
        for (uint32_t K = 0; K <= 140; ++K)
            if (check_shape(n, K)) return 1;
    // K >= n by far, and the sizes next to 2^32: no wrap
    if (check_shape(3, 1000)) return 1;
    {
        const uint32_t n = 0xFFFFFFFFu, K = 0xFFFFFFFFu;
        CHECK(op::chain_blocks(n, K) == 134217728u && op::row_blocks(n) == 67108864u && op::col_tiles(K) == 67108864u,
              "block counts at 2^32 - 1");
        const op::Rows first = op::rows(0, n, K), last = op::rows((uint64_t)(op::chain_blocks(n, K) - 1) * 64, n, K);
        CHECK(first.top == 63 && first.bottom == 0 && last.top == n - 1 && last.bottom == n - 62, "rows at 2^32 - 1");
        uint32_t k_lo = 0, k_hi = 0;
        CHECK(op::row_segment((uint64_t)(op::chain_blocks(n, K) - 1) * 64, n - 1, K, &k_lo, &k_hi) && k_hi == K &&
                  k_lo == K - 61,
              "the last run at 2^32 - 1");
    }
    // the candidate counts of a split
    for (uint32_t lo = 0; lo < 12; ++lo)
        for (uint32_t c = lo; c < 14; ++c)
            for (uint32_t hi = c + 1; hi < 16; ++hi)
                for (uint32_t ms : {2u, 3u, 5u, 0xFFFFFFFFu}) {
                    uint32_t nl = 0, nr = 0, bl = 0, br = 0;
                    op::split_sides(c, lo, hi, ms, &nl, &nr);
                    for (uint32_t a = lo; a <= c; ++a) bl += (uint64_t)c - a + 1 >= ms;
                    for (uint32_t b = c + 1; b <= hi; ++b) br += (uint64_t)b - c >= ms;
                    CHECK(nl == bl && nr == br, "sides of (%u, %u, %u) at min_side %u", lo, c, hi, ms);
                }
    // splits: repeated coordinates with gaps, strictly increasing large ones, plain indices
    std::vector<uint64_t> rep, inc, idx;
    uint64_t s = 12345, p = 0;
    for (uint32_t i = 0; i < 150; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        p += i % 37 == 0 ? 60 : (s >> 60) % 4;
        rep.push_back(p);
        inc.push_back(0xFFFFFFFF00000000ull + 1000ull * i + (s >> 58));
        idx.push_back(i);
    }
    if (check_splits(rep, false) || check_splits(inc, false) || check_splits(idx, true)) return 1;
    if (check_splits(std::vector<uint64_t>{7, 7}, false) || check_splits(std::vector<uint64_t>{0, 1}, true)) return 1;
    printf("OK\n");
    return 0;
}
