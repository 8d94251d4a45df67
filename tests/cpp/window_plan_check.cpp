// Host check of the windowed run's plan (weightedld_amd/csrc/window_plan.hpp,
// used by capi.hip window_prepare / build_tiles) against a brute-force O(L^2)
// restatement of the window predicate: for every pair a < b,
//   in window  <=>  (D == 0 || pos[b] - pos[a] <= D) && (K == 0 || b - a <= K).
// Checked per case: hi[] (and that a's partners are exactly a + 1 .. hi[a]),
// the per-chunk pair counts, the windowed tile list against
// tile_order::range_tiles filtered by "holds an in-window pair" (whole sets
// and sub-ranges, element for element; the unfiltered list when the window
// admits everything, less a single-site last diagonal tile, which holds no
// pair), and the shard partition (the shards tile the chunk
// sequence; none exceeds total / n_shards by more than the largest chunk).
#include <cstdio>
#include <cstdlib>

#include "window_plan.hpp"

using namespace wld;

static int g_fail = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            if (++g_fail <= 20) {        \
                printf("FAIL: ");        \
                printf(__VA_ARGS__);     \
                printf("\n");            \
            }                            \
        }                                \
    } while (0)

// a gappy, duplicate-bearing monotone map: increments in [0, 40), every 97th
// raised by 5000, starting at 3
static std::vector<uint32_t> gappy_map(uint32_t L) {
    std::vector<uint32_t> pos(L);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    uint32_t at = 3;
    for (uint32_t i = 0; i < L; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        uint32_t inc = (uint32_t)((s >> 33) % 40);
        if (i % 5 == 2) inc = 0;  // equal neighbours
        if (i % 97 == 96) inc += 5000;
        if (i) at += inc;
        pos[i] = at;
    }
    return pos;
}

static void check_case(uint32_t L, const uint32_t *pos, const char *map_name, uint64_t D, uint64_t K) {
    const uint32_t n = window_plan::chunk_rows(L), T_used = (L + 63) / 64, m = n * (n + 1) / 2;
    auto P = [&](uint32_t i) -> uint64_t { return pos ? pos[i] : i; };
    auto in_window = [&](uint32_t a, uint32_t b) {
        return (D == 0 || P(b) - P(a) <= D) && (K == 0 || (uint64_t)(b - a) <= K);
    };
    // brute force
    std::vector<uint32_t> hi_ref(L), partners(L, 0);
    std::vector<uint64_t> chunk_ref(m, 0);
    std::vector<uint8_t> tile_ref((size_t)T_used * T_used, 0);
    uint64_t total_ref = 0;
    for (uint32_t a = 0; a < L; ++a) {
        hi_ref[a] = a;
        for (uint32_t b = a + 1; b < L; ++b) {
            if (!in_window(a, b)) continue;
            hi_ref[a] = b;
            ++partners[a];
            ++chunk_ref[tile_order::chunk_linear_host(n, a / 256, b / 256)];
            tile_ref[(size_t)(a / 64) * T_used + b / 64] = 1;
            ++total_ref;
        }
    }
    const std::vector<uint32_t> hi = window_plan::limits(pos, L, D, K);
    CHECK(hi.size() == L, "L=%u %s D=%llu K=%llu: hi size", L, map_name, (unsigned long long)D, (unsigned long long)K);
    for (uint32_t a = 0; a < L; ++a) {
        CHECK(hi[a] == hi_ref[a], "L=%u %s D=%llu K=%llu: hi[%u] = %u, brute force %u", L, map_name,
              (unsigned long long)D, (unsigned long long)K, a, hi[a], hi_ref[a]);
        CHECK(partners[a] == hi_ref[a] - a, "L=%u %s D=%llu K=%llu: partners of %u not contiguous", L, map_name,
              (unsigned long long)D, (unsigned long long)K, a);
    }
    const std::vector<uint64_t> pre = window_plan::chunk_prefix(hi);
    CHECK(pre.size() == (size_t)m + 1, "L=%u: prefix size %zu, chunks %u", L, pre.size(), m);
    uint64_t max_chunk = 0;
    for (uint32_t i = 0; i < m && pre.size() == (size_t)m + 1; ++i) {
        CHECK(pre[i + 1] - pre[i] == chunk_ref[i], "L=%u %s D=%llu K=%llu: chunk %u count %llu, brute force %llu", L,
              map_name, (unsigned long long)D, (unsigned long long)K, i, (unsigned long long)(pre[i + 1] - pre[i]),
              (unsigned long long)chunk_ref[i]);
        max_chunk = std::max(max_chunk, chunk_ref[i]);
    }
    CHECK(pre.back() == total_ref, "L=%u: total %llu vs %llu", L, (unsigned long long)pre.back(),
          (unsigned long long)total_ref);
    // tile lists: the whole set and sub-ranges
    const uint32_t ranges[][2] = {{0, m}, {0, m / 2}, {m / 3, m}, {m / 3, (2 * m + 2) / 3}, {m ? m - 1 : 0, m}};
    for (auto &r : ranges) {
        const uint32_t lb = r[0], le = r[1];
        if (lb > le) continue;
        const std::vector<uint32_t> full = tile_order::range_tiles(n, T_used, lb, le);
        std::vector<uint32_t> want;
        for (uint32_t t : full)
            if (tile_ref[(size_t)(t >> 16) * T_used + (t & 0xFFFFu)]) want.push_back(t);
        const std::vector<uint32_t> got = window_plan::range_tiles(n, T_used, lb, le, hi);
        CHECK(got == want, "L=%u %s D=%llu K=%llu chunks [%u,%u): windowed tile list differs (%zu vs %zu tiles)", L,
              map_name, (unsigned long long)D, (unsigned long long)K, lb, le, got.size(), want.size());
        if (total_ref == (uint64_t)L * (L ? L - 1 : 0) / 2) {  // the window admits every pair
            // ... so the list is range_tiles' own, but for the one tile of it
            // that holds no pair at all: a last diagonal tile of a single site
            // (L = 1 mod 64), which "holds an in-window pair" leaves out
            std::vector<uint32_t> all(full);
            const uint32_t lone = L % 64 == 1 ? ((T_used - 1) << 16) | (T_used - 1) : ~0u;
            all.erase(std::remove(all.begin(), all.end(), lone), all.end());
            CHECK(got == all, "L=%u %s D=%llu K=%llu chunks [%u,%u): an all-admitting window changed the list", L,
                  map_name, (unsigned long long)D, (unsigned long long)K, lb, le);
        }
    }
    // shards
    for (int ns : {2, 3, 8}) {
        uint32_t next_end = m;  // shard 0 takes the last range
        for (int k = 0; k < ns; ++k) {
            uint32_t b = ~0u, e = ~0u;
            window_plan::shard_range(pre, ns, k, &b, &e);
            CHECK(b <= e && e == next_end, "L=%u %s D=%llu K=%llu: shard %d/%d [%u,%u) does not end at %u", L, map_name,
                  (unsigned long long)D, (unsigned long long)K, k, ns, b, e, next_end);
            if (b <= e && e <= m)
                CHECK((pre[e] - pre[b]) * ns <= pre[m] + max_chunk * ns,
                      "L=%u %s D=%llu K=%llu: shard %d/%d holds %llu of %llu pairs (largest chunk %llu)", L, map_name,
                      (unsigned long long)D, (unsigned long long)K, k, ns, (unsigned long long)(pre[e] - pre[b]),
                      (unsigned long long)pre[m], (unsigned long long)max_chunk);
            next_end = b;
        }
        CHECK(next_end == 0, "L=%u: %d shards do not start at chunk 0", L, ns);
    }
}

int main() {
    const uint32_t sizes[] = {1, 64, 65, 256, 257, 700, 5000};
    const uint64_t edges[] = {1, 63, 64, 65, 255, 256, 257};
    int cases = 0;
    for (uint32_t L : sizes) {
        const std::vector<uint32_t> gap = gappy_map(L);
        if (window_plan::first_descent(gap.data(), L) != L) {
            printf("FAIL: the gappy map descends\n");
            return 1;
        }
        for (int mi = 0; mi < 2; ++mi) {
            const uint32_t *pos = mi ? gap.data() : nullptr;
            const char *name = mi ? "gappy" : "identity";
            for (uint64_t v : edges) {
                check_case(L, pos, name, 0, v), ++cases;  // K alone
                check_case(L, pos, name, v, 0), ++cases;  // D alone
            }
            // both members, either one binding; large distances on the gappy map
            check_case(L, pos, name, 64, 255), ++cases;
            check_case(L, pos, name, 256, 63), ++cases;
            check_case(L, pos, name, 1000, 64), ++cases;
            check_case(L, pos, name, 4999, 0), ++cases;
            check_case(L, pos, name, 5100, 300), ++cases;
            // windows that admit everything
            check_case(L, pos, name, 0, L), ++cases;
            check_case(L, pos, name, 0xFFFFFFFFFFull, 0), ++cases;
            check_case(L, pos, name, 0xFFFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFFull), ++cases;
        }
    }
    // first_descent names the first offending index
    {
        std::vector<uint32_t> p = gappy_map(300);
        p[200] = p[199] - 1;
        p[250] = 0;
        if (window_plan::first_descent(p.data(), 300) != 200) ++g_fail, printf("FAIL: first_descent\n");
        if (window_plan::first_descent(p.data(), 0) != 0) ++g_fail, printf("FAIL: first_descent of nothing\n");
    }
    if (g_fail) {
        printf("%d checks failed\n", g_fail);
        return 1;
    }
    printf("%d cases OK\n", cases);
    return 0;
}
