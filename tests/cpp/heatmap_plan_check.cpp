// Host check of the LD heat map's host-side pieces
// (weightedld_amd/csrc/heatmap_plan.hpp, used by capi.hip wld_run_heatmap and
// by the kernel's epilogue in pair_heatmap.hip) against brute force:
//   * validate(): the first offending index of maps with an id >= n_cells, an
//     id < -1 and a descending id (also across -1 gaps), and valid maps with
//     gaps and empty cells, against a scan that follows the rules literally;
//   * float_key / key_float over negatives, +-0, denormals, the largest finite
//     values and +-inf: strictly monotone in the float order, round-tripping
//     bit for bit, every finite key above kNoKey;
//   * blocks() and filter_tiles() against "both blocks hold a site with a
//     cell", and against "some pair of the tile is considered": a tile with a
//     considered pair is always kept, and without a window an off-diagonal
//     tile is kept iff it holds one;
//   * considered_pairs() against a double loop, under random windows, random
//     -1 gaps and every chunk range of small sets;
//   * merge(): counts add, max keys combine, tiles add, kernel_ms the larger.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "heatmap_plan.hpp"
#include "window_plan.hpp"

using namespace wld;
namespace hp = wld::heatmap_plan;

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

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_rng >> 33) % n);
}

// ---- validation ---------------------------------------------------------
static hp::MapCheck validate_ref(const std::vector<int32_t> &m, uint32_t n_cells) {
    for (uint32_t s = 0; s < m.size(); ++s) {
        if (m[s] == -1) continue;
        if (m[s] < -1) return {hp::kMapNegative, s, 0};
        if ((uint32_t)m[s] >= n_cells) return {hp::kMapTooLarge, s, 0};
        for (uint32_t p = s; p-- > 0;)
            if (m[p] != -1) {
                if (m[s] < m[p]) return {hp::kMapDescends, s, p};
                break;
            }
    }
    return {hp::kMapOk, (uint32_t)m.size(), 0};
}

// a valid random map: L sites, ids < n_cells non-decreasing, -1 gaps
static std::vector<int32_t> random_map(uint32_t L, uint32_t n_cells, uint32_t gap_pct) {
    std::vector<int32_t> m(L);
    int32_t c = (int32_t)rnd(2);
    for (uint32_t s = 0; s < L; ++s) {
        if (rnd(4) == 0) c += (int32_t)rnd(3);
        if (c >= (int32_t)n_cells) c = (int32_t)n_cells - 1;
        m[s] = rnd(100) < gap_pct ? -1 : c;
    }
    // a run of -1 now and then (a whole block without a cell)
    if (L > 100 && gap_pct) {
        const uint32_t at = rnd(L - 90);
        for (uint32_t s = at; s < at + 90; ++s) m[s] = -1;
    }
    return m;
}

static void check_validate() {
    uint32_t cases = 0;
    for (int it = 0; it < 3000; ++it) {
        const uint32_t L = 1 + rnd(200), n_cells = 1 + rnd(40);
        std::vector<int32_t> m = random_map(L, n_cells, it % 3 ? 20 : 0);
        const int kind = it % 5;
        const uint32_t k = rnd(L);
        if (kind == 1) m[k] = (int32_t)n_cells + (int32_t)rnd(3);
        if (kind == 2) m[k] = -2 - (int32_t)rnd(5);
        if (kind == 3 && m[k] > 0) m[k] -= 1 + (int32_t)rnd((uint32_t)m[k]);
        if (kind == 4) {  // two defects: the first one is reported
            m[k] = -7;
            m[rnd(L)] = (int32_t)n_cells;
        }
        const hp::MapCheck got = hp::validate(m.data(), L, n_cells), ref = validate_ref(m, n_cells);
        CHECK(got.what == ref.what && got.index == ref.index && (got.what != hp::kMapDescends || got.prev == ref.prev),
              "validate case %d: got (%d, %u, %u), brute force (%d, %u, %u)", it, got.what, got.index, got.prev,
              ref.what, ref.index, ref.prev);
        ++cases;
    }
    // the edges by hand
    const int32_t ok[] = {-1, 0, 0, -1, -1, 2, 2, 5, -1};
    CHECK(hp::validate(ok, 9, 6).what == hp::kMapOk && hp::validate(ok, 9, 6).index == 9, "a valid map with gaps");
    CHECK(hp::validate(ok, 9, 5).what == hp::kMapTooLarge && hp::validate(ok, 9, 5).index == 7, "id == n_cells");
    const int32_t desc[] = {3, -1, -1, 2};
    const hp::MapCheck d = hp::validate(desc, 4, 4);
    CHECK(d.what == hp::kMapDescends && d.index == 3 && d.prev == 0, "descent across a gap");
    CHECK(hp::validate(nullptr, 0, 1).what == hp::kMapOk, "no sites");
    printf("%u validation cases\n", cases);
}

// ---- keys ---------------------------------------------------------------
static float from_bits(uint32_t u) {
    float x;
    memcpy(&x, &u, 4);
    return x;
}
static uint32_t bits_of(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}

static void check_keys() {
    // ascending in the float order: -inf, negatives, -denormals, -0, +0, ...
    std::vector<float> v;
    v.push_back(-INFINITY);
    const uint32_t mags[] = {0x7F7FFFFFu, 0x7F7FFFFEu, 0x7F000000u, 0x3F800001u, 0x3F800000u, 0x3F7FFFFFu, 0x00800001u,
                             0x00800000u, 0x007FFFFFu, 0x00000002u, 0x00000001u};
    for (uint32_t m : mags) v.push_back(from_bits(0x80000000u | m));
    v.push_back(from_bits(0x80000000u));  // -0
    v.push_back(0.0f);
    for (size_t i = sizeof(mags) / sizeof(mags[0]); i-- > 0;) v.push_back(from_bits(mags[i]));
    v.push_back(INFINITY);
    for (size_t i = 0; i < v.size(); ++i) {
        const uint32_t k = hp::float_key(v[i]);
        CHECK(bits_of(hp::key_float(k)) == bits_of(v[i]), "round trip of %a (bits %08x)", v[i], bits_of(v[i]));
        CHECK(k > hp::kNoKey, "key of %a is not above kNoKey", v[i]);
        if (std::isfinite(v[i])) CHECK(k >= 0x00800000u, "finite key of %a below 0x00800000", v[i]);
        if (i) CHECK(hp::float_key(v[i - 1]) < k, "keys of %a and %a not strictly ascending", v[i - 1], v[i]);
    }
    // pseudo-random pairs of non-NaN floats: the key order is the float order
    // (with -0 < +0), and every pattern round-trips
    uint64_t n = 0;
    for (int it = 0; it < 2000000; ++it) {
        g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
        // (every other pair a few ulps apart, or the same magnitude with the other sign)
        const uint32_t ua = (uint32_t)(g_rng >> 32), lo = (uint32_t)g_rng;
        const uint32_t ub = it & 1 ? ua ^ (lo & 0x8000000Fu) : lo;
        const float a = from_bits(ua), b = from_bits(ub);
        CHECK(bits_of(hp::key_float(hp::float_key(a))) == ua, "round trip of bits %08x", ua);
        if (std::isnan(a) || std::isnan(b)) continue;
        const uint32_t ka = hp::float_key(a), kb = hp::float_key(b);
        const bool lt = a < b || (a == b && std::signbit(a) && !std::signbit(b));
        CHECK((ka < kb) == lt, "order of %a and %a: keys %08x %08x", a, b, ka, kb);
        CHECK((ka == kb) == (ua == ub), "equal keys of different floats %08x %08x", ua, ub);
        ++n;
    }
    // neighbours: every step of one ulp across the whole line moves the key by one
    for (uint32_t u = 0x00000000u; u < 0x7F800000u; u += 0x00010001u) {
        CHECK(hp::float_key(from_bits(u + 1)) == hp::float_key(from_bits(u)) + 1, "positive ulp step at %08x", u);
        CHECK(hp::float_key(from_bits(0x80000000u | (u + 1))) + 1 == hp::float_key(from_bits(0x80000000u | u)),
              "negative ulp step at %08x", u);
    }
    printf("%zu ordered values, %" PRIu64 " random pairs\n", v.size(), n);
}

// ---- tiles and pairs ----------------------------------------------------
// a random window's limits: hi[a] non-decreasing, a <= hi[a] < L
static std::vector<uint32_t> random_window(uint32_t L, int kind) {
    std::vector<uint32_t> pos(L);
    uint32_t p = 0;
    for (uint32_t i = 0; i < L; ++i) pos[i] = (p += rnd(4) + (rnd(50) == 0 ? 200 : 0));
    const uint64_t D = kind & 1 ? 20 + rnd(400) : 0, K = kind & 2 ? 1 + rnd(150) : 0;
    return window_plan::limits(pos.data(), L, D, K);
}

static bool considered(const std::vector<int32_t> &m, const std::vector<uint32_t> *hi, uint32_t a, uint32_t b) {
    return a < b && m[a] >= 0 && m[b] >= 0 && (!hi || b <= (*hi)[a]);
}

static void check_plan() {
    uint64_t tiles_seen = 0, ranges = 0;
    for (int it = 0; it < 60; ++it) {
        const uint32_t L = it < 4 ? 1 + (uint32_t)it : 2 + rnd(700), n_cells = 1 + rnd(60);
        const std::vector<int32_t> m = random_map(L, n_cells, it % 4 == 0 ? 0 : 10 + rnd(60));
        const int wk = it % 4;  // none, distance, sites, both
        const std::vector<uint32_t> hi = wk ? random_window(L, wk) : std::vector<uint32_t>();
        const std::vector<uint32_t> *hp_ = wk ? &hi : nullptr;
        const uint32_t T = (L + 63) / 64, n = (L + 255) / 256, n_chunks = n * (n + 1) / 2;
        const hp::Blocks blk = hp::blocks(m.data(), L, T + 1);  // (a padded block too)
        for (uint32_t t = 0; t <= T; ++t) {
            int32_t lo = 0, hi_c = -1;
            bool any = false;
            for (uint32_t s = t * 64; s < std::min(L, (t + 1) * 64); ++s)
                if (m[s] >= 0) {
                    if (!any) lo = m[s];
                    hi_c = m[s];
                    any = true;
                }
            CHECK(blk.mapped(t) == any && (!any || (blk.lo[t] == lo && blk.hi[t] == hi_c)), "case %d: block %u", it, t);
        }
        // every chunk range of small sets, a few of larger ones
        for (uint32_t lb = 0; lb <= n_chunks; ++lb)
            for (uint32_t le = lb; le <= n_chunks; ++le) {
                if (n_chunks > 3 && rnd(3) && !(lb == 0 && le == n_chunks)) continue;
                const std::vector<uint32_t> full =
                    wk ? window_plan::range_tiles(n, T, lb, le, hi) : tile_order::range_tiles(n, T, lb, le);
                const std::vector<uint32_t> kept = hp::filter_tiles(full, blk);
                size_t k = 0;
                uint64_t pairs = 0;
                for (uint32_t t : full) {
                    const uint32_t ta = t >> 16, tb = t & 0xFFFFu;
                    uint64_t in_tile = 0;
                    for (uint32_t a = ta * 64; a < std::min(L, (ta + 1) * 64); ++a)
                        for (uint32_t b = std::max(a + 1, tb * 64); b < std::min(L, (tb + 1) * 64); ++b)
                            in_tile += considered(m, hp_, a, b) ? 1 : 0;
                    const bool is_kept = k < kept.size() && kept[k] == t;
                    if (is_kept) ++k;
                    CHECK(is_kept == (blk.mapped(ta) && blk.mapped(tb)), "case %d: tile (%u,%u) kept %d", it, ta, tb,
                          (int)is_kept);
                    CHECK(!in_tile || is_kept, "case %d: tile (%u,%u) holds %" PRIu64 " considered pairs but was dropped",
                          it, ta, tb, in_tile);
                    if (!wk && ta != tb) CHECK(is_kept == (in_tile != 0), "case %d: off-diagonal tile (%u,%u)", it, ta, tb);
                    pairs += in_tile;
                    ++tiles_seen;
                }
                CHECK(k == kept.size(), "case %d: the kept list is not a sub-list", it);
                // (the listed tiles hold every in-window pair of the range)
                const uint64_t got = hp::considered_pairs(m.data(), wk ? hi.data() : nullptr, L, lb, le);
                CHECK(got == pairs, "case %d (L %u, window %d) chunks [%u,%u): considered_pairs %" PRIu64
                                    ", brute force %" PRIu64, it, L, wk, lb, le, got, pairs);
                ++ranges;
            }
    }
    // a region of 2,000 sites out of 20,000 starting on a tile edge: 32 blocks
    {
        const uint32_t L = 20000, T = (L + 63) / 64, n = (L + 255) / 256;
        std::vector<int32_t> m(L, -1);
        for (uint32_t s = 1984; s < 3984; ++s) m[s] = (int32_t)((s - 1984) / 20);
        const std::vector<uint32_t> full = tile_order::range_tiles(n, T, 0, n * (n + 1) / 2);
        const std::vector<uint32_t> kept = hp::filter_tiles(full, hp::blocks(m.data(), L, T));
        CHECK(full.size() == (size_t)T * (T + 1) / 2 && kept.size() == 32 * 33 / 2, "region: %zu of %zu tiles",
              kept.size(), full.size());
        CHECK(hp::considered_pairs(m.data(), nullptr, L, 0, n * (n + 1) / 2) == 2000ull * 1999 / 2, "region pairs");
    }
    printf("%" PRIu64 " tiles, %" PRIu64 " chunk ranges\n", tiles_seen, ranges);
}

// ---- merge --------------------------------------------------------------
static void check_merge() {
    const uint32_t nc = 7;
    auto make = [&](uint32_t seed, uint64_t tiles, double ms) {
        hp::Heatmap h;
        h.n_cells = nc;
        h.count.assign(nc * nc, 0);
        h.sum.assign(nc * nc, 0.0);
        h.max_key.assign(nc * nc, hp::kNoKey);
        g_rng = seed;
        for (int i = 0; i < 300; ++i) {
            const uint32_t a = rnd(nc), b = a + rnd(nc - a), cls = rnd(10);
            ++h.pairs;
            if (cls == 0) ++h.none_pairs;
            else if (cls == 1) ++h.nonfinite_pairs;
            else {
                const float x = (float)((int)rnd(2001) - 1000) / 1000.0f;  // negatives too
                ++h.counted_pairs;
                ++h.count[a * nc + b];
                h.sum[a * nc + b] += (double)x;
                h.max_key[a * nc + b] = std::max(h.max_key[a * nc + b], hp::float_key(x));
            }
        }
        h.tiles = tiles;
        h.kernel_ms = ms;
        return h;
    };
    const hp::Heatmap x = make(11, 5, 1.0), y = make(23, 9, 2.0);
    hp::Heatmap z = x;
    hp::merge(z, y);
    CHECK(z.pairs == x.pairs + y.pairs && z.none_pairs == x.none_pairs + y.none_pairs &&
              z.nonfinite_pairs == x.nonfinite_pairs + y.nonfinite_pairs &&
              z.counted_pairs == x.counted_pairs + y.counted_pairs,
          "merge: class counts");
    CHECK(z.pairs == z.none_pairs + z.nonfinite_pairs + z.counted_pairs, "merge: identity");
    CHECK(z.tiles == 14 && z.kernel_ms == 2.0 && z.n_cells == nc, "merge: tiles, kernel_ms, n_cells");
    uint64_t total = 0;
    for (uint32_t i = 0; i < nc * nc; ++i) {
        total += z.count[i];
        CHECK(z.count[i] == x.count[i] + y.count[i], "merge: count[%u]", i);
        CHECK(z.sum[i] == x.sum[i] + y.sum[i], "merge: sum[%u]", i);
        float want = NAN;
        if (x.count[i] && y.count[i]) want = std::max(hp::key_float(x.max_key[i]), hp::key_float(y.max_key[i]));
        else if (x.count[i]) want = hp::key_float(x.max_key[i]);
        else if (y.count[i]) want = hp::key_float(y.max_key[i]);
        if (z.count[i]) CHECK(hp::key_float(z.max_key[i]) == want, "merge: max[%u]", i);
        else CHECK(z.max_key[i] == hp::kNoKey, "merge: empty max[%u]", i);
        if (i / nc > i % nc) CHECK(z.count[i] == 0, "merge: lower triangle");
    }
    CHECK(total == z.counted_pairs, "merge: sum of counts");
    hp::Heatmap e;  // into an empty map: a copy
    hp::merge(e, x);
    CHECK(e.n_cells == nc && e.count == x.count && e.sum == x.sum && e.max_key == x.max_key && e.pairs == x.pairs &&
              e.tiles == x.tiles && e.kernel_ms == x.kernel_ms,
          "merge into an empty map");
}

int main() {
    check_validate();
    check_keys();
    check_plan();
    check_merge();
    if (g_fail) {
        printf("%d failures\n", g_fail);
        return 1;
    }
    printf("OK\n");
    return 0;
}
