// Host check of the LD blocks' host-side pieces
// (weightedld_amd/csrc/blocks_plan.hpp, used by capi.hip's block calls and by
// the epilogues in pair_blocks.hip) against brute force:
//   * partition(): on a random weak matrix under a random window, both rules,
//     min_sites 2..5, n up to ~300, against the definition itself — the
//     validity of a run is tested on the matrix, NOT via the break arrays;
//     all-weak, no-weak, single-site and empty sets;
//   * the break arrays of a random split of the weak pairs merged by min / max
//     equal those of the whole set, totals add, times the larger; mergeable();
//   * stats_tiles() against a scan of every tile and every block; block_pairs;
//     id_limits() stays inside the epilogue's table;
//   * inv_key: the unsigned max of inverted keys is the float min over
//     negatives, +-0, denormals and the largest finite values; round trip;
//   * the argument checks.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "blocks_plan.hpp"

using namespace wld;
namespace bp = wld::blocks_plan;

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

// a set: n sites, last[] (non-decreasing, last[a] >= a), weak[a * n + b] for
// the considered pairs a < b <= last[a]
struct Set {
    uint32_t n = 0;
    std::vector<uint32_t> last;
    std::vector<uint8_t> weak;
    bool w(uint32_t a, uint32_t b) const { return weak[(size_t)a * n + b] != 0; }
};

// density: a pair is weak with probability 1 / density (0: never; 1: always),
// except inside planted strong runs
static Set make_set(uint32_t n, uint32_t density, bool windowed) {
    Set s;
    s.n = n;
    s.last.assign(n, n ? n - 1 : 0);
    if (windowed) {
        uint32_t prev = 0;
        for (uint32_t a = 0; a < n; ++a) {
            const uint32_t want = std::min(n - 1, a + rnd(40));
            prev = std::max(std::max(prev, want), a);
            s.last[a] = prev;
        }
    }
    s.weak.assign((size_t)n * n, 0);
    // planted runs: no weak pair inside, so blocks of some length exist
    std::vector<uint32_t> run(n, 0);
    for (uint32_t a = 0, id = 1; a < n; ++id) {
        const uint32_t len = 1 + rnd(30);
        for (uint32_t i = a; i < std::min(n, a + len); ++i) run[i] = id;
        a += len;
    }
    for (uint32_t a = 0; a < n; ++a)
        for (uint32_t b = a + 1; b <= s.last[a]; ++b) {
            if (density == 0) continue;
            const bool inside = run[a] == run[b] && density > 1;
            // (inside a run: rarely an interior weak pair, so the rules differ)
            const bool weak = inside ? rnd(60) == 0 : rnd(density) == 0;
            s.weak[(size_t)a * n + b] = weak;
        }
    return s;
}

static bool valid_brute(const Set &s, uint32_t a, uint32_t e, int rule) {
    if (e > s.last[a]) return false;
    if (rule == bp::kRuleAll) {
        for (uint32_t i = a; i <= e; ++i)
            for (uint32_t j = i + 1; j <= e; ++j)
                if (s.w(i, j)) return false;
        return true;
    }
    for (uint32_t k = a + 1; k <= e; ++k)
        if (s.w(a, k)) return false;
    for (uint32_t k = a; k < e; ++k)
        if (s.w(k, e)) return false;
    return true;
}

static bp::Partition partition_brute(const Set &s, int rule, uint32_t min_sites) {
    bp::Partition p;
    p.site_block.assign(s.n, -1);
    for (uint32_t a = 0; a < s.n;) {
        uint32_t e = a;
        for (uint32_t c = s.last[a]; c > a; --c)
            if (valid_brute(s, a, c, rule)) {
                e = c;
                break;
            }
        if (e - a + 1 >= min_sites) {
            const int32_t id = (int32_t)p.first.size();
            p.first.push_back(a);
            p.last.push_back(e);
            for (uint32_t i = a; i <= e; ++i) p.site_block[i] = id;
        }
        a = e + 1;
    }
    return p;
}

// the break arrays of the pairs with keep(a, b)
template <class F>
static bp::Breaks breaks_of(const Set &s, F keep) {
    bp::Breaks b;
    b.n_sites = s.n;
    b.fwd.assign(s.n, bp::kNone);
    b.bwd.assign(s.n, bp::kNone);
    b.last = s.last;
    for (uint32_t a = 0; a < s.n; ++a)
        for (uint32_t c = a + 1; c <= s.last[a]; ++c) {
            if (!keep(a, c)) continue;
            ++b.pairs;
            if (!s.w(a, c)) {
                ++b.strong_pairs;
                continue;
            }
            ++b.weak_pairs;
            if (b.fwd[a] == bp::kNone) b.fwd[a] = c;  // (c ascending: the smallest)
            if (b.bwd[c] == bp::kNone || a > b.bwd[c]) b.bwd[c] = a;
        }
    return b;
}

static bool same(const bp::Partition &x, const bp::Partition &y) {
    return x.first == y.first && x.last == y.last && x.site_block == y.site_block;
}

static void check_set(const Set &s, const char *what, bool &rules_differ) {
    const bp::Breaks whole = breaks_of(s, [](uint32_t, uint32_t) { return true; });
    // a split of the pairs by a hash of their chunk-like cell, merged
    const uint32_t cut = 1 + rnd(7);
    bp::Breaks m;
    for (uint32_t part = 0; part < cut; ++part) {
        bp::Breaks piece = breaks_of(s, [&](uint32_t a, uint32_t b) { return ((a / 16) * 31 + b / 16) % cut == part; });
        piece.tiles = part + 1;
        piece.kernel_ms = (double)((part * 7) % cut);
        bp::merge(m, piece);
    }
    CHECK(m.fwd == whole.fwd && m.bwd == whole.bwd && m.last == whole.last, "%s: merged break arrays differ", what);
    CHECK(m.pairs == whole.pairs && m.weak_pairs == whole.weak_pairs && m.strong_pairs == whole.strong_pairs,
          "%s: merged totals differ", what);
    CHECK(m.tiles == (uint64_t)cut * (cut + 1) / 2, "%s: tiles do not add", what);
    CHECK(m.kernel_ms <= (double)cut && m.kernel_ms >= 0.0, "%s: kernel_ms", what);
    for (int rule : {bp::kRuleAll, bp::kRuleSpine})
        for (uint32_t min_sites = 2; min_sites <= 5; ++min_sites) {
            const bp::Partition got =
                bp::partition(whole.fwd.data(), whole.bwd.data(), whole.last.data(), s.n, rule, min_sites);
            const bp::Partition ref = partition_brute(s, rule, min_sites);
            CHECK(same(got, ref), "%s: n %u rule %d min_sites %u: %zu blocks, brute force %zu", what, s.n, rule,
                  min_sites, got.first.size(), ref.first.size());
            // blocks: in order, disjoint, long enough, every pair in the window
            for (size_t k = 0; k < got.first.size(); ++k) {
                CHECK(got.last[k] - got.first[k] + 1 >= min_sites, "%s: a short block", what);
                CHECK(got.last[k] <= s.last[got.first[k]], "%s: a block leaves the window", what);
                CHECK(k == 0 || got.first[k] > got.last[k - 1], "%s: blocks overlap", what);
            }
            // pass 2's tiles against a scan of all tiles and blocks
            const uint32_t T = (s.n + 63) / 64;
            std::vector<uint32_t> tb;
            for (uint32_t ta = 0; ta < T; ++ta)
                for (uint32_t tc = ta; tc < T; ++tc) {
                    bool hit = false;
                    for (size_t k = 0; k < got.first.size() && !hit; ++k) {
                        auto meets = [&](uint32_t t) { return got.first[k] <= t * 64 + 63 && got.last[k] >= t * 64; };
                        hit = meets(ta) && meets(tc);
                    }
                    if (hit) tb.push_back((ta << 16) | tc);
                }
            CHECK(bp::stats_tiles(got) == tb, "%s: pass-2 tile list differs (rule %d)", what, rule);
            uint64_t inside = 0;
            for (uint32_t a = 0; a < s.n; ++a)
                for (uint32_t c = a + 1; c < s.n; ++c)
                    inside += got.site_block[a] >= 0 && got.site_block[a] == got.site_block[c];
            CHECK(bp::block_pairs(got) == inside, "%s: block_pairs", what);
            const heatmap_plan::Blocks lim = bp::id_limits(got, T);
            for (uint32_t t = 0; t < T; ++t) {
                int32_t lo = 0, hi = -1;
                for (uint32_t i = t * 64; i < std::min(s.n, t * 64 + 64); ++i)
                    if (got.site_block[i] >= 0) {
                        if (lo > hi) lo = got.site_block[i];
                        hi = got.site_block[i];
                    }
                CHECK(lim.lo[t] == lo && lim.hi[t] == hi, "%s: id limits of block %u", what, t);
                CHECK(lo > hi || (uint32_t)(hi - lo) < bp::kTableIds, "%s: ids of block %u leave the table", what, t);
            }
        }
    const bp::Partition a2 = bp::partition(whole.fwd.data(), whole.bwd.data(), whole.last.data(), s.n, bp::kRuleAll, 2);
    const bp::Partition s2 = bp::partition(whole.fwd.data(), whole.bwd.data(), whole.last.data(), s.n, bp::kRuleSpine, 2);
    rules_differ |= !same(a2, s2);
}

int main() {
    bool rules_differ = false;
    // random sets
    for (int rep = 0; rep < 60; ++rep) {
        const uint32_t n = 1 + rnd(300);
        const Set s = make_set(n, 2 + rnd(6), rep % 2 == 1);
        check_set(s, "random", rules_differ);
    }
    CHECK(rules_differ, "no random set told the rules apart");
    // the smallest blocks: many ids in one 64-site block
    {
        Set s = make_set(200, 0, false);
        for (uint32_t a = 0; a < s.n; ++a)
            for (uint32_t b = a + 1; b < s.n; ++b) s.weak[(size_t)a * s.n + b] = a / 2 != b / 2;
        bool d = false;
        check_set(s, "pairs of sites", d);
        const bp::Breaks w = breaks_of(s, [](uint32_t, uint32_t) { return true; });
        CHECK(bp::partition(w.fwd.data(), w.bwd.data(), w.last.data(), s.n, bp::kRuleAll, 2).first.size() == 100,
              "pairs of sites: not 100 blocks");
    }
    // all weak, none weak, one site, none
    for (int windowed = 0; windowed < 2; ++windowed) {
        bool d = false;
        const Set all = make_set(150, 1, windowed), none = make_set(150, 0, windowed);
        check_set(all, "all weak", d);
        check_set(none, "no weak", d);
        const bp::Breaks wa = breaks_of(all, [](uint32_t, uint32_t) { return true; });
        const bp::Breaks wn = breaks_of(none, [](uint32_t, uint32_t) { return true; });
        for (int rule : {bp::kRuleAll, bp::kRuleSpine}) {
            CHECK(bp::partition(wa.fwd.data(), wa.bwd.data(), wa.last.data(), 150, rule, 2).first.empty(),
                  "all weak: a block");
            const bp::Partition p = bp::partition(wn.fwd.data(), wn.bwd.data(), wn.last.data(), 150, rule, 2);
            CHECK(!p.first.empty() && p.first[0] == 0 && p.last[0] == none.last[0], "no weak: first block");
            if (!windowed) CHECK(p.first.size() == 1 && p.last[0] == 149, "no weak, no window: one block");
        }
    }
    {
        bool d = false;
        check_set(make_set(1, 2, false), "one site", d);
        const uint32_t f = bp::kNone, l = 0;
        const bp::Partition p = bp::partition(&f, &f, &l, 1, bp::kRuleAll, 2);
        CHECK(p.first.empty() && p.site_block.size() == 1 && p.site_block[0] == -1, "one site");
        const bp::Partition z = bp::partition(nullptr, nullptr, nullptr, 0, bp::kRuleSpine, 2);
        CHECK(z.first.empty() && z.site_block.empty() && bp::stats_tiles(z).empty(), "no site");
    }
    // mergeable
    {
        const uint32_t la[3] = {2, 2, 2}, lb[3] = {1, 2, 2};
        CHECK(bp::mergeable(3, 0, 0.5f, la, 3, 0, 0.5f, la), "mergeable: equal");
        CHECK(!bp::mergeable(3, 0, 0.5f, la, 2, 0, 0.5f, la), "mergeable: n_sites");
        CHECK(!bp::mergeable(3, 0, 0.5f, la, 3, 1, 0.5f, la), "mergeable: stat");
        CHECK(!bp::mergeable(3, 0, 0.5f, la, 3, 0, 0.25f, la), "mergeable: strong_min");
        CHECK(!bp::mergeable(3, 0, 0.0f, la, 3, 0, -0.0f, la), "mergeable: strong_min by bits");
        CHECK(!bp::mergeable(3, 0, 0.5f, la, 3, 0, 0.5f, lb), "mergeable: last");
    }
    // the inverted key
    {
        const float v[] = {-std::numeric_limits<float>::max(), -1.5f, -std::numeric_limits<float>::denorm_min(), -0.0f,
                           0.0f, std::numeric_limits<float>::denorm_min(), 0.25f, 1.0f,
                           std::numeric_limits<float>::max()};
        const size_t n = sizeof(v) / sizeof(v[0]);
        for (size_t i = 0; i < n; ++i) {
            const float back = bp::inv_key_float(bp::inv_key(v[i]));
            CHECK(std::memcmp(&back, &v[i], 4) == 0, "inv_key round trip of %g", (double)v[i]);
            CHECK(bp::inv_key(v[i]) > bp::kNoInvKey, "inv_key of %g is the empty key", (double)v[i]);
            if (i + 1 < n) CHECK(bp::inv_key(v[i]) > bp::inv_key(v[i + 1]), "inv_key order at %zu", i);
        }
    }
    // the argument checks
    CHECK(bp::check_stat(0, 0.5f) == bp::kArgOk && bp::check_stat(1, -3.0f) == bp::kArgOk, "check_stat ok");
    CHECK(bp::check_stat(2, 0.5f) == bp::kArgStat && bp::check_stat(-1, 0.5f) == bp::kArgStat, "check_stat stat");
    CHECK(bp::check_stat(0, std::nanf("")) == bp::kArgStrongMin, "check_stat NaN");
    CHECK(bp::check_stat(0, std::numeric_limits<float>::infinity()) == bp::kArgStrongMin, "check_stat inf");
    CHECK(bp::check_rule(0, 2) == bp::kArgOk && bp::check_rule(1, 9) == bp::kArgOk, "check_rule ok");
    CHECK(bp::check_rule(2, 2) == bp::kArgRule, "check_rule rule");
    CHECK(bp::check_rule(0, 1) == bp::kArgMinSites && bp::check_rule(1, 0) == bp::kArgMinSites, "check_rule min_sites");

    if (g_fail) {
        printf("%d failures\n", g_fail);
        return 1;
    }
    printf("OK\n");
    return 0;
}
