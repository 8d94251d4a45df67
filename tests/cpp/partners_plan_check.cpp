// Host check of the best-partner lists' host-side pieces
// (weightedld_amd/csrc/partners_plan.hpp, used by capi.hip wld_run_partners and
// by the kernels in pair_partners.hip) against brute force:
//   * pack_key / key_r2 / key_partner over negatives, +-0, denormals, the
//     largest finite values and +inf, and partners up to 2^32 - 2: the unsigned
//     order of the keys is (r2 descending under float_key, then partner
//     ascending), both halves round-trip bit for bit, every key is above
//     kNoKey;
//   * build_csr() of plain, XCD-ordered (padded) and windowed tile lists, whole
//     and cut into batches: every (tile, side) of the batch under exactly its
//     block, in list order, positions relative to the batch;
//   * batches(): a partition of the list in order, every batch within the
//     byte budget unless it is a single tile; staging_bytes by hand;
//   * considered_pairs() against a double loop, under random windows and every
//     chunk range of small sets;
//   * merge_lists() / merge(): the best k of the union of two lists against a
//     sort, the merge of results over a random split of a pair set against the
//     result of the whole set, counters and tiles add, times the larger.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "partners_plan.hpp"
#include "window_plan.hpp"

using namespace wld;
namespace pp = wld::partners_plan;

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

static uint32_t bits_of(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}

// ---- keys ----------------------------------------------------------------
static void check_keys() {
    const float inf = std::numeric_limits<float>::infinity();
    // ascending in the total order: -0 below +0
    const float vals[] = {-3.4028235e38f, -1.0f, -1e-30f, -1e-45f, -0.0f, 0.0f, 1e-45f, 1e-38f, 0.1f,
                          0.99999994f,    1.0f,  1.0000001f, 3.4028235e38f, inf};
    const uint32_t partners[] = {0u, 1u, 63u, 64u, 70000u, 0x7FFFFFFFu, 0xFFFFFFFEu};
    const size_t nv = sizeof(vals) / sizeof(vals[0]), np = sizeof(partners) / sizeof(partners[0]);
    for (size_t i = 0; i < nv; ++i)
        for (size_t p = 0; p < np; ++p) {
            const uint64_t k = pp::pack_key(vals[i], partners[p]);
            CHECK(k > pp::kNoKey, "key of %g is not above kNoKey", (double)vals[i]);
            CHECK(bits_of(pp::key_r2(k)) == bits_of(vals[i]), "r2 %g does not round-trip", (double)vals[i]);
            CHECK(pp::key_partner(k) == partners[p], "partner %u does not round-trip", partners[p]);
            for (size_t j = 0; j < nv; ++j)
                for (size_t q = 0; q < np; ++q) {
                    const uint64_t k2 = pp::pack_key(vals[j], partners[q]);
                    // first in the order = larger key: r2 descending, then partner ascending
                    const bool first = i > j || (i == j && partners[p] < partners[q]);
                    CHECK((k > k2) == first, "order of (%g, %u) and (%g, %u)", (double)vals[i], partners[p],
                          (double)vals[j], partners[q]);
                }
        }
    // random bit patterns (no NaN): the key order is the order of float_key, then partner
    for (int t = 0; t < 20000; ++t) {
        uint32_t u1 = rnd(1u << 16) << 16 | rnd(1u << 16), u2 = rnd(4) ? rnd(1u << 16) << 16 | rnd(1u << 16) : u1;
        float x, y;
        memcpy(&x, &u1, 4);
        memcpy(&y, &u2, 4);
        if (x != x || y != y) continue;
        const uint32_t p = rnd(1000), q = rnd(1000);
        const uint32_t kx = heatmap_plan::float_key(x), ky = heatmap_plan::float_key(y);
        const bool first = kx > ky || (kx == ky && p < q);
        CHECK((pp::pack_key(x, p) > pp::pack_key(y, q)) == first, "random order %08x %u / %08x %u", u1, p, u2, q);
        if (x < y) CHECK(kx < ky, "float_key is not monotone at %08x %08x", u1, u2);
    }
}

// ---- CSR and batches -------------------------------------------------------
static void check_csr_of(const std::vector<uint32_t> &t, uint32_t n_blocks, uint64_t batch_bytes, uint32_t kp) {
    const auto cuts = pp::batches(t.size(), batch_bytes, kp);
    uint64_t at = 0;
    for (const auto &c : cuts) {
        CHECK(c.first == at && c.second > c.first && c.second <= t.size(), "batch [%" PRIu64 ", %" PRIu64 ") at %" PRIu64,
              c.first, c.second, at);
        at = c.second;
        const uint64_t n = c.second - c.first;
        CHECK(n == 1 || pp::staging_bytes(n, kp) <= batch_bytes, "a batch of %" PRIu64 " tiles over the budget", n);
        CHECK(c.second == t.size() || n == pp::batch_tiles(batch_bytes, kp), "a short batch before the last");
        const pp::Csr csr = pp::build_csr(t.data(), c.first, c.second, n_blocks);
        CHECK(csr.off.size() == (size_t)n_blocks + 1 && csr.off[0] == 0 && csr.off[n_blocks] == csr.ent.size(),
              "csr offsets");
        // brute force: per block, scan the batch
        for (uint32_t b = 0; b < n_blocks; ++b) {
            std::vector<uint32_t> want;
            for (uint64_t p = c.first; p < c.second; ++p) {
                if (t[p] == tile_order::kNoTileEntry) continue;
                if ((t[p] >> 16) == b) want.push_back((uint32_t)(2 * (p - c.first)));
                if ((t[p] & 0xFFFFu) == b) want.push_back((uint32_t)(2 * (p - c.first) + 1));
            }
            CHECK(csr.off[b] <= csr.off[b + 1] && csr.off[b + 1] <= csr.ent.size(), "csr range of block %u", b);
            const std::vector<uint32_t> got(csr.ent.begin() + csr.off[b], csr.ent.begin() + csr.off[b + 1]);
            CHECK(got == want, "csr entries of block %u (%zu, want %zu)", b, got.size(), want.size());
            for (uint32_t e : got) CHECK(e < pp::parts_of(n) / pp::kTileSide, "entry %u past the batch's parts", e);
        }
    }
    CHECK(at == t.size(), "the batches end at %" PRIu64 " of %zu", at, t.size());
}

static void check_csr() {
    CHECK(pp::tile_bytes(8) == 128 * (8 * 16 + 4) && pp::staging_bytes(3, 64) == 3ull * 128 * (64 * 16 + 4) &&
              pp::parts_of(5) == 640 && sizeof(pp::Entry) == 16,
          "staging sizes");
    CHECK(pp::batch_tiles(1, 64) == 1 && pp::batch_tiles(pp::tile_bytes(5) * 7 + 1, 5) == 7, "batch_tiles");
    CHECK(pp::batches(0, 100, 4).empty(), "an empty list has no batch");
    for (uint32_t L : {1u, 64u, 65u, 300u, 600u, 1500u}) {
        const uint32_t T = (L + 63) / 64, n = (L + 255) / 256, nc = n * (n + 1) / 2;
        for (int rep = 0; rep < 4; ++rep) {
            uint32_t lb = rep ? rnd(nc + 1) : 0, le = rep ? rnd(nc + 1) : nc;
            if (lb > le) std::swap(lb, le);
            std::vector<uint32_t> t = tile_order::range_tiles(n, T, lb, le);
            for (uint32_t kp : {1u, 5u, 64u})
                for (uint64_t bytes : {(uint64_t)1, 3 * pp::tile_bytes(kp), (uint64_t)1 << 30})
                    check_csr_of(t, T, bytes, kp);
            if (!t.empty()) {
                const std::vector<uint32_t> x = tile_order::xcd_order(t, 8);  // (padded with empty entries)
                check_csr_of(x, T, 5 * pp::tile_bytes(8) + 3, 8);
            }
            // a windowed list
            std::vector<uint32_t> hi(L);
            for (uint32_t a = 0; a < L; ++a) hi[a] = std::min(L - 1, a + rnd(100));
            for (uint32_t a = 1; a < L; ++a) hi[a] = std::max(hi[a], hi[a - 1]);
            check_csr_of(window_plan::range_tiles(n, T, lb, le, hi), T, 2 * pp::tile_bytes(3), 3);
        }
    }
}

// ---- considered pairs --------------------------------------------------------
static void check_pairs() {
    for (uint32_t L : {0u, 1u, 2u, 255u, 256u, 257u, 600u, 777u}) {
        const uint32_t n = (L + 255) / 256, nc = n * (n + 1) / 2;
        for (int win = 0; win < 3; ++win) {
            std::vector<uint32_t> hi(L);
            for (uint32_t a = 0; a < L; ++a) hi[a] = win == 0 ? L - 1 : std::min(L - 1, a + rnd(win == 1 ? 40 : 400));
            std::vector<uint64_t> per(nc + 1, 0);
            for (uint32_t a = 0; a < L; ++a)
                for (uint32_t b = a + 1; b <= hi[a] && b < L; ++b)
                    ++per[tile_order::chunk_linear_host(n, a / 256, b / 256)];
            for (uint32_t lb = 0; lb <= nc; ++lb)
                for (uint32_t le = lb; le <= nc; ++le) {
                    uint64_t want = 0;
                    for (uint32_t c = lb; c < le; ++c) want += per[c];
                    const uint64_t got = pp::considered_pairs(win ? hi.data() : nullptr, L, lb, le);
                    CHECK(got == want, "pairs L %u win %d [%u,%u): %" PRIu64 " want %" PRIu64, L, win, lb, le, got, want);
                }
        }
    }
}

// ---- merge -------------------------------------------------------------------
static bool same_entry(const pp::Entry &x, const pp::Entry &y) {
    return x.key == y.key && bits_of(x.d) == bits_of(y.d) && bits_of(x.dp) == bits_of(y.dp);
}

// the result of a set of (site, partner, r2) candidates, by sorting
static pp::Partners result_of(const std::vector<std::vector<pp::Entry>> &cand, uint32_t k) {
    pp::Partners p;
    p.n_sites = (uint32_t)cand.size();
    p.k = k;
    p.list.assign((size_t)p.n_sites * k, pp::Entry{pp::kNoKey, 0.0f, 0.0f});
    for (uint32_t s = 0; s < p.n_sites; ++s) {
        std::vector<pp::Entry> c = cand[s];
        std::sort(c.begin(), c.end(), [](const pp::Entry &x, const pp::Entry &y) { return x.key > y.key; });
        for (uint32_t i = 0; i < k && i < c.size(); ++i) p.list[(size_t)s * k + i] = c[i];
    }
    return p;
}

static void check_merge() {
    for (int rep = 0; rep < 60; ++rep) {
        const uint32_t L = 1 + rnd(40), k = 1 + rnd(rep % 3 ? 8 : 64);
        std::vector<std::vector<pp::Entry>> all(L), one(L), two(L);
        for (uint32_t s = 0; s < L; ++s) {
            const uint32_t m = rnd(3) ? rnd(3 * k + 1) : 0;
            for (uint32_t i = 0; i < m; ++i) {
                const uint32_t partner = 100 * i + rnd(100);  // distinct partners: distinct keys
                const float r2 = rnd(3) ? (float)rnd(8) / 8.0f : (float)rnd(1000) / 999.0f;  // many ties
                const pp::Entry e{pp::pack_key(r2, partner), (float)rnd(100) - 50.0f, (float)rnd(100) / 100.0f};
                all[s].push_back(e);
                (rnd(2) ? one : two)[s].push_back(e);
            }
        }
        pp::Partners a = result_of(one, k), b = result_of(two, k);
        const pp::Partners whole = result_of(all, k);
        a.pairs = 10, a.none_pairs = 2, a.passing_pairs = 5, a.tiles = 3, a.kernel_ms = 1.5, a.merge_ms = 0.25;
        b.pairs = 7, b.none_pairs = 1, b.passing_pairs = 4, b.tiles = 2, b.kernel_ms = 0.5, b.merge_ms = 0.75;
        pp::Partners m = a;
        pp::merge(m, b);
        CHECK(m.n_sites == L && m.k == k && m.list.size() == whole.list.size(), "merged shape");
        for (size_t i = 0; i < whole.list.size() && i < m.list.size(); ++i)
            CHECK(same_entry(m.list[i], whole.list[i]), "merged entry %zu (L %u k %u)", i, L, k);
        CHECK(m.pairs == 17 && m.none_pairs == 3 && m.passing_pairs == 9 && m.tiles == 5 && m.kernel_ms == 1.5 &&
                  m.merge_ms == 0.75,
              "merged counters");
        // the other way round, and into an empty result
        pp::Partners r = b;
        pp::merge(r, a);
        for (size_t i = 0; i < whole.list.size() && i < r.list.size(); ++i)
            CHECK(same_entry(r.list[i], whole.list[i]), "merge is symmetric at %zu", i);
        pp::Partners z;
        pp::merge(z, a);
        CHECK(z.n_sites == L && z.k == k && z.pairs == 10 && z.list.size() == a.list.size(), "merge into an empty result");
        for (size_t i = 0; i < a.list.size() && i < z.list.size(); ++i)
            CHECK(same_entry(z.list[i], a.list[i]), "empty + a at %zu", i);
    }
}

int main() {
    check_keys();
    check_csr();
    check_pairs();
    check_merge();
    if (g_fail) {
        printf("%d checks failed\n", g_fail);
        return 1;
    }
    printf("partners_plan_check OK\n");
    return 0;
}
