// Host check of the LD summary's host-side pieces
// (weightedld_amd/csrc/summary_plan.hpp, used by capi.hip wld_run_summary and
// by the kernel's epilogue in pair_summary.hip) against brute force:
//   * bin_index(dist, bin_width, n_bins) against the definition — the largest
//     k with k * bin_width <= dist (found by counting up in 128-bit
//     arithmetic, no division), capped at n_bins - 1 — over widths 1, small,
//     2^32 +- 1 and near 2^64, distances on and beside every bin edge, in the
//     overflow bin, beyond 32 bits and up to 2^64 - 1, n_bins 1, 2, 7 and 1024;
//   * merge() against summaries of a pair list split in two at every point of
//     a grid: the counts and integer arrays of the parts add up exactly to
//     the whole's, the f64 arrays to within the rounding of one more addition,
//     a merge into an empty summary copies, and kernel_ms is the larger one.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "summary_plan.hpp"

using namespace wld;
using summary_plan::Summary;

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

// the definition, without a division
static uint32_t bin_ref(uint64_t dist, uint64_t w, uint32_t n_bins) {
    uint32_t k = 0;
    while (k + 1 < n_bins && (unsigned __int128)(k + 1) * w <= dist) ++k;
    return k;
}

static uint64_t g_checked = 0;
static void check_bin(uint64_t dist, uint64_t w, uint32_t n_bins) {
    const uint32_t got = summary_plan::bin_index(dist, w, n_bins), ref = bin_ref(dist, w, n_bins);
    ++g_checked;
    CHECK(got == ref, "bin_index(%" PRIu64 ", %" PRIu64 ", %u) = %u, brute force %u", dist, w, n_bins, got, ref);
    CHECK(got < n_bins, "bin_index(%" PRIu64 ", %" PRIu64 ", %u) = %u out of range", dist, w, n_bins, got);
}

static void check_bins() {
    const uint64_t widths[] = {1, 2, 3, 7, 8, 1000, 65536, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull,
                               0x123456789ABull, 1ull << 53, 1ull << 63, ~0ull};
    const uint32_t counts[] = {1, 2, 7, 1024};
    for (uint64_t w : widths)
        for (uint32_t nb : counts) {
            // every edge k * w (where it fits), one below, one above; 0; the
            // overflow bin's start and far beyond it; the 32-bit boundary
            for (uint32_t k = 0; k <= nb + 1; ++k) {
                const unsigned __int128 e = (unsigned __int128)k * w;
                if (e >> 64) break;
                const uint64_t d = (uint64_t)e;
                check_bin(d, w, nb);
                if (d) check_bin(d - 1, w, nb);
                if (d != ~0ull) check_bin(d + 1, w, nb);
            }
            const uint64_t extra[] = {0, 1, 0xFFFFFFFEull, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull,
                                      1ull << 40, (1ull << 63) - 1, 1ull << 63, ~0ull - 1, ~0ull};
            for (uint64_t d : extra) check_bin(d, w, nb);
        }
    // bin_width 1: the bin is the distance itself up to the overflow bin
    for (uint64_t d = 0; d < 3000; ++d) {
        const uint32_t got = summary_plan::bin_index(d, 1, 1024);
        CHECK(got == (d < 1023 ? (uint32_t)d : 1023u), "width 1: bin_index(%" PRIu64 ") = %u", d, got);
    }
    // pseudo-random distances and widths, 64-bit positions
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 200000; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const uint64_t d = s >> (s % 61);
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const uint64_t w = (s >> (s % 63)) | 1;
        check_bin(d, w, counts[i & 3]);
    }
}

// the summary of pairs [lo, hi) of a fixed pseudo-random pair list: L sites,
// nb bins, score and bins accumulated in list order
struct PairRec {
    uint32_t a, b, bin;
    int cls;  // 0 none, 1 nonfinite, 2 counted
    double r2;
};

static Summary summarize(const std::vector<PairRec> &p, size_t lo, size_t hi, uint32_t L, uint32_t nb, double ms) {
    Summary s;
    s.score.assign(L, 0.0);
    s.partners.assign(L, 0);
    s.bin_pairs.assign(nb, 0);
    s.bin_r2_sum.assign(nb, 0.0);
    s.kernel_ms = ms;
    for (size_t i = lo; i < hi; ++i) {
        ++s.pairs;
        if (p[i].cls == 0) ++s.none_pairs;
        else if (p[i].cls == 1) ++s.nonfinite_pairs;
        else {
            ++s.counted_pairs;
            s.r2_sum += p[i].r2;
            s.score[p[i].a] += p[i].r2;
            s.score[p[i].b] += p[i].r2;
            ++s.partners[p[i].a];
            ++s.partners[p[i].b];
            if (nb) {
                ++s.bin_pairs[p[i].bin];
                s.bin_r2_sum[p[i].bin] += p[i].r2;
            }
        }
    }
    return s;
}

// |x - y| within n roundings of an any-order sum of n nonnegative terms
static bool close_sum(double x, double y, uint64_t n) { return std::fabs(x - y) <= (double)(n + 1) * 0x1p-52 * y; }

static void check_merge(uint32_t L, uint32_t nb) {
    std::vector<PairRec> p;
    uint64_t s = 0xD1B54A32D192ED03ull + L * 131 + nb;
    for (uint32_t a = 0; a < L; ++a)
        for (uint32_t b = a + 1; b < L; ++b) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            PairRec r;
            r.a = a;
            r.b = b;
            r.bin = nb ? summary_plan::bin_index(b - a, 3, nb) : 0;
            const unsigned c = (unsigned)(s >> 60);
            r.cls = c == 0 ? 0 : c == 1 ? 1 : 2;
            r.r2 = (double)(float)((double)((s >> 20) & 0xFFFFFF) / 16777216.0);
            p.push_back(r);
        }
    const Summary whole = summarize(p, 0, p.size(), L, nb, 3.0);
    const size_t step = p.size() / 9 + 1;
    for (size_t cut = 0; cut <= p.size(); cut += step) {
        Summary x = summarize(p, 0, cut, L, nb, 1.0);
        const Summary y = summarize(p, cut, p.size(), L, nb, 2.0);
        summary_plan::merge(x, y);
        CHECK(x.pairs == whole.pairs && x.none_pairs == whole.none_pairs &&
                  x.nonfinite_pairs == whole.nonfinite_pairs && x.counted_pairs == whole.counted_pairs,
              "merge at %zu: class counts", cut);
        CHECK(x.pairs == x.none_pairs + x.nonfinite_pairs + x.counted_pairs, "merge at %zu: identity", cut);
        CHECK(x.partners == whole.partners, "merge at %zu: partners", cut);
        CHECK(x.bin_pairs == whole.bin_pairs, "merge at %zu: bin_pairs", cut);
        CHECK(x.kernel_ms == 2.0, "merge at %zu: kernel_ms %g", cut, x.kernel_ms);
        CHECK(close_sum(x.r2_sum, whole.r2_sum, whole.counted_pairs), "merge at %zu: r2_sum %.17g vs %.17g", cut,
              x.r2_sum, whole.r2_sum);
        uint64_t np = 0, nbp = 0;
        for (uint32_t i = 0; i < L; ++i) {
            np += x.partners[i];
            CHECK(close_sum(x.score[i], whole.score[i], whole.partners[i]), "merge at %zu: score[%u]", cut, i);
        }
        for (uint32_t k = 0; k < nb; ++k) {
            nbp += x.bin_pairs[k];
            CHECK(close_sum(x.bin_r2_sum[k], whole.bin_r2_sum[k], whole.bin_pairs[k]), "merge at %zu: bin %u", cut, k);
        }
        CHECK(np == 2 * x.counted_pairs, "merge at %zu: sum of partners", cut);
        CHECK(!nb || nbp == x.counted_pairs, "merge at %zu: sum of bin_pairs", cut);
        CHECK(x.score.size() == L && x.bin_r2_sum.size() == nb, "merge at %zu: array lengths", cut);
    }
    // into an empty summary: a copy, bit for bit
    Summary e;
    summary_plan::merge(e, whole);
    CHECK(e.pairs == whole.pairs && e.counted_pairs == whole.counted_pairs && e.r2_sum == whole.r2_sum &&
              e.score == whole.score && e.partners == whole.partners && e.bin_pairs == whole.bin_pairs &&
              e.bin_r2_sum == whole.bin_r2_sum && e.kernel_ms == whole.kernel_ms,
          "merge into an empty summary (L %u, %u bins)", L, nb);
}

int main() {
    check_bins();
    check_merge(1, 0);
    check_merge(2, 1);
    check_merge(37, 0);
    check_merge(37, 1);
    check_merge(90, 16);
    check_merge(64, 1024);
    if (g_fail) {
        printf("%d failures\n", g_fail);
        return 1;
    }
    printf("%" PRIu64 " bin indices, 6 merge cases\nOK\n", g_checked);
    return 0;
}
