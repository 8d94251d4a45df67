// Host check of the fp6 screen's fp4 A image (no device code runs;
// tests/test_f6_a4.py builds this plain and under AddressSanitizer +
// UndefinedBehaviorSanitizer).
//
// Part 1 (fp6_scale.hpp fp6_to_fp4_code): the e2m3 -> e2m1 code map keeps the
// value on exactly the eight codes 0, 4, ..., 28 (0, 0.5, 1, 1.5, 2, 3, 4, 6)
// and rejects the other 24.
// Part 2 (fp6_choose_scale + fp6_codes_fit_fp4): the committed scale rule puts
// unit, constant, {1, 0.5}, {1, 0.75}, {0.25, 0.5, 1, 1} and narrow
// Henikoff-like weights on e2m1 values, and {1, 0.875}, uniform [0.9, 1] and a
// set spread over 2^4 not; with a file of f32 weights as argv[1] and a code
// count as argv[2] (the GPU tests' "spread" set) it checks that set too.
// Part 3 (fp6_pack.hpp f6_pack_lane): for random symbols and fitting codes the
// fp4 A lane dwords and the fp6 A lane dwords decode to the same values at
// every (site, sequence), and to the values the coding defines, over the
// image's own lane map, padded sequences (N <= k < NP) and sequence counts
// that are no multiple of 128; the B dwords do not depend on the A format.
// Part 4: a 16 x 16 x 128 block's four sums (missing / minor channel x B raw
// / B's minor bit), formed in f32 from either decoding, agree bit for bit.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "fp6_pack.hpp"
#include "fp6_scale.hpp"

namespace {
int g_fail = 0;
#define CHECK(cond, ...)                                 \
    do {                                                 \
        if (!(cond)) {                                   \
            if (++g_fail <= 20) {                        \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);                \
                std::printf("\n");                       \
            }                                            \
        }                                                \
    } while (0)

uint32_t bits_of(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    return u;
}

void map_part() {
    const double e2m1[8] = {0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0};
    int kept = 0;
    for (uint32_t c = 0; c < 8; ++c) CHECK(wld::fp4_value(c) == e2m1[c], "e2m1 code %u: %g", c, wld::fp4_value(c));
    for (uint32_t c = 0; c < 32; ++c) {
        double v;
        CHECK(wld::fp6_code(wld::fp6_value(c), &v) == c && v == wld::fp6_value(c), "e2m3 code %u: value %g", c,
              wld::fp6_value(c));
        const int m = wld::fp6_to_fp4_code(c);
        bool is_e2m1 = false;
        for (double x : e2m1) is_e2m1 = is_e2m1 || x == wld::fp6_value(c);
        CHECK((m >= 0) == is_e2m1 && (m >= 0) == (c % 4 == 0), "code %u (%g): map %d", c, wld::fp6_value(c), m);
        if (m >= 0) {
            ++kept;
            CHECK(m < 8 && wld::fp4_value((uint32_t)m) == wld::fp6_value(c), "code %u: %g -> %d: %g", c,
                  wld::fp6_value(c), m, wld::fp4_value((uint32_t)m));
        }
    }
    CHECK(kept == 8, "%d codes kept", kept);
    CHECK(wld::fp6_to_fp4_code(32) < 0 && wld::fp6_to_fp4_code(0x84) < 0, "codes past 31");
}

// the committed rule's codes of a weight set
std::vector<uint8_t> codes_of(const std::vector<float> &w) {
    double wmax = 0.0, v;
    for (float x : w) wmax = std::max(wmax, (double)x);
    const double S = wld::fp6_choose_scale(w.data(), w.size(), wmax).S;
    std::vector<uint8_t> c(w.size());
    for (size_t k = 0; k < w.size(); ++k) c[k] = (uint8_t)wld::fp6_code(S * (double)w[k], &v);
    return c;
}
void rule_case(const char *name, const std::vector<float> &w, const std::set<int> &want, int want_count, bool fits) {
    const std::vector<uint8_t> c = codes_of(w);
    const std::set<int> got(c.begin(), c.end());
    std::printf("rule %-12s N %5zu: %zu code(s):", name, w.size(), got.size());
    for (int x : got) std::printf(" %d", x);
    const bool f = wld::fp6_codes_fit_fp4(c.data(), c.size());
    std::printf("  fits e2m1: %s\n", f ? "yes" : "no");
    if (!want.empty()) CHECK(got == want, "%s: codes differ from the table", name);
    if (want_count > 0) CHECK((int)got.size() == want_count, "%s: %zu codes, not %d", name, got.size(), want_count);
    CHECK(f == fits, "%s: fits %d", name, (int)f);
}
void rule_part(const char *spread_file, int spread_count) {
    std::mt19937_64 rng(0xA4A4ull);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    auto rep2 = [](size_t n, float a, float b) {
        std::vector<float> w(n);
        for (size_t k = 0; k < n; ++k) w[k] = k % 2 ? b : a;
        return w;
    };
    std::vector<float> narrow(2000), tenth(2000), spread(130);
    for (float &x : narrow) x = (float)(0.965 + 0.035 * u(rng));
    for (float &x : tenth) x = (float)(0.9 + 0.1 * u(rng));
    for (float &x : spread) x = (float)std::exp2(-4.0 * u(rng));
    rule_case("unit", std::vector<float>(130, 1.0f), {24}, 0, true);
    rule_case("const 0.37", std::vector<float>(130, 0.37f), {24}, 0, true);
    rule_case("{1, 0.5}", rep2(130, 1.0f, 0.5f), {24, 16}, 0, true);
    rule_case("{1, 0.75}", rep2(130, 1.0f, 0.75f), {24, 20}, 0, true);
    rule_case("quarter..1", {0.25f, 0.5f, 1.0f, 1.0f}, {8, 16, 24}, 0, true);
    rule_case("[0.965, 1]", narrow, {24}, 0, true);
    rule_case("{1, 0.875}", rep2(130, 1.0f, 0.875f), {24, 22}, 0, false);
    rule_case("[0.9, 1]", tenth, {23, 24}, 0, false);
    rule_case("spread", spread, {}, 0, false);
    if (spread_file) {
        std::vector<float> w;
        if (FILE *f = std::fopen(spread_file, "rb")) {
            float x;
            while (std::fread(&x, sizeof x, 1, f) == 1) w.push_back(x);
            std::fclose(f);
        }
        CHECK(!w.empty(), "no weights in %s", spread_file);
        if (!w.empty()) rule_case("spread/file", w, {}, spread_count, false);
    }
}

enum : uint8_t { kMiss = 0, kMinor = 1, kMajor = 3 };  // kernels.hpp: kCodeIn = 1, kCodeMaj = 2

// One 16-site block's operand image of one format over NK 128-sequence
// blocks, laid out by lane as frag6_kernel does: lane l = site l & 15,
// sequences 128 kb + 32 (l >> 4) + j.
struct Lane {
    uint32_t ai[6], am[6], b[4];
};
template <bool kA4>
std::vector<Lane> image(const std::vector<std::vector<uint8_t>> &sym, const std::vector<uint8_t> &wa, size_t NP) {
    const size_t NK = (NP + 127) / 128;
    std::vector<Lane> img(NK * 64);
    for (size_t kb = 0; kb < NK; ++kb)
        for (uint32_t l = 0; l < 64; ++l) {
            const size_t k0 = 128 * kb + 32 * (l >> 4);
            const uint32_t n = k0 < NP ? (uint32_t)std::min<size_t>(32, NP - k0) : 0u;
            Lane &o = img[kb * 64 + l];
            // (past NP nothing is read: n = 0 there, and the arrays end at NP)
            wld::f6_pack_lane<kA4>(sym[l & 15].data() + std::min(k0, NP), wa.data() + std::min(k0, NP), n, o.ai, o.am,
                                   o.b);
        }
    return img;
}

uint64_t pack_part() {
    std::mt19937_64 rng(0xF4A6ull);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    uint64_t values = 0;
    const uint8_t fit[8] = {0, 4, 8, 12, 16, 20, 24, 28};
    // (N, NP): the padded count a multiple of 64 as well as of 128, so that whole lanes lie past NP
    const size_t shapes[][2] = {{1, 64}, {1, 128}, {31, 64}, {127, 128}, {128, 128}, {130, 192}, {130, 256}, {300, 320}};
    for (const auto &sh : shapes) {
        const size_t N = sh[0], NP = sh[1], NK = (NP + 127) / 128;
        for (int rep = 0; rep < 40; ++rep) {
            std::vector<uint8_t> w6(NP, 0), w4(NP, 0);
            for (size_t k = 0; k < N; ++k) {
                w6[k] = rep == 0 ? 24 : rep == 1 ? 28 : fit[rng() % 8];
                w4[k] = (uint8_t)wld::fp6_to_fp4_code(w6[k]);
            }
            CHECK(wld::fp6_codes_fit_fp4(w6.data(), N), "fitting codes refused");
            const double p_miss = rep % 4 == 3 ? 0.9 : 0.1;
            std::vector<std::vector<uint8_t>> a(16, std::vector<uint8_t>(NP, kMiss)), b = a;
            for (auto *s : {&a, &b})
                for (auto &row : *s)
                    for (size_t k = 0; k < N; ++k) row[k] = u(rng) < p_miss ? kMiss : u(rng) < 0.3 ? kMinor : kMajor;
            const std::vector<Lane> a6 = image<false>(a, w6, NP), a4 = image<true>(a, w4, NP);
            const std::vector<Lane> b6 = image<false>(b, w6, NP), b4 = image<true>(b, w4, NP);
            for (size_t i = 0; i < a6.size(); ++i) {
                const uint32_t l = (uint32_t)(i % 64);
                const size_t k0 = 128 * (i / 64) + 32 * (l >> 4);
                CHECK(a4[i].ai[4] == 0 && a4[i].ai[5] == 0 && a4[i].am[4] == 0 && a4[i].am[5] == 0, "fp4 dwords 4-5");
                CHECK(std::memcmp(b6[i].b, b4[i].b, sizeof b6[i].b) == 0 && std::memcmp(a6[i].b, a4[i].b, 16) == 0,
                      "N %zu lane %u: B dwords depend on the A format", N, l);
                for (uint32_t j = 0; j < 32; ++j) {
                    const size_t k = k0 + j;
                    const uint8_t s = k < NP ? a[l & 15][k] : (uint8_t)kMiss;
                    const double wv = k < N ? wld::fp6_value(w6[k]) : 0.0;
                    const double want_i = s == kMiss ? wv : 0.0, want_m = s == kMinor ? wv : 0.0;
                    const double i6 = wld::fp6_value(wld::f6_lane_code6(a6[i].ai, j)),
                                 m6 = wld::fp6_value(wld::f6_lane_code6(a6[i].am, j)),
                                 i4 = wld::fp4_value(wld::f6_lane_code4(a4[i].ai, j)),
                                 m4 = wld::fp4_value(wld::f6_lane_code4(a4[i].am, j));
                    CHECK(i6 == i4 && m6 == m4 && i6 == want_i && m6 == want_m,
                          "N %zu NP %zu rep %d site %u k %zu: missing %g/%g/%g minor %g/%g/%g", N, NP, rep, l & 15, k, i6,
                          i4, want_i, m6, m4, want_m);
                    const uint32_t nb = wld::f6_lane_code4(a6[i].b, j);
                    CHECK(nb == (k < NP ? (s == kMiss ? 4u : s == kMinor ? 2u : 0u) : 0u), "B nibble %u at k %zu", nb, k);
                    values += 2;
                }
            }
            // the block's four sums, per (a site, b site), summed in f32 over the K order of the operand
            for (uint32_t sa = 0; sa < 16; ++sa)
                for (uint32_t sb = 0; sb < 16; ++sb) {
                    float s6[4] = {0, 0, 0, 0}, s4[4] = {0, 0, 0, 0};
                    for (size_t kb = 0; kb < NK; ++kb)
                        for (uint32_t g = 0; g < 4; ++g)
                            for (uint32_t j = 0; j < 32; ++j) {
                                const Lane &A6 = a6[kb * 64 + 16 * g + sa], &A4 = a4[kb * 64 + 16 * g + sa],
                                           &B = b4[kb * 64 + 16 * g + sb];
                                const uint32_t nb = wld::f6_lane_code4(B.b, j);
                                const float braw = (float)wld::fp4_value(nb), bmin = (float)wld::fp4_value(nb & 2u);
                                const float i6 = (float)wld::fp6_value(wld::f6_lane_code6(A6.ai, j)),
                                            m6 = (float)wld::fp6_value(wld::f6_lane_code6(A6.am, j)),
                                            i4 = (float)wld::fp4_value(wld::f6_lane_code4(A4.ai, j)),
                                            m4 = (float)wld::fp4_value(wld::f6_lane_code4(A4.am, j));
                                s6[0] += i6 * braw, s6[1] += i6 * bmin, s6[2] += m6 * braw, s6[3] += m6 * bmin;
                                s4[0] += i4 * braw, s4[1] += i4 * bmin, s4[2] += m4 * braw, s4[3] += m4 * bmin;
                            }
                    for (int q = 0; q < 4; ++q)
                        CHECK(bits_of(s6[q]) == bits_of(s4[q]), "N %zu rep %d sites %u x %u sum %d: %a / %a", N, rep, sa,
                              sb, q, s6[q], s4[q]);
                }
        }
    }
    return values;
}
}  // namespace

int main(int argc, char **argv) {
    map_part();
    rule_part(argc > 2 ? argv[1] : nullptr, argc > 2 ? std::atoi(argv[2]) : 0);
    const uint64_t values = pack_part();
    std::printf("packing: %" PRIu64 " operand values in both formats\n", values);
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
