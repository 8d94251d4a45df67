// Host check of the fp6 screen's shared code image (no device code runs;
// tests/test_f6_shared.py builds this plain and under AddressSanitizer +
// UndefinedBehaviorSanitizer).
//
// Part 1 (fp6_scale.hpp fp6_shared_code): the qualification: one nonzero code
// for every sequence, whatever the code; refused for mixed codes, a zero code
// among them, codes past 31 and N = 0; N = 1 qualifies.  Under the committed
// scale rule unit and constant weights qualify, two-valued ones do not.
// Part 2 (fp6_pack.hpp f6_pack_lane_shared): masking a shared-image dword with
// kF6MaskMissing / kF6MaskMinor gives exactly the nibbles the fp4 A image
// (f6_pack_lane<true>) packs for the same symbols at the weight codes of 2.0
// and 1.0, over frag6_kernel's lane map, sequence counts that are no multiple
// of 32 or 128 and a padded tail (N <= k < NP), which the shared image codes 0
// (no nibble set) where the B image of the other formats codes it missing.
// Part 3 (pair_common.hpp f6s_direct): for every e2m3 code c, the shared
// image's four count accumulators restored with f6s_direct equal, bit for
// bit, the complement coding's accumulators restored with f6c_direct and the
// direct sums X0, Y0, X1, Y1 formed per sequence in f64: exhaustive 2 x 2
// tables of up to 6 sequences, and random tables up to N = 2,048.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "fp6_pack.hpp"
#include "fp6_scale.hpp"
#include "pair_common.hpp"

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

enum : uint8_t { kMiss = 0, kMinor = 1, kMajor = 3 };  // kernels.hpp: kCodeIn = 1, kCodeMaj = 2

std::vector<uint8_t> codes_of(const std::vector<float> &w) {
    double wmax = 0.0, v;
    for (float x : w) wmax = std::max(wmax, (double)x);
    const double S = wld::fp6_choose_scale(w.data(), w.size(), wmax).S;
    std::vector<uint8_t> c(w.size());
    for (size_t k = 0; k < w.size(); ++k) c[k] = (uint8_t)wld::fp6_code(S * (double)w[k], &v);
    return c;
}

void qualify_part() {
    for (uint32_t c = 1; c < 32; ++c)
        for (size_t N : {(size_t)1, (size_t)2, (size_t)130, (size_t)2048}) {
            std::vector<uint8_t> w(N, (uint8_t)c);
            CHECK(wld::fp6_shared_code(w.data(), N) == c, "code %u N %zu refused", c, N);
            if (N > 1) {
                for (size_t at : {(size_t)0, N / 2, N - 1}) {
                    std::vector<uint8_t> m = w;
                    m[at] = (uint8_t)(c == 31 ? 30 : c + 1);
                    CHECK(wld::fp6_shared_code(m.data(), N) == 0, "mixed codes %u at %zu of %zu taken", c, at, N);
                    m[at] = 0;
                    CHECK(wld::fp6_shared_code(m.data(), N) == 0, "a zero code at %zu of %zu taken", at, N);
                }
            }
        }
    const uint8_t zero[4] = {0, 0, 0, 0}, big[2] = {32, 32};
    CHECK(wld::fp6_shared_code(zero, 4) == 0 && wld::fp6_shared_code(zero, 1) == 0, "all-zero codes taken");
    CHECK(wld::fp6_shared_code(big, 2) == 0, "codes past 31 taken");
    CHECK(wld::fp6_shared_code(zero, 0) == 0, "N = 0 taken");
    // the committed scale rule: unit and constant weights sit on 4.0 (code 24), a single sequence too
    for (const std::vector<float> &w : {std::vector<float>(130, 1.0f), std::vector<float>(1, 1.0f),
                                        std::vector<float>(2000, 0.37f), std::vector<float>(1, 0.001f)}) {
        const std::vector<uint8_t> c = codes_of(w);
        CHECK(wld::fp6_shared_code(c.data(), c.size()) == 24, "constant %g x %zu: code %u", w[0], w.size(),
              wld::fp6_shared_code(c.data(), c.size()));
    }
    std::vector<float> two(130, 1.0f);
    for (size_t k = 1; k < two.size(); k += 2) two[k] = 0.5f;
    const std::vector<uint8_t> c2 = codes_of(two);
    CHECK(wld::fp6_shared_code(c2.data(), c2.size()) == 0, "{1, 0.5} taken");
}

uint64_t mask_part() {
    std::mt19937_64 rng(0x5A4Eull);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    uint64_t values = 0;
    // (N, NP): padding inside a lane, a whole lane, a whole 128-block
    const size_t shapes[][2] = {{1, 64}, {1, 128}, {31, 64}, {100, 128}, {127, 128}, {128, 128},
                                {129, 192}, {130, 256}, {200, 256}, {300, 320}};
    for (const auto &sh : shapes) {
        const size_t N = sh[0], NP = sh[1], NK = (NP + 127) / 128;
        for (int rep = 0; rep < 20; ++rep) {
            const double p_miss = rep % 4 == 3 ? 0.6 : 0.1;
            // the padded tail's symbols are 0 (missing), as the device's code rows hold them
            std::vector<uint8_t> sym(NP, kMiss), w2(NP, 0), w1(NP, 0);
            for (size_t k = 0; k < N; ++k) {
                sym[k] = u(rng) < p_miss ? kMiss : u(rng) < 0.3 ? kMinor : kMajor;
                w2[k] = 4;  // e2m1 2.0
                w1[k] = 2;  // e2m1 1.0
            }
            for (size_t kb = 0; kb < NK; ++kb)
                for (uint32_t g = 0; g < 4; ++g) {
                    const size_t k0 = 128 * kb + 32 * g;
                    const uint32_t n_pad = k0 < NP ? (uint32_t)std::min<size_t>(32, NP - k0) : 0u;
                    const uint32_t n_real = k0 < N ? (uint32_t)std::min<size_t>(32, N - k0) : 0u;
                    uint32_t sh_b[4], ai2[6], am2[6], ai1[6], am1[6], b4[4];
                    wld::f6_pack_lane_shared(sym.data() + (n_real ? k0 : 0), n_real, sh_b);
                    // the fp4 A image of the same symbols at weight 2.0 and at weight 1.0
                    wld::f6_pack_lane<true>(sym.data() + std::min(k0, NP), w2.data() + std::min(k0, NP), n_pad, ai2, am2, b4);
                    wld::f6_pack_lane<true>(sym.data() + std::min(k0, NP), w1.data() + std::min(k0, NP), n_pad, ai1, am1, b4);
                    for (int d = 0; d < 4; ++d) {
                        CHECK((sh_b[d] & wld::kF6MaskMissing) == ai2[d], "N %zu NP %zu k0 %zu dword %d: missing %08x / %08x", N,
                              NP, k0, d, sh_b[d] & wld::kF6MaskMissing, ai2[d]);
                        CHECK((sh_b[d] & wld::kF6MaskMinor) == am1[d], "N %zu NP %zu k0 %zu dword %d: minor %08x / %08x", N, NP,
                              k0, d, sh_b[d] & wld::kF6MaskMinor, am1[d]);
                        CHECK((sh_b[d] & ~(wld::kF6MaskMissing | wld::kF6MaskMinor)) == 0u, "stray bits %08x", sh_b[d]);
                    }
                    for (uint32_t j = 0; j < 32; ++j) {
                        const size_t k = k0 + j;
                        const uint32_t nb = wld::f6_lane_code4(sh_b, j), other = wld::f6_lane_code4(b4, j);
                        const uint32_t want = k < N ? (sym[k] == kMiss ? 4u : sym[k] == kMinor ? 2u : 0u) : 0u;
                        CHECK(nb == want, "N %zu k %zu: shared nibble %u, not %u", N, k, nb, want);
                        // the other formats' B image: the same inside N, missing in the padded tail
                        CHECK(other == (k < N ? want : k < NP ? 4u : 0u), "N %zu k %zu: B nibble %u", N, k, other);
                        ++values;
                    }
                }
        }
    }
    return values;
}

// One pair's restoration from both codings against the direct sums.  a, b: N
// symbols each; c: the e2m3 code every sequence carries.
void restore_case(const std::vector<uint8_t> &a, const std::vector<uint8_t> &b, uint32_t c, const char *what) {
    const size_t N = a.size();
    const double v = wld::fp6_value(c);
    // counts of (miss | minor of a) x (miss | minor of b), and the marginals
    double C00 = 0, C01 = 0, C10 = 0, C11 = 0, Ma = 0, ma = 0, Mb = 0, mb = 0;
    double X0 = 0, Y0 = 0, X1 = 0, Y1 = 0;  // the direct coding's sums, in f64 (exact)
    for (size_t k = 0; k < N; ++k) {
        const bool am_ = a[k] == kMiss, an = a[k] == kMinor, bm = b[k] == kMiss, bn = b[k] == kMinor;
        C00 += am_ && bm, C01 += am_ && bn, C10 += an && bm, C11 += an && bn;
        Ma += am_, ma += an, Mb += bm, mb += bn;
        const double in_a = am_ ? 0.0 : 1.0, bx = bn ? 1.0 : bm ? 0.0 : 2.0, by = bn ? 1.0 : 0.0;
        X0 += v * in_a * bx, Y0 += v * in_a * by, X1 += v * (an ? 1.0 : 0.0) * bx, Y1 += v * (an ? 1.0 : 0.0) * by;
    }
    const float W6 = (float)(v * (double)N), fMa = (float)(v * Ma), fma = (float)(v * ma), fMb = (float)(v * Mb),
                fmb = (float)(v * mb);
    const float row = wld::f6c_row_term(W6, fMa), col = wld::f6c_col_term(fMb, fmb), ma2 = 2.0f * fma;
    // the complement coding's accumulators (weights v) ...
    float px0 = (float)(v * (2 * C00 + C01)), py0 = (float)(v * C01), px1 = (float)(v * (2 * C10 + C11)),
          py1 = (float)(v * C11);
    wld::f6c_direct(px0, py0, px1, row, col, ma2, fmb);
    // ... and the shared image's (A weights 2.0 and 1.0: counts)
    float sx0 = (float)(2 * (2 * C00 + C01)), sy0 = (float)(2 * C01), sx1 = (float)(2 * C10 + C11), sy1 = (float)C11;
    wld::f6s_direct(sx0, sy0, sx1, sy1, row, col, ma2, fmb, (float)v, (float)(0.5 * v));
    CHECK(bits_of(sx0) == bits_of(px0) && bits_of(sy0) == bits_of(py0) && bits_of(sx1) == bits_of(px1) &&
              bits_of(sy1) == bits_of(py1),
          "%s code %u N %zu: shared %a %a %a %a, parent %a %a %a %a", what, c, N, sx0, sy0, sx1, sy1, px0, py0, px1, py1);
    CHECK((double)sx0 == X0 && (double)sy0 == Y0 && (double)sx1 == X1 && (double)sy1 == Y1,
          "%s code %u N %zu: shared %a %a %a %a, direct %a %a %a %a", what, c, N, sx0, sy0, sx1, sy1, X0, Y0, X1, Y1);
}

uint64_t restore_part() {
    uint64_t cases = 0;
    const uint8_t s3[3] = {kMiss, kMinor, kMajor};
    // exhaustive: every pair of symbol rows of 1 .. 6 sequences (9^N tables), every code
    for (size_t N = 1; N <= 6; ++N) {
        size_t tables = 1;
        for (size_t k = 0; k < N; ++k) tables *= 9;
        std::vector<uint8_t> a(N), b(N);
        for (size_t t = 0; t < tables; ++t) {
            size_t x = t;
            for (size_t k = 0; k < N; ++k, x /= 9) a[k] = s3[x % 3], b[k] = s3[x / 3 % 3];
            // (N <= 4: every code; longer: the codes of 0.125, 1.0, 1.375, 4.0, 7.5)
            if (N <= 4)
                for (uint32_t c = 1; c < 32; ++c) restore_case(a, b, c, "exhaustive"), ++cases;
            else
                for (uint32_t c : {1u, 8u, 11u, 24u, 31u}) restore_case(a, b, c, "exhaustive"), ++cases;
        }
    }
    std::mt19937_64 rng(0x5EA2ull);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (size_t N : {(size_t)7, (size_t)100, (size_t)128, (size_t)129, (size_t)200, (size_t)1000, (size_t)2000, (size_t)2048})
        for (int rep = 0; rep < 24; ++rep) {
            // (rep 0-2: one symbol everywhere, the sums' extremes)
            const double pm = rep % 4 == 3 ? 0.6 : 0.1;
            std::vector<uint8_t> a(N), b(N);
            for (size_t k = 0; k < N; ++k) {
                a[k] = rep < 3 ? s3[rep] : u(rng) < pm ? kMiss : u(rng) < 0.3 ? kMinor : kMajor;
                b[k] = rep < 3 ? s3[rep] : u(rng) < 0.5 ? a[k] : u(rng) < pm ? kMiss : u(rng) < 0.3 ? kMinor : kMajor;
            }
            for (uint32_t c = 1; c < 32; ++c) restore_case(a, b, c, "random"), ++cases;
        }
    return cases;
}
}  // namespace

int main() {
    qualify_part();
    const uint64_t values = mask_part();
    std::printf("masking: %" PRIu64 " nibbles against the fp4 A image\n", values);
    const uint64_t cases = restore_part();
    std::printf("restoration: %" PRIu64 " (table, code) cases\n", cases);
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
