// Host check of the fp6 screen's complement coding and of its weight-code
// scale rule (no device code runs; tests/test_f6_complement.py builds this
// plain and under AddressSanitizer + UndefinedBehaviorSanitizer).
//
// Part 1 (pair_common.hpp f6c_row_term / f6c_col_term / f6c_direct): for
// seeded random site pairs it sums, in f32 as the MFMAs do, the direct
// coding's accumulators (A: w6 [in], w6 [minor]; B: minor + 2 major, minor)
// and the complement coding's (A: w6 [missing], w6 [minor]; B: 2 missing +
// minor, minor), the latter over the padded tail too (sequences N <= k < NP:
// code 0, which reads as missing, and weight code 0), forms the per-site
// marginals as fp6_marginals_kernel does (integers, 8 x the value, converted
// once), and asserts that the restored X0, Y0, X1, Y1 equal the direct ones
// bit for bit, and that r2_screen_terms_xy2 returns bit-identical t1 and mlo.
//
// Part 2 (fp6_scale.hpp fp6_choose_scale): the chosen scale's residual is
// within 1% of the smallest over all candidates (recomputed here) and no
// candidate inside that condition has fewer set mantissa bits; unit weights
// and a narrow Henikoff-like set get one code with an all-zero mantissa (unit
// weights with residual 0); a set spread over 2^4 keeps the minimum-residual
// scale unless another candidate lies inside the 1% condition with fewer
// bits, and never exceeds the condition.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

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
// 8 x the value of an e2m3 code (as fp6_marginals_kernel decodes it)
uint32_t value8(uint32_t q) {
    const uint32_t e = q >> 3;
    return e ? (8u + (q & 7u)) << (e - 1) : q;
}
enum : uint8_t { kMiss = 0, kMinor = 1, kMajor = 3 };  // kernels.hpp: kCodeIn = 1, kCodeMaj = 2

// one site's symbols over NP sequences (the tail past N is code 0)
std::vector<uint8_t> site(std::mt19937_64 &rng, size_t N, size_t NP, double p_miss, bool no_minor) {
    std::vector<uint8_t> s(NP, kMiss);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    const double p_minor = no_minor ? 0.0 : 0.05 + 0.45 * u(rng);
    for (size_t k = 0; k < N; ++k) s[k] = u(rng) < p_miss ? kMiss : (u(rng) < p_minor ? kMinor : kMajor);
    return s;
}

uint64_t complement_part() {
    std::mt19937_64 rng(0xF6C0DEull);
    uint64_t pairs = 0;
    for (size_t N : {(size_t)1, (size_t)127, (size_t)128, (size_t)130, (size_t)16384}) {
        const size_t NP = (N + 127) / 128 * 128;
        for (double p_miss : {0.0, 0.1, 0.9, 1.0}) {
            const int reps = N > 1000 ? 60 : 600;
            for (int rep = 0; rep < reps; ++rep) {
                // arbitrary e2m3 codes, 0 and 7.5 (code 31) among them; rep 0: all 7.5, the largest sums
                std::vector<uint8_t> q(NP, 0);
                for (size_t k = 0; k < N; ++k) q[k] = rep == 0 ? 31u : (uint8_t)(rng() % 32);
                if (N > 2 && rep) q[0] = 0, q[1] = 31;
                const bool a_flat = rep % 7 == 3, b_flat = rep % 5 == 2;  // sites with no minor
                const std::vector<uint8_t> a = site(rng, N, NP, p_miss, a_flat),
                                           b = site(rng, N, NP, rep % 3 == 1 ? 0.0 : p_miss, b_flat);
                float X0 = 0, Y0 = 0, X1 = 0, Y1 = 0, aX = 0, aY = 0, bX = 0, bY = 0;
                uint32_t W8 = 0, Ma8 = 0, ma8 = 0, Mb8 = 0, mb8 = 0;
                for (size_t k = 0; k < NP; ++k) {
                    const float w = 0.125f * (float)value8(q[k]);
                    const bool a_in = a[k] & 1, a_min = a[k] == kMinor, b_in = b[k] & 1, b_min = b[k] == kMinor;
                    // direct: B raw = minor + 2 major, masked = minor (real sequences only: the parent's padded
                    // sequences are not "in")
                    const float braw = b_in ? (b_min ? 1.0f : 2.0f) : 0.0f, bmin = b_min ? 1.0f : 0.0f;
                    X0 += (a_in ? w : 0.0f) * braw;
                    Y0 += (a_in ? w : 0.0f) * bmin;
                    X1 += (a_min ? w : 0.0f) * braw;
                    Y1 += (a_min ? w : 0.0f) * bmin;
                    // complement: B raw = 2 missing + minor, masked = minor
                    const float craw = b_in ? (b_min ? 1.0f : 0.0f) : 2.0f;
                    aX += (a_in ? 0.0f : w) * craw;
                    aY += (a_in ? 0.0f : w) * bmin;
                    bX += (a_min ? w : 0.0f) * craw;
                    bY += (a_min ? w : 0.0f) * bmin;
                    W8 += value8(q[k]);
                    Ma8 += a_in ? 0u : value8(q[k]);
                    ma8 += a_min ? value8(q[k]) : 0u;
                    Mb8 += b_in ? 0u : value8(q[k]);
                    mb8 += b_min ? value8(q[k]) : 0u;
                }
                const float W6 = 0.125f * (float)W8, Ma = 0.125f * (float)Ma8, ma = 0.125f * (float)ma8,
                            Mb = 0.125f * (float)Mb8, mb = 0.125f * (float)mb8;
                float x0 = aX, y0 = aY, x1 = bX;
                const float y1 = bY;
                wld::f6c_direct(x0, y0, x1, wld::f6c_row_term(W6, Ma), wld::f6c_col_term(Mb, mb), 2.0f * ma, mb);
                CHECK(bits_of(x0) == bits_of(X0) && bits_of(y0) == bits_of(Y0) && bits_of(x1) == bits_of(X1) &&
                          bits_of(y1) == bits_of(Y1),
                      "N %zu miss %.1f rep %d: X0 %a/%a Y0 %a/%a X1 %a/%a Y1 %a/%a", N, p_miss, rep, x0, X0, y0, Y0,
                      x1, X1, y1, Y1);
                // the screen's test on both, with a launch's constants (R on the 1/32 grid, doubled)
                const float Rf = std::ceil((0.01f * W6 + 0.3f) * 32.0f) / 32.0f, R2 = 2.0f * Rf;
                float E, mloc, mlo_d, mlo_c;
                wld::screen_consts(2.0f * W6, R2, E, mloc);
                for (float thr : {0.5f, 0.05f}) {
                    const float thr_c = thr * (1.0f - 0x1p-7f);
                    const float t_d = wld::r2_screen_terms_xy2(X0, Y0, X1, Y1, R2, thr_c, E, mlo_d);
                    const float t_c = wld::r2_screen_terms_xy2(x0, y0, x1, y1, R2, thr_c, E, mlo_c);
                    CHECK(bits_of(t_d) == bits_of(t_c) && bits_of(mlo_d) == bits_of(mlo_c),
                          "N %zu miss %.1f rep %d thr %g: t1 %a/%a mlo %a/%a", N, p_miss, rep, thr, t_c, t_d, mlo_c,
                          mlo_d);
                }
                ++pairs;
            }
        }
    }
    return pairs;
}

// fp6_choose_scale against the rule recomputed here over the same candidates
void scale_case(const char *name, const std::vector<float> &w, bool one_zero_mantissa_code, bool zero_resid,
                bool spread) {
    double wmax = 0.0;
    for (float x : w) wmax = std::max(wmax, (double)x);
    const wld::Fp6ScaleCost got = wld::fp6_choose_scale(w.data(), w.size(), wmax);
    const std::vector<double> cand = wld::fp6_scale_candidates(w.data(), w.size(), wmax);
    CHECK(cand.size() >= 51, "%s: %zu candidates", name, cand.size());
    double rmin = INFINITY, smin = 0.0;
    std::vector<double> res;
    std::vector<uint64_t> mb;
    for (double S : cand) {
        double r = 0.0, v;
        uint64_t bits = 0;
        for (float x : w) {
            const uint32_t c = wld::fp6_code(S * (double)x, &v);
            r += std::fabs(S * (double)x - v);
            bits += (uint64_t)__builtin_popcount(c & 7u);
        }
        res.push_back(r / S);
        mb.push_back(bits);
        if (r / S < rmin) rmin = r / S, smin = S;
    }
    bool listed = false;
    size_t inside = 0;
    uint64_t bits_min_resid = 0;
    for (size_t i = 0; i < cand.size(); ++i) {
        if (cand[i] == got.S) {
            listed = true;
            CHECK(res[i] == got.resid && mb[i] == got.mant_bits, "%s: cost of S %.17g", name, got.S);
        }
        if (cand[i] == smin) bits_min_resid = mb[i];
        if (res[i] <= 1.01 * rmin) {
            ++inside;
            CHECK(mb[i] >= got.mant_bits, "%s: S %.17g inside the condition with %" PRIu64 " < %" PRIu64 " bits",
                  name, cand[i], mb[i], got.mant_bits);
        }
    }
    CHECK(listed, "%s: S %.17g is no candidate", name, got.S);
    CHECK(got.resid <= 1.01 * rmin, "%s: residual %.17g outside 1%% of %.17g", name, got.resid, rmin);
    if (spread) {
        // the minimum-residual scale unless the condition admits a quieter one
        CHECK(got.mant_bits <= bits_min_resid, "%s: more bits than the minimum-residual scale", name);
        if (inside == 1 || got.mant_bits == bits_min_resid) CHECK(got.resid == rmin, "%s: not the minimum", name);
    }
    double v;
    const uint32_t c0 = wld::fp6_code(got.S * (double)w[0], &v);
    if (one_zero_mantissa_code) {
        for (float x : w) CHECK(wld::fp6_code(got.S * (double)x, &v) == c0, "%s: more than one code", name);
        CHECK((c0 & 7u) == 0 && c0 != 0, "%s: code %u", name, c0);
        CHECK(got.mant_bits == 0, "%s: %" PRIu64 " mantissa bits", name, got.mant_bits);
    }
    if (zero_resid) CHECK(got.resid == 0.0, "%s: residual %.17g", name, got.resid);
    std::printf("scale %-10s N %6zu: S %.6f code(w[0]) %2u value %.3f resid %.6g (min %.6g at S %.6f) bits %" PRIu64
                " inside %zu\n",
                name, w.size(), got.S, c0, v, got.resid, rmin, smin, got.mant_bits, inside);
}

void scale_part() {
    std::mt19937_64 rng(0x5CA1Eull);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (size_t N : {(size_t)1, (size_t)130, (size_t)2000}) {
        std::vector<float> unit(N, 1.0f), narrow(N), spread(N), wide(N);
        for (size_t k = 0; k < N; ++k) {
            narrow[k] = (float)(5e-4 * (0.965 + 0.035 * u(rng)));  // Henikoff weights of a large alignment
            spread[k] = (float)std::exp2(-4.0 * u(rng));
            wide[k] = (float)(u(rng) * u(rng));
        }
        scale_case("unit", unit, true, true, false);
        scale_case("narrow", narrow, true, N == 1, false);
        scale_case("spread", spread, false, false, true);
        scale_case("wide", wide, false, false, false);
    }
}
}  // namespace

int main() {
    const uint64_t pairs = complement_part();
    std::printf("complement coding: %" PRIu64 " site pairs\n", pairs);
    scale_part();
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
