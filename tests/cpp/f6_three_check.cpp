// Host check of the fp6 screen's three-sum test (pair_common.hpp
// r2_screen_terms_xy2_t, f6_cap2; no device code runs; tests/test_f6_three.py
// builds this plain and under AddressSanitizer + UndefinedBehaviorSanitizer).
//
// The property: wherever the three-sum test skips a pair (t1 <= 0 and mlo >=
// mloc, from the sums without the missing-by-missing one), the four-sum test
// r2_screen_terms_xy2 on the true sums, in f32, skips it too.  Also checked:
// the cap brackets the true sum (0 <= 2 P00 <= cap2, exact), the three-sum
// mlo never exceeds the four-sum one, and with cap 0 both tests agree bit for
// bit.  r2_screen_terms_f6t, the form the kernel evaluates (from the three sums
// and per-site terms, without restoring), gives r2_screen_terms_xy2_t's t1 and
// mlo bit for bit on every test.
//
// Part 1: more than 10^7 tables of the nine weight sums of (missing, minor,
// major of a) x (the same of b), on the 1/8 grid, random and adversarial:
// empty cells (cap 0: nothing missing in a or in b beside the other's minor;
// cap maximal: every sequence missing in a is missing in b), P00 at 0 and at
// the cap, marginals near mloc, totals from 1/8 to 2^17, residuals R from 0
// to a third of the total, and for every table thresholds at the boundary:
// the f32 numbers around the critical threshold of the four-sum test and of
// the three-sum one, where t1 changes sign.  Through f6c_direct (fp4 and fp6
// A images) and, for every e2m3 code, through f6s_direct from the shared
// image's counts.
// Part 2: 512 sites x 2,000 sequences of bench.synth's distribution (missing
// 0.1, major 0.6, minor 0.3; every weight on the code of 4.0), R = 37.53 and
// thr = 0.05 as C4 has them, E and mloc by screen_consts: the implication on
// every pair, and at most 1 pair in 10^4 left in doubt (the same distribution
// gave 5.6e-8 over 1.8e7 pairs).
#include <algorithm>
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

// The restored sums of one pair, with and without the fourth sum.
struct Sums {
    float X0, X0lo, Y0, X1, Y1, cap2;
    // the three sums as the kernel holds them (weights; the shared image's counts scaled), and the sites' marginals
    float p, s, t, W6, Ma, ma, Mb, mb;
};
// c[i][j]: the weight sum of the sequences where a is (missing, minor, major)[i]
// and b is [j], in eighths (integers).  v8 = 0: the weights are in the cells
// (f6c_direct); else the cells are counts and every weight is v8 / 8 (f6s_direct).
Sums restore(const uint64_t (&c)[3][3], uint32_t v8) {
    const double u = v8 ? (double)v8 / 8.0 : 0.125;  // one cell unit in weight
    double Ma = 0, ma = 0, Mb = 0, mb = 0, W = 0;
    for (int j = 0; j < 3; ++j) Ma += (double)c[0][j], ma += (double)c[1][j], Mb += (double)c[j][0], mb += (double)c[j][1];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W += (double)c[i][j];
    const float W6 = (float)(u * W), fMa = (float)(u * Ma), fma = (float)(u * ma), fMb = (float)(u * Mb),
                fmb = (float)(u * mb);
    const float row = wld::f6c_row_term(W6, fMa), col = wld::f6c_col_term(fMb, fmb), ma2 = 2.0f * fma;
    const double P00 = (double)c[0][0], P01 = (double)c[0][1], P10 = (double)c[1][0], P11 = (double)c[1][1];
    Sums s;
    float x0, y0, x1, y1, t0, ty0, tx1, ty1;
    if (v8) {  // the shared image's counts: 2 (2 C00 + C01), 2 C01, 2 C10 + C11, C11
        const float v = (float)u, hv = 0.5f * v;
        x0 = (float)(2 * (2 * P00 + P01)), y0 = (float)(2 * P01), x1 = (float)(2 * P10 + P11), y1 = (float)P11;
        t0 = y0, ty0 = y0, tx1 = x1, ty1 = y1;  // three sums: aX's count stands in as aY's
        wld::f6s_direct(x0, y0, x1, y1, row, col, ma2, fmb, v, hv);
        wld::f6s_direct(t0, ty0, tx1, ty1, row, col, ma2, fmb, v, hv);
    } else {
        x0 = (float)(u * (2 * P00 + P01)), y0 = (float)(u * P01), x1 = (float)(u * (2 * P10 + P11)), y1 = (float)(u * P11);
        t0 = y0, ty0 = y0, tx1 = x1, ty1 = y1;
        wld::f6c_direct(x0, y0, x1, row, col, ma2, fmb);
        wld::f6c_direct(t0, ty0, tx1, row, col, ma2, fmb);
    }
    CHECK(bits_of(y0) == bits_of(ty0) && bits_of(x1) == bits_of(tx1) && bits_of(y1) == bits_of(ty1), "Y0, X1, Y1 moved");
    s.X0 = x0, s.X0lo = t0, s.Y0 = y0, s.X1 = x1, s.Y1 = y1;
    s.p = (float)(u * P01), s.s = (float)(u * (2 * P10 + P11)), s.t = (float)(u * P11);
    s.W6 = W6, s.Ma = fMa, s.ma = fma, s.Mb = fMb, s.mb = fmb;
    s.cap2 = wld::f6_cap2(2.0f * fMa, ma2, 2.0f * fMb, 2.0f * fmb, y0, x1, y1);
    // exact: X0 = X0lo + 2 P00, and the cap is 2 min(M_a - P01, M_b - P10) >= 2 P00
    CHECK((double)s.X0 == (double)s.X0lo + 2.0 * u * P00, "X0 %a is not X0lo %a + 2 P00 %a", s.X0, s.X0lo, 2.0 * u * P00);
    CHECK((double)s.cap2 == 2.0 * u * std::min(Ma - P01, Mb - P10), "cap2 %a, not %a", s.cap2, 2.0 * u * std::min(Ma - P01, Mb - P10));
    CHECK((double)s.cap2 >= 2.0 * u * P00, "cap2 %a below 2 P00 %a", s.cap2, 2.0 * u * P00);
    return s;
}

struct Tally {
    uint64_t tests = 0, skip3 = 0, skip4 = 0;
};
// One (table, R2, E, mloc, thr_c): the implication.
void implication(const Sums &s, float R2, float thr_c, float E, float mloc, Tally &t, const char *what) {
    float mlo3, mlo4;
    const float t3 = wld::r2_screen_terms_xy2_t(s.X0lo, s.Y0, s.X1, s.Y1, s.cap2, R2, thr_c, E, mlo3);
    const float t4 = wld::r2_screen_terms_xy2(s.X0, s.Y0, s.X1, s.Y1, R2, thr_c, E, mlo4);
    const bool k3 = t3 <= 0.0f && mlo3 >= mloc, k4 = t4 <= 0.0f && mlo4 >= mloc;
    ++t.tests, t.skip3 += k3, t.skip4 += k4;
    CHECK(!k3 || k4, "%s: three sums skip (t1 %a mlo %a), four do not (t1 %a mlo %a, mloc %a): X0lo %a cap2 %a X0 %a Y0 %a X1 %a Y1 %a R2 %a thr_c %a",
          what, t3, mlo3, t4, mlo4, mloc, s.X0lo, s.cap2, s.X0, s.Y0, s.X1, s.Y1, R2, thr_c);
    CHECK(mlo3 <= mlo4, "%s: mlo %a above the four-sum mlo %a", what, mlo3, mlo4);
    // the kernel's form, from the three sums and the per-site terms: the same bits
    float mloK;
    const float tK = wld::r2_screen_terms_f6t(s.p, s.s, s.t, wld::f6t_row(s.W6, s.Ma, s.ma, R2), wld::f6t_col(s.Mb, s.mb, R2),
                                              thr_c, E, mloK);
    CHECK(bits_of(tK) == bits_of(t3) && bits_of(mloK) == bits_of(mlo3), "%s: per-site form t1 %a mlo %a, restored form %a %a", what,
          tK, mloK, t3, mlo3);
    if (s.cap2 == 0.0f) CHECK(bits_of(t3) == bits_of(t4) && bits_of(mlo3) == bits_of(mlo4), "%s: cap 0, t1 %a / %a", what, t3, t4);
}

// The f32 thresholds around the one at which t1 of the given sums changes sign.
void critical(float X0, const Sums &s, float cap2, float R2, float E, float (&out)[3]) {
    float mlo;
    // t1 = nub^2 - thr_c P: with thr_c = 0 it is nub^2, with thr_c = 1 nub^2 - P
    const double n2 = (double)wld::r2_screen_terms_xy2_t(X0, s.Y0, s.X1, s.Y1, cap2, R2, 0.0f, E, mlo);
    const double P = n2 - (double)wld::r2_screen_terms_xy2_t(X0, s.Y0, s.X1, s.Y1, cap2, R2, 1.0f, E, mlo);
    float c = P > 0.0 ? (float)(n2 / P) : 0.5f;
    if (!(c > 0.0f) || !std::isfinite(c)) c = 0.5f;
    out[0] = std::nextafterf(c, 0.0f), out[1] = c, out[2] = std::nextafterf(c, INFINITY);
}

uint64_t tables_part(Tally &t) {
    std::mt19937_64 rng(0x7E3ull);
    auto below = [&](uint64_t n) { return n ? rng() % n : 0; };
    uint64_t tables = 0;
    const uint64_t kTables = 10000000;  // each at 3 fixed and 2 x 3 boundary thresholds
    for (uint64_t it = 0; it < kTables; ++it) {
        // every 8th table through the shared route, its code cycling through all e2m3 codes
        const uint32_t code = it % 8 == 7 ? 1 + (uint32_t)(it / 8 % 31) : 0;
        const uint32_t v8 = code ? (uint32_t)std::lround(8.0 * wld::fp6_value(code)) : 0;
        // total in cell units: weights up to 2^17 (2^20 eighths), counts up to 16384
        const uint64_t cap_total = v8 ? 16384 : (1ull << 20);
        const int mag = (int)below(4);
        const uint64_t total = mag == 0 ? 1 + below(64) : mag == 1 ? 1 + below(4096) : mag == 2 ? 1 + below(cap_total) : cap_total - below(16);
        uint64_t c[3][3] = {};
        // proportions: synth-like, uniform, or skewed to one cell
        double p[9];
        const int shape = (int)below(3);
        double sum = 0;
        for (int k = 0; k < 9; ++k) {
            const double x = (double)(rng() >> 11) * 0x1p-53;
            const double sy[3] = {0.1, 0.3, 0.6};
            p[k] = shape == 0 ? sy[k / 3] * sy[k % 3] * (0.5 + x) : shape == 1 ? x : x * x * x * x;
            sum += p[k];
        }
        // adversarial structure: empty cells
        const int adv = (int)below(12);
        auto zero = [&](int i, int j) { sum -= p[3 * i + j], p[3 * i + j] = 0; };
        if (adv == 0) zero(0, 0), zero(0, 2);             // cap 0 by M_a = P01
        if (adv == 1) zero(0, 0), zero(2, 0);             // cap 0 by M_b = P10
        if (adv == 2) zero(0, 1), zero(0, 2);             // P00 at the cap: M_a = P00
        if (adv == 3) zero(1, 0), zero(2, 0);             // P00 at the cap: M_b = P00
        if (adv == 4) zero(0, 0);                         // P00 = 0, cap open
        if (adv == 5) zero(1, 0), zero(1, 1);             // a's minor marginal small (only x major)
        if (adv == 6) zero(0, 1), zero(1, 1), zero(2, 1); // m_b = 0
        if (adv == 7) zero(1, 0), zero(1, 1), zero(1, 2); // m_a = 0
        if (adv == 8) zero(1, 1);                         // Y1 = 0: the numerator does not see X0
        uint64_t left = total;
        for (int k = 0; k < 9 && sum > 0; ++k) {
            const uint64_t x = std::min<uint64_t>(left, (uint64_t)((double)total * p[k] / sum));
            c[k / 3][k % 3] = x;
            left -= x;
        }
        if (adv >= 9) {  // a marginal near mloc: one or two units in a minor cell
            c[1][0] = below(2), c[1][1] = below(3), c[1][2] = below(3);
        }
        const Sums s = restore(c, v8);
        ++tables;
        // R: none, the rounding residual's size, large; on the 1/32 grid as fp6_screen_args puts it
        const double unit = v8 ? (double)v8 / 8.0 : 0.125, Wt = unit * (double)total;
        const int rk = (int)below(4);
        const double R = rk == 0 ? 0.0 : rk == 1 ? Wt * 0.002 * (double)below(16) : rk == 2 ? Wt / 3.0 : (double)below(8) / 32.0;
        const float Rf = (float)(std::ceil(R * 32.0) / 32.0), R2 = 2.0f * Rf;
        float E, mloc;
        // Tg bounds every doubled T: 2 W6, or a load's larger bound
        wld::screen_consts((float)(2.0 * Wt * (below(2) ? 1.0 : 1.5)), R2, E, mloc);
        const float fixed[3] = {0.05f * (1.0f - 0x1p-7f), 0.5f * (1.0f - 0x1p-7f), (float)((double)(rng() >> 11) * 0x1p-53)};
        for (float thr_c : fixed) implication(s, R2, thr_c, E, mloc, t, code ? "shared" : "table");
        float crit[3];
        critical(s.X0, s, 0.0f, R2, E, crit);  // the four-sum test's boundary
        for (float thr_c : crit) implication(s, R2, thr_c, E, mloc, t, code ? "shared, four-sum boundary" : "four-sum boundary");
        critical(s.X0lo, s, s.cap2, R2, E, crit);  // the three-sum test's
        for (float thr_c : crit) implication(s, R2, thr_c, E, mloc, t, code ? "shared, three-sum boundary" : "three-sum boundary");
    }
    return tables;
}

// Part 2: the synth-like sample.
void synth_part() {
    const size_t L = 512, N = 2000, NW = (N + 63) / 64;
    std::mt19937_64 rng(0x5EEDull);
    std::vector<uint64_t> miss(L * NW, 0), minor(L * NW, 0);
    for (size_t s = 0; s < L; ++s)
        for (size_t k = 0; k < N; ++k) {
            const double x = (double)(rng() >> 11) * 0x1p-53;
            if (x < 0.1)
                miss[s * NW + k / 64] |= 1ull << (k % 64);
            else if (x >= 0.7)
                minor[s * NW + k / 64] |= 1ull << (k % 64);
        }
    const uint32_t v8 = 32;  // every weight on the code of 4.0
    const float Rf = (float)(std::ceil(37.53 * 32.0) / 32.0), R2 = 2.0f * Rf, thr_c = 0.05f * (1.0f - 0x1p-7f);
    float E, mloc;
    wld::screen_consts((float)(2.0 * 4.0 * (double)N), R2, E, mloc);
    Tally t;
    uint64_t doubt = 0, pairs = 0;
    for (size_t a = 0; a < L; ++a)
        for (size_t b = a + 1; b < L; ++b) {
            uint64_t n[2][2] = {}, Ma = 0, ma = 0, Mb = 0, mb = 0;
            for (size_t w = 0; w < NW; ++w) {
                const uint64_t am = miss[a * NW + w], an = minor[a * NW + w], bm = miss[b * NW + w], bn = minor[b * NW + w];
                n[0][0] += (uint64_t)__builtin_popcountll(am & bm), n[0][1] += (uint64_t)__builtin_popcountll(am & bn);
                n[1][0] += (uint64_t)__builtin_popcountll(an & bm), n[1][1] += (uint64_t)__builtin_popcountll(an & bn);
                Ma += (uint64_t)__builtin_popcountll(am), ma += (uint64_t)__builtin_popcountll(an);
                Mb += (uint64_t)__builtin_popcountll(bm), mb += (uint64_t)__builtin_popcountll(bn);
            }
            uint64_t c[3][3];
            c[0][0] = n[0][0], c[0][1] = n[0][1], c[0][2] = Ma - n[0][0] - n[0][1];
            c[1][0] = n[1][0], c[1][1] = n[1][1], c[1][2] = ma - n[1][0] - n[1][1];
            c[2][0] = Mb - n[0][0] - n[1][0], c[2][1] = mb - n[0][1] - n[1][1];
            c[2][2] = N - Ma - ma - c[2][0] - c[2][1];
            const Sums s = restore(c, v8);
            const uint64_t before = t.skip3;
            implication(s, R2, thr_c, E, mloc, t, "synth");
            doubt += t.skip3 == before;
            ++pairs;
        }
    std::printf("synth sample: %" PRIu64 " pairs, %" PRIu64 " in doubt on three sums, %" PRIu64 " not skipped on four\n", pairs,
                doubt, pairs - t.skip4);
    CHECK(doubt * 10000 <= pairs, "%" PRIu64 " of %" PRIu64 " pairs in doubt: more than 1 in 10^4", doubt, pairs);
}
}  // namespace

int main() {
    Tally t;
    const uint64_t tables = tables_part(t);
    std::printf("tables: %" PRIu64 ", tests %" PRIu64 ": skipped on three sums %" PRIu64 ", on four %" PRIu64 "\n", tables, t.tests,
                t.skip3, t.skip4);
    CHECK(tables * 1 >= 1 && t.tests >= 10000000ull, "only %" PRIu64 " tests", t.tests);
    // the check has teeth only if both outcomes occur in number
    CHECK(t.skip3 * 20 >= t.tests && (t.tests - t.skip4) * 20 >= t.tests && t.skip4 > t.skip3, "outcomes %" PRIu64 " / %" PRIu64 " of %" PRIu64,
          t.skip3, t.skip4, t.tests);
    synth_part();
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
