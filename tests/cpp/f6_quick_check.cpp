// Host check of the fp6 screen's quick test (pair_common.hpp f6q_pair,
// f6q_lane_terms, f6q_skip: WLD_OPT_FP6_QUICK; no device code runs;
// tests/test_f6_quick.py builds this plain and under AddressSanitizer +
// UndefinedBehaviorSanitizer).
//
// The property: wherever the quick test skips a lane's 16 pairs of a row block
// (4 row sites by 4 column sites) together, r2_screen_terms_f6t, in f32 as
// written, skips every one of them (t1 <= 0 and mlo >= mloc).  Also checked:
// each pair's nt from f6q_pair is the full test's, bit for bit (the full
// test's numerator is re-formed here by its own expressions, and that copy is
// tied to r2_screen_terms_f6t by reproducing its t1 and mlo bits); the lane's
// mlo' never exceeds a pair's mlo; and where the primed marginals are
// nonnegative, t1' is at least every pair's t1.
//
// Part 1: lanes built from real small alignments, so that a site's marginals
// are shared by its pairs as in the kernel: 4 row and 4 column sites over 1 to
// 512 sequences, weights on the 1/8 grid up to 7.5 or, for every e2m3 code,
// all on that code through the shared image's counts.  Adversarial columns: no
// missing, all missing, no minor, one minor, a copy of a row site.  R and Tg
// varied as in f6_three_check.cpp.  Per lane: thresholds 0.05 and 0.5, a
// random one, the f32 neighbours of the threshold at which t1' changes sign,
// and those of the threshold at which the worst pair's t1 does.
// Part 2: 2,048 sites x 2,000 sequences of bench.synth's distribution (missing
// 0.1, major 0.6, minor 0.3; every weight on the code of 4.0), R = 37.53 and
// thr = 0.05 as C4 has them: the implication on every lane of every
// off-diagonal tile, and at most 1/10 of the 1,984 row blocks (16 sites x a
// 64-site tile, 64 lanes) falling through to the full test.
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

// One lane's view of a row block: the sites' marginals and the 16 pairs' sums
// as the kernel holds them (weights; the shared image's counts scaled).
struct Lane {
    float W6;
    float Ma[4], ma[4], Mb[4], mb[4];
    float p[4][4], s[4][4], t[4][4];  // [e][n]
};

// The full test's numerator maximum and marginal product by its own
// expressions (r2_screen_terms_f6t, pair_common.hpp), for the nt comparison.
struct FullParts {
    float nt, prod, mlo;
};
FullParts full_parts(float p, float s, float t, const wld::F6tRow &a, const wld::F6tCol &b) {
    const float d = s - t;
    const float m1 = a.c1 - d, m2 = (a.rA2 + b.cB2) + d;
    const float m3 = fmaf(2.0f, p, a.rA + b.cB3), m4 = fmaf(-2.0f, p, b.c4);
    const float cap2 = fminf(fmaf(-2.0f, p, a.Ma2), b.Mb2 - d);
    const float q = -((a.ma2 - s) * (b.mb - p));
    const float X0lo = p + (a.row + b.col);
    FullParts r;
    r.nt = fmaxf(fabsf(fmaf(X0lo, t, q)), fabsf(fmaf(X0lo + cap2, t, q)));
    r.prod = (m1 * m2) * (m3 * m4);
    r.mlo = fminf(fminf(m1, m2), fminf(m3, m4));
    return r;
}

struct Tally {
    uint64_t tests = 0, quick = 0, full_all = 0;
};

struct LaneTerms {
    wld::F6tRow ra[4];
    wld::F6tCol cb[4];
    wld::F6qAcc acc;
    wld::F6qRowMin rm;
    wld::F6qColMin cm;
};
// The threshold-free part of a lane: the sites' terms, the maxima, the nt bits.
LaneTerms lane_terms(const Lane &L, float R2, const char *what) {
    LaneTerms z;
    z.rm = wld::F6qRowMin{INFINITY, INFINITY, INFINITY};
    for (int n = 0; n < 4; ++n) z.cb[n] = wld::f6t_col(L.Mb[n], L.mb[n], R2);
    z.cm = wld::f6q_col_min(z.cb);
    for (int e = 0; e < 4; ++e) {
        z.ra[e] = wld::f6t_row(L.W6, L.Ma[e], L.ma[e], R2);
        wld::f6q_row_min(z.rm, z.ra[e]);
        for (int n = 0; n < 4; ++n) {
            CHECK(L.s[e][n] - L.t[e][n] >= 0.0f && L.p[e][n] >= 0.0f, "%s: d or p negative", what);
            const float nt = wld::f6q_pair(L.p[e][n], L.s[e][n], L.t[e][n], z.ra[e], z.cb[n], z.acc);
            const FullParts f = full_parts(L.p[e][n], L.s[e][n], L.t[e][n], z.ra[e], z.cb[n]);
            CHECK(bits_of(nt) == bits_of(f.nt), "%s: pair (%d, %d) nt %a, the full test's %a", what, e, n, nt, f.nt);
        }
    }
    return z;
}

// One (lane, thr_c): the implication.  Returns whether the quick test skipped.
bool implication(const Lane &L, const LaneTerms &z, float thr_c, float E, float mloc, Tally &ty, const char *what) {
    float mloq;
    const float tq = wld::f6q_lane_terms(z.acc, z.rm, z.cm, thr_c, E, mloq);
    const bool kq = wld::f6q_skip(tq, mloq, mloc);
    bool all = true;
    for (int e = 0; e < 4; ++e)
        for (int n = 0; n < 4; ++n) {
            float mlo;
            const float t1 = wld::r2_screen_terms_f6t(L.p[e][n], L.s[e][n], L.t[e][n], z.ra[e], z.cb[n], thr_c, E, mlo);
            const bool k = t1 <= 0.0f && mlo >= mloc;
            all = all && k;
            CHECK(!kq || k, "%s: the quick test skips (t1' %a mlo' %a mloc %a), pair (%d, %d) does not (t1 %a mlo %a): p %a s %a t %a thr_c %a E %a",
                  what, tq, mloq, mloc, e, n, t1, mlo, L.p[e][n], L.s[e][n], L.t[e][n], thr_c, E);
            CHECK(mloq <= mlo, "%s: mlo' %a above pair (%d, %d)'s mlo %a", what, mloq, e, n, mlo);
            if (mloq >= 0.0f) CHECK(tq >= t1, "%s: t1' %a below pair (%d, %d)'s t1 %a", what, tq, e, n, t1);
            // the copy of the full test's expressions is the full test
            const FullParts f = full_parts(L.p[e][n], L.s[e][n], L.t[e][n], z.ra[e], z.cb[n]);
            const float nub = fmaf(2.0f, f.nt, E);
            CHECK(bits_of(fmaf(nub, nub, -(thr_c * f.prod))) == bits_of(t1) && bits_of(f.mlo) == bits_of(mlo),
                  "%s: the full test's parts do not give its t1 %a", what, t1);
        }
    ++ty.tests, ty.quick += kq, ty.full_all += all;
    return kq;
}

// The f32 thresholds around n2 / P, where a t1 = n2 - thr_c P changes sign.
void around(double n2, double P, float (&out)[3]) {
    float c = P > 0.0 ? (float)(n2 / P) : 0.5f;
    if (!(c > 0.0f) || !std::isfinite(c)) c = 0.5f;
    out[0] = std::nextafterf(c, 0.0f), out[1] = c, out[2] = std::nextafterf(c, INFINITY);
}

uint64_t lanes_part(Tally &ty) {
    std::mt19937_64 rng(0xF6A1ull);
    auto below = [&](uint64_t n) { return n ? rng() % n : 0; };
    auto unit = [&] { return (double)(rng() >> 11) * 0x1p-53; };
    const uint64_t kLanes = 125000;  // each at 3 fixed and 2 x 3 boundary thresholds
    std::vector<uint8_t> sym(8 * 512);
    std::vector<uint32_t> w8(512);
    for (uint64_t it = 0; it < kLanes; ++it) {
        // every 4th lane through the shared route, its code cycling through all e2m3 codes
        const uint32_t code = it % 4 == 3 ? 1 + (uint32_t)(it / 4 % 31) : 0;
        const uint32_t v8 = code ? (uint32_t)std::lround(8.0 * wld::fp6_value(code)) : 0;
        const int mag = (int)below(4);
        const uint32_t N = mag == 0 ? 1 + (uint32_t)below(8) : mag == 1 ? 1 + (uint32_t)below(64) : mag == 2 ? 1 + (uint32_t)below(512) : 512 - (uint32_t)below(8);
        const int wk = (int)below(3);  // weights: one value, small, any
        const uint32_t w1 = 1 + (uint32_t)below(60);
        for (uint32_t k = 0; k < N; ++k) w8[k] = v8 ? v8 : wk == 0 ? w1 : wk == 1 ? 1 + (uint32_t)below(8) : 1 + (uint32_t)below(60);
        // sites 0-3 the rows, 4-7 the columns: symbols 0 missing, 1 minor, 2 major
        // (two lanes in three synth-like in every site, so that the quick test
        // skips in number; the others any mixture per site)
        const bool benign = below(3) != 0;
        for (int site = 0; site < 8; ++site) {
            const int shape = benign ? 3 : (int)below(3);
            const double pm = shape == 3 ? 0.02 + 0.18 * unit() : shape == 0 ? 0.1 : shape == 1 ? unit() : unit() * unit() * unit();
            const double pn = shape == 3 ? 0.15 + 0.3 * unit() : shape == 0 ? 0.3 : (1.0 - pm) * unit();
            for (uint32_t k = 0; k < N; ++k) {
                const double x = unit();
                sym[site * 512 + k] = x < pm ? 0 : x < pm + pn ? 1 : 2;
            }
        }
        // adversarial columns
        const int adv = (int)below(15);  // (5 and above: none)
        const int col = 4 + (int)below(4);
        for (uint32_t k = 0; k < N; ++k) {
            uint8_t &c = sym[col * 512 + k];
            if (adv == 0 && c == 0) c = 2;                       // no missing
            if (adv == 1) c = 0;                                 // all missing
            if (adv == 2 && c == 1) c = 2;                       // no minor
            if (adv == 3) c = c == 1 ? 2 : c;                    // one minor (set below)
            if (adv == 4) c = sym[(int)(it % 4) * 512 + k];      // a copy of a row site
        }
        if (adv == 3) sym[col * 512 + below(N)] = 1;
        Lane L;
        const double u = 0.125;
        uint64_t W = 0, M[8] = {}, m[8] = {};
        for (uint32_t k = 0; k < N; ++k) {
            W += w8[k];
            for (int site = 0; site < 8; ++site) M[site] += sym[site * 512 + k] == 0 ? w8[k] : 0, m[site] += sym[site * 512 + k] == 1 ? w8[k] : 0;
        }
        L.W6 = (float)(u * (double)W);
        for (int i = 0; i < 4; ++i) {
            L.Ma[i] = (float)(u * (double)M[i]), L.ma[i] = (float)(u * (double)m[i]);
            L.Mb[i] = (float)(u * (double)M[4 + i]), L.mb[i] = (float)(u * (double)m[4 + i]);
        }
        for (int e = 0; e < 4; ++e)
            for (int n = 0; n < 4; ++n) {
                uint64_t P01 = 0, P10 = 0, P11 = 0, C01 = 0, C10 = 0, C11 = 0;
                for (uint32_t k = 0; k < N; ++k) {
                    const uint8_t a = sym[e * 512 + k], b = sym[(4 + n) * 512 + k];
                    if (a == 0 && b == 1) P01 += w8[k], ++C01;
                    if (a == 1 && b == 0) P10 += w8[k], ++C10;
                    if (a == 1 && b == 1) P11 += w8[k], ++C11;
                }
                if (v8) {  // the shared image's counts 2 C01, 2 C10 + C11, C11, scaled as the kernel scales them
                    const float v = (float)(u * (double)v8);
                    L.p[e][n] = (float)(2 * C01) * (0.5f * v), L.s[e][n] = (float)(2 * C10 + C11) * v, L.t[e][n] = (float)C11 * v;
                    CHECK((double)L.p[e][n] == u * (double)P01 && (double)L.s[e][n] == u * (double)(2 * P10 + P11) && (double)L.t[e][n] == u * (double)P11,
                          "the scaled counts are not the weight sums");
                } else {
                    L.p[e][n] = (float)(u * (double)P01), L.s[e][n] = (float)(u * (double)(2 * P10 + P11)), L.t[e][n] = (float)(u * (double)P11);
                }
            }
        // R: none, the rounding residual's size, large; on the 1/32 grid as fp6_screen_args puts it
        const double Wt = u * (double)W;
        const int rk = (int)below(4);
        const double R = rk == 0 ? 0.0 : rk == 1 ? Wt * 0.002 * (double)below(16) : rk == 2 ? Wt / 3.0 : (double)below(8) / 32.0;
        const float Rf = (float)(std::ceil(R * 32.0) / 32.0), R2 = 2.0f * Rf;
        float E, mloc;
        // Tg bounds every doubled T: 2 W6, or a load's larger bound
        wld::screen_consts((float)(2.0 * Wt * (below(2) ? 1.0 : 1.5)), R2, E, mloc);
        const char *what = code ? "shared lane" : "lane";
        const LaneTerms z = lane_terms(L, R2, what);
        const float fixed[3] = {0.05f * (1.0f - 0x1p-7f), 0.5f * (1.0f - 0x1p-7f), (float)unit()};
        for (float thr_c : fixed) implication(L, z, thr_c, E, mloc, ty, what);
        // the lane's boundary: t1' = n2 - thr_c P'
        float crit[3], mlo;
        {
            const double n2 = (double)wld::f6q_lane_terms(z.acc, z.rm, z.cm, 0.0f, E, mlo);
            around(n2, n2 - (double)wld::f6q_lane_terms(z.acc, z.rm, z.cm, 1.0f, E, mlo), crit);
        }
        for (float thr_c : crit) implication(L, z, thr_c, E, mloc, ty, code ? "shared lane, quick boundary" : "lane, quick boundary");
        // the worst pair's: the one whose t1 changes sign at the largest threshold
        double worst = -1.0, wn2 = 0.0, wP = 0.0;
        for (int e = 0; e < 4; ++e)
            for (int n = 0; n < 4; ++n) {
                const double n2 = (double)wld::r2_screen_terms_f6t(L.p[e][n], L.s[e][n], L.t[e][n], z.ra[e], z.cb[n], 0.0f, E, mlo);
                const double P = n2 - (double)wld::r2_screen_terms_f6t(L.p[e][n], L.s[e][n], L.t[e][n], z.ra[e], z.cb[n], 1.0f, E, mlo);
                const double c = P > 0.0 ? n2 / P : INFINITY;
                if (std::isfinite(c) && c > worst) worst = c, wn2 = n2, wP = P;
            }
        around(wn2, wP, crit);
        for (float thr_c : crit) implication(L, z, thr_c, E, mloc, ty, code ? "shared lane, pair boundary" : "lane, pair boundary");
    }
    return kLanes;
}

// Part 2: the synth-like sample, lane by lane as the kernel lays a tile out:
// row block r of a tile, lane l: rows 16 r + 4 (l >> 4) + e, columns (l & 15) + 16 n.
void synth_part() {
    const size_t L = 2048, N = 2000, NW = (N + 63) / 64, T = L / 64;
    std::mt19937_64 rng(0x5EEDull);
    std::vector<uint64_t> miss(L * NW, 0), minor(L * NW, 0);
    std::vector<uint64_t> Mc(L, 0), mc(L, 0);
    for (size_t s = 0; s < L; ++s)
        for (size_t k = 0; k < N; ++k) {
            const double x = (double)(rng() >> 11) * 0x1p-53;
            if (x < 0.1)
                miss[s * NW + k / 64] |= 1ull << (k % 64), ++Mc[s];
            else if (x >= 0.7)
                minor[s * NW + k / 64] |= 1ull << (k % 64), ++mc[s];
        }
    const float v = 4.0f;  // every weight on the code of 4.0
    const float Rf = (float)(std::ceil(37.53 * 32.0) / 32.0), R2 = 2.0f * Rf, thr_c = 0.05f * (1.0f - 0x1p-7f);
    float E, mloc;
    wld::screen_consts((float)(2.0 * 4.0 * (double)N), R2, E, mloc);
    Tally ty;
    uint64_t blocks = 0, fell = 0, lanes = 0;
    for (size_t ta = 0; ta < T; ++ta)
        for (size_t tb = ta + 1; tb < T; ++tb)
            for (size_t r = 0; r < 4; ++r) {
                bool every = true;
                for (size_t l = 0; l < 64; ++l) {
                    Lane ln;
                    ln.W6 = v * (float)N;
                    for (int i = 0; i < 4; ++i) {
                        const size_t a = 64 * ta + 16 * r + 4 * (l >> 4) + (size_t)i, b = 64 * tb + (l & 15) + 16 * (size_t)i;
                        ln.Ma[i] = v * (float)Mc[a], ln.ma[i] = v * (float)mc[a];
                        ln.Mb[i] = v * (float)Mc[b], ln.mb[i] = v * (float)mc[b];
                    }
                    for (int e = 0; e < 4; ++e)
                        for (int n = 0; n < 4; ++n) {
                            const size_t a = 64 * ta + 16 * r + 4 * (l >> 4) + (size_t)e, b = 64 * tb + (l & 15) + 16 * (size_t)n;
                            uint64_t C01 = 0, C10 = 0, C11 = 0;
                            for (size_t w = 0; w < NW; ++w) {
                                const uint64_t am = miss[a * NW + w], an = minor[a * NW + w], bm = miss[b * NW + w], bn = minor[b * NW + w];
                                C01 += (uint64_t)__builtin_popcountll(am & bn), C10 += (uint64_t)__builtin_popcountll(an & bm);
                                C11 += (uint64_t)__builtin_popcountll(an & bn);
                            }
                            ln.p[e][n] = (float)(2 * C01) * (0.5f * v), ln.s[e][n] = (float)(2 * C10 + C11) * v, ln.t[e][n] = (float)C11 * v;
                        }
                    const LaneTerms z = lane_terms(ln, R2, "synth");
                    every = implication(ln, z, thr_c, E, mloc, ty, "synth") && every;
                    ++lanes;
                }
                ++blocks, fell += !every;
            }
    std::printf("synth sample: %" PRIu64 " row blocks (%" PRIu64 " lanes), %" PRIu64 " fell through the quick test; lanes skipped %" PRIu64
                ", lanes whose 16 pairs the full test skips %" PRIu64 "\n", blocks, lanes, fell, ty.quick, ty.full_all);
    CHECK(blocks == 1984, "%" PRIu64 " row blocks", blocks);
    CHECK(fell * 10 <= blocks, "%" PRIu64 " of %" PRIu64 " row blocks fell through: more than 1 in 10", fell, blocks);
}
}  // namespace

int main() {
    Tally ty;
    const uint64_t lanes = lanes_part(ty);
    std::printf("lanes: %" PRIu64 ", tests %" PRIu64 ": skipped by the quick test %" PRIu64 ", all 16 pairs skipped by the full test %" PRIu64 "\n",
                lanes, ty.tests, ty.quick, ty.full_all);
    CHECK(ty.tests >= 1000000ull, "only %" PRIu64 " tests", ty.tests);
    // the check has teeth only if both outcomes occur in number
    CHECK(ty.quick * 20 >= ty.tests && (ty.tests - ty.quick) * 20 >= ty.tests && ty.full_all >= ty.quick,
          "outcomes %" PRIu64 " / %" PRIu64 " of %" PRIu64, ty.quick, ty.full_all, ty.tests);
    synth_part();
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
