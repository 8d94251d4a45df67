// Host check of the fp6 screen's per-load site records, its count units and
// its quick test on the one-sided cap (pair_common.hpp f6_row_rec, f6_col_rec,
// f6_row_min_rec, f6_col_min_rec, f6q_pair1, f6q_pmax; no device code runs;
// tests/test_f6_quick_units.py builds this plain and under AddressSanitizer +
// UndefinedBehaviorSanitizer).
//
// (i)   Records.  A site's record holds f6t_row's / f6t_col's fields bit for
//       bit (weight units), and in count units the same fields times 1 / wv,
//       which are also those functions' on the inputs times 1 / wv; cW is (row
//       + col) + Ma2 of every row site of the lane; the group records are
//       f6q_row_min / f6q_col_min of the sites' records.
// (ii)  Count units.  For every power-of-two weight code (0.125 ... 4) the
//       quick test and the three-sum test on the shared image's raw counts,
//       count-unit records, E / wv^2 and mloc / wv decide exactly as on the
//       scaled sums and weight-unit records: t1 <= 0 and mlo >= mloc agree on
//       every lane and on every pair.
// (iii) One-sided cap.  Wherever the new quick test skips a lane's 16 pairs,
//       r2_screen_terms_f6t skips every one of them, and each pair's nt' is at
//       least f6q_pair's nt.
//
// Part 1: tests/cpp/f6_quick_check.cpp's lane generator (4 row and 4 column
// sites over 1 to 512 sequences, weights on the 1/8 grid, adversarial columns,
// R and Tg varied; per lane thresholds 0.05 and 0.5, a random one, the f32
// neighbours of the threshold at which the quick test's t1' changes sign and
// of the one at which the worst pair's t1 does); every 4th lane goes through
// the shared image's counts, alternately on a power-of-two code (cycling
// through the six) and on any of the 31 codes.
// Part 2: 2,048 sites x 2,000 sequences of bench.synth's distribution, every
// weight on the code of 4.0, R = 37.53 and thr = 0.05 as C4 has them, in count
// units as the kernel runs them: the implication on every lane, and at most
// 1/10 of the 1,984 row blocks falling through (f6_quick_check.cpp's cap; the
// two-sided cap leaves 32, this one 54).
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
bool same6(const float *a, const float *b, float scale) {
    for (int i = 0; i < 6; ++i)
        if (bits_of(a[i]) != bits_of(b[i] * scale)) return false;
    return true;
}

// One lane's view of a row block: the sites' marginals and the 16 pairs' sums
// in weight units, and for a shared lane (v > 0) the image's raw counts 2 C01,
// 2 C10 + C11, C11.
struct Lane {
    float W6;
    float Ma[4], ma[4], Mb[4], mb[4];
    float p[4][4], s[4][4], t[4][4];  // [e][n]
    float v = 0.0f;
    float c2p[4][4], cs[4][4], ct[4][4];
};

bool pow2(float v) {
    int e;
    return v > 0.0f && std::frexp(v, &e) == 0.5f;
}

// A lane's records in one unit (inv = 1: weight units), checked against
// f6t_row / f6t_col as they are formed: (i).
struct Recs {
    wld::F6RowRec r[4];
    wld::F6ColRec c[4];
    wld::F6MinRec rmin, cmin;
};
Recs records(const Lane &L, float R2, float inv, const char *what) {
    Recs z;
    for (int e = 0; e < 4; ++e) {
        z.r[e] = wld::f6_row_rec(L.W6, L.Ma[e], L.ma[e], R2, inv);
        const wld::F6tRow a = wld::f6t_row(L.W6, L.Ma[e], L.ma[e], R2);
        const wld::F6tRow ai = wld::f6t_row(L.W6 * inv, L.Ma[e] * inv, L.ma[e] * inv, R2 * inv);
        CHECK(same6(&z.r[e].a.rA, &a.rA, inv) && same6(&z.r[e].a.rA, &ai.rA, 1.0f), "%s: row record %d is not f6t_row's (inv %a)", what, e, inv);
    }
    for (int n = 0; n < 4; ++n) {
        z.c[n] = wld::f6_col_rec(L.W6, L.Mb[n], L.mb[n], R2, inv);
        const wld::F6tCol b = wld::f6t_col(L.Mb[n], L.mb[n], R2);
        const wld::F6tCol bi = wld::f6t_col(L.Mb[n] * inv, L.mb[n] * inv, R2 * inv);
        CHECK(same6(&z.c[n].b.cB2, &b.cB2, inv) && same6(&z.c[n].b.cB2, &bi.cB2, 1.0f), "%s: column record %d is not f6t_col's (inv %a)", what, n, inv);
        for (int e = 0; e < 4; ++e) {
            const wld::F6tRow a = wld::f6t_row(L.W6, L.Ma[e], L.ma[e], R2);
            CHECK(bits_of(z.c[n].cW) == bits_of(((a.row + b.col) + a.Ma2) * inv), "%s: cW of column %d is not (row + col) + Ma2 of row %d", what, n, e);
        }
    }
    z.rmin = wld::f6_row_min_rec(z.r);
    z.cmin = wld::f6_col_min_rec(z.c);
    wld::F6qRowMin rm{INFINITY, INFINITY, INFINITY};
    wld::F6tCol cb[4];
    for (int i = 0; i < 4; ++i) wld::f6q_row_min(rm, z.r[i].a), cb[i] = z.c[i].b;
    const wld::F6qColMin cm = wld::f6q_col_min(cb);
    CHECK(bits_of(z.rmin.x) == bits_of(rm.c1) && bits_of(z.rmin.y) == bits_of(rm.rA2) && bits_of(z.rmin.z) == bits_of(rm.rA) &&
              bits_of(z.cmin.x) == bits_of(cm.cB2) && bits_of(z.cmin.y) == bits_of(cm.cB3) && bits_of(z.cmin.z) == bits_of(cm.c4),
          "%s: the group records are not the sites' minima", what);
    return z;
}

// The new quick test of a lane as the kernel runs it (pair_mfma.hip
// f6t_quick_skip): kCounts on the raw counts and count-unit records.
struct Quick {
    bool skip;
    float t1, mlo;
    float nt[4][4];
};
template <bool kCounts>
Quick quick(const Lane &L, const Recs &z, float thr_c, float E, float mloc) {
    Quick k;
    wld::F6qAcc acc;
    for (int e = 0; e < 4; ++e)
        for (int n = 0; n < 4; ++n)
            k.nt[e][n] = wld::f6q_pair1<kCounts>(kCounts ? L.c2p[e][n] : L.p[e][n], kCounts ? L.cs[e][n] : L.s[e][n],
                                                 kCounts ? L.ct[e][n] : L.t[e][n], z.r[e].a.ma2, z.r[e].a.row, z.c[n].b.mb,
                                                 z.c[n].b.col, z.c[n].cW, acc);
    wld::f6q_pmax<kCounts>(acc);
    k.t1 = wld::f6q_lane_terms(acc, wld::F6qRowMin{z.rmin.x, z.rmin.y, z.rmin.z}, wld::F6qColMin{z.cmin.x, z.cmin.y, z.cmin.z},
                               thr_c, E, k.mlo);
    k.skip = wld::f6q_skip(k.t1, k.mlo, mloc);
    return k;
}

struct Tally {
    uint64_t tests = 0, quick = 0, full_all = 0, count_tests = 0, count_quick = 0;
};

// One (lane, thr_c): (iii) in weight units, and for a power-of-two shared lane
// (ii) against count units.  Returns whether the quick test skipped.
bool implication(const Lane &L, const Recs &zw, const Recs *zc, float thr_c, float E, float mloc, Tally &ty, const char *what) {
    const Quick kw = quick<false>(L, zw, thr_c, E, mloc);
    const float inv = zc ? 1.0f / L.v : 1.0f, Ec = E * inv * inv, mlocc = mloc * inv;
    Quick kc{};
    if (zc) {
        kc = quick<true>(L, *zc, thr_c, Ec, mlocc);
        CHECK((kc.t1 <= 0.0f) == (kw.t1 <= 0.0f) && (kc.mlo >= mlocc) == (kw.mlo >= mloc) && kc.skip == kw.skip,
              "%s: the count-unit quick test (t1' %a mlo' %a mloc %a) decides otherwise than the scaled one (t1' %a mlo' %a mloc %a), v %a",
              what, kc.t1, kc.mlo, mlocc, kw.t1, kw.mlo, mloc, L.v);
        ++ty.count_tests, ty.count_quick += kc.skip;
    }
    bool all = true;
    wld::F6qAcc old;
    for (int e = 0; e < 4; ++e)
        for (int n = 0; n < 4; ++n) {
            const wld::F6tRow &ra = zw.r[e].a;  // (f6t_row's bit for bit: records())
            const wld::F6tCol &cb = zw.c[n].b;
            float mlo;
            const float t1 = wld::r2_screen_terms_f6t(L.p[e][n], L.s[e][n], L.t[e][n], ra, cb, thr_c, E, mlo);
            const bool k = t1 <= 0.0f && mlo >= mloc;
            all = all && k;
            CHECK(!kw.skip || k, "%s: the quick test skips (t1' %a mlo' %a mloc %a), pair (%d, %d) does not (t1 %a mlo %a): p %a s %a t %a thr_c %a E %a",
                  what, kw.t1, kw.mlo, mloc, e, n, t1, mlo, L.p[e][n], L.s[e][n], L.t[e][n], thr_c, E);
            CHECK(kw.mlo <= mlo, "%s: mlo' %a above pair (%d, %d)'s mlo %a", what, kw.mlo, e, n, mlo);
            if (kw.mlo >= 0.0f) CHECK(kw.t1 >= t1, "%s: t1' %a below pair (%d, %d)'s t1 %a", what, kw.t1, e, n, t1);
            const float nt = wld::f6q_pair(L.p[e][n], L.s[e][n], L.t[e][n], ra, cb, old);
            CHECK(kw.nt[e][n] >= nt, "%s: pair (%d, %d) nt' %a below f6q_pair's nt %a", what, e, n, kw.nt[e][n], nt);
            if (zc) {
                float mloq;
                const float t1c = wld::r2_screen_terms_f6t(0.5f * L.c2p[e][n], L.cs[e][n], L.ct[e][n], zc->r[e].a, zc->c[n].b, thr_c, Ec, mloq);
                CHECK((t1c <= 0.0f) == (t1 <= 0.0f) && (mloq >= mlocc) == (mlo >= mloc),
                      "%s: the count-unit full test of pair (%d, %d) (t1 %a mlo %a mloc %a) decides otherwise than the scaled one (t1 %a mlo %a mloc %a), v %a",
                      what, e, n, t1c, mloq, mlocc, t1, mlo, mloc, L.v);
                CHECK(!kc.skip || (t1c <= 0.0f && mloq >= mlocc), "%s: the count-unit quick test skips, pair (%d, %d) in count units does not", what, e, n);
                CHECK(bits_of(kc.nt[e][n]) == bits_of(kw.nt[e][n] * (inv * inv)), "%s: pair (%d, %d) count-unit nt' %a is not the scaled %a / v^2", what, e, n, kc.nt[e][n], kw.nt[e][n]);
            }
        }
    ++ty.tests, ty.quick += kw.skip, ty.full_all += all;
    return kw.skip;
}

// The f32 thresholds around n2 / P, where a t1 = n2 - thr_c P changes sign.
void around(double n2, double P, float (&out)[3]) {
    float c = P > 0.0 ? (float)(n2 / P) : 0.5f;
    if (!(c > 0.0f) || !std::isfinite(c)) c = 0.5f;
    out[0] = std::nextafterf(c, 0.0f), out[1] = c, out[2] = std::nextafterf(c, INFINITY);
}

uint64_t lanes_part(Tally &ty) {
    std::mt19937_64 rng(0xF6A2ull);
    auto below = [&](uint64_t n) { return n ? rng() % n : 0; };
    auto unit = [&] { return (double)(rng() >> 11) * 0x1p-53; };
    const uint64_t kLanes = 125000;  // each at 3 fixed and 2 x 3 boundary thresholds
    const uint32_t kPow2Codes[6] = {1, 2, 4, 8, 16, 24};  // e2m3 codes of 0.125, 0.25, 0.5, 1, 2, 4
    std::vector<uint8_t> sym(8 * 512);
    std::vector<uint32_t> w8(512);
    for (uint64_t it = 0; it < kLanes; ++it) {
        // every 4th lane through the shared route: alternately a power-of-two code and any code
        uint32_t code = 0;
        if (it % 4 == 3) code = it / 4 % 2 == 0 ? kPow2Codes[it / 8 % 6] : 1 + (uint32_t)(it / 8 % 31);
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
        L.v = v8 ? (float)(u * (double)v8) : 0.0f;
        for (int e = 0; e < 4; ++e)
            for (int n = 0; n < 4; ++n) {
                uint64_t P01 = 0, P10 = 0, P11 = 0, C01 = 0, C10 = 0, C11 = 0;
                for (uint32_t k = 0; k < N; ++k) {
                    const uint8_t a = sym[e * 512 + k], b = sym[(4 + n) * 512 + k];
                    if (a == 0 && b == 1) P01 += w8[k], ++C01;
                    if (a == 1 && b == 0) P10 += w8[k], ++C10;
                    if (a == 1 && b == 1) P11 += w8[k], ++C11;
                }
                L.c2p[e][n] = (float)(2 * C01), L.cs[e][n] = (float)(2 * C10 + C11), L.ct[e][n] = (float)C11;
                if (v8) {  // the shared image's counts, scaled as the kernel's scaled path scales them
                    L.p[e][n] = L.c2p[e][n] * (0.5f * L.v), L.s[e][n] = L.cs[e][n] * L.v, L.t[e][n] = L.ct[e][n] * L.v;
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
        const bool counts = pow2(L.v);
        const char *what = counts ? "count-unit lane" : code ? "shared lane" : "lane";
        const Recs zw = records(L, R2, 1.0f, what);
        Recs zcs;
        if (counts) zcs = records(L, R2, 1.0f / L.v, what);
        const Recs *zc = counts ? &zcs : nullptr;
        const float fixed[3] = {0.05f * (1.0f - 0x1p-7f), 0.5f * (1.0f - 0x1p-7f), (float)unit()};
        for (float thr_c : fixed) implication(L, zw, zc, thr_c, E, mloc, ty, what);
        // the lane's boundary: t1' = n2 - thr_c P'
        float crit[3], mlo;
        {
            const double n2 = (double)quick<false>(L, zw, 0.0f, E, mloc).t1;
            around(n2, n2 - (double)quick<false>(L, zw, 1.0f, E, mloc).t1, crit);
        }
        for (float thr_c : crit) implication(L, zw, zc, thr_c, E, mloc, ty, what);
        // the worst pair's: the one whose t1 changes sign at the largest threshold
        double worst = -1.0, wn2 = 0.0, wP = 0.0;
        for (int e = 0; e < 4; ++e)
            for (int n = 0; n < 4; ++n) {
                const double n2 = (double)wld::r2_screen_terms_f6t(L.p[e][n], L.s[e][n], L.t[e][n], zw.r[e].a, zw.c[n].b, 0.0f, E, mlo);
                const double P = n2 - (double)wld::r2_screen_terms_f6t(L.p[e][n], L.s[e][n], L.t[e][n], zw.r[e].a, zw.c[n].b, 1.0f, E, mlo);
                const double c = P > 0.0 ? n2 / P : INFINITY;
                if (std::isfinite(c) && c > worst) worst = c, wn2 = n2, wP = P;
            }
        around(wn2, wP, crit);
        for (float thr_c : crit) implication(L, zw, zc, thr_c, E, mloc, ty, what);
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
                    ln.v = v;
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
                            ln.c2p[e][n] = (float)(2 * C01), ln.cs[e][n] = (float)(2 * C10 + C11), ln.ct[e][n] = (float)C11;
                            ln.p[e][n] = ln.c2p[e][n] * (0.5f * v), ln.s[e][n] = ln.cs[e][n] * v, ln.t[e][n] = ln.ct[e][n] * v;
                        }
                    const Recs zw = records(ln, R2, 1.0f, "synth"), zc = records(ln, R2, 1.0f / v, "synth");
                    every = implication(ln, zw, &zc, thr_c, E, mloc, ty, "synth") && every;
                    ++lanes;
                }
                ++blocks, fell += !every;
            }
    std::printf("synth sample: %" PRIu64 " row blocks (%" PRIu64 " lanes), %" PRIu64 " fell through the quick test; lanes skipped %" PRIu64
                " (%" PRIu64 " in count units), lanes whose 16 pairs the full test skips %" PRIu64 "\n",
                blocks, lanes, fell, ty.quick, ty.count_quick, ty.full_all);
    CHECK(blocks == 1984, "%" PRIu64 " row blocks", blocks);
    CHECK(ty.count_quick == ty.quick, "count units skipped %" PRIu64 " lanes, the scaled path %" PRIu64, ty.count_quick, ty.quick);
    CHECK(fell * 10 <= blocks, "%" PRIu64 " of %" PRIu64 " row blocks fell through: more than 1 in 10", fell, blocks);
}
}  // namespace

int main() {
    Tally ty;
    const uint64_t lanes = lanes_part(ty);
    std::printf("lanes: %" PRIu64 ", tests %" PRIu64 ": skipped by the quick test %" PRIu64 ", all 16 pairs skipped by the full test %" PRIu64
                "; in count units %" PRIu64 " tests, %" PRIu64 " skipped\n",
                lanes, ty.tests, ty.quick, ty.full_all, ty.count_tests, ty.count_quick);
    CHECK(ty.tests >= 1000000ull, "only %" PRIu64 " tests", ty.tests);
    // the check has teeth only if both outcomes occur in number
    CHECK(ty.quick * 20 >= ty.tests && (ty.tests - ty.quick) * 20 >= ty.tests && ty.full_all >= ty.quick,
          "outcomes %" PRIu64 " / %" PRIu64 " of %" PRIu64, ty.quick, ty.full_all, ty.tests);
    CHECK(ty.count_tests >= 100000ull && ty.count_quick * 20 >= ty.count_tests && (ty.count_tests - ty.count_quick) * 20 >= ty.count_tests,
          "count-unit outcomes %" PRIu64 " of %" PRIu64, ty.count_quick, ty.count_tests);
    synth_part();
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
