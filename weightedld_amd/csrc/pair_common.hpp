// Device helpers shared by the pair kernels: the LdStats epilogue and the
// tile compaction that feeds the reference-order gather (order.hip).
#pragma once

#include "kernels.hpp"

namespace wld {

// lib.rs:482-520, operation for operation in f32 (the library is built with
// -ffp-contract=off, divisions are IEEE-rounded, fminf/fmaxf ignore NaN like
// Rust's f32::min/max).  Inputs are the four masked weight sums of
// lib.rs:423-480: total_weight, PA (a major), PB (b major), ld_obs[3] (both).
//
// The eight quotients by total_weight (WLD_EPI_DIVT 1, the default) are the
// IEEE f32 quotients computed as RN_f32(x * r) in f64, r a reciprocal of
// total_weight refined to within a few f64 ulps (one hardware estimate, two
// Newton steps), instead of eight f32 division sequences.  Why that is the
// correctly rounded quotient: a midpoint m between two f32 values (a 25-bit
// odd significand M) can equal x / T only if T is a power of two, and then
// x / T is an f32 value itself, so no quotient of two f32 values is a tie;
// and a quotient that is not a midpoint lies at least 1 / (M U) >= 2^-49 of m
// from it (|x - m T| is at least the unit of m T's last place, x = X 2^a with
// 24-bit X, T = U 2^c), while RN_f64(x * r) is within ~2^-51 of x / T: both
// round to the same f32 value (subnormal results too: their midpoints are
// coarser).  T = 0 or non-finite takes the plain divisions (IEEE's inf / NaN).
#ifndef WLD_EPI_DIVT
#define WLD_EPI_DIVT 1
#endif
// (r0: the estimate to refine; the device's v_rcp_f64, the host check's a
// coarser one, the f32 reciprocal)
__host__ __device__ __forceinline__ double recip_f64(double t, double r0) {
    double r = r0;
    double e = fma(-t, r, 1.0);
    r = fma(r, e, r);
    e = fma(-t, r, 1.0);
    return fma(r, e, r);
}
// The host's estimate: the f32 reciprocal, a subnormal t first scaled into
// the normal range (1.0f / t overflows to inf there)
__host__ __forceinline__ double recip_seed_host(float t) {
    return fabsf(t) < 0x1p-126f ? (double)(1.0f / (t * 0x1p64f)) * 0x1p64 : (double)(1.0f / t);
}
__host__ __device__ __forceinline__ void ld_epilogue(float total_weight, float PA, float PB, float ld3, float &d_out,
                                                     float &dp_out, float &r2_out) {
    float ld_obs0, ld_obs1, ld_obs2, ld_obs3 = ld3;
    float Pa = total_weight - PA;
    float Pb = total_weight - PB;
    ld_obs2 = PA - ld_obs3;
    ld_obs1 = PB - ld_obs3;
    ld_obs0 = Pa - ld_obs1;
    if (WLD_EPI_DIVT && total_weight != 0.0f && fabsf(total_weight) <= 3.4028235e38f) {
#if defined(__HIP_DEVICE_COMPILE__)
        const double r = recip_f64((double)total_weight, __builtin_amdgcn_rcp((double)total_weight));
#else
        const double r = recip_f64((double)total_weight, recip_seed_host(total_weight));
#endif
        PA = (float)((double)PA * r);
        PB = (float)((double)PB * r);
        Pa = (float)((double)Pa * r);
        Pb = (float)((double)Pb * r);
        ld_obs0 = (float)((double)ld_obs0 * r);
        ld_obs1 = (float)((double)ld_obs1 * r);
        ld_obs2 = (float)((double)ld_obs2 * r);
        ld_obs3 = (float)((double)ld_obs3 * r);
    } else {
        PA = PA / total_weight;
        PB = PB / total_weight;
        Pa = Pa / total_weight;
        Pb = Pb / total_weight;
        ld_obs0 = ld_obs0 / total_weight;
        ld_obs1 = ld_obs1 / total_weight;
        ld_obs2 = ld_obs2 / total_weight;
        ld_obs3 = ld_obs3 / total_weight;
    }
    const float PAB = PA * PB;
    const float PAb = PA * Pb;
    const float PaB = Pa * PB;
    const float Pab = Pa * Pb;
    const float d = ((PAB - ld_obs3) + (Pab - ld_obs0) + (ld_obs2 - PAb) + (ld_obs1 - PaB)) / 4.0f;
    float den;
    if (d < 0.0f) {
        den = fmaxf(-ld_obs0, -ld_obs3);
        if (den == 0.0f) den = fminf(-ld_obs0, -ld_obs3);
    } else {
        den = fminf(ld_obs1, ld_obs2);
        if (den == 0.0f) den = fmaxf(ld_obs1, ld_obs2);
    }
    d_out = d;
    dp_out = d / den;
    r2_out = d * d / (PA * Pa * PB * Pb);
}

// Rigorous skip test for the r2 > thr filter (thr > 0).  T, A, B, AB are
// approximations of a pair's exact masked sums T, SA, SB, SAB (any common
// unit) whose 2x2 cells n11 = AB, n10 = A-AB, n01 = B-AB, n00 = T-A-B+AB are
// each within e_c of the exact cells, sum_c |e_c| <= R (R = 0: the sums are
// exact).  Returns true only if ld_epilogue, run on the correctly rounded f32
// values of the EXACT sums, cannot give r2 > thr — so skipping the pair never
// changes the output.  Derivation ("Prefilter and screen"):
//   * the f32 epilogue's d is within e_d = 16.25u (u = 2^-24) of the exact
//     D = (SA SB - SAB T) / T^2 (all normalised quantities in [0, 1]), and its
//     denominator PA Pa PB Pb is >= P (1 - 5u sum_i 1/f_i - 3u), f_i the four
//     normalised marginals, so r2_f32 <= (|D| + e_d)^2 (1+u)^2 / (P (1 - rel));
//   * with uncertain sums, |num - num^| <= R max_c |n^_c| + R^2/4, each
//     marginal is within R, T within R.
// Evaluated division-free in f64 with e_d = 24u, rel = 28u T/m + 8u, and a
// 1e-12 relative allowance for the f64 evaluation itself.  Exact cells must be
// >= 0 (normalised quantities in [0, 1]): guaranteed for nonnegative weights,
// else checked as n^_c >= R.
// (__host__ as well: tests/cpp/bound_check.cpp runs the same code on the CPU.)
__host__ __device__ __forceinline__ bool r2_bound_skip(double T, double A, double B, double AB, double R, float thr,
                                                       bool nonneg) {
    constexpr double u = 0x1p-24;
    const double n10 = A - AB, n01 = B - AB, n00 = (T - A) - n01;
    if (!nonneg && fmin(fmin(AB, n10), fmin(n01, n00)) < R) return false;
    const double cmax = fmax(fmax(fabs(AB), fabs(n10)), fmax(fabs(n01), fabs(n00)));
    const double m1 = A - R, m2 = (T - A) - R, m3 = B - R, m4 = (T - B) - R;
    const double mlo = fmin(fmin(m1, m2), fmin(m3, m4));
    if (!(mlo > 0.0)) return false;
    const double Tub = T + R;
    const double nub = fabs(A * B - AB * T) + R * cmax + 0.25 * R * R + (24.0 * u + 0x1p-40) * Tub * Tub;
    const double lhs = nub * nub * ((1.0 + 4.0 * u) * (1.0 + 1e-12)) * mlo;
    const double rhs = (double)thr * ((m1 * m2) * (m3 * m4)) * (mlo * (1.0 - 8.0 * u) - 28.0 * u * Tub);
    return lhs <= rhs;
}

// The screen's per-pair test in f32 (about a third of r2_bound_skip's f64
// cost; the one-plane screen kernel is VALU-issue bound).
// Sound under: nonnegative weights; T, A, B, AB integers of magnitude
// <= 2^22 (exact in f32, and so are T - A, T - B); R >= the L1 cell residual
// (rounded up to f32).  It implies r2_bound_skip's inequality:
//   * every approximate sum and cell is <= Tb = T + 2R (exact cells >= 0 sum
//     to at most T + R, each within R), so R cmax <= R Tb, Tub <= Tb;
//   * |fl(fl(A B) - fl(AB T)) - |A B - AB T|| <= 4.02u Tb^2, so
//     E = R Tb + R^2 + 2^-19 Tb^2 (2^-19 = 32u >= 24u + 2^-40 + 4.02u, the
//     slack covering E's own rounding) gives nub <= fl(num + E)(1 + 2u);
//   * m_i = fl(x_i - R) <= (x_i - R)(1 + u), so the f32 product of the four
//     marginals is <= their exact product times (1 + u)^7;
//   * mlo >= 2^-12 Tb bounds r2_bound_skip's 28u Tub / mlo term by 6.84e-3,
//     and c = 1 - 2^-7 covers it with every f32 rounding above (16u).
// No skip (the tile becomes a candidate) whenever it cannot decide.  Finite
// inputs only (integer sums).  tests/test_r2_bound.py checks it on the host.
// Returned as a violation margin: the pair is skipped iff it is <= 0 (both
// terms are differences of f32 values, whose rounded sign is exact).
// thr_c = thr * (1 - 2^-7) in f32.
// The derivation holds for Tb any f32 upper bound of T + 2R (it only bounds
// sums, cells and T + R from above), so a launch may fix Tb from a bound Tg on
// every T it screens (the screen: Tg = 2 sum_k |top digit_k|, doubled sums)
// and precompute E(Tb) and 2^-12 Tb once (screen_consts); per pair that leaves
// r2_screen_terms, whose two terms must both be <= 0 for a skip.
__host__ __device__ __forceinline__ void screen_consts(float Tg, float R, float &E, float &mloc) {
    const float Tb = (Tg + 2.0f * R) * (1.0f + 0x1p-20f);
    E = R * Tb + R * R + 0x1p-19f * (Tb * Tb);
    mloc = 0x1p-12f * Tb;
}
__host__ __device__ __forceinline__ float r2_screen_terms(float T, float A, float B, float AB, float R, float thr_c,
                                                          float E, float mloc, float &t2) {
    const float m1 = A - R, m2 = (T - A) - R, m3 = B - R, m4 = (T - B) - R;
    const float mlo = fminf(fminf(m1, m2), fminf(m3, m4));
    const float nub = fabsf(A * B - AB * T) + E;
    t2 = mloc - mlo;
    return nub * nub - thr_c * ((m1 * m2) * (m3 * m4));
}
// The same terms straight from the i8 kernel's accumulators in doubled units
// (X0 = S(raw), Y0 = S(minor) of channel_a "in", X1, Y1 of "major"; T = X0 +
// Y0, B = X0 - Y0, A = X1 + Y1, AB = X1 - Y1, all exact): T - B = 2 Y0 and
// A B - AB T = 2 (X0 Y1 - X1 Y0).  The marginals round exactly as in
// r2_screen_terms; the numerator by one FMA (error <= 2u (X0 Y1 + X1 Y0) <= 2u
// T^2, inside the 4.02u Tb^2 the derivation allows) and nub = fl(2 |num'| + E)
// rounds once, as fl(|num| + E) did.
__host__ __device__ __forceinline__ float r2_screen_terms_xy(float X0, float Y0, float X1, float Y1, float R,
                                                             float thr_c, float E, float mloc, float &t2) {
    const float T = X0 + Y0, B = X0 - Y0, A = X1 + Y1;
    const float m1 = A - R, m2 = (T - A) - R, m3 = B - R, m4 = fmaf(2.0f, Y0, -R);
    const float mlo = fminf(fminf(m1, m2), fminf(m3, m4));
    const float nub = fmaf(2.0f, fabsf(fmaf(X0, Y1, -(X1 * Y0))), E);
    t2 = mloc - mlo;
    return nub * nub - thr_c * ((m1 * m2) * (m3 * m4));
}
// The same test from the fp6 screen's accumulators (pair_mfma.hip): the b
// codes read as e2m3 (F: minor 2, major 1) and as e3m2 (G: minor 2, major
// 0.5) give, in doubled units, F0 = 2T - SB, G0 = 2T - 1.5 SB (channel_a
// "in") and F1 = 2SA - SAB, G1 = 2SA - 1.5 SAB (channel_a major), so D0 =
// F0 - G0 = SB / 2, D1 = SAB / 2, and the doubled marginals of
// r2_screen_terms_xy are 2T = F0 + 2 D0, 2SB = 4 D0, 2(T - SB) = F0 - 2 D0,
// 2SA = F1 + 2 D1.  Every accumulator is an exact multiple of 1/16 below 2^19
// and R (doubled, R2) is put on that grid by the caller, so every marginal
// below, R subtracted, is exact — the xy form's marginals rounded, these equal
// the exact values.  The numerator A B - AB T = F1 D0 - F0 D1 by one product
// and one FMA: |error| <= 2u (F1 D0 + F0 D1)(1 + u) <= 4u (1 + u) T^2 of the
// doubled T, so 4 |.| is within the 4.02u Tb^2 the derivation allows (nub
// rounds once, as in the xy form).  t1 = fma(nub, nub, -fl(thr_c P)) is <= 0
// only if fl(nub^2) <= fl(thr_c P) (rounding is monotone), i.e. only where
// the xy form's t1 is <= 0.  The second test (every marginal >= mloc) is left
// to the caller as mlo (the screen tracks one minimum over a lane's pairs:
// a tile whose minimum falls below mloc is a candidate, as the xy form's t2
// would make the pair holding it).  Skip iff t1 <= 0 and mlo >= mloc.
__host__ __device__ __forceinline__ float r2_screen_terms_fg(float F0, float G0, float F1, float G1, float R2,
                                                             float thr_c, float E, float &mlo) {
    const float D0 = F0 - G0, D1 = F1 - G1;
    const float F0r = F0 - R2;
    const float m4 = fmaf(-2.0f, D0, F0r), T2r = fmaf(2.0f, D0, F0r), m3 = fmaf(4.0f, D0, -R2);
    const float A2 = fmaf(2.0f, D1, F1);
    const float m1 = A2 - R2, m2 = T2r - A2;
    mlo = fminf(fminf(m1, m2), fminf(m3, m4));
    const float nub = fmaf(4.0f, fabsf(fmaf(F1, D0, -(F0 * D1))), E);
    return fmaf(nub, nub, -(thr_c * ((m1 * m2) * (m3 * m4))));
}
// The same from the fp4-coded b sites' accumulators (pair_mfma.hip, the
// tile-pair fp6 screen with fp4 B): X = the raw codes read as e2m1 (minor 1,
// major 2), Y = their minor bit (raw & 0x2222...): X0 = T + SB, Y0 = T - SB,
// X1 = SA + SAB, Y1 = SA - SAB, so 2T = X0 + Y0, 2SB = X0 - Y0, 2(T - SB) =
// 2 Y0, 2SA = X1 + Y1 (doubled units, as r2_screen_terms_xy).  Accumulators
// and R2 on the 1/8 grid below 2^19: the marginals are exact; the numerator
// and t1 as in r2_screen_terms_xy / _fg (X0 Y1 - X1 Y0 = 2 num, error <= 2u
// (X0 Y1 + X1 Y0)(1 + u) <= 4u T^2: 2u T2^2 after doubling).  Skip iff t1 <= 0
// and mlo >= mloc.  (The fp6 screen's images are complement coded, missing /
// minor in place of in / minor + 2 major; its epilogue first restores these
// X0, Y0, X1, Y1 exactly, f6c_direct below, so nothing here changes.)
// The a site's other allele: with X1', Y1' summed over the sequences where a
// is minor (SA' = T - SA, SA'B = SB - SAB; X1' = X0 - X1, Y1' = Y0 - Y1) the
// function computes the same test with m1 and m2 exchanged: A2' = 2(T - SA),
// so m1' = 2(T - SA) - R2 = m2 and m2' = T2r - A2' = 2SA - R2 = m1, both
// still exact, and the product (m1 m2)(m3 m4) and the minimum are symmetric
// in them, bit for bit.  The numerator X0 Y1' - X1' Y0 = -(X0 Y1 - X1 Y0)
// enters by its magnitude, rounded within 2u (X0 Y1' + X1' Y0)(1 + u), which
// the same 4u T^2 bounds (X1' <= X0, Y1' <= Y0).  So either channel of the a
// site may be passed (the fp6 screen passes the minor one, the i8 screen the
// major one); only the numerator's last ulp can differ between the two.
__host__ __device__ __forceinline__ float r2_screen_terms_xy2(float X0, float Y0, float X1, float Y1, float R2,
                                                              float thr_c, float E, float &mlo) {
    const float X0r = X0 - R2;
    const float T2r = X0r + Y0, m3 = X0r - Y0, m4 = fmaf(2.0f, Y0, -R2);
    const float A2 = X1 + Y1;
    const float m1 = A2 - R2, m2 = T2r - A2;
    mlo = fminf(fminf(m1, m2), fminf(m3, m4));
    const float nub = fmaf(2.0f, fabsf(fmaf(X0, Y1, -(X1 * Y0))), E);
    return fmaf(nub, nub, -(thr_c * ((m1 * m2) * (m3 * m4))));
}
// The fp6 screen's complement coding (pair_mfma.hip frag6_kernel): the A
// channels hold w6 [missing] and w6 [minor], the B nibbles 2.0 for missing,
// 1.0 for minor and 0 for major, so the MFMAs sum mostly zero products where
// the direct coding (in / minor x minor + 2 major) summed mostly nonzero
// ones.  With P = sum_k w6_k (miss | minor of a)_k (miss | minor of b)_k the
// accumulators are aX = 2 P00 + P01, aY = P01, bX = 2 P10 + P11, bY = P11.
// Per sequence [in a] = 1 - [miss a] and [minor b] + 2 [major b] = 2 - 2 [miss
// b] - [minor b], so with the per-site marginals M_s = sum_k w6_k [s missing],
// m_s = sum_k w6_k [s minor] and W6 = sum_k w6_k (fp6_marginals_kernel, once
// per load) the direct coding's accumulators are
//   X0 = aX + (2 (W6 - M_a) + (-2 M_b - m_b))    Y0 = m_b - aY
//   X1 = 2 m_a - bX                              Y1 = bY.
// Exact in f32: w6 is a multiple of 1/8 <= 7.5 and at most 16384 sequences
// carry one, so W6, M, m and every P are multiples of 1/8 below 2^17, and
// every operand, intermediate and result above is a multiple of 1/8 of
// magnitude below 2^19 (|2 (W6 - M_a)|, |2 M_b + m_b| < 2^18, their sum's and
// aX's < 2^18 + 2^17): 22 significant bits at most, no rounding anywhere, in
// any order of evaluation.  So r2_screen_terms_xy2 receives the X0, Y0, X1,
// Y1 the direct coding's MFMAs summed, bit for bit, and every verdict is the
// same (tests/cpp/f6_complement_check.cpp).  The a row's term and the b
// column's are formed once per row / column of a lane's pairs:
__host__ __device__ __forceinline__ float f6c_row_term(float W6, float Ma) { return 2.0f * (W6 - Ma); }
__host__ __device__ __forceinline__ float f6c_col_term(float Mb, float mb) { return fmaf(-2.0f, Mb, -mb); }
// (aX, aY, bX) -> (X0, Y0, X1) in place; row = f6c_row_term of a, col =
// f6c_col_term of b, ma2 = 2 m_a
__host__ __device__ __forceinline__ void f6c_direct(float &x0, float &y0, float &x1, float row, float col, float ma2,
                                                    float mb) {
    x0 = x0 + (row + col);
    y0 = mb - y0;
    x1 = ma2 - x1;
}
// The same from the shared image's accumulators (pair_mfma.hip, a load whose
// weight codes are all the one value v): the A operands are masks of the row
// tile's B image, missing at 2.0 and minor at 1.0, so the four accumulators
// hold counts, 2 (2 C00 + C01), 2 C01, 2 C10 + C11 and C11 with C = sum_k
// (miss | minor of a)_k (miss | minor of b)_k, and aX = (v/2) acc, aY = (v/2)
// acc, bX = v acc, bY = v acc.  Every count is an integer of at most 2^16 (4 x
// 16384) and v, v/2 have at most 4 significant bits, so each product is exact
// and each fmaf below rounds an exactly representable value (f6c_direct's
// argument): X0, Y0, X1, Y1 are f6c_direct's bit for bit
// (tests/cpp/f6_shared_check.cpp).  hv = v / 2.
__host__ __device__ __forceinline__ void f6s_direct(float &x0, float &y0, float &x1, float &y1, float row, float col,
                                                    float ma2, float mb, float v, float hv) {
    x0 = fmaf(hv, x0, row + col);
    y0 = fmaf(-hv, y0, mb);
    x1 = fmaf(-v, x1, ma2);
    y1 = v * y1;
}
// The fp6 screen on three sums (pair_mfma.hip, kThree): the missing-by-missing
// sum P00 is not formed, and the pair is decided from the other three where
// that is possible.  P00 enters the direct coding's sums through X0 alone,
//   X0 = X0lo + 2 P00,  X0lo = X0 restored with aX = aY (P00 = 0: aX = P01),
// and it is bracketed by the sequences where a is missing split by b's symbol
// (M_a = P00 + P01 + sum_k w6_k [a missing][b major]) and the same for b:
//   0 <= P00 <= c = min(M_a - P01, M_b - P10).
// In the restored sums P01 = m_b - Y0 and 2 P10 = 2 m_a - X1 - Y1, so
//   cap2 = 2 c = min(2 M_a + (2 Y0 - 2 m_b), 2 M_b + ((X1 + Y1) - 2 m_a))
// (f6_cap2: operands on the 1/8 grid below 2^19 as everywhere here, exact in
// any order), and X0 lies in [X0lo, X0hi = X0lo + cap2], both exact.
// r2_screen_terms_xy2_t is r2_screen_terms_xy2 with X0 known only as that
// interval.  It is implied-conservative: wherever it skips (t1 <= 0 and mlo >=
// mloc), r2_screen_terms_xy2 on the true X0, in f32 as written above, skips
// too, so the kernel that decides on three sums where it can and forms the
// fourth where it cannot leaves the four-sum kernel's candidate sets and
// sub-block masks, and the four-sum test's soundness proof is all it needs.
//   * Marginals.  m1 and m4 do not contain X0; m2 = (X0 - R2) + Y0 - A2 and m3
//     = (X0 - R2) - Y0 are exact and nondecreasing in X0.  Taken at X0lo they
//     are <= the true ones, so mlo(t) <= mlo(true): mlo(t) >= mloc implies the
//     true test's mlo >= mloc.
//   * Product.  A skip has mlo(t) >= mloc >= 0, so all four marginals at X0lo,
//     and the true ones above them, are nonnegative.  A rounded f32 product
//     of nonnegative factors is nondecreasing in each factor (rounding is
//     monotone), so fl(m1 m2), fl(m3 m4), their rounded product and its
//     rounded product with thr_c >= 0 at X0lo are each <= the same at the
//     true X0: Pt <= P.
//   * Numerator.  q = fl(X1 Y0) is the same f32 number in both tests, and n(X)
//     = fl(X Y1 - q) (one fmaf: a single rounding of the exact value) is
//     nondecreasing in X because Y1 = P11 >= 0 and rounding is monotone.  So
//     the true test's n(X0) lies in [n(X0lo), n(X0hi)] as computed, and
//     |n(X0)| <= max(|n(X0lo)|, |n(X0hi)|) =: nt with no allowance at all: the
//     roundings of the two ends bracket the rounding of the true one.
//   * nub(t) = fl(2 nt + E) >= fl(2 |n(X0)| + E) = nub >= 0 (E >= 0; one fmaf
//     each, monotone), hence nub(t)^2 - Pt >= nub^2 - P exactly, and t1(t) =
//     fl(nub(t)^2 - Pt) >= fl(nub^2 - P) = t1.  So t1(t) <= 0 implies t1 <= 0.
// With cap2 = 0 the two ends coincide and the function is r2_screen_terms_xy2
// bit for bit.  The a site's other allele (r2_screen_terms_xy2's note) needs
// nothing more: the fp6 screen passes the minor channel to both tests.  The
// shared image's counts come through f6s_direct with aX's count = aY's, the
// other images' sums through f6c_direct with aX = aY: the same X0lo, Y0, X1,
// Y1, so one function serves the three formats
// (tests/cpp/f6_three_check.cpp).
__host__ __device__ __forceinline__ float f6_cap2(float Ma2, float ma2, float Mb2, float mb2, float Y0, float X1,
                                                  float Y1) {
    return fminf(Ma2 + fmaf(2.0f, Y0, -mb2), Mb2 + ((X1 + Y1) - ma2));
}
__host__ __device__ __forceinline__ float r2_screen_terms_xy2_t(float X0lo, float Y0, float X1, float Y1, float cap2,
                                                                float R2, float thr_c, float E, float &mlo) {
    const float X0r = X0lo - R2;
    const float T2r = X0r + Y0, m3 = X0r - Y0, m4 = fmaf(2.0f, Y0, -R2);
    const float A2 = X1 + Y1;
    const float m1 = A2 - R2, m2 = T2r - A2;
    mlo = fminf(fminf(m1, m2), fminf(m3, m4));
    const float q = -(X1 * Y0);
    const float nt = fmaxf(fabsf(fmaf(X0lo, Y1, q)), fabsf(fmaf(X0lo + cap2, Y1, q)));
    const float nub = fmaf(2.0f, nt, E);
    return fmaf(nub, nub, -(thr_c * ((m1 * m2) * (m3 * m4))));
}
// The same test straight from the three complement-coded sums p = aY = P01, s
// = bX = 2 P10 + P11, t = bY = P11, with what depends on one site alone formed
// once per row and per column of a lane's pairs: 30 operations per pair where
// restoring X0lo, Y0, X1, Y1 and calling r2_screen_terms_xy2_t takes 37 (the
// kernel's epilogue is bound by exactly these: three waves per SIMD reach it
// together).  With d = s - t = 2 P10:
//   m1 = (2 m_a - R2) - d                        m4 = (2 m_b - R2) - 2 p
//   m2 = ((row - R2 - 2 m_a) + (col + m_b)) + d  m3 = 2 p + ((row - R2) + (col - m_b))
//   cap2 = min(2 M_a - 2 p, 2 M_b - d)           X0lo = p + (row + col)
//   X1 = 2 m_a - s, Y0 = m_b - p, Y1 = t.
// Every operand and intermediate is a multiple of 1/16 of magnitude below
// 2^20 (the 1/8 grid of f6c_direct's argument, and R2 = 2 R with R a multiple
// of 1/32 below 2^17: capi.hip fp6_screen_args), at most 24 significant bits,
// so each value above is exact however it is associated and equals, bit for
// bit, what r2_screen_terms_xy2_t forms from the restored sums; the rounded
// operations (the products, q, the two fmaf of the numerator, nub, t1) are
// the same operations on the same values.  So t1 and mlo are
// r2_screen_terms_xy2_t's bit for bit (tests/cpp/f6_three_check.cpp compares
// them on every table), and its implication holds here unchanged.
struct F6tRow {  // of the a site
    float rA, rA2, c1, Ma2, ma2, row;
};
struct F6tCol {  // of the b site
    float cB2, cB3, c4, Mb2, mb, col;
};
__host__ __device__ __forceinline__ F6tRow f6t_row(float W6, float Ma, float ma, float R2) {
    const float row = f6c_row_term(W6, Ma), ma2 = 2.0f * ma, rA = row - R2;
    return F6tRow{rA, rA - ma2, ma2 - R2, 2.0f * Ma, ma2, row};
}
__host__ __device__ __forceinline__ F6tCol f6t_col(float Mb, float mb, float R2) {
    const float col = f6c_col_term(Mb, mb);
    return F6tCol{col + mb, col - mb, fmaf(2.0f, mb, -R2), 2.0f * Mb, mb, col};
}
__host__ __device__ __forceinline__ float r2_screen_terms_f6t(float p, float s, float t, const F6tRow &a,
                                                              const F6tCol &b, float thr_c, float E, float &mlo) {
    const float d = s - t;
    const float m1 = a.c1 - d, m2 = (a.rA2 + b.cB2) + d;
    const float m3 = fmaf(2.0f, p, a.rA + b.cB3), m4 = fmaf(-2.0f, p, b.c4);
    mlo = fminf(fminf(m1, m2), fminf(m3, m4));
    const float cap2 = fminf(fmaf(-2.0f, p, a.Ma2), b.Mb2 - d);
    const float q = -((a.ma2 - s) * (b.mb - p));
    const float X0lo = p + (a.row + b.col);
    const float nt = fmaxf(fabsf(fmaf(X0lo, t, q)), fabsf(fmaf(X0lo + cap2, t, q)));
    const float nub = fmaf(2.0f, nt, E);
    return fmaf(nub, nub, -(thr_c * ((m1 * m2) * (m3 * m4))));
}
// The quick test in front of r2_screen_terms_f6t (WLD_OPT_FP6_QUICK; pair_mfma.hip
// f6t_quick_skip): a lane's 16 pairs of a row block, 4 row sites e by 4 column
// sites n, rejected together.  Per pair only the numerator is formed, with
// the operations of r2_screen_terms_f6t on the same values (d, q, X0lo, cap2
// and the two fmaf: so the pair's nt is that function's bit for bit), and
// three maxima are kept: nt, d = 2 P10 and p = P01 (f6q_pair, 15 operations
// where the full test takes 30).  Once per lane and row block (f6q_lane_terms)
// the marginals are bounded from the sites' terms alone,
//   m1' = min_e c1 - dmax              m2' = min_e rA2 + min_n cB2
//   m3' = min_e rA + min_n cB3         m4' = min_n c4 - 2 pmax,
// and t1' = fma(nub', nub', -fl(thr_c P')) with nub' = fl(2 nt + E) and P' the
// product of the primed marginals, rounded as r2_screen_terms_f6t rounds its
// own.  Quick skip iff t1' <= 0 and mlo' >= mloc.
// It is implied-conservative: where it skips, r2_screen_terms_f6t skips every
// one of the 16 pairs (t1 <= 0 and mlo >= mloc), in f32 as written, so a row
// block it rejects has no pair in doubt and the three-sum kernel's verdicts
// are unchanged.
//   * Marginals.  Every operand is on the 1/16 grid below 2^20 (the argument
//     above), and so are the minima and maxima of such values: each primed
//     marginal is exact.  d = 2 P10 >= 0 and p = P01 >= 0 are weight sums, so
//     for every pair (e, n) m1' <= c1(e) - d = m1, m2' <= (rA2(e) + cB2(n)) +
//     d = m2, m3' <= 2 p + (rA(e) + cB3(n)) = m3 and m4' <= c4(n) - 2 p = m4:
//     mlo' <= mlo, and mlo' >= mloc implies the pair's mlo >= mloc.
//   * Product.  A skip has mlo' >= mloc >= 0, so the primed marginals and the
//     pair's above them are nonnegative.  A rounded f32 product of nonnegative
//     factors is nondecreasing in each (rounding is monotone): fl(m1' m2'),
//     fl(m3' m4'), their rounded product and its rounded product with thr_c >=
//     0 are each <= the pair's: P' <= P.
//   * Numerator.  nt' is the maximum of the 16 pairs' own nt, so nub' = fl(2
//     nt' + E) >= fl(2 nt + E) = nub >= 0 (one fmaf each, monotone; E >= 0).
//   * Hence nub'^2 - P' >= nub^2 - P exactly, and t1' = fl(nub'^2 - P') >=
//     fl(nub^2 - P) = t1 (one rounding of a monotone exact value): t1' <= 0
//     implies t1 <= 0.  No slack term anywhere.
// A NaN (there is none: every input is finite and far from overflow) would
// fail both comparisons and send the lane to the full test.
// tests/cpp/f6_quick_check.cpp checks the implication and the nt bits on lanes
// built from small alignments.
struct F6qAcc {  // a lane's maxima over a row block's 16 pairs (all >= 0)
    float dmax = 0.0f, pmax = 0.0f, nt = 0.0f;
};
struct F6qRowMin {  // minima over the lane's 4 row sites
    float c1, rA2, rA;
};
struct F6qColMin {  // minima over the lane's 4 column sites
    float cB2, cB3, c4;
};
// (start from INFINITY; one row site at a time)
__host__ __device__ __forceinline__ void f6q_row_min(F6qRowMin &m, const F6tRow &a) {
    m.c1 = fminf(m.c1, a.c1);
    m.rA2 = fminf(m.rA2, a.rA2);
    m.rA = fminf(m.rA, a.rA);
}
__host__ __device__ __forceinline__ F6qColMin f6q_col_min(const F6tCol (&b)[4]) {
    return F6qColMin{fminf(fminf(b[0].cB2, b[1].cB2), fminf(b[2].cB2, b[3].cB2)),
                     fminf(fminf(b[0].cB3, b[1].cB3), fminf(b[2].cB3, b[3].cB3)),
                     fminf(fminf(b[0].c4, b[1].c4), fminf(b[2].c4, b[3].c4))};
}
// one pair into the lane's maxima; returns the pair's nt (r2_screen_terms_f6t's)
__host__ __device__ __forceinline__ float f6q_pair(float p, float s, float t, const F6tRow &a, const F6tCol &b,
                                                   F6qAcc &acc) {
    const float d = s - t;
    acc.dmax = fmaxf(acc.dmax, d);
    acc.pmax = fmaxf(acc.pmax, p);
    const float q = -((a.ma2 - s) * (b.mb - p));
    const float X0lo = p + (a.row + b.col);
    const float cap2 = fminf(fmaf(-2.0f, p, a.Ma2), b.Mb2 - d);
    const float nt = fmaxf(fabsf(fmaf(X0lo, t, q)), fabsf(fmaf(X0lo + cap2, t, q)));
    acc.nt = fmaxf(acc.nt, nt);
    return nt;
}
// t1' of the lane and row block, mlo its smallest primed marginal
__host__ __device__ __forceinline__ float f6q_lane_terms(const F6qAcc &acc, const F6qRowMin &a, const F6qColMin &b,
                                                         float thr_c, float E, float &mlo) {
    const float m1 = a.c1 - acc.dmax, m2 = a.rA2 + b.cB2;
    const float m3 = a.rA + b.cB3, m4 = fmaf(-2.0f, acc.pmax, b.c4);
    mlo = fminf(fminf(m1, m2), fminf(m3, m4));
    const float nub = fmaf(2.0f, acc.nt, E);
    return fmaf(nub, nub, -(thr_c * ((m1 * m2) * (m3 * m4))));
}
// (written so that a NaN does not skip)
__host__ __device__ __forceinline__ bool f6q_skip(float t1, float mlo, float mloc) { return t1 <= 0.0f && mlo >= mloc; }
// The quick test on a one-sided cap (f6q_pair1; round 15).  f6q_pair bounds
// P00 by cap2 = min(2 M_a - 2 p, 2 M_b - d); either side alone is an upper
// bound of 2 P00 too, and the row side's makes the interval's upper end
//   X0lo + (2 M_a - 2 p) = ((row + col) + 2 M_a) - p = cW - p,  cW = col + 2 W6
// (row + 2 M_a = 2 (W6 - M_a) + 2 M_a = 2 W6: every value on the 1/16 grid
// below 2^20, exact however it is associated), a term of the column site alone.
// The upper end n(X) = fl(X t - q) is nondecreasing in X (t >= 0, one fmaf), and
// cW - p >= X0lo + cap2, so the pair's nt' = max(|n(X0lo)|, |n(cW - p)|) >= its
// nt: the proof above goes through with nt' for nt, and no slack term is
// needed.  d is still formed for dmax.  On the synth sample with C4's
// constants 54 of 1,984 row blocks fall through where f6q_pair leaves 32
// (tests/cpp/f6_quick_units_check.cpp).
// kTwice: ap is 2 p (the shared image's count of 2 C01, count units below)
// and the halving rides in the three fmaf, each of which rounds a value that
// is exact; acc.pmax is then kept in ap's units (f6q_pmax).
template <bool kTwice>
__host__ __device__ __forceinline__ float f6q_pair1(float ap, float s, float t, float ma2, float row, float mb,
                                                    float col, float cW, F6qAcc &acc) {
    const float d = s - t;
    acc.dmax = fmaxf(acc.dmax, d);
    acc.pmax = fmaxf(acc.pmax, ap);
    const float rc = row + col;
    const float y0 = kTwice ? fmaf(-0.5f, ap, mb) : mb - ap;
    const float lo = kTwice ? fmaf(0.5f, ap, rc) : ap + rc;
    const float hi = kTwice ? fmaf(-0.5f, ap, cW) : cW - ap;
    const float q = -((ma2 - s) * y0);
    const float nt = fmaxf(fabsf(fmaf(lo, t, q)), fabsf(fmaf(hi, t, q)));
    acc.nt = fmaxf(acc.nt, nt);
    return nt;
}
// the lane's pmax for f6q_lane_terms from f6q_pair1's
template <bool kTwice>
__host__ __device__ __forceinline__ void f6q_pmax(F6qAcc &acc) {
    if (kTwice) acc.pmax *= 0.5f;
}
// Per-load site records (pair_mfma.hip fp6_records_kernel; round 15): what
// f6t_row and f6t_col return depends on the load alone (W6, R, the site's
// marginals), so it is formed once per load, by those very functions, and the
// tile-pair kernel's epilogue reads it where every wave of every entry formed
// it anew.  A row site's record is its F6tRow; a column site's its F6tCol with
// cW = col + 2 W6 (f6q_pair1); the quick test's lane minima (f6q_row_min over
// an aligned group of 4 sites, f6q_col_min over a tile's 4 sites of equal index
// mod 16: both groupings are the kernel's, fixed per load) are records of
// their own.  M = Ma2 / 2 and m = ma2 / 2 are exact, so f6c_rebuild reads
// the same records.
// Count units (inv = 1 / wv; the shared image of a load whose one weight
// value wv is a power of two, 0.125 ... 4): every field is stored times inv,
// and the quick test and the three-sum test take the shared image's counts as
// they are (2 C01, 2 C10 + C11, C11), E / wv^2 and mloc / wv, where the scaled
// path multiplies each count by wv first.  Every operation of f6q_pair,
// f6q_pair1, f6q_lane_terms and r2_screen_terms_f6t is a sum, difference,
// product, fmaf, minimum, maximum or absolute value of values each of which
// scales by a fixed power of wv (the site terms, sums, d, p, the marginals and
// mloc by wv; q, nt, nub and E by wv^2; the marginals' pair products by wv^2,
// the product of the four by wv^4; thr_c by 1; t1 by wv^4), and scaling by a
// power of two commutes with IEEE rounding where nothing under- or overflows:
// magnitudes lie below 2^80 8^4, and the nonzero sums, marginals and their
// products above 2^-16 8^-4.  (thr_c P alone can be smaller, under a tiny
// threshold; but a skip needs thr_c P >= nub^2 >= E^2 > 2^-60 8^-4, so where
// it could round differently both paths have t1 > 0.)  So the count-unit t1 is
// the scaled path's times wv^-4 and mlo - mloc its difference times 1 / wv,
// bit for bit wherever the sign is in question: every verdict is the same.
// Other weight values keep the scaled path (inv = 1).
struct alignas(8) F6RowRec {
    F6tRow a;
};
struct alignas(16) F6ColRec {
    F6tCol b;
    float cW, pad;
};
struct alignas(16) F6MinRec {  // row group: c1, rA2, rA; column group: cB2, cB3, c4
    float x, y, z, pad;
};
__host__ __device__ __forceinline__ F6RowRec f6_row_rec(float W6, float Ma, float ma, float R2, float inv) {
    const F6tRow a = f6t_row(W6, Ma, ma, R2);
    return F6RowRec{{a.rA * inv, a.rA2 * inv, a.c1 * inv, a.Ma2 * inv, a.ma2 * inv, a.row * inv}};
}
__host__ __device__ __forceinline__ F6ColRec f6_col_rec(float W6, float Mb, float mb, float R2, float inv) {
    const F6tCol b = f6t_col(Mb, mb, R2);
    return F6ColRec{{b.cB2 * inv, b.cB3 * inv, b.c4 * inv, b.Mb2 * inv, b.mb * inv, b.col * inv},
                    fmaf(2.0f, W6, b.col) * inv, 0.0f};
}
__host__ __device__ __forceinline__ F6MinRec f6_row_min_rec(const F6RowRec (&r)[4]) {
    F6qRowMin m{INFINITY, INFINITY, INFINITY};
    for (int e = 0; e < 4; ++e) f6q_row_min(m, r[e].a);
    return F6MinRec{m.c1, m.rA2, m.rA, 0.0f};
}
__host__ __device__ __forceinline__ F6MinRec f6_col_min_rec(const F6ColRec (&c)[4]) {
    const F6tCol b[4] = {c[0].b, c[1].b, c[2].b, c[3].b};
    const F6qColMin m = f6q_col_min(b);
    return F6MinRec{m.cB2, m.cB3, m.c4, 0.0f};
}
__host__ __device__ __forceinline__ float r2_screen_violation(float T, float A, float B, float AB, float R,
                                                              float thr_c) {
    float E, mloc, t2;
    screen_consts(T, R, E, mloc);
    const float t1 = r2_screen_terms(T, A, B, AB, R, thr_c, E, mloc, t2);
    return fmaxf(t1, t2);
}
__host__ __device__ __forceinline__ bool r2_screen_skip_f32(float T, float A, float B, float AB, float R, float thr) {
    return r2_screen_violation(T, A, B, AB, R, thr * (1.0f - 0x1p-7f)) <= 0.0f;
}
// largest |top-plane sum| for which the screen may use r2_screen_skip_f32
constexpr uint32_t kScreenF32MaxNP = 32768;  // 128 NP <= 2^22

// One full-wave LDS-DMA (global_load_lds_dwordx4): each lane copies 16 bytes
// from gsrc to LDS byte address lds_dst + 16*lane (lds_dst wave-uniform).  Issued
// as inline asm so that the compiler's wait-count bookkeeping does not see it
// (it would otherwise wait for every in-flight copy before any LDS read of the
// other buffer): completion is ordered only by the kernel's own protocol —
// s_waitcnt vmcnt(0) by every issuing wave, then a barrier, then the reads.
// M0 is saved and restored inside the statement (it is compiler-reserved).
__device__ __forceinline__ void glds16(const void *gsrc, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gsrc), "s"(lds_dst)
        : "memory");
}

// The same copy addressed as SGPR base + per-lane 32-bit VGPR offset (no
// 64-bit per-lane address arithmetic).
__device__ __forceinline__ void glds16_s(const void *sbase, uint32_t voff, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(sbase), "s"(lds_dst)
        : "memory");
}

// ... and one dword per lane (64 lanes: 256 bytes to lds_dst + 4*lane)
__device__ __forceinline__ void glds4_s(const void *sbase, uint32_t voff, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dword %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(sbase), "s"(lds_dst)
        : "memory");
}

__device__ __forceinline__ uint32_t lds_addr(const void *p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}

// A tile (or part of one) of the run is finished (one thread of its
// workgroup): with per-chunk progress on, the workgroup that finishes its
// chunk's last tile appends the chunk's pair count to the host log (the value
// lib.rs's per-chunk fetch_add adds, lib.rs:670-671; the host sums the log in
// slot order).  A chunk counts kTileQuarters per tile (progress_init_kernel):
// a work item that finishes q of a tile's four 16-row blocks counts q.
constexpr uint32_t kTileQuarters = 4;
__device__ __forceinline__ void tile_done(const OrderArgs &o, uint32_t ta, uint32_t tb, uint32_t n_chunk_rows,
                                          uint32_t quarters = kTileQuarters) {
    if (!o.chunk_left) return;
    const uint32_t row = ta / kTilesPerChunk, col = tb / kTilesPerChunk;
    const uint32_t lin = chunk_linear(n_chunk_rows, row, col);
    if (atomicSub(&o.chunk_left[lin], quarters) == quarters) {
        const unsigned slot = atomicAdd(o.prog_n, 1u);
        // (under a window: the chunk's in-window pairs)
        const unsigned long long pairs = o.win_pairs ? o.win_pairs[lin] : chunk_pairs(o.L, row, col);
        __hip_atomic_store(&o.prog_log[slot], pairs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        uint32_t t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// The run's chunk scan (ScanArgs) by one workgroup of any size that is a
// multiple of 64, up to 1024: each thread sums a contiguous run of chunk
// totals, a wave scan and a scan of the wave totals give its base.  The
// counters and totals it reads were last written by other workgroups'
// agent-scope atomics in this launch (scan_tail): every load of them is an
// agent-scope (sc1) load, served past this CU's L1.
__device__ inline void chunk_scan_block(const ScanArgs &a) {
    __shared__ unsigned long long sw[16];
    auto ld32 = [](const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    const uint32_t tid = threadIdx.x, nth = blockDim.x;
    const uint32_t per = (a.count + nth - 1) / nth;
    const uint32_t lo = min(a.count, tid * per), hi = min(a.count, lo + per);
    uint32_t *ct = a.chunk_total + a.lin_begin;
    // up to kScanRegs totals per thread (every run up to 16 x 256 chunks on a
    // 256-thread workgroup) are loaded at once, all in flight together, and
    // kept in registers for the second pass; longer runs loop
    constexpr uint32_t kScanRegs = 16;
    const bool in_regs = per <= kScanRegs;
    uint32_t vals[kScanRegs];
    unsigned long long s = 0;
    if (in_regs) {
#pragma unroll
        for (uint32_t j = 0; j < kScanRegs; ++j) vals[j] = lo + j < hi ? ld32(ct + lo + j) : 0u;
#pragma unroll
        for (uint32_t j = 0; j < kScanRegs; ++j) s += vals[j];
    } else {
        for (uint32_t i = lo; i < hi; ++i) s += ld32(ct + i);
    }
    const int lane = tid & 63, wv = tid >> 6;
    unsigned long long v = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    if (lane == 63) sw[wv] = v;
    __syncthreads();
    if (tid == 0) {
        unsigned long long run = 0;
        for (uint32_t k = 0; k < nth / 64; ++k) {
            const unsigned long long t = sw[k];
            sw[k] = run;
            run += t;
        }
        *a.total = run;
        if (a.count_out) *a.count_out = run;  // e.g. the caller's tensor for the RCCL count exchange
        const unsigned long long cur = __hip_atomic_load(a.cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *a.cursor = 0;
        unsigned cand = 0, blocks = 0;
        if (a.cand_count) {
            cand = ld32(a.cand_count);
            blocks = ld32(a.cand_count + 1);
        }
        // (an abandoned pass's rows are not gathered: the host re-runs it)
        if (a.cursor_seen) *a.cursor_seen = (cand & kAbandonBit) ? ~0ull : cur;
        // the next pass's candidate set starts at 0 (nothing in this launch
        // reads or writes it)
        if (a.cand_reset) a.cand_reset[0] = a.cand_reset[1] = 0;
        if (a.cand_buckets_reset)
            for (int b = 0; b < 16; ++b) a.cand_buckets_reset[b] = 0;
        if (a.host_out) {
            a.host_out[0] = cur;
            a.host_out[1] = run;
            a.host_out[2] = cand;
            a.host_out[3] = blocks;
            if (a.rechecked)  // ([4]: the guard word)
                a.host_out[5] = (unsigned long long)ld32(a.rechecked) | (unsigned long long)ld32(a.rechecked + 1) << 32;
            __threadfence_system();
        }
        // (every screen workgroup that counted has finished: the scan runs
        // in a launch behind the screen's)
        if (a.rechecked) a.rechecked[0] = a.rechecked[1] = 0;
    }
    __syncthreads();
    unsigned long long base = sw[wv] + v - s;
    if (in_regs) {
#pragma unroll
        for (uint32_t j = 0; j < kScanRegs; ++j)
            if (lo + j < hi) {
                ct[lo + j] = 0;
                a.chunk_base[lo + j] = (uint32_t)base;
                base += vals[j];
            }
        return;
    }
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t t = ld32(ct + i);
        ct[i] = 0;
        a.chunk_base[i] = (uint32_t)base;
        base += t;
    }
}

// The screen's candidate list in 16 buckets of capacity cap by computed 16x16
// sub-blocks (a tile with c of them in bucket 16 - c: the heaviest first, so
// the workgroups dealt round-robin over the CUs each get a mix and the list's
// light tail goes to whichever finish first); entry (b, k) at b cap + k of the
// tile and bit arrays.  The launch maps its u-th tile through the buckets'
// prefix sums, which cand_prefix puts in s_pre[17] (every thread calls it).
// An abandoned screen (kAbandonBit on bucket 0) leaves no candidate.
__device__ inline void cand_prefix(const unsigned *buckets, uint32_t *s_pre) {
    if (threadIdx.x == 0) {
        const bool abandoned = buckets[0] & kAbandonBit;
        uint32_t run = 0;
        for (int b = 0; b < 16; ++b) {
            s_pre[b] = run;
            run += abandoned ? 0u : buckets[b];
        }
        s_pre[16] = run;
    }
    __syncthreads();
}
__device__ inline uint32_t cand_entry(const uint32_t *s_pre, uint32_t cap, uint32_t u) {
    uint32_t b = 0;
    while (b < 15 && s_pre[b + 1] <= u) ++b;
    return b * cap + (u - s_pre[b]);
}
// ... guarded: ~0u (and kGuardEntry reported) unless the u-th candidate lies
// inside the buckets the screen filled (u below their total, its bucket slot
// below the capacity)
__device__ inline uint32_t cand_entry_checked(const OrderArgs &o, const uint32_t *s_pre, uint32_t cap, uint32_t u) {
    uint32_t b = 0;
    while (b < 15 && s_pre[b + 1] <= u) ++b;
    if (u >= s_pre[16] || u - s_pre[b] >= cap) {
        report_guard(o, kGuardEntry);
        return ~0u;
    }
    return b * cap + (u - s_pre[b]);
}

// The end of every workgroup of a candidate launch (a grid-stride loop over
// the screen's n_work candidate tiles).  With the scan fused (a.ticket set)
// the workgroups that computed a tile take a ticket and the last one runs the
// run's chunk scan (with no candidate, workgroup 0 alone): one launch (and
// its dispatch gap) less per run, and no ticket traffic in the common case.
// What the scan reads from this launch — the chunk totals and the staging
// cursor — is written only by agent-scope atomics (lane 63's in the
// compaction; an atomic leaves no copy of its line in the issuing XCD's L2).
// Each writing wave waits for its atomics (s_waitcnt vmcnt(0)) before lane 0
// takes the ticket; the winner then runs an agent-scope ACQUIRE (buffer_inv
// sc1: no line of the run state cached in its CU's L1 or its XCD's L2
// survives) before the scan's agent-scope loads (MI355X_MICROARCH.md,
// inter-workgroup visibility).  The acquire is the last workgroup's alone;
// no workgroup pays an L2 write-back.  WLD_OPT_FUSED_SCAN 0 runs the scan as
// a launch of its own instead (the kernel boundary orders everything).
// The screen before the launch only appended candidates (atomics, before the
// kernel boundary).
// (all_waves: every wave wrote what the scan reads, and drains before the ticket)
// first: the workgroup's first work item (a permutation of the grid's ids:
// the workgroups that computed anything are exactly those with first < p).
__device__ inline void scan_tail(const ScanArgs &a, uint32_t n_work, bool all_waves = false,
                                 uint32_t first = blockIdx.x) {
    if (!a.ticket) return;
    const uint32_t p = min(gridDim.x, n_work);  // workgroups that computed a tile
    if (first >= max(p, 1u)) return;
    __shared__ unsigned s_run;
    if (all_waves || threadIdx.x < 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // atomics performed
    // every wave has drained (waves that work independently may still be
    // writing when wave 0 arrives) before the workgroup takes its ticket
    if (all_waves) __syncthreads();
    if (threadIdx.x == 0) {
        s_run = p <= 1 || atomicAdd(a.ticket, 1u) == p - 1;
        if (s_run) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the invalidate completed before the barrier
        }
    }
    __syncthreads();
    if (!s_run) return;
    if (threadIdx.x == 0 && p > 1) atomicExch(a.ticket, 0u);
    chunk_scan_block(a);
}

}  // namespace wld
