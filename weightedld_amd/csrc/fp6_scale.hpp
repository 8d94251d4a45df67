// The fp6 screen's weight codes (host only): the e2m3 encoding and the choice
// of the common scale S at which the weights are rounded to it (capi.hip
// fp6_prepare; tests/cpp/f6_complement_check.cpp runs the same code).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace wld {

// e2m3 (fp6) encoding of a value in [0, 7.5] rounded to the nearest grid
// point, ties to the even code: sign 0, exponent bias 1, 3 mantissa bits.
// The grid steps by 1/8 below 2, by 1/4 in [2, 4) and by 1/2 from 4; within
// each the code's parity is the grid index's, so round-half-even on the index
// (nearbyint) is ties-to-even on the code (an index rounding up to the next
// binade's first point lands on its even code, m = 0).
inline uint32_t fp6_code(double x, double *rounded) {
    x = std::min(std::max(x, 0.0), 7.5);
    const double step = x < 2.0 ? 0.125 : x < 4.0 ? 0.25 : 0.5;
    const double v = std::min(std::nearbyint(x / step) * step, 7.5);
    *rounded = v;
    if (v < 1.0) return (uint32_t)(v * 8.0);                             // e = 0 (subnormal), m = 8v
    if (v < 2.0) return 8u + (uint32_t)((v - 1.0) * 8.0);                // e = 1
    if (v < 4.0) return 16u + (uint32_t)((v * 0.5 - 1.0) * 8.0);         // e = 2
    return 24u + (uint32_t)((v * 0.25 - 1.0) * 8.0);                     // e = 3
}

// One candidate scale's L1 rounding residual in the weights' own units
// (sum_k |S w_k - w6_k| / S) and the set mantissa bits of its N codes.
struct Fp6ScaleCost {
    double S, resid;
    uint64_t mant_bits;
};
inline Fp6ScaleCost fp6_scale_cost(const float *w, size_t N, double S) {
    double r = 0.0, v;
    uint64_t bits = 0;
    for (size_t k = 0; k < N; ++k) {
        const uint32_t c = fp6_code(S * (double)w[k], &v) & 7u;
        r += std::fabs(S * (double)w[k] - v);
        bits += (c & 1u) + (c >> 1 & 1u) + (c >> 2);
    }
    return {S, r / S, bits};
}
// The candidates: 51 scales that put the largest weight on [3.75, 7.5] (one
// binade of the grid, 1% apart), and the scales that put the weights' median
// on an e2m3 value whose mantissa is all zero (1, 2, 4) or one bit (1.5, 3,
// 6), where the largest weight stays within 7.5.
inline std::vector<double> fp6_scale_candidates(const float *w, size_t N, double wmax) {
    std::vector<double> S;
    for (int f = 0; f <= 50; ++f) S.push_back(7.5 * (0.5 + 0.01 * f) / wmax);
    std::vector<float> s(w, w + N);
    std::nth_element(s.begin(), s.begin() + N / 2, s.end());
    const double med = (double)s[N / 2];
    // (the larger value first: of equals the earlier wins, and R's 1/32 grid is finer against larger sums)
    for (double v : {4.0, 2.0, 1.0, 6.0, 3.0, 1.5})
        if (med > 0.0 && v / med * wmax <= 7.5) S.push_back(v / med);
    return S;
}
// The scale: among the candidates whose residual is within 1% of the smallest
// (a condition, not a measurement: it bounds how far the screen's R, and with
// it the candidate count, can move), the one whose codes have the fewest set
// mantissa bits, then the smaller residual, then the earlier candidate.  The
// operands' set bits cost energy in the matrix pipe, which limits the screen's
// clock; where the weights collapse onto one code (Henikoff
// weights of a large alignment, unit weights) the residual does not depend on
// which code that is, and 4.0 (mantissa 000) serves as well as 7.0 (110).
// w: N > 0 nonnegative finite weights, wmax > 0 their maximum.
inline Fp6ScaleCost fp6_choose_scale(const float *w, size_t N, double wmax) {
    std::vector<Fp6ScaleCost> c;
    for (double S : fp6_scale_candidates(w, N, wmax)) c.push_back(fp6_scale_cost(w, N, S));
    double rmin = INFINITY;
    for (const Fp6ScaleCost &x : c) rmin = std::min(rmin, x.resid);
    const Fp6ScaleCost *best = nullptr;
    for (const Fp6ScaleCost &x : c) {
        if (!(x.resid <= 1.01 * rmin)) continue;
        if (!best || x.mant_bits < best->mant_bits || (x.mant_bits == best->mant_bits && x.resid < best->resid))
            best = &x;
    }
    return *best;
}

// e2m3 codes whose value is also an e2m1 (fp4) value: mantissa bits 1-0 clear,
// that is 0, 4, 8, 12, 16, 20, 24, 28 for 0, 0.5, 1, 1.5, 2, 3, 4, 6.  Both
// formats have two exponent bits at bias 1, so the e2m1 code of the same
// value is the e2m3 code without those two bits.  -1: no e2m1 value.
inline int fp6_to_fp4_code(uint32_t c6) { return c6 < 32u && (c6 & 3u) == 0u ? (int)(c6 >> 2) : -1; }
// The value of an e2m3 / e2m1 code (sign 0).
inline double fp6_value(uint32_t c6) {
    const uint32_t e = c6 >> 3 & 3u, m = c6 & 7u;
    return e ? std::ldexp(1.0 + m / 8.0, (int)e - 1) : m / 8.0;
}
inline double fp4_value(uint32_t c4) {
    const uint32_t e = c4 >> 1 & 3u, m = c4 & 1u;
    return e ? std::ldexp(1.0 + m / 2.0, (int)e - 1) : m / 2.0;
}
// Whether a load's N weight codes all fit e2m1: its A image can then be fp4
// nibbles (pair_mfma.hip, WLD_OPT_FP6_A4), every product and sum unchanged.
inline bool fp6_codes_fit_fp4(const uint8_t *w6, size_t N) {
    for (size_t k = 0; k < N; ++k)
        if (fp6_to_fp4_code(w6[k]) < 0) return false;
    return true;
}
// The one nonzero e2m3 code that all N weight codes of a load share (unit
// weights, Henikoff weights of a large alignment: the scale rule puts either
// on 4.0), or 0 where they differ, one of them is 0, or N is 0.  With one
// weight value v the A image is a function of the B image: its channels are v
// [missing] and v [minor], B's nibbles 2.0 [missing] + 1.0 [minor], so two
// masks of the row tile's B image give them at the weights 2.0 and 1.0, and v
// enters the restored sums as a scale (pair_mfma.hip, WLD_OPT_FP6_SHARED;
// pair_common.hpp f6s_direct).  Any code serves, e2m1 value or not.
inline uint32_t fp6_shared_code(const uint8_t *w6, size_t N) {
    if (N == 0 || w6[0] == 0u || w6[0] >= 32u) return 0u;
    for (size_t k = 1; k < N; ++k)
        if (w6[k] != w6[0]) return 0u;
    return w6[0];
}

}  // namespace wld
