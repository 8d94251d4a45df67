// The fp6 screen's operand packing for one lane (pair_mfma.hip frag6_kernel,
// frag6_shared_kernel; tests/cpp/f6_a4_check.cpp and f6_shared_check.cpp run
// the same code on the host): a lane of the
// MFMA's 16 x 128 operand holds one site's 32 consecutive sequences, sequence j
// at bits 6 j of six dwords (e2m3, the fp6 A image) or at bits 4 j of four
// (e2m1: the B image, and the fp4 A image of a load whose weight codes all fit
// e2m1, fp6_scale.hpp fp6_codes_fit_fp4).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define WLD_HD __host__ __device__
#else
#define WLD_HD
#endif

namespace wld {

// the symbol codes' bits (kernels.hpp kCodeIn, kCodeMaj): 0 missing, 1 minor, 3 major
constexpr uint32_t kF6SymIn = 1, kF6SymMaj = 2;

// One lane's operand dwords.  A: ai the missing channel (w [symbol missing]),
// am the minor channel (w [symbol minor]); kA4 false: wa holds e2m3 codes, six
// dwords each; true: e2m1 codes, four dwords each (dwords 4-5 stay 0).  b: the
// B nibbles, 4 (2.0) missing, 2 (1.0) minor, 0 major.  sym / wa: the lane's 32
// sequences, of which the first n exist (n <= 32; the rest, past the padded
// sequence count, are 0 in every operand).  A padded sequence inside n has
// symbol 0 and so reads as missing in A and in B: it weighs nothing only
// because its weight code is 0.
template <bool kA4>
WLD_HD inline void f6_pack_lane(const uint8_t *sym, const uint8_t *wa, uint32_t n, uint32_t (&ai)[6], uint32_t (&am)[6],
                                uint32_t (&b)[4]) {
    for (int d = 0; d < 6; ++d) ai[d] = am[d] = 0u;
    for (int d = 0; d < 4; ++d) b[d] = 0u;
    for (uint32_t j = 0; j < 32; ++j) {
        const uint32_t c = j < n ? sym[j] : 0u, v = j < n ? wa[j] : 0u;
        const uint32_t vi = (c & kF6SymIn) ? 0u : v, vm = (c & (kF6SymIn | kF6SymMaj)) == kF6SymIn ? v : 0u;
        if (kA4) {
            ai[j >> 3] |= vi << (4 * (j & 7));
            am[j >> 3] |= vm << (4 * (j & 7));
        } else {
            const uint32_t bit = 6 * j, d = bit >> 5, o = bit & 31;
            ai[d] |= vi << o;
            am[d] |= vm << o;
            if (o > 26) {
                ai[d + 1] |= vi >> (32 - o);
                am[d + 1] |= vm >> (32 - o);
            }
        }
        if (j < n) b[j >> 3] |= ((c & kF6SymIn) ? ((c & kF6SymMaj) ? 0u : 2u) : 4u) << (4 * (j & 7));
    }
}

// The shared image's lane (a load whose weight codes are all one code,
// fp6_scale.hpp fp6_shared_code): the B nibbles alone, which the kernels read
// for both operands.  n counts the lane's real sequences (below N, not NP): a
// padded sequence is coded 0 here, not missing, because no A image's zero
// weight nulls it; with 0 it adds to none of the four products from either
// side.  The row tile's A channels are two masks of these dwords: missing at
// 2.0 (0x4 nibbles), minor at 1.0 (0x2 nibbles, the mask the B side applies).
constexpr uint32_t kF6MaskMissing = 0x44444444u, kF6MaskMinor = 0x22222222u;
WLD_HD inline void f6_pack_lane_shared(const uint8_t *sym, uint32_t n, uint32_t (&b)[4]) {
    for (int d = 0; d < 4; ++d) b[d] = 0u;
    for (uint32_t j = 0; j < n && j < 32; ++j) {
        const uint32_t c = sym[j];
        b[j >> 3] |= ((c & kF6SymIn) ? ((c & kF6SymMaj) ? 0u : 2u) : 4u) << (4 * (j & 7));
    }
}

// sequence j's code of a lane's operand dwords, as the MFMA reads them
WLD_HD inline uint32_t f6_lane_code6(const uint32_t (&d)[6], uint32_t j) {
    const uint32_t bit = 6 * j, i = bit >> 5, o = bit & 31;
    uint32_t v = d[i] >> o;
    if (o > 26) v |= d[i + 1] << (32 - o);
    return v & 63u;
}
WLD_HD inline uint32_t f6_lane_code4(const uint32_t *d, uint32_t j) { return d[j >> 3] >> (4 * (j & 7)) & 15u; }

}  // namespace wld
