// The dense LD matrix (wld_run_matrix_device / wld_run_matrix): every in-window
// pair's d, d', r2 exactly as the default row path computes them —
// pair_valu_kernel<MF, REF>'s operands, lane-class chains, ordered horizontal
// sum, scalar tail and ld_epilogue, instantiated from the one template in
// pair_valu_kernel.hpp — stored into a caller's matrix instead of compacted
// into rows.  Pair (a, b), a < b, is evaluated once, by its tile; entries
// (a, b) and (b, a) both receive its value, so the matrix is symmetric bit for
// bit.  Nothing is reduced but the four class counts (one u64 atomic per class
// and tile); no matrix value goes through an atomic.
//
// The epilogue.  After the sums, wave w's lane (r, g) holds tot[i][j] of the
// pairs (a = a0 + 16 w + 4 g + i, b = b0 + 16 j + r), i, j = 0..3.  The lane
// picks the stat — r = -+sqrt(r2) with the sign of -d, the square root the
// correctly rounded f32 one (taken in f64 and rounded once more: exact for a
// 24-bit result) — applies the rules (a pair out of the range a < b < L or out
// of the window: +0.0; a none pair: NaN; WLD_MATRIX_ZERO_MISSING: NaN and
// +-inf to +0.0) and puts the value at [a - a0][b - b0] of a 64x64 f32 matrix in
// LDS (row stride 65).  The classes of the pairs the launch counts
// (matrix_plan::counts_here) are counted with wave ballots.  Then the tile's
// images that meet the band (matrix_plan::images) are stored: the direct one
// reads the LDS matrix by rows, the mirrored one by columns (stride 65: no
// bank conflict), so in either a wave's 64 lanes store 64 consecutive elements
// of one destination row; every store is clipped to the band.  A diagonal
// tile stores its block once: the LDS matrix above the diagonal, its
// transpose below, the diagonal rule on it.
#include "pair_valu_kernel.hpp"

namespace wld {

namespace {
constexpr int kVStride = 65;  // floats per row of the staged tile

// the value of entry (u, u): r2 and r are 1 where the site has a major and a
// minor symbol; d and d' have none
__device__ __forceinline__ float matrix_diag(const MatrixArgs &m, const uint8_t *site_ok, uint32_t u) {
    if (m.stat == matrix_plan::kStatR2 || m.stat == matrix_plan::kStatR)
        return (m.zero_missing || site_ok[u]) ? 1.0f : __builtin_nanf("");
    return m.zero_missing ? 0.0f : __builtin_nanf("");
}
// entry (u, v) of the band := x (u, v inside the band)
__device__ __forceinline__ void matrix_store(const MatrixArgs &m, uint32_t u, uint32_t v, float x) {
    const size_t k = (size_t)(u - m.band.r0) * m.ld + (v - m.band.c0);
    if (m.f16) {
        const _Float16 h = (_Float16)x;  // round to nearest even, subnormals kept
        reinterpret_cast<_Float16 *>(m.dst)[k] = h;
    } else {
        reinterpret_cast<float *>(m.dst)[k] = x;
    }
}
__device__ __forceinline__ bool in_band(const MatrixArgs &m, uint32_t u, uint32_t v) {
    return u >= m.band.r0 && u < m.band.r1 && v >= m.band.c0 && v < m.band.c1;
}
}  // namespace

__device__ __attribute__((always_inline)) void matrix_epilogue(const MatrixArgs &m, const OrderArgs &o,
                                                               const uint8_t *site_ok, uint32_t L, uint32_t a0,
                                                               uint32_t b0, uint32_t tid,
                                                               const float (&tot)[4][4][4]) {
    __shared__ float sV[kTile * kVStride];
    __shared__ uint32_t sCls[4];  // pairs, none, nonfinite, counted of the tile
    const uint32_t lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
    const uint32_t ar = a0 + 16 * wave + 4 * g;  // this lane's a rows ar + i; its b columns b0 + 16 j + r
    if (tid < 4) sCls[tid] = 0;

    // which of the lane's 16 pairs are in the range (bit 4 i + j), which of
    // them this launch counts, and the site flags: every load issued before
    // the sums' epilogue (a, b < LP: nothing is read past an array)
    uint32_t inr = 0, cnt = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t a = ar + i, b = b0 + 16 * j + r;
            if ((a < b) & (b < L) & in_window(o, a, b)) {
                inr |= 1u << (4 * i + j);
                if (matrix_plan::counts_here(m.full, m.band, a, b)) cnt |= 1u << (4 * i + j);
            }
        }
    const uint32_t okA4 = *reinterpret_cast<const uint32_t *>(site_ok + ar);
    uint32_t okB = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) okB |= site_ok[b0 + 16 * j + r] ? 1u << j : 0u;
    __syncthreads();  // the class counts are zero

    uint32_t n_pairs = 0, n_none = 0, n_nonfin = 0, n_counted = 0;  // of the wave (uniform)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float d, dp, r2;
            ld_epilogue(tot[i][j][0], tot[i][j][1], tot[i][j][2], tot[i][j][3], d, dp, r2);
            const bool in = (inr >> (4 * i + j)) & 1u, c = (cnt >> (4 * i + j)) & 1u;
            const bool some = ((okA4 >> (8 * i)) & 0xFFu) && ((okB >> j) & 1u);
            const bool finite = fabsf(r2) <= 3.4028235e38f;  // (false for NaN)
            n_pairs += (uint32_t)__popcll(__ballot(c));
            n_none += (uint32_t)__popcll(__ballot(c && !some));
            n_nonfin += (uint32_t)__popcll(__ballot(c && some && !finite));
            n_counted += (uint32_t)__popcll(__ballot(c && some && finite));
            float x;
            if (m.stat == matrix_plan::kStatR) {  // (uniform)
                const float s = (float)__builtin_sqrt((double)r2);
                x = d > 0.0f ? -s : s;
            } else {
                x = m.stat == matrix_plan::kStatR2 ? r2 : m.stat == matrix_plan::kStatD ? d : dp;
            }
            if (!some) x = __builtin_nanf("");
            if (m.zero_missing && !(fabsf(x) <= 3.4028235e38f)) x = 0.0f;
            if (!in) x = 0.0f;
            sV[(16 * wave + 4 * g + i) * kVStride + 16 * j + r] = x;
        }
    }
    if (lane == 0) {
        if (n_pairs) atomicAdd(&sCls[0], n_pairs);
        if (n_none) atomicAdd(&sCls[1], n_none);
        if (n_nonfin) atomicAdd(&sCls[2], n_nonfin);
        if (n_counted) atomicAdd(&sCls[3], n_counted);
    }
    __syncthreads();  // the staged tile and the class counts are complete
    if (tid < 4 && sCls[tid]) atomicAdd(&m.counts[tid], (unsigned long long)sCls[tid]);

    // the stores: wave w takes the image's rows w, w + 4, ...; lane = column
    const uint32_t img = matrix_plan::images(m.band, a0 / kTile, b0 / kTile);  // (uniform)
    if (a0 == b0) {
        if (!img) return;
#pragma unroll 4
        for (uint32_t row = wave; row < (uint32_t)kTile; row += 4) {
            const uint32_t u = a0 + row, v = a0 + lane;
            if (!in_band(m, u, v)) continue;  // (inside the band: u, v < L)
            const float x = row < lane ? sV[row * kVStride + lane]
                                       : row > lane ? sV[lane * kVStride + row] : matrix_diag(m, site_ok, u);
            matrix_store(m, u, v, x);
        }
        return;
    }
    if (img & matrix_plan::kDirect) {
#pragma unroll 4
        for (uint32_t row = wave; row < (uint32_t)kTile; row += 4) {
            const uint32_t u = a0 + row, v = b0 + lane;
            if (in_band(m, u, v)) matrix_store(m, u, v, sV[row * kVStride + lane]);
        }
    }
    if (img & matrix_plan::kMirror) {
#pragma unroll 4
        for (uint32_t row = wave; row < (uint32_t)kTile; row += 4) {
            const uint32_t u = b0 + row, v = a0 + lane;
            if (in_band(m, u, v)) matrix_store(m, u, v, sV[lane * kVStride + row]);
        }
    }
}

// the blocks of the band no listed tile covers: one workgroup per block
__global__ __launch_bounds__(256) void matrix_fill_kernel(const uint32_t *__restrict__ blocks,
                                                          const uint8_t *__restrict__ site_ok, MatrixArgs m) {
    const uint32_t e = blocks[blockIdx.x], bi = e >> 16, bj = e & 0xFFFFu;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t row = wave; row < (uint32_t)kTile; row += 4) {
        const uint32_t u = bi * kTile + row, v = bj * kTile + lane;
        if (in_band(m, u, v)) matrix_store(m, u, v, u == v ? matrix_diag(m, site_ok, u) : 0.0f);
    }
}

void launch_pair_matrix(const ValuLaunch &v, const OrderArgs &o, const MatrixArgs &m, hipStream_t st) {
    if (!v.n_tiles) return;
    // one whole-tile workgroup per listed tile at every list size, as the
    // summary launches: a tile's two images come from one staged copy
    hipLaunchKernelGGL((pair_valu_kernel<false, false, true, true, false, kReduceMatrix>), dim3(v.n_tiles), dim3(256),
                       0, st, v.codes, v.w, v.site_ok, v.tiles, v.n_tiles, (const unsigned *)nullptr,
                       (const uint32_t *)nullptr, (unsigned *)nullptr, (const unsigned *)nullptr, 0u, v.L, v.NP, 1u,
                       v.ref_cls / 64, v.ref_tail_n, v.n_chunk_rows, 0.0f, o, m, ScanArgs{});
}

void launch_matrix_fill(const uint32_t *blocks, uint32_t n_blocks, const uint8_t *site_ok, const MatrixArgs &m,
                        hipStream_t st) {
    if (!n_blocks) return;
    hipLaunchKernelGGL(matrix_fill_kernel, dim3(n_blocks), dim3(256), 0, st, blocks, site_ok, m);
}

}  // namespace wld
