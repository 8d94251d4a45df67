// The banded LD matrix (wld_run_matrix_banded_device / wld_run_matrix_banded):
// the values of the dense matrix (pair_matrix.hip: pair_valu_kernel<MF, REF>'s
// operands, sums and ld_epilogue, the stat, the none / zero_missing / window
// rules and the class ballots of matrix_epilogue) stored once, into the upper
// band of a caller's banded matrix: element k of row u is entry (u, u + k).
// Pair (a, b), a < b, is evaluated once, by its tile, and stored once, in row a
// at k = b - a.  Nothing is reduced but the four class counts (one u64 atomic
// per class and tile); no matrix value goes through an atomic.
//
// The epilogue.  The lane's 16 values go to [a - a0][b - b0] of a 64x64 f32
// matrix in LDS (row stride 65) exactly as in matrix_epilogue; the pairs the
// launch counts are the in-window pairs whose row a lies in [r0, r1).  Then
// wave w stores the tile's rows w, w + 4, ...: the row of site u = a0 + row
// holds the columns b = b0 .. b0 + 63, which are the 64 consecutive elements
// k = b0 - u .. b0 - u + 63 of destination row u, clipped to 0 <= k <= K and to
// the rows [r0, r1): one contiguous run per row.  In the diagonal tile the
// lanes below the diagonal store nothing and the lane on it stores the
// diagonal rule's value at k = 0.  Columns b >= L of a listed tile hold +0.0
// (the range rule), so a listed tile writes its whole run.
#include "pair_valu_kernel.hpp"

namespace wld {

namespace {
constexpr int kVStride = 65;  // floats per row of the staged tile

// the value of entry (u, u): r2 and r are 1 where the site has a major and a
// minor symbol; d and d' have none
__device__ __forceinline__ float banded_diag(const MatrixBandedArgs &m, const uint8_t *site_ok, uint32_t u) {
    if (m.stat == matrix_plan::kStatR2 || m.stat == matrix_plan::kStatR)
        return (m.zero_missing || site_ok[u]) ? 1.0f : __builtin_nanf("");
    return m.zero_missing ? 0.0f : __builtin_nanf("");
}
// element k of row u := x (r0 <= u < r1, k <= K)
__device__ __forceinline__ void banded_store(const MatrixBandedArgs &m, uint32_t u, uint32_t k, float x) {
    const size_t e = (size_t)(u - m.r0) * m.ld + k;
    if (m.f16) {
        const _Float16 h = (_Float16)x;  // round to nearest even, subnormals kept
        reinterpret_cast<_Float16 *>(m.dst)[e] = h;
    } else {
        reinterpret_cast<float *>(m.dst)[e] = x;
    }
}
}  // namespace

__device__ __attribute__((always_inline)) void matrix_banded_epilogue(const MatrixBandedArgs &m, const OrderArgs &o,
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
                if (a >= m.r0 && a < m.r1) cnt |= 1u << (4 * i + j);
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

    // the stores: wave w takes the tile's rows w, w + 4, ...; lane = column
    const bool diag = a0 == b0;  // (uniform)
#pragma unroll 4
    for (uint32_t row = wave; row < (uint32_t)kTile; row += 4) {
        const uint32_t u = a0 + row;
        if (u < m.r0 || u >= m.r1) continue;  // (uniform; inside the rows: u < L)
        if (diag && lane < row) continue;     // below the diagonal: another row's pair
        const uint32_t k = b0 + lane - u;     // (b0 + lane >= u here)
        if (k > m.K) continue;
        banded_store(m, u, k, diag && lane == row ? banded_diag(m, site_ok, u) : sV[row * kVStride + lane]);
    }
}

// the elements of the listed blocks no listed tile covers: one workgroup per block
__global__ __launch_bounds__(256) void matrix_banded_fill_kernel(const matrix_banded_plan::FillBlock *__restrict__ blocks,
                                                                 const uint8_t *__restrict__ site_ok,
                                                                 MatrixBandedArgs m) {
    const matrix_banded_plan::FillBlock e = blocks[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t k = (uint64_t)e.kb * kTile + lane;
    if (k > m.K) return;
    for (uint32_t row = wave; row < (uint32_t)kTile; row += 4) {
        const uint32_t u = e.ta * kTile + row;
        if (u < m.r0 || u >= m.r1) continue;
        if (matrix_banded_plan::covered(e.c0, e.c1, row, (uint32_t)k)) continue;
        banded_store(m, u, (uint32_t)k, k == 0 ? banded_diag(m, site_ok, u) : 0.0f);
    }
}

void launch_pair_matrix_banded(const ValuLaunch &v, const OrderArgs &o, const MatrixBandedArgs &m, hipStream_t st) {
    if (!v.n_tiles) return;
    // one whole-tile workgroup per listed tile at every list size, as the
    // dense matrix launches
    hipLaunchKernelGGL((pair_valu_kernel<false, false, true, true, false, kReduceMatrixBanded>), dim3(v.n_tiles),
                       dim3(256), 0, st, v.codes, v.w, v.site_ok, v.tiles, v.n_tiles, (const unsigned *)nullptr,
                       (const uint32_t *)nullptr, (unsigned *)nullptr, (const unsigned *)nullptr, 0u, v.L, v.NP, 1u,
                       v.ref_cls / 64, v.ref_tail_n, v.n_chunk_rows, 0.0f, o, m, ScanArgs{});
}

void launch_matrix_banded_fill(const matrix_banded_plan::FillBlock *blocks, uint32_t n_blocks, const uint8_t *site_ok,
                               const MatrixBandedArgs &m, hipStream_t st) {
    if (!n_blocks) return;
    hipLaunchKernelGGL(matrix_banded_fill_kernel, dim3(n_blocks), dim3(256), 0, st, blocks, site_ok, m);
}

}  // namespace wld
