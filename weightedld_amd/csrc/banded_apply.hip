// The band product (wld_banded_apply_device): Y = S X, S the symmetric n x n
// matrix whose upper band B (element k of row i = S[i][i + k], k = 0..K, ld
// elements apart, float or binary16) a banded LD matrix call wrote, X a block
// of n_cols vectors (float or double), Y double:
//
//   Y[i][c] = sum_{k=0..K, i+k<n} B[i][k] X[i+k][c] + sum_{k=1..min(K,i)} B[i-k][k] X[i-k][c]
//
// Owner computes: a workgroup owns the 64 output rows i0 .. i0 + 63 and up to
// 64 columns, walks the 64x64 blocks S[i0..][jb..] that meet the band from left
// to right and adds S_block X[jb..] on v_mfma_f64_16x16x4_f64, so every Y
// element is one f64 accumulator's sum in one fixed order: no atomic, two calls
// give identical bytes.  The band is read twice over the grid (each B[i][k]
// serves rows i and i + k); that is the price of a deterministic sum.
//
// Unskew.  Both shares of a block are contiguous runs of band rows:
//   * right of the diagonal (jb > i0): S[i][j] = B[i][j - i], the 64 elements
//     k = jb - i .. jb - i + 63 of band row i: a wave loads one row's run and
//     writes it to row i - i0 of the LDS block;
//   * left (jb < i0): S[i][j] = B[j][i - j], the 64 elements k = i0 - j .. i0 -
//     j + 63 of band row j: the same load, written as column j - jb (row stride
//     65 floats: no bank conflict);
//   * the diagonal block: the run k = 0 .. 63 - (i - i0) of band row i, written
//     at [i][j] and at [j][i].
// Elements outside the band (k > K), the matrix (j >= n) or the block's
// triangle are +0.0 in LDS and never read from memory: a band element with
// i + k >= n is never touched, whatever it holds.  A +0.0 of the block still
// multiplies its X entry, so X must be finite (a non-finite X entry reaches the
// outputs of the whole 64-blocks around it, not only its band); non-finite
// band values propagate by IEEE rules to the rows i and i + k they belong to.
//
// MFMA.  Wave w owns the output rows 16 w .. 16 w + 15 of the block and one
// 16x16 accumulator per 16-column chunk.  In step kk lane (r, g) carries
// A[row r][k] = S[16 w + r][16 g + kk] and B[k][column r] = X[jb + 16 g +
// kk][16 chunk + r] (any one-to-one k order serves a sum; this one keeps the
// 32 lanes of an LDS lane group on 32 banks), both converted to f64 at the LDS
// read: a float x float product is exact in f64, a double X rounds each
// product once, inside the fused multiply-add.  The result's element e of lane
// (r, g) is row g + 4 e of the wave's 16, column r (the f64 form's own C/D
// map, not the f32 forms').
//
// The next block's loads are issued into registers before the current block's
// MFMAs, so a workgroup keeps one block of loads in flight.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace wld {

namespace {
typedef double v4d __attribute__((ext_vector_type(4)));
constexpr int kSide = 64, kSStride = 65;
constexpr uint64_t kMaxGridY = 32768;

template <typename T>
__device__ __forceinline__ float band_load(const void *p, size_t e) {
    return (float)reinterpret_cast<const T *>(p)[e];
}

// NCH: 16-column chunks per workgroup (1 or 4)
template <typename TB, typename TX, int NCH>
__global__ __launch_bounds__(256) void banded_apply_kernel(BandedApplyArgs a) {
    constexpr int NC = 16 * NCH, kXStride = NC + 1, kXPer = kSide * NC / 256;
    __shared__ float sS[kSide * kSStride];
    __shared__ TX sX[kSide * kXStride];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
    const uint32_t n = a.n, K = a.K;
    const uint32_t i0 = blockIdx.x * kSide, c0 = blockIdx.y * NC;
    const TX *__restrict__ X = reinterpret_cast<const TX *>(a.x);

    // the blocks jb = i0 + 64 m that meet the band and the matrix
    const uint32_t reach = (uint32_t)(((uint64_t)K + kSide - 1) / kSide);
    const int m_lo = -(int)min(i0 / kSide, reach), m_hi = (int)min(reach, (n - 1 - i0) / kSide);

    float vs[16];   // this thread's 16 band elements of a block: rows wave + 4 q
    TX vx[kXPer];   // and its share of the X rows
    // Every load is unconditional (an element out of the band reads element 0
    // of its array, which always exists, and is replaced by +0.0 afterwards): a
    // branch around each load would make the compiler wait for one load before
    // it issues the next.  The three block kinds share one address rule: the
    // band rows are those of the block's rows (right of and on the diagonal) or
    // of its columns (left), `col` is the other index, and k = col - band row.
    auto load_block = [&](int m) {
        const uint32_t jb = (uint32_t)((int)i0 + m * kSide);
        const uint32_t brow0 = m < 0 ? jb : i0, col = (m > 0 ? jb : i0) + lane;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const uint32_t brow = brow0 + wave + 4 * q;
            const bool ok = brow < n && col < n && col >= brow && col - brow <= K;  // (i + k < n: col < n)
            const float v = band_load<TB>(a.band, ok ? (size_t)brow * a.ld + (col - brow) : 0);
            vs[q] = ok ? v : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < kXPer; ++q) {
            const uint32_t e = tid + 256 * q, row = e / NC, c = c0 + e % NC;
            const uint32_t j = jb + row;
            const bool ok = j < n && c < a.n_cols;
            const TX v = X[ok ? (size_t)j * a.ldx + c : 0];
            vx[q] = ok ? v : (TX)0;
        }
    };

    v4d acc[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) acc[ch] = v4d{0.0, 0.0, 0.0, 0.0};

    load_block(m_lo);
    for (int m = m_lo; m <= m_hi; ++m) {
        __syncthreads();  // the previous block's reads are done
        if (m != 0) {  // (uniform) by rows right of the diagonal, by columns left of it
            const uint32_t at = m < 0 ? lane * kSStride + wave : wave * kSStride + lane, step = m < 0 ? 4 : 4 * kSStride;
#pragma unroll
            for (int q = 0; q < 16; ++q) sS[at + q * step] = vs[q];
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const uint32_t row = wave + 4 * q;
                if (lane >= row) {
                    sS[row * kSStride + lane] = vs[q];
                    if (lane > row) sS[lane * kSStride + row] = vs[q];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < kXPer; ++q) {
            const uint32_t e = tid + 256 * q;
            sX[(e / NC) * kXStride + e % NC] = vx[q];
        }
        __syncthreads();  // the block is staged
        if (m < m_hi) load_block(m + 1);
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const uint32_t kq = 16 * g + kk;
            const double s = (double)sS[(16 * wave + r) * kSStride + kq];
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
                acc[ch] = __builtin_amdgcn_mfma_f64_16x16x4f64(s, (double)sX[kq * kXStride + 16 * ch + r], acc[ch], 0, 0, 0);
        }
    }

#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t i = i0 + 16 * wave + g + 4 * e, c = c0 + 16 * ch + r;
            if (i < n && c < a.n_cols) a.y[(size_t)i * a.ldy + c] = acc[ch][e];
        }
}

template <typename TB, typename TX>
void launch_typed(const BandedApplyArgs &a, hipStream_t st) {
    const uint32_t rows = (a.n + kSide - 1) / kSide;
    if (a.n_cols <= 16)
        hipLaunchKernelGGL((banded_apply_kernel<TB, TX, 1>), dim3(rows, 1), dim3(256), 0, st, a);
    else
        for (uint64_t c = 0; c < a.n_cols; c += 64 * kMaxGridY) {  // (a grid's y extent is 16-bit)
            BandedApplyArgs b = a;
            b.x = static_cast<const TX *>(a.x) + c;
            b.y = a.y + c;
            b.n_cols = (uint32_t)std::min<uint64_t>(a.n_cols - c, 64 * kMaxGridY);
            hipLaunchKernelGGL((banded_apply_kernel<TB, TX, 4>), dim3(rows, (b.n_cols + 63) / 64), dim3(256), 0, st, b);
        }
}
}  // namespace

void launch_banded_apply(const BandedApplyArgs &a, hipStream_t st) {
    if (!a.n || !a.n_cols) return;
    if (a.band_f16) {
        if (a.x64) launch_typed<_Float16, double>(a, st);
        else launch_typed<_Float16, float>(a, st);
    } else {
        if (a.x64) launch_typed<float, double>(a, st);
        else launch_typed<float, float>(a, st);
    }
}

}  // namespace wld
