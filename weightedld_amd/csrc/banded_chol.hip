// The banded Cholesky factorisation and its triangular solves
// (wld_banded_cholesky_device, wld_banded_solve_device): A = U^T U for the
// symmetric positive definite matrix A of bandwidth K, U upper triangular with
// the same bandwidth, in the band layout of a banded LD matrix in f64:
// f[i * ldf + k] = U(i, i + k), k = 0..K.
//
// Right-looking, blocked by 64 rows (banded_chol_plan.hpp).  The fill kernel
// writes f64(band) + shifts and the +0.0 tails into f; then block row I (rows
// i0 .. i0 + 63) takes up to three launches, ordered by the stream and nothing
// else:
//
//   diag    one workgroup factors the 64x64 diagonal block (the plain
//           right-looking algorithm, one pivot per step; the block in
//           registers, the pivot row through LDS) and stores it.
//   panel   every workgroup stages the factored block in LDS and solves 64
//           columns of the panel U(I, i0 + 64 ..) against U_II^T by forward
//           substitution, 64 steps, the columns in registers.  (Factoring the
//           block again in every panel workgroup would save this launch, but
//           the block's owner stores U_II where the others read A_II: they
//           would need a second copy of the block.)
//   window  workgroup (a, b), a <= b, of the panel's 64-column blocks subtracts
//           U_Ia^T U_Ib from the trailing block at rows i0 + 64 a, columns i0 +
//           64 b on v_mfma_f64_16x16x4_f64: both panel blocks staged in LDS,
//           the block's elements the accumulators' initial values, so every
//           element of U is one accumulator's sum in one fixed order.
//
// Right-looking rather than left-looking: a step's window gives (K/64)^2 / 2
// independent workgroups where a left-looking step gives K/64, and a block row
// is final once its own step ran, which is what a failed factorisation leaves
// behind (the rows before the failing block row).
//
// Elements outside the band (k > K) or the matrix (j >= n) are +0.0 in LDS and
// registers and are never loaded or stored.  A pivot that is not > 0 (NaN
// included) stops the factorisation: the diagonal launch writes
// its row to the status word, and every kernel launched afterwards reads the
// word and returns.  No kernel waits for another workgroup.
//
// The solve kernel: a workgroup owns 16 or 64 right-hand-side columns and
// marches over the block rows itself, left-looking: forward, y_I = U_II^-T (b_I
// - sum_m U_{I-m,I}^T y_{I-m}), the sum on f64 MFMAs over the panel blocks of
// the earlier block rows, the y blocks read back from memory (b is streamed,
// never held in LDS as a whole); backward, x_I = U_II^-1 (y_I - sum_m U_{I,I+m}
// x_{I+m}).  The diagonal block is solved by substitution in LDS, 64 steps.
// The next block's loads are issued into registers before the current block's
// MFMAs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "banded_chol_plan.hpp"
#include "kernels.hpp"

namespace wld {

namespace {
typedef double v4d __attribute__((ext_vector_type(4)));
namespace bcp = banded_chol_plan;
constexpr int kSide = 64;
constexpr uint32_t kMaxGridY = 32768;
constexpr uint64_t kMaxGridX = 1u << 30;

template <typename TB>
__global__ __launch_bounds__(256) void chol_fill_kernel(BandedCholArgs a) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        a.status->first_bad = a.n;
        a.status->pad = 0;
        a.status->min_pivot = INFINITY;
    }
    if (k > a.K) return;
    const TB *__restrict__ B = reinterpret_cast<const TB *>(a.band);
    for (uint64_t i = blockIdx.y; i < a.n; i += gridDim.y) {
        double v = 0.0;
        if (i + k < a.n) {
            v = (double)B[i * a.ld + k];
            if (k == 0) {
                v = v + a.ridge;
                if (a.diag) v = v + a.diag[i];
            }
        }
        a.f[i * a.ldf + k] = v;
    }
}

// the status word, read once per workgroup (every thread sees the same value)
__device__ __forceinline__ bool chol_stopped(const BandedCholArgs &a, uint32_t *s_word) {
    if (threadIdx.x == 0) *s_word = a.status->first_bad;
    __syncthreads();
    return *s_word != a.n;
}

// one workgroup: the 64x64 diagonal block of the block row at i0, factored and
// stored; a bad pivot goes to the status word instead.  Thread (j, q) keeps the
// rows 16 q .. 16 q + 15 of column j in registers; in step k the wave that owns
// row k scales it and publishes it in LDS (two buffers, one barrier per step),
// and every wave with later rows subtracts its rank-1 update.
__global__ __launch_bounds__(256) void chol_diag_kernel(BandedCholArgs a, uint32_t i0) {
    __shared__ double sRow[2][kSide];
    __shared__ double sPiv[kSide];
    __shared__ uint32_t sBadAt[2];
    __shared__ uint32_t sWord;
    if (chol_stopped(a, &sWord)) return;
    const uint32_t tid = threadIdx.x, j = tid & 63, q = tid >> 6, n = a.n, K = a.K;
    const uint32_t nr = min((uint32_t)kSide, n - i0);
    double *__restrict__ F = a.f;

    // the upper triangle; everything else +0.0
    double r[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const uint32_t i = 16 * q + t;
        const bool ok = j >= i && j - i <= K && (uint64_t)i0 + j < n;
        const double v = F[ok ? (size_t)(i0 + i) * a.ldf + (j - i) : 0];
        r[t] = ok ? v : 0.0;
    }
    int bad = -1;
#pragma unroll
    for (int k = 0; k < kSide; ++k) {
        if (bad >= 0 || (uint32_t)k >= nr) continue;  // (uniform; no break: the loop unrolls, r[] stays in registers)
        if (q == (uint32_t)(k >> 4)) {
            const double mine = r[k & 15];      // row k, column j (+0.0 left of the diagonal)
            const double p = __shfl(mine, k);   // the pivot, from lane k
            const double s = sqrt(p);
            const double u = j == (uint32_t)k ? s : mine / s;
            r[k & 15] = u;
            sRow[k & 1][j] = u;
            if (j == 0) {
                sBadAt[k & 1] = p > 0.0 ? 0u : 1u;  // (NaN: bad)
                sPiv[k] = s;
            }
        }
        __syncthreads();
        if (sBadAt[k & 1]) {  // (uniform: one LDS word)
            bad = k;
            continue;
        }
        if (16 * q + 15 > (uint32_t)k) {  // (per wave)
            const double ukj = sRow[k & 1][j];
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const uint32_t i = 16 * q + t;
                const double v = fma(-sRow[k & 1][i], ukj, r[t]);
                r[t] = i > (uint32_t)k && j >= i ? v : r[t];
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        double m = a.status->min_pivot;
        const uint32_t done = bad < 0 ? nr : (uint32_t)bad;
        for (uint32_t e = 0; e < done; ++e) m = sPiv[e] < m ? sPiv[e] : m;
        a.status->min_pivot = m;
        if (bad >= 0) a.status->first_bad = i0 + (uint32_t)bad;
    }
    if (bad >= 0) return;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const uint32_t i = 16 * q + t;
        if (j >= i && j - i <= K && (uint64_t)i0 + j < n) F[(size_t)(i0 + i) * a.ldf + (j - i)] = r[t];
    }
}

// the panel of the block row at i0 (a full block row: a panel exists only
// right of one): U_II^T X = A_I,panel by forward substitution against the
// factored diagonal block, staged in LDS.  64 panel columns per workgroup;
// thread (c, q) keeps the rows 16 q .. 16 q + 15 of column c in registers; in
// step i the wave that owns row i divides and publishes it, and every wave with
// later rows subtracts (one barrier per step).
__global__ __launch_bounds__(256) void chol_panel_kernel(BandedCholArgs a, uint32_t i0) {
    __shared__ double sD[kSide * kSide];
    __shared__ double sXb[2][kSide];
    __shared__ uint32_t sWord;
    if (chol_stopped(a, &sWord)) return;
    const uint32_t tid = threadIdx.x, n = a.n, K = a.K;
    double *__restrict__ F = a.f;
    for (uint32_t e = tid; e < kSide * kSide; e += 256) {
        const uint32_t rr = e >> 6, cc = e & 63;
        const bool ok = cc >= rr && cc - rr <= K;
        const double v = F[ok ? (size_t)(i0 + rr) * a.ldf + (cc - rr) : 0];
        sD[e] = ok ? v : 0.0;
    }
    const uint32_t c = tid & 63, q = tid >> 6;
    const uint64_t j = (uint64_t)i0 + kSide + (uint64_t)kSide * blockIdx.x + c;
    double r[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const uint32_t i = 16 * q + t;
        const uint64_t k = j - (i0 + i);
        const bool ok = j < n && k <= K;
        const double x = F[ok ? (size_t)(i0 + i) * a.ldf + k : 0];
        r[t] = ok ? x : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kSide; ++i) {
        if (q == (uint32_t)(i >> 4)) {
            const double x = r[i & 15] / sD[i * kSide + i];
            r[i & 15] = x;
            sXb[i & 1][c] = x;
        }
        __syncthreads();
        if (16 * q + 15 > (uint32_t)i) {  // (per wave)
            const double x = sXb[i & 1][c];
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const uint32_t i2 = 16 * q + t;
                const double v = fma(-sD[i * kSide + i2], x, r[t]);
                r[t] = i2 > (uint32_t)i ? v : r[t];
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const uint32_t i = 16 * q + t;
        const uint64_t k = j - (i0 + i);
        if (j < n && k <= K) F[(size_t)(i0 + i) * a.ldf + k] = r[t];
    }
}

// workgroup t0 + x: the t-th pair a <= b of the panel's blocks in the plan's
// order (banded_chol_plan::tri_decode; 0-based here): the trailing block at
// the panel blocks a + 1 (rows) and b + 1 (columns)
__global__ __launch_bounds__(256) void chol_window_kernel(BandedCholArgs a, uint32_t i0, uint64_t t0) {
    constexpr int S = 80;  // (row stride: the four k rows of an MFMA step on distinct banks)
    __shared__ double sA[kSide * S];
    __shared__ double sB[kSide * S];
    __shared__ uint32_t sWord;
    uint32_t ma, mb;
    bcp::tri_decode(t0 + blockIdx.x, &ma, &mb);
    if (chol_stopped(a, &sWord)) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
    const uint32_t n = a.n, K = a.K;
    double *__restrict__ F = a.f;
    const uint64_t ja = (uint64_t)i0 + (uint64_t)kSide * (ma + 1), jb = (uint64_t)i0 + (uint64_t)kSide * (mb + 1);

    // the two panel blocks: rows i0 .. i0 + 63 (all < n), a run of k per row
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const uint32_t row = wave + 4 * q;
        const uint64_t i = (uint64_t)i0 + row;
        {
            const uint64_t j = ja + lane, k = j - i;
            const bool ok = j < n && k <= K;
            const double x = F[ok ? i * a.ldf + k : 0];
            sA[row * S + lane] = ok ? x : 0.0;
        }
        if (mb != ma) {
            const uint64_t j = jb + lane, k = j - i;
            const bool ok = j < n && k <= K;
            const double x = F[ok ? i * a.ldf + k : 0];
            sB[row * S + lane] = ok ? x : 0.0;
        }
    }
    const double *pB = mb == ma ? sA : sB;

    // the block's own elements start the accumulators: element e of lane (r, g)
    // is row 16 wave + g + 4 e, column 16 ch + r
    v4d acc[4];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint64_t j = ja + 16 * wave + g + 4 * e, jj = jb + 16 * ch + r;
            const bool ok = jj < n && jj >= j && jj - j <= K;
            const double x = F[ok ? j * a.ldf + (jj - j) : 0];
            acc[ch][e] = ok ? x : 0.0;
        }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const uint32_t i = 4 * s + g;
        const double ua = -sA[i * S + 16 * wave + r];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
            acc[ch] = __builtin_amdgcn_mfma_f64_16x16x4f64(ua, pB[i * S + 16 * ch + r], acc[ch], 0, 0, 0);
    }
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint64_t j = ja + 16 * wave + g + 4 * e, jj = jb + 16 * ch + r;
            if (jj < n && jj >= j && jj - j <= K) F[j * a.ldf + (jj - j)] = acc[ch][e];
        }
}

// NCH: 16-column chunks per workgroup (1 or 4)
template <int NCH>
__global__ __launch_bounds__(256) void banded_solve_kernel(BandedSolveArgs a) {
    constexpr int NC = 16 * NCH, SP = 65, SX = NCH == 1 ? 16 : 80, kXPer = kSide * NC / 256, Q = 256 / NC;
    __shared__ double sP[kSide * SP];
    __shared__ double sX[kSide * SX];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
    const uint32_t n = a.n, K = a.K;
    const uint64_t c0 = (uint64_t)blockIdx.x * NC;
    const double *__restrict__ F = a.f;
    double *X = a.b;
    const uint32_t R = (uint32_t)(((uint64_t)n + kSide - 1) / kSide);
    const uint32_t reach = (uint32_t)(((uint64_t)K + kSide - 1) / kSide);
    const uint32_t sc = tid % NC, sq = tid / NC;  // the substitution's column and row group

    double vs[16], vx[kXPer];
    // block (rows rb .., columns cb ..) of U and the 64 solution rows xb .. :
    // unconditional loads, as in banded_apply.hip
    auto load_block = [&](uint64_t rb, uint64_t cb, bool with_x, uint64_t xb) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const uint64_t i = rb + wave + 4 * q, j = cb + lane;
            const bool ok = j < n && j >= i && j - i <= K;  // (i <= j < n)
            const double v = F[ok ? i * a.ldf + (j - i) : 0];
            vs[q] = ok ? v : 0.0;
        }
#pragma unroll
        for (int q = 0; q < kXPer; ++q) {
            const uint32_t e = tid + 256 * q;
            const uint64_t j = xb + e / NC, c = c0 + e % NC;
            const bool ok = with_x && j < n && c < a.n_cols;
            const double v = X[ok ? j * a.ldb + c : 0];
            vx[q] = ok ? v : 0.0;
        }
    };

    for (int pass = 0; pass < 2; ++pass) {
        const bool back = pass == 1;
        if (back ? !a.bwd : !a.fwd) continue;
        for (uint32_t step = 0; step < R; ++step) {
            const uint32_t I = back ? R - 1 - step : step;
            const uint64_t i0 = (uint64_t)I * kSide;
            const uint32_t nr = (uint32_t)min((uint64_t)kSide, n - i0);
            // the blocks before the diagonal one: forward, the earlier block rows'
            // panel blocks above this one (farthest first); backward, this block
            // row's own panel blocks (nearest first)
            const uint32_t ns = back ? min(reach, (uint32_t)((n - 1 - i0) / kSide)) : min(I, reach);
            auto load_stage = [&](uint32_t s) {
                const uint64_t off = (uint64_t)kSide * (back ? s + 1 : ns - s);
                const uint64_t rb = s == ns || back ? i0 : i0 - off, cb = s != ns && back ? i0 + off : i0;
                load_block(rb, cb, s != ns, back ? cb : rb);
            };
            // this block row's right-hand side, in the accumulators' layout
            double bv[4 * NCH];
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint64_t i = i0 + 16 * wave + g + 4 * e, c = c0 + 16 * ch + r;
                    const bool ok = i < n && c < a.n_cols;
                    const double v = X[ok ? i * a.ldb + c : 0];
                    bv[4 * ch + e] = ok ? v : 0.0;
                }
            v4d acc[NCH];
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) acc[ch] = v4d{0.0, 0.0, 0.0, 0.0};

            load_stage(0);
            for (uint32_t s = 0; s <= ns; ++s) {
                __syncthreads();  // the previous block's reads are done
#pragma unroll
                for (int q = 0; q < 16; ++q) sP[(wave + 4 * q) * SP + lane] = vs[q];
                if (s < ns) {
#pragma unroll
                    for (int q = 0; q < kXPer; ++q) {
                        const uint32_t e = tid + 256 * q;
                        sX[(e / NC) * SX + e % NC] = vx[q];
                    }
                } else {
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            sX[(16 * wave + g + 4 * e) * SX + 16 * ch + r] = bv[4 * ch + e] - acc[ch][e];
                }
                __syncthreads();  // the block is staged
                if (s < ns) {
                    load_stage(s + 1);
#pragma unroll
                    for (int kk = 0; kk < 16; ++kk) {
                        const uint32_t kq = 4 * kk + g;
                        // forward: U^T, row = the block's column; backward: U, row = its row
                        const double u = back ? sP[(16 * wave + r) * SP + kq] : sP[kq * SP + 16 * wave + r];
#pragma unroll
                        for (int ch = 0; ch < NCH; ++ch)
                            acc[ch] = __builtin_amdgcn_mfma_f64_16x16x4f64(u, sX[kq * SX + 16 * ch + r], acc[ch], 0, 0, 0);
                    }
                }
            }
            // the diagonal block by substitution: thread (sc, sq) owns column sc
            // and every Q-th row; the row just solved goes to memory
            const bool col_ok = c0 + sc < a.n_cols;
            for (uint32_t t = 0; t < nr; ++t) {
                const uint32_t i = back ? nr - 1 - t : t;
                const double x = sX[i * SX + sc] / sP[i * SP + i];
                if (sq == i % Q && col_ok) X[(i0 + i) * a.ldb + c0 + sc] = x;
                if (back) {
                    for (uint32_t i2 = sq; i2 < i; i2 += Q)
                        sX[i2 * SX + sc] = fma(-sP[i2 * SP + i], x, sX[i2 * SX + sc]);
                } else {
                    for (uint32_t i2 = i + 1 + sq; i2 < nr; i2 += Q)
                        sX[i2 * SX + sc] = fma(-sP[i * SP + i2], x, sX[i2 * SX + sc]);
                }
                __syncthreads();
            }
            __syncthreads();  // the block row's solution is in memory before the next one reads it
        }
    }
}
}  // namespace

void launch_banded_chol(const BandedCholArgs &a, hipStream_t st) {
    if (!a.n) return;
    const dim3 fill((uint32_t)(((uint64_t)a.K + 256) / 256), std::min(a.n, kMaxGridY));
    if (a.band_f16) hipLaunchKernelGGL((chol_fill_kernel<_Float16>), fill, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((chol_fill_kernel<float>), fill, dim3(256), 0, st, a);
    const uint32_t R = bcp::block_rows(a.n);
    for (uint32_t I = 0; I < R; ++I) {
        const bcp::Step s = bcp::step(a.n, a.K, I);
        const uint32_t cols = s.panel_end - s.panel_begin;
        hipLaunchKernelGGL(chol_diag_kernel, dim3(1), dim3(256), 0, st, a, s.i0);
        if (cols) hipLaunchKernelGGL(chol_panel_kernel, dim3(s.blocks), dim3(256), 0, st, a, s.i0);
        const uint64_t pairs = bcp::tri_count(s.blocks);
        for (uint64_t t0 = 0; t0 < pairs; t0 += kMaxGridX)  // (one launch unless the panel has > 46,340 blocks)
            hipLaunchKernelGGL(chol_window_kernel, dim3((uint32_t)std::min<uint64_t>(pairs - t0, kMaxGridX)), dim3(256), 0,
                               st, a, s.i0, t0);
    }
}

void launch_banded_solve(const BandedSolveArgs &a, hipStream_t st) {
    if (!a.n || !a.n_cols) return;
    if (a.n_cols <= 16) hipLaunchKernelGGL((banded_solve_kernel<1>), dim3(1), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((banded_solve_kernel<4>), dim3((a.n_cols + 63) / 64), dim3(256), 0, st, a);
}

}  // namespace wld
