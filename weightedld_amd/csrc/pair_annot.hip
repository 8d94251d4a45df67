// Partitioned LD scores (wld_run_annot_scores): every in-window pair's r2
// exactly as the default row path computes it — pair_valu_kernel<MF, REF>'s
// operands, lane-class chains, ordered horizontal sum, scalar tail and
// ld_epilogue, instantiated from the one template in pair_valu_kernel.hpp —
// multiplied into the annotation rows of the pair's two sites instead of
// compacted into rows:
//     score[a][c] += r2(a, b) annot[b][c],  score[b][c] += r2(a, b) annot[a][c].
// No row, segment count, staging slot or chunk total is written: a tile adds
// to the run's accumulators (AnnotArgs) and nothing else.
//
// The epilogue.  After the sums, wave w's lane (r, g) holds tot[i][j] of the
// pairs (a = a0 + 16 w + 4 g + i, b = b0 + 16 j + r), i, j = 0..3.  The pairs
// are classified and counted as summary_epilogue does it (wave ballots; the
// partner counts reduced over the row's lanes by shuffles and over the
// column's waves through LDS, one u32 atomic per site with a counted pair).
// The tile's counted r2 go to LDS as a 64x64 f32 matrix X (0 where a pair is
// not counted).  Per chunk of 16 annotation columns the tile then forms
//     R[a][c] = sum_b X[a][b] A_b[b][c]     (the a sites' share: A_b = the
//                                            annotation tile of the b sites)
//     C[b][c] = sum_a X[a][b] A_a[a][c]     (the b sites' share)
// on v_mfma_f64_16x16x4_f64: wave w owns the 16 output sites 16 w .. 16 w + 15
// of either product and runs the K loop over the tile's other 64 sites, 16
// MFMAs per product.  Lane (r, g) carries A[row r][k] and B[k][column r] at k =
// 16 g + kk in step kk (any one-to-one k order serves a sum over k; this one
// reads X — stride 65 — and the annotation tiles — stride 17 — without a bank
// conflict in either product); both operands are converted f32 -> f64 at the
// LDS read, so every product is exact (two 24-bit significands) and the
// accumulation is f64.  The result's element e of lane (r, g) is site g + 4 e of
// the wave's 16, column r (the f64 form's own C/D map), so the 16 lanes of a
// lane group add to 16 consecutive doubles of score[site][16 chunk ..]: one
// f64 atomic per (site, column) destination of the tile, none for an exact 0.
// A chunk whose annotation tile holds only zeros (AnnotArgs::zero) is skipped
// with its staging, product and atomics: it would add exact zeros.
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "pair_valu_kernel.hpp"

namespace wld {

namespace {
typedef double v4d __attribute__((ext_vector_type(4)));
constexpr int kXStride = 65;  // floats per row of X
constexpr int kAStride = 17;  // floats per site of an annotation tile
// f64 add into global memory by the hardware's atomic add (not a
// compare-and-swap loop); every destination is device memory of this context
__device__ __forceinline__ void global_add(double *p, double x) { (void)unsafeAtomicAdd(p, x); }
}  // namespace

__device__ __attribute__((always_inline)) void annot_epilogue(const AnnotArgs &k, const OrderArgs &o,
                                                              const uint8_t *site_ok, uint32_t L, uint32_t a0,
                                                              uint32_t b0, uint32_t tid,
                                                              const float (&tot)[4][4][4]) {
    __shared__ float sX[kTile * kXStride];
    __shared__ float sAa[kTile * kAStride];  // the a sites' annotation rows of the chunk
    __shared__ float sAb[kTile * kAStride];  // the b sites'
    __shared__ uint32_t sColCnt[4][kTile];
    __shared__ uint32_t sCls[4];  // pairs, none, nonfinite, counted of the tile
    const uint32_t lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
    const uint32_t ar = a0 + 16 * wave + 4 * g;  // this lane's a rows ar + i; its b columns b0 + 16 j + r
    if (tid < 4) sCls[tid] = 0;

    // which of the lane's 16 pairs are in the range (bit 4 i + j) and the site
    // flags: every load issued before the sums' epilogue (a, b < LP: nothing
    // is read past an array)
    uint32_t inr = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t a = ar + i, b = b0 + 16 * j + r;
            if ((a < b) & (b < L) & in_window(o, a, b)) inr |= 1u << (4 * i + j);
        }
    const uint32_t okA4 = *reinterpret_cast<const uint32_t *>(site_ok + ar);
    uint32_t okB = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) okB |= site_ok[b0 + 16 * j + r] ? 1u << j : 0u;
    __syncthreads();  // the class counts are zero

    uint32_t rn = 0, cn = 0;                        // counted pairs per row slot i / column slot j, 8 bits each
    uint32_t n_pairs = 0, n_none = 0, n_nonfin = 0;  // of the wave (uniform)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float d, dp, r2;
            ld_epilogue(tot[i][j][0], tot[i][j][1], tot[i][j][2], tot[i][j][3], d, dp, r2);
            const bool in = (inr >> (4 * i + j)) & 1u;
            const bool some = ((okA4 >> (8 * i)) & 0xFFu) && ((okB >> j) & 1u);
            const bool finite = fabsf(r2) <= 3.4028235e38f;  // (false for NaN)
            const bool counted = in && some && finite;
            n_pairs += (uint32_t)__popcll(__ballot(in));
            n_none += (uint32_t)__popcll(__ballot(in && !some));
            n_nonfin += (uint32_t)__popcll(__ballot(in && some && !finite));
            rn += (counted ? 1u : 0u) << (8 * i);
            cn += (counted ? 1u : 0u) << (8 * j);
            sX[(16 * wave + 4 * g + i) * kXStride + 16 * j + r] = counted ? r2 : 0.0f;
        }
    }
    if (lane == 0) {
        if (n_pairs) atomicAdd(&sCls[0], n_pairs);
        if (n_none) atomicAdd(&sCls[1], n_none);
        if (n_nonfin) atomicAdd(&sCls[2], n_nonfin);
    }

    // partners of the rows: over the 16 lanes r of a lane group; lane r == 0 holds the row
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) rn += __shfl_xor(rn, off, 64);
    if (r == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t c = (rn >> (8 * i)) & 0xFFu;
            if (c) atomicAdd(&k.partners[ar + i], c);  // (a counted pair: ar + i < L)
        }
    }
    // ... of the columns: over the four lane groups, then the four waves through LDS
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) cn += __shfl_xor(cn, off, 64);
    if (g == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) sColCnt[wave][16 * j + r] = (cn >> (8 * j)) & 0xFFu;
    }
    __syncthreads();  // X, the column counts and the class counts are complete
    if (tid < kTile) {
        uint32_t c = sColCnt[0][tid] + sColCnt[1][tid] + sColCnt[2][tid] + sColCnt[3][tid];
        if (c) atomicAdd(&k.partners[b0 + tid], c);  // (a counted pair: b0 + tid < L)
        // the tile's counted pairs: every one is in exactly one column
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) c += __shfl_xor(c, off, 64);
        if (tid == 0) {
            sCls[3] = c;
            if (c) atomicAdd(&k.counts[3], (unsigned long long)c);
            if (sCls[0]) atomicAdd(&k.counts[0], (unsigned long long)sCls[0]);
            if (sCls[1]) atomicAdd(&k.counts[1], (unsigned long long)sCls[1]);
            if (sCls[2]) atomicAdd(&k.counts[2], (unsigned long long)sCls[2]);
        }
    }
    __syncthreads();
    if (!sCls[3]) return;  // (uniform) X is all zero

    // the products, 16 annotation columns at a time
    const uint32_t chunks = k.CP / 16, ta = a0 / kTile, tb = b0 / kTile;
    const uint32_t lr = tid >> 2, part = tid & 3;  // stager: site row, 4-column part
    const uint32_t sw = 16 * wave;                 // the wave's 16 output sites of either product
    for (uint32_t cc = 0; cc < chunks; ++cc) {
        const bool do_rows = !k.zero[(size_t)tb * chunks + cc];  // R needs the b sites' tile (uniform)
        const bool do_cols = !k.zero[(size_t)ta * chunks + cc];  // C the a sites'
        if (!do_rows && !do_cols) continue;
        __syncthreads();  // the previous chunk's reads of sAa / sAb are done
        // (a0 + lr, b0 + lr < LP and 16 cc + 4 part + 3 < CP: inside the image; 16-byte aligned)
        if (do_cols) {
            const float4 v = *reinterpret_cast<const float4 *>(k.annot + (size_t)(a0 + lr) * k.CP + 16 * cc + 4 * part);
            float *p = sAa + lr * kAStride + 4 * part;
            p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
        }
        if (do_rows) {
            const float4 v = *reinterpret_cast<const float4 *>(k.annot + (size_t)(b0 + lr) * k.CP + 16 * cc + 4 * part);
            float *p = sAb + lr * kAStride + 4 * part;
            p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
        }
        __syncthreads();
        if (do_rows) {
            v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const uint32_t kq = 16 * g + kk;  // the b site of this step
                const double x = (double)sX[(sw + r) * kXStride + kq];
                const double y = (double)sAb[kq * kAStride + r];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)  // site a0 + sw + g + 4 e, column 16 cc + r (a nonzero sum: inside L x n_annot)
                if (acc[e] != 0.0) global_add(&k.score[(size_t)(a0 + sw + g + 4 * e) * k.CP + 16 * cc + r], acc[e]);
        }
        if (do_cols) {
            v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const uint32_t kq = 16 * g + kk;  // the a site of this step
                const double x = (double)sX[kq * kXStride + sw + r];
                const double y = (double)sAa[kq * kAStride + r];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)  // site b0 + sw + g + 4 e, column 16 cc + r
                if (acc[e] != 0.0) global_add(&k.score[(size_t)(b0 + sw + g + 4 * e) * k.CP + 16 * cc + r], acc[e]);
        }
    }
}

void launch_pair_annot(const ValuLaunch &v, const OrderArgs &o, const AnnotArgs &a, hipStream_t st) {
    if (!v.n_tiles) return;
    // one whole-tile workgroup per listed tile at every list size, as the
    // summary launches (16-row items would split a tile's columns over four
    // workgroups: four atomics per destination)
    hipLaunchKernelGGL((pair_valu_kernel<false, false, true, true, false, kReduceAnnot>), dim3(v.n_tiles), dim3(256),
                       0, st, v.codes, v.w, v.site_ok, v.tiles, v.n_tiles, (const unsigned *)nullptr,
                       (const uint32_t *)nullptr, (unsigned *)nullptr, (const unsigned *)nullptr, 0u, v.L, v.NP, 1u,
                       v.ref_cls / 64, v.ref_tail_n, v.n_chunk_rows, 0.0f, o, a, ScanArgs{});
}

}  // namespace wld
