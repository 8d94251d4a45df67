// LD summaries (wld_run_summary): every in-window pair's r2 exactly as the
// default row path computes it — pair_valu_kernel<MF, REF>'s operands (the
// lane-class layout), f32 MFMA chains per lane class, ordered horizontal sum,
// scalar tail and ld_epilogue, instantiated from the one template in
// pair_valu_kernel.hpp — with a reducing epilogue instead of the row path's
// compaction.  No row, segment count, staging slot or chunk total is written:
// a tile adds to the run's accumulators (SummaryArgs) and nothing else.
//
// The epilogue.  After the sums, wave w's lane (r, g) holds tot[i][j] of the
// pairs (a = a0 + 16 w + 4 g + i, b = b0 + 16 j + r), i, j = 0..3.  A pair in
// the range (a < b < L, in the window) is none (a site without a major or
// minor symbol), nonfinite (r2 NaN or +-inf) or counted; the three classes
// are counted with wave ballots (no atomics).  A counted pair's r2, converted
// to f64, goes
//   * to its row's sum: over j in the lane, then over the row's 16 lanes by
//     shuffles — each of the tile's 64 rows ends in one lane, which issues the
//     row's one global atomic (f64 add; u32 add for the partner count);
//   * to its column's sum: over i in the lane, over the four lane groups by
//     shuffles, over the four waves through LDS in wave order — 64 threads
//     issue the columns' atomics, and their wave-wide sum is the tile's share
//     of r2_sum and of the counted pairs (one atomic each);
//   * to its decay bin (bin_width > 0): an LDS histogram (u32 count, f64 sum)
//     over the bins the tile can touch — sites ascend in position, so the
//     tile's distances lie between those of its corners, a contiguous bin
//     range — with a lane's consecutive pairs of one bin merged in registers
//     first (wide bins: one LDS atomic per lane); the range is then flushed,
//     one global atomic per touched bin.
// So a tile issues at most one global atomic per destination, and the f64
// work is confined to the epilogue (16 converts and ~40 adds per lane).
// Counts are exact; the f64 sums are any-order sums of exact terms (the order
// of the tiles' atomics differs from run to run).
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "pair_valu_kernel.hpp"
#include "summary_plan.hpp"

namespace wld {

namespace {
// f64 add into LDS / global memory by the hardware's atomic add (not a
// compare-and-swap loop); every destination is device memory of this context
__device__ __forceinline__ void lds_add(double *p, double x) {
    (void)__hip_atomic_fetch_add(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void global_add(double *p, double x) { (void)unsafeAtomicAdd(p, x); }
}  // namespace

__device__ __attribute__((always_inline)) void summary_epilogue(const SummaryArgs &s, const OrderArgs &o,
                                                                const uint8_t *site_ok, uint32_t L, uint32_t a0,
                                                                uint32_t b0, uint32_t tid,
                                                                const float (&tot)[4][4][4]) {
    __shared__ double sColSum[4][kTile];
    __shared__ uint32_t sColCnt[4][kTile];
    __shared__ uint32_t sCls[3];  // pairs, none, nonfinite of the tile
    __shared__ double sBinSum[summary_plan::kMaxBins];
    __shared__ uint32_t sBinCnt[summary_plan::kMaxBins];
    const uint32_t lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
    const uint32_t ar = a0 + 16 * wave + 4 * g;  // this lane's a rows ar + i; its b columns b0 + 16 j + r
    const bool bins = s.bin_width != 0;          // (uniform)
    auto pos_of = [&](uint32_t x) -> uint32_t { return s.pos ? s.pos[x] : x; };  // x < L

    // the bins this tile can touch: positions ascend with the site index, so
    // every pair's distance lies between (first b - last a) and (last b - first a)
    uint32_t bin_lo = 0, bin_hi = 0;
    if (bins) {
        const uint32_t a_hi = min(a0 + kTile - 1, L - 1), b_hi = min(b0 + kTile - 1, L - 1);
        const uint32_t pa_lo = pos_of(a0), pa_hi = pos_of(a_hi), pb_lo = pos_of(b0), pb_hi = pos_of(b_hi);
        bin_lo = summary_plan::bin_index(pb_lo > pa_hi ? pb_lo - pa_hi : 0u, s.bin_width, s.n_bins);
        bin_hi = summary_plan::bin_index(pb_hi > pa_lo ? pb_hi - pa_lo : 0u, s.bin_width, s.n_bins);
        for (uint32_t k = bin_lo + tid; k <= bin_hi; k += 256) {
            sBinSum[k] = 0.0;
            sBinCnt[k] = 0;
        }
    }
    if (tid < 3) sCls[tid] = 0;

    // which of the lane's 16 pairs are in the range (bit 4 i + j), the site
    // flags and (with bins) the positions: every load issued before the sums'
    // epilogue (a, b < LP: nothing is read past an array)
    uint32_t inr = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t a = ar + i, b = b0 + 16 * j + r;
            if ((a < b) & (b < L) & in_window(o, a, b)) inr |= 1u << (4 * i + j);
        }
    const uint32_t okA4 = *reinterpret_cast<const uint32_t *>(site_ok + ar);
    uint32_t okB = 0, posA[4] = {0, 0, 0, 0}, posB[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) okB |= site_ok[b0 + 16 * j + r] ? 1u << j : 0u;
    if (bins) {
#pragma unroll
        for (int i = 0; i < 4; ++i) posA[i] = ar + i < L ? pos_of(ar + i) : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) posB[j] = b0 + 16 * j + r < L ? pos_of(b0 + 16 * j + r) : 0u;
    }
    __syncthreads();  // the histogram and the class counts are zero

    double rs[4] = {0.0, 0.0, 0.0, 0.0}, cs[4] = {0.0, 0.0, 0.0, 0.0};
    uint32_t rn = 0, cn = 0;                        // counted pairs per row slot i / column slot j, 8 bits each
    uint32_t n_pairs = 0, n_none = 0, n_nonfin = 0;  // of the wave (uniform)
    uint32_t cur_bin = 0, cur_cnt = 0;               // the lane's run of pairs in one bin
    double cur_sum = 0.0;
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
            const double x = counted ? (double)r2 : 0.0;
            rs[i] += x;
            cs[j] += x;
            rn += (counted ? 1u : 0u) << (8 * i);
            cn += (counted ? 1u : 0u) << (8 * j);
            if (bins && counted) {
                const uint32_t k = summary_plan::bin_index(posB[j] - posA[i], s.bin_width, s.n_bins);
                if (k != cur_bin && cur_cnt) {
                    lds_add(&sBinSum[cur_bin], cur_sum);
                    atomicAdd(&sBinCnt[cur_bin], cur_cnt);
                    cur_cnt = 0;
                    cur_sum = 0.0;
                }
                cur_bin = k;
                cur_cnt += 1;
                cur_sum += x;
            }
        }
    }
    if (cur_cnt) {
        lds_add(&sBinSum[cur_bin], cur_sum);
        atomicAdd(&sBinCnt[cur_bin], cur_cnt);
    }
    if (lane == 0) {
        if (n_pairs) atomicAdd(&sCls[0], n_pairs);
        if (n_none) atomicAdd(&sCls[1], n_none);
        if (n_nonfin) atomicAdd(&sCls[2], n_nonfin);
    }

    // rows: over the 16 lanes r of a lane group; lane r == 0 holds the row
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) rs[i] += __shfl_xor(rs[i], off, 64);
        rn += __shfl_xor(rn, off, 64);
    }
    if (r == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t c = (rn >> (8 * i)) & 0xFFu;
            if (c) {  // (a counted pair: ar + i < L)
                global_add(&s.score[ar + i], rs[i]);
                atomicAdd(&s.partners[ar + i], c);
            }
        }
    }
    // columns: over the four lane groups, then the four waves through LDS
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) cs[j] += __shfl_xor(cs[j], off, 64);
        cn += __shfl_xor(cn, off, 64);
    }
    if (g == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sColSum[wave][16 * j + r] = cs[j];
            sColCnt[wave][16 * j + r] = (cn >> (8 * j)) & 0xFFu;
        }
    }
    __syncthreads();
    if (tid < kTile) {
        double x = ((sColSum[0][tid] + sColSum[1][tid]) + sColSum[2][tid]) + sColSum[3][tid];
        uint32_t c = sColCnt[0][tid] + sColCnt[1][tid] + sColCnt[2][tid] + sColCnt[3][tid];
        if (c) {  // (a counted pair: b0 + tid < L)
            global_add(&s.score[b0 + tid], x);
            atomicAdd(&s.partners[b0 + tid], c);
        }
        // the tile's totals: every counted pair is in exactly one column
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            x += __shfl_xor(x, off, 64);
            c += __shfl_xor(c, off, 64);
        }
        if (tid == 0) {
            if (c) {
                global_add(s.r2_sum, x);
                atomicAdd(&s.counts[3], (unsigned long long)c);
            }
            if (sCls[0]) atomicAdd(&s.counts[0], (unsigned long long)sCls[0]);
            if (sCls[1]) atomicAdd(&s.counts[1], (unsigned long long)sCls[1]);
            if (sCls[2]) atomicAdd(&s.counts[2], (unsigned long long)sCls[2]);
        }
    }
    if (bins) {
        for (uint32_t k = bin_lo + tid; k <= bin_hi; k += 256) {
            const uint32_t c = sBinCnt[k];
            if (c) {
                global_add(&s.bin_r2_sum[k], sBinSum[k]);
                atomicAdd(&s.bin_pairs[k], (unsigned long long)c);
            }
        }
    }
}

void launch_pair_summary(const ValuLaunch &v, const OrderArgs &o, const SummaryArgs &s, hipStream_t st) {
    if (!v.n_tiles) return;
    // one whole-tile workgroup per listed tile at every list size (the row
    // path's 16-row items below 3,072 tiles split a tile's columns over four
    // workgroups, which would issue four atomics per column)
    hipLaunchKernelGGL((pair_valu_kernel<false, false, true, true, false, kReduceSummary>), dim3(v.n_tiles), dim3(256), 0, st,
                       v.codes, v.w, v.site_ok, v.tiles, v.n_tiles, (const unsigned *)nullptr,
                       (const uint32_t *)nullptr, (unsigned *)nullptr, (const unsigned *)nullptr, 0u, v.L, v.NP, 1u,
                       v.ref_cls / 64, v.ref_tail_n, v.n_chunk_rows, 0.0f, o, s, ScanArgs{});
}

}  // namespace wld
