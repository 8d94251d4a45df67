// LD blocks (wld_run_block_breaks, wld_blocks_from_breaks, wld_run_blocks):
// every considered pair's r2 or |d'| exactly as the default row path computes
// it — pair_valu_kernel<MF, REF>'s operands, lane-class chains, ordered
// horizontal sum, scalar tail and ld_epilogue, instantiated from the one
// template in pair_valu_kernel.hpp — classified against strong_min and reduced
// to what a partition of the site axis needs.  No row, segment count, staging
// slot or chunk total is written.
//
// After the sums, wave w's lane (r, g) holds tot[i][j] of the pairs (a = a0 +
// 16 w + 4 g + i, b = b0 + 16 j + r), i, j = 0..3.  A pair is considered when
// a < b < L and it is in the window; it is then none (a site without a major
// or minor symbol), nonfinite (the chosen value NaN or +-inf), strong (value >=
// strong_min) or weak.
//
// Pass 1, blocks_break_epilogue.  The classes are counted with wave ballots,
// one global atomic per class and tile.  The weak pairs are reduced to the
// smallest b per a row and the largest a per b column:
//   * in the lane, over its four columns resp. its four rows;
//   * a row lives in the 16 lanes (r = 0..15) of one lane group of one wave:
//     four butterfly steps inside the group, and the group's lane r = 0 holds
//     the row's minimum;
//   * a column lives in the four lane groups of all four waves: two butterfly
//     steps across the groups, then the four waves meet in an LDS table of 64
//     column slots (ds_max_u32 of a + 1, 0 = none).
// One global atomicMin per touched row and one global atomicMax per touched
// column and tile; a wave without a weak pair skips the butterflies, a tile
// without one writes nothing but the class counts.  Min and max of integers:
// exact and order independent, whatever order the tiles finish in.
//
// Pass 2, blocks_stats_epilogue.  A pair counts iff both sites carry the same
// block id >= 0.  Ids ascend over the sites, so the ids a tile can count lie
// in [max(lo_a, lo_b), min(hi_a, hi_b)] of its two 64-site blocks' id limits
// (uniform loads), fewer than blocks_plan::kTableIds: an LDS table {u32 pairs,
// informative, strong; f64 sum; u32 inverted key} over that run.  A lane walks
// its pairs column by column — its four rows are consecutive sites, so a
// column slot is mostly one run of one id, merged in registers — and adds each
// run with one LDS update per field.  The touched entries are then flushed
// with global atomics.  Counts and min are exact; the f64 sums are any-order
// sums of exact terms, as the heat map's.
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "blocks_plan.hpp"
#include "pair_valu_kernel.hpp"

namespace wld {

namespace {
__device__ __forceinline__ void blk_lds_add(double *p, double x) {
    (void)__hip_atomic_fetch_add(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void blk_global_add(double *p, double x) { (void)unsafeAtomicAdd(p, x); }

// which of the lane's 16 pairs are considered (bit 4 i + j)
__device__ __forceinline__ uint32_t considered_bits(const OrderArgs &o, uint32_t L, uint32_t ar, uint32_t b0,
                                                    uint32_t r) {
    uint32_t inr = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t a = ar + i, b = b0 + 16 * j + r;
            if ((a < b) & (b < L) & in_window(o, a, b)) inr |= 1u << (4 * i + j);
        }
    return inr;
}
}  // namespace

__device__ __attribute__((always_inline)) void blocks_break_epilogue(const BlockBreakArgs &k, const OrderArgs &o,
                                                                     const uint8_t *site_ok, uint32_t L, uint32_t a0,
                                                                     uint32_t b0, uint32_t tid,
                                                                     const float (&tot)[4][4][4]) {
    __shared__ uint32_t sCol[kTile];  // per b column of the tile: the largest weak a + 1
    __shared__ uint32_t sCls[5];      // pairs, none, nonfinite, strong, weak of the tile
    const uint32_t lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
    const uint32_t ar = a0 + 16 * wave + 4 * g;  // this lane's a rows ar + i; its b columns b0 + 16 j + r
    if (tid < kTile) sCol[tid] = 0;
    if (tid < 5) sCls[tid] = 0;

    // every load issued before the sums' epilogue (a, b < LP: nothing is read
    // past an array)
    const uint32_t inr = considered_bits(o, L, ar, b0, r);
    const uint32_t okA4 = *reinterpret_cast<const uint32_t *>(site_ok + ar);
    uint32_t okB = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) okB |= site_ok[b0 + 16 * j + r] ? 1u << j : 0u;
    __syncthreads();  // the table and the class counts are zero

    uint32_t n_pairs = 0, n_none = 0, n_nonfin = 0, n_strong = 0, n_weak = 0;  // of the wave (uniform)
    uint32_t row_min[4], col_max1[4];  // the lane's weak pairs: min b per row, max a + 1 per column
#pragma unroll
    for (int i = 0; i < 4; ++i) row_min[i] = blocks_plan::kNone, col_max1[i] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // (i ascending: the last weak row of a column is its largest)
            float d, dp, r2;
            ld_epilogue(tot[i][j][0], tot[i][j][1], tot[i][j][2], tot[i][j][3], d, dp, r2);
            const float val = k.stat ? fabsf(dp) : r2;  // (uniform)
            const bool in = (inr >> (4 * i + j)) & 1u;
            const bool some = ((okA4 >> (8 * i)) & 0xFFu) && ((okB >> j) & 1u);
            const bool finite = fabsf(val) <= 3.4028235e38f;  // (false for NaN)
            const bool inf = in && some && finite;
            const bool strong = inf && val >= k.strong_min;
            const bool weak = inf && !strong;
            n_pairs += (uint32_t)__popcll(__ballot(in));
            n_none += (uint32_t)__popcll(__ballot(in && !some));
            n_nonfin += (uint32_t)__popcll(__ballot(in && some && !finite));
            n_strong += (uint32_t)__popcll(__ballot(strong));
            n_weak += (uint32_t)__popcll(__ballot(weak));
            if (weak) {
                row_min[i] = min(row_min[i], b0 + 16 * j + r);  // (j ascending: the first one stays)
                col_max1[j] = ar + i + 1;
            }
        }
    }
    if (n_weak) {  // (uniform in the wave)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) row_min[i] = min(row_min[i], (uint32_t)__shfl_xor((int)row_min[i], m, 64));
#pragma unroll
            for (int m = 16; m < 64; m <<= 1)
                col_max1[i] = max(col_max1[i], (uint32_t)__shfl_xor((int)col_max1[i], m, 64));
        }
        if (r == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i)  // (a weak pair has a < b < L: ar + i < L)
                if (row_min[i] != blocks_plan::kNone) atomicMin(&k.fwd_weak[ar + i], row_min[i]);
        }
        if (g == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (col_max1[j]) atomicMax(&sCol[16 * j + r], col_max1[j]);
        }
    }
    if (lane == 0) {
        if (n_pairs) atomicAdd(&sCls[0], n_pairs);
        if (n_none) atomicAdd(&sCls[1], n_none);
        if (n_nonfin) atomicAdd(&sCls[2], n_nonfin);
        if (n_strong) atomicAdd(&sCls[3], n_strong);
        if (n_weak) atomicAdd(&sCls[4], n_weak);
    }
    __syncthreads();
    if (tid < 5 && sCls[tid]) atomicAdd(&k.classes[tid], (unsigned long long)sCls[tid]);
    if (tid < kTile && sCol[tid]) atomicMax(&k.bwd_weak1[b0 + tid], sCol[tid]);  // (a weak column: b0 + tid < L)
}

__device__ __attribute__((always_inline)) void blocks_stats_epilogue(const BlockStatsArgs &k, const OrderArgs &o,
                                                                     const uint8_t *site_ok, uint32_t L, uint32_t a0,
                                                                     uint32_t b0, uint32_t tid,
                                                                     const float (&tot)[4][4][4]) {
    constexpr uint32_t G = blocks_plan::kTableIds;
    __shared__ double sSum[G];
    __shared__ uint32_t sPairs[G], sInf[G], sStrong[G], sKey[G];
    const uint32_t lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
    const uint32_t ar = a0 + 16 * wave + 4 * g;

    // the ids the tile can count (uniform): both blocks' limits intersected
    const int32_t lo = max(k.blk_lo[a0 / kTile], k.blk_lo[b0 / kTile]);
    const int32_t hi = min(k.blk_hi[a0 / kTile], k.blk_hi[b0 / kTile]);
    const bool any = (lo >= 0) & (lo <= hi);
    // a table index is below this (the host's tables guarantee hi - lo < G; an
    // index that is not is dropped, never written through)
    const uint32_t run = any ? min((uint32_t)(hi - lo) + 1u, G) : 0u;
    if (tid < G) {
        sSum[tid] = 0.0;
        sPairs[tid] = 0;
        sInf[tid] = 0;
        sStrong[tid] = 0;
        sKey[tid] = blocks_plan::kNoInvKey;
    }
    const uint32_t inr = considered_bits(o, L, ar, b0, r);
    const uint32_t okA4 = *reinterpret_cast<const uint32_t *>(site_ok + ar);
    const int4 cA4 = *reinterpret_cast<const int4 *>(k.site_block + ar);
    const int32_t cA[4] = {cA4.x, cA4.y, cA4.z, cA4.w};
    uint32_t okB = 0;
    int32_t cB[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        okB |= site_ok[b0 + 16 * j + r] ? 1u << j : 0u;
        cB[j] = k.site_block[b0 + 16 * j + r];
    }
    __syncthreads();  // the table is zero

    // the lane's run of pairs in one block
    uint32_t cur_id = 0, cur_pairs = 0, cur_inf = 0, cur_strong = 0, cur_key = blocks_plan::kNoInvKey;
    double cur_sum = 0.0;
    auto flush = [&]() {
        if (cur_pairs && cur_id < run) {
            atomicAdd(&sPairs[cur_id], cur_pairs);
            if (cur_inf) {
                atomicAdd(&sInf[cur_id], cur_inf);
                if (cur_strong) atomicAdd(&sStrong[cur_id], cur_strong);
                blk_lds_add(&sSum[cur_id], cur_sum);
                atomicMax(&sKey[cur_id], cur_key);
            }
        }
        cur_pairs = cur_inf = cur_strong = 0;
        cur_sum = 0.0;
        cur_key = blocks_plan::kNoInvKey;
    };
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float d, dp, r2;
            ld_epilogue(tot[i][j][0], tot[i][j][1], tot[i][j][2], tot[i][j][3], d, dp, r2);
            const float val = k.stat ? fabsf(dp) : r2;  // (uniform)
            const bool in = ((inr >> (4 * i + j)) & 1u) && cA[i] >= lo && cA[i] == cB[j];  // (lo >= 0 where any)
            const bool some = ((okA4 >> (8 * i)) & 0xFFu) && ((okB >> j) & 1u);
            const bool finite = fabsf(val) <= 3.4028235e38f;  // (false for NaN)
            if (any && in) {
                const uint32_t id = (uint32_t)(cA[i] - lo);
                if (id != cur_id) flush();
                cur_id = id;
                cur_pairs += 1;
                if (some && finite) {
                    cur_inf += 1;
                    cur_strong += val >= k.strong_min ? 1u : 0u;
                    cur_sum += (double)val;
                    cur_key = max(cur_key, blocks_plan::inv_key(val));
                }
            }
        }
    }
    flush();
    __syncthreads();
    if (tid < run && sPairs[tid]) {
        const uint32_t id = (uint32_t)lo + tid;
        if (id < k.n_blocks) {
            atomicAdd(&k.pairs[id], (unsigned long long)sPairs[tid]);
            if (sInf[tid]) {
                atomicAdd(&k.informative[id], (unsigned long long)sInf[tid]);
                if (sStrong[tid]) atomicAdd(&k.strong[id], (unsigned long long)sStrong[tid]);
                blk_global_add(&k.sum[id], sSum[tid]);
                atomicMax(&k.min_key[id], sKey[tid]);
            }
        }
    }
}

namespace {
template <int REDUCE, class Args>
void launch_blocks(const ValuLaunch &v, const OrderArgs &o, const Args &b, hipStream_t st) {
    if (!v.n_tiles) return;
    // one whole-tile workgroup per listed tile at every list size, as the
    // summary and heat-map launches
    hipLaunchKernelGGL((pair_valu_kernel<false, false, true, true, false, REDUCE>), dim3(v.n_tiles), dim3(256), 0, st,
                       v.codes, v.w, v.site_ok, v.tiles, v.n_tiles, (const unsigned *)nullptr,
                       (const uint32_t *)nullptr, (unsigned *)nullptr, (const unsigned *)nullptr, 0u, v.L, v.NP, 1u,
                       v.ref_cls / 64, v.ref_tail_n, v.n_chunk_rows, 0.0f, o, b, ScanArgs{});
}
}  // namespace

void launch_pair_block_breaks(const ValuLaunch &v, const OrderArgs &o, const BlockBreakArgs &b, hipStream_t st) {
    launch_blocks<kReduceBreaks>(v, o, b, st);
}
void launch_pair_block_stats(const ValuLaunch &v, const OrderArgs &o, const BlockStatsArgs &b, hipStream_t st) {
    launch_blocks<kReduceBlockStats>(v, o, b, st);
}

}  // namespace wld
