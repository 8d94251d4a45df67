// LD heat map (wld_run_heatmap): every considered pair's r2 or |d'| exactly
// as the default row path computes it — pair_valu_kernel<MF, REF>'s operands,
// lane-class chains, ordered horizontal sum, scalar tail and ld_epilogue,
// instantiated from the one template in pair_valu_kernel.hpp — reduced over a
// caller-defined grid of site cells instead of compacted into rows.  No row,
// segment count, staging slot or chunk total is written: a tile adds to the
// run's accumulators (HeatmapArgs) and nothing else.
//
// The epilogue.  After the sums, wave w's lane (r, g) holds tot[i][j] of the
// pairs (a = a0 + 16 w + 4 g + i, b = b0 + 16 j + r), i, j = 0..3.  A pair is
// considered when a < b < L, it is in the window and both sites have a cell;
// it is then none (a site without a major or minor symbol), nonfinite (the
// chosen value NaN or +-inf) or counted.  The classes are counted with wave
// ballots, one global atomic per class and tile.  A counted pair's value goes
// to cell (site_cell[a], site_cell[b]): count + 1, sum + (double) value, max
// by the order-preserving key of heatmap_plan.hpp (right for negative values
// too: an f32 r2 can come out slightly below 0).
//
// Cell ids do not descend over the sites, so the tile touches the rectangle
// [cell of its first a site with one .. cell of its last] x [the same for b],
// which the host gives per 64-site block (blk_lo, blk_hi: uniform loads).
//   * Coarse (the rectangle holds at most G = kGridCells cells; any map with
//     cells of two sites or more and no long runs of empty cells): an LDS
//     grid {u32 count, f64 sum, u32 key} over the rectangle.  A lane walks its
//     pairs column by column; its four rows are consecutive sites, so with
//     cells of >= 4 sites a column slot is one run of one cell, merged in
//     registers and added with one LDS update (ds_add_u32, ds_add_f64,
//     ds_max_u32).  The rectangle is then flushed: one global atomic triple
//     per touched cell and tile, empty cells skipped.
//   * Fine (a larger rectangle: cells about a site wide, or many empty cells
//     inside a block): after the same in-lane merge the lanes add straight to
//     the global grid.  Correct, not fast.
// Counts and max are exact and order independent; the f64 sums are any-order
// sums of exact terms (the order of the tiles' atomics differs from run to
// run).
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "heatmap_plan.hpp"
#include "pair_valu_kernel.hpp"

namespace wld {

namespace {
// f64 add into LDS / global memory by the hardware's atomic add (not a
// compare-and-swap loop); every destination is device memory of this context
__device__ __forceinline__ void lds_add(double *p, double x) {
    (void)__hip_atomic_fetch_add(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void global_add(double *p, double x) { (void)unsafeAtomicAdd(p, x); }
}  // namespace

__device__ __attribute__((always_inline)) void heatmap_epilogue(const HeatmapArgs &h, const OrderArgs &o,
                                                                const uint8_t *site_ok, uint32_t L, uint32_t a0,
                                                                uint32_t b0, uint32_t tid,
                                                                const float (&tot)[4][4][4]) {
    constexpr uint32_t G = heatmap_plan::kGridCells;
    __shared__ double sSum[G];
    __shared__ uint32_t sCnt[G];
    __shared__ uint32_t sKey[G];
    __shared__ uint32_t sCls[3];  // pairs, none, nonfinite of the tile
    const uint32_t lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
    const uint32_t ar = a0 + 16 * wave + 4 * g;  // this lane's a rows ar + i; its b columns b0 + 16 j + r

    // the tile's cell rectangle (uniform) and its regime
    const int32_t ra_lo = h.blk_lo[a0 / kTile], ra_hi = h.blk_hi[a0 / kTile];
    const int32_t cb_lo = h.blk_lo[b0 / kTile], cb_hi = h.blk_hi[b0 / kTile];
    const bool any = (ra_lo >= 0) & (ra_lo <= ra_hi) & (cb_lo >= 0) & (cb_lo <= cb_hi);
    const uint32_t Wd = any ? (uint32_t)(cb_hi - cb_lo) + 1u : 0u;
    const uint32_t rect = any ? ((uint32_t)(ra_hi - ra_lo) + 1u) * Wd : 0u;  // (<= 4096^2)
    const bool coarse = rect <= G;
    // a destination index is below this (the host's tables guarantee it; an
    // index that is not is dropped, never written through)
    const uint32_t limit = coarse ? rect : h.n_cells * h.n_cells;
    if (coarse)
        for (uint32_t k = tid; k < rect; k += 256) {
            sSum[k] = 0.0;
            sCnt[k] = 0;
            sKey[k] = heatmap_plan::kNoKey;
        }
    if (tid < 3) sCls[tid] = 0;

    // which of the lane's 16 pairs are in range and window (bit 4 i + j), the
    // site flags and the cells of its rows and columns: every load issued
    // before the sums' epilogue (a, b < LP: nothing is read past an array)
    uint32_t inr = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t a = ar + i, b = b0 + 16 * j + r;
            if ((a < b) & (b < L) & in_window(o, a, b)) inr |= 1u << (4 * i + j);
        }
    const uint32_t okA4 = *reinterpret_cast<const uint32_t *>(site_ok + ar);
    const int4 cA4 = *reinterpret_cast<const int4 *>(h.site_cell + ar);
    const int32_t cA[4] = {cA4.x, cA4.y, cA4.z, cA4.w};
    uint32_t okB = 0;
    int32_t cB[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        okB |= site_ok[b0 + 16 * j + r] ? 1u << j : 0u;
        cB[j] = h.site_cell[b0 + 16 * j + r];
    }
    __syncthreads();  // the grid and the class counts are zero

    uint32_t n_pairs = 0, n_none = 0, n_nonfin = 0;  // of the wave (uniform)
    // the lane's run of counted pairs in one cell
    uint32_t cur_cell = 0, cur_cnt = 0, cur_key = heatmap_plan::kNoKey;
    double cur_sum = 0.0;
    auto flush = [&]() {
        if (cur_cnt && cur_cell < limit) {
            if (coarse) {
                atomicAdd(&sCnt[cur_cell], cur_cnt);
                lds_add(&sSum[cur_cell], cur_sum);
                atomicMax(&sKey[cur_cell], cur_key);
            } else {
                atomicAdd(&h.count[cur_cell], (unsigned long long)cur_cnt);
                global_add(&h.sum[cur_cell], cur_sum);
                atomicMax(&h.max_key[cur_cell], cur_key);
            }
        }
        cur_cnt = 0;
        cur_sum = 0.0;
        cur_key = heatmap_plan::kNoKey;
    };
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float d, dp, r2;
            ld_epilogue(tot[i][j][0], tot[i][j][1], tot[i][j][2], tot[i][j][3], d, dp, r2);
            const float val = h.stat ? fabsf(dp) : r2;  // (uniform)
            const bool in = ((inr >> (4 * i + j)) & 1u) && cA[i] >= 0 && cB[j] >= 0;
            const bool some = ((okA4 >> (8 * i)) & 0xFFu) && ((okB >> j) & 1u);
            const bool finite = fabsf(val) <= 3.4028235e38f;  // (false for NaN)
            n_pairs += (uint32_t)__popcll(__ballot(in));
            n_none += (uint32_t)__popcll(__ballot(in && !some));
            n_nonfin += (uint32_t)__popcll(__ballot(in && some && !finite));
            if (in && some && finite) {
                const uint32_t cell = coarse ? (uint32_t)(cA[i] - ra_lo) * Wd + (uint32_t)(cB[j] - cb_lo)
                                             : (uint32_t)cA[i] * h.n_cells + (uint32_t)cB[j];
                if (cell != cur_cell) flush();
                cur_cell = cell;
                cur_cnt += 1;
                cur_sum += (double)val;
                cur_key = max(cur_key, heatmap_plan::float_key(val));
            }
        }
    }
    flush();
    if (lane == 0) {
        if (n_pairs) atomicAdd(&sCls[0], n_pairs);
        if (n_none) atomicAdd(&sCls[1], n_none);
        if (n_nonfin) atomicAdd(&sCls[2], n_nonfin);
    }
    __syncthreads();
    if (tid < 3 && sCls[tid]) atomicAdd(&h.classes[tid], (unsigned long long)sCls[tid]);
    if (coarse)
        for (uint32_t k = tid; k < rect; k += 256) {
            const uint32_t c = sCnt[k];
            if (c) {
                const size_t gi = (size_t)((uint32_t)ra_lo + k / Wd) * h.n_cells + (uint32_t)cb_lo + k % Wd;
                atomicAdd(&h.count[gi], (unsigned long long)c);
                global_add(&h.sum[gi], sSum[k]);
                atomicMax(&h.max_key[gi], sKey[k]);
            }
        }
}

void launch_pair_heatmap(const ValuLaunch &v, const OrderArgs &o, const HeatmapArgs &h, hipStream_t st) {
    if (!v.n_tiles) return;
    // one whole-tile workgroup per listed tile at every list size, as the
    // summary launches (16-row items would split a tile's cells over four
    // workgroups: four atomics per cell)
    hipLaunchKernelGGL((pair_valu_kernel<false, false, true, true, false, kReduceHeatmap>), dim3(v.n_tiles),
                       dim3(256), 0, st, v.codes, v.w, v.site_ok, v.tiles, v.n_tiles, (const unsigned *)nullptr,
                       (const uint32_t *)nullptr, (unsigned *)nullptr, (const unsigned *)nullptr, 0u, v.L, v.NP, 1u,
                       v.ref_cls / 64, v.ref_tail_n, v.n_chunk_rows, 0.0f, o, h, ScanArgs{});
}

}  // namespace wld
