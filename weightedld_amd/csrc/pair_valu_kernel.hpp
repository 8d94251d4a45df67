// f32 pair kernel: the exact-f32 path, the fallback for weights the integer
// MFMA kernel's fixed-point planes cannot hold exactly, and the reference-order
// path (WLD_OPT_REF_SUMS).  For finite weights the products and sums run on
// f32-input MFMA (MF below); the VALU loop described next is the SAFE
// (non-finite weights) path and the WLD_VALU_PLAIN=1 variant.
//
// Replaces the inner loop of single_weighted_ld_pair (lib.rs:416-480) for a
// 64x64 tile of site pairs per 256-thread workgroup.  Each thread owns a 4x4
// block of pairs (a = a0 + ty + 16i, b = b0 + tx + 16j) and keeps the four
// weighted masked sums of lib.rs:441-444 per pair in registers:
//     T   += w  where a in {maj,min} and b in {maj,min}
//     SA  += w  where additionally a == maj
//     SB  += w  where additionally b == maj
//     SAB += w  where a == maj and b == maj
// as fmaf(u, f, acc) with u = w or 0 (a side) and f = 1.0 or 0.0 (b side):
// w*1 and w*0 are exact, so each sum is an f32 sum over sequences in order
// (the same terms in the same order for all four sums, so SA == T still
// implies SAB == SB exactly and degenerate pairs stay NaN as in the
// reference).  (The SAFE variant uses selects, for non-finite weights where
// 0*inf would differ from the reference's select.)  Codes of both 64-site
// panels and the weights are staged through LDS 64 sequences at a time.
//
// Summation blocks.  acc holds the current block of 64-sequence stages, tot
// the running total:
//   * default: blocks of `flush` stages (about sqrt(N) sequences), tot += acc
//     after each (~2 sqrt(N) 2^-24 relative error, below the reference's own);
//   * REF (WLD_OPT_REF_SUMS): the reference's own f32 order, lib.rs:416-480.
//     The sequences are permuted at load (ref_layout_kernel) into the lane
//     classes of the 8-lane loop: block j (j = 0..7) holds sequences j, j+8,
//     j+16, ... < 8 floor(N/8) in order, zero padded to `cs` stages, then one
//     stage with the scalar tail (sequences 8 floor(N/8) .. N-1).  Block j's
//     chain from 0 is lane j's f32x8 sum (lib.rs:441-444: each add rounds
//     once, adding a masked-out 0 is exact); tot += acc after block j is the
//     ordered horizontal sum ((((0 + l0) + l1) + ...) + l7) that packed_simd's
//     f32x8::sum() computes on x86 (lib.rs:447-452); the <= 7 tail sequences
//     are then added onto tot one by one on the VALU, as the scalar loop adds
//     onto the horizontal sums (lib.rs:461-480).  With the epilogue op for
//     op, the rows are bit-identical to lib.rs.  Inside a class each group of
//     16 positions is stored transposed (position 4g + j holds element 4j + g
//     of the group): the MFMA's lane group g takes element 4j + g at step j,
//     so one dword read gives a lane its codes (one 16-byte read its weights)
//     for four steps.
// With LOOP the workgroup strides over a tile list whose length is known only
// on the device (the candidate tiles of the i8 screen, pair_mfma.hip), and
// the last workgroup runs the run's chunk scan (scan_tail).
//
// The kernel template lives in this header so that pair_valu.hip (the row
// kernels), pair_summary.hip, pair_heatmap.hip, pair_partners.hip,
// pair_blocks.hip, pair_annot.hip, pair_matrix.hip and pair_matrix_banded.hip (REDUCE: the same operands, sums and
// ld_epilogue, each tile reduced on chip instead of compacted into rows)
// instantiate one body: there is no second copy of the sum stages to drift.
#pragma once
#include <type_traits>

#include "pair_common.hpp"

namespace wld {

namespace {
constexpr int kStride = 68;  // LDS row stride in bytes (17 dwords: conflict-free b reads)
}

typedef float v4f __attribute__((ext_vector_type(4)));

// MF = true: the products and f32 sums of the non-SAFE path on the matrix
// cores, v_mfma_f32_16x16x4_f32 (f32 inputs, exact products, an f32 fma chain
// over k, bitwise equal to a sequential fmaf loop: MI355X_MICROARCH.md, Matrix
// cores).  Wave w owns a rows 16w..16w+15 against the tile's 64 b columns in
// four 16x16 blocks; lane l = 16g + r carries a row r (A) / b column r (B) at
// sequence kk + g, and holds the sums of pairs (a = 16w + 4g + e, b = 16n + r)
// — the same thread -> (4 a rows, 4 b columns) shape as the VALU mapping (a =
// ty + 16i), so the epilogue and compaction only change how a row slot maps
// to a.  The VALU's code extraction then overlaps the matrix pipe instead of
// competing with the FMAs for VALU issue.
#ifndef WLD_VALU_MF_WG
#define WLD_VALU_MF_WG 2  // MF: 164 VGPRs would fit 3 per CU; measured equal
#endif
#ifndef WLD_VALU_REF_WG
#define WLD_VALU_REF_WG 3  // MF + REF: three workgroups per CU (<= 168 VGPRs; 2 leave 208)
#endif
// REDUCE (MF + REF, every sub-block of every listed tile): no row is emitted;
// the tile's pairs are classified and reduced in the workgroup into the run's
// accumulators — kReduceSummary (pair_summary.hip, summary_epilogue): per
// site, per bin and total; kReduceHeatmap (pair_heatmap.hip,
// heatmap_epilogue): per cell of a site grid; kReducePartners
// (pair_partners.hip, partners_epilogue): the best candidates of every a row
// and b column staged for the merge; kReduceBreaks and kReduceBlockStats
// (pair_blocks.hip, blocks_break_epilogue / blocks_stats_epilogue): the weak
// pairs' per-site break arrays, and the statistics of the pairs inside a
// block; kReduceAnnot (pair_annot.hip, annot_epilogue): the tile's counted r2
// times the annotation tiles of its column and row sites, per site and
// annotation column; kReduceMatrix (pair_matrix.hip, matrix_epilogue): nothing
// reduced but the class counts — the tile's r2, r, d or d' stored into a
// caller's matrix, directly and transposed; kReduceMatrixBanded
// (pair_matrix_banded.hip, matrix_banded_epilogue): the same values stored once,
// into the upper band of a caller's banded matrix.  The kernel then takes
// SummaryArgs / HeatmapArgs / PartnersArgs / BlockBreakArgs / BlockStatsArgs /
// AnnotArgs / MatrixArgs / MatrixBandedArgs where the row kernels take
// DenseArgs; o gives it the window only.
constexpr int kReduceNone = 0, kReduceSummary = 1, kReduceHeatmap = 2, kReducePartners = 3;
constexpr int kReduceBreaks = 4, kReduceBlockStats = 5, kReduceAnnot = 6, kReduceMatrix = 7;
constexpr int kReduceMatrixBanded = 8;
template <int REDUCE>
struct ReduceArgsOf { using type = DenseArgs; };
template <> struct ReduceArgsOf<kReduceSummary> { using type = SummaryArgs; };
template <> struct ReduceArgsOf<kReduceHeatmap> { using type = HeatmapArgs; };
template <> struct ReduceArgsOf<kReducePartners> { using type = PartnersArgs; };
template <> struct ReduceArgsOf<kReduceBreaks> { using type = BlockBreakArgs; };
template <> struct ReduceArgsOf<kReduceBlockStats> { using type = BlockStatsArgs; };
template <> struct ReduceArgsOf<kReduceAnnot> { using type = AnnotArgs; };
template <> struct ReduceArgsOf<kReduceMatrix> { using type = MatrixArgs; };
template <> struct ReduceArgsOf<kReduceMatrixBanded> { using type = MatrixBandedArgs; };
__device__ __attribute__((always_inline)) void summary_epilogue(const SummaryArgs &s, const OrderArgs &o,
                                                                const uint8_t *site_ok, uint32_t L, uint32_t a0,
                                                                uint32_t b0, uint32_t tid,
                                                                const float (&tot)[4][4][4]);
__device__ __attribute__((always_inline)) void heatmap_epilogue(const HeatmapArgs &h, const OrderArgs &o,
                                                                const uint8_t *site_ok, uint32_t L, uint32_t a0,
                                                                uint32_t b0, uint32_t tid,
                                                                const float (&tot)[4][4][4]);
__device__ __attribute__((always_inline)) void partners_epilogue(const PartnersArgs &p, const OrderArgs &o,
                                                                 const uint8_t *site_ok, uint32_t L, uint32_t a0,
                                                                 uint32_t b0, uint32_t tid, float thr,
                                                                 const float (&tot)[4][4][4]);
__device__ __attribute__((always_inline)) void blocks_break_epilogue(const BlockBreakArgs &k, const OrderArgs &o,
                                                                     const uint8_t *site_ok, uint32_t L, uint32_t a0,
                                                                     uint32_t b0, uint32_t tid,
                                                                     const float (&tot)[4][4][4]);
__device__ __attribute__((always_inline)) void blocks_stats_epilogue(const BlockStatsArgs &k, const OrderArgs &o,
                                                                     const uint8_t *site_ok, uint32_t L, uint32_t a0,
                                                                     uint32_t b0, uint32_t tid,
                                                                     const float (&tot)[4][4][4]);
__device__ __attribute__((always_inline)) void annot_epilogue(const AnnotArgs &k, const OrderArgs &o,
                                                              const uint8_t *site_ok, uint32_t L, uint32_t a0,
                                                              uint32_t b0, uint32_t tid,
                                                              const float (&tot)[4][4][4]);
__device__ __attribute__((always_inline)) void matrix_epilogue(const MatrixArgs &m, const OrderArgs &o,
                                                               const uint8_t *site_ok, uint32_t L, uint32_t a0,
                                                               uint32_t b0, uint32_t tid,
                                                               const float (&tot)[4][4][4]);
__device__ __attribute__((always_inline)) void matrix_banded_epilogue(const MatrixBandedArgs &m, const OrderArgs &o,
                                                                      const uint8_t *site_ok, uint32_t L, uint32_t a0,
                                                                      uint32_t b0, uint32_t tid,
                                                                      const float (&tot)[4][4][4]);
template <bool DENSE, bool SAFE, bool MF, bool REF, bool LOOP, int REDUCE = kReduceNone>
__global__ __launch_bounds__(256, MF ? (REF ? WLD_VALU_REF_WG : WLD_VALU_MF_WG) : 2) void pair_valu_kernel(
    const uint8_t *__restrict__ codes, const float *__restrict__ w, const uint8_t *__restrict__ site_ok,
    const uint32_t *__restrict__ tiles, uint32_t n_tiles, const unsigned *tile_count,
    const uint32_t *__restrict__ tile_bits, unsigned *tile_work, const unsigned *tile_buckets, uint32_t bucket_cap,
    uint32_t L, uint32_t NP, uint32_t flush,
    uint32_t ref_cs, uint32_t ref_tail_n, uint32_t n_chunk_rows, float thr, OrderArgs o,
    typename ReduceArgsOf<REDUCE>::type dn,
    ScanArgs sa) {
    static_assert(!REDUCE || (MF && REF && !SAFE && !DENSE && !LOOP), "the reductions run lib.rs's order on f32 MFMA");
    constexpr int NS = 4;  // 16x16 slots per wave: a whole 64x64 tile per workgroup
    __shared__ __attribute__((aligned(16))) uint8_t sA[kTile * kStride];
    __shared__ __attribute__((aligned(16))) uint8_t sB[kTile * kStride];
    __shared__ __attribute__((aligned(16))) float sW[64];
    __shared__ unsigned long long sBits[kTile];  // compaction: passing b per a row
    __shared__ uint32_t sRowBase[kTile];

    // bits: the 16x16 sub-blocks whose pairs are computed (bit 4 (a / 16) +
    // b / 16); the others' pairs provably fail (the screen's bound).  owned:
    // the tile's 16-row blocks whose segment counts this work item writes (a
    // tile split over several items gives each its own row blocks)
    auto compute_tile = [&](uint32_t tile, uint32_t tid, uint32_t bits, uint32_t owned) {
        const uint32_t ta = tile >> 16, tb = tile & 0xFFFFu;
        const uint32_t a0 = ta * kTile, b0 = tb * kTile;
        const uint32_t tx = tid & 15, ty = tid >> 4;

        float acc[4][4][4], tot[4][NS][4];
        v4f accM[NS][4];  // MF: [slot j][sum q], element e = a row slot
        // MF + REF: the computed sub-blocks dealt over the waves.  In
        // column-major order (k = 4 n + i: a rows 16 i.., b columns 16 n..)
        // the u-th computed one goes to wave u % 4, slot u / 4: the stage
        // barriers pace a tile by its busiest wave, and a diagonal tile's 10
        // sub-blocks then take 3 slots on it instead of 4; all 16 give wave w
        // the a rows 16 w.. against b block j in slot j.
        uint32_t ui[NS], un[NS];
        bool us[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) ui[j] = 0, un[j] = j, us[j] = true;
        if constexpr (MF && REF) {
            const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
            uint32_t cm = 0;
            for (uint32_t k = 0; k < 16; ++k) cm |= ((bits >> (4 * (k & 3) + (k >> 2))) & 1u) << k;
            cm = __builtin_amdgcn_readfirstlane(cm);
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                uint32_t m = cm;
                for (uint32_t t = 0; t < 4 * (uint32_t)j + wave; ++t) m &= m - 1u;  // drop the first 4j + w
                const uint32_t k = m ? (uint32_t)__builtin_ctz(m) : 0u;
                us[j] = m != 0;
                ui[j] = k & 3u;
                un[j] = k >> 2;
            }
        }
        // the tile's a row / b column of this thread's pair (row slot i, slot j)
        auto pa = [&](int i, int j) -> uint32_t {
            if constexpr (MF && REF) return 16 * ui[j] + 4 * (ty & 3) + i;
            else return MF ? 4 * ty + i : ty + 16 * i;
        };
        auto pb = [&](int i, int j) -> uint32_t {
            if constexpr (MF && REF) return 16 * un[j] + tx;
            else return tx + 16 * j;
        };
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) tot[i][j][q] = 0.0f;

        const uint32_t lr = tid >> 2, part = tid & 3;  // loader: site row, 16-byte part
        const uint8_t *gA = codes + (size_t)(a0 + lr) * NP + part * 16;
        const uint8_t *gB = codes + (size_t)(b0 + lr) * NP + part * 16;

        // one 64-sequence stage of both panels' codes and the weights: fetch
        // (global loads into registers, issued a stage ahead so that their
        // latency overlaps the previous stage's MFMAs), then store (into LDS).
        // PF: the fetch a stage ahead; a whole tile per workgroup in lib.rs's
        // order has no registers to spare for it (it would spill), and fetches
        // each stage just before storing it
        constexpr bool PF = !REF;
        uint4 va, vb;
        float wv;
        auto fetch_stage = [&](uint32_t k0) {
            va = *reinterpret_cast<const uint4 *>(gA + k0);
            vb = *reinterpret_cast<const uint4 *>(gB + k0);
            wv = tid < 64 ? w[k0 + tid] : 0.0f;
        };
        auto store_stage = [&]() {
            __syncthreads();
            uint32_t *pa = reinterpret_cast<uint32_t *>(sA + lr * kStride + part * 16);
            uint32_t *pb = reinterpret_cast<uint32_t *>(sB + lr * kStride + part * 16);
            pa[0] = va.x, pa[1] = va.y, pa[2] = va.z, pa[3] = va.w;
            pb[0] = vb.x, pb[1] = vb.y, pb[2] = vb.z, pb[3] = vb.w;
            if (tid < 64) sW[tid] = wv;
            __syncthreads();
        };
        // the staged 64 sequences into acc (VALU) / accM (MF), in sequence order
        auto compute_stage = [&]() {
            if constexpr (MF && REF) {
                // transposed 16-position groups: lane (r, g) reads the dword of
                // its row at 16 grp + 4 g = elements 16 grp + 4 e + g, e = 0..3;
                // slot j (a rows 16 ui[j].., b block un[j]) runs its 16 MFMAs of
                // the group when the wave holds it (us[j], wave-uniform)
                const uint32_t lane = tid & 63, r = lane & 15, g = lane >> 4;
#pragma unroll
                for (int grp = 0; grp < 4; ++grp) {
                    const float4 w4 = *reinterpret_cast<const float4 *>(sW + 16 * grp + 4 * g);
                    const float we[4] = {w4.x, w4.y, w4.z, w4.w};
                    float u[4], v[4];
#pragma unroll
                    for (int j = 0; j < NS; ++j) {
                        if (!us[j]) continue;  // (slots fill in order: us[j] implies us[j - 1])
                        if (j == 0 || ui[j] != ui[j - 1]) {  // a rows of a new row block (all 16: slot 0 only)
                            const uint32_t a4 =
                                *reinterpret_cast<const uint32_t *>(sA + (16 * ui[j] + r) * kStride + 4 * g + 16 * grp);
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const uint32_t ca = a4 >> (8 * e);
                                u[e] = (ca & kCodeIn) ? we[e] : 0.0f;
                                v[e] = (ca & kCodeMaj) ? we[e] : 0.0f;
                            }
                        }
                        const uint32_t b4 =
                            *reinterpret_cast<const uint32_t *>(sB + (16 * un[j] + r) * kStride + 4 * g + 16 * grp);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float fi = (float)((b4 >> (8 * e)) & 1u), fm = (float)((b4 >> (8 * e + 1)) & 1u);
                            accM[j][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[e], fi, accM[j][0], 0, 0, 0);
                            accM[j][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[e], fi, accM[j][1], 0, 0, 0);
                            accM[j][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[e], fm, accM[j][2], 0, 0, 0);
                            accM[j][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[e], fm, accM[j][3], 0, 0, 0);
                        }
                    }
                }
            } else if constexpr (MF) {
                const uint32_t lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
                const uint8_t *rowA = sA + (16 * wave + r) * kStride + g;
                const uint8_t *rowB = sB + r * kStride + g;
#pragma unroll 4
                for (int kk = 0; kk < 64; kk += 4) {
                    const float we = sW[kk + g];
                    const uint32_t ca = rowA[kk];
                    const float u = (ca & kCodeIn) ? we : 0.0f;
                    const float v = (ca & kCodeMaj) ? we : 0.0f;
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        const uint32_t cb = rowB[16 * n * kStride + kk];
                        const float fi = (float)(cb & 1u), fm = (float)(cb >> 1);
                        accM[n][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(u, fi, accM[n][0], 0, 0, 0);
                        accM[n][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v, fi, accM[n][1], 0, 0, 0);
                        accM[n][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(u, fm, accM[n][2], 0, 0, 0);
                        accM[n][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(v, fm, accM[n][3], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll 2
                for (int kk = 0; kk < 64; kk += 4) {
                    uint32_t A[4], B[4];
                    float wk[4];
                    if constexpr (REF) {
                        // elements kk + e (e = 0..3) of the transposed group
                        // sit at 16 (kk / 16) + 4 e + (kk % 16) / 4
                        const int p0 = 16 * (kk / 16) + (kk % 16) / 4;
                        auto gather = [&](const uint8_t *row) {
                            return (uint32_t)row[p0] | (uint32_t)row[p0 + 4] << 8 | (uint32_t)row[p0 + 8] << 16 |
                                   (uint32_t)row[p0 + 12] << 24;
                        };
#pragma unroll
                        for (int i = 0; i < 4; ++i) A[i] = gather(sA + (ty + 16 * i) * kStride);
#pragma unroll
                        for (int j = 0; j < 4; ++j) B[j] = gather(sB + (tx + 16 * j) * kStride);
#pragma unroll
                        for (int e = 0; e < 4; ++e) wk[e] = sW[p0 + 4 * e];
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            A[i] = *reinterpret_cast<const uint32_t *>(sA + (ty + 16 * i) * kStride + kk);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            B[j] = *reinterpret_cast<const uint32_t *>(sB + (tx + 16 * j) * kStride + kk);
                        const float4 w4 = *reinterpret_cast<const float4 *>(sW + kk);
                        wk[0] = w4.x; wk[1] = w4.y; wk[2] = w4.z; wk[3] = w4.w;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float we = wk[e];
                        float u[4], v[4];
                        uint32_t ca[4], cb[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            ca[i] = (A[i] >> (8 * e)) & 3u;
                            u[i] = (ca[i] & kCodeIn) ? we : 0.0f;
                            v[i] = (ca[i] & kCodeMaj) ? we : 0.0f;
                        }
#pragma unroll
                        for (int j = 0; j < 4; ++j) cb[j] = (B[j] >> (8 * e)) & 3u;
                        if constexpr (!SAFE) {
                            float fi[4], fm[4];
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                fi[j] = (float)(cb[j] & 1u);
                                fm[j] = (float)(cb[j] >> 1);
                            }
#pragma unroll
                            for (int i = 0; i < 4; ++i)
#pragma unroll
                                for (int j = 0; j < 4; ++j) {
                                    acc[i][j][0] = __builtin_fmaf(u[i], fi[j], acc[i][j][0]);
                                    acc[i][j][1] = __builtin_fmaf(v[i], fi[j], acc[i][j][1]);
                                    acc[i][j][2] = __builtin_fmaf(u[i], fm[j], acc[i][j][2]);
                                    acc[i][j][3] = __builtin_fmaf(v[i], fm[j], acc[i][j][3]);
                                }
                        } else {
#pragma unroll
                            for (int i = 0; i < 4; ++i)
#pragma unroll
                                for (int j = 0; j < 4; ++j) {
                                    const bool bi = cb[j] & 1u, bm = cb[j] & 2u;
                                    acc[i][j][0] += bi ? u[i] : 0.0f;
                                    acc[i][j][1] += bi ? v[i] : 0.0f;
                                    acc[i][j][2] += bm ? u[i] : 0.0f;
                                    acc[i][j][3] += bm ? v[i] : 0.0f;
                                }
                        }
                    }
                }
            }
        };
        // block start: acc = 0; block end: tot += acc
        auto acc_zero = [&]() {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NS; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if constexpr (MF) accM[j][q][i] = 0.0f;
                        else acc[i][j][q] = 0.0f;
                    }
        };
        auto acc_fold = [&]() {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NS; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) tot[i][j][q] += MF ? accM[j][q][i] : acc[i][j][q];
        };

        if constexpr (REF) {
            // the eight lane classes, each a chain from 0 folded into the
            // ordered horizontal sum; then the tail stage on that sum.  The
            // stages are consecutive (class c's are [c cls, (c + 1) cls), the
            // tail's 8 cls), so each stage's fetch is issued before the
            // previous stage's compute.
            const uint32_t cls = 64 * ref_cs;
            if (PF && (ref_cs || ref_tail_n)) fetch_stage(0);
            for (uint32_t c = 0; c < (ref_cs ? 8u : 0u); ++c) {
                acc_zero();
                for (uint32_t k0 = c * cls; k0 < (c + 1) * cls; k0 += 64) {
                    if (!PF) fetch_stage(k0);
                    store_stage();
                    if (PF && (k0 + 64 < 8 * cls || ref_tail_n)) fetch_stage(k0 + 64);
                    compute_stage();
                }
                acc_fold();
            }
            if (ref_tail_n) {
                // the scalar tail (lib.rs:461-480): its <= 7 sequences added
                // onto the horizontal sums one by one, in order, on the VALU
                // (fmaf(u, f, tot) = tot + u f rounded once: u f is exact)
                if (!PF) fetch_stage(8 * cls);
                store_stage();
                for (uint32_t t = 0; t < ref_tail_n; ++t) {
                    const float we = sW[t];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < NS; ++j) {
                            const uint32_t ca = sA[pa(i, j) * kStride + t], cb = sB[pb(i, j) * kStride + t];
                            const float u = (ca & kCodeIn) ? we : 0.0f;
                            const float v = (ca & kCodeMaj) ? we : 0.0f;
                            if constexpr (!SAFE) {
                                const float fi = (float)(cb & 1u), fm = (float)(cb >> 1);
                                tot[i][j][0] = __builtin_fmaf(u, fi, tot[i][j][0]);
                                tot[i][j][1] = __builtin_fmaf(v, fi, tot[i][j][1]);
                                tot[i][j][2] = __builtin_fmaf(u, fm, tot[i][j][2]);
                                tot[i][j][3] = __builtin_fmaf(v, fm, tot[i][j][3]);
                            } else {
                                const bool bi = cb & 1u, bm = cb & 2u;
                                tot[i][j][0] += bi ? u : 0.0f;
                                tot[i][j][1] += bi ? v : 0.0f;
                                tot[i][j][2] += bm ? u : 0.0f;
                                tot[i][j][3] += bm ? v : 0.0f;
                            }
                        }
                }
            }
        } else {
            // blocks of `flush` stages
            fetch_stage(0);
            for (uint32_t k0 = 0; k0 < NP; k0 += 64 * flush) {
                acc_zero();
                for (uint32_t k1 = k0; k1 < min(NP, k0 + 64 * flush); k1 += 64) {
                    store_stage();
                    if (k1 + 64 < NP) fetch_stage(k1 + 64);
                    compute_stage();
                }
                acc_fold();
            }
        }

        if constexpr (REDUCE != kReduceNone) {
            // (bits 0xFFFF: wave w holds a rows 16 w + 4 g + i against b column
            // 16 j + r in tot[i][j], the mapping the reducing epilogues assume)
            if constexpr (REDUCE == kReduceSummary) summary_epilogue(dn, o, site_ok, L, a0, b0, tid, tot);
            else if constexpr (REDUCE == kReduceHeatmap) heatmap_epilogue(dn, o, site_ok, L, a0, b0, tid, tot);
            else if constexpr (REDUCE == kReducePartners) partners_epilogue(dn, o, site_ok, L, a0, b0, tid, thr, tot);
            else if constexpr (REDUCE == kReduceBreaks) blocks_break_epilogue(dn, o, site_ok, L, a0, b0, tid, tot);
            else if constexpr (REDUCE == kReduceBlockStats) blocks_stats_epilogue(dn, o, site_ok, L, a0, b0, tid, tot);
            else if constexpr (REDUCE == kReduceAnnot) annot_epilogue(dn, o, site_ok, L, a0, b0, tid, tot);
            else if constexpr (REDUCE == kReduceMatrix) matrix_epilogue(dn, o, site_ok, L, a0, b0, tid, tot);
            else matrix_banded_epilogue(dn, o, site_ok, L, a0, b0, tid, tot);
            return;
        }
        // ---- epilogue ------------------------------------------------------
        uint32_t passmask[4] = {0, 0, 0, 0};  // bit j per row slot i
        float res[4][NS][3];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                const uint32_t al = pa(i, j), bl = pb(i, j), a = a0 + al, b = b0 + bl;
                float d, dp, r2;
                ld_epilogue(tot[i][j][0], tot[i][j][1], tot[i][j][2], tot[i][j][3], d, dp, r2);
                res[i][j][0] = d;
                res[i][j][1] = dp;
                res[i][j][2] = r2;
                // (every load issued, no short-circuit: a, b < LP; the compiler
                // batches them instead of one round trip per pair)
                const bool valid = (a < b) & (b < L) & ((site_ok[a] & site_ok[b]) != 0);
                if constexpr (DENSE) {
                    if (a < b && b < L) {
                        const size_t k = (size_t)a * L + b;
                        dn.d[k] = d;
                        dn.dp[k] = dp;
                        dn.r2[k] = r2;
                        dn.valid[k] = valid ? 1 : 0;
                    }
                } else {
                    // lib.rs:660 strict '>' (a skipped sub-block's pairs provably fail;
                    // an empty slot's pairs alias slot 0's sub-block)
                    if (valid && r2 > thr && us[j] && ((bits >> (4 * (al >> 4) + (bl >> 4))) & 1u) &&
                        in_window(o, a, b))
                        passmask[i] |= 1u << j;
                }
            }
        }
        if constexpr (DENSE) return;

        // ---- compaction: a 64x64 pass-bit matrix in LDS, rows in b order ----
        // (a tile with no passing pair writes only its 64 zero counts)
        const bool own_row = tid < kTile && ((owned >> (tid >> 4)) & 1u);  // (row tid: its 16-row block)
        const uint32_t quarters = (uint32_t)__popc(owned);
        if (!__syncthreads_or((passmask[0] | passmask[1] | passmask[2] | passmask[3]) != 0)) {
            if (own_row) o.seg_cnt[(size_t)(a0 + tid) * o.T + tb] = 0;
            if (tid == 0) tile_done(o, ta, tb, n_chunk_rows, quarters);
            return;
        }
        if (tid < kTile) sBits[tid] = 0ull;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j)
                if (passmask[i] & (1u << j)) atomicOr(&sBits[pa(i, j)], 1ull << pb(i, j));
        __syncthreads();
        if (tid < kTile) {
            const uint32_t r = tid;
            const uint32_t cnt = __popcll(sBits[r]);
            const uint32_t incl = wave_inclusive_scan(cnt);
            const uint32_t excl = incl - cnt;
            const uint32_t total = __shfl(incl, 63, 64);
            unsigned long long base = 0;
            if (r == 63 && total) base = atomicAdd(o.cursor, (unsigned long long)total);
            base = __shfl(base, 63, 64);
            sRowBase[r] = (uint32_t)base + excl;
            const uint32_t a = a0 + r;
            if (own_row) {  // (a row outside the item's blocks has no pass: cnt 0)
                o.seg_cnt[(size_t)a * o.T + tb] = (uint8_t)cnt;
                o.seg_off[(size_t)a * o.T + tb] = (uint32_t)base + excl;
            }
            if (r == 63 && total)
                atomicAdd(&o.chunk_total[chunk_linear(n_chunk_rows, ta / kTilesPerChunk, tb / kTilesPerChunk)], total);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!passmask[i]) continue;
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                if (!(passmask[i] & (1u << j))) continue;
                const uint32_t al = pa(i, j), bl = pb(i, j);
                const uint64_t pos = (uint64_t)sRowBase[al] + __popcll(sBits[al] & ((1ull << bl) - 1ull));
                if (pos < o.st_capacity) {
                    o.st_a[pos] = a0 + al;
                    o.st_b[pos] = b0 + bl;
                    o.st_d[pos] = res[i][j][0];
                    o.st_dp[pos] = res[i][j][1];
                    o.st_r2[pos] = res[i][j][2];
                }
            }
        }
        if (tid == 0) tile_done(o, ta, tb, n_chunk_rows, quarters);
    };

    if constexpr (!LOOP) {
        const uint32_t tile = tiles[blockIdx.x];
        if constexpr (REDUCE == kReducePartners) {
            // (the tile addresses the staging's parts: checked like a candidate entry's)
            if (tile != kNoTile && !tile_in_range(tile, L)) {
                if (threadIdx.x == 0) atomicOr(dn.guard, kPartnersGuardTile);
                return;
            }
        }
        if (tile != kNoTile)  // kNoTile: padding of an XCD-ordered list
            compute_tile(tile, threadIdx.x, 0xFFFFu, 0xFu);
    } else {
        // (the list entries come from the screen's atomics: each is checked —
        // bucket slot, then the tile — before anything is read through it)
        // the first tile by workgroup id, the next ones from a work counter
        // (tile_work, zeroed by the screen): the workgroups that finish first
        // take the list's tail, not fixed ones (tiles differ in their computed
        // sub-blocks)
        __shared__ uint32_t s_next, s_pre[17];
        const uint32_t nt = (*tile_count & kAbandonBit) ? 0u : *tile_count;
        // first items: the list is heaviest first and the dispatcher deals
        // workgroups i, i + m, i + 2m, ... (m = grid / R, R resident per CU)
        // to one CU, so that CU would start R of the heaviest items at once
        // (one wave of each on every SIMD): deal the rounds in snake order
        // instead (j, 2m - 1 - j, 2m + j, ...), heavy next to light (a
        // permutation of [0, grid))
        uint32_t first = blockIdx.x;
        if (tile_buckets) {
            constexpr uint32_t R = WLD_VALU_REF_WG;
            const uint32_t m = gridDim.x / R, k = m ? blockIdx.x / m : R, j = blockIdx.x - (k < R ? k * m : 0u);
            if (k < R) first = (k & 1) ? (k + 1) * m - 1 - j : k * m + j;
        }
        if (tile_buckets && first < nt) cand_prefix(tile_buckets, s_pre);  // (a workgroup without a tile skips it)
        for (uint32_t bi = first; bi < nt;) {
            const uint32_t e = tile_buckets ? cand_entry_checked(o, s_pre, bucket_cap, bi) : bi < n_tiles ? bi : ~0u;
            const uint32_t tile = e != ~0u ? tiles[e] : kNoTile;
            // (a refused entry reads nothing through e: the guard has reported it)
            const uint32_t bits = tile_bits && e != ~0u ? tile_bits[e] : 0xFFFFu;
            if (tile_in_range(tile, L))
                compute_tile(tile, threadIdx.x, bits, 0xFu);  // (a whole-tile entry writes all 64 rows' segments)
            else if (e != ~0u && threadIdx.x == 0)
                report_guard(o, kGuardTile);
            if (threadIdx.x == 0) s_next = gridDim.x + atomicAdd(tile_work, 1u);
            __syncthreads();  // (also: the next tile's staging and compaction reuse the LDS)
            bi = s_next;
            __syncthreads();
        }
        scan_tail(sa, nt, false, first);
    }
}

}  // namespace wld
