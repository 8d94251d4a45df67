// Device-side layout and launchers shared by capi.hip and the kernel files.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "matrix_banded_plan.hpp"
#include "matrix_plan.hpp"
#include "screen_policy.hpp"

namespace wld {

// ---- layout constants (see DESIGN.md "Data layout in HBM") ----
constexpr int kChunk = 256;      // reference chunk side, lib.rs:615
constexpr int kTile = 64;        // pair-kernel tile side (sites); 4 tiles per chunk side
constexpr int kSeqPad = 64;      // sequences padded to a multiple of this
constexpr int kTilesPerChunk = kChunk / kTile;
// an empty slot of a reordered tile list (never a real tile: T_used < 65535 there)
constexpr uint32_t kNoTile = 0xFFFFFFFFu;

// Code byte per (site, sequence): bit0 = sequence is major or minor at the site
// ("in" the pair mask, lib.rs:435), bit1 = sequence is major (lib.rs:430,432).
constexpr uint8_t kCodeIn = 1;
constexpr uint8_t kCodeMaj = 2;

struct OrderArgs {
    // staging written by the pair kernels (filtered indices, unordered tiles)
    uint32_t *st_a, *st_b;
    float *st_d, *st_dp, *st_r2;
    uint64_t st_capacity;
    // per (site a, 64-wide b tile) segment: count (<= 64) and staging offset
    uint8_t *seg_cnt;   // [LP][T]
    uint32_t *seg_off;  // [LP][T]
    uint32_t T;         // number of 64-wide tiles (LP / 64)
    uint32_t *chunk_total;  // [n_chunks_total] rows per reference chunk (linear triu index)
    unsigned long long *cursor;  // staging allocation cursor
    // per-chunk progress (lib.rs:670-674; wld_run_host with a callback, else
    // null): tiles left per linear chunk; the workgroup that finishes a
    // chunk's last tile appends the chunk's pair count to the mapped host log
    // at slot atomicAdd(prog_n, 1) (tile_done, pair_common.hpp)
    unsigned *chunk_left;
    unsigned *prog_n;
    unsigned long long *prog_log;
    uint32_t L;  // sites of the loaded set (a chunk's pair count)
    // guard word in mapped host memory (report_guard): a kernel that finds an
    // index out of range (a candidate-list entry, a tile, a staged pair, a
    // gather destination) records what it found here and skips the access
    // instead of faulting the context; run_complete turns it into WLD_E_STATE
    unsigned *guard;
    // the run's window (wld_set_window; both null without one): win_hi[a] =
    // the last in-window partner of site a ([LP], a itself where it has none
    // and for padding sites), and the in-window pair count of every linear
    // chunk (what tile_done logs instead of the chunk's geometric count)
    const uint32_t *win_hi;
    const uint32_t *win_pairs;
};

// report_guard bits (wld_run_stats.guard and the WLD_E_STATE message)
enum : unsigned {
    kGuardEntry = 1u,   // a candidate-list entry outside the list's buckets
    kGuardTile = 2u,    // a listed tile with ta > tb or tb past the set's last tile
    kGuardPair = 4u,    // a staged candidate pair with a >= b or b past the set
    kGuardSlice = 8u,   // a candidate slice outside staging or with a bad tile
    kGuardGather = 16u  // a gather destination past the run's row count, or a source past staging
};
__device__ inline void report_guard(const OrderArgs &o, unsigned bit) {
    if (o.guard) __hip_atomic_store(o.guard, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// The window's part of every row-emitting kernel's pass test: b is one of a's
// in-window partners (a < b given; a < LP).  Uniform branch; no window, no load.
__device__ __forceinline__ bool in_window(const OrderArgs &o, uint32_t a, uint32_t b) {
    return !o.win_hi || b <= o.win_hi[a];
}
// a tile (ta << 16 | tb) the pair kernels may compute: ta <= tb < T_used
__device__ inline bool tile_in_range(uint32_t tile, uint32_t L) {
    const uint32_t ta = tile >> 16, tb = tile & 0xFFFFu;
    return ta <= tb && (uint64_t)tb * kTile < L;
}

// The run's chunk scan (order.hip): exclusive scan of the chunk totals
// [lin_begin, lin_begin + count) into chunk_base; the row total into *total,
// *count_out (may be null) and host_out[1], the staging cursor into
// host_out[0], the candidate-tile count cand_count[0] into host_out[2] and
// their computed 16x16 sub-blocks cand_count[1] into host_out[3], *rechecked
// (with rechecked[1] in the upper half) into host_out[5] (host_out: mapped pinned memory, may be null); cursor, the chunk totals and both
// candidate counts are left at 0 for the next run.  With ticket set, the last
// workgroup of the candidate launch after a screen runs it (scan_tail,
// pair_common.hpp) instead of a launch of its own.
struct ScanArgs {
    uint32_t *chunk_total;
    uint32_t lin_begin, count;
    uint32_t *chunk_base;
    unsigned long long *total, *cursor, *host_out, *count_out;
    unsigned long long *cursor_seen;  // device word: the staging cursor before its reset (may be null)
    unsigned *cand_count;  // this pass's {candidate tiles, their candidate sub-blocks} (read)
    // the OTHER candidate set (the next pass's: {count, sub-blocks} and 16
    // bucket counts), zeroed here; this pass's set is never written by its
    // own scan, so a workgroup still reading it cannot see it reset (capi.hip
    // enqueue_pass alternates the sets by pass parity)
    unsigned *cand_reset;
    unsigned *cand_buckets_reset;
    unsigned *ticket;  // 0 between launches; null: the scan is launched on its own
    // the fp6 screen's count of entries that formed the fourth sum (may be
    // null) and, in the word after it, of the row blocks its quick test did
    // not reject: into host_out[5] (lower and upper half), and back to 0 for
    // the next pass
    unsigned *rechecked = nullptr;
};

// 64-bit words of a context's run counters (capi.hip enqueue_pass):
// {cursor, total, {ticket, work}, set 0: {candidates, sub-blocks} + 16 bucket
// counts (9 words), set 1: the same, the cursor the scan saw, the fp6
// screen's entries that formed the fourth sum (lower half) and row blocks
// its quick test did not reject (upper half)}
constexpr uint32_t kCounterWords = 23;
constexpr uint32_t kCursorSeen = 21;
constexpr uint32_t kF6Rechecked = 22;
// set on a pass's candidate count and on its bucket 0 by a screen that gave
// up (the fp6 screen past ScreenArgs::bail candidates): the candidate launch
// then computes nothing, the scan reports the count with the bit to the host
// (which re-runs the pass on the i8 screen) and a cursor the gather enqueued
// behind it refuses
constexpr unsigned kAbandonBit = 0x80000000u;
constexpr uint32_t kCandSetWords = 9;
constexpr uint32_t kCandSet0 = 3;

struct DenseArgs {
    float *d, *dp, *r2;
    uint8_t *valid;
};

// The accumulators of a summary run (pair_summary.hip; wld_run_summary): all
// zero before the launch, added to by at most one atomic per destination and
// tile.  counts = {pairs, none, nonfinite, counted}; score/partners have LP
// entries; the bin arrays n_bins (bin_width 0: no bins, both null).  pos: the
// resident site_map (L entries; null: pos[i] = i), read only with bins.
struct SummaryArgs {
    unsigned long long *counts;
    double *r2_sum;
    double *score;
    uint32_t *partners;
    unsigned long long *bin_pairs;
    double *bin_r2_sum;
    const uint32_t *pos;
    uint64_t bin_width;
    uint32_t n_bins;
};

// The accumulators of a heat-map run (pair_heatmap.hip; wld_run_heatmap): all
// zero before the launch (a max key of 0 lies below every finite value's,
// heatmap_plan.hpp).  classes = {pairs, none, nonfinite}, one atomic each per
// tile; count/sum/max_key have n_cells x n_cells entries, row-major.
// site_cell: LP entries, -1 for a site on no cell and for padding; blk_lo /
// blk_hi: per 64-site block the cells of its first and last site with a cell
// (lo > hi: none), LP / 64 entries.  stat: WLD_HEAT_R2 / WLD_HEAT_ABS_DPRIME.
struct HeatmapArgs {
    unsigned long long *classes;
    unsigned long long *count;
    double *sum;
    uint32_t *max_key;
    const int32_t *site_cell;
    const int32_t *blk_lo, *blk_hi;
    uint32_t n_cells;
    int stat;
};

// Pass 1 of the LD blocks (pair_blocks.hip blocks_break_epilogue;
// wld_run_block_breaks).  classes = {pairs, none, nonfinite, strong, weak},
// zero before the launch, one atomic each per tile.  fwd_weak: LP entries,
// 0xFFFFFFFF before the launch, atomicMin of b over the weak pairs (a, b).
// bwd_weak1: LP entries, zero before the launch, atomicMax of a + 1 over the
// weak pairs (a, b) (0: none; the host takes the 1 off).  stat:
// WLD_BLOCKS_R2 / WLD_BLOCKS_ABS_DPRIME.
struct BlockBreakArgs {
    unsigned long long *classes;
    uint32_t *fwd_weak;
    uint32_t *bwd_weak1;
    int stat;
    float strong_min;
};

// Pass 2 of the LD blocks (pair_blocks.hip blocks_stats_epilogue;
// wld_blocks_from_breaks): per reported block, all zero before the launch,
// the considered pairs whose two sites carry its id (pairs), the informative
// and the strong ones, the f64 sum of the informative values and the largest
// blocks_plan::inv_key of them (0: none).  site_block: LP entries, -1 for a
// site in no block and for padding; blk_lo / blk_hi: per 64-site block the ids
// of its first and last site with one (lo > hi: none), LP / 64 entries.
struct BlockStatsArgs {
    unsigned long long *pairs, *informative, *strong;
    double *sum;
    uint32_t *min_key;
    const int32_t *site_block;
    const int32_t *blk_lo, *blk_hi;
    uint32_t n_blocks;
    int stat;
    float strong_min;
};

// The accumulators and operands of a partitioned-score run (pair_annot.hip;
// wld_run_annot_scores; annot_plan.hpp builds the image and the mask).
// counts = {pairs, none, nonfinite, counted}, score [LP][CP] and partners [LP]
// are zero before the launch; a tile adds to a destination with at most one
// atomic.  annot: the padded image [LP][CP] (CP a multiple of 16; zero past the
// loaded sites and the caller's columns); zero: per (64-site tile, 16-column
// chunk) [tile * (CP / 16) + chunk], 1 where the image holds only zeros.
struct AnnotArgs {
    unsigned long long *counts;
    double *score;
    uint32_t *partners;
    const float *annot;
    const uint8_t *zero;
    uint32_t CP;
};

// The destination of a dense LD matrix launch (pair_matrix.hip;
// wld_run_matrix_device / wld_run_matrix; matrix_plan.hpp lists the tiles and
// the fill blocks).  dst: the element of entry (band.r0, band.c0), ld elements
// per row, float (f16 false) or IEEE binary16; only entries inside band are
// written, by plain stores.  full: the call's rectangle, of which band is a
// range of whole rows (the counting rule, matrix_plan::counts_here).  counts =
// {pairs, none, nonfinite, counted}, zero before the launch, one atomic each
// per tile.  stat: WLD_MATRIX_*; zero_missing: WLD_MATRIX_ZERO_MISSING.
struct MatrixArgs {
    void *dst;
    size_t ld;
    matrix_plan::Rect full, band;
    int stat;
    bool f16, zero_missing;
    unsigned long long *counts;
};

// The destination of a banded LD matrix launch (pair_matrix_banded.hip;
// wld_run_matrix_banded_device / wld_run_matrix_banded; matrix_banded_plan.hpp
// lists the tiles and the fill blocks).  dst: the element k = 0 of row r0, ld
// elements per row, float (f16 false) or IEEE binary16; element k of row u is
// entry (u, u + k); only the elements k <= K of the rows [r0, r1) are written,
// by plain stores.  counts = {pairs, none, nonfinite, counted} of the in-window
// pairs a < b with a in [r0, r1), zero before the launch, one atomic each per
// tile.  stat: WLD_MATRIX_*; zero_missing: WLD_MATRIX_ZERO_MISSING.
struct MatrixBandedArgs {
    void *dst;
    size_t ld;
    uint32_t r0, r1, K;
    int stat;
    bool f16, zero_missing;
    unsigned long long *counts;
};

// The operands of a band product (banded_apply.hip; wld_banded_apply_device):
// Y[n][ldy] f64 := S X, S the symmetric matrix whose upper band (elements k =
// 0..K of every row, ld apart, float or binary16) is `band`, X[n][ldx] float
// (x64 false) or double, n_cols columns.
struct BandedApplyArgs {
    const void *band;
    size_t ld;
    uint32_t n, K;
    bool band_f16, x64;
    const void *x;
    size_t ldx;
    uint32_t n_cols;
    double *y;
    size_t ldy;
};

// The status of a banded Cholesky factorisation (banded_chol.hip), on the
// device: first_bad = n while every pivot so far was > 0, else the first row
// whose pivot was not (every later kernel reads it and returns); min_pivot the
// smallest U[i][0] of the rows factored.  Written by the fill kernel and by the
// one workgroup of each diagonal-block launch, with plain stores.
struct BandedCholStatus {
    uint32_t first_bad, pad;
    double min_pivot;
};

// A banded Cholesky factorisation (wld_banded_cholesky_device): A = the
// symmetric matrix of `band` (float or binary16, ld apart) with fl(fl(B[i][0] +
// ridge) + diag[i]) on the diagonal (diag may be null), factored in place in f
// ([n][ldf] f64, the same band layout, U of A = U^T U).
struct BandedCholArgs {
    const void *band;
    size_t ld;
    bool band_f16;
    uint32_t n, K;
    double ridge;
    const double *diag;
    double *f;
    size_t ldf;
    BandedCholStatus *status;
};

// The triangular solves with such a factor (wld_banded_solve_device): b
// ([n][ldb] f64, n_cols columns) is overwritten by the solution; fwd: U^T y =
// b, bwd: U x = y, both: A x = b.
struct BandedSolveArgs {
    const double *f;
    size_t ldf;
    uint32_t n, K;
    bool fwd, bwd;
    double *b;
    size_t ldb;
    uint32_t n_cols;
};

// The pair-sum table of a band (banded_omega.hip; wld_banded_pairsum_device):
// sums ([n][lds] f64, the band's layout) := M, M[j][k] the sum of the band's
// finite entries (u, v) with j <= u < v <= j + k; nonfinite counts the band
// elements (k >= 1, j + k < n) that were NaN or +-inf and counted as +0.0.
struct BandedPairsumArgs {
    const void *band;
    size_t ld;
    bool band_f16;
    uint32_t n, K;
    double *sums;
    size_t lds;
    unsigned long long *nonfinite;
};

// A sweep scan over such a table (wld_banded_omega_device): per split g the
// largest omega over the flank borders with its borders, and ZnS of [lo, hi];
// counts: {evaluated, skipped} candidates; status: the first split that breaks
// lo <= c < hi < n, hi - lo <= K (UINT32_MAX: none), written by the check launch.
struct BandedOmegaArgs {
    const double *sums;
    size_t lds;
    uint32_t n, K;
    const uint32_t *split, *lo, *hi;
    uint32_t n_splits, min_side;
    double eps;
    double *omega;
    uint32_t *left, *right;
    double *zns;
    unsigned long long *counts;
    uint32_t *status;
};

// The staging of one batch of a best-partner run (pair_partners.hip;
// wld_run_partners; layout in partners_plan.hpp).  Tile position p of the
// launch's list (p < n_tiles, the workgroup id) owns the parts (2 p + side) *
// 64 + local site: cnt[part] = its entries, min(kp, the site's candidates in
// the tile), written for every part of a listed tile; stage[part * kp + rank]
// = {key, d, d'}, rank < cnt[part], best first.  Nothing of it needs zeroing.
// classes = {pairs, none, passing} (zero before the run's first launch), one
// atomic each per tile.  guard: a device word, zero before the launch.
struct PartnerEntry {
    unsigned long long key;
    float d, dp;
};
struct PartnersArgs {
    unsigned long long *classes;
    PartnerEntry *stage;
    uint32_t *cnt;
    uint32_t kp;  // list length per part: min(k, 64)
    unsigned *guard;
};
// The merge of a batch into the running lists run[site * k + rank] (k entries
// per site, best first, key 0 past the site's count; all zero before the first
// batch): csr_off [n_blocks + 1] / csr_ent: per 64-site block the (2 position +
// side) entries of the batch that hold parts of its sites.
struct PartnersMerge {
    const PartnerEntry *stage;
    const uint32_t *cnt;
    uint32_t kp, k;
    uint32_t n_parts;  // 128 x the batch's tiles
    const uint32_t *csr_off, *csr_ent;
    uint32_t n_ent, n_blocks, L;
    PartnerEntry *run;
    unsigned *guard;
};
constexpr unsigned kPartnersGuardTile = 1, kPartnersGuardEntry = 2, kPartnersGuardPart = 4;

// encode.hip
// site_index: nullptr, or the kept-site map of the device pre-pass (row s of the
// filtered set = raw row site_index[s])
void launch_encode(const uint8_t *d_sites, const uint32_t *site_index, size_t L, size_t N, size_t LP, size_t NP,
                   uint8_t *codes, uint8_t *site_ok, hipStream_t s);
void launch_weight_prep(const float *d_w, size_t N, size_t NP, float *w_pad, float *wstats, hipStream_t s);

// prepass.hip (device site filter + Henikoff weights, bit-exact with host.cpp)
void launch_site_stats(const uint8_t *raw, size_t L, size_t N, uint32_t min_acgt, float min_minor, float max_minor,
                       uint8_t *keep, float *tab, hipStream_t s);
void launch_henikoff(const uint8_t *raw, const uint32_t *site_index, size_t n_kept, size_t N, const float *tab,
                     float *tabK, float *w, hipStream_t s);
void launch_fill_ones(float *w, size_t N, hipStream_t s);

// pair_valu.hip
struct ValuLaunch {
    const uint8_t *codes;    // site-major codes, NP bytes per site (REF: the lane-class layout)
    const float *w;          // NP weights (REF: the lane-class layout)
    const uint8_t *site_ok;
    const uint32_t *tiles;   // tile list (or the candidate list with tile_count)
    uint32_t n_tiles;        // list length, or (tile_count) its capacity
    const unsigned *tile_count;  // device tile count: the looping candidate launch; else null
    uint32_t L, NP, n_chunk_rows;
    float thr;
    bool safe;   // non-finite weights: the select loop
    bool plain;  // WLD_OPT_VALU_PLAIN: the VALU fmaf loop instead of f32 MFMA
    bool ref;    // WLD_OPT_REF_SUMS: lib.rs's own f32 summation order
    uint32_t ref_cls;  // REF: sequence positions per lane class (multiple of 64, 0 when N < 8)
    uint32_t ref_tail_n;  // REF: the scalar tail's sequences (N mod 8), in the stage after the classes
    // tile_count launches: per list entry, the 16x16 sub-blocks (bit 4 (a/16)
    // + b/16) whose pairs are computed; the others' pairs provably fail (the
    // screen's per-pair bound) and are skipped.  Null: every sub-block.
    const uint32_t *tile_bits;
    unsigned *tile_work;  // tile_count launches: the work counter (0 before the launch)
    // tile_count launches: the list in 16 buckets of bucket_cap entries
    // (pair_common.hpp cand_entry; null: one plain list)
    const unsigned *tile_buckets;
    uint32_t bucket_cap;
    ScanArgs scan;        // tile_count launches: the run's scan fused into the last workgroup (ticket set)
    // tile_count launches: the list's entries are 16-row blocks of candidate
    // tiles (pair_mfma.hip ScreenArgs::rb_items), counted by the buckets
    bool rb_items;
};
// returns true when the run's chunk scan ran in the launch (v.scan given, the
// item kernel of a full run); else the caller launches it
bool launch_pair_valu(const ValuLaunch &v, const OrderArgs &o, const DenseArgs *dense, hipStream_t s);
// The candidate pairs a kModeRefPairs launch (pair_mfma.hip) staged: summed in
// lib.rs's order one pair per thread from the lane-class layout
// (ref_sums_kernel), then per tile slice the passing rows kept in place (in
// order), its segment counts/offsets and chunk total corrected, the rest
// dropped (ref_compact_kernel, whose last workgroup runs the run's chunk scan:
// scan.ticket).
struct RefRowsLaunch {
    const uint8_t *rcodes;  // the lane-class layout (NPr bytes per site)
    const float *rw;
    uint32_t NPr, ref_cls, ref_tail_n, n_chunk_rows;
    float thr;
    const uint32_t *slices;  // per tile with candidates: {staging base, rows, ta << 16 | tb}
    const unsigned *slice_count;
    unsigned *work;  // work counter, 0 before the launch
    ScanArgs scan;
};
void launch_ref_rows(const RefRowsLaunch &r, const OrderArgs &o, hipStream_t s);
// the lane-class layout of REF: cls positions per class, the tail stage, NPr
void ref_layout_dims(size_t N, uint32_t *cls, uint32_t *tail, size_t *NPr);
void launch_ref_layout(const uint8_t *codes, const float *w_pad, size_t LP, size_t NP, size_t N, uint8_t *rcodes,
                       float *rw, hipStream_t s);

// pair_summary.hip
// Every tile of v's list (v.ref: the lane-class layout, finite weights) summed
// in lib.rs's order and reduced into s; o gives the window (win_hi) only —
// nothing of the row path's run state is read or written.
void launch_pair_summary(const ValuLaunch &v, const OrderArgs &o, const SummaryArgs &s, hipStream_t st);

// pair_heatmap.hip
// The same sums over v's list (the heat map's own filtered tile list), every
// considered pair reduced into its cell of h; o gives the window only.
void launch_pair_heatmap(const ValuLaunch &v, const OrderArgs &o, const HeatmapArgs &h, hipStream_t st);

// pair_annot.hip
// The same sums over v's list (the call's own tile list of the range and
// window); every tile's counted r2 multiplied into a's score rows; o gives the
// window only.
void launch_pair_annot(const ValuLaunch &v, const OrderArgs &o, const AnnotArgs &a, hipStream_t st);

// pair_matrix.hip
// The same sums over v's list (the call's own list of the band's tiles); every
// tile's values staged in LDS and stored into m.dst directly and transposed
// (matrix_plan::images); o gives the window only.  launch_matrix_fill writes
// the n_blocks listed 64x64 blocks (bi << 16 | bj) no tile of the list covers:
// +0.0, and the diagonal rule where a block holds the diagonal.
void launch_pair_matrix(const ValuLaunch &v, const OrderArgs &o, const MatrixArgs &m, hipStream_t st);
void launch_matrix_fill(const uint32_t *blocks, uint32_t n_blocks, const uint8_t *site_ok, const MatrixArgs &m,
                        hipStream_t st);

// pair_matrix_banded.hip
// The same sums over v's list (the call's own list of the row range's tiles);
// every tile's values staged in LDS and stored into the rows of m.dst, each
// tile row one contiguous run of k; o gives the window only.
// launch_matrix_banded_fill writes the elements of the n_blocks listed blocks
// that no tile of the list covers: +0.0, and the diagonal rule at k = 0.
void launch_pair_matrix_banded(const ValuLaunch &v, const OrderArgs &o, const MatrixBandedArgs &m, hipStream_t st);
void launch_matrix_banded_fill(const matrix_banded_plan::FillBlock *blocks, uint32_t n_blocks, const uint8_t *site_ok,
                               const MatrixBandedArgs &m, hipStream_t st);

// banded_apply.hip
// Y := S X on st: one workgroup per 64 output rows and 16 or 64 columns, each Y
// element summed by its owner in a fixed order (f64 MFMA accumulation).
void launch_banded_apply(const BandedApplyArgs &a, hipStream_t st);

// banded_chol.hip
// launch_banded_chol: the fill (f := f64(band) + shifts, +0.0 tails, the status
// reset), then per block row of 64 rows a diagonal-block launch, a panel
// launch and a window launch (the trailing update on f64 MFMAs); ordered by
// the stream alone.  launch_banded_solve: one workgroup per 16 or 64 columns
// marches over the block rows, forward and/or backward.
void launch_banded_chol(const BandedCholArgs &a, hipStream_t st);
void launch_banded_solve(const BandedSolveArgs &a, hipStream_t st);

// banded_omega.hip
// launch_banded_pairsum: the row scan (P in place in a.sums), then the chain
// scan (M in place, +0.0 tails); a.nonfinite zeroed by the caller.
// launch_banded_omega_check writes a.status (set to UINT32_MAX by the caller);
// launch_banded_omega runs one workgroup per split on splits the check passed.
void launch_banded_pairsum(const BandedPairsumArgs &a, hipStream_t st);
void launch_banded_omega_check(const BandedOmegaArgs &a, hipStream_t st);
void launch_banded_omega(const BandedOmegaArgs &a, hipStream_t st);

// pair_blocks.hip
// The same sums over v's list: pass 1 (every tile of the range and window)
// reduces the weak pairs to the per-site break arrays of b; pass 2 (the tiles
// the reported blocks touch, a list of its own) reduces the pairs inside a
// block to its statistics.  o gives the window only.
void launch_pair_block_breaks(const ValuLaunch &v, const OrderArgs &o, const BlockBreakArgs &b, hipStream_t st);
void launch_pair_block_stats(const ValuLaunch &v, const OrderArgs &o, const BlockStatsArgs &b, hipStream_t st);

// pair_partners.hip
// The same sums over v's list (one batch of the run's own tile list, v.thr the
// run's threshold); every tile's candidates selected per a row and per b
// column into the batch's staging; o gives the window only.  Then the merge of
// the staged parts into the running lists.
void launch_pair_partners(const ValuLaunch &v, const OrderArgs &o, const PartnersArgs &p, hipStream_t st);
void launch_partners_merge(const PartnersMerge &m, hipStream_t st);

// pair_targets.hip (wld_run_targets): one batch of target blocks against their
// partner tiles.  Slot 16 b + j is the j-th target of the batch's block b.
// The pair launch writes d, d', r2 of every passing (slot, site) into the dense
// staging and a 64-bit pass mask per (slot, partner tile) (zero before the
// launch); the count launches give every slot's rows, their prefix over the
// slot's tiles and over the slots; the row launch then writes the rows in
// (slot, partner) order.
struct TargetsLaunch {
    const uint8_t *rcodes;  // the lane-class layout (NPr bytes per site)
    const float *rw;
    const uint8_t *site_ok;
    const uint32_t *win_hi;    // the window's limits ([LP]); null: no window
    const uint32_t *site_map;  // parent indices (L entries); null: identity
    uint32_t L, LP, NPr, ref_cs, ref_tail_n;
    float thr;
    uint32_t n_blocks;           // of the batch
    const uint32_t *slot_site;   // [16 n_blocks] loaded index of the slot's target (targets_plan::kNoTarget: empty)
    const uint32_t *slot_pos;    // [16 n_blocks] its position in the caller's list
    const uint32_t *items;       // n_items x {block, partner tile}
    uint32_t n_items;
    float *d, *dp, *r2;          // [16 n_blocks][LP]
    unsigned long long *mask;    // [16 n_blocks][LP / 64]
    uint32_t *tile_pref;         // [16 n_blocks][LP / 64]: the slot's rows in the tiles before
    uint32_t *slot_cnt;          // [16 n_blocks]
    uint32_t *slot_base;         // [16 n_blocks + 1]: the rows of the slots before; the last: the batch's rows
    unsigned *guard;             // zero before the launches; kGuard* bits of refused indices
    // the batch's rows (out_cap entries each)
    uint32_t *out_target, *out_site_target, *out_site_partner;
    float *out_d, *out_dp, *out_r2;
    uint64_t out_cap;
};
constexpr unsigned kTargetsGuardItem = 1, kTargetsGuardSite = 2, kTargetsGuardRow = 4;
void launch_targets_pairs(const TargetsLaunch &t, hipStream_t s);
void launch_targets_count(const TargetsLaunch &t, hipStream_t s);
void launch_targets_rows(const TargetsLaunch &t, hipStream_t s);

// pair_mfma.hip
bool mfma_supported();
// weight digits (two layouts) + per-64-site filter bits
size_t mfma_planes_bytes(size_t LP, size_t NP);
void launch_mfma_prep(const uint8_t *site_ok, const float *w_pad, size_t L, size_t LP, size_t NP, int shift,
                      int8_t *planes, hipStream_t s);
// frag holds 2 LP NP bytes: selector-coded, then 0/1/2-coded (B operands)
void launch_frag(const uint8_t *codes, size_t LP, size_t NP, uint8_t *frag, hipStream_t s);
// weight-plane statistics written by launch_mfma_prep (read back once per load)
struct MfmaWeightStats {
    unsigned plane_mask;  // bit p = digit plane p (of 4) has a nonzero digit
    int nonneg;           // every weight >= 0
    uint64_t resid[3];    // resid[t-1] = sum_k |q_k - 2^(8t) d_t,k|: what top plane t alone leaves out
    uint64_t dsum[4];     // dsum[p] = sum_k |d_p,k|: bounds every one-plane sum of plane p
};
// synchronises s; returns 0, or -1 on a HIP error
int mfma_weight_stats(const int8_t *wplanes, size_t LP, size_t NP, hipStream_t s, MfmaWeightStats *out);

// workgroups of the candidate launch after a screen (it strides over a tile
// list whose length is known only on the device): 4 rounds of 2 per CU
constexpr uint32_t kCandidateGrid = 2048;
// ... and of the reference-order f32 kernel's candidate loop: its resident
// workgroups (three per CU, 256 CUs); extra workgroups would only queue (and
// cost dispatch time when there is no candidate at all)
constexpr uint32_t kRefCandidateGrid = 768;
// ... and of its items (ref_item_kernel<LOOP>, one sub-block per wave, five
// workgroups per CU): 1,024 (4 per CU) measured faster than 768, 896 or
// every slot (1,280) on LD blocks (profiles/r06t/, r06u/)
constexpr uint32_t kRefItemGrid = 1024;
// ... and of ref_sums_kernel / ref_compact_kernel (low-register: eight per CU)
constexpr uint32_t kRefRowsGrid = 2048;

// The fp6 screen's operands (pair_mfma.hip frag6_kernel) and constants: R
// (residual bound of the rounded weights plus the reference's rounding) and
// Tg (>= every doubled T), in the units of the fp6 weights (capi.hip).  The
// images are complement-coded (missing / minor), so the screen also takes the
// per-site marginals marg[2 s] = sum_k w6_k [s missing], marg[2 s + 1] = sum_k
// w6_k [s minor] (LP sites) and W6 = sum_k w6_k, all exact multiples of 1/8
// below 2^17, from which its epilogue restores the direct coding's sums
// (pair_common.hpp f6c_direct).
struct Fp6Screen {
    const uint8_t *a6, *b6;
    const float *marg;
    float W6;
    uint32_t NK;  // 128-sequence blocks
    double R;
    float Tg;
    // the A image is fp4 nibbles (every weight code an e2m1 value,
    // fp6_scale.hpp fp6_codes_fit_fp4, and WLD_OPT_FP6_A4 on): 8 KB per tile
    // and 128 sequences instead of 12, the same products and sums
    bool a4;
    // no A image: every weight code of the load is the one code of value wv
    // (fp6_scale.hpp fp6_shared_code, and WLD_OPT_FP6_SHARED on), a6 is b6,
    // the kernels mask the row tile's B image into the A operands and scale
    // the restored sums by wv; the padded sequences are coded 0 in b6
    bool shared;
    float wv;
    // the per-load site records of the tile-pair kernel's three-sum tests
    // (launch_fp6_records; pair_common.hpp F6RowRec): fp6_rec_bytes(LP) bytes,
    // built from marg, W6 and R at the load, so valid as long as those are;
    // counts: held in count units (shared and wv a power of two)
    const void *rec;
    bool counts;
};
size_t fp6_a_bytes(size_t LP, size_t NP, bool a4);
size_t fp6_b_bytes(size_t LP, size_t NP);
size_t fp6_rec_bytes(size_t LP);
// f: marg, W6, R, shared and wv set; writes LP sites' records to rec and sets
// f.rec and f.counts
void launch_fp6_records(Fp6Screen &f, size_t LP, void *rec, hipStream_t s);
// w6: NP fp6 (e2m3) codes of the rounded weights (0 for padding: a padded
// sequence reads as missing and must weigh nothing); wa: the codes the A
// image holds, w6 itself or (a4) their e2m1 codes; marg: 2 LP floats.
// shared: b6 alone is built (a6, wa unused), the N real sequences' symbols
void launch_frag6(const uint8_t *codes, const uint8_t *w6, const uint8_t *wa, bool a4, bool shared, size_t LP,
                  size_t NP, size_t N, uint8_t *a6, uint8_t *b6, float *marg, hipStream_t s);

// The i8 one-plane screen's pre-multiplied operand images (pair_mfma.hip
// pair_i8_screen2w_kernel; capi.hip i8img_prepare): A = the top weight digit
// times in / major, B = the codes, per 64-site tile and 64-sequence block.
struct I8Screen {
    const uint8_t *a8, *b8;
    uint32_t digit_plane;  // the digit plane the images hold
};
size_t i8_a_bytes(size_t LP, size_t NP);
size_t i8_b_bytes(size_t LP, size_t NP);
// digit: NP int8 digits of the plane (planes + plane * NP)
void launch_i8img(const uint8_t *codes, const int8_t *digit, size_t LP, size_t NP, uint8_t *a8, uint8_t *b8,
                  hipStream_t s);

struct MfmaLaunch {
    const uint8_t *codes;   // site-major codes (used when frag is null)
    const uint8_t *frag;    // fragment-major selector-coded copy (LDS kernel), or null
    const uint8_t *frag_b;  // fragment-major 0/1/2-coded copy (B operands)
    const int8_t *wplanes;
    const uint32_t *tiles;
    uint32_t n_tiles, L, LP, NP, n_chunk_rows;
    float thr;
    int shift;
    unsigned plane_mask;
    int nonneg;
    screen_policy::Route route;  // the pass's path (screen_policy.hpp): IntAll, a screen, or CandidatePairs
    bool bound_test;             // thr > 0: skip pairs r2_bound_skip rejects
    uint64_t resid[3];
    uint64_t dsum[4];
    uint32_t *cand_list;   // 32 n_tiles entries: 16 buckets of tiles, then 16 of their sub-block bits
    unsigned *cand_count;  // 0 before the launch (chunk_scan_kernel resets it)
    unsigned *cand_buckets;  // 16 bucket counts, 0 before the launch (chunk_scan_kernel resets them)
    int test_guard = 0;      // WLD_OPT_TEST_GUARD (launch_candidates)
    unsigned *cand_work;   // the candidate launch's work counter (the screen zeroes it)
    // WLD_OPT_REF_SUMS: the candidate tiles go to the reference-order f32
    // kernel (ref_valu, tiles/tile_count filled in here) and the screen's
    // residual bound grows by r_extra_q (fixed-point units: how far the
    // reference's f32 sums can lie from the fixed-point sums, 2x2-cell L1)
    const ValuLaunch *ref_valu;
    double r_extra_q;
    // WLD_OPT_REF_SUMS without a screen: every tile on all planes, the pairs
    // the bound cannot reject (residual r_extra_q) staged as candidates, then
    // summed one by one in lib.rs's order (launch_ref_rows; ref_rows filled in
    // here but for the slices, count and work counter)
    const RefRowsLaunch *ref_rows;
    // with a screen: the run's scan, fused into the screen's or the candidate
    // launch's last workgroup when scan.ticket is set
    ScanArgs scan;
    // Fp6Screen (and the sample run): the fp6 operands
    const Fp6Screen *fp6;
    // ... gives up past this many candidate tiles (0: never; kAbandonBit)
    uint32_t fp6_bail;
    // ... its tile-pair list (pair_fp6_screen2w_kernel; XCD-ordered, kNoTile padded)
    const uint32_t *f6_pairs;
    uint32_t f6_n_pairs;
    // ... on three masked sums per pair, the fourth only for entries with a
    // pair in doubt (tile pairs only; screen_policy.hpp), which it counts into
    // *f6_rechecked (0 before the launch: the scan resets it)
    bool fp6_three = false;
    unsigned *f6_rechecked = nullptr;
    // ... with the lane-shared quick test in front of the three-sum test
    // (WLD_OPT_FP6_QUICK), which counts the row blocks that fell through to it
    // into f6_rechecked[1]
    bool fp6_quick = false;
    // I8PairScreen: the pre-multiplied operands of the top active plane
    const I8Screen *i8img = nullptr;
};
// The fp6 screen's sample run over every stride-th entry of its list: probe[0]
// = the sampled tiles holding a pair its bound cannot reject, probe[1] = the
// sampled tiles, probe[2] = with m.fp6_three (tile pairs) the sampled entries
// that formed the fourth sum, else 0, probe[3] = with m.fp6_quick the row
// blocks (four per tile) the quick test did not reject, else 0 (m as for the
// pass; nothing else is written)
void launch_fp6_probe(const MfmaLaunch &m, unsigned *probe, uint32_t stride, hipStream_t s);
// Enqueues the MFMA pair kernel(s) of one pass by m.route; where a screen runs
// (screen_policy::ran_screen; never for dense stats or site-major, which the
// policy sends to IntAll) screen_done, if given, is recorded between the two
// launches.
void launch_pair_mfma(const MfmaLaunch &m, const OrderArgs &o, const DenseArgs *dense, hipStream_t s,
                      hipEvent_t screen_done);

// order.hip
// per-chunk progress of the chunks [lin_begin, lin_begin + count): tiles per
// chunk into chunk_left[lin], prog_n = 0
void launch_progress_init(unsigned *chunk_left, uint32_t lin_begin, uint32_t count, uint32_t n_chunk_rows, uint32_t L,
                          unsigned *prog_n, hipStream_t s);
// the same under a window: the tiles of the run's list only (n_tiles entries,
// kNoTile padding skipped); a chunk without a listed tile stays at 0 and is
// never reported
void launch_progress_init_window(unsigned *chunk_left, uint32_t lin_begin, uint32_t count, uint32_t n_chunk_rows,
                                 const uint32_t *tiles, uint32_t n_tiles, unsigned *prog_n, hipStream_t s);
// The window's per-site limits (window_plan.hpp limits, bit for bit): hi[a] =
// the last b <= min(L - 1, a + K) (K == 0: L - 1) with pos[b] - pos[a] <= D
// (D == 0: no limit; pos null: pos[i] = i), hi[a] = a for a in [L, LP)
void launch_window_limits(const uint32_t *pos, uint32_t L, uint32_t LP, uint64_t D, uint64_t K, uint32_t *hi,
                          hipStream_t s);
// zeroes the run state (staging cursor, row total, every chunk total)
void launch_run_init(unsigned long long *counters, uint32_t *chunk_total, uint32_t n_chunks, hipStream_t s);
// the run's chunk scan as a launch of its own (ScanArgs; ticket unused)
void launch_chunk_scan(const ScanArgs &a, hipStream_t s);
// (rows: the run's row count, the bound of every destination.  With state
// (the run counters) set, the gather is enqueued before the host has seen the
// scan: it reads the row total and the cursor the scan saw from the device and
// writes nothing if the staging overflowed or the rows exceed out_cap — the
// host then re-runs the pass or gathers again into larger buffers)
void launch_gather(const OrderArgs &o, const uint32_t *chunk_base, uint32_t lin_begin, uint32_t count,
                   uint32_t n_chunk_rows, uint32_t L, uint64_t rows, const unsigned long long *state,
                   uint64_t out_cap, const uint32_t *site_map, uint32_t *out_a, uint32_t *out_b, float *out_d,
                   float *out_dp, float *out_r2, hipStream_t s);

// prune.hip (wld_run_prune): the greedy r2-independent site set of an edge list.
// ea/eb: m edges in loaded indices; rank: the order (a permutation of 0..L-1);
// off [L + 1], cur [L], hp [m]: the directed CSR (off zero before
// launch_prune_csr); state [L]: prune_plan's codes, kUndecided (0) before the
// first round; guard, n_kept: zero before the first launch.
struct PruneArgs {
    const uint32_t *ea, *eb;
    uint32_t m, L;
    const uint32_t *rank;
    uint32_t *off, *cur, *hp, *state;
    unsigned *guard, *n_kept;
    uint8_t *keep;
    uint32_t *tag;
};
constexpr unsigned kPruneGuardEdge = 1, kPruneGuardFill = 2, kPruneGuardList = 4, kPruneGuardTag = 8;
constexpr uint32_t kPruneSweeps = 4;  // sweeps over its vertices per decide launch
// degrees, scan, fill: hp[off[v] .. off[v + 1]) = the neighbours ranking before v
void launch_prune_csr(const PruneArgs &p, hipStream_t s);
// one round; prev: the launch before's undecided count (null: unknown), at 0
// the launch does nothing; left (zero before): the vertices it leaves undecided
void launch_prune_decide(const PruneArgs &p, const unsigned *prev, unsigned *left, hipStream_t s);
// keep[], tag[] and *n_kept from the final states
void launch_prune_tags(const PruneArgs &p, hipStream_t s);

// Linear index of chunk (row, col) in the reference's triu_index order
// (lib.rs:623-632): rows descend, so row r starts at (n-1-r)(n-r)/2.
__host__ __device__ inline uint32_t chunk_linear(uint32_t n, uint32_t row, uint32_t col) {
    uint32_t rf = n - 1 - row;
    return rf * (rf + 1) / 2 + (col - row);
}

// pairs (a < b) of chunk (row, col) of an L-site set: lib.rs:636-667's loops
__host__ __device__ inline uint64_t chunk_pairs(uint32_t L, uint32_t row, uint32_t col) {
    const uint64_t lo_a = (uint64_t)row * kChunk, lo_b = (uint64_t)col * kChunk;
    const uint64_t ra = lo_a >= L ? 0 : (L - lo_a < (uint64_t)kChunk ? L - lo_a : (uint64_t)kChunk);
    const uint64_t rb = lo_b >= L ? 0 : (L - lo_b < (uint64_t)kChunk ? L - lo_b : (uint64_t)kChunk);
    return row == col ? ra * (ra ? ra - 1 : 0) / 2 : ra * rb;
}

}  // namespace wld
