// C ABI of the device hot path (include/weightedld.h).
//
// wld_all_weighted_ld_pairs is the drop-in for all_weighted_ld_pairs
// (lib.rs:578-684).  It is built from the staged calls:
//   wld_load  : H2D of SiteSet.buffer + weights, encode on device
//   wld_run   : pair kernel over the shard's tiles -> staging + segment counts,
//               chunk scan, reference-order gather (order.hip)
//   wld_rows_copy : D2H of the ordered rows
// There is no CPU compute path: without a gfx950 device every device entry
// point fails with WLD_E_NODEV.
#include <algorithm>
#include <cmath>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "common.hpp"
#include "tile_order.hpp"
#include "window_plan.hpp"
#include "summary_plan.hpp"
#include "heatmap_plan.hpp"
#include "annot_plan.hpp"
#include "matrix_plan.hpp"
#include "blocks_plan.hpp"
#include "partners_plan.hpp"
#include "prune_plan.hpp"
#include "targets_plan.hpp"
#include "banded_omega_plan.hpp"
#include "kernels.hpp"
#include "fp6_scale.hpp"

using namespace wld;

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail(e_ == hipErrorOutOfMemory ? WLD_E_OOM : WLD_E_HIP, "%s failed: %s (%s:%d)", \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                          \
    } while (0)

#define WLD_TRY(expr)          \
    do {                       \
        int st_ = (expr);      \
        if (st_ != WLD_OK)     \
            return st_;        \
    } while (0)

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

int ensure(DevBuf &b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.p && b.bytes >= bytes) return WLD_OK;
    if (b.p) {
        (void)hipFree(b.p);
        b.p = nullptr;
        b.bytes = 0;
    }
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        b.p = nullptr;
        (void)hipGetLastError();
        return fail(WLD_E_OOM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    }
    b.bytes = bytes;
    return WLD_OK;
}

void release(DevBuf &b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

template <class T>
T *ptr(DevBuf &b) {
    return reinterpret_cast<T *>(b.p);
}

size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

}  // namespace

// A run between wld_run_chunks_async (or run_chunks' first phase) and its
// completion: what run_complete needs to check, re-run and assemble it.
struct RunPending {
    bool active = false;
    float thr = 0.f;
    uint32_t lin_begin = 0, lin_end = 0;
    uint64_t pairs = 0;
    unsigned long long *count_out = nullptr;
};

struct wld_ctx {
    int device = 0;
    // a device group (wld_create_multi): one member context per device; the
    // group itself owns no stream or buffers
    std::vector<wld_ctx *> members;
    hipStream_t stream = nullptr;      // where the context's work goes (own_stream or the caller's)
    hipStream_t own_stream = nullptr;  // created with the context
    hipEvent_t ev[7] = {};  // 2..3 pair phase (6: after the screen), 3..4/5 order phase
    RunPending pend;                      // the run between run_enqueue and run_complete
    bool run_dirty = true;                // run state (cursor, chunk totals) may be nonzero: re-initialise
    // mapped pinned {cursor, rows, candidate tiles, sub-blocks} (the scan), then
    // the kernels' guard word (OrderArgs::guard; 0 unless an index was refused)
    unsigned long long *h_cnt = nullptr;
    unsigned long long *d_hcnt = nullptr;
    int cand_set = 0;  // the candidate set (counter words) of the next pass; flips after each scan
    int kernel_pref = WLD_KERNEL_AUTO;
    // wld_set_option (include/weightedld.h)
    bool opt_prefilter = true, opt_tile_rows = false, opt_all_planes = false;
    int opt_screen = 1;  // WLD_OPT_SCREEN: 0 never, 1 auto (default), 2 always, 3 two-plane, 4 exact candidate pairs
    screen_policy::Learned learned;  // auto: the thresholds the passes so far have taught (screen_policy.hpp)
    screen_policy::Plan pass;        // the last row pass's plan (its route as launched)
    DevBuf fp6_probe_buf;  // the sample run's four counts
    bool opt_site_major = false, opt_valu_plain = false;
    bool opt_fused_scan = true;  // WLD_OPT_FUSED_SCAN: the chunk scan in the candidate launch's last workgroup
    int opt_test_guard = 0;      // WLD_OPT_TEST_GUARD (tests: a bucket count corrupted before the candidate launch)
    // WLD_OPT_FP6_PAIRS_MIN_TILES: the fp6 screen runs on tile pairs from this
    // many tiles in the run's list, below it one tile per workgroup.  Alone
    // (one pass at a time) single tiles screen rank 0's 1/8 and 1/4 shards of
    // C4 5-7% faster (profiles/r05q, r05s), but in the N>1 step path, where
    // the passes of three contexts overlap, the 1/4 shard steps 6% faster on
    // pairs and the 1/8 shard is even within noise (profiles/r05x); C5 pairs
    // 4.8% faster (profiles/r05j)
    int64_t opt_fp6_pairs_min = 0;  // (tile pairs at every list size: profiles/r05ar/)
    bool opt_i8_pairs = true;    // WLD_OPT_I8_PAIRS: the i8 screen on tile pairs (pre-multiplied images)
    int opt_fp6 = 1;             // WLD_OPT_SCREEN_FP6: 0 off, 1 auto, 2 whenever it applies, 3 auto without the sample run
    bool opt_fp6_a4 = true;      // WLD_OPT_FP6_A4: the fp6 screen's A image as fp4 where the weight codes fit e2m1
    int opt_fp6_quick = 1;  // WLD_OPT_FP6_QUICK: the lane-shared quick test in front of the three-sum test (0 never, 1 auto: after a sample run, 2 always)
    int opt_fp6_three = 1;  // WLD_OPT_FP6_THREE: the tile-pair fp6 screen on three sums (0 never, 1 auto: after a sample run, 2 always)
    bool opt_fp6_shared = true;  // WLD_OPT_FP6_SHARED: no A image where the weight codes are all one code (the B image serves both operands)
    bool opt_ref_sums = true;  // WLD_OPT_REF_SUMS: lib.rs's own f32 summation order (default)
    uint64_t opt_staging_rows = 1ull << 25, opt_host_batch_pairs = 1ull << 31;
    uint64_t opt_target_slots = targets_plan::kDefaultBatchSlots;  // WLD_OPT_TARGET_BATCH_SLOTS
    uint64_t opt_partners_bytes = partners_plan::kDefaultBatchBytes;  // WLD_OPT_PARTNERS_BATCH_BYTES
    uint64_t opt_matrix_bytes = matrix_plan::kDefaultBatchBytes;      // WLD_OPT_MATRIX_BATCH_BYTES

    // loaded SiteSet
    bool loaded = false;
    size_t L = 0, N = 0, LP = 0, NP = 0;
    DevBuf raw, wraw, codes, w_pad, wstats, site_ok, site_map, planes, frag;
    DevBuf rcodes, rw;       // WLD_OPT_REF_SUMS: codes and weights in lane-class order (ref_layout_kernel)
    // the fp6 screen (fp6_prepare): weight codes, packed operands, constants
    DevBuf w6, f6a, f6b, f6marg;  // (f6marg: the per-site marginals of the complement-coded images)
    DevBuf f6rec;                  // (the site records built from them: launch_fp6_records)
    DevBuf w4;                    // the weights' e2m1 codes, where the A image is fp4 (Fp6Screen::a4)
    Fp6Screen f6{};
    // the i8 one-plane screen's pre-multiplied images (i8img_prepare, at the
    // first pass that screens on i8 with them)
    DevBuf i8a, i8b;
    I8Screen i8s{};
    bool i8img_ok = false;
    bool fp6_tried = false;   // fp6_prepare ran for this load
    bool fp6_sampled = false; // this pass's screen was chosen by a sample run (fp6_sample)
    bool fp6_ok = false;      // operands built for this load (the weights allow it)
    bool fp6_better = false;  // ... and its residual is within twice the i8 top digit's (auto)
    double fp6_rel = 0.0, i8_rel = 0.0;  // the two screens' residuals relative to their sums
    bool have_ref = false;   // rcodes/rw hold this load's layout
    uint32_t ref_cls = 0;    // its positions per lane class
    size_t NPr = 0;          // its positions per site
    DevBuf keep, htab, htab_kept, site_index;  // device pre-pass (prepass.hip)
    std::vector<uint64_t> kept_map;  // parent indices of the kept sites (wld_site_map_copy)
    bool prepass_loaded = false;
    bool has_map = false;
    bool use_frag = false;
    int kernel = WLD_KERNEL_VALU;
    bool safe = false;
    int shift = 0;
    int fixed_planes = 3;      // digit planes of the fixed-point weights (3: 23 bits, 4: 31 bits)
    unsigned plane_mask = 7;   // weight-digit planes with a nonzero digit (MFMA)
    MfmaWeightStats wst{7, 1, {0, 0, 0}, {0, 0, 0, 0}};  // digit-plane statistics of the load (MFMA)

    // run state
    DevBuf tiles, cand, seg_cnt, seg_off, chunk_total, chunk_base, counters;
    DevBuf f6_pairs;          // the fp6 screen's tile-pair list of the tile list (pair_fp6_screen2w_kernel)
    uint32_t f6_n_pairs = 0;
    std::vector<uint64_t> chunk_pairs_pre;  // prefix sums of the loaded set's per-chunk pair counts (linear order)
    DevBuf st_a, st_b, st_d, st_dp, st_r2;
    DevBuf out_a, out_b, out_d, out_dp, out_r2;
    uint64_t st_capacity = 0;
    uint32_t tiles_lb = ~0u, tiles_le = ~0u;  // linear chunk range the tile list covers
    uint32_t n_tiles = 0;
    bool have_rows = false;
    uint64_t rows = 0;
    // the gather goes into the stream behind the scan, before the host has
    // seen the row count, when the previous run had rows:
    // no host round trip between scan and gather; gather_cap: the output
    // rows the enqueued gather may write (0: none enqueued)
    bool spec_gather = false;
    int ev_end = 4;            // the event that ends a pass's scan: 4, or 3 when the scan ran inside the pair launch
    uint64_t gather_cap = 0;
    wld_run_stats stats{};
    // the last pass's phase times, read from its events only when the stats
    // are asked for (materialize_times; ~3 hipEventElapsedTime calls the N>1
    // step loop, which never reads them, does not pay)
    bool times_pending = false;
    int times_order_end = 4;
    // per-chunk progress (wld_run_host with a callback): the run's chunk
    // countdowns and log slot counter on the device, the log in mapped pinned
    // host memory (one u64 pair count per completed chunk, ~0 until written)
    DevBuf chunk_left, prog_n;
    unsigned long long *h_plog = nullptr, *d_plog = nullptr;
    size_t plog_cap = 0;
    const std::function<void(uint64_t)> *on_chunk = nullptr;  // set by run_host_range for its runs
    bool prog_pass = false;  // the pass in flight logs its chunks
    uint32_t prog_expect = 0;  // ... this many of them (under a window: the chunks with an in-window pair)

    // the window (wld_set_window; 0 = no limit; persists across loads) and its
    // plan for the loaded set (window_prepare; window_plan.hpp)
    uint64_t win_d = 0, win_k = 0;
    bool has_pos = false;
    std::vector<uint32_t> pos_host;      // the loaded site_map (has_pos), for the plan
    std::vector<uint32_t> win_hi_host;   // hi[a], the last in-window partner of a
    std::vector<uint64_t> win_pre;       // prefix of the in-window pairs per linear chunk
    std::vector<uint32_t> win_live_pre;  // prefix of the chunks holding an in-window pair
    DevBuf win_hi, win_pairs;            // hi[] ([LP], window_limits_kernel) and the per-chunk counts on the device
    bool tiles_windowed = false;         // the tile list was cut to the window ...
    uint64_t tiles_win_d = 0, tiles_win_k = 0;  // ... this one
    uint32_t n_tiles_listed = 0;         // its tiles without the XCD order's padding
    bool seg_clear = false;              // a windowed list was built: seg_cnt is zeroed before the next pass

    // wld_run_summary: its accumulators (zeroed per call) and the two events
    // around its launch (created at the first summary; the row path's events
    // keep the last row run's times)
    DevBuf sum_buf;
    hipEvent_t ev_sum[2] = {};

    // wld_run_heatmap: its accumulators (zeroed per call), its own tile list
    // (the range's list cut to the tiles that touch a cell: the row path's
    // cached list and its range stay as they are), the site -> cell map with
    // the per-block cell limits, and the two events around its launch
    DevBuf heat_buf, heat_tiles, heat_map;
    hipEvent_t ev_heat[2] = {};

    // wld_run_annot_scores: its accumulators {score[LP][CP], counts[4],
    // partners[LP]} (zeroed per call), its own tile list, the call's
    // annotation image with the zero-chunk mask, and the two events around its
    // launch
    DevBuf an_buf, an_tiles, an_img;
    hipEvent_t ev_an[2] = {};

    // wld_run_matrix_device / wld_run_matrix: the tile list and fill list of
    // a band, the four class counts, and the two events around a band's
    // launches (the host call's band buffer lives for the call only)
    DevBuf mx_lists, mx_cnt;
    hipEvent_t ev_mx[2] = {};

    // wld_banded_cholesky_device / wld_banded_solve_device: the factorisation's
    // status word and the two events around a call's launches
    DevBuf chol_status;
    hipEvent_t ev_chol[2] = {};

    // wld_banded_pairsum_device / wld_banded_omega_device: the words {nonfinite,
    // evaluated, skipped, status} and the two events around a call's launches
    DevBuf om_words;
    hipEvent_t ev_om[2] = {};

    // wld_run_partners: its own tile list, a batch's staging (entries and
    // counts), the batch's CSR, the running lists and the words {classes[3],
    // guard}; its events are created per call
    DevBuf pt_tiles, pt_stage, pt_cnt, pt_csr, pt_run, pt_words;

    // the LD blocks: pass 1's accumulators {classes[5], fwd[LP], bwd + 1 [LP]},
    // pass 2's per-block accumulators and its site -> block map with the
    // per-block id limits, a tile list of their own (either pass), and the
    // two events around each pass's launch (created at the first call)
    DevBuf blk_brk, blk_acc, blk_map, blk_tiles;
    hipEvent_t ev_blk[4] = {};

    // wld_run_prune: while it runs, the gathers leave loaded indices in
    // out_a/out_b (no site_map); its four events (created at the first prune:
    // before the CSR build, after it, after the rounds, after the tags) and
    // the last prune's three phase times (wld_prune_times)
    bool prune_run = false;
    hipEvent_t ev_pr[4] = {};
    double pr_ms[3] = {0.0, 0.0, 0.0};

    // wld_run_targets: a batch's lists, dense staging, masks, counts and rows
    // (kept between calls while small: run_targets), and the two events around
    // its pair launch (created at the first call)
    struct TargetBufs {
        DevBuf slot_site, slot_pos, items, d, dp, r2, mask, tile_pref, slot_cnt, slot_base, guard;
        DevBuf o_t, o_st, o_sp, o_d, o_dp, o_r2;
        std::vector<DevBuf *> all() {
            return {&slot_site, &slot_pos, &items, &d, &dp, &r2, &mask, &tile_pref, &slot_cnt, &slot_base, &guard,
                    &o_t, &o_st, &o_sp, &o_d, &o_dp, &o_r2};
        }
    } tg;
    hipEvent_t ev_tg[2] = {};

    ~wld_ctx() {
        for (wld_ctx *m : members) delete m;
        if (!members.empty()) return;
        (void)hipSetDevice(device);
        // work queued on a borrowed stream (wld_set_stream) may still use the
        // buffers: it completes before they are freed
        if (stream && stream != own_stream) (void)hipStreamSynchronize(stream);
        DevBuf *all[] = {&keep, &htab, &htab_kept, &site_index, &raw, &wraw, &codes, &w_pad, &wstats, &site_ok, &site_map, &planes, &frag, &rcodes, &rw, &w6, &w4, &f6a, &f6b, &f6marg, &f6rec, &i8a, &i8b, &tiles, &cand, &f6_pairs, &fp6_probe_buf,
                         &seg_cnt, &seg_off, &chunk_total, &chunk_base, &counters, &chunk_left, &prog_n, &win_hi, &win_pairs, &sum_buf, &heat_buf, &heat_tiles, &heat_map, &an_buf, &an_tiles, &an_img, &mx_lists, &mx_cnt, &chol_status, &om_words, &pt_tiles, &pt_stage, &pt_cnt, &pt_csr, &pt_run, &pt_words, &blk_brk, &blk_acc, &blk_map, &blk_tiles, &st_a, &st_b, &st_d,
                         &st_dp, &st_r2, &out_a, &out_b, &out_d, &out_dp, &out_r2};
        for (DevBuf *b : all) release(*b);
        for (DevBuf *b : tg.all()) release(*b);
        for (auto &e : ev_tg)
            if (e) (void)hipEventDestroy(e);
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
        for (auto &e : ev_sum)
            if (e) (void)hipEventDestroy(e);
        for (auto &e : ev_heat)
            if (e) (void)hipEventDestroy(e);
        for (auto &e : ev_an)
            if (e) (void)hipEventDestroy(e);
        for (auto &e : ev_mx)
            if (e) (void)hipEventDestroy(e);
        for (auto &e : ev_chol)
            if (e) (void)hipEventDestroy(e);
        for (auto &e : ev_om)
            if (e) (void)hipEventDestroy(e);
        for (auto &e : ev_blk)
            if (e) (void)hipEventDestroy(e);
        for (auto &e : ev_pr)
            if (e) (void)hipEventDestroy(e);
        if (h_cnt) (void)hipHostFree(h_cnt);
        if (h_plog) (void)hipHostFree(h_plog);
        if (own_stream) (void)hipStreamDestroy(own_stream);
    }
};

namespace {

// Every single-device entry point starts here; a device group (wld_create_multi)
// supports only wld_load, wld_run_host, wld_all_weighted_ld_pairs,
// wld_run_summary, wld_run_heatmap, wld_run_annot_scores, wld_run_partners, the LD-block calls and the option/kernel/stats calls,
// which dispatch to its members.
int set_dev(wld_ctx *c) {
    if (!c) return fail(WLD_E_ARG, "null context");
    if (!c->members.empty())
        return fail(WLD_E_STATE, "this call needs a single-device context; a multi-device context supports "
                                 "wld_load, wld_run_host and wld_all_weighted_ld_pairs");
    HIP_TRY(hipSetDevice(c->device));
    return WLD_OK;
}

float event_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    if (a == b) return 0.0f;  // (a phase that ended where it began: no API call)
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) {
        (void)hipGetLastError();
        return -1.0f;
    }
    return ms;
}

// the last completed pass's phase times from its events (run_complete defers them)
void materialize_times(wld_ctx *c) {
    if (!c->times_pending) return;
    c->times_pending = false;
    c->stats.pair_kernel_ms = event_ms(c->ev[2], c->ev[3]);
    c->stats.order_ms = event_ms(c->ev[3], c->ev[c->times_order_end]);
    c->stats.screen_ms = screen_policy::ran_screen(c->pass.route) ? event_ms(c->ev[2], c->ev[6]) : 0.0;
}

// fixed-point exponent for the MFMA weight planes: max|w| * 2^shift must fit
// `planes` balanced base-256 digits (|q| <= 127 * (1 + 2^8 + 2^16 [+ 2^24])).
int weight_shift(float maxabs, int planes) {
    const double lim = 127.0 * (1.0 + 256.0 + 65536.0 + (planes == 4 ? 16777216.0 : 0.0));
    int e = 0;
    std::frexp((double)maxabs, &e);  // maxabs = m * 2^e, m in [0.5, 1)
    int shift = (planes == 4 ? 30 : 22) - e;  // maxabs * 2^shift < 2^22 (2^30) < lim
    while (std::ldexp((double)maxabs, shift + 1) <= lim) ++shift;
    while (std::ldexp((double)maxabs, shift) > lim) --shift;
    return shift;
}

double ref_extra_residual(const wld_ctx *c);

// The fp6 screen's operands for this load (pair_mfma.hip): nonnegative
// finite weights, NP <= 16384 (its f32 test on doubled sums), the i8 kernel's
// fragment layout in use.  The weights are rounded to e2m3 (fp6_scale.hpp) at
// the common scale S whose L1 rounding residual is within 1% of the smallest
// of its candidates' and whose codes have the fewest set mantissa bits
// (fp6_choose_scale); R (in fp6 units) bounds each pass's 2x2-cell L1 distance
// between the screen's sums and the sums the candidate launch computes: the
// rounding, plus the fixed point's 0.5 per sequence (exact mode) and lib.rs's
// f32 summation (9 gamma_m sum w, ref_extra_residual) — both added, so one
// R serves either mode.  Where every weight code is also an e2m1 value (unit
// weights, Henikoff weights of a large alignment, dyadic sets: fp6_scale.hpp
// fp6_codes_fit_fp4) and WLD_OPT_FP6_A4 is on, the A image is built as fp4
// nibbles of the same values: two thirds of the bytes, the same sums, one
// image per load that every fp6 kernel reads.  Where every weight code is the
// same nonzero code (unit weights, Henikoff weights of a large alignment:
// fp6_shared_code) and WLD_OPT_FP6_SHARED is on, no A image is built at all:
// the kernels form the A operands from the row tile's B image, whose padded
// sequences are then coded 0, and scale the restored sums by the code's value.
// Built at load unless WLD_OPT_SCREEN_FP6 is 0, else on the first run that
// may screen on fp6 after the option is set.
int fp6_prepare(wld_ctx *c) {
    c->fp6_ok = c->fp6_better = false;
    c->fp6_tried = true;
    if (c->kernel != WLD_KERNEL_MFMA || !c->use_frag || !c->wst.nonneg || c->NP > 16384 || c->N == 0) return WLD_OK;
    std::vector<float> w(c->NP);
    HIP_TRY(hipMemcpyAsync(w.data(), c->w_pad.p, c->NP * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    double wmax = 0.0, wsum = 0.0;
    for (size_t k = 0; k < c->N; ++k) wmax = std::max(wmax, (double)w[k]), wsum += (double)w[k];
    if (!(wmax > 0.0) || !std::isfinite(wsum)) return WLD_OK;
    const double S = fp6_choose_scale(w.data(), c->N, wmax).S;
    std::vector<uint8_t> codes(c->NP, 0);
    double r6 = 0.0, sum6 = 0.0, v;
    for (size_t k = 0; k < c->N; ++k) {
        codes[k] = (uint8_t)fp6_code(S * w[k], &v);
        r6 += std::fabs(S * w[k] - v);
        sum6 += v;
    }
    const double u = 0x1p-24, m = (double)(c->N / 8) + 16.0, gamma = m * u / (1.0 - m * u);
    const double extra = S * (9.0 * gamma * wsum + 0.5 * (double)c->N * std::ldexp(1.0, -c->shift) * (1.0 + 9.0 * gamma));
    c->f6.R = (r6 + extra) * (1.0 + 1e-9) + 1e-9 * sum6;
    c->f6.Tg = (float)(2.0 * sum6);  // exact: a multiple of 1/8 below 2^21
    c->f6.W6 = (float)sum6;          // ... and so is the sum itself (the complement coding's W6)
    c->f6.NK = (uint32_t)((c->NP + 127) / 128);
    c->fp6_rel = c->f6.R / std::max(sum6, 1e-300);
    // the i8 top digit's: its residual (and the reference's rounding) against
    // the top plane's digit sum, in the same fixed-point units
    uint32_t top = 0;
    for (uint32_t p = 0; p < 4; ++p)
        if (c->wst.plane_mask >> p & 1) top = p;
    const double r8 = (top > 0 ? (double)c->wst.resid[top - 1] : 0.0) + ref_extra_residual(c);
    c->i8_rel = r8 / std::max(std::ldexp((double)c->wst.dsum[top], 8 * (int)top), 1e-300);
    c->f6.a4 = c->opt_fp6_a4 && fp6_codes_fit_fp4(codes.data(), c->N);
    const uint32_t one = c->opt_fp6_shared ? fp6_shared_code(codes.data(), c->N) : 0u;
    c->f6.shared = one != 0u;
    c->f6.wv = (float)fp6_value(one);
    WLD_TRY(ensure(c->w6, c->NP));
    if (c->f6.shared)
        release(c->f6a);  // (an earlier load's, or the same load's before the option was set)
    else
        WLD_TRY(ensure(c->f6a, fp6_a_bytes(c->LP, c->NP, c->f6.a4)));
    WLD_TRY(ensure(c->f6b, fp6_b_bytes(c->LP, c->NP)));
    WLD_TRY(ensure(c->f6marg, 2 * c->LP * sizeof(float)));
    WLD_TRY(ensure(c->f6rec, fp6_rec_bytes(c->LP)));
    // (codes: zero past N, which the complement coding needs, pair_mfma.hip frag6_kernel)
    HIP_TRY(hipMemcpyAsync(c->w6.p, codes.data(), c->NP, hipMemcpyHostToDevice, c->stream));
    std::vector<uint8_t> codes4;  // (outlives the copy: the stream is synchronized below)
    if (c->f6.a4 && !c->f6.shared) {
        codes4.resize(c->NP);
        for (size_t k = 0; k < c->NP; ++k) codes4[k] = (uint8_t)fp6_to_fp4_code(codes[k]);
        WLD_TRY(ensure(c->w4, c->NP));
        HIP_TRY(hipMemcpyAsync(c->w4.p, codes4.data(), c->NP, hipMemcpyHostToDevice, c->stream));
    }
    launch_frag6(ptr<uint8_t>(c->codes), ptr<uint8_t>(c->w6), ptr<uint8_t>(c->f6.a4 ? c->w4 : c->w6), c->f6.a4,
                 c->f6.shared, c->LP, c->NP, c->N, ptr<uint8_t>(c->f6a), ptr<uint8_t>(c->f6b), ptr<float>(c->f6marg),
                 c->stream);
    HIP_TRY(hipGetLastError());
    // (the site records: of this load's marginals, W6, R and wv, all set above
    // and changed by nothing but the next fp6_prepare)
    c->f6.marg = ptr<float>(c->f6marg);
    launch_fp6_records(c->f6, c->LP, c->f6rec.p, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->f6.b6 = ptr<uint8_t>(c->f6b);
    c->f6.a6 = c->f6.shared ? c->f6.b6 : ptr<uint8_t>(c->f6a);  // (shared: the row tiles are read from b6)
    c->fp6_ok = true;
    c->fp6_better = c->fp6_rel <= std::max(2.0 * c->i8_rel, 0.02);
    return WLD_OK;
}

// The i8 screen's pre-multiplied operand images of this load (pair_mfma.hip
// pair_i8_screen2w_kernel): the top nonzero digit plane times the site
// indicators, and the codes, 3 bytes per site and sequence; built on the
// context's stream at the first pass that screens on i8 with them.
int i8img_prepare(wld_ctx *c) {
    uint32_t top = 0;
    for (uint32_t p = 0; p < 4; ++p)
        if (c->plane_mask >> p & 1) top = p;
    WLD_TRY(ensure(c->i8a, i8_a_bytes(c->LP, c->NP)));
    WLD_TRY(ensure(c->i8b, i8_b_bytes(c->LP, c->NP)));
    launch_i8img(ptr<uint8_t>(c->codes), ptr<int8_t>(c->planes) + (size_t)top * c->NP, c->LP, c->NP,
                 ptr<uint8_t>(c->i8a), ptr<uint8_t>(c->i8b), c->stream);
    HIP_TRY(hipGetLastError());
    c->i8s = I8Screen{ptr<uint8_t>(c->i8a), ptr<uint8_t>(c->i8b), top};
    c->i8img_ok = true;
    return WLD_OK;
}

int build_tiles(wld_ctx *c, uint32_t lb, uint32_t le, bool windowed);
int window_prepare(wld_ctx *c);
int ensure_ref_layout(wld_ctx *c);
uint32_t chunks_of(size_t L);
uint32_t chunk_rows_of(size_t L);
void chunk_of_linear_host(uint32_t n, uint32_t i, uint32_t &row, uint32_t &col);
uint64_t pairs_in_chunk(size_t L, uint32_t row, uint32_t col);

int common_load(wld_ctx *c, const uint8_t *d_sites, const float *d_w, const uint64_t *site_map,
                const uint32_t *d_site_index = nullptr) {
    const size_t L = c->L, N = c->N;
    // a new data set: the auto screen policy (thresholds learned on the last
    // one) starts over; the reference-order layout is rebuilt when needed
    c->learned.reset();
    c->have_ref = false;
    c->LP = round_up(std::max<size_t>(L, 1), kChunk);
    c->NP = round_up(std::max<size_t>(N, 1), kSeqPad);
    WLD_TRY(ensure(c->codes, c->LP * c->NP));
    WLD_TRY(ensure(c->site_ok, c->LP));
    WLD_TRY(ensure(c->w_pad, c->NP * sizeof(float)));
    WLD_TRY(ensure(c->wstats, 4 * sizeof(float)));
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    launch_encode(d_sites, d_site_index, L, N, c->LP, c->NP, ptr<uint8_t>(c->codes), ptr<uint8_t>(c->site_ok),
                  c->stream);
    HIP_TRY(hipGetLastError());
    launch_weight_prep(d_w, N, c->NP, ptr<float>(c->w_pad), ptr<float>(c->wstats), c->stream);
    HIP_TRY(hipGetLastError());
    float ws[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(ws, c->wstats.p, 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));

    const bool finite = ws[2] == 0.0f;
    const float maxabs = ws[0], minabs = ws[1];
    // MFMA planes hold w * 2^shift in fixed point: 3 digit planes (q < 2^23) or
    // 4 (q < 2^31).  Each weight is then within 0.5 / q_min relative of its f32
    // value; AUTO requires that to be <= 2^-19 (sums of nonnegative weights,
    // any cell of the 2x2 table included, keep that relative error, so d and
    // r2 move by ~1e-6 at most: DESIGN.md §5), i.e. min|w| >= 2^-4 max|w| for
    // 3 planes and >= 2^-12 max|w| for 4; wider ranges take the f32 kernel.
    // The int32 accumulators hold X = S(minor) + 2 S(major) and Y = S(minor)
    // with |X| + |Y| <= 3 * 128 * NP (pair_mfma.hip, Acc16::get): NP < 2^31 / 384;
    // 4 planes fold two planes into int32 (NP <= 65024).
    constexpr size_t kMfmaMaxNP = 5592320, kMfma4MaxNP = 65024;
    const bool mfma_fits = c->NP <= kMfmaMaxNP;
    const bool range3 = minabs >= maxabs * 0x1p-4f, range4 = minabs >= maxabs * 0x1p-12f;
    const bool mfma_ok = mfma_supported() && mfma_fits && finite && maxabs > 0.0f &&
                         (range3 || (range4 && c->NP <= kMfma4MaxNP));
    int k = c->kernel_pref;
    if (k == WLD_KERNEL_AUTO) k = mfma_ok ? WLD_KERNEL_MFMA : WLD_KERNEL_VALU;
    if (k == WLD_KERNEL_MFMA && !(mfma_supported() && finite && maxabs > 0.0f))
        return fail(WLD_E_ARG, "MFMA kernel requested but weights are not finite/nonzero");
    if (k == WLD_KERNEL_MFMA && !mfma_fits)
        return fail(WLD_E_ARG, "MFMA kernel requested but %zu sequences exceed its int32 sums (max %zu)", N,
                    kMfmaMaxNP);
    c->kernel = k;
    c->safe = !finite;
    c->shift = 0;
    c->use_frag = false;
    if (k == WLD_KERNEL_MFMA) {
        // 3 planes when they hold every weight to 2^-19; else 4 (an explicit
        // MFMA request beyond 2^-12 keeps 4 planes and loses precision on the
        // smallest weights)
        c->fixed_planes = range3 || c->NP > kMfma4MaxNP ? 3 : 4;
        if (c->fixed_planes == 4 && c->opt_site_major)
            return fail(WLD_E_ARG, "the site-major MFMA kernel (WLD_OPT_MFMA_LAYOUT) multiplies 3 digit planes; "
                                   "these weights need 4");
        c->shift = weight_shift(maxabs, c->fixed_planes);
        WLD_TRY(ensure(c->planes, mfma_planes_bytes(c->LP, c->NP)));
        launch_mfma_prep(ptr<uint8_t>(c->site_ok), ptr<float>(c->w_pad), L, c->LP, c->NP, c->shift,
                         ptr<int8_t>(c->planes), c->stream);
        HIP_TRY(hipGetLastError());
        // fragment-major copy of the codes (1 KB contiguous per wave operand load);
        // WLD_OPT_MFMA_LAYOUT = 1 keeps the site-major reads (tests)
        c->use_frag = !c->opt_site_major;
        if (c->use_frag) {
            // two copies: the selector-coded one (A operands) and the
            // 0/1/2-coded one the B side reads raw
            WLD_TRY(ensure(c->frag, 2 * c->LP * c->NP));
            launch_frag(ptr<uint8_t>(c->codes), c->LP, c->NP, ptr<uint8_t>(c->frag), c->stream);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));

    c->has_map = site_map != nullptr;
    c->has_pos = false;
    c->pos_host.clear();
    if (site_map) {
        std::vector<uint32_t> &m = c->pos_host;  // kept: a window's plan reads it
        m.resize(L);
        for (size_t i = 0; i < L; ++i) {
            if (site_map[i] > 0xFFFFFFFFull) return fail(WLD_E_ARG, "site_map[%zu] exceeds 32 bits", i);
            m[i] = (uint32_t)site_map[i];
        }
        c->has_pos = true;
        WLD_TRY(ensure(c->site_map, std::max<size_t>(L, 1) * sizeof(uint32_t)));
        if (L) HIP_TRY(hipMemcpyAsync(c->site_map.p, m.data(), L * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    // a window set before the load: its plan for this set (a site_map that
    // descends fails a distance window here)
    c->win_hi_host.clear();
    c->win_pre.clear();
    c->win_live_pre.clear();
    if (c->win_d || c->win_k) WLD_TRY(window_prepare(c));
    c->wst = MfmaWeightStats{7, 1, {0, 0, 0}, {0, 0, 0, 0}};
    if (c->kernel == WLD_KERNEL_MFMA && mfma_weight_stats(ptr<int8_t>(c->planes), c->LP, c->NP, c->stream, &c->wst))
        return fail(WLD_E_HIP, "reading the weight-plane statistics failed");
    const unsigned all_planes = (1u << c->fixed_planes) - 1;
    c->plane_mask = c->kernel == WLD_KERNEL_MFMA && !c->opt_all_planes ? c->wst.plane_mask : all_planes;
    c->stats.load_ms = event_ms(c->ev[0], c->ev[1]);
    c->fp6_ok = c->fp6_better = c->fp6_tried = false;  // (fp6_prepare: at the first run that may use it)
    c->i8img_ok = false;  // (i8img_prepare: at the first pass that screens on i8)
    c->stats.mfma_planes = c->kernel == WLD_KERNEL_MFMA ? __builtin_popcount(c->plane_mask) : 0;
    c->stats.kernel = c->kernel;
    c->stats.weight_shift = c->shift;
    c->loaded = true;
    c->have_rows = false;
    c->tiles_lb = c->tiles_le = ~0u;
    // what a first run would otherwise build: the fp6 screen's operands (not
    // with WLD_OPT_SCREEN_FP6 0), lib.rs's lane-class layout (WLD_OPT_REF_SUMS),
    // the whole set's tile lists; a fresh context's first pass then costs
    // about a steady one (a run over a shard builds its own
    // lists on its first pass)
    if (c->opt_fp6 != 0) WLD_TRY(fp6_prepare(c));
    if (c->opt_ref_sums) WLD_TRY(ensure_ref_layout(c));
    {  // a run's pair count in O(1) (the per-chunk loop took microseconds per run);
       // up to 2^24 chunks (128 MB of prefix; ~1.48M sites), beyond that per run
        const uint32_t m = chunks_of(L), nr = chunk_rows_of(L);
        c->chunk_pairs_pre.assign(m <= (1u << 24) ? (size_t)m + 1 : 0, 0);
        for (uint32_t i = 0; i < m && m <= (1u << 24); ++i) {
            uint32_t row, col;
            chunk_of_linear_host(nr, i, row, col);
            c->chunk_pairs_pre[i + 1] = c->chunk_pairs_pre[i] + pairs_in_chunk(L, row, col);
        }
    }
    // the whole set's tile lists only where a whole-set run is possible (<=
    // 2^32 pairs, run_enqueue's limit; about 92,700 sites) and the lists stay
    // small (<= 2^22 tiles: 512 MB of candidate-list space at most); larger
    // sets run only as shards, whose first run builds its own lists
    {
        const uint64_t T_used = (L + kTile - 1) / kTile;
        if ((uint64_t)L * (L - 1) / 2 <= 0xFFFFFFFFull && T_used * (T_used + 1) / 2 <= (1ull << 22))
            WLD_TRY(build_tiles(c, 0, chunks_of(L), true));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return WLD_OK;
}

bool window_on(const wld_ctx *c) { return c->win_d != 0 || c->win_k != 0; }

// The window's plan for the loaded set (window_plan.hpp): hi[] on the host
// (tile lists, pair counts, shards) and, by window_limits_kernel from the
// resident site_map, on the device (the kernels' pass test), the per-chunk
// in-window pair counts on both.  Needs L, LP and the site map of the load;
// runs when a load meets a window or a window meets a load.
int window_prepare(wld_ctx *c) {
    const uint32_t L = (uint32_t)c->L;
    const uint32_t *pos = c->has_pos ? c->pos_host.data() : nullptr;
    if (c->win_d && pos) {
        const uint32_t i = window_plan::first_descent(pos, L);
        if (i < L)
            return fail(WLD_E_ARG, "a distance window (max_distance %llu) needs a non-decreasing site_map: "
                                   "site_map[%u] = %u < site_map[%u] = %u",
                        (unsigned long long)c->win_d, i, pos[i], i - 1, pos[i - 1]);
    }
    const uint32_t m = chunks_of(L);
    if (m > (1u << 24))
        return fail(WLD_E_ARG, "a window's plan covers up to 2^24 chunks; %zu sites have %u", c->L, m);
    c->win_hi_host = window_plan::limits(pos, L, c->win_d, c->win_k);
    c->win_pre = window_plan::chunk_prefix(c->win_hi_host);
    c->win_live_pre.assign((size_t)m + 1, 0);
    std::vector<uint32_t> cnt(std::max<uint32_t>(m, 1), 0);
    for (uint32_t i = 0; i < m; ++i) {
        cnt[i] = (uint32_t)(c->win_pre[i + 1] - c->win_pre[i]);  // (<= 256 x 256)
        c->win_live_pre[i + 1] = c->win_live_pre[i] + (cnt[i] ? 1u : 0u);
    }
    WLD_TRY(ensure(c->win_pairs, cnt.size() * sizeof(uint32_t)));
    WLD_TRY(ensure(c->win_hi, c->LP * sizeof(uint32_t)));
    HIP_TRY(hipMemcpyAsync(c->win_pairs.p, cnt.data(), cnt.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    launch_window_limits(c->has_pos ? ptr<uint32_t>(c->site_map) : nullptr, L, (uint32_t)c->LP, c->win_d, c->win_k,
                         ptr<uint32_t>(c->win_hi), c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));  // (cnt is read by the copy)
    c->tiles_lb = c->tiles_le = ~0u;  // the tile lists follow the window
    return WLD_OK;
}

// pairs of the linear chunks [lb, le) that a run computes: the in-window ones
// under a window, else every pair a < b
uint64_t pairs_in_chunks(size_t L, uint32_t lb, uint32_t le);
uint64_t run_pairs(const wld_ctx *c, uint32_t lb, uint32_t le) {
    if (window_on(c) && c->win_pre.size() > le) return c->win_pre[le] - c->win_pre[lb];
    if (c->chunk_pairs_pre.size() > le) return c->chunk_pairs_pre[le] - c->chunk_pairs_pre[lb];
    return pairs_in_chunks(c->L, lb, le);
}

uint32_t chunk_rows_of(size_t L) { return (uint32_t)((L + kChunk - 1) / kChunk); }

uint64_t pairs_in_rows(size_t L, uint32_t rb, uint32_t re) {
    // pairs (a<b) with a in [rb*256, re*256) ∩ [0, L)
    uint64_t a0 = std::min<uint64_t>(L, (uint64_t)rb * kChunk), a1 = std::min<uint64_t>(L, (uint64_t)re * kChunk);
    uint64_t s = 0;
    // sum_{a=a0}^{a1-1} (L-1-a)
    if (a1 > a0) s = (a1 - a0) * (uint64_t)(L - 1) - (a1 - 1 + a0) * (a1 - a0) / 2;
    return s;
}

uint32_t chunks_of(size_t L) {
    const uint32_t n = chunk_rows_of(L);
    return n * (n + 1) / 2;
}

// (row, col) of linear chunk i: triu_index (lib.rs:623-632) in exact integers
void chunk_of_linear_host(uint32_t n, uint32_t i, uint32_t &row, uint32_t &col) {
    uint32_t rf = (uint32_t)((std::sqrt(8.0 * (double)i + 1.0) - 1.0) * 0.5);
    while ((uint64_t)(rf + 1) * (rf + 2) / 2 <= i) ++rf;
    while ((uint64_t)rf * (rf + 1) / 2 > i) --rf;
    row = n - rf - 1;
    col = row + i - rf * (rf + 1) / 2;
}

// pairs (a<b) of chunk (row, col): lib.rs:636-667's a/b loops
uint64_t pairs_in_chunk(size_t L, uint32_t row, uint32_t col) {
    auto side = [&](uint32_t r) -> uint64_t {
        const uint64_t lo = (uint64_t)r * kChunk;
        return lo >= L ? 0 : std::min<uint64_t>(L - lo, kChunk);
    };
    const uint64_t ra = side(row);
    return row == col ? ra * (ra ? ra - 1 : 0) / 2 : ra * side(col);
}

uint64_t pairs_in_chunks(size_t L, uint32_t lb, uint32_t le) {
    const uint32_t n = chunk_rows_of(L);
    uint64_t s = 0;
    for (uint32_t i = lb; i < le; ++i) {
        uint32_t r, c;
        chunk_of_linear_host(n, i, r, c);
        s += pairs_in_chunk(L, r, c);
    }
    return s;
}

// linear chunk range of chunk rows [rb, re): rows descend in linear order
void rows_to_linear(uint32_t n, uint32_t rb, uint32_t re, uint32_t &lb, uint32_t &le) {
    lb = re > rb ? chunk_linear(n, re - 1, re - 1) : 0;
    le = re > rb ? chunk_linear(n, rb, rb) + (n - rb) : 0;
}

// xcd_order and range_tiles: tile_order.hpp
using tile_order::xcd_order;

// windowed: the list is cut to the context's window, if it has one (every
// run); false: every tile (wld_dense, which ignores the window).  The cached
// list is kept only for the same range AND the same window.
int build_tiles(wld_ctx *c, uint32_t lb, uint32_t le, bool windowed) {
    windowed = windowed && window_on(c);
    const uint64_t wd = windowed ? c->win_d : 0, wk = windowed ? c->win_k : 0;
    if (c->tiles_lb == lb && c->tiles_le == le && c->n_tiles && c->tiles_windowed == windowed &&
        c->tiles_win_d == wd && c->tiles_win_k == wk)
        return WLD_OK;
    const uint32_t T_used = (uint32_t)((c->L + kTile - 1) / kTile);
    const uint32_t n = chunk_rows_of(c->L);
    // (ta, tb) order; under a window only the tiles holding an in-window pair
    std::vector<uint32_t> t = windowed ? window_plan::range_tiles(n, T_used, lb, le, c->win_hi_host)
                                       : tile_order::range_tiles(n, T_used, lb, le);
    c->n_tiles_listed = (uint32_t)t.size();
    c->tiles_windowed = windowed;
    c->tiles_win_d = wd;
    c->tiles_win_k = wk;
    // a tile left out of the list is never written, and the gather reads the
    // segment counts of all four b tiles of a chunk with rows: they must read
    // as zero, whatever an earlier run (a wider window, none) left there
    if (windowed) c->seg_clear = true;
    const uint32_t kS = tile_order::super_block_side((uint32_t)c->NP);
    // the fp6 screen's tile pairs (ordered as the tiles below, by first tile;
    // single tiles keep their flag through the ordering)
    std::vector<uint32_t> pl;
    if (T_used <= 0x7FFF && (int64_t)t.size() >= c->opt_fp6_pairs_min) {
        pl = tile_order::fp6_pair_list(t);
        if (!c->opt_tile_rows && pl.size() >= 2048) pl = xcd_order(pl, kS, ~tile_order::kSingleEntry);
    }
    // only with many rounds of resident tiles: whole super-blocks per XCD
    // leave up to one super-block of imbalance (C2's 528 tiles: +14%)
    if (!c->opt_tile_rows && t.size() >= 4096 && T_used < 65535) t = xcd_order(t, kS);
    c->n_tiles = (uint32_t)t.size();
    WLD_TRY(ensure(c->tiles, std::max<size_t>(t.size(), 1) * sizeof(uint32_t)));
    // screen candidates: 16 weight buckets of tiles, then of their sub-block bits
    WLD_TRY(ensure(c->cand, std::max<size_t>(t.size(), 1) * 32 * sizeof(uint32_t)));
    if (!t.empty())
        HIP_TRY(hipMemcpyAsync(c->tiles.p, t.data(), t.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    c->f6_n_pairs = (uint32_t)pl.size();
    if (!pl.empty()) {
        WLD_TRY(ensure(c->f6_pairs, pl.size() * sizeof(uint32_t)));
        HIP_TRY(hipMemcpyAsync(c->f6_pairs.p, pl.data(), pl.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                               c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->tiles_lb = lb;
    c->tiles_le = le;
    return WLD_OK;
}

OrderArgs order_args(wld_ctx *c) {
    OrderArgs o;
    o.st_a = ptr<uint32_t>(c->st_a);
    o.st_b = ptr<uint32_t>(c->st_b);
    o.st_d = ptr<float>(c->st_d);
    o.st_dp = ptr<float>(c->st_dp);
    o.st_r2 = ptr<float>(c->st_r2);
    o.st_capacity = c->st_capacity;
    o.seg_cnt = ptr<uint8_t>(c->seg_cnt);
    o.seg_off = ptr<uint32_t>(c->seg_off);
    o.T = (uint32_t)(c->LP / kTile);
    o.chunk_total = ptr<uint32_t>(c->chunk_total);
    o.cursor = ptr<unsigned long long>(c->counters);
    o.chunk_left = c->prog_pass ? ptr<unsigned>(c->chunk_left) : nullptr;
    o.prog_n = c->prog_pass ? ptr<unsigned>(c->prog_n) : nullptr;
    o.prog_log = c->prog_pass ? c->d_plog : nullptr;
    o.L = (uint32_t)c->L;
    o.guard = reinterpret_cast<unsigned *>(c->d_hcnt + 4);
    // (the list in use is the window's: every run; wld_dense builds the full one)
    o.win_hi = c->tiles_windowed ? ptr<uint32_t>(c->win_hi) : nullptr;
    o.win_pairs = c->tiles_windowed ? ptr<uint32_t>(c->win_pairs) : nullptr;
    return o;
}

// WLD_OPT_REF_SUMS: the codes and weights in the reference's lane-class order
// (pair_valu.hip), built once per load on first use
int ensure_ref_layout(wld_ctx *c) {
    if (c->have_ref) return WLD_OK;
    uint32_t tail = 0;
    ref_layout_dims(c->N, &c->ref_cls, &tail, &c->NPr);
    WLD_TRY(ensure(c->rcodes, c->LP * c->NPr));
    WLD_TRY(ensure(c->rw, c->NPr * sizeof(float)));
    launch_ref_layout(ptr<uint8_t>(c->codes), ptr<float>(c->w_pad), c->LP, c->NP, c->N, ptr<uint8_t>(c->rcodes),
                      ptr<float>(c->rw), c->stream);
    HIP_TRY(hipGetLastError());
    c->have_ref = true;
    return WLD_OK;
}

// How far (2x2-cell L1, fixed-point units of the weight planes) the
// reference's f32 sums can lie from the fixed-point sums the screen bounds:
// each weight is within 0.5 of w 2^shift (every sequence in one cell), and
// each of the four f32 sums within gamma_m sum|w| of its exact value
// (recursive summation: every term passes through at most m = N/8 + 16
// roundings — its lane chain, the horizontal sum, the scalar tail); the
// cells are n11 = SAB, n10 = SA - SAB, n01 = SB - SAB, n00 = T - SA - SB +
// SAB, so their L1 error is at most 9 times a sum's.  sum|q| <= sum_p 2^(8p)
// sum|d_p|.
double ref_extra_residual(const wld_ctx *c) {
    const double u = 0x1p-24, m = (double)(c->N / 8) + 16.0;
    const double gamma = m * u / (1.0 - m * u);
    double qsum = 0.0;
    for (int p = 0; p < 4; ++p) qsum += std::ldexp((double)c->wst.dsum[p], 8 * p);
    const double r = 9.0 * gamma * (qsum + 0.5 * (double)c->N) + 0.5 * (double)c->N;
    return r * (1.0 + 1e-9) + 1.0;  // slack for this evaluation's own rounding
}

// The policy's view of the context and of a pass at thr (screen_policy.hpp).
struct PolicyInputs {
    screen_policy::Options opt;
    screen_policy::LoadFacts load;
    screen_policy::PassFacts pass;
};
PolicyInputs policy_inputs(const wld_ctx *c, float thr, bool dense) {
    return {{c->opt_screen, c->opt_fp6, c->opt_ref_sums, c->opt_prefilter, c->opt_i8_pairs, c->opt_fp6_three,
             c->opt_fp6_quick},
            {c->kernel == WLD_KERNEL_MFMA, c->use_frag, c->wst.nonneg != 0, c->NP, c->plane_mask, c->fp6_ok,
             c->fp6_better},
            {c->f6_n_pairs != 0, c->n_tiles, thr, dense, c->prog_pass, c->pend.count_out != nullptr}};
}

// The tile list on the reference-order f32 kernel (lane-class layout: after ensure_ref_layout).
ValuLaunch ref_valu_launch(wld_ctx *c, float thr) {
    return ValuLaunch{ptr<uint8_t>(c->rcodes), ptr<float>(c->rw), ptr<uint8_t>(c->site_ok), ptr<uint32_t>(c->tiles),
                      c->n_tiles, nullptr, (uint32_t)c->L, (uint32_t)c->NPr, chunk_rows_of(c->L), thr, c->safe, false,
                      true, c->ref_cls, (uint32_t)(c->N % 8)};
}

// What every MFMA launch of the tile list at thr needs (the pass and the fp6 sample run).
MfmaLaunch mfma_base(wld_ctx *c, float thr) {
    MfmaLaunch m{};
    m.wplanes = ptr<int8_t>(c->planes);
    m.tiles = ptr<uint32_t>(c->tiles);
    m.n_tiles = c->n_tiles;
    m.L = (uint32_t)c->L;
    m.NP = (uint32_t)c->NP;
    m.LP = (uint32_t)c->LP;
    m.n_chunk_rows = chunk_rows_of(c->L);
    m.thr = thr;
    m.nonneg = c->wst.nonneg;
    m.fp6 = &c->f6;
    m.f6_pairs = c->f6_n_pairs ? ptr<uint32_t>(c->f6_pairs) : nullptr;
    m.f6_n_pairs = c->f6_n_pairs;
    return m;
}

// Enqueues the pair kernel(s) of a pass on the route the screen policy
// decides; *pass receives the plan as launched (where a screen ran, ev[6]
// separates it from the candidate launch).
// With scan given, a screen fuses the run's chunk scan into its last
// workgroup or the candidate launch's (then the caller launches no scan).
int launch_pairs(wld_ctx *c, float thr, const OrderArgs &o, const DenseArgs *dense,
                 screen_policy::Plan *pass = nullptr, const ScanArgs *scan = nullptr, bool *scan_fused = nullptr) {
    using screen_policy::Route;
    bool fused = false;  // the run's chunk scan ran inside a launch (the caller launches none)
    c->stats.ref_sums = c->opt_ref_sums ? 1 : 0;
    const PolicyInputs in = policy_inputs(c, thr, dense != nullptr);
    screen_policy::Plan plan = screen_policy::decide(in.opt, in.load, in.pass, c->learned);
    ValuLaunch rv{};
    if (c->opt_ref_sums) {
        WLD_TRY(ensure_ref_layout(c));
        rv = ref_valu_launch(c, thr);
    }
    // the i8 screen on tile pairs (WLD_OPT_I8_PAIRS): its images built at the
    // first pass that needs them, and used only while they hold the top
    // active plane (else single tiles)
    if (plan.i8_images) {
        if (!c->i8img_ok) WLD_TRY(i8img_prepare(c));
        plan.route = screen_policy::settle_i8(plan.route, c->i8s.digit_plane, c->plane_mask);
    }
    // (a full run on the item kernel fuses the scan into its last workgroup)
    if (scan && !dense) rv.scan = *scan;
    if (plan.route == Route::F32RefOrder) {
        fused = launch_pair_valu(rv, o, dense, c->stream);
    } else if (plan.route == Route::F32Plain) {
        launch_pair_valu(ValuLaunch{ptr<uint8_t>(c->codes), ptr<float>(c->w_pad), ptr<uint8_t>(c->site_ok),
                                    ptr<uint32_t>(c->tiles), c->n_tiles, nullptr, (uint32_t)c->L, (uint32_t)c->NP,
                                    chunk_rows_of(c->L), thr, c->safe, c->opt_valu_plain, false, 0, 0},
                         o, dense, c->stream);
    } else {
        MfmaLaunch m = mfma_base(c, thr);
        m.codes = ptr<uint8_t>(c->codes);
        m.frag = c->use_frag ? ptr<uint8_t>(c->frag) : nullptr;
        m.frag_b = c->use_frag ? ptr<uint8_t>(c->frag) + c->LP * c->NP : nullptr;
        m.shift = c->shift;
        m.plane_mask = c->plane_mask;
        m.route = plan.route;
        m.bound_test = plan.bound_test;
        m.fp6_bail = plan.fp6_bail;
        m.fp6_three = plan.fp6_three;
        m.fp6_quick = plan.fp6_quick;
        m.f6_rechecked = reinterpret_cast<unsigned *>(ptr<unsigned long long>(c->counters) + kF6Rechecked);
        m.i8img = &c->i8s;
        for (int t = 0; t < 3; ++t) m.resid[t] = c->wst.resid[t];
        for (int p = 0; p < 4; ++p) m.dsum[p] = c->wst.dsum[p];
        m.cand_list = ptr<uint32_t>(c->cand);
        // this pass's candidate set (the scan zeroes the other one, enqueue_pass)
        unsigned long long *set = ptr<unsigned long long>(c->counters) + kCandSet0 + kCandSetWords * c->cand_set;
        m.cand_count = reinterpret_cast<unsigned *>(set);
        m.cand_work = reinterpret_cast<unsigned *>(ptr<unsigned long long>(c->counters) + 2) + 1;  // beside the ticket
        m.cand_buckets = reinterpret_cast<unsigned *>(set + 1);
        m.test_guard = c->opt_test_guard;
        if (scan && !dense) m.scan = *scan;
        RefRowsLaunch rr{};
        if (c->opt_ref_sums) {  // lib.rs's order behind the integer kernel: the candidates' sums, the bound's slack
            m.ref_valu = &rv;
            m.r_extra_q = ref_extra_residual(c);
            if (plan.route == Route::CandidatePairs) {
                rr = RefRowsLaunch{ptr<uint8_t>(c->rcodes), ptr<float>(c->rw), (uint32_t)c->NPr, c->ref_cls,
                                   (uint32_t)(c->N % 8), m.n_chunk_rows, thr, nullptr, nullptr, nullptr, ScanArgs{}};
                m.ref_rows = &rr;
            }
        }
        launch_pair_mfma(m, o, dense, c->stream, c->ev[6]);
        // (a screen's candidate launch, or the candidate pairs' compaction)
        fused = screen_policy::ran_screen(plan.route) && scan && !dense;
    }
    HIP_TRY(hipGetLastError());
    if (pass) *pass = plan;
    if (scan_fused) *scan_fused = fused;
    return WLD_OK;
}

}  // namespace

extern "C" {

const char *wld_version(void) { return "weightedld-amd 0.1.0 (gfx950)"; }

int wld_create(int device, wld_ctx **out) {
    if (!out) return fail(WLD_E_ARG, "wld_create: null out");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        (void)hipGetLastError();
        return fail(WLD_E_NODEV, "no HIP device visible (%s); the weightedld hot path runs only on a gfx950 GPU",
                    e == hipSuccess ? "0 devices" : hipGetErrorString(e));
    }
    if (device < 0 || device >= n) return fail(WLD_E_ARG, "device %d out of range (%d visible)", device, n);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        return fail(WLD_E_NODEV, "device %d is %s, not gfx950 (MI355X)", device, prop.gcnArchName);
    HIP_TRY(hipSetDevice(device));
    auto *c = new wld_ctx;
    c->device = device;
    hipError_t es = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    c->stream = c->own_stream;
    if (es != hipSuccess) {
        delete c;
        return fail(WLD_E_HIP, "hipStreamCreate: %s", hipGetErrorString(es));
    }
    for (auto &ev : c->ev)
        if (hipEventCreate(&ev) != hipSuccess) {
            delete c;
            return fail(WLD_E_HIP, "hipEventCreate failed");
        }
    if (hipHostMalloc((void **)&c->h_cnt, 6 * sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent) !=
            hipSuccess ||
        hipHostGetDevicePointer((void **)&c->d_hcnt, c->h_cnt, 0) != hipSuccess) {
        (void)hipGetLastError();
        delete c;
        return fail(WLD_E_HIP, "hipHostMalloc of the run counters failed");
    }
    *out = c;
    return WLD_OK;
}

int wld_create_multi(const int *devices, int n_devices, wld_ctx **out) {
    if (!out) return fail(WLD_E_ARG, "wld_create_multi: null out");
    *out = nullptr;
    if (!devices || n_devices < 1) return fail(WLD_E_ARG, "wld_create_multi: need at least one device");
    if (n_devices == 1) return wld_create(devices[0], out);  // a plain context: every entry point works
    auto *g = new wld_ctx;
    g->device = devices[0];
    for (int k = 0; k < n_devices; ++k) {
        wld_ctx *m = nullptr;
        const int st = wld_create(devices[k], &m);
        if (st != WLD_OK) {
            delete g;
            return st;
        }
        g->members.push_back(m);
    }
    *out = g;
    return WLD_OK;
}

int wld_n_devices(const wld_ctx *ctx) { return !ctx ? 0 : ctx->members.empty() ? 1 : (int)ctx->members.size(); }

void wld_destroy(wld_ctx *ctx) { delete ctx; }

int wld_set_kernel(wld_ctx *ctx, int kernel) {
    if (!ctx) return fail(WLD_E_ARG, "null context");
    for (wld_ctx *m : ctx->members) WLD_TRY(wld_set_kernel(m, kernel));
    if (kernel < WLD_KERNEL_AUTO || kernel > WLD_KERNEL_MFMA) return fail(WLD_E_ARG, "bad kernel id %d", kernel);
    if (kernel == WLD_KERNEL_MFMA && !mfma_supported()) return fail(WLD_E_ARG, "MFMA kernel not built");
    ctx->kernel_pref = kernel;
    return WLD_OK;
}

int wld_set_option(wld_ctx *c, int option, int64_t value) {
    if (!c) return fail(WLD_E_ARG, "null context");
    for (wld_ctx *m : c->members) WLD_TRY(wld_set_option(m, option, value));
    if (c->pend.active) return fail(WLD_E_STATE, "wld_set_option during a run");
    switch (option) {
        case WLD_OPT_PREFILTER: c->opt_prefilter = value != 0; break;
        case WLD_OPT_SCREEN:
            if (value < 0 || value > 4) return fail(WLD_E_ARG, "WLD_OPT_SCREEN takes 0 to 4");
            c->opt_screen = (int)value;
            c->learned.reset();
            break;
        case WLD_OPT_TILE_ORDER:
            c->opt_tile_rows = value != 0;
            c->tiles_lb = c->tiles_le = ~0u;  // rebuild the list at the next run
            break;
        case WLD_OPT_ALL_PLANES:
            c->opt_all_planes = value != 0;
            if (c->loaded && c->kernel == WLD_KERNEL_MFMA)
                c->plane_mask = c->opt_all_planes ? (1u << c->fixed_planes) - 1 : c->wst.plane_mask;
            if (c->loaded) c->stats.mfma_planes = c->kernel == WLD_KERNEL_MFMA ? __builtin_popcount(c->plane_mask) : 0;
            break;
        case WLD_OPT_MFMA_LAYOUT: c->opt_site_major = value != 0; break;
        case WLD_OPT_VALU_PLAIN: c->opt_valu_plain = value != 0; break;
        case WLD_OPT_REF_SUMS:
            c->opt_ref_sums = value != 0;
            c->learned.reset();  // the policy's break-even differs
            break;
        case WLD_OPT_STAGING_ROWS:
            if (value < 1) return fail(WLD_E_ARG, "WLD_OPT_STAGING_ROWS must be >= 1");
            c->opt_staging_rows = (uint64_t)value;
            break;
        case WLD_OPT_HOST_BATCH_PAIRS:
            if (value < 1) return fail(WLD_E_ARG, "WLD_OPT_HOST_BATCH_PAIRS must be >= 1");
            c->opt_host_batch_pairs = (uint64_t)value;
            break;
        case WLD_OPT_TARGET_BATCH_SLOTS:
            if (value < 1) return fail(WLD_E_ARG, "WLD_OPT_TARGET_BATCH_SLOTS must be >= 1");
            c->opt_target_slots = (uint64_t)value;
            break;
        case WLD_OPT_PARTNERS_BATCH_BYTES:
            if (value < 1) return fail(WLD_E_ARG, "WLD_OPT_PARTNERS_BATCH_BYTES must be >= 1");
            c->opt_partners_bytes = (uint64_t)value;
            break;
        case WLD_OPT_MATRIX_BATCH_BYTES:
            if (value < 1) return fail(WLD_E_ARG, "WLD_OPT_MATRIX_BATCH_BYTES must be >= 1");
            c->opt_matrix_bytes = (uint64_t)value;
            break;
        case WLD_OPT_FUSED_SCAN: c->opt_fused_scan = value != 0; break;
        case WLD_OPT_I8_PAIRS: c->opt_i8_pairs = value != 0; break;
        case WLD_OPT_TEST_GUARD: c->opt_test_guard = value != 0; break;
        case WLD_OPT_FP6_PAIRS_MIN_TILES:
            if (value < 0) return fail(WLD_E_ARG, "WLD_OPT_FP6_PAIRS_MIN_TILES must be >= 0");
            c->opt_fp6_pairs_min = value;
            c->tiles_lb = c->tiles_le = ~0u;  // rebuild the lists at the next run
            break;
        case WLD_OPT_SCREEN_FP6:
            if (value < 0 || value > 3) return fail(WLD_E_ARG, "WLD_OPT_SCREEN_FP6 takes 0 to 3");
            c->opt_fp6 = (int)value;
            c->learned.reset();  // another screen's break-even
            break;
        case WLD_OPT_FP6_A4:
            c->opt_fp6_a4 = value != 0;
            // the A image's format may change: rebuilt by the next run that may screen on fp6
            c->fp6_ok = c->fp6_better = c->fp6_tried = false;
            break;
        case WLD_OPT_FP6_SHARED:
            c->opt_fp6_shared = value != 0;
            // the operand images may change: rebuilt by the next run that may screen on fp6
            c->fp6_ok = c->fp6_better = c->fp6_tried = false;
            break;
        case WLD_OPT_FP6_THREE:
            if (value < 0 || value > 2) return fail(WLD_E_ARG, "WLD_OPT_FP6_THREE takes 0 to 2");
            c->opt_fp6_three = (int)value;
            c->learned.reset();  // (what a sample run counts depends on it)
            break;
        case WLD_OPT_FP6_QUICK:
            if (value < 0 || value > 2) return fail(WLD_E_ARG, "WLD_OPT_FP6_QUICK takes 0 to 2");
            c->opt_fp6_quick = (int)value;
            c->learned.reset();  // (what a sample run counts depends on it)
            break;
        default: return fail(WLD_E_ARG, "unknown option %d", option);
    }
    return WLD_OK;
}

int wld_fp6_weight_codes(wld_ctx *c, uint8_t *codes, int *fits_fp4) {
    if (!c || !codes || !fits_fp4) return fail(WLD_E_ARG, "null argument");
    if (!c->members.empty()) return fail(WLD_E_ARG, "wld_fp6_weight_codes takes a single-device context");
    if (c->pend.active) return fail(WLD_E_STATE, "wld_fp6_weight_codes during a run");
    if (!c->loaded || !c->fp6_ok) return fail(WLD_E_STATE, "the loaded set has no fp6 operands");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(codes, c->w6.p, c->N, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *fits_fp4 = fp6_codes_fit_fp4(codes, c->N) ? 1 : 0;
    return WLD_OK;
}

int wld_set_window(wld_ctx *c, uint64_t max_distance, uint64_t max_sites) {
    if (!c) return fail(WLD_E_ARG, "null context");
    if (c->pend.active) return fail(WLD_E_STATE, "wld_set_window during a run");
    for (wld_ctx *m : c->members)
        if (m->pend.active) return fail(WLD_E_STATE, "wld_set_window during a run");
    if (!c->members.empty()) {
        // every member gets the window; one that refuses it (a descending
        // site_map) leaves the group on the window it had
        for (size_t k = 0; k < c->members.size(); ++k) {
            const int st = wld_set_window(c->members[k], max_distance, max_sites);
            if (st != WLD_OK) {
                const std::string msg = wld_last_error();
                for (size_t j = 0; j < k; ++j) (void)wld_set_window(c->members[j], c->win_d, c->win_k);
                return fail(st, "%s", msg.c_str());
            }
        }
        c->win_d = max_distance;
        c->win_k = max_sites;
        return WLD_OK;
    }
    if (c->win_d == max_distance && c->win_k == max_sites) return WLD_OK;
    const uint64_t old_d = c->win_d, old_k = c->win_k;
    c->win_d = max_distance;
    c->win_k = max_sites;
    if (c->loaded && window_on(c)) {
        int st = set_dev(c);
        if (st == WLD_OK) st = window_prepare(c);
        if (st != WLD_OK) {  // (a descending site_map under max_distance: the window stays as it was)
            c->win_d = old_d;
            c->win_k = old_k;
            return st;
        }
    }
    c->tiles_lb = c->tiles_le = ~0u;  // the tile lists follow the window
    // the auto screen policy learned its thresholds on another set of tiles
    c->learned.reset();
    return WLD_OK;
}

int wld_get_window(wld_ctx *c, uint64_t *max_distance, uint64_t *max_sites) {
    if (!c) return fail(WLD_E_ARG, "null context");
    if (max_distance) *max_distance = c->win_d;
    if (max_sites) *max_sites = c->win_k;
    return WLD_OK;
}

int wld_window_pairs_in_chunks(wld_ctx *c, uint32_t begin, uint32_t end, uint64_t *pairs) {
    if (!c || !pairs) return fail(WLD_E_ARG, "null argument");
    if (!c->members.empty()) c = c->members[0];
    if (!c->loaded) return fail(WLD_E_STATE, "wld_window_pairs_in_chunks before wld_load");
    const uint32_t m = chunks_of(c->L);
    end = std::min(end, m);
    *pairs = begin < end ? run_pairs(c, begin, end) : 0;
    return WLD_OK;
}

int wld_shard_chunks_window(wld_ctx *c, int n_shards, int shard, uint32_t *begin, uint32_t *end) {
    if (!c) return fail(WLD_E_ARG, "null context");
    if (!c->members.empty()) c = c->members[0];
    if (!c->loaded) return fail(WLD_E_STATE, "wld_shard_chunks_window before wld_load");
    if (!window_on(c)) return wld_shard_chunks(c->L, n_shards, shard, begin, end);
    if (n_shards < 1 || shard < 0 || shard >= n_shards || !begin || !end)
        return fail(WLD_E_ARG, "bad shard %d/%d", shard, n_shards);
    window_plan::shard_range(c->win_pre, n_shards, shard, begin, end);
    return WLD_OK;
}

int wld_window_limits_copy(wld_ctx *c, uint32_t *hi) {
    WLD_TRY(set_dev(c));
    if (!c->loaded) return fail(WLD_E_STATE, "wld_window_limits_copy before wld_load");
    if (!window_on(c)) return fail(WLD_E_STATE, "wld_window_limits_copy without a window");
    if (!hi && c->L) return fail(WLD_E_ARG, "wld_window_limits_copy: null output");
    if (c->L) HIP_TRY(hipMemcpyAsync(hi, c->win_hi.p, c->L * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return WLD_OK;
}

int wld_get_option(wld_ctx *c, int option, int64_t *value) {
    if (!c || !value) return fail(WLD_E_ARG, "null argument");
    switch (option) {
        case WLD_OPT_PREFILTER: *value = c->opt_prefilter; break;
        case WLD_OPT_SCREEN: *value = c->opt_screen; break;
        case WLD_OPT_TILE_ORDER: *value = c->opt_tile_rows; break;
        case WLD_OPT_ALL_PLANES: *value = c->opt_all_planes; break;
        case WLD_OPT_MFMA_LAYOUT: *value = c->opt_site_major; break;
        case WLD_OPT_VALU_PLAIN: *value = c->opt_valu_plain; break;
        case WLD_OPT_REF_SUMS: *value = c->opt_ref_sums; break;
        case WLD_OPT_STAGING_ROWS: *value = (int64_t)c->opt_staging_rows; break;
        case WLD_OPT_HOST_BATCH_PAIRS: *value = (int64_t)c->opt_host_batch_pairs; break;
        case WLD_OPT_TARGET_BATCH_SLOTS: *value = (int64_t)c->opt_target_slots; break;
        case WLD_OPT_PARTNERS_BATCH_BYTES: *value = (int64_t)c->opt_partners_bytes; break;
        case WLD_OPT_MATRIX_BATCH_BYTES: *value = (int64_t)c->opt_matrix_bytes; break;
        case WLD_OPT_FUSED_SCAN: *value = c->opt_fused_scan; break;
        case WLD_OPT_TEST_GUARD: *value = c->opt_test_guard; break;
        case WLD_OPT_FP6_PAIRS_MIN_TILES: *value = c->opt_fp6_pairs_min; break;
        case WLD_OPT_SCREEN_FP6: *value = c->opt_fp6; break;
        case WLD_OPT_I8_PAIRS: *value = c->opt_i8_pairs; break;
        case WLD_OPT_FP6_A4: *value = c->opt_fp6_a4; break;
        case WLD_OPT_FP6_SHARED: *value = c->opt_fp6_shared; break;
        case WLD_OPT_FP6_THREE: *value = c->opt_fp6_three; break;
        case WLD_OPT_FP6_QUICK: *value = c->opt_fp6_quick; break;
        default: return fail(WLD_E_ARG, "unknown option %d", option);
    }
    return WLD_OK;
}

int wld_load(wld_ctx *c, const uint8_t *sites, size_t n_sites, size_t n_seqs, const uint64_t *site_map,
             const float *weights) {
    if (c && !c->members.empty()) {
        // every device gets the whole input (replicated; it is small next to
        // the pair space), loaded concurrently
        const size_t G = c->members.size();
        std::vector<int> st(G, WLD_OK);
        std::vector<std::string> msg(G);
        std::vector<std::thread> th;
        for (size_t k = 0; k < G; ++k)
            th.emplace_back([&, k] {
                st[k] = wld_load(c->members[k], sites, n_sites, n_seqs, site_map, weights);
                if (st[k] != WLD_OK) msg[k] = wld_last_error();
            });
        for (auto &t : th) t.join();
        for (size_t k = 0; k < G; ++k)
            if (st[k] != WLD_OK) return fail(st[k], "device %d: %s", c->members[k]->device, msg[k].c_str());
        c->stats = c->members[0]->stats;
        return WLD_OK;
    }
    WLD_TRY(set_dev(c));
    if ((!sites && n_sites * n_seqs) || (!weights && n_seqs)) return fail(WLD_E_ARG, "wld_load: null input");
    if (n_sites >= (1u << 16) * (size_t)kTile) return fail(WLD_E_ARG, "n_sites %zu too large", n_sites);
    c->loaded = false;
    c->prepass_loaded = false;
    c->L = n_sites;
    c->N = n_seqs;
    WLD_TRY(ensure(c->raw, n_sites * n_seqs));
    WLD_TRY(ensure(c->wraw, n_seqs * sizeof(float)));
    if (n_sites * n_seqs)
        HIP_TRY(hipMemcpyAsync(c->raw.p, sites, n_sites * n_seqs, hipMemcpyHostToDevice, c->stream));
    if (n_seqs) HIP_TRY(hipMemcpyAsync(c->wraw.p, weights, n_seqs * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return common_load(c, ptr<uint8_t>(c->raw), ptr<float>(c->wraw), site_map);
}

int wld_load_device(wld_ctx *c, const void *d_sites, size_t n_sites, size_t n_seqs, const uint64_t *site_map,
                    const void *d_weights) {
    WLD_TRY(set_dev(c));
    if ((!d_sites && n_sites * n_seqs) || (!d_weights && n_seqs)) return fail(WLD_E_ARG, "wld_load_device: null input");
    if (n_sites >= (1u << 16) * (size_t)kTile) return fail(WLD_E_ARG, "n_sites %zu too large", n_sites);
    c->loaded = false;
    c->prepass_loaded = false;
    c->L = n_sites;
    c->N = n_seqs;
    return common_load(c, (const uint8_t *)d_sites, (const float *)d_weights, site_map);
}

namespace {
// wld_load_filtered[_device]: site stats on every raw site, kept-site map on
// the host (one byte per site back), Henikoff on the kept sites, then the
// common load of the kept set straight from the raw rows.
int load_filtered(wld_ctx *c, const uint8_t *d_raw, size_t n_sites, size_t n_seqs, const uint64_t *raw_map,
                  float min_acgt, float min_minor, float max_minor, int unweighted, size_t *n_kept) {
    if (n_sites >= (1u << 31)) return fail(WLD_E_ARG, "n_sites %zu too large", n_sites);
    c->loaded = false;
    c->prepass_loaded = false;
    const size_t L0 = n_sites, N = n_seqs;
    // main.rs:139: ceil(min_acgt * n_seqs) in f32, `as usize` saturating at 0 (host.cpp)
    const float cnt = std::ceil(min_acgt * (float)N);
    const uint32_t min_acgt_cnt = cnt <= 0.0f ? 0u : (uint32_t)std::min<double>(cnt, 4294967295.0);
    WLD_TRY(ensure(c->keep, std::max<size_t>(L0, 1)));
    WLD_TRY(ensure(c->htab, std::max<size_t>(L0, 1) * 6 * sizeof(float)));
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    launch_site_stats(d_raw, L0, N, min_acgt_cnt, min_minor, max_minor, ptr<uint8_t>(c->keep), ptr<float>(c->htab),
                      c->stream);
    HIP_TRY(hipGetLastError());
    std::vector<uint8_t> keep(L0);
    if (L0) HIP_TRY(hipMemcpyAsync(keep.data(), c->keep.p, L0, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->kept_map.clear();
    std::vector<uint32_t> idx;
    for (size_t i = 0; i < L0; ++i)
        if (keep[i]) {
            c->kept_map.push_back(raw_map ? raw_map[i] : (uint64_t)i);
            idx.push_back((uint32_t)i);
        }
    const size_t L = idx.size();
    if (L >= (1u << 16) * (size_t)kTile) return fail(WLD_E_ARG, "%zu kept sites: too many", L);
    WLD_TRY(ensure(c->site_index, std::max<size_t>(L, 1) * sizeof(uint32_t)));
    if (L) HIP_TRY(hipMemcpyAsync(c->site_index.p, idx.data(), L * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    WLD_TRY(ensure(c->wraw, std::max<size_t>(N, 1) * sizeof(float)));
    if (unweighted)
        launch_fill_ones(ptr<float>(c->wraw), N, c->stream);
    else {
        WLD_TRY(ensure(c->htab_kept, std::max<size_t>(L, 1) * 6 * sizeof(float)));
        launch_henikoff(d_raw, ptr<uint32_t>(c->site_index), L, N, ptr<float>(c->htab), ptr<float>(c->htab_kept),
                        ptr<float>(c->wraw), c->stream);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(hipEventSynchronize(c->ev[1]));
    const double prepass_ms = event_ms(c->ev[0], c->ev[1]);
    c->L = L;
    c->N = N;
    WLD_TRY(common_load(c, d_raw, ptr<float>(c->wraw), c->kept_map.data(), ptr<uint32_t>(c->site_index)));
    c->stats.load_ms += prepass_ms;
    c->prepass_loaded = true;
    if (n_kept) *n_kept = L;
    return WLD_OK;
}
}  // namespace

int wld_load_filtered(wld_ctx *c, const uint8_t *sites, size_t n_sites, size_t n_seqs, const uint64_t *site_map,
                      float min_acgt, float min_minor, float max_minor, int unweighted, size_t *n_kept) {
    WLD_TRY(set_dev(c));
    if (!sites && n_sites * n_seqs) return fail(WLD_E_ARG, "wld_load_filtered: null input");
    WLD_TRY(ensure(c->raw, std::max<size_t>(n_sites * n_seqs, 1)));
    if (n_sites * n_seqs)
        HIP_TRY(hipMemcpyAsync(c->raw.p, sites, n_sites * n_seqs, hipMemcpyHostToDevice, c->stream));
    return load_filtered(c, ptr<uint8_t>(c->raw), n_sites, n_seqs, site_map, min_acgt, min_minor, max_minor,
                         unweighted, n_kept);
}

int wld_load_filtered_device(wld_ctx *c, const void *d_sites, size_t n_sites, size_t n_seqs,
                             const uint64_t *site_map, float min_acgt, float min_minor, float max_minor,
                             int unweighted, size_t *n_kept) {
    WLD_TRY(set_dev(c));
    if (!d_sites && n_sites * n_seqs) return fail(WLD_E_ARG, "wld_load_filtered_device: null input");
    return load_filtered(c, (const uint8_t *)d_sites, n_sites, n_seqs, site_map, min_acgt, min_minor, max_minor,
                         unweighted, n_kept);
}

int wld_weights_copy(wld_ctx *c, float *out) {
    WLD_TRY(set_dev(c));
    if (!c->prepass_loaded) return fail(WLD_E_STATE, "wld_weights_copy before wld_load_filtered");
    if (!out && c->N) return fail(WLD_E_ARG, "wld_weights_copy: null output");
    if (c->N) HIP_TRY(hipMemcpyAsync(out, c->wraw.p, c->N * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return WLD_OK;
}

int wld_site_map_copy(wld_ctx *c, uint64_t *out) {
    if (!c) return fail(WLD_E_ARG, "null context");
    if (!c->prepass_loaded) return fail(WLD_E_STATE, "wld_site_map_copy before wld_load_filtered");
    if (!out && !c->kept_map.empty()) return fail(WLD_E_ARG, "wld_site_map_copy: null output");
    std::copy(c->kept_map.begin(), c->kept_map.end(), out);
    return WLD_OK;
}

uint32_t wld_chunk_rows(size_t n_sites) { return chunk_rows_of(n_sites); }

int wld_shard_chunk_rows(size_t n_sites, int n_shards, int shard, uint32_t *begin, uint32_t *end) {
    if (n_shards < 1 || shard < 0 || shard >= n_shards || !begin || !end)
        return fail(WLD_E_ARG, "bad shard %d/%d", shard, n_shards);
    const uint32_t n = chunk_rows_of(n_sites);
    const uint64_t total = pairs_in_rows(n_sites, 0, n);
    // boundaries: first chunk row where the cumulative pair count reaches k/n_shards
    auto boundary = [&](int k) -> uint32_t {
        if (k <= 0) return 0;
        if (k >= n_shards) return n;
        const long double target = (long double)total * k / n_shards;
        uint32_t r = 0;
        while (r < n && (long double)pairs_in_rows(n_sites, 0, r + 1) <= target) ++r;
        // pick the closer of r and r+1
        if (r < n) {
            long double lo = (long double)pairs_in_rows(n_sites, 0, r), hi = (long double)pairs_in_rows(n_sites, 0, r + 1);
            if (hi - target < target - lo) ++r;
        }
        return r;
    };
    *begin = boundary(shard);
    *end = boundary(shard + 1);
    if (*end < *begin) *end = *begin;
    return WLD_OK;
}

uint32_t wld_chunks(size_t n_sites) { return chunks_of(n_sites); }

uint64_t wld_pairs_in_chunks(size_t n_sites, uint32_t begin, uint32_t end) {
    return pairs_in_chunks(n_sites, begin, std::min<uint32_t>(end, chunks_of(n_sites)));
}

int wld_shard_chunks(size_t n_sites, int n_shards, int shard, uint32_t *begin, uint32_t *end) {
    if (n_shards < 1 || shard < 0 || shard >= n_shards || !begin || !end)
        return fail(WLD_E_ARG, "bad shard %d/%d", shard, n_shards);
    const uint32_t m = chunks_of(n_sites), n = chunk_rows_of(n_sites);
    std::vector<uint64_t> pre(m + 1, 0);  // pairs in linear chunks [0, i)
    for (uint32_t i = 0; i < m; ++i) {
        uint32_t r, c;
        chunk_of_linear_host(n, i, r, c);
        pre[i + 1] = pre[i] + pairs_in_chunk(n_sites, r, c);
    }
    // boundary j: the linear chunk whose prefix is closest to j/n_shards of the total
    auto boundary = [&](int j) -> uint32_t {
        if (j <= 0) return 0;
        if (j >= n_shards) return m;
        const long double target = (long double)pre[m] * j / n_shards;
        uint32_t i = (uint32_t)(std::upper_bound(pre.begin(), pre.end(), (uint64_t)target) - pre.begin()) - 1;
        if (i < m && (long double)pre[i + 1] - target < target - (long double)pre[i]) ++i;
        return i;
    };
    // shard k takes the k-th range from the END of the linear order, so shards
    // concatenate in descending shard order as with wld_shard_chunk_rows
    *begin = boundary(n_shards - 1 - shard);
    *end = boundary(n_shards - shard);
    if (*end < *begin) *end = *begin;
    return WLD_OK;
}

namespace {
int ensure_outputs(wld_ctx *c, uint64_t rows) {
    rows = std::max<uint64_t>(rows, 1);
    WLD_TRY(ensure(c->out_a, rows * 4));
    WLD_TRY(ensure(c->out_b, rows * 4));
    WLD_TRY(ensure(c->out_d, rows * 4));
    WLD_TRY(ensure(c->out_dp, rows * 4));
    WLD_TRY(ensure(c->out_r2, rows * 4));
    return WLD_OK;
}

int grow_staging(wld_ctx *c, uint64_t cap) {
    cap = std::max<uint64_t>(cap, 1);
    if (c->st_capacity >= cap) return WLD_OK;
    WLD_TRY(ensure(c->st_a, cap * 4));
    WLD_TRY(ensure(c->st_b, cap * 4));
    WLD_TRY(ensure(c->st_d, cap * 4));
    WLD_TRY(ensure(c->st_dp, cap * 4));
    WLD_TRY(ensure(c->st_r2, cap * 4));
    c->st_capacity = cap;
    return WLD_OK;
}

// One pass of a run, enqueued on the context's stream with no host wait:
// run-state init, the pair kernel, then the chunk scan, which leaves
// {staging cursor, row total} in the mapped host counters (and the total in
// the caller's device word, if given).
int enqueue_pass(wld_ctx *c) {
    const RunPending &r = c->pend;
    if (c->times_pending) {  // the last pass's times were never asked for: its events are re-recorded now
        c->times_pending = false;
        c->stats.pair_kernel_ms = c->stats.order_ms = c->stats.screen_ms = -1.0;
    }
    const uint32_t lin_count = r.lin_end - r.lin_begin;
    // The chunk scan of every completed run leaves the cursor and its chunk
    // totals at 0, and every computed tile writes all of its segment counts,
    // so the init kernel runs only after (re)allocation or a failed run.
    if (c->run_dirty) {
        const uint32_t n = chunk_rows_of(c->L);
        launch_run_init(ptr<unsigned long long>(c->counters), ptr<uint32_t>(c->chunk_total), n * (n + 1) / 2,
                        c->stream);
        HIP_TRY(hipGetLastError());
    }
    c->run_dirty = true;  // until run_complete has seen this pass's scan
    // the reference-order layout is built (once per load) before the pass's
    // first event, so its kernel never lands in the pair phase's time
    if (c->opt_ref_sums && c->n_tiles) WLD_TRY(ensure_ref_layout(c));
    const OrderArgs o = order_args(c);
    // counters: {cursor, total, {ticket, work}, candidate set 0, candidate set 1}
    // (kernels.hpp).  The pass appends to set cand_set; its scan reads that
    // set's counts and zeroes the other one, which the next pass then uses —
    // no kernel of this pass can read a count its own scan has reset.
    unsigned long long *cn = ptr<unsigned long long>(c->counters);
    unsigned long long *cur = cn + kCandSet0 + kCandSetWords * c->cand_set;
    unsigned long long *nxt = cn + kCandSet0 + kCandSetWords * (c->cand_set ^ 1);
    ScanArgs sa{ptr<uint32_t>(c->chunk_total), r.lin_begin, lin_count, ptr<uint32_t>(c->chunk_base), cn + 1, cn,
                c->d_hcnt, r.count_out, cn + kCursorSeen, reinterpret_cast<unsigned *>(cur), reinterpret_cast<unsigned *>(nxt),
                reinterpret_cast<unsigned *>(nxt + 1), reinterpret_cast<unsigned *>(cn + 2),
                reinterpret_cast<unsigned *>(cn + kF6Rechecked)};
    c->h_cnt[0] = c->h_cnt[1] = lin_count ? ~0ull : 0ull;
    c->h_cnt[2] = c->h_cnt[3] = c->h_cnt[5] = 0;
    c->h_cnt[4] = 0;  // the guard word
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    c->pass = screen_policy::Plan{};  // (a range without tiles launches nothing: no screen ran)
    // the scan is fused into the launch after a screen for ranges up to 4096
    // chunks (C4: 3,160, ~10 us in one 256-thread workgroup); a larger range
    // (C5: 19,306 chunks, ~70 us fused) gets the 1024-thread scan kernel
    const bool fuse_scan = c->opt_fused_scan && lin_count && lin_count <= 4096;
    bool scan_fused = false;
    if (c->n_tiles)
        WLD_TRY(launch_pairs(c, r.thr, o, nullptr, &c->pass, fuse_scan ? &sa : nullptr, &scan_fused));
    if (lin_count) c->cand_set ^= 1;  // this pass's scan (fused or below) zeroes the other set
    HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    if (lin_count && !scan_fused) {  // else the last workgroup of the pair launch ran it
        sa.ticket = nullptr;
        launch_chunk_scan(sa, c->stream);
        HIP_TRY(hipGetLastError());
    } else if (!lin_count && r.count_out) {
        HIP_TRY(hipMemsetAsync(r.count_out, 0, sizeof(unsigned long long), c->stream));
    }
    // (a scan fused into the pair launch ends with it: ev[3] marks both, one
    // event record fewer per pass)
    c->ev_end = scan_fused ? 3 : 4;
    if (!scan_fused) HIP_TRY(hipEventRecord(c->ev[4], c->stream));
    c->gather_cap = 0;
    if (c->spec_gather && lin_count) {
        // outputs for a quarter more rows than the last run's (the scan's
        // count decides; more than that and run_complete gathers again)
        const uint64_t cap = std::min<uint64_t>(c->st_capacity, c->rows + c->rows / 4 + 4096);
        WLD_TRY(ensure_outputs(c, cap));
        launch_gather(o, ptr<uint32_t>(c->chunk_base), r.lin_begin, lin_count, chunk_rows_of(c->L), (uint32_t)c->L, 0,
                      cn, c->out_a.bytes / 4, c->has_map && !c->prune_run ? ptr<uint32_t>(c->site_map) : nullptr,
                      ptr<uint32_t>(c->out_a), ptr<uint32_t>(c->out_b), ptr<float>(c->out_d), ptr<float>(c->out_dp),
                      ptr<float>(c->out_r2), c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev[5], c->stream));
        c->gather_cap = c->out_a.bytes / 4;
    }
    return WLD_OK;
}

// The fp6 screen's eligibility for this pass, decided from a sample (auto,
// WLD_OPT_SCREEN_FP6 1) instead of a given-up pass: on linkage-structured
// data the fp6 rounding leaves nearly every tile a candidate, and a pass that
// gives up past a sixteenth of them still costs several times a screen
// (DESIGN.md §4.1).  Every stride-th entry of the screen's list (about 1/64
// of it) is screened, counting only; past a sixteenth of the sampled tiles as
// candidates the threshold (and any lower one) goes to the i8 screen, else it
// (and any higher one) stays on fp6 with no further sample.  Small lists
// (fewer than 2,048 tiles) take the pass itself as the test, as before.
// Only where the pass would screen on fp6 (screen_policy::wants_sample).  On
// the context's own stream when the caller lent it one and the fp6 operands
// were built before this run (the probe reads only them), so the read-back
// does not wait for the caller's earlier work on the borrowed stream (ADVICE
// r5).
int fp6_sample(wld_ctx *c, float thr, bool operands_fresh) {
    const PolicyInputs in = policy_inputs(c, thr, false);
    if (!screen_policy::wants_sample(in.opt, in.load, in.pass, c->learned)) return WLD_OK;
    const hipStream_t s = !operands_fresh && c->own_stream ? c->own_stream : c->stream;
    WLD_TRY(ensure(c->fp6_probe_buf, 4 * sizeof(unsigned)));
    MfmaLaunch m = mfma_base(c, thr);
    // on three sums where the pass might be (the same candidate counts: the
    // fourth sum is formed wherever a verdict needs it), so that the sample
    // also tells how often the second pass runs
    m.fp6_three = c->opt_fp6_three != 0 && m.f6_pairs != nullptr;
    // ... and with the quick test where the pass might be, to count the row
    // blocks that fall through it
    m.fp6_quick = m.fp6_three && c->opt_fp6_quick != 0;
    const uint32_t entries = m.f6_pairs ? m.f6_n_pairs : m.n_tiles;
    const uint32_t stride = std::max<uint32_t>(1, std::min<uint32_t>(64, entries / 256));
    launch_fp6_probe(m, ptr<unsigned>(c->fp6_probe_buf), stride, s);
    HIP_TRY(hipGetLastError());
    unsigned h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, c->fp6_probe_buf.p, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->fp6_sampled = true;
    screen_policy::learn(c->learned, screen_policy::Sample{thr, h[0], h[1], m.fp6_three, h[2], m.fp6_quick, h[3]});
    return WLD_OK;
}

// Phase 1 of a run over linear chunks [lin_begin, lin_end): sizing, then the
// first pass, enqueued.  Staging starts at min(pairs, 32M rows); the pair
// kernels count every passing row but store only below capacity, so an
// overflow is detected from the cursor in run_complete and the pass re-run
// once with staging of the exact size.
int run_enqueue(wld_ctx *c, float thr, uint32_t lin_begin, uint32_t lin_end, unsigned long long *count_out) {
    const uint32_t n = chunk_rows_of(c->L);
    c->have_rows = false;
    c->pend.active = false;
    const bool fp6_fresh = !c->fp6_tried && c->opt_fp6 != 0;
    if (fp6_fresh) WLD_TRY(fp6_prepare(c));
    WLD_TRY(build_tiles(c, lin_begin, lin_end, true));
    c->fp6_sampled = false;
    WLD_TRY(fp6_sample(c, thr, fp6_fresh));
    const uint64_t pairs = run_pairs(c, lin_begin, lin_end);  // (in-window pairs under a window)
    const uint32_t T = (uint32_t)(c->LP / kTile);
    const uint32_t n_chunks = n * (n + 1) / 2;
    if (pairs > 0xFFFFFFFFull)
        return fail(WLD_E_ARG, "shard has %llu pairs; > 2^32 per device not supported (shard over more devices)",
                    (unsigned long long)pairs);
    WLD_TRY(grow_staging(c, std::min<uint64_t>(pairs, c->opt_staging_rows)));
    WLD_TRY(ensure(c->seg_cnt, c->LP * T));
    WLD_TRY(ensure(c->seg_off, c->LP * T * sizeof(uint32_t)));
    if (c->seg_clear) {  // a windowed list since the last clear: its unlisted tiles read as zero
        HIP_TRY(hipMemsetAsync(c->seg_cnt.p, 0, c->LP * T, c->stream));
        c->seg_clear = false;
    }
    const size_t ct_bytes = c->chunk_total.bytes, cn_bytes = c->counters.bytes;
    WLD_TRY(ensure(c->chunk_total, std::max<size_t>(n_chunks, 1) * sizeof(uint32_t)));
    WLD_TRY(ensure(c->chunk_base, std::max<size_t>(n_chunks, 1) * sizeof(uint32_t)));
    WLD_TRY(ensure(c->counters, kCounterWords * sizeof(unsigned long long)));
    if (c->chunk_total.bytes != ct_bytes || c->counters.bytes != cn_bytes) c->run_dirty = true;  // fresh memory
    c->pend = RunPending{true, thr, lin_begin, lin_end, pairs, count_out};
    c->prog_pass = false;
    if (c->on_chunk && lin_end > lin_begin) {
        // per-chunk progress: countdowns of the range's chunks, an empty log
        const uint32_t cnt = lin_end - lin_begin;
        WLD_TRY(ensure(c->chunk_left, std::max<size_t>(n_chunks, 1) * sizeof(unsigned)));
        WLD_TRY(ensure(c->prog_n, sizeof(unsigned)));
        if (c->plog_cap < cnt) {
            if (c->h_plog) (void)hipHostFree(c->h_plog);
            c->h_plog = c->d_plog = nullptr;
            c->plog_cap = 0;
            HIP_TRY(hipHostMalloc((void **)&c->h_plog, (size_t)cnt * sizeof(unsigned long long),
                                  hipHostMallocMapped | hipHostMallocCoherent));
            HIP_TRY(hipHostGetDevicePointer((void **)&c->d_plog, c->h_plog, 0));
            c->plog_cap = cnt;
        }
        memset(c->h_plog, 0xFF, (size_t)cnt * sizeof(unsigned long long));
        if (c->tiles_windowed) {
            launch_progress_init_window(ptr<unsigned>(c->chunk_left), lin_begin, cnt, n, ptr<uint32_t>(c->tiles),
                                        c->n_tiles, ptr<unsigned>(c->prog_n), c->stream);
            c->prog_expect = c->win_live_pre[lin_end] - c->win_live_pre[lin_begin];
        } else {
            launch_progress_init(ptr<unsigned>(c->chunk_left), lin_begin, cnt, n, (uint32_t)c->L,
                                 ptr<unsigned>(c->prog_n), c->stream);
            c->prog_expect = cnt;
        }
        HIP_TRY(hipGetLastError());
        c->prog_pass = true;
    }
    return enqueue_pass(c);
}

// The progress log of a pass with per-chunk progress: every chunk pair count
// logged so far, in slot order, to on_chunk (on the calling thread), polled
// while the pass runs; then the rest once it has completed.  Progress is a
// report, not a result: entries still missing once the pass has completed
// are reported from the chunk pair counts the host knows rather than failing
// the run, and counted in wld_run_stats.progress_filled — a pass that
// completes logs every chunk (a refused tile fails the run at check_guard),
// so a nonzero count is a lost tile_done count, which the tests look for.
int drain_progress(wld_ctx *c, uint32_t n_chunks) {
    uint32_t seen = 0;
    auto drain = [&] {
        while (seen < n_chunks) {
            const unsigned long long v = __atomic_load_n(&c->h_plog[seen], __ATOMIC_ACQUIRE);
            if (v == ~0ull) break;
            (*c->on_chunk)(v);
            ++seen;
        }
    };
    for (;;) {
        const hipError_t q = hipEventQuery(c->ev[c->ev_end]);  // the pass's end (the stream may hold later work)
        drain();
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) HIP_TRY(q);
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
    // the pass has completed: every chunk's entry is written (system-scope
    // stores); allow the last ones a moment to land
    for (int spin = 0; seen < n_chunks && spin < 100000; ++spin) drain();
    if (seen < n_chunks) {
        // the logged chunks' pairs, then the pairs of the chunks whose entries
        // did not arrive, one report each (the sum is the range's pairs)
        uint64_t logged = 0;
        for (uint32_t k = 0; k < seen; ++k) logged += c->h_plog[k];
        const uint64_t all = c->pend.pairs;  // the run's pairs (in-window ones under a window)
        uint64_t rest = all - std::min<uint64_t>(logged, all);
        const uint32_t missing = n_chunks - seen;
        c->stats.progress_filled += missing;
        for (uint32_t k = 0; k < missing; ++k) {
            const uint64_t v = rest / (missing - k);
            (*c->on_chunk)(v);
            rest -= v;
        }
    }
    return WLD_OK;
}

// The kernels' guard word (OrderArgs::guard) after a completed phase: nonzero
// when a kernel refused an out-of-range index (a candidate entry or tile, a
// staged pair, a gather destination) instead of reading or writing through
// it.  The run is then wrong, not just slow: WLD_E_STATE, and the next run
// starts from re-initialised run state.
int check_guard(wld_ctx *c, const char *phase) {
    const unsigned g = (unsigned)__atomic_load_n(&c->h_cnt[4], __ATOMIC_ACQUIRE);
    if (!g) return WLD_OK;
    c->run_dirty = true;
    c->have_rows = false;
    return fail(WLD_E_STATE, "internal: the %s refused an out-of-range index (guard 0x%x: %s%s%s%s%s); no rows", phase,
                g, g & kGuardEntry ? "candidate entry " : "", g & kGuardTile ? "tile " : "",
                g & kGuardPair ? "staged pair " : "", g & kGuardSlice ? "candidate slice " : "",
                g & kGuardGather ? "gather destination" : "");
}

// Phase 2: one host wait, the overflow re-run if needed, then (only when rows
// passed) the reference-order gather.
int run_complete(wld_ctx *c, uint64_t *n_rows) {
    if (!c->pend.active) return fail(WLD_E_STATE, "no run in flight");
    c->pend.active = false;
    const RunPending r = c->pend;
    const uint32_t n = chunk_rows_of(c->L);
    const uint32_t lin_count = r.lin_end - r.lin_begin;
    unsigned long long h[4] = {0, 0, 0, 0};
    bool regrown = false, abandoned = false;
    for (;;) {
        if (c->prog_pass) {
            c->prog_pass = false;  // a re-run after a staging overflow does not report again
            WLD_TRY(drain_progress(c, c->prog_expect));
        }
        // the pass's end, not the stream's: on a shared stream (wld_set_stream)
        // the next context's run may already be queued behind it
        HIP_TRY(hipEventSynchronize(c->ev[c->gather_cap ? 5 : c->ev_end]));
        WLD_TRY(check_guard(c, c->gather_cap ? "pair phase or reference-order gather" : "pair phase"));
        c->run_dirty = false;  // the pass completed: its scan cleaned the run state
        h[0] = __atomic_load_n(&c->h_cnt[0], __ATOMIC_ACQUIRE);
        h[1] = __atomic_load_n(&c->h_cnt[1], __ATOMIC_ACQUIRE);
        h[2] = __atomic_load_n(&c->h_cnt[2], __ATOMIC_ACQUIRE);
        h[3] = __atomic_load_n(&c->h_cnt[3], __ATOMIC_ACQUIRE);
        if (h[2] & kAbandonBit) {
            // the fp6 screen gave the pass up: this threshold (and any lower
            // one) screens on i8 from now on, this pass included
            if (abandoned) return fail(WLD_E_HIP, "internal: a re-run pass was abandoned again");
            abandoned = true;
            screen_policy::learn(c->learned,
                                 screen_policy::Outcome{c->pass.route, r.thr, true, 0, c->n_tiles, 0, r.pairs});
            WLD_TRY(enqueue_pass(c));
            continue;
        }
        if (h[0] <= c->st_capacity) break;
        if (regrown) return fail(WLD_E_HIP, "internal: staging overflow after resize");
        regrown = true;
        WLD_TRY(grow_staging(c, h[0]));
        WLD_TRY(enqueue_pass(c));
    }
    const uint64_t rows = h[1];
    // (exact candidate pairs: the cursor counts the candidates staged, the
    // chunk totals the rows kept)
    const screen_policy::Route route = c->pass.route;
    const bool screened = screen_policy::ran_screen(route), cand_pairs = route == screen_policy::Route::CandidatePairs;
    if (cand_pairs ? h[0] < h[1] : h[0] != h[1])
        return fail(WLD_E_HIP, "internal: staging cursor %llu vs chunk total %llu", h[0], h[1]);
    int order_end = c->gather_cap ? 5 : c->ev_end;  // with no rows (and no gather enqueued) it ends at the scan
    if (rows && lin_count && rows > c->gather_cap) {  // not gathered behind the scan
        WLD_TRY(ensure_outputs(c, rows));
        launch_gather(order_args(c), ptr<uint32_t>(c->chunk_base), r.lin_begin, lin_count, n, (uint32_t)c->L, rows,
                      nullptr, rows, c->has_map && !c->prune_run ? ptr<uint32_t>(c->site_map) : nullptr, ptr<uint32_t>(c->out_a),
                      ptr<uint32_t>(c->out_b), ptr<float>(c->out_d), ptr<float>(c->out_dp), ptr<float>(c->out_r2),
                      c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev[5], c->stream));
        HIP_TRY(hipEventSynchronize(c->ev[5]));
        WLD_TRY(check_guard(c, "reference-order gather"));
        order_end = 5;
    }
    c->rows = rows;
    c->have_rows = true;
    c->spec_gather = rows > 0;
    c->gather_cap = 0;
    c->stats.kernel = c->kernel;
    c->stats.pairs = r.pairs;
    c->stats.rows = rows;
    c->times_pending = true;  // (pair_kernel_ms, order_ms, screen_ms: materialize_times)
    c->times_order_end = order_end;
    c->stats.pair_kernel_launches = c->n_tiles ? screen_policy::stat_launches(route) : 0;
    // (under a window: the tiles holding an in-window pair, without the launch order's padding)
    c->stats.tiles = c->tiles_windowed ? c->n_tiles_listed : c->n_tiles;
    c->stats.screened = screen_policy::stat_screened(route);
    c->stats.screen_fp6 = screen_policy::stat_screen_fp6(route) ? 1 : abandoned ? 2 : 0;
    c->stats.fp6_sampled = c->fp6_sampled ? 1 : 0;
    c->stats.fp6_a4 = c->stats.screen_fp6 == 1 && c->f6.a4 ? 1 : 0;
    c->stats.fp6_shared = c->stats.screen_fp6 == 1 && c->f6.shared ? 1 : 0;
    c->stats.fp6_three = c->stats.screen_fp6 == 1 ? screen_policy::stat_fp6_three(c->pass) : 0;
    // (h_cnt[5]: the entries rechecked, and above them the quick test's row blocks)
    const unsigned long long f6_counts = __atomic_load_n(&c->h_cnt[5], __ATOMIC_ACQUIRE);
    c->stats.fp6_rechecked = c->stats.fp6_three ? (f6_counts & 0xFFFFFFFFull) : 0;
    c->stats.fp6_quick = c->stats.screen_fp6 == 1 ? screen_policy::stat_fp6_quick(c->pass) : 0;
    c->stats.fp6_quick_full = c->stats.fp6_quick ? (f6_counts >> 32) : 0;
    c->stats.candidate_pairs = cand_pairs ? h[0] : 0;
    // auto: what this pass's counts teach the policy (screen_policy.hpp: the break-evens)
    screen_policy::learn(c->learned, screen_policy::Outcome{route, r.thr, false, h[2], c->n_tiles, h[0], r.pairs});
    c->stats.candidate_tiles = screened ? h[2] : c->n_tiles;
    c->stats.candidate_blocks = screened && !cand_pairs ? h[3] : 16 * (uint64_t)c->n_tiles;
    if (n_rows) *n_rows = rows;
    return WLD_OK;
}

int run_chunks(wld_ctx *c, float thr, uint32_t lin_begin, uint32_t lin_end, uint64_t *n_rows) {
    WLD_TRY(run_enqueue(c, thr, lin_begin, lin_end, nullptr));
    return run_complete(c, n_rows);
}
}  // namespace

int wld_run(wld_ctx *c, float thr, uint32_t rb, uint32_t re, uint64_t *n_rows) {
    WLD_TRY(set_dev(c));
    if (!c->loaded) return fail(WLD_E_STATE, "wld_run before wld_load");
    const uint32_t n = chunk_rows_of(c->L);
    if (re == 0 || re > n) re = n;
    if (rb > re) return fail(WLD_E_ARG, "row range [%u,%u) invalid", rb, re);
    uint32_t lb, le;
    rows_to_linear(n, rb, re, lb, le);
    return run_chunks(c, thr, lb, le, n_rows);
}

int wld_run_chunks(wld_ctx *c, float thr, uint32_t chunk_begin, uint32_t chunk_end, uint64_t *n_rows) {
    WLD_TRY(set_dev(c));
    if (!c->loaded) return fail(WLD_E_STATE, "wld_run_chunks before wld_load");
    const uint32_t m = chunks_of(c->L);
    if (chunk_end == 0 || chunk_end > m) chunk_end = m;
    if (chunk_begin > chunk_end) return fail(WLD_E_ARG, "chunk range [%u,%u) invalid", chunk_begin, chunk_end);
    return run_chunks(c, thr, chunk_begin, chunk_end, n_rows);
}

int wld_run_chunks_async(wld_ctx *c, float thr, uint32_t chunk_begin, uint32_t chunk_end, void *d_count_out) {
    WLD_TRY(set_dev(c));
    if (!c->loaded) return fail(WLD_E_STATE, "wld_run_chunks_async before wld_load");
    const uint32_t m = chunks_of(c->L);
    if (chunk_end == 0 || chunk_end > m) chunk_end = m;
    if (chunk_begin > chunk_end) return fail(WLD_E_ARG, "chunk range [%u,%u) invalid", chunk_begin, chunk_end);
    return run_enqueue(c, thr, chunk_begin, chunk_end, static_cast<unsigned long long *>(d_count_out));
}

int wld_run_wait(wld_ctx *c, uint64_t *n_rows) {
    WLD_TRY(set_dev(c));
    return run_complete(c, n_rows);
}

int wld_run_after(wld_ctx *c, wld_ctx *prev) {
    if (!c || !prev) return fail(WLD_E_ARG, "null context");
    if (!c->members.empty() || !prev->members.empty()) return fail(WLD_E_ARG, "wld_run_after on a device group");
    if (c->pend.active) return fail(WLD_E_STATE, "wld_run_after during a run of ctx");
    if (!prev->pend.active) return WLD_OK;  // nothing in flight
    WLD_TRY(set_dev(c));
    // ev[6] separates a screened pass's screen from its candidate launch;
    // ev[3] follows the pair kernel(s) (enqueue_pass)
    if (c->stream == prev->stream) return WLD_OK;  // one stream: already in order
    const bool screened = screen_policy::ran_screen(prev->pass.route);
    HIP_TRY(hipStreamWaitEvent(c->stream, screened ? prev->ev[6] : prev->ev[3], 0));
    return WLD_OK;
}

int wld_set_stream(wld_ctx *c, void *stream) {
    if (!c) return fail(WLD_E_ARG, "null context");
    if (!c->members.empty()) return fail(WLD_E_ARG, "wld_set_stream on a device group");
    if (c->pend.active) return fail(WLD_E_STATE, "wld_set_stream during a run");
    WLD_TRY(set_dev(c));
    HIP_TRY(hipStreamSynchronize(c->stream));  // work already queued completes first
    c->stream = stream ? static_cast<hipStream_t>(stream) : c->own_stream;
    return WLD_OK;
}

void *wld_stream(wld_ctx *c) { return c ? (void *)c->stream : nullptr; }

int wld_rows_device(wld_ctx *c, wld_pairs *v) {
    if (!c || !v) return fail(WLD_E_ARG, "null argument");
    if (!c->have_rows) return fail(WLD_E_STATE, "no rows: call wld_run first");
    v->n = c->rows;
    v->site_a = ptr<uint32_t>(c->out_a);
    v->site_b = ptr<uint32_t>(c->out_b);
    v->d = ptr<float>(c->out_d);
    v->d_prime = ptr<float>(c->out_dp);
    v->r2 = ptr<float>(c->out_r2);
    return WLD_OK;
}

int wld_rows_copy(wld_ctx *c, uint32_t *site_a, uint32_t *site_b, float *d, float *d_prime, float *r2) {
    WLD_TRY(set_dev(c));
    if (!c->have_rows) return fail(WLD_E_STATE, "no rows: call wld_run first");
    const size_t n = c->rows;
    if (n) {
        if (site_a) HIP_TRY(hipMemcpyAsync(site_a, c->out_a.p, n * 4, hipMemcpyDeviceToHost, c->stream));
        if (site_b) HIP_TRY(hipMemcpyAsync(site_b, c->out_b.p, n * 4, hipMemcpyDeviceToHost, c->stream));
        if (d) HIP_TRY(hipMemcpyAsync(d, c->out_d.p, n * 4, hipMemcpyDeviceToHost, c->stream));
        if (d_prime) HIP_TRY(hipMemcpyAsync(d_prime, c->out_dp.p, n * 4, hipMemcpyDeviceToHost, c->stream));
        if (r2) HIP_TRY(hipMemcpyAsync(r2, c->out_r2.p, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return WLD_OK;
}

int wld_rows_copy_device(wld_ctx *c, void *site_a, void *site_b, void *d, void *d_prime, void *r2) {
    WLD_TRY(set_dev(c));
    if (!c->have_rows) return fail(WLD_E_STATE, "no rows: call wld_run first");
    const size_t n = c->rows;
    if (n) {
        if (site_a) HIP_TRY(hipMemcpyAsync(site_a, c->out_a.p, n * 4, hipMemcpyDeviceToDevice, c->stream));
        if (site_b) HIP_TRY(hipMemcpyAsync(site_b, c->out_b.p, n * 4, hipMemcpyDeviceToDevice, c->stream));
        if (d) HIP_TRY(hipMemcpyAsync(d, c->out_d.p, n * 4, hipMemcpyDeviceToDevice, c->stream));
        if (d_prime) HIP_TRY(hipMemcpyAsync(d_prime, c->out_dp.p, n * 4, hipMemcpyDeviceToDevice, c->stream));
        if (r2) HIP_TRY(hipMemcpyAsync(r2, c->out_r2.p, n * 4, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return WLD_OK;
}

int wld_dense(wld_ctx *c, float *d, float *d_prime, float *r2, uint8_t *valid) {
    WLD_TRY(set_dev(c));
    if (!c->loaded) return fail(WLD_E_STATE, "wld_dense before wld_load");
    if (!d || !d_prime || !r2 || !valid) return fail(WLD_E_ARG, "wld_dense: null output");
    const size_t L = c->L, LL = L * L;
    if (LL == 0) return WLD_OK;
    if (L > 8192) return fail(WLD_E_ARG, "wld_dense is for tests (n_sites <= 8192)");
    WLD_TRY(build_tiles(c, 0, chunks_of(L), false));  // every tile: wld_dense ignores the window
    DevBuf dd, ddp, dr2, dv;
    int st = WLD_OK;
    if ((st = ensure(dd, LL * 4)) || (st = ensure(ddp, LL * 4)) || (st = ensure(dr2, LL * 4)) || (st = ensure(dv, LL))) {
        release(dd); release(ddp); release(dr2); release(dv);
        return st;
    }
    DenseArgs da{ptr<float>(dd), ptr<float>(ddp), ptr<float>(dr2), ptr<uint8_t>(dv)};
    (void)hipMemsetAsync(dv.p, 0, LL, c->stream);
    OrderArgs o = order_args(c);
    st = launch_pairs(c, 0.0f, o, &da);
    if (st == WLD_OK) {
        hipError_t e = hipSuccess;
        if (e == hipSuccess) e = hipMemcpyAsync(d, dd.p, LL * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_prime, ddp.p, LL * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(r2, dr2.p, LL * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(valid, dv.p, LL, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) st = fail(WLD_E_HIP, "wld_dense copy: %s", hipGetErrorString(e));
    }
    release(dd); release(ddp); release(dr2); release(dv);
    return st;
}

int wld_last_stats(wld_ctx *c, wld_run_stats *out) {
    if (!c || !out) return fail(WLD_E_ARG, "null argument");
    if (c->members.empty()) {
        (void)hipSetDevice(c->device);
        materialize_times(c);
    }
    *out = c->stats;
    return WLD_OK;
}

void wld_pairs_free(wld_pairs *p) {
    if (!p) return;
    free(p->site_a);
    free(p->site_b);
    free(p->d);
    free(p->d_prime);
    free(p->r2);
    memset(p, 0, sizeof(*p));
}

namespace {
// The chunks [lb, le) of the loaded set, rows to host: batches of whole
// chunks, contiguous in the reference order, of at most opt_host_batch_pairs
// (2^31) pairs each (a run's staging positions are 32-bit); their rows
// concatenate in order.  on_chunk (may be null) gets each chunk's pair count
// as the chunk completes, on the calling thread.
int run_host_range(wld_ctx *c, float r2_threshold, uint32_t lb, uint32_t le,
                   const std::function<void(uint64_t)> *on_chunk, wld_pairs *out) {
    memset(out, 0, sizeof(*out));
    WLD_TRY(set_dev(c));
    if (!c->loaded) return fail(WLD_E_STATE, "wld_run_host before wld_load");
    c->stats.progress_filled = 0;
    const uint64_t limit = std::max<uint64_t>(1, c->opt_host_batch_pairs);
    uint64_t cap = 0, done = 0, pairs_done = 0;
    auto grow = [&](uint64_t need) -> int {
        if (need <= cap) return WLD_OK;
        uint64_t k = std::max<uint64_t>(need, cap + cap / 2);
        void *p[5] = {realloc(out->site_a, k * 4), nullptr, nullptr, nullptr, nullptr};
        if (p[0]) out->site_a = (uint32_t *)p[0];
        if (p[0] && (p[1] = realloc(out->site_b, k * 4))) out->site_b = (uint32_t *)p[1];
        if (p[1] && (p[2] = realloc(out->d, k * 4))) out->d = (float *)p[2];
        if (p[2] && (p[3] = realloc(out->d_prime, k * 4))) out->d_prime = (float *)p[3];
        if (p[3] && (p[4] = realloc(out->r2, k * 4))) out->r2 = (float *)p[4];
        if (!p[4]) return fail(WLD_E_OOM, "host allocation of %llu rows failed", (unsigned long long)k);
        cap = k;
        return WLD_OK;
    };
    int st = grow(1);
    for (uint32_t b = lb; st == WLD_OK && b < le;) {
        uint32_t e = b;
        uint64_t pairs = 0;
        while (e < le) {
            const uint64_t p1 = run_pairs(c, e, e + 1);  // (in-window pairs under a window)
            if (e > b && pairs + p1 > limit) break;
            pairs += p1;
            ++e;
        }
        uint64_t rows = 0;
        c->on_chunk = on_chunk;
        st = run_chunks(c, r2_threshold, b, e, &rows);
        c->on_chunk = nullptr;
        if (st != WLD_OK) break;
        if ((st = grow(done + rows)) != WLD_OK) break;
        if (rows &&
            (st = wld_rows_copy(c, out->site_a + done, out->site_b + done, out->d + done, out->d_prime + done,
                                out->r2 + done)) != WLD_OK)
            break;
        done += rows;
        pairs_done += pairs;
        b = e;
    }
    if (st != WLD_OK) {
        wld_pairs_free(out);
        return st;
    }
    out->n = done;
    c->stats.pairs = pairs_done;
    c->stats.rows = done;
    return WLD_OK;
}

// wld_run_host on a device group: member k runs shard k of the reference's
// chunk sequence (wld_shard_chunks: contiguous, balanced by pair count) on
// its own host thread (each run blocks on its device); the members' chunk
// completions queue up for the calling thread, which reports them (on_chunk)
// and concatenates the shards' rows in DESCENDING shard order (shard 0 holds
// the last chunks).
int run_host_group(wld_ctx *g, float thr, const std::function<void(uint64_t)> *on_chunk, wld_pairs *out) {
    const int G = (int)g->members.size();
    const size_t L = g->members[0]->L;
    std::vector<wld_pairs> part(G);
    std::vector<int> status(G, WLD_OK);
    std::vector<std::string> msg(G);
    std::vector<uint64_t> pairs(G, 0);
    std::mutex mu;
    std::condition_variable cv;
    std::vector<int> finished;
    // every shard's range before any thread starts: an early return must not
    // leave a joinable std::thread behind (std::terminate)
    std::vector<uint32_t> lb(G), le(G);
    // (under a window: the partition balanced by in-window pairs, and their counts)
    const bool win = window_on(g->members[0]);
    for (int k = 0; k < G; ++k) {
        if (win) WLD_TRY(wld_shard_chunks_window(g->members[0], G, k, &lb[k], &le[k]));
        else WLD_TRY(wld_shard_chunks(L, G, k, &lb[k], &le[k]));
        pairs[k] = run_pairs(g->members[0], lb[k], le[k]);
    }
    std::deque<uint64_t> events;  // chunk pair counts from the members, in completion order
    const std::function<void(uint64_t)> push = [&](uint64_t p) {
        std::lock_guard<std::mutex> lk(mu);
        events.push_back(p);
        cv.notify_one();
    };
    std::vector<std::thread> th;
    for (int k = 0; k < G; ++k) {
        th.emplace_back([&, k] {
            const int st = run_host_range(g->members[k], thr, lb[k], le[k], on_chunk ? &push : nullptr, &part[k]);
            std::lock_guard<std::mutex> lk(mu);
            status[k] = st;
            if (st != WLD_OK) msg[k] = wld_last_error();
            finished.push_back(k);
            cv.notify_one();
        });
    }
    uint64_t pairs_done = 0;
    for (;;) {  // progress on the calling thread, chunk by chunk
        std::deque<uint64_t> batch;
        bool all_done;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !events.empty() || (int)finished.size() == G; });
            batch.swap(events);
            all_done = (int)finished.size() == G;
        }
        for (uint64_t p : batch) (*on_chunk)(p);
        if (all_done) {
            std::lock_guard<std::mutex> lk(mu);
            if (events.empty()) break;
        }
    }
    for (auto &t : th) t.join();
    for (int k = 0; k < G; ++k) pairs_done += pairs[k];
    int st = WLD_OK;
    for (int k = 0; k < G; ++k)
        if (status[k] != WLD_OK && st == WLD_OK) st = fail(status[k], "device %d (shard %d): %s", g->members[k]->device, k, msg[k].c_str());
    uint64_t total = 0;
    for (auto &p : part) total += p.n;
    if (st == WLD_OK) {
        const uint64_t n = std::max<uint64_t>(total, 1);
        out->site_a = (uint32_t *)malloc(n * 4);
        out->site_b = (uint32_t *)malloc(n * 4);
        out->d = (float *)malloc(n * 4);
        out->d_prime = (float *)malloc(n * 4);
        out->r2 = (float *)malloc(n * 4);
        if (!out->site_a || !out->site_b || !out->d || !out->d_prime || !out->r2)
            st = fail(WLD_E_OOM, "host allocation of %llu rows failed", (unsigned long long)total);
    }
    if (st == WLD_OK) {
        uint64_t at = 0;
        for (int k = G - 1; k >= 0; --k) {
            const wld_pairs &p = part[k];
            memcpy(out->site_a + at, p.site_a, p.n * 4);
            memcpy(out->site_b + at, p.site_b, p.n * 4);
            memcpy(out->d + at, p.d, p.n * 4);
            memcpy(out->d_prime + at, p.d_prime, p.n * 4);
            memcpy(out->r2 + at, p.r2, p.n * 4);
            at += p.n;
        }
        out->n = total;
    } else {
        wld_pairs_free(out);
    }
    for (auto &p : part) wld_pairs_free(&p);
    for (wld_ctx *m : g->members) {
        (void)hipSetDevice(m->device);
        materialize_times(m);
    }
    g->stats = g->members[0]->stats;
    g->stats.progress_filled = 0;
    for (wld_ctx *m : g->members) g->stats.progress_filled += m->stats.progress_filled;
    g->stats.pairs = pairs_done;
    g->stats.rows = st == WLD_OK ? total : 0;
    double kms = 0.0;
    for (wld_ctx *m : g->members) kms = std::max(kms, m->stats.pair_kernel_ms);
    g->stats.pair_kernel_ms = kms;  // the slowest device's last batch
    return st;
}

}  // namespace

int wld_run_host(wld_ctx *c, float r2_threshold, wld_progress_fn progress, void *user, wld_pairs *out) {
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    if (!c) return fail(WLD_E_ARG, "null context");
    // lib.rs:670-674: per chunk, the running count of pairs in the chunks
    // completed BEFORE it (fetch_add's previous value)
    uint64_t before = 0;
    const std::function<void(uint64_t)> on_chunk = [&](uint64_t p) {
        progress(before, user);
        before += p;
    };
    const std::function<void(uint64_t)> *oc = progress ? &on_chunk : nullptr;
    if (!c->members.empty()) {
        for (wld_ctx *m : c->members)
            if (!m->loaded) return fail(WLD_E_STATE, "wld_run_host before wld_load");
        return run_host_group(c, r2_threshold, oc, out);
    }
    return run_host_range(c, r2_threshold, 0, chunks_of(c->L), oc, out);
}

namespace {
// What wld_run_summary refuses, checked on a loaded single-device context
// (every member of a group holds the same load).
int summary_check(wld_ctx *c, uint64_t bin_width, uint32_t n_bins) {
    if (n_bins > summary_plan::kMaxBins)
        return fail(WLD_E_ARG, "wld_run_summary: n_bins %u exceeds %u", n_bins, summary_plan::kMaxBins);
    if (bin_width && !n_bins) return fail(WLD_E_ARG, "wld_run_summary: bin_width %llu with n_bins 0",
                                          (unsigned long long)bin_width);
    if (c->safe)
        return fail(WLD_E_ARG, "wld_run_summary needs finite weights (this load takes the select loop)");
    if (bin_width && c->has_pos) {  // (the rule of a distance window: window_prepare)
        const uint32_t *pos = c->pos_host.data();
        const uint32_t i = window_plan::first_descent(pos, (uint32_t)c->L);
        if (i < c->L)
            return fail(WLD_E_ARG, "decay bins (bin_width %llu) need a non-decreasing site_map: "
                                   "site_map[%u] = %u < site_map[%u] = %u",
                        (unsigned long long)bin_width, i, pos[i], i - 1, pos[i - 1]);
    }
    return WLD_OK;
}

// The summary of the linear chunks [lb, le) on one device: the tile list of
// the range under the window (build_tiles: the row path's cached list when it
// covers the same range, else rebuilt — a windowed rebuild leaves seg_clear
// set for the next row run), zeroed accumulators, one launch,
// one copy back.  Touches no staging, segment count, chunk total, run counter
// or row-path event.
int summary_range(wld_ctx *c, uint32_t lb, uint32_t le, uint64_t bin_width, uint32_t n_bins,
                  summary_plan::Summary *out) {
    WLD_TRY(set_dev(c));
    if (!c->loaded) return fail(WLD_E_STATE, "wld_run_summary before wld_load");
    if (c->pend.active) return fail(WLD_E_STATE, "wld_run_summary during a run");
    WLD_TRY(summary_check(c, bin_width, n_bins));
    const size_t L = c->L, LP = c->LP, nb = bin_width ? n_bins : 0;
    *out = summary_plan::Summary{};
    out->score.assign(L, 0.0);
    out->partners.assign(L, 0);
    out->bin_pairs.assign(nb, 0);
    out->bin_r2_sum.assign(nb, 0.0);
    if (lb >= le) return WLD_OK;
    WLD_TRY(ensure_ref_layout(c));
    WLD_TRY(build_tiles(c, lb, le, true));
    if (!c->n_tiles) return WLD_OK;  // (a window without a pair in the range)
    for (auto &e : c->ev_sum)
        if (!e) HIP_TRY(hipEventCreate(&e));
    // {r2_sum, score[LP], bin_r2_sum[nb]} f64 | {counts[4], bin_pairs[nb]} u64 | partners[LP] u32
    const size_t n_f64 = 1 + LP + nb, n_u64 = 4 + nb, bytes = 8 * (n_f64 + n_u64) + 4 * LP;
    WLD_TRY(ensure(c->sum_buf, bytes));
    double *d_f64 = ptr<double>(c->sum_buf);
    unsigned long long *d_u64 = reinterpret_cast<unsigned long long *>(d_f64 + n_f64);
    uint32_t *d_u32 = reinterpret_cast<uint32_t *>(d_u64 + n_u64);
    HIP_TRY(hipMemsetAsync(c->sum_buf.p, 0, bytes, c->stream));
    const SummaryArgs sa{d_u64, d_f64, d_f64 + 1, d_u32, nb ? d_u64 + 4 : nullptr, nb ? d_f64 + 1 + LP : nullptr,
                         c->has_pos ? ptr<uint32_t>(c->site_map) : nullptr, bin_width, (uint32_t)nb};
    const ValuLaunch v = ref_valu_launch(c, 0.0f);  // (finite weights: summary_check)
    OrderArgs o{};  // the window only
    o.L = (uint32_t)L;
    o.T = (uint32_t)(LP / kTile);
    o.win_hi = c->tiles_windowed ? ptr<uint32_t>(c->win_hi) : nullptr;
    HIP_TRY(hipEventRecord(c->ev_sum[0], c->stream));
    launch_pair_summary(v, o, sa, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_sum[1], c->stream));
    std::vector<unsigned char> h(bytes);
    HIP_TRY(hipMemcpyAsync(h.data(), c->sum_buf.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    out->kernel_ms = event_ms(c->ev_sum[0], c->ev_sum[1]);
    const double *h_f64 = reinterpret_cast<const double *>(h.data());
    const uint64_t *h_u64 = reinterpret_cast<const uint64_t *>(h_f64 + n_f64);
    const uint32_t *h_u32 = reinterpret_cast<const uint32_t *>(h_u64 + n_u64);
    out->pairs = h_u64[0];
    out->none_pairs = h_u64[1];
    out->nonfinite_pairs = h_u64[2];
    out->counted_pairs = h_u64[3];
    out->r2_sum = h_f64[0];
    std::copy(h_f64 + 1, h_f64 + 1 + L, out->score.begin());
    std::copy(h_u32, h_u32 + L, out->partners.begin());
    std::copy(h_f64 + 1 + LP, h_f64 + 1 + LP + nb, out->bin_r2_sum.begin());
    std::copy(h_u64 + 4, h_u64 + 4 + nb, out->bin_pairs.begin());
    // the kernel's own accounting against the host's plan
    const uint64_t expect = run_pairs(c, lb, le);
    if (out->pairs != expect || out->pairs != out->none_pairs + out->nonfinite_pairs + out->counted_pairs)
        return fail(WLD_E_HIP, "internal: summary counted %llu pairs (%llu none, %llu nonfinite, %llu counted); "
                               "the range holds %llu",
                    (unsigned long long)out->pairs, (unsigned long long)out->none_pairs,
                    (unsigned long long)out->nonfinite_pairs, (unsigned long long)out->counted_pairs,
                    (unsigned long long)expect);
    return WLD_OK;
}

// ... on a device group: member k takes its shard of the chunk sequence (as
// run_host_group deals them) cut to [lb, le), on its own host thread; the
// members' summaries are added in member order.
int summary_group(wld_ctx *g, uint32_t lb, uint32_t le, uint64_t bin_width, uint32_t n_bins,
                  summary_plan::Summary *out) {
    const int G = (int)g->members.size();
    wld_ctx *c0 = g->members[0];
    std::vector<uint32_t> sb(G), se(G);
    for (int k = 0; k < G; ++k) {  // every range before any thread starts
        if (window_on(c0)) WLD_TRY(wld_shard_chunks_window(c0, G, k, &sb[k], &se[k]));
        else WLD_TRY(wld_shard_chunks(c0->L, G, k, &sb[k], &se[k]));
        sb[k] = std::max(sb[k], lb);
        se[k] = std::max(sb[k], std::min(se[k], le));
    }
    std::vector<summary_plan::Summary> part(G);
    std::vector<int> status(G, WLD_OK);
    std::vector<std::string> msg(G);
    std::vector<std::thread> th;
    for (int k = 0; k < G; ++k)
        th.emplace_back([&, k] {
            status[k] = summary_range(g->members[k], sb[k], se[k], bin_width, n_bins, &part[k]);
            if (status[k] != WLD_OK) msg[k] = wld_last_error();
        });
    for (auto &t : th) t.join();
    for (int k = 0; k < G; ++k)
        if (status[k] != WLD_OK)
            return fail(status[k], "device %d (shard %d): %s", g->members[k]->device, k, msg[k].c_str());
    *out = summary_plan::Summary{};
    for (int k = 0; k < G; ++k) summary_plan::merge(*out, part[k]);
    return WLD_OK;
}
}  // namespace

int wld_run_summary(wld_ctx *c, uint32_t chunk_begin, uint32_t chunk_end, uint64_t bin_width, uint32_t n_bins,
                    wld_summary *out) {
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    if (!c) return fail(WLD_E_ARG, "null context");
    wld_ctx *c0 = c->members.empty() ? c : c->members[0];
    for (wld_ctx *m : c->members.empty() ? std::vector<wld_ctx *>{c} : c->members) {
        if (!m->loaded) return fail(WLD_E_STATE, "wld_run_summary before wld_load");
        if (m->pend.active) return fail(WLD_E_STATE, "wld_run_summary during a run");
    }
    WLD_TRY(summary_check(c0, bin_width, n_bins));
    const uint32_t m = chunks_of(c0->L);
    if (chunk_end == 0 || chunk_end > m) chunk_end = m;
    if (chunk_begin > chunk_end) return fail(WLD_E_ARG, "chunk range [%u,%u) invalid", chunk_begin, chunk_end);
    summary_plan::Summary s;
    if (c->members.empty()) WLD_TRY(summary_range(c, chunk_begin, chunk_end, bin_width, n_bins, &s));
    else WLD_TRY(summary_group(c, chunk_begin, chunk_end, bin_width, n_bins, &s));
    const size_t L = c0->L, nb = bin_width ? n_bins : 0;
    out->score = (double *)malloc(std::max<size_t>(L, 1) * sizeof(double));
    out->partners = (uint32_t *)malloc(std::max<size_t>(L, 1) * sizeof(uint32_t));
    if (nb) {
        out->bin_pairs = (uint64_t *)malloc(nb * sizeof(uint64_t));
        out->bin_r2_sum = (double *)malloc(nb * sizeof(double));
    }
    if (!out->score || !out->partners || (nb && (!out->bin_pairs || !out->bin_r2_sum))) {
        wld_summary_free(out);
        return fail(WLD_E_OOM, "host allocation of the summary (%zu sites, %zu bins) failed", L, nb);
    }
    std::copy(s.score.begin(), s.score.end(), out->score);
    std::copy(s.partners.begin(), s.partners.end(), out->partners);
    std::copy(s.bin_pairs.begin(), s.bin_pairs.end(), out->bin_pairs);
    std::copy(s.bin_r2_sum.begin(), s.bin_r2_sum.end(), out->bin_r2_sum);
    out->n_sites = L;
    out->bin_width = bin_width;
    out->n_bins = (uint32_t)nb;
    out->pairs = s.pairs;
    out->none_pairs = s.none_pairs;
    out->nonfinite_pairs = s.nonfinite_pairs;
    out->counted_pairs = s.counted_pairs;
    out->r2_sum = s.r2_sum;
    out->kernel_ms = s.kernel_ms;
    return WLD_OK;
}

void wld_summary_free(wld_summary *s) {
    if (!s) return;
    free(s->score);
    free(s->partners);
    free(s->bin_pairs);
    free(s->bin_r2_sum);
    memset(s, 0, sizeof(*s));
}

namespace {
// What wld_run_heatmap refuses, checked on a loaded single-device context
// (every member of a group holds the same load).
int heatmap_check(wld_ctx *c, const int32_t *site_cell, uint32_t n_cells, int stat) {
    if (n_cells == 0) return fail(WLD_E_ARG, "wld_run_heatmap: n_cells 0");
    if (n_cells > WLD_HEAT_MAX_CELLS)
        return fail(WLD_E_ARG, "wld_run_heatmap: n_cells %u exceeds %u", n_cells, (unsigned)WLD_HEAT_MAX_CELLS);
    if (stat != WLD_HEAT_R2 && stat != WLD_HEAT_ABS_DPRIME)
        return fail(WLD_E_ARG, "wld_run_heatmap: unknown stat %d", stat);
    if (!site_cell) return fail(WLD_E_ARG, "wld_run_heatmap: null site_cell");
    if (c->safe)
        return fail(WLD_E_ARG, "wld_run_heatmap needs finite weights (this load takes the select loop)");
    const heatmap_plan::MapCheck m = heatmap_plan::validate(site_cell, (uint32_t)c->L, n_cells);
    if (m.what == heatmap_plan::kMapTooLarge)
        return fail(WLD_E_ARG, "wld_run_heatmap: site_cell[%u] = %d is not below n_cells %u", m.index,
                    site_cell[m.index], n_cells);
    if (m.what == heatmap_plan::kMapNegative)
        return fail(WLD_E_ARG, "wld_run_heatmap: site_cell[%u] = %d (-1 means no cell)", m.index, site_cell[m.index]);
    if (m.what == heatmap_plan::kMapDescends)
        return fail(WLD_E_ARG, "wld_run_heatmap needs non-decreasing cell ids: site_cell[%u] = %d < site_cell[%u] = %d",
                    m.index, site_cell[m.index], m.prev, site_cell[m.prev]);
    return WLD_OK;
}

// The heat map of the linear chunks [lb, le) on one device (site_cell
// checked): the range's tile list under the window, cut to the tiles that
// touch a cell, in a buffer of its own — the row path's cached list, its
// range and seg_clear are not touched — zeroed accumulators, one launch, one
// copy back.  Touches no staging, segment count, chunk total, run counter or
// row-path event.
int heatmap_range(wld_ctx *c, const int32_t *site_cell, uint32_t n_cells, int stat, uint32_t lb, uint32_t le,
                  heatmap_plan::Heatmap *out) {
    WLD_TRY(set_dev(c));
    if (!c->loaded) return fail(WLD_E_STATE, "wld_run_heatmap before wld_load");
    if (c->pend.active) return fail(WLD_E_STATE, "wld_run_heatmap during a run");
    const size_t L = c->L, LP = c->LP, nc2 = (size_t)n_cells * n_cells, TB = LP / kTile;
    *out = heatmap_plan::Heatmap{};
    out->n_cells = n_cells;
    try {
        out->count.assign(nc2, 0);
        out->sum.assign(nc2, 0.0);
        out->max_key.assign(nc2, heatmap_plan::kNoKey);
    } catch (const std::bad_alloc &) {
        return fail(WLD_E_OOM, "host allocation of the heat map (%u x %u cells) failed", n_cells, n_cells);
    }
    if (lb >= le) return WLD_OK;
    const bool windowed = window_on(c);
    if (windowed && c->win_hi_host.size() != L) return fail(WLD_E_STATE, "internal: the window has no plan");
    // the plan: block limits, the filtered list, the pairs the launch must see
    const heatmap_plan::Blocks blk = heatmap_plan::blocks(site_cell, (uint32_t)L, (uint32_t)TB);
    const uint32_t T_used = (uint32_t)((L + kTile - 1) / kTile), n = chunk_rows_of(L);
    std::vector<uint32_t> t = heatmap_plan::filter_tiles(
        windowed ? window_plan::range_tiles(n, T_used, lb, le, c->win_hi_host) : tile_order::range_tiles(n, T_used, lb, le),
        blk);
    out->tiles = t.size();
    const uint64_t expect =
        heatmap_plan::considered_pairs(site_cell, windowed ? c->win_hi_host.data() : nullptr, (uint32_t)L, lb, le);
    if (t.empty()) {
        if (expect) return fail(WLD_E_HIP, "internal: the heat map's tile list is empty; the range holds %llu pairs",
                                (unsigned long long)expect);
        return WLD_OK;
    }
    if (!c->opt_tile_rows && t.size() >= 4096 && T_used < 65535)
        t = xcd_order(t, tile_order::super_block_side((uint32_t)c->NP));
    WLD_TRY(ensure_ref_layout(c));
    for (auto &e : c->ev_heat)
        if (!e) HIP_TRY(hipEventCreate(&e));
    // {sum[nc2]} f64 | {classes[4], count[nc2]} u64 | max_key[nc2] u32: one memset
    const size_t bytes = 8 * nc2 + 8 * (4 + nc2) + 4 * nc2;
    WLD_TRY(ensure(c->heat_buf, bytes));
    WLD_TRY(ensure(c->heat_tiles, t.size() * sizeof(uint32_t)));
    WLD_TRY(ensure(c->heat_map, (LP + 2 * TB) * sizeof(int32_t)));
    std::vector<int32_t> map(LP + 2 * TB, -1);  // site_cell[LP] (-1 past L), blk_lo[TB], blk_hi[TB]
    std::copy(site_cell, site_cell + L, map.begin());
    std::copy(blk.lo.begin(), blk.lo.end(), map.begin() + LP);
    std::copy(blk.hi.begin(), blk.hi.end(), map.begin() + LP + TB);
    HIP_TRY(hipMemcpyAsync(c->heat_map.p, map.data(), map.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->heat_tiles.p, t.data(), t.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->heat_buf.p, 0, bytes, c->stream));
    double *d_sum = ptr<double>(c->heat_buf);
    unsigned long long *d_cls = reinterpret_cast<unsigned long long *>(d_sum + nc2);
    unsigned long long *d_cnt = d_cls + 4;
    uint32_t *d_key = reinterpret_cast<uint32_t *>(d_cnt + nc2);
    const int32_t *d_map = ptr<int32_t>(c->heat_map);
    const HeatmapArgs ha{d_cls, d_cnt, d_sum, d_key, d_map, d_map + LP, d_map + LP + TB, n_cells, stat};
    ValuLaunch v = ref_valu_launch(c, 0.0f);  // (finite weights: heatmap_check)
    v.tiles = ptr<uint32_t>(c->heat_tiles);
    v.n_tiles = (uint32_t)t.size();
    OrderArgs o{};  // the window only
    o.L = (uint32_t)L;
    o.T = (uint32_t)TB;
    o.win_hi = windowed ? ptr<uint32_t>(c->win_hi) : nullptr;
    HIP_TRY(hipEventRecord(c->ev_heat[0], c->stream));
    launch_pair_heatmap(v, o, ha, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_heat[1], c->stream));
    uint64_t cls[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(out->sum.data(), d_sum, 8 * nc2, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(cls, d_cls, sizeof(cls), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out->count.data(), d_cnt, 8 * nc2, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out->max_key.data(), d_key, 4 * nc2, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (map and t are read by the copies)
    out->kernel_ms = event_ms(c->ev_heat[0], c->ev_heat[1]);
    out->pairs = cls[0];
    out->none_pairs = cls[1];
    out->nonfinite_pairs = cls[2];
    uint64_t in_cells = 0;
    for (uint64_t x : out->count) in_cells += x;
    out->counted_pairs = in_cells;
    // the kernel's own accounting against the host's plan
    if (out->pairs != expect || out->pairs != out->none_pairs + out->nonfinite_pairs + out->counted_pairs)
        return fail(WLD_E_HIP, "internal: heat map counted %llu pairs (%llu none, %llu nonfinite, %llu in cells); "
                               "the range holds %llu",
                    (unsigned long long)out->pairs, (unsigned long long)out->none_pairs,
                    (unsigned long long)out->nonfinite_pairs, (unsigned long long)out->counted_pairs,
                    (unsigned long long)expect);
    return WLD_OK;
}

// ... on a device group: member k takes its shard of the chunk sequence (as
// summary_group deals them) cut to [lb, le), on its own host thread; the
// members' maps are merged in member order.
int heatmap_group(wld_ctx *g, const int32_t *site_cell, uint32_t n_cells, int stat, uint32_t lb, uint32_t le,
                  heatmap_plan::Heatmap *out) {
    const int G = (int)g->members.size();
    wld_ctx *c0 = g->members[0];
    std::vector<uint32_t> sb(G), se(G);
    for (int k = 0; k < G; ++k) {  // every range before any thread starts
        if (window_on(c0)) WLD_TRY(wld_shard_chunks_window(c0, G, k, &sb[k], &se[k]));
        else WLD_TRY(wld_shard_chunks(c0->L, G, k, &sb[k], &se[k]));
        sb[k] = std::max(sb[k], lb);
        se[k] = std::max(sb[k], std::min(se[k], le));
    }
    std::vector<heatmap_plan::Heatmap> part(G);
    std::vector<int> status(G, WLD_OK);
    std::vector<std::string> msg(G);
    std::vector<std::thread> th;
    for (int k = 0; k < G; ++k)
        th.emplace_back([&, k] {
            status[k] = heatmap_range(g->members[k], site_cell, n_cells, stat, sb[k], se[k], &part[k]);
            if (status[k] != WLD_OK) msg[k] = wld_last_error();
        });
    for (auto &t : th) t.join();
    for (int k = 0; k < G; ++k)
        if (status[k] != WLD_OK)
            return fail(status[k], "device %d (shard %d): %s", g->members[k]->device, k, msg[k].c_str());
    *out = heatmap_plan::Heatmap{};
    for (int k = 0; k < G; ++k) heatmap_plan::merge(*out, part[k]);
    return WLD_OK;
}
}  // namespace

int wld_run_heatmap(wld_ctx *c, const int32_t *site_cell, uint32_t n_cells, int stat, uint32_t chunk_begin,
                    uint32_t chunk_end, wld_heatmap *out) {
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    if (!c) return fail(WLD_E_ARG, "null context");
    wld_ctx *c0 = c->members.empty() ? c : c->members[0];
    for (wld_ctx *m : c->members.empty() ? std::vector<wld_ctx *>{c} : c->members) {
        if (!m->loaded) return fail(WLD_E_STATE, "wld_run_heatmap before wld_load");
        if (m->pend.active) return fail(WLD_E_STATE, "wld_run_heatmap during a run");
    }
    WLD_TRY(heatmap_check(c0, site_cell, n_cells, stat));
    const uint32_t m = chunks_of(c0->L);
    if (chunk_end == 0 || chunk_end > m) chunk_end = m;
    if (chunk_begin > chunk_end) return fail(WLD_E_ARG, "chunk range [%u,%u) invalid", chunk_begin, chunk_end);
    heatmap_plan::Heatmap h;
    if (c->members.empty()) WLD_TRY(heatmap_range(c, site_cell, n_cells, stat, chunk_begin, chunk_end, &h));
    else WLD_TRY(heatmap_group(c, site_cell, n_cells, stat, chunk_begin, chunk_end, &h));
    const size_t nc2 = (size_t)n_cells * n_cells;
    out->count = (uint64_t *)malloc(nc2 * sizeof(uint64_t));
    out->sum = (double *)malloc(nc2 * sizeof(double));
    out->max = (float *)malloc(nc2 * sizeof(float));
    if (!out->count || !out->sum || !out->max) {
        wld_heatmap_free(out);
        return fail(WLD_E_OOM, "host allocation of the heat map (%u x %u cells) failed", n_cells, n_cells);
    }
    for (size_t i = 0; i < nc2; ++i) {
        out->count[i] = h.count[i];
        out->sum[i] = h.sum[i];
        out->max[i] = h.count[i] ? heatmap_plan::key_float(h.max_key[i]) : std::nanf("");
    }
    out->n_cells = n_cells;
    out->stat = stat;
    out->pairs = h.pairs;
    out->none_pairs = h.none_pairs;
    out->nonfinite_pairs = h.nonfinite_pairs;
    out->counted_pairs = h.counted_pairs;
    out->tiles = h.tiles;
    out->kernel_ms = h.kernel_ms;
    return WLD_OK;
}

void wld_heatmap_free(wld_heatmap *h) {
    if (!h) return;
    free(h->count);
    free(h->sum);
    free(h->max);
    memset(h, 0, sizeof(*h));
}

namespace {
// What wld_run_annot_scores refuses, checked on a loaded single-device context
// (every member of a group holds the same load).
int annot_check(wld_ctx *c, const float *annot, uint32_t n_annot, int flags) {
    if (n_annot == 0) return fail(WLD_E_ARG, "wld_run_annot_scores: n_annot 0");
    if (n_annot > WLD_ANNOT_MAX)
        return fail(WLD_E_ARG, "wld_run_annot_scores: n_annot %u exceeds %u", n_annot, (unsigned)WLD_ANNOT_MAX);
    if (flags & ~WLD_ANNOT_SELF) return fail(WLD_E_ARG, "wld_run_annot_scores: unknown flags 0x%x", (unsigned)flags);
    if (!annot) return fail(WLD_E_ARG, "wld_run_annot_scores: null annot");
    if (c->safe)
        return fail(WLD_E_ARG, "wld_run_annot_scores needs finite weights (this load takes the select loop)");
    const annot_plan::Check k = annot_plan::validate(annot, c->L, n_annot);
    if (!k.ok)
        return fail(WLD_E_ARG, "wld_run_annot_scores: annot[site %llu][column %u] = %g is not finite",
                    (unsigned long long)k.site, k.column, (double)annot[k.site * n_annot + k.column]);
    return WLD_OK;
}

// The partitioned scores of the linear chunks [lb, le) on one device (annot
// checked; im: its padded image): the range's tile list under the window in a
// buffer of its own — the row path's cached list, its range and seg_clear are
// not touched — zeroed accumulators, one launch, one copy back, then the self
// terms on the host.  Touches no staging, segment count, chunk total, run
// counter or row-path event.
int annot_range(wld_ctx *c, const float *annot, const annot_plan::Image &im, uint32_t n_annot, int flags, uint32_t lb,
                uint32_t le, annot_plan::Scores *out) {
    WLD_TRY(set_dev(c));
    if (!c->loaded) return fail(WLD_E_STATE, "wld_run_annot_scores before wld_load");
    if (c->pend.active) return fail(WLD_E_STATE, "wld_run_annot_scores during a run");
    const size_t L = c->L, LP = c->LP, CP = im.CP, TB = LP / kTile;
    *out = annot_plan::Scores{};
    out->n_sites = L;
    out->n_annot = n_annot;
    out->flags = flags;
    std::vector<double> h_score;
    std::vector<uint8_t> h_ok;
    try {
        out->score.assign(L * n_annot, 0.0);
        out->partners.assign(L, 0);
        h_score.resize(LP * CP);
        h_ok.resize(LP);
    } catch (const std::bad_alloc &) {
        return fail(WLD_E_OOM, "host allocation of the scores (%zu sites x %u columns) failed", L, n_annot);
    }
    if (lb >= le) return WLD_OK;
    if (im.values.size() != LP * CP || im.zero.size() != TB * (CP / 16))
        return fail(WLD_E_STATE, "internal: the annotation image does not fit the load");
    const bool windowed = window_on(c);
    if (windowed && c->win_hi_host.size() != L) return fail(WLD_E_STATE, "internal: the window has no plan");
    const uint32_t T_used = (uint32_t)((L + kTile - 1) / kTile), n = chunk_rows_of(L);
    std::vector<uint32_t> t =
        windowed ? window_plan::range_tiles(n, T_used, lb, le, c->win_hi_host) : tile_order::range_tiles(n, T_used, lb, le);
    out->tiles = t.size();
    const uint64_t expect = run_pairs(c, lb, le);
    if (t.empty() && expect)
        return fail(WLD_E_HIP, "internal: the tile list is empty; the range holds %llu pairs", (unsigned long long)expect);
    if (!t.empty()) {
        if (!c->opt_tile_rows && t.size() >= 4096 && T_used < 65535)
            t = xcd_order(t, tile_order::super_block_side((uint32_t)c->NP));
        WLD_TRY(ensure_ref_layout(c));
        for (auto &e : c->ev_an)
            if (!e) HIP_TRY(hipEventCreate(&e));
        // {score[LP][CP]} f64 | counts[4] u64 | partners[LP] u32: one memset
        const size_t bytes = 8 * LP * CP + 8 * 4 + 4 * LP, img_bytes = 4 * LP * CP;
        WLD_TRY(ensure(c->an_buf, bytes));
        WLD_TRY(ensure(c->an_tiles, t.size() * sizeof(uint32_t)));
        WLD_TRY(ensure(c->an_img, img_bytes + im.zero.size()));
        float *d_img = ptr<float>(c->an_img);
        uint8_t *d_zero = ptr<uint8_t>(c->an_img) + img_bytes;
        HIP_TRY(hipMemcpyAsync(d_img, im.values.data(), img_bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_zero, im.zero.data(), im.zero.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->an_tiles.p, t.data(), t.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(c->an_buf.p, 0, bytes, c->stream));
        double *d_score = ptr<double>(c->an_buf);
        unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(d_score + LP * CP);
        uint32_t *d_part = reinterpret_cast<uint32_t *>(d_cnt + 4);
        const AnnotArgs aa{d_cnt, d_score, d_part, d_img, d_zero, (uint32_t)CP};
        ValuLaunch v = ref_valu_launch(c, 0.0f);  // (finite weights: annot_check)
        v.tiles = ptr<uint32_t>(c->an_tiles);
        v.n_tiles = (uint32_t)t.size();
        OrderArgs o{};  // the window only
        o.L = (uint32_t)L;
        o.T = (uint32_t)TB;
        o.win_hi = windowed ? ptr<uint32_t>(c->win_hi) : nullptr;
        HIP_TRY(hipEventRecord(c->ev_an[0], c->stream));
        launch_pair_annot(v, o, aa, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev_an[1], c->stream));
        uint64_t cls[4] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpyAsync(h_score.data(), d_score, 8 * LP * CP, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(cls, d_cnt, sizeof(cls), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(out->partners.data(), d_part, 4 * L, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // (t and the image are read by the copies)
        out->kernel_ms = event_ms(c->ev_an[0], c->ev_an[1]);
        out->pairs = cls[0];
        out->none_pairs = cls[1];
        out->nonfinite_pairs = cls[2];
        out->counted_pairs = cls[3];
        for (size_t i = 0; i < L; ++i)
            std::copy(h_score.begin() + i * CP, h_score.begin() + i * CP + n_annot, out->score.begin() + i * n_annot);
        // the kernel's own accounting against the host's plan
        if (out->pairs != expect || out->pairs != out->none_pairs + out->nonfinite_pairs + out->counted_pairs)
            return fail(WLD_E_HIP, "internal: annot scores counted %llu pairs (%llu none, %llu nonfinite, %llu counted); "
                                   "the range holds %llu",
                        (unsigned long long)out->pairs, (unsigned long long)out->none_pairs,
                        (unsigned long long)out->nonfinite_pairs, (unsigned long long)out->counted_pairs,
                        (unsigned long long)expect);
    }
    if (flags & WLD_ANNOT_SELF) {
        // r2(i, i) = 1 for the sites with a major and a minor symbol whose
        // diagonal chunk the range holds: one more exact term each
        HIP_TRY(hipMemcpyAsync(h_ok.data(), c->site_ok.p, L, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < L; ++i)
            if (h_ok[i] && annot_plan::self_in_range(L, i, lb, le))
                for (uint32_t k = 0; k < n_annot; ++k) out->score[i * n_annot + k] += (double)annot[i * n_annot + k];
    }
    return WLD_OK;
}

// ... on a device group: member k takes its shard of the chunk sequence (as
// summary_group deals them) cut to [lb, le), on its own host thread; the
// members' results are added in member order.
int annot_group(wld_ctx *g, const float *annot, const annot_plan::Image &im, uint32_t n_annot, int flags, uint32_t lb,
                uint32_t le, annot_plan::Scores *out) {
    const int G = (int)g->members.size();
    wld_ctx *c0 = g->members[0];
    std::vector<uint32_t> sb(G), se(G);
    for (int k = 0; k < G; ++k) {  // every range before any thread starts
        if (window_on(c0)) WLD_TRY(wld_shard_chunks_window(c0, G, k, &sb[k], &se[k]));
        else WLD_TRY(wld_shard_chunks(c0->L, G, k, &sb[k], &se[k]));
        sb[k] = std::max(sb[k], lb);
        se[k] = std::max(sb[k], std::min(se[k], le));
    }
    std::vector<annot_plan::Scores> part(G);
    std::vector<int> status(G, WLD_OK);
    std::vector<std::string> msg(G);
    std::vector<std::thread> th;
    for (int k = 0; k < G; ++k)
        th.emplace_back([&, k] {
            status[k] = annot_range(g->members[k], annot, im, n_annot, flags, sb[k], se[k], &part[k]);
            if (status[k] != WLD_OK) msg[k] = wld_last_error();
        });
    for (auto &t : th) t.join();
    for (int k = 0; k < G; ++k)
        if (status[k] != WLD_OK)
            return fail(status[k], "device %d (shard %d): %s", g->members[k]->device, k, msg[k].c_str());
    *out = std::move(part[0]);
    for (int k = 1; k < G; ++k)
        if (!annot_plan::merge(*out, part[k])) return fail(WLD_E_STATE, "internal: the members' results differ in shape");
    return WLD_OK;
}
}  // namespace

int wld_run_annot_scores(wld_ctx *c, const float *annot, uint32_t n_annot, int flags, uint32_t chunk_begin,
                         uint32_t chunk_end, wld_annot_scores *out) {
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    if (!c) return fail(WLD_E_ARG, "null context");
    wld_ctx *c0 = c->members.empty() ? c : c->members[0];
    for (wld_ctx *m : c->members.empty() ? std::vector<wld_ctx *>{c} : c->members) {
        if (!m->loaded) return fail(WLD_E_STATE, "wld_run_annot_scores before wld_load");
        if (m->pend.active) return fail(WLD_E_STATE, "wld_run_annot_scores during a run");
    }
    WLD_TRY(annot_check(c0, annot, n_annot, flags));
    const uint32_t m = chunks_of(c0->L);
    if (chunk_end == 0 || chunk_end > m) chunk_end = m;
    if (chunk_begin > chunk_end) return fail(WLD_E_ARG, "chunk range [%u,%u) invalid", chunk_begin, chunk_end);
    const size_t L = c0->L;
    annot_plan::Image im;
    try {
        im = annot_plan::build_image(annot, L, n_annot, c0->LP);
    } catch (const std::bad_alloc &) {
        return fail(WLD_E_OOM, "host allocation of the annotation image (%zu sites x %u columns) failed", L, n_annot);
    }
    annot_plan::Scores s;
    if (c->members.empty()) WLD_TRY(annot_range(c, annot, im, n_annot, flags, chunk_begin, chunk_end, &s));
    else WLD_TRY(annot_group(c, annot, im, n_annot, flags, chunk_begin, chunk_end, &s));
    out->score = (double *)malloc(std::max<size_t>(L * n_annot, 1) * sizeof(double));
    out->partners = (uint32_t *)malloc(std::max<size_t>(L, 1) * sizeof(uint32_t));
    if (!out->score || !out->partners) {
        wld_annot_scores_free(out);
        return fail(WLD_E_OOM, "host allocation of the scores (%zu sites x %u columns) failed", L, n_annot);
    }
    std::copy(s.score.begin(), s.score.end(), out->score);
    std::copy(s.partners.begin(), s.partners.end(), out->partners);
    out->n_sites = L;
    out->n_annot = n_annot;
    out->flags = flags;
    out->pairs = s.pairs;
    out->none_pairs = s.none_pairs;
    out->nonfinite_pairs = s.nonfinite_pairs;
    out->counted_pairs = s.counted_pairs;
    out->tiles = s.tiles;
    out->kernel_ms = s.kernel_ms;
    return WLD_OK;
}

int wld_annot_scores_merge(wld_annot_scores *into, const wld_annot_scores *from) {
    if (!into || !from) return fail(WLD_E_ARG, "wld_annot_scores_merge: null result");
    if (into->n_sites != from->n_sites || into->n_annot != from->n_annot || into->flags != from->flags)
        return fail(WLD_E_ARG, "wld_annot_scores_merge: the results differ in shape (%llu x %u, flags %d; %llu x %u, flags %d)",
                    (unsigned long long)into->n_sites, into->n_annot, into->flags, (unsigned long long)from->n_sites,
                    from->n_annot, from->flags);
    if (into->n_sites && (!into->score || !into->partners || !from->score || !from->partners))
        return fail(WLD_E_ARG, "wld_annot_scores_merge: a result without arrays");
    into->pairs += from->pairs;
    into->none_pairs += from->none_pairs;
    into->nonfinite_pairs += from->nonfinite_pairs;
    into->counted_pairs += from->counted_pairs;
    into->tiles += from->tiles;
    into->kernel_ms = std::max(into->kernel_ms, from->kernel_ms);
    const size_t n = (size_t)into->n_sites * into->n_annot;
    for (size_t i = 0; i < n; ++i) into->score[i] += from->score[i];
    for (size_t i = 0; i < into->n_sites; ++i) into->partners[i] += from->partners[i];
    return WLD_OK;
}

void wld_annot_scores_free(wld_annot_scores *s) {
    if (!s) return;
    free(s->score);
    free(s->partners);
    memset(s, 0, sizeof(*s));
}


namespace {
static_assert(WLD_MATRIX_R2 == matrix_plan::kStatR2 && WLD_MATRIX_R == matrix_plan::kStatR &&
                  WLD_MATRIX_D == matrix_plan::kStatD && WLD_MATRIX_DPRIME == matrix_plan::kStatDPrime &&
                  WLD_MATRIX_F32 == matrix_plan::kF32 && WLD_MATRIX_F16 == matrix_plan::kF16 &&
                  WLD_MATRIX_ZERO_MISSING == matrix_plan::kZeroMissing,
              "matrix_plan.hpp restates the header's constants");

// What the matrix calls refuse, in the contract's order: the state, then the
// arguments (matrix_plan::validate), then the load's weights.  *q: the
// rectangle with its ends resolved.
int matrix_check(wld_ctx *c, const char *who, uint32_t rb, uint32_t re, uint32_t cb, uint32_t ce, int stat, int dtype,
                 int flags, const void *dst, size_t ld, matrix_plan::Rect *q) {
    WLD_TRY(set_dev(c));
    if (!c->loaded) return fail(WLD_E_STATE, "%s before wld_load", who);
    if (c->pend.active) return fail(WLD_E_STATE, "%s during a run", who);
    switch (matrix_plan::validate(c->L, rb, re, cb, ce, stat, dtype, flags, ld, dst != nullptr, q)) {
        case matrix_plan::kOk: break;
        case matrix_plan::kStat: return fail(WLD_E_ARG, "%s: unknown stat %d", who, stat);
        case matrix_plan::kDtype: return fail(WLD_E_ARG, "%s: unknown dtype %d", who, dtype);
        case matrix_plan::kFlags: return fail(WLD_E_ARG, "%s: unknown flags 0x%x", who, (unsigned)flags);
        case matrix_plan::kNull: return fail(WLD_E_ARG, "%s: null destination", who);
        case matrix_plan::kRange:
            return fail(WLD_E_ARG, "%s: rows [%u,%u) x columns [%u,%u) exceed the %zu loaded sites", who, rb, re, cb, ce,
                        c->L);
        case matrix_plan::kEmpty:
            return fail(WLD_E_ARG, "%s: rows [%u,%u) x columns [%u,%u) hold no entry", who, rb, re, cb, ce);
        case matrix_plan::kLd:
            return fail(WLD_E_ARG, "%s: ld %zu is below the rectangle's width %u", who, ld, q->c1 - q->c0);
    }
    if (c->safe) return fail(WLD_E_ARG, "%s needs finite weights (this load takes the select loop)", who);
    if (window_on(c) && c->win_hi_host.size() != c->L) return fail(WLD_E_STATE, "internal: the window has no plan");
    return WLD_OK;
}

void matrix_info_init(wld_matrix_info *out, const matrix_plan::Rect &q, int stat, int dtype, int flags) {
    memset(out, 0, sizeof(*out));
    out->row_begin = q.r0, out->row_end = q.r1, out->col_begin = q.c0, out->col_end = q.c1;
    out->stat = stat, out->dtype = dtype, out->flags = flags;
}

// One band of the call's rectangle into device memory (d_dst: the element of
// entry (band.r0, band.c0)): the band's tile and fill lists in buffers of the
// matrix calls' own, zeroed class counts, the fill and pair launches, the
// counts back; returns after the work has completed, its counts, tiles and
// time added to *out.  Touches no staging, segment count, chunk total, run
// counter, cached tile list or row-path event.
int matrix_band(wld_ctx *c, const matrix_plan::Rect &full, const matrix_plan::Rect &band, int stat, int dtype,
                int flags, void *d_dst, size_t ld, wld_matrix_info *out) {
    const size_t L = c->L, LP = c->LP;
    const bool windowed = window_on(c);
    matrix_plan::Plan p;
    try {
        p = matrix_plan::plan((uint32_t)L, windowed ? c->win_hi_host.data() : nullptr, band);
        const uint32_t T_used = (uint32_t)((L + kTile - 1) / kTile);
        out->tiles += p.tiles.size();
        if (!c->opt_tile_rows && p.tiles.size() >= 4096 && T_used < 65535)
            p.tiles = xcd_order(p.tiles, tile_order::super_block_side((uint32_t)c->NP));
    } catch (const std::bad_alloc &) {
        return fail(WLD_E_OOM, "host allocation of the matrix's tile list failed");
    }
    const size_t nt = p.tiles.size(), nf = p.fill.size();
    if (nt) WLD_TRY(ensure_ref_layout(c));
    for (auto &e : c->ev_mx)
        if (!e) HIP_TRY(hipEventCreate(&e));
    WLD_TRY(ensure(c->mx_lists, (nt + nf) * sizeof(uint32_t)));
    WLD_TRY(ensure(c->mx_cnt, 4 * sizeof(unsigned long long)));
    uint32_t *d_tiles = ptr<uint32_t>(c->mx_lists), *d_fill = d_tiles + nt;
    if (nt) HIP_TRY(hipMemcpyAsync(d_tiles, p.tiles.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if (nf) HIP_TRY(hipMemcpyAsync(d_fill, p.fill.data(), nf * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->mx_cnt.p, 0, 4 * sizeof(unsigned long long), c->stream));
    const MatrixArgs ma{d_dst, ld, full, band, stat, dtype == WLD_MATRIX_F16, (flags & WLD_MATRIX_ZERO_MISSING) != 0,
                        ptr<unsigned long long>(c->mx_cnt)};
    ValuLaunch v = ref_valu_launch(c, 0.0f);  // (finite weights: matrix_check)
    v.tiles = d_tiles;
    v.n_tiles = (uint32_t)nt;
    OrderArgs o{};  // the window only
    o.L = (uint32_t)L;
    o.T = (uint32_t)(LP / kTile);
    o.win_hi = windowed ? ptr<uint32_t>(c->win_hi) : nullptr;
    HIP_TRY(hipEventRecord(c->ev_mx[0], c->stream));
    launch_matrix_fill(d_fill, (uint32_t)nf, ptr<uint8_t>(c->site_ok), ma, c->stream);
    launch_pair_matrix(v, o, ma, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_mx[1], c->stream));
    uint64_t cls[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(cls, c->mx_cnt.p, sizeof(cls), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (the lists are read by the copies)
    out->kernel_ms += event_ms(c->ev_mx[0], c->ev_mx[1]);
    out->pairs += cls[0];
    out->none_pairs += cls[1];
    out->nonfinite_pairs += cls[2];
    out->counted_pairs += cls[3];
    return WLD_OK;
}

// the kernels' own accounting against the host's plan
int matrix_account(wld_ctx *c, const matrix_plan::Rect &q, const wld_matrix_info *out) {
    const uint64_t expect =
        matrix_plan::count_pairs((uint32_t)c->L, window_on(c) ? c->win_hi_host.data() : nullptr, q);
    if (out->pairs != expect || out->pairs != out->none_pairs + out->nonfinite_pairs + out->counted_pairs)
        return fail(WLD_E_HIP, "internal: the matrix counted %llu pairs (%llu none, %llu nonfinite, %llu counted); "
                               "the rectangle holds %llu",
                    (unsigned long long)out->pairs, (unsigned long long)out->none_pairs,
                    (unsigned long long)out->nonfinite_pairs, (unsigned long long)out->counted_pairs,
                    (unsigned long long)expect);
    return WLD_OK;
}
}  // namespace

int wld_run_matrix_device(wld_ctx *c, uint32_t row_begin, uint32_t row_end, uint32_t col_begin, uint32_t col_end,
                          int stat, int dtype, int flags, void *d_dst, size_t ld, wld_matrix_info *out) {
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    if (!c) return fail(WLD_E_ARG, "null context");
    matrix_plan::Rect q{};
    WLD_TRY(matrix_check(c, "wld_run_matrix_device", row_begin, row_end, col_begin, col_end, stat, dtype, flags, d_dst,
                         ld, &q));
    matrix_info_init(out, q, stat, dtype, flags);
    WLD_TRY(matrix_band(c, q, q, stat, dtype, flags, d_dst, ld, out));
    return matrix_account(c, q, out);
}

int wld_run_matrix(wld_ctx *c, uint32_t row_begin, uint32_t row_end, uint32_t col_begin, uint32_t col_end, int stat,
                   int dtype, int flags, void *h_dst, size_t ld, wld_matrix_info *out) {
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    if (!c) return fail(WLD_E_ARG, "null context");
    matrix_plan::Rect q{};
    WLD_TRY(matrix_check(c, "wld_run_matrix", row_begin, row_end, col_begin, col_end, stat, dtype, flags, h_dst, ld, &q));
    matrix_info_init(out, q, stat, dtype, flags);
    const size_t eb = dtype == WLD_MATRIX_F16 ? 2 : 4, width = q.c1 - q.c0;
    std::vector<matrix_plan::Rect> bands;
    try {
        bands = matrix_plan::bands(q, eb, c->opt_matrix_bytes);
    } catch (const std::bad_alloc &) {
        return fail(WLD_E_OOM, "host allocation of the matrix's bands failed");
    }
    DevBuf buf;  // the call's own: released before it returns
    int st = ensure(buf, (size_t)(bands[0].r1 - bands[0].r0) * width * eb);
    for (size_t k = 0; k < bands.size() && st == WLD_OK; ++k) {
        const matrix_plan::Rect &b = bands[k];
        st = matrix_band(c, q, b, stat, dtype, flags, buf.p, width, out);
        if (st != WLD_OK) break;
        const hipError_t e = hipMemcpy2D(static_cast<char *>(h_dst) + (size_t)(b.r0 - q.r0) * ld * eb, ld * eb, buf.p,
                                         width * eb, width * eb, b.r1 - b.r0, hipMemcpyDeviceToHost);
        if (e != hipSuccess) st = fail(WLD_E_HIP, "wld_run_matrix copy: %s", hipGetErrorString(e));
    }
    release(buf);
    WLD_TRY(st);
    return matrix_account(c, q, out);
}

namespace {
namespace mbp = matrix_banded_plan;

// the window's limits on the host (null: no window), as matrix_check left them
const uint32_t *banded_limits(wld_ctx *c) { return window_on(c) ? c->win_hi_host.data() : nullptr; }

// What the banded matrix calls refuse, in wld_run_matrix_device's order: the
// state, then the arguments (matrix_banded_plan::validate), then the load's
// weights.  *q: the rows with their end resolved.
int banded_check(wld_ctx *c, const char *who, uint32_t rb, uint32_t re, uint32_t K, int stat, int dtype, int flags,
                 bool have_dst, size_t ld, mbp::Rows *q) {
    WLD_TRY(set_dev(c));
    if (!c->loaded) return fail(WLD_E_STATE, "%s before wld_load", who);
    if (c->pend.active) return fail(WLD_E_STATE, "%s during a run", who);
    if (window_on(c) && c->win_hi_host.size() != c->L) return fail(WLD_E_STATE, "internal: the window has no plan");
    const uint32_t needed = mbp::width((uint32_t)std::min<size_t>(c->L, mbp::kMaxSites), banded_limits(c));
    switch (mbp::validate(c->L, rb, re, K, needed, stat, dtype, flags, ld, have_dst, q)) {
        case mbp::kOk: break;
        case mbp::kStat: return fail(WLD_E_ARG, "%s: unknown stat %d", who, stat);
        case mbp::kDtype: return fail(WLD_E_ARG, "%s: unknown dtype %d", who, dtype);
        case mbp::kFlags: return fail(WLD_E_ARG, "%s: unknown flags 0x%x", who, (unsigned)flags);
        case mbp::kNull: return fail(WLD_E_ARG, "%s: null destination", who);
        case mbp::kSites:
            return fail(WLD_E_ARG, "%s: %zu loaded sites exceed the %llu that 16-bit tile indices address", who, c->L,
                        (unsigned long long)mbp::kMaxSites);
        case mbp::kRange: return fail(WLD_E_ARG, "%s: rows [%u,%u) exceed the %zu loaded sites", who, rb, re, c->L);
        case mbp::kEmpty: return fail(WLD_E_ARG, "%s: rows [%u,%u) hold no site", who, rb, re);
        case mbp::kWidth:
            return fail(WLD_E_ARG, "%s: bandwidth %u would drop in-window pairs; the window needs bandwidth %u", who, K,
                        needed);
        case mbp::kLd: return fail(WLD_E_ARG, "%s: ld %zu is below bandwidth + 1 = %llu", who, ld, (unsigned long long)K + 1);
    }
    if (c->safe) return fail(WLD_E_ARG, "%s needs finite weights (this load takes the select loop)", who);
    return WLD_OK;
}

void banded_info_init(wld_matrix_banded_info *out, const mbp::Rows &q, uint32_t K, int stat, int dtype, int flags) {
    memset(out, 0, sizeof(*out));
    out->row_begin = q.r0, out->row_end = q.r1, out->bandwidth = K;
    out->stat = stat, out->dtype = dtype, out->flags = flags;
}

// One strip of rows into device memory (d_dst: element k = 0 of row strip.r0):
// the strip's tile and fill lists in the matrix calls' own buffers, zeroed
// class counts, the fill and pair launches, the counts back; returns after the
// work has completed, its counts, tiles and time added to *out.  Touches no
// staging, segment count, chunk total, run counter, cached tile list or
// row-path event.
int banded_strip(wld_ctx *c, const mbp::Rows &strip, uint32_t K, int stat, int dtype, int flags, void *d_dst, size_t ld,
                 wld_matrix_banded_info *out) {
    const size_t L = c->L, LP = c->LP;
    const bool windowed = window_on(c);
    mbp::Plan p;
    try {
        p = mbp::plan((uint32_t)L, banded_limits(c), strip, K);
        const uint32_t T_used = (uint32_t)((L + kTile - 1) / kTile);
        out->tiles += p.tiles.size();
        if (!c->opt_tile_rows && p.tiles.size() >= 4096 && T_used < 65535)
            p.tiles = xcd_order(p.tiles, tile_order::super_block_side((uint32_t)c->NP));
    } catch (const std::bad_alloc &) {
        return fail(WLD_E_OOM, "host allocation of the banded matrix's tile list failed");
    }
    const size_t nt = p.tiles.size(), nf = p.fill.size();
    if (nf > 0xFFFFFFFFull) return fail(WLD_E_ARG, "the banded matrix's fill list exceeds a launch");
    if (nt) WLD_TRY(ensure_ref_layout(c));
    for (auto &e : c->ev_mx)
        if (!e) HIP_TRY(hipEventCreate(&e));
    WLD_TRY(ensure(c->mx_lists, nt * sizeof(uint32_t) + nf * sizeof(mbp::FillBlock)));
    WLD_TRY(ensure(c->mx_cnt, 4 * sizeof(unsigned long long)));
    uint32_t *d_tiles = ptr<uint32_t>(c->mx_lists);
    mbp::FillBlock *d_fill = reinterpret_cast<mbp::FillBlock *>(d_tiles + nt);
    if (nt) HIP_TRY(hipMemcpyAsync(d_tiles, p.tiles.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if (nf) HIP_TRY(hipMemcpyAsync(d_fill, p.fill.data(), nf * sizeof(mbp::FillBlock), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->mx_cnt.p, 0, 4 * sizeof(unsigned long long), c->stream));
    const MatrixBandedArgs ma{d_dst, ld, strip.r0, strip.r1, K, stat, dtype == WLD_MATRIX_F16,
                              (flags & WLD_MATRIX_ZERO_MISSING) != 0, ptr<unsigned long long>(c->mx_cnt)};
    ValuLaunch v = ref_valu_launch(c, 0.0f);  // (finite weights: banded_check)
    v.tiles = d_tiles;
    v.n_tiles = (uint32_t)nt;
    OrderArgs o{};  // the window only
    o.L = (uint32_t)L;
    o.T = (uint32_t)(LP / kTile);
    o.win_hi = windowed ? ptr<uint32_t>(c->win_hi) : nullptr;
    HIP_TRY(hipEventRecord(c->ev_mx[0], c->stream));
    launch_matrix_banded_fill(d_fill, (uint32_t)nf, ptr<uint8_t>(c->site_ok), ma, c->stream);
    launch_pair_matrix_banded(v, o, ma, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_mx[1], c->stream));
    uint64_t cls[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(cls, c->mx_cnt.p, sizeof(cls), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (the lists are read by the copies)
    out->kernel_ms += event_ms(c->ev_mx[0], c->ev_mx[1]);
    out->pairs += cls[0];
    out->none_pairs += cls[1];
    out->nonfinite_pairs += cls[2];
    out->counted_pairs += cls[3];
    return WLD_OK;
}

// the kernels' own accounting against the host's plan
int banded_account(wld_ctx *c, const mbp::Rows &q, const wld_matrix_banded_info *out) {
    const uint64_t expect = mbp::count_pairs((uint32_t)c->L, banded_limits(c), q);
    if (out->pairs != expect || out->pairs != out->none_pairs + out->nonfinite_pairs + out->counted_pairs)
        return fail(WLD_E_HIP, "internal: the banded matrix counted %llu pairs (%llu none, %llu nonfinite, %llu "
                               "counted); the rows hold %llu",
                    (unsigned long long)out->pairs, (unsigned long long)out->none_pairs,
                    (unsigned long long)out->nonfinite_pairs, (unsigned long long)out->counted_pairs,
                    (unsigned long long)expect);
    return WLD_OK;
}
}  // namespace

int wld_matrix_banded_width(wld_ctx *c, uint32_t *bandwidth_needed) {
    if (!c) return fail(WLD_E_ARG, "null context");
    if (!bandwidth_needed) return fail(WLD_E_ARG, "wld_matrix_banded_width: null output");
    WLD_TRY(set_dev(c));
    if (!c->loaded) return fail(WLD_E_STATE, "wld_matrix_banded_width before wld_load");
    if (window_on(c) && c->win_hi_host.size() != c->L) return fail(WLD_E_STATE, "internal: the window has no plan");
    if (c->L > mbp::kMaxSites)
        return fail(WLD_E_ARG, "wld_matrix_banded_width: %zu loaded sites exceed the %llu that 16-bit tile indices address",
                    c->L, (unsigned long long)mbp::kMaxSites);
    *bandwidth_needed = mbp::width((uint32_t)c->L, banded_limits(c));
    return WLD_OK;
}

int wld_run_matrix_banded_device(wld_ctx *c, uint32_t row_begin, uint32_t row_end, uint32_t bandwidth, int stat,
                                 int dtype, int flags, void *d_dst, size_t ld, wld_matrix_banded_info *out) {
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    if (!c) return fail(WLD_E_ARG, "null context");
    mbp::Rows q{};
    WLD_TRY(banded_check(c, "wld_run_matrix_banded_device", row_begin, row_end, bandwidth, stat, dtype, flags,
                         d_dst != nullptr, ld, &q));
    banded_info_init(out, q, bandwidth, stat, dtype, flags);
    WLD_TRY(banded_strip(c, q, bandwidth, stat, dtype, flags, d_dst, ld, out));
    return banded_account(c, q, out);
}

int wld_run_matrix_banded(wld_ctx *c, uint32_t row_begin, uint32_t row_end, uint32_t bandwidth, int stat, int dtype,
                          int flags, void *h_dst, size_t ld, wld_matrix_banded_info *out) {
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    if (!c) return fail(WLD_E_ARG, "null context");
    mbp::Rows q{};
    WLD_TRY(banded_check(c, "wld_run_matrix_banded", row_begin, row_end, bandwidth, stat, dtype, flags, h_dst != nullptr,
                         ld, &q));
    banded_info_init(out, q, bandwidth, stat, dtype, flags);
    const size_t eb = dtype == WLD_MATRIX_F16 ? 2 : 4, width = (size_t)bandwidth + 1;
    std::vector<mbp::Rows> strips;
    try {
        strips = mbp::strips(q, bandwidth, eb, c->opt_matrix_bytes);
    } catch (const std::bad_alloc &) {
        return fail(WLD_E_OOM, "host allocation of the banded matrix's strips failed");
    }
    DevBuf buf;  // the call's own: released before it returns
    int st = ensure(buf, (size_t)(strips[0].r1 - strips[0].r0) * width * eb);
    for (size_t k = 0; k < strips.size() && st == WLD_OK; ++k) {
        const mbp::Rows &s = strips[k];
        st = banded_strip(c, s, bandwidth, stat, dtype, flags, buf.p, width, out);
        if (st != WLD_OK) break;
        const hipError_t e = hipMemcpy2D(static_cast<char *>(h_dst) + (size_t)(s.r0 - q.r0) * ld * eb, ld * eb, buf.p,
                                         width * eb, width * eb, s.r1 - s.r0, hipMemcpyDeviceToHost);
        if (e != hipSuccess) st = fail(WLD_E_HIP, "wld_run_matrix_banded copy: %s", hipGetErrorString(e));
    }
    release(buf);
    WLD_TRY(st);
    return banded_account(c, q, out);
}

int wld_banded_apply_device(wld_ctx *c, const void *d_band, int band_dtype, size_t ld, uint32_t n_sites,
                            uint32_t bandwidth, const void *d_x, int x_dtype, size_t ldx, uint32_t n_cols, double *d_y,
                            size_t ldy) {
    const char *who = "wld_banded_apply_device";
    if (!c) return fail(WLD_E_ARG, "null context");
    WLD_TRY(set_dev(c));
    if (c->pend.active) return fail(WLD_E_STATE, "%s during a run", who);
    if (!d_band || !d_x || !d_y) return fail(WLD_E_ARG, "%s: null %s", who, !d_band ? "band" : !d_x ? "X" : "Y");
    if (band_dtype != WLD_MATRIX_F32 && band_dtype != WLD_MATRIX_F16)
        return fail(WLD_E_ARG, "%s: unknown band dtype %d", who, band_dtype);
    if (x_dtype != WLD_APPLY_X_F32 && x_dtype != WLD_APPLY_X_F64)
        return fail(WLD_E_ARG, "%s: unknown X dtype %d", who, x_dtype);
    if (!n_sites) return fail(WLD_E_ARG, "%s: no site", who);
    if (!n_cols) return fail(WLD_E_ARG, "%s: no column", who);
    if ((uint64_t)ld < (uint64_t)bandwidth + 1)
        return fail(WLD_E_ARG, "%s: ld %zu is below bandwidth + 1 = %llu", who, ld, (unsigned long long)bandwidth + 1);
    if (ldx < n_cols || ldy < n_cols)
        return fail(WLD_E_ARG, "%s: ldx %zu or ldy %zu is below the %u columns", who, ldx, ldy, n_cols);
    const BandedApplyArgs a{d_band, ld,   n_sites, bandwidth, band_dtype == WLD_MATRIX_F16, x_dtype == WLD_APPLY_X_F64,
                            d_x,    ldx,  n_cols,  d_y,       ldy};
    launch_banded_apply(a, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return WLD_OK;
}

int wld_banded_cholesky_device(wld_ctx *c, const void *d_band, int band_dtype, size_t ld, uint32_t n_sites,
                               uint32_t bandwidth, double ridge, const double *d_diag, double *d_factor, size_t ldf,
                               wld_banded_chol_info *out) {
    const char *who = "wld_banded_cholesky_device";
    if (!c) return fail(WLD_E_ARG, "null context");
    WLD_TRY(set_dev(c));
    if (c->pend.active) return fail(WLD_E_STATE, "%s during a run", who);
    if (!d_band || !d_factor || !out)
        return fail(WLD_E_ARG, "%s: null %s", who, !d_band ? "band" : !d_factor ? "factor" : "info");
    if (band_dtype != WLD_MATRIX_F32 && band_dtype != WLD_MATRIX_F16)
        return fail(WLD_E_ARG, "%s: unknown band dtype %d", who, band_dtype);
    if (!n_sites) return fail(WLD_E_ARG, "%s: no site", who);
    if ((uint64_t)ld < (uint64_t)bandwidth + 1 || (uint64_t)ldf < (uint64_t)bandwidth + 1)
        return fail(WLD_E_ARG, "%s: ld %zu or ldf %zu is below bandwidth + 1 = %llu", who, ld, ldf,
                    (unsigned long long)bandwidth + 1);
    if (!std::isfinite(ridge)) return fail(WLD_E_ARG, "%s: the ridge is not finite", who);
    {  // the extents [first element, one past the last element read or written)
        const size_t esz = band_dtype == WLD_MATRIX_F16 ? 2 : 4;
        const uintptr_t b0 = (uintptr_t)d_band, b1 = b0 + ((size_t)(n_sites - 1) * ld + bandwidth + 1) * esz;
        const uintptr_t f0 = (uintptr_t)d_factor, f1 = f0 + ((size_t)(n_sites - 1) * ldf + bandwidth + 1) * sizeof(double);
        if (b0 < f1 && f0 < b1) return fail(WLD_E_ARG, "%s: the factor overlaps the band", who);
    }
    for (auto &e : c->ev_chol)
        if (!e) HIP_TRY(hipEventCreate(&e));
    WLD_TRY(ensure(c->chol_status, sizeof(BandedCholStatus)));
    const BandedCholArgs a{d_band,   ld,  band_dtype == WLD_MATRIX_F16,         n_sites, bandwidth, ridge, d_diag,
                           d_factor, ldf, ptr<BandedCholStatus>(c->chol_status)};
    HIP_TRY(hipEventRecord(c->ev_chol[0], c->stream));
    launch_banded_chol(a, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_chol[1], c->stream));
    BandedCholStatus st{};
    HIP_TRY(hipMemcpyAsync(&st, c->chol_status.p, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    out->n_sites = n_sites;
    out->bandwidth = bandwidth;
    out->first_bad = st.first_bad;
    out->min_pivot = st.min_pivot;
    out->kernel_ms = event_ms(c->ev_chol[0], c->ev_chol[1]);
    return WLD_OK;
}

int wld_banded_solve_device(wld_ctx *c, const double *d_factor, size_t ldf, uint32_t n_sites, uint32_t bandwidth,
                            int mode, double *d_b, size_t ldb, uint32_t n_cols, double *kernel_ms) {
    const char *who = "wld_banded_solve_device";
    if (!c) return fail(WLD_E_ARG, "null context");
    WLD_TRY(set_dev(c));
    if (c->pend.active) return fail(WLD_E_STATE, "%s during a run", who);
    if (!d_factor || !d_b) return fail(WLD_E_ARG, "%s: null %s", who, !d_factor ? "factor" : "b");
    if (mode != WLD_SOLVE_FULL && mode != WLD_SOLVE_FORWARD && mode != WLD_SOLVE_BACKWARD)
        return fail(WLD_E_ARG, "%s: unknown mode %d", who, mode);
    if (!n_sites) return fail(WLD_E_ARG, "%s: no site", who);
    if (!n_cols) return fail(WLD_E_ARG, "%s: no column", who);
    if ((uint64_t)ldf < (uint64_t)bandwidth + 1)
        return fail(WLD_E_ARG, "%s: ldf %zu is below bandwidth + 1 = %llu", who, ldf, (unsigned long long)bandwidth + 1);
    if (ldb < n_cols) return fail(WLD_E_ARG, "%s: ldb %zu is below the %u columns", who, ldb, n_cols);
    for (auto &e : c->ev_chol)
        if (!e) HIP_TRY(hipEventCreate(&e));
    const BandedSolveArgs a{d_factor, ldf, n_sites, bandwidth, mode != WLD_SOLVE_BACKWARD, mode != WLD_SOLVE_FORWARD,
                            d_b,      ldb, n_cols};
    HIP_TRY(hipEventRecord(c->ev_chol[0], c->stream));
    launch_banded_solve(a, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_chol[1], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (kernel_ms) *kernel_ms = event_ms(c->ev_chol[0], c->ev_chol[1]);
    return WLD_OK;
}

namespace {
namespace bop = banded_omega_plan;

// the words of the sweep-scan calls on the device
struct OmegaWords {
    unsigned long long nonfinite, evaluated, skipped;
    uint32_t status, pad;
};

// the pair sums' launches and their counter, after the arguments were checked
int pairsum_run(wld_ctx *c, const void *d_band, int band_dtype, size_t ld, uint32_t n, uint32_t K, double *d_sums,
                size_t lds, wld_banded_pairsum_info *out) {
    for (auto &e : c->ev_om)
        if (!e) HIP_TRY(hipEventCreate(&e));
    WLD_TRY(ensure(c->om_words, sizeof(OmegaWords)));
    OmegaWords *w = ptr<OmegaWords>(c->om_words);
    HIP_TRY(hipMemsetAsync(w, 0, sizeof(OmegaWords), c->stream));
    const BandedPairsumArgs a{d_band, ld, band_dtype == WLD_MATRIX_F16, n, K, d_sums, lds, &w->nonfinite};
    HIP_TRY(hipEventRecord(c->ev_om[0], c->stream));
    launch_banded_pairsum(a, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_om[1], c->stream));
    OmegaWords h{};
    HIP_TRY(hipMemcpyAsync(&h, w, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    out->n_sites = n;
    out->bandwidth = K;
    out->nonfinite = h.nonfinite;
    out->kernel_ms = event_ms(c->ev_om[0], c->ev_om[1]);
    return WLD_OK;
}

// the scan's check launch, then the scan itself; the arguments were checked
int omega_run(wld_ctx *c, const char *who, const double *d_sums, size_t lds, uint32_t n, uint32_t K,
              const uint32_t *d_split, const uint32_t *d_lo, const uint32_t *d_hi, uint32_t n_splits, uint32_t min_side,
              double eps, double *d_omega, uint32_t *d_left, uint32_t *d_right, double *d_zns,
              wld_banded_omega_info *out) {
    for (auto &e : c->ev_om)
        if (!e) HIP_TRY(hipEventCreate(&e));
    WLD_TRY(ensure(c->om_words, sizeof(OmegaWords)));
    OmegaWords *w = ptr<OmegaWords>(c->om_words);
    OmegaWords h{};
    h.status = 0xFFFFFFFFu;
    HIP_TRY(hipMemcpyAsync(w, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    const BandedOmegaArgs a{d_sums, lds,     n,      K,       d_split, d_lo,          d_hi,      n_splits, min_side,
                            eps,    d_omega, d_left, d_right, d_zns,   &w->evaluated, &w->status};
    launch_banded_omega_check(a, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h, w, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (h.status != 0xFFFFFFFFu)
        return fail(WLD_E_ARG, "%s: split %u breaks lo <= split < hi < %u sites or hi - lo <= bandwidth %u", who, h.status, n,
                    K);
    HIP_TRY(hipEventRecord(c->ev_om[0], c->stream));
    launch_banded_omega(a, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_om[1], c->stream));
    HIP_TRY(hipMemcpyAsync(&h, w, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    out->n_splits = n_splits;
    out->evaluated = h.evaluated;
    out->skipped = h.skipped;
    out->kernel_ms = event_ms(c->ev_om[0], c->ev_om[1]);
    return WLD_OK;
}

// the refusal of a site_map that descends at i (banded_omega_plan::first_descent)
int omega_map_descends(const char *who, uint32_t i, uint64_t at_i, uint64_t before) {
    return fail(WLD_E_ARG, "%s needs a non-decreasing site_map: site_map[%u] = %llu < site_map[%u] = %llu", who, i,
                (unsigned long long)at_i, i - 1, (unsigned long long)before);
}

int omega_check_params(const char *who, uint32_t min_side, double eps) {
    if (min_side < 2) return fail(WLD_E_ARG, "%s: min_side %u is below 2", who, min_side);
    if (!std::isfinite(eps) || eps < 0.0) return fail(WLD_E_ARG, "%s: eps must be finite and >= 0", who);
    return WLD_OK;
}

// the buffers a wld_run_omega call owns on the device, released on every path
struct OmegaBufs {
    DevBuf band, sums, in, out;
    ~OmegaBufs() {
        for (DevBuf *b : {&band, &sums, &in, &out}) release(*b);
    }
};
}  // namespace

int wld_banded_pairsum_device(wld_ctx *c, const void *d_band, int band_dtype, size_t ld, uint32_t n_sites,
                              uint32_t bandwidth, double *d_sums, size_t lds_, wld_banded_pairsum_info *out) {
    const char *who = "wld_banded_pairsum_device";
    if (!c) return fail(WLD_E_ARG, "null context");
    WLD_TRY(set_dev(c));
    if (c->pend.active) return fail(WLD_E_STATE, "%s during a run", who);
    if (!d_band || !d_sums || !out)
        return fail(WLD_E_ARG, "%s: null %s", who, !d_band ? "band" : !d_sums ? "sums" : "info");
    if (band_dtype != WLD_MATRIX_F32 && band_dtype != WLD_MATRIX_F16)
        return fail(WLD_E_ARG, "%s: unknown band dtype %d", who, band_dtype);
    if (!n_sites) return fail(WLD_E_ARG, "%s: no site", who);
    if ((uint64_t)ld < (uint64_t)bandwidth + 1 || (uint64_t)lds_ < (uint64_t)bandwidth + 1)
        return fail(WLD_E_ARG, "%s: ld %zu or lds %zu is below bandwidth + 1 = %llu", who, ld, lds_,
                    (unsigned long long)bandwidth + 1);
    {  // the extents [first element, one past the last element read or written)
        const size_t esz = band_dtype == WLD_MATRIX_F16 ? 2 : 4;
        const uintptr_t b0 = (uintptr_t)d_band, b1 = b0 + ((size_t)(n_sites - 1) * ld + bandwidth + 1) * esz;
        const uintptr_t f0 = (uintptr_t)d_sums, f1 = f0 + ((size_t)(n_sites - 1) * lds_ + bandwidth + 1) * sizeof(double);
        if (b0 < f1 && f0 < b1) return fail(WLD_E_ARG, "%s: the sums overlap the band", who);
    }
    return pairsum_run(c, d_band, band_dtype, ld, n_sites, bandwidth, d_sums, lds_, out);
}

int wld_banded_omega_device(wld_ctx *c, const double *d_sums, size_t lds_, uint32_t n_sites, uint32_t bandwidth,
                            const uint32_t *d_split, const uint32_t *d_lo, const uint32_t *d_hi, uint32_t n_splits,
                            uint32_t min_side, double eps, double *d_omega, uint32_t *d_left, uint32_t *d_right,
                            double *d_zns, wld_banded_omega_info *out) {
    const char *who = "wld_banded_omega_device";
    if (!c) return fail(WLD_E_ARG, "null context");
    WLD_TRY(set_dev(c));
    if (c->pend.active) return fail(WLD_E_STATE, "%s during a run", who);
    if (!d_sums || !d_split || !d_lo || !d_hi || !d_omega || !d_left || !d_right || !d_zns || !out)
        return fail(WLD_E_ARG, "%s: null %s", who,
                    !d_sums ? "sums" : !d_split || !d_lo || !d_hi ? "split array" : !out ? "info" : "output");
    if (!n_sites) return fail(WLD_E_ARG, "%s: no site", who);
    if (!n_splits) return fail(WLD_E_ARG, "%s: no split", who);
    if ((uint64_t)lds_ < (uint64_t)bandwidth + 1)
        return fail(WLD_E_ARG, "%s: lds %zu is below bandwidth + 1 = %llu", who, lds_, (unsigned long long)bandwidth + 1);
    WLD_TRY(omega_check_params(who, min_side, eps));
    return omega_run(c, who, d_sums, lds_, n_sites, bandwidth, d_split, d_lo, d_hi, n_splits, min_side, eps, d_omega,
                     d_left, d_right, d_zns, out);
}

uint64_t wld_omega_n_splits(uint32_t n_sites, uint32_t n_grid) { return n_sites < 2 ? 0 : bop::n_splits(n_sites, n_grid); }

int wld_omega_splits(const uint64_t *site_map, uint32_t n_sites, uint32_t n_grid, uint32_t max_side,
                     uint64_t max_distance, uint64_t *position, uint32_t *split, uint32_t *lo, uint32_t *hi) {
    const char *who = "wld_omega_splits";
    if (!position || !split || !lo || !hi) return fail(WLD_E_ARG, "%s: null output", who);
    if (n_sites < 2) return fail(WLD_E_ARG, "%s: a split needs two sites, not %u", who, n_sites);
    if (!max_side) return fail(WLD_E_ARG, "%s: max_side 0", who);
    const uint32_t d = bop::first_descent(site_map, n_sites);
    if (d < n_sites) return omega_map_descends(who, d, site_map[d], site_map[d - 1]);
    bop::splits(site_map, n_sites, n_grid, max_side, max_distance, position, split, lo, hi);
    return WLD_OK;
}

void wld_omega_free(wld_omega *o) {
    if (!o) return;
    free(o->position);
    free(o->split);
    free(o->lo);
    free(o->hi);
    free(o->omega);
    free(o->left);
    free(o->right);
    free(o->zns);
    memset(o, 0, sizeof(*o));
}

int wld_run_omega(wld_ctx *c, uint32_t n_grid, uint32_t max_side, uint32_t min_side, uint64_t max_distance, double eps,
                  int band_dtype, wld_omega *out) {
    const char *who = "wld_run_omega";
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    if (!c) return fail(WLD_E_ARG, "null context");
    WLD_TRY(set_dev(c));
    if (!c->loaded) return fail(WLD_E_STATE, "%s before wld_load", who);
    if (c->pend.active) return fail(WLD_E_STATE, "%s during a run", who);
    if (!max_side) return fail(WLD_E_ARG, "%s: max_side 0", who);
    WLD_TRY(omega_check_params(who, min_side, eps));
    if (c->L < 2) return fail(WLD_E_ARG, "%s: a split needs two sites; %zu are loaded", who, c->L);
    if (c->L > mbp::kMaxSites)
        return fail(WLD_E_ARG, "%s: %zu loaded sites exceed the %llu that 16-bit tile indices address", who, c->L,
                    (unsigned long long)mbp::kMaxSites);
    if (window_on(c) && c->win_hi_host.size() != c->L) return fail(WLD_E_STATE, "internal: the window has no plan");
    const uint32_t n = (uint32_t)c->L;
    const uint32_t K = mbp::width(n, banded_limits(c));
    mbp::Rows q{};
    // (the destination is the call's own buffer, allocated below)
    WLD_TRY(banded_check(c, who, 0, 0, K, WLD_MATRIX_R2, band_dtype, WLD_MATRIX_ZERO_MISSING, true, (size_t)K + 1, &q));
    const uint64_t total = bop::n_splits(n, n_grid);
    if (total > 0xFFFFFFFFull) return fail(WLD_E_ARG, "%s: too many splits", who);
    const uint32_t G = (uint32_t)total;
    // the results' host arrays double as the splits' staging
    out->position = (uint64_t *)malloc(G * sizeof(uint64_t));
    out->split = (uint32_t *)malloc(G * sizeof(uint32_t));
    out->lo = (uint32_t *)malloc(G * sizeof(uint32_t));
    out->hi = (uint32_t *)malloc(G * sizeof(uint32_t));
    out->omega = (double *)malloc(G * sizeof(double));
    out->left = (uint32_t *)malloc(G * sizeof(uint32_t));
    out->right = (uint32_t *)malloc(G * sizeof(uint32_t));
    out->zns = (double *)malloc(G * sizeof(double));
    // a failed call returns no arrays (the message survives the frees)
    auto refuse = [&](int st) {
        if (st == WLD_OK) return st;
        const std::string msg = wld_last_error();
        wld_omega_free(out);
        return fail(st, "%s", msg.c_str());
    };
    if (!out->position || !out->split || !out->lo || !out->hi || !out->omega || !out->left || !out->right || !out->zns) {
        wld_omega_free(out);
        return fail(WLD_E_OOM, "%s: host allocation of %u splits failed", who, G);
    }
    const uint32_t *pos = c->has_pos ? c->pos_host.data() : nullptr;
    const uint32_t d = bop::first_descent(pos, n);
    if (d < n) return refuse(omega_map_descends(who, d, pos[d], pos[d - 1]));
    bop::splits(pos, n, n_grid, max_side, max_distance, out->position, out->split, out->lo, out->hi);
    // every pair of lo..hi must be in the window: hi[] is non-decreasing, so
    // lo's own limit decides
    const uint32_t *lim = banded_limits(c);
    for (uint32_t g = 0; g < G; ++g) {
        const uint32_t reach = lim ? lim[out->lo[g]] : n - 1;
        if (reach < out->hi[g] || out->hi[g] - out->lo[g] > K) {
            const uint32_t lo = out->lo[g], hi = out->hi[g];
            wld_omega_free(out);
            return fail(WLD_E_ARG, "%s: the context's window drops pairs the scan needs (split %u spans the sites %u..%u, "
                                   "the window ends site %u's partners at %u): max_side %u needs a window of max_sites %llu "
                                   "and no max_distance",
                        who, g, lo, hi, lo, reach, max_side, 2ull * max_side - 1);
        }
    }
    OmegaBufs b;
    const size_t eb = band_dtype == WLD_MATRIX_F16 ? 2 : 4, width = (size_t)K + 1;
    int st = ensure(b.band, (size_t)n * width * eb);
    if (st == WLD_OK) st = ensure(b.sums, (size_t)n * width * sizeof(double));
    if (st == WLD_OK) st = ensure(b.in, (size_t)G * 3 * sizeof(uint32_t));
    if (st == WLD_OK) st = ensure(b.out, (size_t)G * (2 * sizeof(double) + 2 * sizeof(uint32_t)));
    if (st != WLD_OK) return refuse(st);
    out->n_sites = n, out->bandwidth = K, out->n_splits = G, out->min_side = min_side;
    banded_info_init(&out->band, q, K, WLD_MATRIX_R2, band_dtype, WLD_MATRIX_ZERO_MISSING);
    st = banded_strip(c, q, K, WLD_MATRIX_R2, band_dtype, WLD_MATRIX_ZERO_MISSING, b.band.p, width, &out->band);
    if (st == WLD_OK) st = banded_account(c, q, &out->band);
    if (st == WLD_OK) st = pairsum_run(c, b.band.p, band_dtype, width, n, K, ptr<double>(b.sums), width, &out->sums);
    if (st != WLD_OK) return refuse(st);
    uint32_t *d_split = ptr<uint32_t>(b.in), *d_lo = d_split + G, *d_hi = d_lo + G;
    double *d_omega = ptr<double>(b.out), *d_zns = d_omega + G;
    uint32_t *d_left = reinterpret_cast<uint32_t *>(d_zns + G), *d_right = d_left + G;
    auto copy = [&](void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
        if (st != WLD_OK) return;
        const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, c->stream);
        if (e != hipSuccess) st = fail(WLD_E_HIP, "%s copy: %s", who, hipGetErrorString(e));
    };
    copy(d_split, out->split, G * sizeof(uint32_t), hipMemcpyHostToDevice);
    copy(d_lo, out->lo, G * sizeof(uint32_t), hipMemcpyHostToDevice);
    copy(d_hi, out->hi, G * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (st == WLD_OK)
        st = omega_run(c, who, ptr<double>(b.sums), width, n, K, d_split, d_lo, d_hi, G, min_side, eps, d_omega, d_left,
                       d_right, d_zns, &out->scan);
    copy(out->omega, d_omega, G * sizeof(double), hipMemcpyDeviceToHost);
    copy(out->zns, d_zns, G * sizeof(double), hipMemcpyDeviceToHost);
    copy(out->left, d_left, G * sizeof(uint32_t), hipMemcpyDeviceToHost);
    copy(out->right, d_right, G * sizeof(uint32_t), hipMemcpyDeviceToHost);
    // always: a copy enqueued before a failure may still be writing the host arrays refuse() frees
    if (hipStreamSynchronize(c->stream) != hipSuccess && st == WLD_OK) st = fail(WLD_E_HIP, "%s: synchronize failed", who);
    return refuse(st);
}

namespace {
// What wld_run_partners refuses, checked on a loaded single-device context
// (every member of a group holds the same load).
int partners_check(wld_ctx *c, uint32_t k, float thr) {
    if (k == 0) return fail(WLD_E_ARG, "wld_run_partners: k 0");
    if (k > WLD_PARTNERS_MAX_K)
        return fail(WLD_E_ARG, "wld_run_partners: k %u exceeds %u", k, (unsigned)WLD_PARTNERS_MAX_K);
    if (std::isnan(thr)) return fail(WLD_E_ARG, "wld_run_partners: the threshold is NaN");
    if (c->safe)
        return fail(WLD_E_ARG, "wld_run_partners needs finite weights (this load takes the select loop)");
    return WLD_OK;
}

// The per-call events of a best-partner run: three per batch (before the pair
// launch, after it, after the merge), destroyed on every path.
struct PartnerEvents {
    std::vector<hipEvent_t> ev;
    ~PartnerEvents() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// The best partners of the linear chunks [lb, le) on one device (k, thr
// checked): the range's tile list under the window in a buffer of its own —
// the row path's cached list, its range and seg_clear are not touched — cut
// into staging batches; per batch one pair launch and one merge launch; one
// copy back of the running lists.  Touches no staging, segment count, chunk
// total, run counter or row-path event of the row path.
int partners_range(wld_ctx *c, uint32_t k, float thr, uint32_t lb, uint32_t le, partners_plan::Partners *out) {
    WLD_TRY(set_dev(c));
    if (!c->loaded) return fail(WLD_E_STATE, "wld_run_partners before wld_load");
    if (c->pend.active) return fail(WLD_E_STATE, "wld_run_partners during a run");
    const size_t L = c->L, LP = c->LP, TB = LP / kTile;
    const uint32_t kp = std::min<uint32_t>(k, kTile);
    *out = partners_plan::Partners{};
    out->n_sites = (uint32_t)L;
    out->k = k;
    try {
        out->list.assign(L * k, partners_plan::Entry{partners_plan::kNoKey, 0.0f, 0.0f});
    } catch (const std::bad_alloc &) {
        return fail(WLD_E_OOM, "host allocation of the partner lists (%zu sites x %u) failed", L, k);
    }
    if (lb >= le) return WLD_OK;
    const bool windowed = window_on(c);
    if (windowed && c->win_hi_host.size() != L) return fail(WLD_E_STATE, "internal: the window has no plan");
    const uint32_t T_used = (uint32_t)((L + kTile - 1) / kTile), n = chunk_rows_of(L);
    std::vector<uint32_t> t =
        windowed ? window_plan::range_tiles(n, T_used, lb, le, c->win_hi_host) : tile_order::range_tiles(n, T_used, lb, le);
    out->tiles = t.size();
    const uint64_t expect =
        partners_plan::considered_pairs(windowed ? c->win_hi_host.data() : nullptr, (uint32_t)L, lb, le);
    if (t.empty()) {
        if (expect) return fail(WLD_E_HIP, "internal: the partner run's tile list is empty; the range holds %llu pairs",
                                (unsigned long long)expect);
        return WLD_OK;
    }
    if (!c->opt_tile_rows && t.size() >= 4096 && T_used < 65535)
        t = xcd_order(t, tile_order::super_block_side((uint32_t)c->NP));
    WLD_TRY(ensure_ref_layout(c));
    const auto cuts = partners_plan::batches(t.size(), c->opt_partners_bytes, kp);
    uint64_t max_tiles = 0;
    for (const auto &b : cuts) max_tiles = std::max(max_tiles, b.second - b.first);
    if (partners_plan::parts_of(max_tiles) > 0xFFFFFFFFull)
        return fail(WLD_E_ARG, "WLD_OPT_PARTNERS_BATCH_BYTES: a batch of %llu tiles is too large",
                    (unsigned long long)max_tiles);
    // the batches' CSRs, alive until the stream has copied them
    std::vector<partners_plan::Csr> csr;
    size_t max_ent = 0;
    for (const auto &b : cuts) {
        csr.push_back(partners_plan::build_csr(t.data(), b.first, b.second, T_used));
        max_ent = std::max(max_ent, csr.back().ent.size());
    }
    const size_t n_parts_max = (size_t)partners_plan::parts_of(max_tiles);
    const size_t run_bytes = TB * kTile * (size_t)k * sizeof(PartnerEntry), words_bytes = 4 * sizeof(unsigned long long);
    // the staging goes back after the call where it is large
    struct StageRelease {
        wld_ctx *c;
        ~StageRelease() {
            if (c->pt_stage.bytes > (64u << 20)) {
                (void)hipStreamSynchronize(c->stream);
                release(c->pt_stage);
                release(c->pt_cnt);
            }
        }
    } stage_release{c};
    WLD_TRY(ensure(c->pt_tiles, t.size() * sizeof(uint32_t)));
    WLD_TRY(ensure(c->pt_stage, n_parts_max * kp * sizeof(PartnerEntry)));
    WLD_TRY(ensure(c->pt_cnt, n_parts_max * sizeof(uint32_t)));
    WLD_TRY(ensure(c->pt_csr, (T_used + 1 + max_ent) * sizeof(uint32_t)));
    WLD_TRY(ensure(c->pt_run, run_bytes));
    WLD_TRY(ensure(c->pt_words, words_bytes));
    PartnerEvents pe;
    pe.ev.assign(3 * cuts.size(), nullptr);
    for (auto &e : pe.ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipMemcpyAsync(c->pt_tiles.p, t.data(), t.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->pt_run.p, 0, run_bytes, c->stream));
    HIP_TRY(hipMemsetAsync(c->pt_words.p, 0, words_bytes, c->stream));
    unsigned long long *d_cls = ptr<unsigned long long>(c->pt_words);
    unsigned *d_guard = reinterpret_cast<unsigned *>(d_cls + 3);
    OrderArgs o{};  // the window only
    o.L = (uint32_t)L;
    o.T = (uint32_t)TB;
    o.win_hi = windowed ? ptr<uint32_t>(c->win_hi) : nullptr;
    for (size_t bi = 0; bi < cuts.size(); ++bi) {
        const uint64_t b0 = cuts[bi].first, nb = cuts[bi].second - b0;
        const partners_plan::Csr &cs = csr[bi];
        uint32_t *d_off = ptr<uint32_t>(c->pt_csr), *d_ent = d_off + T_used + 1;
        HIP_TRY(hipMemcpyAsync(d_off, cs.off.data(), cs.off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        if (!cs.ent.empty())
            HIP_TRY(hipMemcpyAsync(d_ent, cs.ent.data(), cs.ent.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                   c->stream));
        ValuLaunch v = ref_valu_launch(c, thr);  // (finite weights: partners_check)
        v.tiles = ptr<uint32_t>(c->pt_tiles) + b0;
        v.n_tiles = (uint32_t)nb;
        const PartnersArgs pa{d_cls, ptr<PartnerEntry>(c->pt_stage), ptr<uint32_t>(c->pt_cnt), kp, d_guard};
        const PartnersMerge pm{ptr<PartnerEntry>(c->pt_stage), ptr<uint32_t>(c->pt_cnt), kp, k,
                               (uint32_t)partners_plan::parts_of(nb), d_off, d_ent, (uint32_t)cs.ent.size(), T_used,
                               (uint32_t)L, ptr<PartnerEntry>(c->pt_run), d_guard};
        HIP_TRY(hipEventRecord(pe.ev[3 * bi], c->stream));
        launch_pair_partners(v, o, pa, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(pe.ev[3 * bi + 1], c->stream));
        launch_partners_merge(pm, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(pe.ev[3 * bi + 2], c->stream));
    }
    unsigned long long words[4] = {0, 0, 0, 0};
    static_assert(sizeof(partners_plan::Entry) == sizeof(PartnerEntry), "one entry layout on host and device");
    if (L) HIP_TRY(hipMemcpyAsync(out->list.data(), c->pt_run.p, L * k * sizeof(PartnerEntry), hipMemcpyDeviceToHost,
                                  c->stream));
    HIP_TRY(hipMemcpyAsync(words, c->pt_words.p, words_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (t and the CSRs are read by the copies)
    for (size_t bi = 0; bi < cuts.size(); ++bi) {
        out->kernel_ms += event_ms(pe.ev[3 * bi], pe.ev[3 * bi + 1]);
        out->merge_ms += event_ms(pe.ev[3 * bi + 1], pe.ev[3 * bi + 2]);
    }
    const unsigned guard = (unsigned)(words[3] & 0xFFFFFFFFu);
    if (guard)
        return fail(WLD_E_STATE, "wld_run_partners: a kernel refused an index (guard %u: %s%s%s)", guard,
                    guard & kPartnersGuardTile ? "tile " : "", guard & kPartnersGuardEntry ? "CSR entry " : "",
                    guard & kPartnersGuardPart ? "part count" : "");
    out->pairs = words[0];
    out->none_pairs = words[1];
    out->passing_pairs = words[2];
    // the kernel's own accounting against the host's plan
    uint64_t listed = 0;
    for (const partners_plan::Entry &e : out->list) listed += e.key != partners_plan::kNoKey;
    if (out->pairs != expect || out->none_pairs + out->passing_pairs > out->pairs || listed > 2 * out->passing_pairs)
        return fail(WLD_E_HIP, "internal: partner run counted %llu pairs (%llu none, %llu passing, %llu listed); "
                               "the range holds %llu",
                    (unsigned long long)out->pairs, (unsigned long long)out->none_pairs,
                    (unsigned long long)out->passing_pairs, (unsigned long long)listed, (unsigned long long)expect);
    return WLD_OK;
}

// ... on a device group: member g takes its shard of the chunk sequence (as
// summary_group deals them) cut to [lb, le), on its own host thread; the
// members' results are merged in member order.
int partners_group(wld_ctx *g, uint32_t k, float thr, uint32_t lb, uint32_t le, partners_plan::Partners *out) {
    const int G = (int)g->members.size();
    wld_ctx *c0 = g->members[0];
    std::vector<uint32_t> sb(G), se(G);
    for (int i = 0; i < G; ++i) {  // every range before any thread starts
        if (window_on(c0)) WLD_TRY(wld_shard_chunks_window(c0, G, i, &sb[i], &se[i]));
        else WLD_TRY(wld_shard_chunks(c0->L, G, i, &sb[i], &se[i]));
        sb[i] = std::max(sb[i], lb);
        se[i] = std::max(sb[i], std::min(se[i], le));
    }
    std::vector<partners_plan::Partners> part(G);
    std::vector<int> status(G, WLD_OK);
    std::vector<std::string> msg(G);
    std::vector<std::thread> th;
    for (int i = 0; i < G; ++i)
        th.emplace_back([&, i] {
            status[i] = partners_range(g->members[i], k, thr, sb[i], se[i], &part[i]);
            if (status[i] != WLD_OK) msg[i] = wld_last_error();
        });
    for (auto &t : th) t.join();
    for (int i = 0; i < G; ++i)
        if (status[i] != WLD_OK)
            return fail(status[i], "device %d (shard %d): %s", g->members[i]->device, i, msg[i].c_str());
    *out = partners_plan::Partners{};
    for (int i = 0; i < G; ++i) partners_plan::merge(*out, part[i]);
    return WLD_OK;
}

// lists <-> the caller's arrays
int partners_alloc(wld_partners *out, size_t L, uint32_t k) {
    const size_t n = std::max<size_t>(L * k, 1);
    out->count = (uint32_t *)malloc(std::max<size_t>(L, 1) * sizeof(uint32_t));
    out->partner = (uint32_t *)malloc(n * sizeof(uint32_t));
    out->d = (float *)malloc(n * sizeof(float));
    out->d_prime = (float *)malloc(n * sizeof(float));
    out->r2 = (float *)malloc(n * sizeof(float));
    if (!out->count || !out->partner || !out->d || !out->d_prime || !out->r2) {
        wld_partners_free(out);
        return fail(WLD_E_OOM, "host allocation of the partner lists (%zu sites x %u) failed", L, k);
    }
    return WLD_OK;
}
void partners_store(const partners_plan::Partners &p, wld_partners *out) {
    const size_t L = p.n_sites, k = p.k;
    for (size_t s = 0; s < L; ++s) {
        uint32_t cnt = 0;
        for (size_t i = 0; i < k; ++i) {
            const partners_plan::Entry &e = p.list[s * k + i];
            const bool have = e.key != partners_plan::kNoKey;
            cnt += have;
            out->partner[s * k + i] = have ? partners_plan::key_partner(e.key) : WLD_PARTNERS_NONE;
            out->d[s * k + i] = have ? e.d : std::nanf("");
            out->d_prime[s * k + i] = have ? e.dp : std::nanf("");
            out->r2[s * k + i] = have ? partners_plan::key_r2(e.key) : std::nanf("");
        }
        out->count[s] = cnt;
    }
    out->n_sites = L;
    out->k = (uint32_t)k;
    out->pairs = p.pairs;
    out->none_pairs = p.none_pairs;
    out->passing_pairs = p.passing_pairs;
    out->tiles = p.tiles;
    out->kernel_ms = p.kernel_ms;
    out->merge_ms = p.merge_ms;
}
void partners_fetch(const wld_partners *in, partners_plan::Partners &p) {
    p.n_sites = (uint32_t)in->n_sites;
    p.k = in->k;
    p.pairs = in->pairs;
    p.none_pairs = in->none_pairs;
    p.passing_pairs = in->passing_pairs;
    p.tiles = in->tiles;
    p.kernel_ms = in->kernel_ms;
    p.merge_ms = in->merge_ms;
    const size_t L = in->n_sites, k = in->k;
    p.list.assign(L * k, partners_plan::Entry{partners_plan::kNoKey, 0.0f, 0.0f});
    for (size_t s = 0; s < L; ++s)
        for (size_t i = 0; i < std::min<size_t>(k, in->count[s]); ++i)
            p.list[s * k + i] = partners_plan::Entry{partners_plan::pack_key(in->r2[s * k + i], in->partner[s * k + i]),
                                                     in->d[s * k + i], in->d_prime[s * k + i]};
}
}  // namespace

int wld_run_partners(wld_ctx *c, uint32_t k, float r2_threshold, uint32_t chunk_begin, uint32_t chunk_end,
                     wld_partners *out) {
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    if (!c) return fail(WLD_E_ARG, "null context");
    wld_ctx *c0 = c->members.empty() ? c : c->members[0];
    for (wld_ctx *m : c->members.empty() ? std::vector<wld_ctx *>{c} : c->members) {
        if (!m->loaded) return fail(WLD_E_STATE, "wld_run_partners before wld_load");
        if (m->pend.active) return fail(WLD_E_STATE, "wld_run_partners during a run");
    }
    WLD_TRY(partners_check(c0, k, r2_threshold));
    const uint32_t m = chunks_of(c0->L);
    if (chunk_end == 0 || chunk_end > m) chunk_end = m;
    if (chunk_begin > chunk_end) return fail(WLD_E_ARG, "chunk range [%u,%u) invalid", chunk_begin, chunk_end);
    partners_plan::Partners p;
    if (c->members.empty()) WLD_TRY(partners_range(c, k, r2_threshold, chunk_begin, chunk_end, &p));
    else WLD_TRY(partners_group(c, k, r2_threshold, chunk_begin, chunk_end, &p));
    WLD_TRY(partners_alloc(out, p.n_sites, k));
    partners_store(p, out);
    return WLD_OK;
}

int wld_partners_merge(wld_partners *into, const wld_partners *from) {
    if (!into || !from) return fail(WLD_E_ARG, "wld_partners_merge: null argument");
    if (into->n_sites != from->n_sites || into->k != from->k || !into->k)
        return fail(WLD_E_ARG, "wld_partners_merge: shapes differ (%llu x %u and %llu x %u)",
                    (unsigned long long)into->n_sites, into->k, (unsigned long long)from->n_sites, from->k);
    if (into->n_sites && (!into->count || !into->partner || !into->d || !into->d_prime || !into->r2 || !from->count ||
                          !from->partner || !from->d || !from->d_prime || !from->r2))
        return fail(WLD_E_ARG, "wld_partners_merge: null list");
    try {
        partners_plan::Partners a, b;
        partners_fetch(into, a);
        partners_fetch(from, b);
        partners_plan::merge(a, b);
        partners_store(a, into);
    } catch (const std::bad_alloc &) {
        return fail(WLD_E_OOM, "wld_partners_merge: host allocation failed");
    }
    return WLD_OK;
}

void wld_partners_free(wld_partners *p) {
    if (!p) return;
    free(p->count);
    free(p->partner);
    free(p->d);
    free(p->d_prime);
    free(p->r2);
    memset(p, 0, sizeof(*p));
}

namespace {
// What the LD-block calls refuse, checked on a loaded single-device context
// (every member of a group holds the same load).
int blocks_check_stat(wld_ctx *c, const char *who, int stat, float strong_min) {
    const int a = blocks_plan::check_stat(stat, strong_min);
    if (a == blocks_plan::kArgStat) return fail(WLD_E_ARG, "%s: unknown stat %d", who, stat);
    if (a == blocks_plan::kArgStrongMin) return fail(WLD_E_ARG, "%s: strong_min is not finite", who);
    if (c && c->safe) return fail(WLD_E_ARG, "%s needs finite weights (this load takes the select loop)", who);
    return WLD_OK;
}
int blocks_check_rule(const char *who, int rule, uint32_t min_sites) {
    const int a = blocks_plan::check_rule(rule, min_sites);
    if (a == blocks_plan::kArgRule) return fail(WLD_E_ARG, "%s: unknown rule %d", who, rule);
    if (a == blocks_plan::kArgMinSites) return fail(WLD_E_ARG, "%s: min_sites %u is below 2", who, min_sites);
    return WLD_OK;
}

// the tile list of a blocks pass into the context's own buffer
int blocks_tiles_upload(wld_ctx *c, std::vector<uint32_t> &t, uint32_t T_used) {
    if (!c->opt_tile_rows && t.size() >= 4096 && T_used < 65535)
        t = xcd_order(t, tile_order::super_block_side((uint32_t)c->NP));
    WLD_TRY(ensure(c->blk_tiles, t.size() * sizeof(uint32_t)));
    HIP_TRY(hipMemcpyAsync(c->blk_tiles.p, t.data(), t.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    return WLD_OK;
}

// Pass 1 over the linear chunks [lb, le) on one device (stat, strong_min
// checked): the range's tile list under the window in a buffer of its own —
// the row path's cached list, its range and seg_clear are not touched — the
// break arrays at their neutral values, one launch, one copy back.  Touches
// no staging, segment count, chunk total, run counter or row-path event.
int breaks_range(wld_ctx *c, int stat, float strong_min, uint32_t lb, uint32_t le, blocks_plan::Breaks *out) {
    WLD_TRY(set_dev(c));
    if (!c->loaded) return fail(WLD_E_STATE, "wld_run_block_breaks before wld_load");
    if (c->pend.active) return fail(WLD_E_STATE, "wld_run_block_breaks during a run");
    const size_t L = c->L, LP = c->LP, TB = LP / kTile;
    const bool windowed = window_on(c);
    if (windowed && c->win_hi_host.size() != L) return fail(WLD_E_STATE, "internal: the window has no plan");
    *out = blocks_plan::Breaks{};
    out->n_sites = (uint32_t)L;
    out->stat = stat;
    out->strong_min = strong_min;
    try {
        out->fwd.assign(L, blocks_plan::kNone);
        out->bwd.assign(L, blocks_plan::kNone);
        out->last.assign(L, L ? (uint32_t)(L - 1) : 0u);
    } catch (const std::bad_alloc &) {
        return fail(WLD_E_OOM, "host allocation of the break arrays (%zu sites) failed", L);
    }
    if (windowed)
        for (size_t i = 0; i < L; ++i) out->last[i] = std::min<uint32_t>(c->win_hi_host[i], (uint32_t)(L - 1));
    if (lb >= le) return WLD_OK;
    const uint32_t T_used = (uint32_t)((L + kTile - 1) / kTile), n = chunk_rows_of(L);
    std::vector<uint32_t> t =
        windowed ? window_plan::range_tiles(n, T_used, lb, le, c->win_hi_host) : tile_order::range_tiles(n, T_used, lb, le);
    out->tiles = t.size();
    const uint64_t expect = run_pairs(c, lb, le);
    if (t.empty()) {
        if (expect) return fail(WLD_E_HIP, "internal: the break run's tile list is empty; the range holds %llu pairs",
                                (unsigned long long)expect);
        return WLD_OK;
    }
    WLD_TRY(ensure_ref_layout(c));
    for (auto &e : c->ev_blk)
        if (!e) HIP_TRY(hipEventCreate(&e));
    // {classes[8]} u64 | fwd[LP] u32 (all ones) | bwd + 1 [LP] u32 (zero)
    const size_t bytes = 8 * 8 + 4 * LP + 4 * LP;
    WLD_TRY(ensure(c->blk_brk, bytes));
    WLD_TRY(blocks_tiles_upload(c, t, T_used));
    unsigned long long *d_cls = ptr<unsigned long long>(c->blk_brk);
    uint32_t *d_fwd = reinterpret_cast<uint32_t *>(d_cls + 8), *d_bwd1 = d_fwd + LP;
    HIP_TRY(hipMemsetAsync(c->blk_brk.p, 0, bytes, c->stream));
    HIP_TRY(hipMemsetAsync(d_fwd, 0xFF, 4 * LP, c->stream));
    const BlockBreakArgs ba{d_cls, d_fwd, d_bwd1, stat, strong_min};
    ValuLaunch v = ref_valu_launch(c, 0.0f);  // (finite weights: blocks_check_stat)
    v.tiles = ptr<uint32_t>(c->blk_tiles);
    v.n_tiles = (uint32_t)t.size();
    OrderArgs o{};  // the window only
    o.L = (uint32_t)L;
    o.T = (uint32_t)TB;
    o.win_hi = windowed ? ptr<uint32_t>(c->win_hi) : nullptr;
    HIP_TRY(hipEventRecord(c->ev_blk[0], c->stream));
    launch_pair_block_breaks(v, o, ba, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_blk[1], c->stream));
    uint64_t cls[8] = {};
    std::vector<uint32_t> bwd1(L);
    HIP_TRY(hipMemcpyAsync(cls, d_cls, sizeof(cls), hipMemcpyDeviceToHost, c->stream));
    if (L) {
        HIP_TRY(hipMemcpyAsync(out->fwd.data(), d_fwd, 4 * L, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(bwd1.data(), d_bwd1, 4 * L, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));  // (t is read by the copy)
    out->kernel_ms = event_ms(c->ev_blk[0], c->ev_blk[1]);
    for (size_t i = 0; i < L; ++i) out->bwd[i] = bwd1[i] ? bwd1[i] - 1 : blocks_plan::kNone;
    out->pairs = cls[0];
    out->none_pairs = cls[1];
    out->nonfinite_pairs = cls[2];
    out->strong_pairs = cls[3];
    out->weak_pairs = cls[4];
    // the kernel's own accounting against the host's plan
    if (out->pairs != expect ||
        out->pairs != out->none_pairs + out->nonfinite_pairs + out->strong_pairs + out->weak_pairs)
        return fail(WLD_E_HIP, "internal: break run counted %llu pairs (%llu none, %llu nonfinite, %llu strong, "
                               "%llu weak); the range holds %llu",
                    (unsigned long long)out->pairs, (unsigned long long)out->none_pairs,
                    (unsigned long long)out->nonfinite_pairs, (unsigned long long)out->strong_pairs,
                    (unsigned long long)out->weak_pairs, (unsigned long long)expect);
    return WLD_OK;
}

// ... on a device group: member k takes its shard of the chunk sequence (as
// summary_group deals them) cut to [lb, le), on its own host thread; the
// members' breaks are merged in member order.
int breaks_group(wld_ctx *g, int stat, float strong_min, uint32_t lb, uint32_t le, blocks_plan::Breaks *out) {
    const int G = (int)g->members.size();
    wld_ctx *c0 = g->members[0];
    std::vector<uint32_t> sb(G), se(G);
    for (int k = 0; k < G; ++k) {  // every range before any thread starts
        if (window_on(c0)) WLD_TRY(wld_shard_chunks_window(c0, G, k, &sb[k], &se[k]));
        else WLD_TRY(wld_shard_chunks(c0->L, G, k, &sb[k], &se[k]));
        sb[k] = std::max(sb[k], lb);
        se[k] = std::max(sb[k], std::min(se[k], le));
    }
    std::vector<blocks_plan::Breaks> part(G);
    std::vector<int> status(G, WLD_OK);
    std::vector<std::string> msg(G);
    std::vector<std::thread> th;
    for (int k = 0; k < G; ++k)
        th.emplace_back([&, k] {
            status[k] = breaks_range(g->members[k], stat, strong_min, sb[k], se[k], &part[k]);
            if (status[k] != WLD_OK) msg[k] = wld_last_error();
        });
    for (auto &t : th) t.join();
    for (int k = 0; k < G; ++k)
        if (status[k] != WLD_OK)
            return fail(status[k], "device %d (shard %d): %s", g->members[k]->device, k, msg[k].c_str());
    *out = blocks_plan::Breaks{};
    for (int k = 0; k < G; ++k) blocks_plan::merge(*out, part[k]);
    return WLD_OK;
}

int breaks_run(wld_ctx *c, const char *who, int stat, float strong_min, uint32_t chunk_begin, uint32_t chunk_end,
               blocks_plan::Breaks *b) {
    if (!c) return fail(WLD_E_ARG, "null context");
    wld_ctx *c0 = c->members.empty() ? c : c->members[0];
    for (wld_ctx *m : c->members.empty() ? std::vector<wld_ctx *>{c} : c->members) {
        if (!m->loaded) return fail(WLD_E_STATE, "%s before wld_load", who);
        if (m->pend.active) return fail(WLD_E_STATE, "%s during a run", who);
    }
    WLD_TRY(blocks_check_stat(c0, who, stat, strong_min));
    const uint32_t m = chunks_of(c0->L);
    if (chunk_end == 0 || chunk_end > m) chunk_end = m;
    if (chunk_begin > chunk_end) return fail(WLD_E_ARG, "chunk range [%u,%u) invalid", chunk_begin, chunk_end);
    if (c->members.empty()) return breaks_range(c, stat, strong_min, chunk_begin, chunk_end, b);
    return breaks_group(c, stat, strong_min, chunk_begin, chunk_end, b);
}

int breaks_store(const blocks_plan::Breaks &b, wld_block_breaks *out) {
    const size_t L = b.n_sites, n = std::max<size_t>(L, 1) * sizeof(uint32_t);
    out->fwd_weak = (uint32_t *)malloc(n);
    out->bwd_weak = (uint32_t *)malloc(n);
    out->last = (uint32_t *)malloc(n);
    if (!out->fwd_weak || !out->bwd_weak || !out->last) {
        wld_block_breaks_free(out);
        return fail(WLD_E_OOM, "host allocation of the break arrays (%zu sites) failed", L);
    }
    std::copy(b.fwd.begin(), b.fwd.end(), out->fwd_weak);
    std::copy(b.bwd.begin(), b.bwd.end(), out->bwd_weak);
    std::copy(b.last.begin(), b.last.end(), out->last);
    out->n_sites = L;
    out->stat = b.stat;
    out->strong_min = b.strong_min;
    out->pairs = b.pairs;
    out->none_pairs = b.none_pairs;
    out->nonfinite_pairs = b.nonfinite_pairs;
    out->strong_pairs = b.strong_pairs;
    out->weak_pairs = b.weak_pairs;
    out->tiles = b.tiles;
    out->kernel_ms = b.kernel_ms;
    return WLD_OK;
}

// a breaks result a call can read: arrays present, every index in its place
int breaks_arrays_check(const char *who, const wld_block_breaks *b) {
    if (!b) return fail(WLD_E_ARG, "%s: null breaks", who);
    if (b->n_sites > 0xFFFFFFFEull)
        return fail(WLD_E_ARG, "%s: breaks of %llu sites", who, (unsigned long long)b->n_sites);
    if (b->n_sites && (!b->fwd_weak || !b->bwd_weak || !b->last)) return fail(WLD_E_ARG, "%s: null break array", who);
    for (uint64_t i = 0; i < b->n_sites; ++i) {
        const uint32_t f = b->fwd_weak[i], w = b->bwd_weak[i], l = b->last[i];
        if ((f != WLD_BLOCKS_NONE && (f >= b->n_sites || f <= i)) || (w != WLD_BLOCKS_NONE && w >= i) ||
            l >= b->n_sites || l < i)
            return fail(WLD_E_ARG, "%s: the break arrays hold an index out of place at site %llu", who,
                        (unsigned long long)i);
    }
    return WLD_OK;
}

// the partition of a breaks result into out (statistics NULL)
int blocks_partition_into(const char *who, const wld_block_breaks *b, int rule, uint32_t min_sites,
                          blocks_plan::Partition *p, wld_blocks *out) {
    WLD_TRY(breaks_arrays_check(who, b));
    WLD_TRY(blocks_check_stat(nullptr, who, b->stat, b->strong_min));
    WLD_TRY(blocks_check_rule(who, rule, min_sites));
    const uint32_t n = (uint32_t)b->n_sites;
    try {
        *p = blocks_plan::partition(b->fwd_weak, b->bwd_weak, b->last, n, rule, min_sites);
    } catch (const std::bad_alloc &) {
        return fail(WLD_E_OOM, "%s: host allocation of the partition (%u sites) failed", who, n);
    }
    const size_t nb = p->first.size();
    out->first = (uint32_t *)malloc(std::max<size_t>(nb, 1) * sizeof(uint32_t));
    out->last = (uint32_t *)malloc(std::max<size_t>(nb, 1) * sizeof(uint32_t));
    out->site_block = (int32_t *)malloc(std::max<size_t>(n, 1) * sizeof(int32_t));
    if (!out->first || !out->last || !out->site_block) {
        wld_blocks_free(out);
        return fail(WLD_E_OOM, "%s: host allocation of the blocks (%zu blocks, %u sites) failed", who, nb, n);
    }
    std::copy(p->first.begin(), p->first.end(), out->first);
    std::copy(p->last.begin(), p->last.end(), out->last);
    std::copy(p->site_block.begin(), p->site_block.end(), out->site_block);
    out->n_sites = n;
    out->n_blocks = (uint32_t)nb;
    out->stat = b->stat;
    out->rule = rule;
    out->strong_min = b->strong_min;
    out->min_sites = min_sites;
    return WLD_OK;
}

// Pass 2 on one device: the statistics of partition p's blocks under stat /
// strong_min, over the tiles the blocks touch (a list of its own), zeroed
// accumulators, one launch, one copy back.  Fills out's statistics.
int blocks_stats(wld_ctx *c, const blocks_plan::Partition &p, int stat, float strong_min, wld_blocks *out) {
    WLD_TRY(set_dev(c));
    const size_t L = c->L, LP = c->LP, TB = LP / kTile, nb = p.first.size();
    const size_t na = std::max<size_t>(nb, 1);
    out->pairs = (uint64_t *)calloc(na, sizeof(uint64_t));
    out->informative = (uint64_t *)calloc(na, sizeof(uint64_t));
    out->strong = (uint64_t *)calloc(na, sizeof(uint64_t));
    out->value_sum = (double *)calloc(na, sizeof(double));
    out->value_min = (float *)calloc(na, sizeof(float));
    if (!out->pairs || !out->informative || !out->strong || !out->value_sum || !out->value_min)
        return fail(WLD_E_OOM, "host allocation of the block statistics (%zu blocks) failed", nb);
    if (!nb) return WLD_OK;
    const bool windowed = window_on(c);
    if (windowed && c->win_hi_host.size() != L) return fail(WLD_E_STATE, "internal: the window has no plan");
    const uint32_t T_used = (uint32_t)((L + kTile - 1) / kTile);
    std::vector<uint32_t> t = blocks_plan::stats_tiles(p);
    out->tiles = t.size();
    const heatmap_plan::Blocks lim = blocks_plan::id_limits(p, (uint32_t)TB);
    for (size_t b = 0; b < TB; ++b)
        if (lim.lo[b] <= lim.hi[b] && (uint32_t)(lim.hi[b] - lim.lo[b]) >= blocks_plan::kTableIds)
            return fail(WLD_E_STATE, "internal: 64-site block %zu holds block ids %d..%d", b, lim.lo[b], lim.hi[b]);
    WLD_TRY(ensure_ref_layout(c));
    for (auto &e : c->ev_blk)
        if (!e) HIP_TRY(hipEventCreate(&e));
    // {sum[nb]} f64 | {pairs, informative, strong}[nb] u64 | min_key[nb] u32: one memset
    const size_t bytes = 8 * nb + 3 * 8 * nb + 4 * nb;
    WLD_TRY(ensure(c->blk_acc, bytes));
    WLD_TRY(ensure(c->blk_map, (LP + 2 * TB) * sizeof(int32_t)));
    WLD_TRY(blocks_tiles_upload(c, t, T_used));
    std::vector<int32_t> map(LP + 2 * TB, -1);  // site_block[LP] (-1 past L), blk_lo[TB], blk_hi[TB]
    std::copy(p.site_block.begin(), p.site_block.end(), map.begin());
    std::copy(lim.lo.begin(), lim.lo.end(), map.begin() + LP);
    std::copy(lim.hi.begin(), lim.hi.end(), map.begin() + LP + TB);
    HIP_TRY(hipMemcpyAsync(c->blk_map.p, map.data(), map.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->blk_acc.p, 0, bytes, c->stream));
    double *d_sum = ptr<double>(c->blk_acc);
    unsigned long long *d_pairs = reinterpret_cast<unsigned long long *>(d_sum + nb);
    uint32_t *d_key = reinterpret_cast<uint32_t *>(d_pairs + 3 * nb);
    const int32_t *d_map = ptr<int32_t>(c->blk_map);
    const BlockStatsArgs sa{d_pairs, d_pairs + nb, d_pairs + 2 * nb, d_sum, d_key, d_map, d_map + LP, d_map + LP + TB,
                            (uint32_t)nb, stat, strong_min};
    ValuLaunch v = ref_valu_launch(c, 0.0f);
    v.tiles = ptr<uint32_t>(c->blk_tiles);
    v.n_tiles = (uint32_t)t.size();
    OrderArgs o{};  // the window only
    o.L = (uint32_t)L;
    o.T = (uint32_t)TB;
    o.win_hi = windowed ? ptr<uint32_t>(c->win_hi) : nullptr;
    HIP_TRY(hipEventRecord(c->ev_blk[2], c->stream));
    launch_pair_block_stats(v, o, sa, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_blk[3], c->stream));
    std::vector<uint32_t> key(nb);
    HIP_TRY(hipMemcpyAsync(out->value_sum, d_sum, 8 * nb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out->pairs, d_pairs, 8 * nb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out->informative, d_pairs + nb, 8 * nb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out->strong, d_pairs + 2 * nb, 8 * nb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(key.data(), d_key, 4 * nb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (map and t are read by the copies)
    out->kernel_ms = event_ms(c->ev_blk[2], c->ev_blk[3]);
    uint64_t counted = 0;
    for (size_t k = 0; k < nb; ++k) {
        counted += out->pairs[k];
        out->value_min[k] = out->informative[k] ? blocks_plan::inv_key_float(key[k]) : std::nanf("");
    }
    // the kernel's own accounting against the host's plan, where every pair
    // of every block is in the current window (breaks of this window: always)
    bool in_window = true;
    for (size_t k = 0; k < nb && windowed; ++k) in_window &= p.last[k] <= c->win_hi_host[p.first[k]];
    const uint64_t expect = blocks_plan::block_pairs(p);
    if (in_window && counted != expect)
        return fail(WLD_E_HIP, "internal: block statistics counted %llu pairs; the blocks hold %llu",
                    (unsigned long long)counted, (unsigned long long)expect);
    return WLD_OK;
}

// partition + pass 2 of breaks b on the loaded set (a group: member 0)
int blocks_from_breaks(wld_ctx *c, const char *who, const wld_block_breaks *b, int rule, uint32_t min_sites,
                       wld_blocks *out) {
    if (!c) return fail(WLD_E_ARG, "null context");
    wld_ctx *c0 = c->members.empty() ? c : c->members[0];
    for (wld_ctx *m : c->members.empty() ? std::vector<wld_ctx *>{c} : c->members) {
        if (!m->loaded) return fail(WLD_E_STATE, "%s before wld_load", who);
        if (m->pend.active) return fail(WLD_E_STATE, "%s during a run", who);
    }
    if (!b) return fail(WLD_E_ARG, "%s: null breaks", who);
    WLD_TRY(blocks_check_stat(c0, who, b->stat, b->strong_min));
    WLD_TRY(blocks_check_rule(who, rule, min_sites));
    if (b->n_sites != c0->L)
        return fail(WLD_E_ARG, "%s: the breaks cover %llu sites, the loaded set has %zu", who,
                    (unsigned long long)b->n_sites, c0->L);
    blocks_plan::Partition p;
    WLD_TRY(blocks_partition_into(who, b, rule, min_sites, &p, out));
    const int st = blocks_stats(c0, p, b->stat, b->strong_min, out);
    if (st != WLD_OK) wld_blocks_free(out);
    return st;
}
}  // namespace

int wld_run_block_breaks(wld_ctx *c, int stat, float strong_min, uint32_t chunk_begin, uint32_t chunk_end,
                         wld_block_breaks *out) {
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    blocks_plan::Breaks b;
    WLD_TRY(breaks_run(c, "wld_run_block_breaks", stat, strong_min, chunk_begin, chunk_end, &b));
    return breaks_store(b, out);
}

int wld_block_breaks_merge(wld_block_breaks *into, const wld_block_breaks *from) {
    WLD_TRY(breaks_arrays_check("wld_block_breaks_merge", into));
    WLD_TRY(breaks_arrays_check("wld_block_breaks_merge", from));
    if (!blocks_plan::mergeable(into->n_sites, into->stat, into->strong_min, into->last, from->n_sites, from->stat,
                                from->strong_min, from->last))
        return fail(WLD_E_ARG, "wld_block_breaks_merge: the results differ in n_sites, stat, strong_min or last");
    blocks_plan::merge_arrays(into->fwd_weak, into->bwd_weak, from->fwd_weak, from->bwd_weak, into->n_sites);
    into->pairs += from->pairs;
    into->none_pairs += from->none_pairs;
    into->nonfinite_pairs += from->nonfinite_pairs;
    into->strong_pairs += from->strong_pairs;
    into->weak_pairs += from->weak_pairs;
    into->tiles += from->tiles;
    into->kernel_ms = std::max(into->kernel_ms, from->kernel_ms);
    return WLD_OK;
}

void wld_block_breaks_free(wld_block_breaks *b) {
    if (!b) return;
    free(b->fwd_weak);
    free(b->bwd_weak);
    free(b->last);
    memset(b, 0, sizeof(*b));
}

int wld_blocks_partition(const wld_block_breaks *breaks, int rule, uint32_t min_sites, wld_blocks *out) {
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    blocks_plan::Partition p;
    return blocks_partition_into("wld_blocks_partition", breaks, rule, min_sites, &p, out);
}

int wld_blocks_from_breaks(wld_ctx *c, const wld_block_breaks *breaks, int rule, uint32_t min_sites, wld_blocks *out) {
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    return blocks_from_breaks(c, "wld_blocks_from_breaks", breaks, rule, min_sites, out);
}

int wld_run_blocks(wld_ctx *c, int stat, float strong_min, int rule, uint32_t min_sites, wld_blocks *out) {
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    WLD_TRY(blocks_check_rule("wld_run_blocks", rule, min_sites));  // (before pass 1 runs)
    blocks_plan::Breaks b;
    WLD_TRY(breaks_run(c, "wld_run_blocks", stat, strong_min, 0, 0, &b));
    wld_block_breaks view{};  // (the plan's vectors, not owned)
    view.n_sites = b.n_sites;
    view.stat = b.stat;
    view.strong_min = b.strong_min;
    view.fwd_weak = b.fwd.data();
    view.bwd_weak = b.bwd.data();
    view.last = b.last.data();
    WLD_TRY(blocks_from_breaks(c, "wld_run_blocks", &view, rule, min_sites, out));
    out->break_pairs = b.pairs;
    out->break_none_pairs = b.none_pairs;
    out->break_nonfinite_pairs = b.nonfinite_pairs;
    out->break_strong_pairs = b.strong_pairs;
    out->break_weak_pairs = b.weak_pairs;
    out->break_tiles = b.tiles;
    out->break_kernel_ms = b.kernel_ms;
    return WLD_OK;
}

void wld_blocks_free(wld_blocks *b) {
    if (!b) return;
    free(b->first);
    free(b->last);
    free(b->site_block);
    free(b->pairs);
    free(b->informative);
    free(b->strong);
    free(b->value_sum);
    free(b->value_min);
    memset(b, 0, sizeof(*b));
}

namespace {
// The device buffers of one wld_run_prune call, released when it returns on
// every path: after WLD_E_OOM the context holds nothing of the call.
struct PruneBufs {
    DevBuf ea, eb, rank, off, cur, hp, state, words, keep, tag;
    ~PruneBufs() {
        for (DevBuf *b : {&ea, &eb, &rank, &off, &cur, &hp, &state, &words, &keep, &tag}) release(*b);
    }
};

// Room for `need` edges in ea/eb, the first `have` kept (device to device).
int grow_edges(wld_ctx *c, PruneBufs &pb, uint64_t &cap, uint64_t have, uint64_t need) {
    if (need <= cap) return WLD_OK;
    const uint64_t k = std::min<uint64_t>(std::max<uint64_t>(need, 2 * cap), prune_plan::kMaxEdges);
    for (DevBuf *b : {&pb.ea, &pb.eb}) {
        DevBuf nb;
        WLD_TRY(ensure(nb, k * 4));
        hipError_t e = hipSuccess;
        if (have) e = hipMemcpyAsync(nb.p, b->p, have * 4, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            release(nb);
            return fail(WLD_E_HIP, "wld_run_prune: edge buffer copy: %s", hipGetErrorString(e));
        }
        release(*b);
        *b = nb;
    }
    cap = k;
    return WLD_OK;
}

// launches per read of the undecided count (wld_run_prune's host loop)
constexpr uint32_t kPruneRoundsPerRead = 8;
}  // namespace

int wld_run_prune(wld_ctx *c, float r2_threshold, const float *priority, wld_prune *out) {
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    WLD_TRY(set_dev(c));
    if (!c->loaded) return fail(WLD_E_STATE, "wld_run_prune before wld_load");
    if (c->pend.active) return fail(WLD_E_STATE, "wld_run_prune during a run");
    const size_t L = c->L;
    if (priority) {
        const size_t i = prune_plan::first_nan(priority, L);
        if (i < L) return fail(WLD_E_ARG, "wld_run_prune: priority[%zu] is NaN", i);
    }
    const std::vector<uint32_t> rank = prune_plan::rank_of(priority, L);

    // The edges: the rows of the chunk sequence at this threshold and window,
    // in run_host_range's batches, their (a, b) gathered as loaded indices and
    // appended device to device.  Whatever happens, the row path is handed
    // back without rows (wld_rows_* must not give out loaded indices) and with
    // no gather queued behind its next scan.
    PruneBufs pb;
    uint64_t cap = 0, m = 0;
    double pair_ms = 0.0;
    struct Restore {
        wld_ctx *c;
        ~Restore() {
            c->prune_run = false;
            c->have_rows = false;
            c->spec_gather = false;
        }
    } restore{c};
    c->prune_run = true;
    const uint64_t limit = std::max<uint64_t>(1, c->opt_host_batch_pairs);
    const uint32_t le = chunks_of(L);
    for (uint32_t b = 0; b < le;) {
        uint32_t e = b;
        uint64_t pairs = 0;
        while (e < le) {
            const uint64_t p1 = run_pairs(c, e, e + 1);  // (in-window pairs under a window)
            if (e > b && pairs + p1 > limit) break;
            pairs += p1;
            ++e;
        }
        uint64_t rows = 0;
        WLD_TRY(run_chunks(c, r2_threshold, b, e, &rows));
        materialize_times(c);
        pair_ms += std::max(0.0, c->stats.pair_kernel_ms) + std::max(0.0, c->stats.order_ms);
        if (m + rows > prune_plan::kMaxEdges)
            return fail(WLD_E_ARG, "wld_run_prune: more than %llu edges (rows with r2 > %g in the window): raise the "
                                   "threshold or narrow the window",
                        (unsigned long long)prune_plan::kMaxEdges, (double)r2_threshold);
        if (rows) {
            WLD_TRY(grow_edges(c, pb, cap, m, m + rows));
            HIP_TRY(hipMemcpyAsync(ptr<uint32_t>(pb.ea) + m, c->out_a.p, rows * 4, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(ptr<uint32_t>(pb.eb) + m, c->out_b.p, rows * 4, hipMemcpyDeviceToDevice, c->stream));
        }
        m += rows;
        b = e;
    }
    c->pr_ms[0] = c->pr_ms[1] = c->pr_ms[2] = 0.0;
    out->keep = (uint8_t *)malloc(std::max<size_t>(L, 1));
    out->tag = (uint32_t *)malloc(std::max<size_t>(L, 1) * sizeof(uint32_t));
    if (!out->keep || !out->tag) {
        wld_prune_free(out);
        return fail(WLD_E_OOM, "host allocation of the pruned set (%zu sites) failed", L);
    }
    out->n_sites = L;
    out->edges = m;
    out->pair_ms = pair_ms;
    if (m == 0) {  // no edge: every site is kept, no launch
        for (size_t i = 0; i < L; ++i) {
            out->keep[i] = 1;
            out->tag[i] = (uint32_t)i;
        }
        out->n_kept = L;
        return WLD_OK;
    }

    // CSR, rounds, tags.  words: {guard, n_kept, the undecided counts of a
    // group of launches}
    const uint32_t R = kPruneRoundsPerRead;
    unsigned h_words[2 + kPruneRoundsPerRead];
    int st = WLD_OK;
    auto run = [&]() -> int {
        WLD_TRY(ensure(pb.rank, L * 4));
        WLD_TRY(ensure(pb.off, (L + 1) * 4));
        WLD_TRY(ensure(pb.cur, L * 4));
        WLD_TRY(ensure(pb.hp, m * 4));
        WLD_TRY(ensure(pb.state, L * 4));
        WLD_TRY(ensure(pb.words, sizeof h_words));
        WLD_TRY(ensure(pb.keep, L));
        WLD_TRY(ensure(pb.tag, L * 4));
        for (auto &e : c->ev_pr)
            if (!e) HIP_TRY(hipEventCreate(&e));
        unsigned *words = ptr<unsigned>(pb.words);
        const PruneArgs p{ptr<uint32_t>(pb.ea), ptr<uint32_t>(pb.eb), (uint32_t)m, (uint32_t)L, ptr<uint32_t>(pb.rank),
                          ptr<uint32_t>(pb.off), ptr<uint32_t>(pb.cur), ptr<uint32_t>(pb.hp), ptr<uint32_t>(pb.state),
                          words, words + 1, ptr<uint8_t>(pb.keep), ptr<uint32_t>(pb.tag)};
        HIP_TRY(hipMemcpyAsync(pb.rank.p, rank.data(), L * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(pb.off.p, 0, (L + 1) * 4, c->stream));
        HIP_TRY(hipMemsetAsync(pb.state.p, 0, L * 4, c->stream));  // (kUndecided)
        HIP_TRY(hipMemsetAsync(pb.words.p, 0, sizeof h_words, c->stream));
        HIP_TRY(hipEventRecord(c->ev_pr[0], c->stream));
        launch_prune_csr(p, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev_pr[1], c->stream));
        // Rounds: R launches, then one read of the last one's undecided count
        // (a launch that finds its predecessor's at 0 returns at once).  Every
        // launch decides at least the best-ranked undecided vertex, so L
        // launches always suffice.
        uint32_t rounds = 0;
        for (;;) {
            if (rounds) HIP_TRY(hipMemsetAsync(words + 2, 0, R * sizeof(unsigned), c->stream));
            for (uint32_t k = 0; k < R; ++k) launch_prune_decide(p, k ? words + 2 + k - 1 : nullptr, words + 2 + k, c->stream);
            rounds += R;
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h_words, words, sizeof h_words, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (h_words[0]) break;  // (reported below)
            if (h_words[2 + R - 1] == 0) break;
            if ((uint64_t)rounds >= (uint64_t)L + R)
                return fail(WLD_E_HIP, "internal: %u vertices undecided after %u rounds on %zu sites",
                            h_words[2 + R - 1], rounds, L);
        }
        HIP_TRY(hipEventRecord(c->ev_pr[2], c->stream));
        if (!h_words[0]) {
            launch_prune_tags(p, c->stream);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(c->ev_pr[3], c->stream));
        HIP_TRY(hipMemcpyAsync(out->keep, pb.keep.p, L, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(out->tag, pb.tag.p, L * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(h_words, words, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (h_words[0])
            return fail(WLD_E_STATE, "internal: the prune kernels refused an out-of-range index (guard 0x%x: %s%s%s%s)",
                        h_words[0], h_words[0] & kPruneGuardEdge ? "edge endpoint " : "",
                        h_words[0] & kPruneGuardFill ? "list cursor " : "", h_words[0] & kPruneGuardList ? "list entry " : "",
                        h_words[0] & kPruneGuardTag ? "tag" : "");
        out->rounds = rounds;
        out->n_kept = h_words[1];
        for (int k = 0; k < 3; ++k) c->pr_ms[k] = event_ms(c->ev_pr[k], c->ev_pr[k + 1]);
        out->prune_ms = event_ms(c->ev_pr[0], c->ev_pr[3]);
        return WLD_OK;
    };
    st = run();
    if (st != WLD_OK) {
        (void)hipStreamSynchronize(c->stream);  // nothing of the call is in flight when its buffers go
        wld_prune_free(out);
    }
    return st;
}

void wld_prune_free(wld_prune *p) {
    if (!p) return;
    free(p->keep);
    free(p->tag);
    memset(p, 0, sizeof(*p));
}

size_t wld_loaded_sites(const wld_ctx *c) {
    if (!c) return 0;
    const wld_ctx *m = c->members.empty() ? c : c->members[0];
    return m->loaded ? m->L : 0;
}

int wld_prune_times(wld_ctx *c, double *csr_ms, double *rounds_ms, double *tags_ms) {
    if (!c) return fail(WLD_E_ARG, "null context");
    if (!c->members.empty()) return fail(WLD_E_STATE, "wld_prune_times needs a single-device context");
    if (csr_ms) *csr_ms = c->pr_ms[0];
    if (rounds_ms) *rounds_ms = c->pr_ms[1];
    if (tags_ms) *tags_ms = c->pr_ms[2];
    return WLD_OK;
}

namespace {
// the rows of one batch on the host, in (slot, partner) order
struct TargetCols {
    std::vector<uint32_t> t, st, sp;
    std::vector<float> d, dp, r2;
};

// wld_run_targets past its argument checks.  Per batch of the plan: the lists
// up, masks zeroed, the pair launch (pair_targets.hip) between the call's two
// events, the counts and their scans, one read of the slots' bases (the
// batch's exact row total, before its row buffers are sized), the row launch,
// the rows down.  Every slot's rows are one run of its batch's arrays; the
// list order is put together on the host once every batch has been counted.
// Uses the context's stream, the lane-class layout and the window's limits;
// touches no tile list, staging, counter, row or event of the row path.
int run_targets(wld_ctx *c, const uint32_t *targets, uint32_t n, float thr, wld_target_rows *out) {
    const uint32_t L = (uint32_t)c->L, LP = (uint32_t)c->LP, T = LP / kTile;
    const std::vector<uint32_t> no_window;
    const bool windowed = window_on(c) && c->win_hi_host.size() == L;
    const targets_plan::Plan p =
        targets_plan::make(targets, n, L, LP, windowed ? c->win_hi_host : no_window, c->opt_target_slots);
    out->items = p.items();
    out->batches = p.batches();
    if (!p.items()) return WLD_OK;  // (a single site, or a window that leaves no partner)
    WLD_TRY(ensure_ref_layout(c));
    for (auto &e : c->ev_tg)
        if (!e) HIP_TRY(hipEventCreate(&e));
    wld_ctx::TargetBufs &tb = c->tg;
    const size_t n_slots_all = p.slot_site.size();
    std::vector<TargetCols> cols(p.batches());
    std::vector<uint64_t> slot_begin(n_slots_all, 0), slot_rows(n_slots_all, 0);  // within the slot's batch
    std::vector<uint32_t> base;
    double ms = 0.0;
    for (uint32_t k = 0; k < p.batches(); ++k) {
        const uint32_t b0 = p.batch_begin[k], nb = p.batch_begin[k + 1] - b0;
        const size_t ns = (size_t)nb * targets_plan::kBlock;
        const std::vector<uint32_t> items = targets_plan::batch_items(p, b0, b0 + nb);
        const uint32_t n_items = (uint32_t)(items.size() / 2);
        if (!n_items) continue;
        WLD_TRY(ensure(tb.slot_site, ns * 4));
        WLD_TRY(ensure(tb.slot_pos, ns * 4));
        WLD_TRY(ensure(tb.items, items.size() * 4));
        WLD_TRY(ensure(tb.d, ns * LP * 4));
        WLD_TRY(ensure(tb.dp, ns * LP * 4));
        WLD_TRY(ensure(tb.r2, ns * LP * 4));
        WLD_TRY(ensure(tb.mask, ns * T * 8));
        WLD_TRY(ensure(tb.tile_pref, ns * T * 4));
        WLD_TRY(ensure(tb.slot_cnt, ns * 4));
        WLD_TRY(ensure(tb.slot_base, (ns + 1) * 4));
        WLD_TRY(ensure(tb.guard, 16));
        TargetsLaunch t{};
        t.rcodes = ptr<uint8_t>(c->rcodes);
        t.rw = ptr<float>(c->rw);
        t.site_ok = ptr<uint8_t>(c->site_ok);
        t.win_hi = windowed ? ptr<uint32_t>(c->win_hi) : nullptr;
        t.site_map = c->has_map ? ptr<uint32_t>(c->site_map) : nullptr;
        t.L = L;
        t.LP = LP;
        t.NPr = (uint32_t)c->NPr;
        t.ref_cs = c->ref_cls / 64;
        t.ref_tail_n = (uint32_t)(c->N % 8);
        t.thr = thr;
        t.n_blocks = nb;
        t.slot_site = ptr<uint32_t>(tb.slot_site);
        t.slot_pos = ptr<uint32_t>(tb.slot_pos);
        t.items = ptr<uint32_t>(tb.items);
        t.n_items = n_items;
        t.d = ptr<float>(tb.d);
        t.dp = ptr<float>(tb.dp);
        t.r2 = ptr<float>(tb.r2);
        t.mask = ptr<unsigned long long>(tb.mask);
        t.tile_pref = ptr<uint32_t>(tb.tile_pref);
        t.slot_cnt = ptr<uint32_t>(tb.slot_cnt);
        t.slot_base = ptr<uint32_t>(tb.slot_base);
        t.guard = ptr<unsigned>(tb.guard);
        const size_t s0 = (size_t)b0 * targets_plan::kBlock;
        HIP_TRY(hipMemcpyAsync(tb.slot_site.p, p.slot_site.data() + s0, ns * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(tb.slot_pos.p, p.slot_pos.data() + s0, ns * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(tb.items.p, items.data(), items.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(tb.mask.p, 0, ns * T * 8, c->stream));
        HIP_TRY(hipMemsetAsync(tb.guard.p, 0, 16, c->stream));
        HIP_TRY(hipEventRecord(c->ev_tg[0], c->stream));
        launch_targets_pairs(t, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev_tg[1], c->stream));
        launch_targets_count(t, c->stream);
        HIP_TRY(hipGetLastError());
        base.assign(ns + 1, 0);
        unsigned guard = 0;
        HIP_TRY(hipMemcpyAsync(base.data(), tb.slot_base.p, (ns + 1) * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(&guard, tb.guard.p, sizeof guard, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // (items, too, has been read)
        ms += std::max(0.0f, event_ms(c->ev_tg[0], c->ev_tg[1]));
        const uint64_t rows = base[ns];
        for (size_t s = 0; s < ns; ++s) {
            slot_begin[s0 + s] = base[s];
            slot_rows[s0 + s] = base[s + 1] - base[s];
        }
        if (!guard && rows) {
            for (DevBuf *b : {&tb.o_t, &tb.o_st, &tb.o_sp, &tb.o_d, &tb.o_dp, &tb.o_r2}) WLD_TRY(ensure(*b, rows * 4));
            t.out_target = ptr<uint32_t>(tb.o_t);
            t.out_site_target = ptr<uint32_t>(tb.o_st);
            t.out_site_partner = ptr<uint32_t>(tb.o_sp);
            t.out_d = ptr<float>(tb.o_d);
            t.out_dp = ptr<float>(tb.o_dp);
            t.out_r2 = ptr<float>(tb.o_r2);
            t.out_cap = rows;
            launch_targets_rows(t, c->stream);
            HIP_TRY(hipGetLastError());
            TargetCols &h = cols[k];
            h.t.resize(rows), h.st.resize(rows), h.sp.resize(rows), h.d.resize(rows), h.dp.resize(rows), h.r2.resize(rows);
            HIP_TRY(hipMemcpyAsync(h.t.data(), tb.o_t.p, rows * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(h.st.data(), tb.o_st.p, rows * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(h.sp.data(), tb.o_sp.p, rows * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(h.d.data(), tb.o_d.p, rows * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(h.dp.data(), tb.o_dp.p, rows * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(h.r2.data(), tb.o_r2.p, rows * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(&guard, tb.guard.p, sizeof guard, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        if (guard)
            return fail(WLD_E_STATE, "internal: the target kernels refused an out-of-range index (guard 0x%x: %s%s%s)",
                        guard, guard & kTargetsGuardItem ? "work item " : "", guard & kTargetsGuardSite ? "target site " : "",
                        guard & kTargetsGuardRow ? "row position" : "");
    }
    out->kernel_ms = ms;
    // the list order: target k's rows are its slot's run of its batch's arrays
    std::vector<uint32_t> slot_batch(n_slots_all, 0);
    for (uint32_t k = 0; k < p.batches(); ++k)
        for (size_t s = (size_t)p.batch_begin[k] * targets_plan::kBlock; s < (size_t)p.batch_begin[k + 1] * targets_plan::kBlock; ++s)
            slot_batch[s] = k;
    std::vector<size_t> slot_of(n);
    for (size_t s = 0; s < n_slots_all; ++s)
        if (p.slot_pos[s] != targets_plan::kNoTarget) slot_of[p.slot_pos[s]] = s;
    for (uint32_t k = 0; k < n; ++k) out->offset[k + 1] = out->offset[k] + slot_rows[slot_of[k]];
    const uint64_t total = out->offset[n];
    const size_t bytes = std::max<uint64_t>(total, 1) * 4;
    out->target = (uint32_t *)malloc(bytes);
    out->site_target = (uint32_t *)malloc(bytes);
    out->site_partner = (uint32_t *)malloc(bytes);
    out->d = (float *)malloc(bytes);
    out->d_prime = (float *)malloc(bytes);
    out->r2 = (float *)malloc(bytes);
    if (!out->target || !out->site_target || !out->site_partner || !out->d || !out->d_prime || !out->r2)
        return fail(WLD_E_OOM, "host allocation of %llu target rows failed", (unsigned long long)total);
    for (uint32_t k = 0; k < n; ++k) {
        const size_t s = slot_of[k];
        const uint64_t m = slot_rows[s], from = slot_begin[s], to = out->offset[k];
        if (!m) continue;
        const TargetCols &h = cols[slot_batch[s]];
        memcpy(out->target + to, h.t.data() + from, m * 4);
        memcpy(out->site_target + to, h.st.data() + from, m * 4);
        memcpy(out->site_partner + to, h.sp.data() + from, m * 4);
        memcpy(out->d + to, h.d.data() + from, m * 4);
        memcpy(out->d_prime + to, h.dp.data() + from, m * 4);
        memcpy(out->r2 + to, h.r2.data() + from, m * 4);
    }
    out->n = total;
    return WLD_OK;
}
}  // namespace

int wld_run_targets(wld_ctx *c, const uint32_t *targets, uint32_t n_targets, float r2_threshold,
                    wld_target_rows *out) {
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    WLD_TRY(set_dev(c));  // (a device group: WLD_E_STATE)
    if (!c->loaded) return fail(WLD_E_STATE, "wld_run_targets before wld_load");
    if (c->pend.active) return fail(WLD_E_STATE, "wld_run_targets during a run");
    if (n_targets && !targets) return fail(WLD_E_ARG, "wld_run_targets: null targets with n_targets %u", n_targets);
    if (c->safe)
        return fail(WLD_E_ARG, "wld_run_targets needs finite weights (this load takes the select loop)");
    const size_t L = c->L;
    int st = WLD_OK;
    try {
        const targets_plan::Bad bad = targets_plan::validate(targets, n_targets, (uint32_t)L);
        if (bad.kind == targets_plan::kOutOfRange)
            return fail(WLD_E_ARG, "wld_run_targets: targets[%u] = %u is not a loaded site (%zu loaded)", bad.pos,
                        targets[bad.pos], L);
        if (bad.kind == targets_plan::kRepeated)
            return fail(WLD_E_ARG, "wld_run_targets: targets[%u] = %u repeats targets[%u]", bad.pos, targets[bad.pos],
                        bad.first);
        if (n_targets && (uint64_t)n_targets * (L - 1) > targets_plan::kMaxRows)
            return fail(WLD_E_ARG, "wld_run_targets: %u targets x %zu partners exceed 2^32 - 1 rows: split the list",
                        n_targets, L - 1);
        out->n_targets = n_targets;
        out->offset = (uint64_t *)calloc((size_t)n_targets + 1, sizeof(uint64_t));
        if (!out->offset) return fail(WLD_E_OOM, "host allocation of %u offsets failed", n_targets);
        if (n_targets) st = run_targets(c, targets, n_targets, r2_threshold, out);
    } catch (const std::bad_alloc &) {
        st = fail(WLD_E_OOM, "wld_run_targets: host allocation failed");
    }
    // the staging goes back unless it is small (a later row run finds the
    // memory it would have found without this call)
    size_t held = 0;
    for (DevBuf *b : c->tg.all()) held += b->bytes;
    if (st != WLD_OK || held > (64u << 20)) {
        (void)hipStreamSynchronize(c->stream);  // nothing of the call is in flight when its buffers go
        for (DevBuf *b : c->tg.all()) release(*b);
    }
    if (st != WLD_OK) {
        const std::string msg = wld_last_error();  // (wld_target_rows_free does not fail, but keep the message)
        wld_target_rows_free(out);
        return fail(st, "%s", msg.c_str());
    }
    return WLD_OK;
}

void wld_target_rows_free(wld_target_rows *r) {
    if (!r) return;
    free(r->offset);
    free(r->target);
    free(r->site_target);
    free(r->site_partner);
    free(r->d);
    free(r->d_prime);
    free(r->r2);
    memset(r, 0, sizeof(*r));
}

int wld_all_weighted_ld_pairs(wld_ctx *c, const uint8_t *sites, size_t n_sites, size_t n_seqs,
                              const uint64_t *site_map, const float *weights, float r2_threshold,
                              wld_progress_fn progress, void *user, wld_pairs *out) {
    if (!out) return fail(WLD_E_ARG, "null out");
    memset(out, 0, sizeof(*out));
    if (progress) progress(0, user);  // lib.rs:584
    WLD_TRY(wld_load(c, sites, n_sites, n_seqs, site_map, weights));
    return wld_run_host(c, r2_threshold, progress, user, out);
}

int wld_single_weighted_ld_pair(wld_ctx *c, const uint8_t *a, const uint8_t *b, const float *weights, size_t n_seqs,
                                float out[3]) {
    if (!a || !b || !weights || !out) return fail(WLD_E_ARG, "null argument");
    if (c && !c->members.empty()) {
        // one pair: the first device; the group's loaded set is replaced (as
        // on a single context), so every member needs a new wld_load
        for (wld_ctx *m : c->members) m->loaded = false;
        c = c->members[0];
    }
    std::vector<uint8_t> buf(2 * n_seqs);
    memcpy(buf.data(), a, n_seqs);
    memcpy(buf.data() + n_seqs, b, n_seqs);
    WLD_TRY(wld_load(c, buf.data(), 2, n_seqs, nullptr, weights));
    float d[4], dp[4], r2[4];
    uint8_t v[4];
    WLD_TRY(wld_dense(c, d, dp, r2, v));
    if (!v[1]) return 0;
    out[0] = d[1];
    out[1] = dp[1];
    out[2] = r2[1];
    return 1;
}

}  // extern "C"
