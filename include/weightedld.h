/*
 * weightedld.h — C ABI of the MI355X-native WeightedLD all-pairs LD hot path.
 *
 * The reference (ojcharles/WeightedLD, Rust crate rust/weighted_ld) has no FFI;
 * its hot path is the generic Rust fn
 *     pub fn all_weighted_ld_pairs(site_set: &SiteSet, weights: &[f32],
 *                                  r2_threshold: f32,
 *                                  progress_report: impl FnMut(usize) + Send)
 *         -> PairStore<LdStats>                               (lib.rs:578-684)
 * called once from main.rs:180-190.  The entry points below are what a Rust
 * `extern "C"` binding of that seam needs: plain pointers
 * and sizes, no Rust/C++/torch types, no exceptions across the boundary, every
 * call returns a status code (WLD_OK or a negative WLD_E_*), and
 * wld_last_error() gives the message for the calling thread.
 *
 * Symbol codes are the reference's #[repr(u8)] Symbol (lib.rs:20-29):
 *     A=0 C=1 G=2 T=3 Missing('-')=4 Unknown=5
 * A "site-major" buffer is SiteSet.buffer (lib.rs:163): buffer[site*n_seqs+seq].
 */
#ifndef WEIGHTEDLD_H
#define WEIGHTEDLD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status */
#define WLD_OK 0
#define WLD_E_ARG (-1)    /* bad argument (the reference would panic)           */
#define WLD_E_HIP (-2)    /* HIP runtime error                                   */
#define WLD_E_OOM (-3)    /* device or host allocation failed                    */
#define WLD_E_NODEV (-4)  /* no usable gfx950 device                             */
#define WLD_E_IO (-5)     /* file could not be read / written                    */
#define WLD_E_FORMAT (-6) /* input violates the reference's format (it panics)  */
#define WLD_E_STATE (-7)  /* call order violated (e.g. run before load), or a
                             device guard refused an out-of-range index (the
                             run produced no rows; the context stays usable)    */

#define WLD_SYM_A 0
#define WLD_SYM_C 1
#define WLD_SYM_G 2
#define WLD_SYM_T 3
#define WLD_SYM_MISSING 4
#define WLD_SYM_UNKNOWN 5
#define WLD_NONE (-1) /* Option<Symbol>::None */

const char *wld_status_string(int status);
/* Message of the last failed call on this thread ("" if none). */
const char *wld_last_error(void);
/* Library version string, e.g. "weightedld-amd 0.1.0 (gfx950)". */
const char *wld_version(void);

/* ========================================================================
 * Host pre-pass — stays on the host per north_star.  Mirrors lib.rs:20-380.
 * ======================================================================== */

/* Opaque SiteSet (lib.rs:158-173): site-major symbol buffer, optional
 * site_map (filtered index -> parent index, lib.rs:165-169) and per-site
 * histograms (lib.rs:171-172). */
typedef struct wld_siteset wld_siteset;

/* read_fasta + SiteSet::from_multiseq (lib.rs:277-307, 176-206), including the
 * reader's quirks: every non-'>' line is one sequence and its '\n' becomes a
 * trailing Unknown site.  WLD_E_FORMAT where the reference panics (sequences
 * of unequal length, lib.rs:180-182; no sequence at all, lib.rs:178). */
int wld_read_fasta(const char *path, wld_siteset **out);

/* VCF reader following the Python reference's handle_vcf
 * (WeightedLD.py:311-379): phased diploid calls split into two haplotypes,
 * '.' -> 4 (Missing), allele digits used as symbol codes, the last data line
 * dropped (:365), haplotypes in reversed order (np.rot90, :375) and
 * site_map = POS.  The Rust crate has no VCF input; this serves BASELINE
 * config 3.  WLD_E_FORMAT where the Python code exits. */
int wld_read_vcf(const char *path, wld_siteset **out);

/* Builds a SiteSet from a caller buffer (copied); histograms computed as in
 * from_multiseq (lib.rs:194-196). site_map may be NULL (identity). */
int wld_siteset_from_buffer(const uint8_t *site_major, size_t n_sites, size_t n_seqs,
                            const uint64_t *site_map, wld_siteset **out);
void wld_siteset_free(wld_siteset *s);
size_t wld_siteset_n_sites(const wld_siteset *s);                        /* lib.rs:254-256 */
size_t wld_siteset_n_seqs(const wld_siteset *s);                         /* lib.rs:259-261 */
const uint8_t *wld_siteset_buffer(const wld_siteset *s);                 /* SiteSet.buffer */
const uint64_t *wld_siteset_site_map(const wld_siteset *s);              /* NULL = identity */
uint64_t wld_siteset_parent_site_index(const wld_siteset *s, size_t i);  /* lib.rs:263-265 */
int wld_siteset_histogram(const wld_siteset *s, size_t site, uint64_t out[6]); /* lib.rs:272 */

/* SymbolHistogram::from_slice (lib.rs:98-104) and major_minor_symbols
 * (lib.rs:126-140): ties keep the earlier of A,C,G,T,-; Unknown never
 * eligible; WLD_NONE for None. */
int wld_histogram(const uint8_t *symbols, size_t n, uint64_t out[6]);
int wld_major_minor(const uint64_t hist[6], int *major, int *minor);

/* is_site_of_interest (lib.rs:309-338); min_acgt is the COUNT
 * ceil(min_acgt_frac * n_seqs) of main.rs:139.  Returns 1/0. */
int wld_is_site_of_interest(const uint8_t *site, size_t n, size_t min_acgt, float min_minor,
                            float max_minor);

/* main.rs:139-143: siteset.filter_by(is_site_of_interest) with
 * min_acgt = ceil(min_acgt_frac * n_seqs) (f32 arithmetic), i.e.
 * SiteSet::filter_by (lib.rs:230-251). */
int wld_siteset_filter_sites_of_interest(const wld_siteset *s, float min_acgt_frac,
                                         float min_minor, float max_minor, wld_siteset **out);

/* henikoff_weights (lib.rs:340-380), out has n_seqs floats. */
int wld_henikoff_weights(const wld_siteset *s, float *out);

/* ========================================================================
 * Device hot path — replaces all_weighted_ld_pairs / single_weighted_ld_pair.
 * ======================================================================== */

typedef struct wld_ctx wld_ctx;

/* One context per device; owns its HIP stream, device buffers and results.
 * Not thread-safe; separate contexts are independent.  device = HIP ordinal. */
int wld_create(int device, wld_ctx **out);
/* A context over n_devices devices (HIP ordinals; repeats allowed, e.g. to run
 * several shards on one device in tests): one member context per entry.
 * wld_load replicates the input to every member; wld_run_host and
 * wld_all_weighted_ld_pairs (the reference's one call, lib.rs:578-684, which
 * uses every core) shard the reference's chunk sequence over the members
 * (wld_shard_chunks: contiguous ranges balanced by pair count), run them
 * concurrently, and return the rows in the reference order (shards
 * concatenated in descending shard order).  Options and the kernel choice
 * apply to every member; wld_last_stats reports member 0's kernel with the
 * group's pair/row totals.  wld_run_summary shards the same way and adds the
 * members' summaries.  Other device entry points (wld_run_prune among them)
 * fail with WLD_E_STATE on such a context.  With n_devices == 1 it returns a plain single-device
 * context (wld_create(devices[0], out)), on which every entry point works. */
int wld_create_multi(const int *devices, int n_devices, wld_ctx **out);
int wld_n_devices(const wld_ctx *ctx); /* 1, or the member count of a multi-device context */
void wld_destroy(wld_ctx *ctx);

/* Kernel selection.  AUTO (default): the exact-integer MFMA kernel when the
 * weights are finite, their dynamic range fits its fixed-point weight planes
 * (3 digit planes, 23-bit fixed point, when min |w| >= 2^-4 max |w|; 4 planes,
 * 31-bit, when min |w| >= 2^-12 max |w| and n_seqs <= 65,024: every weight
 * within 2^-19 relative) and n_seqs <= 5,592,320 (int32 sums),
 * else the exact-product f32 kernel (WLD_KERNEL_VALU: f32-input MFMA for
 * finite weights, a VALU loop otherwise).  An explicit WLD_KERNEL_MFMA with
 * non-finite or all-zero weights, or more sequences, fails with WLD_E_ARG at
 * load (a wide dynamic range is allowed: small weights lose precision).  Both
 * run on the GPU; there is no CPU path. */
#define WLD_KERNEL_AUTO 0
#define WLD_KERNEL_VALU 1
#define WLD_KERNEL_MFMA 2
int wld_set_kernel(wld_ctx *ctx, int kernel);

/* Per-context options (the library reads no environment variables).  Except
 * WLD_OPT_REF_SUMS none changes a result: every setting gives bit-identical
 * rows; they exist for A/B measurements and tests.  Set between runs; WLD_E_ARG for an unknown
 * option or a bad value.
 *   WLD_OPT_PREFILTER  1 (default): with r2_threshold > 0 the MFMA kernel
 *                      skips the f32 epilogue of pairs that a rigorous bound
 *                      proves cannot pass; 0: every pair.
 *   WLD_OPT_SCREEN     1 (default, auto): with the prefilter on, a screen
 *                      launch on the top nonzero weight-digit plane bounds
 *                      every pair's r2 (the lower planes' share bounded
 *                      exactly; none with a single nonzero plane, e.g. equal
 *                      weights) and only candidate 64x64 tiles are recomputed
 *                      with every plane — unless at this or a higher threshold
 *                      the screen left more than half the tiles as candidates.
 *                      Then (three or more active planes) the screen runs on
 *                      the top two planes, the planes below bounded the same
 *                      way, unless at this or a higher threshold that left more
 *                      than a fifth of the tiles as candidates (then every
 *                      tile goes to the full kernel directly); 2: always the
 *                      one-plane screen; 3: always the two-plane screen (the
 *                      one-plane one with fewer than three active planes);
 *                      0: every tile, every plane.  In lib.rs's order
 *                      (WLD_OPT_REF_SUMS 1) auto replaces the two-plane tier:
 *                      where the one-plane screen does not pay, every tile runs
 *                      once on the top two digit planes, staging the pairs the bound cannot
 *                      reject (the reference's rounding as residual), and only
 *                      those are summed in lib.rs's order, one by one — unless
 *                      at this or a higher threshold they were more than a
 *                      tenth of all pairs (then the full f32 kernel); 4: always
 *                      that path (lib.rs's order; otherwise as 0).
 *   WLD_OPT_TILE_ORDER 0 (default): L2/XCD-aware tile launch order; 1: plain
 *                      (a-tile, b-tile) order.
 *   WLD_OPT_ALL_PLANES 0 (default): all-zero digit planes are skipped; 1: the
 *                      MFMA kernel multiplies all three.
 *   WLD_OPT_MFMA_LAYOUT 0 (default): LDS-streaming fragment-major kernel; 1:
 *                      the site-major register kernel (takes effect at the
 *                      next load).
 *   WLD_OPT_VALU_PLAIN 0 (default): the f32 fallback multiplies on f32-input
 *                      MFMA; 1: a VALU fmaf loop (same sums, same order).
 *   WLD_OPT_REF_SUMS   1 (default): the four masked sums of every pair are
 *                      formed in lib.rs's own f32 order — 8 lane sums of the
 *                      sequences k = j mod 8 (lib.rs:416-445), their ordered
 *                      horizontal sum (packed_simd's x86 f32x8::sum(),
 *                      :447-452), then the scalar tail (:461-480) — on the f32
 *                      kernel, so d, d' and r2 are bit-identical to lib.rs's
 *                      on every input, including pairs whose f32 sums lib.rs
 *                      itself gets wrong (minor alleles carried by a few
 *                      low-weight sequences).  With the MFMA kernel and a
 *                      positive threshold the i8 screen runs first, its bound
 *                      widened by the reference's rounding, and only candidate
 *                      tiles take the f32 kernel.  0: exact sums (integer
 *                      MFMA, all digit planes; the f32 kernel's two-level sums
 *                      when the weights need it) rounded once — more accurate
 *                      than lib.rs, faster where many tiles are candidates
 *                      (linkage, thresholds <= 0), and different from lib.rs
 *                      in the last bits (or more on ill-conditioned pairs).
 *                      The one option that changes results.
 *   WLD_OPT_STAGING_ROWS   initial staging capacity in rows (default 2^25;
 *                      grown on overflow by a re-run).
 *   WLD_OPT_HOST_BATCH_PAIRS  pairs per batch of wld_run_host (default 2^31).
 *   WLD_OPT_SCREEN_FP6 1 (default, auto): the one-plane screen multiplies
 *                      fp6 (e2m3) weights by fp4 codes on the block-scaled
 *                      MFMA (128 sequences per instruction, twice the i8
 *                      rate) when the weights are nonnegative, at most 16,384
 *                      sequences, and their fp6 rounding leaves a residual
 *                      within 2% of the sums or twice the i8 top digit's, at
 *                      thresholds above any at which it left more than a
 *                      quarter of the tiles as candidates; 0: the i8 screen;
 *                      2: fp6 whenever it applies; 3: auto without the
 *                      sample run (below).  Auto decides a threshold it has
 *                      not seen from a sample run first (about 1/64 of the
 *                      tiles screened on fp6, counting only): past a
 *                      sixteenth of them as candidates the pass screens on
 *                      i8.  Same rows (a screen only decides which tiles are
 *                      computed).
 *   WLD_OPT_FUSED_SCAN 1 (default): after a screen, the run's chunk scan runs
 *                      in the candidate launch's last workgroup (ranges up to
 *                      4096 chunks); 0: as a launch of its own (the kernel
 *                      boundary orders it).  Same rows.
 *   WLD_OPT_FP6_PAIRS_MIN_TILES  the fp6 screen computes two tiles of a row
 *                      per workgroup (one shared A operand stream) when the
 *                      run's tile list has at least this many tiles (default
 *                      0: always), else one tile per workgroup.  Same rows.
 *   WLD_OPT_I8_PAIRS   1 (default): the i8 one-plane screen (nonnegative
 *                      weights, at most 16,384 sequences) runs on the fp6
 *                      screen's tile-pair list with wide waves, its operands
 *                      (the top weight digit times the site indicators, and
 *                      the codes) pre-multiplied once per load (3 bytes per
 *                      site and sequence); 0: one tile per workgroup, the
 *                      operands formed per stage.  Same rows.
 *   WLD_OPT_FP6_A4     1 (default, auto): where every rounded weight of a load
 *                      is also an fp4 (e2m1) value (0, 0.5, 1, 1.5, 2, 3, 4, 6:
 *                      unit weights, Henikoff weights of a large alignment) the
 *                      fp6 screen's A operand image is built as fp4, two thirds
 *                      of the bytes and four operand registers instead of six
 *                      at the same MFMA rate; 0: always fp6.  Every product is
 *                      exact either way: same sums, candidates and rows.
 *                      Setting it discards the built images (the next run that
 *                      may screen on fp6 rebuilds them).
 *   WLD_OPT_FP6_SHARED 1 (default, auto): where every rounded weight of a load
 *                      is the same nonzero value (unit weights, an unweighted
 *                      VCF, Henikoff weights of a large alignment) the fp6
 *                      screen builds no A operand image: its kernels read the
 *                      row tile from the B code image as well, mask it into
 *                      the two A channels and scale the sums by the one weight
 *                      value afterwards (a third of the operand bytes per load,
 *                      three quarters of the bytes per stage); 0: the A image
 *                      WLD_OPT_FP6_A4 chooses.  Every scaled sum is exact: same
 *                      sums, candidates and rows.  Setting it discards the
 *                      built images, as WLD_OPT_FP6_A4.
 *   WLD_OPT_FP6_THREE  1 (default, auto): where the fp6 screen runs on tile
 *                      pairs and its sample run (WLD_OPT_SCREEN_FP6 1) found it
 *                      worthwhile at this threshold or a lower one, the screen
 *                      forms three of the four masked sums per pair, decides
 *                      every pair it can from the interval they leave for the
 *                      fourth (the missing-by-missing sum), and forms the
 *                      fourth, in a second pass over the entry, only for
 *                      entries with a pair in doubt (at most an eighth of the
 *                      sampled entries, else four sums); lists that are not
 *                      sampled stay on four sums.  2: three sums wherever the
 *                      tile-pair fp6 screen runs; 0: always four.  A pair the
 *                      three sums reject is rejected on four: same candidate
 *                      tiles, sub-blocks and rows.
 *   WLD_OPT_FP6_QUICK  1 (default, auto): where the fp6 screen runs on three
 *                      sums (WLD_OPT_FP6_THREE) and its sample run found it
 *                      worthwhile at this threshold or a lower one, each wave
 *                      first tries to reject a lane's 16 pairs of a row block
 *                      together, from one numerator maximum and marginal
 *                      bounds shared by the lane, at half the vector
 *                      operations per pair; a row block where some lane
 *                      cannot (at most a quarter of the sampled ones, else
 *                      off) takes the per-pair test as before.  Lists that
 *                      are not sampled stay off.  2: wherever the three-sum
 *                      kernel runs; 0: never.  A row block the quick test
 *                      rejects holds no pair the per-pair test keeps: same
 *                      second passes, candidate tiles, sub-blocks and rows.
 *   WLD_OPT_TARGET_BATCH_SLOTS  wld_run_targets: the pair slots (16 x target
 *                      blocks x padded site count, three floats each) of the
 *                      dense staging one batch may use (default 2^26: 768 MiB;
 *                      a batch always holds at least one block of 16 targets).
 *                      Changes no result; it exists so tests can force several
 *                      batches.
 *   WLD_OPT_PARTNERS_BATCH_BYTES  wld_run_partners: the bytes of tile staging
 *                      one batch may use (default 2^30; a batch always holds at
 *                      least one tile).  Changes no bit of a result; it exists
 *                      to bound memory and so tests can force several batches.
 *   WLD_OPT_MATRIX_BATCH_BYTES  wld_run_matrix: the bytes of the device buffer
 *                      one band of whole rows may use (default 2^30; a band
 *                      always holds at least 64 rows).  Changes no byte of a
 *                      result; it bounds memory and lets tests force bands.
 *   WLD_OPT_TEST_GUARD 0 (default); 1 (tests only): before each candidate
 *                      launch the last candidate bucket's count is set one
 *                      past its capacity, so the launch meets an entry outside
 *                      the buckets.  Its guard refuses the entry and the run
 *                      fails with WLD_E_STATE instead of reading through it;
 *                      the next run (option back at 0) starts clean.
 *                      (Ids 9 and 10, an experimental 64x128-tile screen and an fp4
 *                      screen of round 2, are retired: WLD_E_ARG.) */
#define WLD_OPT_PREFILTER 1
#define WLD_OPT_SCREEN 2
#define WLD_OPT_TILE_ORDER 3
#define WLD_OPT_ALL_PLANES 4
#define WLD_OPT_MFMA_LAYOUT 5
#define WLD_OPT_VALU_PLAIN 6
#define WLD_OPT_STAGING_ROWS 7
#define WLD_OPT_HOST_BATCH_PAIRS 8
#define WLD_OPT_REF_SUMS 11
#define WLD_OPT_FUSED_SCAN 12
#define WLD_OPT_SCREEN_FP6 13
#define WLD_OPT_TEST_GUARD 14
#define WLD_OPT_FP6_PAIRS_MIN_TILES 15
#define WLD_OPT_I8_PAIRS 16
#define WLD_OPT_FP6_A4 17
#define WLD_OPT_TARGET_BATCH_SLOTS 18
#define WLD_OPT_FP6_SHARED 19
#define WLD_OPT_PARTNERS_BATCH_BYTES 20
#define WLD_OPT_FP6_THREE 21
#define WLD_OPT_FP6_QUICK 22
#define WLD_OPT_MATRIX_BATCH_BYTES 23
int wld_set_option(wld_ctx *ctx, int option, int64_t value);
int wld_get_option(wld_ctx *ctx, int option, int64_t *value);

/* The window: which pairs a run computes at all (PLINK's --ld-window /
 * --ld-window-kb, VCFtools' --ld-window / --ld-window-bp; not in the
 * reference).  With pos[i] = site_map[i] of the loaded (filtered) set, or i
 * without a map, a pair a < b of loaded indices is in the window iff
 *   (max_distance == 0 || pos[b] - pos[a] <= max_distance) and
 *   (max_sites == 0 || b - a <= max_sites);
 * 0 means no limit, (0, 0) (the default) no window.  max_distance is in
 * parent coordinates (VCF POS, alignment columns), max_sites counts loaded
 * sites.  The rows of a windowed run are exactly the rows of the same run
 * without a window whose pair is in the window: same order, parent indices
 * and bits, on every kernel path; tiles without an in-window pair are not
 * computed.  Per context (a device group forwards it to every member), it
 * persists across loads until changed, and is obeyed by wld_run,
 * wld_run_chunks[_async], wld_run_host and wld_all_weighted_ld_pairs.
 * wld_dense and wld_single_weighted_ld_pair IGNORE it.  Under a window
 * wld_run_stats.pairs counts the in-window pairs of the run's chunks and
 * .tiles the 64x64 tiles holding one; staging, the 2^32 pairs-per-run limit
 * and wld_run_host's batches are sized by in-window pairs; progress is called
 * once per chunk that holds an in-window pair, with in-window counts.
 * With max_distance > 0 the loaded site_map must be non-decreasing (equal
 * neighbours allowed: multi-allelic VCF lines share a POS): otherwise
 * WLD_E_ARG naming the first offending index, from whichever of wld_load* and
 * wld_set_window comes second (a refused window leaves the previous one).
 * WLD_E_STATE while a run is in flight.  Sets of more than 2^24 chunks
 * (about 1.48M sites) take no window. */
int wld_set_window(wld_ctx *ctx, uint64_t max_distance, uint64_t max_sites);
int wld_get_window(wld_ctx *ctx, uint64_t *max_distance, uint64_t *max_sites);
/* In-window pairs of the linear chunks [begin,end) of the loaded set under
 * the current window (= wld_pairs_in_chunks without one). */
int wld_window_pairs_in_chunks(wld_ctx *ctx, uint32_t begin, uint32_t end, uint64_t *pairs);
/* wld_shard_chunks for the loaded set, balanced by in-window pairs: contiguous
 * linear ranges, shard 0 takes the LAST one; no shard exceeds total/n_shards
 * by more than the largest single chunk's count.  wld_run_host on a device
 * group uses it when a window is set.  (= wld_shard_chunks without one.) */
int wld_shard_chunks_window(wld_ctx *ctx, int n_shards, int shard, uint32_t *begin, uint32_t *end);
/* The window's per-site limits as the device computed them from the resident
 * site_map: hi[a] = the last in-window partner of loaded site a (a itself:
 * none), n_sites entries; for tests.  WLD_E_STATE without a window. */
int wld_window_limits_copy(wld_ctx *ctx, uint32_t *hi);

/* Rows of PairStore<LdStats> (lib.rs:523-576) as structure-of-arrays, in the
 * reference's order: 256x256 chunks in triu_index order (lib.rs:623-635:
 * chunk rows descending, columns ascending), then site_a, then site_b
 * ascending.  Site indices are PARENT indices (lib.rs:662-663).  Only rows
 * with r2 > r2_threshold (strict, lib.rs:660; NaN never passes). */
typedef struct {
    uint64_t n;
    uint32_t *site_a;
    uint32_t *site_b;
    float *d;
    float *d_prime;
    float *r2;
} wld_pairs;
void wld_pairs_free(wld_pairs *p); /* only for host results made by this library */

/* progress_report (lib.rs:582, main.rs:184-188).  Called on the calling
 * thread (never from a worker): once with 0 before any work (lib.rs:584, by
 * wld_all_weighted_ld_pairs), then once per completed 256x256 chunk with the
 * number of pairs in the chunks completed before it — the previous value of
 * lib.rs's fetch_add counter (lib.rs:670-674); values never decrease. */
typedef void (*wld_progress_fn)(uint64_t pairs_done, void *user);

/* Drop-in for all_weighted_ld_pairs (lib.rs:578-684).  Blocking.  sites is
 * SiteSet.buffer (n_sites*n_seqs bytes, host memory), site_map the SiteSet's
 * site_map (NULL = identity), weights n_seqs floats.  Allocates out's host
 * arrays (release with wld_pairs_free). */
int wld_all_weighted_ld_pairs(wld_ctx *ctx, const uint8_t *sites, size_t n_sites, size_t n_seqs,
                              const uint64_t *site_map, const float *weights, float r2_threshold,
                              wld_progress_fn progress, void *user, wld_pairs *out);

/* Drop-in for single_weighted_ld_pair (lib.rs:390-521) with the histograms of
 * a and b taken from the slices themselves (as SiteSet does).  Returns 1 and
 * fills out[3] = {d, d_prime, r2} for Some, 0 for None, <0 on error.  Ignores
 * the window (wld_set_window). */
int wld_single_weighted_ld_pair(wld_ctx *ctx, const uint8_t *a, const uint8_t *b,
                                const float *weights, size_t n_seqs, float out[3]);

/* ---- staged API: inputs resident in HBM, shardable, results on device ---- */

/* Uploads a SiteSet (host pointers) and encodes it on the device: per-site
 * histogram -> major/minor (lib.rs:126-140, hoisted out of the pair loop)
 * -> per-sequence codes and weight planes.  Replaces any previous load. */
int wld_load(wld_ctx *ctx, const uint8_t *sites, size_t n_sites, size_t n_seqs,
             const uint64_t *site_map, const float *weights);
/* Same, from device pointers already resident in HBM (d_sites: n_sites*n_seqs
 * bytes site-major; d_weights: n_seqs floats; site_map host, may be NULL). */
int wld_load_device(wld_ctx *ctx, const void *d_sites, size_t n_sites, size_t n_seqs,
                    const uint64_t *site_map, const void *d_weights);

/* Device pre-pass, replacing the host steps of
 * main.rs:139-156 for the staged API: from the UNFILTERED SiteSet buffer
 * (n_sites*n_seqs site-major Symbol codes, lib.rs:163), keeps the sites for
 * which is_site_of_interest(site, ceil(min_acgt*n_seqs), min_minor, max_minor)
 * holds (lib.rs:309-338; filter_by, lib.rs:230-251), computes Henikoff weights
 * on the kept sites (lib.rs:340-380) or unit weights if `unweighted`
 * (main.rs:150-153), and loads the kept set for wld_run with parent site
 * indices as its site_map.  Bit-identical to wld_siteset_filter_sites_of_interest
 * + wld_henikoff_weights + wld_load.  *n_kept receives the kept site count. */
int wld_load_filtered(wld_ctx *ctx, const uint8_t *sites, size_t n_sites, size_t n_seqs,
                      const uint64_t *site_map, float min_acgt, float min_minor, float max_minor,
                      int unweighted, size_t *n_kept);
/* Same, from a device pointer (read during the call only).  In both, site_map
 * is the unfiltered SiteSet's own map (host, NULL = identity); kept sites
 * report site_map[i] as their parent index, as filter_by composes it. */
int wld_load_filtered_device(wld_ctx *ctx, const void *d_sites, size_t n_sites, size_t n_seqs,
                             const uint64_t *site_map, float min_acgt, float min_minor, float max_minor,
                             int unweighted, size_t *n_kept);
/* After wld_load_filtered[_device]: the n_seqs weights (for the weights TSV,
 * main.rs:157-165) and the n_kept parent site indices. */
int wld_weights_copy(wld_ctx *ctx, float *out);
int wld_site_map_copy(wld_ctx *ctx, uint64_t *out);

/* Number of 256-site chunk rows n = ceil(n_sites/256) (lib.rs:615-619), and a
 * balanced contiguous partition of chunk rows [begin,end) for shard `shard` of
 * `n_shards` (equal pair counts up to chunk granularity).  Each shard's rows
 * are a contiguous run of the reference order; shards concatenate in
 * DESCENDING shard order (chunk rows descend in triu_index order). */
uint32_t wld_chunk_rows(size_t n_sites);
int wld_shard_chunk_rows(size_t n_sites, int n_shards, int shard, uint32_t *begin, uint32_t *end);

/* The reference's chunk sequence (lib.rs:615-634): n(n+1)/2 chunks of 256x256
 * sites, linear index i <-> (row, col) by triu_index, rows descending and
 * columns ascending; PairStore rows come chunk by chunk in this order.
 * wld_shard_chunks partitions it into contiguous linear ranges [begin,end) of
 * near-equal pair count (single-chunk granularity, finer than chunk rows);
 * shard 0 takes the LAST range, so shards concatenate in DESCENDING shard
 * order, as with wld_shard_chunk_rows.  wld_pairs_in_chunks counts the pairs
 * (a<b) of a range. */
uint32_t wld_chunks(size_t n_sites);
int wld_shard_chunks(size_t n_sites, int n_shards, int shard, uint32_t *begin, uint32_t *end);
uint64_t wld_pairs_in_chunks(size_t n_sites, uint32_t begin, uint32_t end);

/* Evaluates every pair (a<b) whose a lies in chunk rows [row_begin,row_end)
 * (pass 0, wld_chunk_rows() for all), filters r2 > r2_threshold and leaves
 * the rows on the device in reference order.  *n_rows receives the count. */
int wld_run(wld_ctx *ctx, float r2_threshold, uint32_t row_begin, uint32_t row_end,
            uint64_t *n_rows);
/* wld_run over the linear chunk range [chunk_begin,chunk_end) (end 0 = all):
 * the rows of those chunks, in reference order (all_weighted_ld_pairs'
 * par_iter over 0..n(n+1)/2, lib.rs:621-683, restricted to a sub-range). */
int wld_run_chunks(wld_ctx *ctx, float r2_threshold, uint32_t chunk_begin, uint32_t chunk_end,
                   uint64_t *n_rows);
/* The same run in two calls, for callers that overlap it with a collective:
 * wld_run_chunks_async enqueues the pair kernel and the row count on the
 * context's stream (wld_stream) and returns without waiting; when
 * d_count_out (device, 8 bytes) is given the run's row total lands there as a
 * uint64 on that stream.  wld_run_wait completes the run (host wait, staging
 * regrowth, reference-order assembly) exactly as wld_run_chunks would.  No
 * other call may touch the context in between. */
int wld_run_chunks_async(wld_ctx *ctx, float r2_threshold, uint32_t chunk_begin, uint32_t chunk_end,
                         void *d_count_out);
int wld_run_wait(wld_ctx *ctx, uint64_t *n_rows);
/* Orders ctx's next run after prev's enqueued one on the device, no host wait:
 * ctx's stream waits until prev's pair kernels (for a screened pass: its
 * screen kernel) have completed; prev's candidate launch, row count and
 * assembly may still overlap ctx's kernels.  For callers that pipeline runs
 * over several contexts (the N>1 step loop): one pair kernel at a time with
 * the next one already queued.  A no-op when prev has no run in flight;
 * WLD_E_STATE when ctx has one; WLD_E_ARG for device groups. */
int wld_run_after(wld_ctx *ctx, wld_ctx *prev);
/* The context's HIP stream (hipStream_t), for ordering caller work after a run. */
void *wld_stream(wld_ctx *ctx);
/* Runs the context's device work on the caller's HIP stream from now on
 * (a hipStream_t of the context's device; NULL: back to the context's own
 * stream).  Contexts given one stream run one after another in enqueue order
 * with nothing between their kernels (the N=1 pipelined loop: the next run
 * queued behind the previous one without a cross-queue event, cf.
 * wld_run_after, which then returns at once).  WLD_E_STATE during a run,
 * WLD_E_ARG for device groups.  The stream is borrowed: it must outlive its
 * use by ctx (set the context back to NULL, or destroy ctx, before destroying
 * the stream or the context that owns it); wld_destroy waits for the work ctx
 * queued on a borrowed stream. */
int wld_set_stream(wld_ctx *ctx, void *stream);
/* All pairs of the loaded set, any size, rows to host: runs the reference's
 * chunk sequence in batches of at most 2^31 pairs (one wld_run_chunks each),
 * appending each batch's rows to library-allocated host arrays in reference
 * order (release with wld_pairs_free); progress (may be NULL) is called per
 * completed chunk as in wld_progress_fn: the kernels count down each chunk's
 * tiles and log finished chunks to mapped host memory, which the calling
 * thread polls while the batch runs. */
int wld_run_host(wld_ctx *ctx, float r2_threshold, wld_progress_fn progress, void *user, wld_pairs *out);
/* Device pointers of the last run's rows (valid until the next run/load or
 * destroy; do not free). */
int wld_rows_device(wld_ctx *ctx, wld_pairs *view);
/* Copies the last run's rows to caller host arrays of at least n_rows each
 * (any pointer may be NULL to skip that column). */
int wld_rows_copy(wld_ctx *ctx, uint32_t *site_a, uint32_t *site_b, float *d, float *d_prime,
                  float *r2);
/* Device-to-device copy of the last run's rows into caller device buffers
 * (e.g. tensors handed to an RCCL gather); NULL skips a column.  Completes
 * before returning. */
int wld_rows_copy_device(wld_ctx *ctx, void *site_a, void *site_b, void *d, void *d_prime, void *r2);
/* Dense stats of every pair a<b of the loaded set into host n_sites*n_sites
 * row-major matrices (valid[a*L+b] = 1 for Some); for tests.  Ignores the
 * window (wld_set_window): every pair. */
int wld_dense(wld_ctx *ctx, float *d, float *d_prime, float *r2, uint8_t *valid);

typedef struct {
    int kernel;              /* WLD_KERNEL_VALU or WLD_KERNEL_MFMA actually used   */
    uint64_t pairs;          /* pairs evaluated (a<b) in the last run              */
    uint64_t rows;           /* rows that passed the threshold                     */
    double pair_kernel_ms;   /* HIP-event time of the pair phase (last run): the pair
                                kernel, or screen + candidate launch           */
    double order_ms;         /* HIP-event time of the ordering kernels (last run)  */
    double load_ms;          /* HIP-event time of the encode kernel (last load)    */
    uint64_t pair_kernel_launches; /* 2 when screened: screen + candidate tiles */
    int weight_shift;        /* fixed-point exponent of the MFMA weight planes     */
    int mfma_planes;         /* weight-digit planes the MFMA kernel multiplies (1-3; all-zero planes skipped) */
    uint64_t tiles;          /* 64x64 site tiles of the last run                   */
    uint64_t candidate_tiles;/* tiles computed with every plane (= tiles unless screened) */
    double screen_ms;        /* HIP-event time of the screen launch (0 if none)    */
    int screened;            /* 1: the last run ran the one-plane i8 screen; 3: the two-plane
                                i8 screen; 4: (lib.rs's order) an i8 pass (the top two digit
                                planes) staging the pairs its bound cannot reject, each then
                                summed alone in lib.rs's order; 0: none */
    int ref_sums;            /* 1: the last run summed in lib.rs's f32 order (WLD_OPT_REF_SUMS) */
    uint64_t candidate_blocks; /* 16x16 sub-blocks of the candidate tiles holding a pair the screen
                                  could not reject (16 x candidate_tiles unless screened); with
                                  WLD_OPT_REF_SUMS only these are computed */
    uint64_t candidate_pairs; /* screened == 4: the pairs summed one by one in lib.rs's order */
    int screen_fp6;          /* screened == 1 on fp6 x fp4 block-scaled MFMA (WLD_OPT_SCREEN_FP6), not i8;
                                2: the fp6 screen gave the pass up (more than a sixteenth of the tiles were
                                candidates) and it re-ran on the i8 screen */
    int fp6_sampled;         /* 1: this pass's screen (fp6 or i8) was chosen by the fp6 screen's sample run
                                (WLD_OPT_SCREEN_FP6 1: about 1/64 of the tiles screened first, at a
                                threshold not decided before) */
    uint64_t progress_filled; /* per-chunk progress (wld_run_host with a callback): chunk reports the
                                 host made up from the chunk pair counts because the pass's log lacked
                                 their entries once it had completed; 0 unless the kernels' chunk
                                 accounting lost a count (the tests assert 0) */
    int fp6_a4;              /* 1: the pass screened on fp6 (screen_fp6 == 1) with the fp4 A image (WLD_OPT_FP6_A4),
                                or, where fp6_shared is 1, on a load whose codes would have taken it */
    int fp6_shared;          /* 1: the pass screened on fp6 (screen_fp6 == 1) with one code image for both
                                operands and no A image (WLD_OPT_FP6_SHARED) */
    int fp6_three;           /* 1: the pass screened on fp6 (screen_fp6 == 1) with three masked sums per pair
                                (WLD_OPT_FP6_THREE), the fourth only for the entries counted below */
    uint64_t fp6_rechecked;  /* fp6_three == 1: the screen's entries (tile pairs or single tiles) that ran the
                                second pass for the fourth sum; else 0 */
    int fp6_quick;           /* 1: the three-sum screen (fp6_three == 1) ran the lane-shared quick test in front of
                                its per-pair test (WLD_OPT_FP6_QUICK) */
    uint64_t fp6_quick_full; /* fp6_quick == 1: the screen's row blocks (16 sites x a 64-site tile, four per tile)
                                that the quick test did not reject and the per-pair test looked at; else 0 */
} wld_run_stats;
int wld_last_stats(wld_ctx *ctx, wld_run_stats *out);
/* The fp6 screen's weight codes of the loaded set (tests, diagnostics): the
 * e2m3 code of every sequence's rounded weight into codes[n_seqs], and
 * *fits_fp4 = 1 when every one is also an fp4 (e2m1) value, which is when
 * WLD_OPT_FP6_A4 builds the A image as fp4.  WLD_E_STATE where the load has no
 * fp6 operands (negative weights, more than 16,384 sequences, the VALU kernel,
 * or WLD_OPT_SCREEN_FP6 0 and no run since).  Single-device contexts. */
int wld_fp6_weight_codes(wld_ctx *ctx, uint8_t *codes, int *fits_fp4);

/* ---- LD summaries: per-site LD scores and r2 decay by distance (not in the
 * reference; what LD-decay curves and LD-score tools need from every pair) ----
 *
 * wld_run_summary evaluates every pair a < b of the linear chunk range
 * [chunk_begin,chunk_end) (end 0 = all; a pair belongs to chunk (a/256, b/256)
 * as in wld_run_chunks) that is in the context's current window
 * (wld_set_window), and reduces the pairs on the device: no row is produced,
 * staged or copied, so there is no 2^32 pairs-per-run limit and the result is
 * O(n_sites + n_bins) numbers.  Every such pair falls into exactly one class:
 *   none       single_weighted_ld_pair gives None (lib.rs:404-410: a site
 *              without a major or minor symbol);
 *   nonfinite  Some, but r2 is NaN or +-inf;
 *   counted    Some and r2 finite.
 * r2 is the f32 value the default row path (WLD_OPT_REF_SUMS 1) puts in the
 * pair's row, bit for bit: the summary always sums in lib.rs's order.
 * WLD_OPT_REF_SUMS, the kernel choice and the screen options do not apply, and
 * no threshold applies.
 *
 * Outputs (library-allocated; release with wld_summary_free).  Site arrays
 * are indexed by LOADED site index and have n_sites entries:
 *   pairs, none_pairs, nonfinite_pairs, counted_pairs
 *              pairs = none_pairs + nonfinite_pairs + counted_pairs
 *                    = wld_window_pairs_in_chunks(begin, end);
 *   r2_sum     sum of (double) r2 over the counted pairs;
 *   score[i]   sum of (double) r2 over the counted pairs that contain site i
 *              (each pair adds to both of its sites);
 *   partners[i] the number of those pairs; sum_i partners[i] = 2 counted_pairs;
 *   bin_pairs[k], bin_r2_sum[k]  (bin_width > 0 only, n_bins entries each; NULL
 *              otherwise) the counted pairs with
 *              k = min((pos[b] - pos[a]) / bin_width, n_bins - 1) and the sum of
 *              their r2, pos[i] = site_map[i] or i without a map — the distance
 *              the window uses; the last bin also takes everything beyond it;
 *              sum_k bin_pairs[k] = counted_pairs;
 *   kernel_ms  HIP-event time of the summary launch (device group: the
 *              slowest member's).
 * All counts are exact.  The f64 sums are NOT bitwise reproducible from run to
 * run: tiles add to a destination with f64 atomics in whatever order they
 * finish.  Every term is exact ((double) of an f32), so each sum is within the
 * rounding of an any-order f64 sum of its terms: relative error at most about
 * n 2^-53 for n nonnegative terms.  Summaries over disjoint chunk ranges add
 * up to the whole run's (counts exactly, sums to that rounding).
 *
 * On a device group (wld_create_multi) the range is sharded as wld_run_host
 * shards it (wld_shard_chunks / wld_shard_chunks_window), the members run
 * concurrently and their summaries are added on the host in member order.
 *
 * WLD_E_ARG: n_bins > 1024; bin_width > 0 with n_bins == 0; bin_width > 0 on
 * a site_map that descends (the rule of wld_set_window with a distance; the
 * message names the first offending index); non-finite weights (a load that
 * takes the row path's select loop); chunk_begin > chunk_end.  WLD_E_STATE:
 * before a load, or while a run is in flight.  A summary changes nothing a
 * later row run depends on, and wld_last_stats keeps describing the last row
 * run.  No progress callback. */
typedef struct {
    uint64_t n_sites;
    uint64_t bin_width;
    uint32_t n_bins; /* entries of the bin arrays: 0 when bin_width == 0 */
    uint64_t pairs, none_pairs, nonfinite_pairs, counted_pairs;
    double r2_sum;
    double *score;
    uint32_t *partners;
    uint64_t *bin_pairs;
    double *bin_r2_sum;
    double kernel_ms;
} wld_summary;
int wld_run_summary(wld_ctx *ctx, uint32_t chunk_begin, uint32_t chunk_end, uint64_t bin_width, uint32_t n_bins,
                    wld_summary *out);
void wld_summary_free(wld_summary *s);

/* ---- LD heat map: r2 or |D'| reduced on the device over a grid of site
 * cells (not in the reference; the LD heat map of a genome, of one region, or
 * gene x gene) ----
 *
 * wld_run_heatmap reduces every considered pair over a caller-defined grid of
 * n_cells x n_cells cells: per cell the pair count, the sum of the value and
 * its max.  No row is produced, staged or copied; O(n_cells^2) numbers come
 * back, and 64x64 tiles that touch no cell are not computed.
 *
 * site_cell has one entry per LOADED site (wld_loaded_sites): -1 (the site is
 * on no cell) or a cell id < n_cells; the ids must be non-decreasing over the
 * sites that have one.  Gaps of -1 are allowed anywhere, and so are cells
 * without a site.  Equal runs of sites, equal bins of a coordinate, gene
 * boundaries and a zoom on one region are all maps of this kind.
 *
 * A pair a < b of the linear chunk range [chunk_begin,chunk_end) (end 0 =
 * all, as wld_run_summary) is considered iff it is in the context's current
 * window (wld_set_window) and both sites have a cell.  Every considered pair
 * falls into exactly one class:
 *   none       single_weighted_ld_pair gives None;
 *   nonfinite  Some, but the chosen value is NaN or +-inf;
 *   counted    Some and the value finite.
 * A counted pair adds to cell (site_cell[a], site_cell[b]) — always row <=
 * column; the lower triangle stays at count 0, sum 0, max NaN.  The value is
 * the f32 the default row path (WLD_OPT_REF_SUMS 1) puts in the pair's row,
 * bit for bit: r2 (WLD_HEAT_R2) or fabsf of its d_prime (WLD_HEAT_ABS_DPRIME);
 * the heat map always sums in lib.rs's order.  WLD_OPT_REF_SUMS, the kernel
 * choice and the screen options do not apply, and no threshold applies.
 *
 * Outputs (library-allocated; release with wld_heatmap_free), n_cells x
 * n_cells each, row-major [i * n_cells + j]:
 *   pairs, none_pairs, nonfinite_pairs, counted_pairs
 *              pairs = none_pairs + nonfinite_pairs + counted_pairs;
 *   count      the counted pairs of the cell; their sum is counted_pairs;
 *   sum        the sum of (double) value over them;
 *   max        their largest value, ordered as floats over ALL finite values
 *              (an f32 r2 can come out slightly negative); NaN where count
 *              is 0;
 *   tiles      the 64x64 tiles launched: those of the range and window whose
 *              row block and column block both hold a site with a cell;
 *   kernel_ms  HIP-event time of the launch (device group: the slowest
 *              member's).
 * The result depends only on the set of considered pairs, not on the order in
 * which tiles finish: count and max are exact and identical from run to run,
 * across splits of the chunk range and across device groups.  The f64 sums are
 * NOT bitwise reproducible from run to run: tiles add to a cell with f64
 * atomics in whatever order they finish.  Every term is exact ((double) of an
 * f32), so each sum is within the rounding of an any-order f64 sum of its
 * terms: relative error at most about n 2^-53 for n nonnegative terms.  Heat
 * maps over disjoint chunk ranges combine to the whole run's: counts add, max
 * is the max of the parts, sums agree to that rounding.
 *
 * On a device group (wld_create_multi) the range is sharded exactly as
 * wld_run_summary shards it, the members run concurrently and their maps are
 * merged on the host in member order.
 *
 * WLD_E_ARG: n_cells == 0 or > WLD_HEAT_MAX_CELLS; an unknown stat; site_cell
 * NULL; an id >= n_cells, an id < -1 or a descending id (the message names
 * the first offending index); non-finite weights (a load that takes the row
 * path's select loop); chunk_begin > chunk_end.  WLD_E_STATE: before a load,
 * or while a run is in flight.  WLD_E_OOM leaves the context usable.  A heat
 * map changes nothing a later row run depends on — it keeps its tile list in
 * a buffer of its own — and wld_last_stats and the last run's rows stay as
 * they were.  No progress callback. */
#define WLD_HEAT_R2 0         /* value = r2 */
#define WLD_HEAT_ABS_DPRIME 1 /* value = fabsf(d_prime) */
#define WLD_HEAT_MAX_CELLS 4096
typedef struct {
    uint32_t n_cells;
    int stat;
    uint64_t pairs, none_pairs, nonfinite_pairs, counted_pairs;
    uint64_t *count; /* n_cells*n_cells, row-major [i*n_cells + j] */
    double *sum;     /* same shape */
    float *max;      /* same shape; NaN where count == 0 */
    uint64_t tiles;  /* 64x64 tiles launched */
    double kernel_ms; /* HIP-event time of the launch (device group: slowest member) */
} wld_heatmap;
int wld_run_heatmap(wld_ctx *ctx, const int32_t *site_cell, uint32_t n_cells, int stat, uint32_t chunk_begin,
                    uint32_t chunk_end, wld_heatmap *out);
void wld_heatmap_free(wld_heatmap *h);

/* ---- Partitioned LD scores: sum of r2 times site annotations, reduced on the
 * device (not in the reference; what stratified LD-score regression,
 * partitioned heritability and annotation-aware PRS need: LDSC's --l2 --annot) ----
 *
 * wld_run_annot_scores computes, for every loaded site i and every column c of
 * a caller-given annotation matrix,
 *     score[i][c] = sum over the counted pairs {i, k} of r2(i, k) annot[k][c].
 * annot is a host array of n_sites x n_annot floats, row-major
 * [site * n_annot + c], indexed by LOADED site index (wld_loaded_sites): binary
 * or continuous, any sign, all finite; 1 <= n_annot <= WLD_ANNOT_MAX.  It goes
 * to the device once per call.  No row is produced, staged or copied.
 *
 * The considered pairs and their classes are exactly wld_run_summary's: every
 * pair a < b of the linear chunk range [chunk_begin,chunk_end) (end 0 = all)
 * that is in the context's current window (wld_set_window) is none, nonfinite
 * or counted.  r2 is the f32 value the default row path (WLD_OPT_REF_SUMS 1)
 * puts in the pair's row, bit for bit.  WLD_OPT_REF_SUMS, the kernel choice and
 * the screen options do not apply, and no threshold applies.  pairs, the three
 * class counts and partners[] equal wld_run_summary's for the same range and
 * window, exactly.
 *
 * Outputs (library-allocated; release with wld_annot_scores_free), indexed by
 * LOADED site index:
 *   pairs, none_pairs, nonfinite_pairs, counted_pairs   as wld_summary's;
 *   score      n_sites x n_annot, row-major [site * n_annot + c].  A counted
 *              pair (a, b) adds (double) r2 * (double) annot[b][c] to
 *              score[a][c] and (double) r2 * (double) annot[a][c] to
 *              score[b][c];
 *   partners[i] the counted pairs that contain site i (the self term is not
 *              one);
 *   tiles      the 64x64 tiles launched;
 *   kernel_ms  HIP-event time of the launch (device group: the slowest
 *              member's).
 * With WLD_ANNOT_SELF in flags (LDSC counts r2(i, i) = 1) site i additionally
 * gets the term (double) annot[i][c], iff the site has a major and a minor
 * symbol (the sites whose pairs are not all none) and its diagonal chunk
 * (i/256, i/256) lies in the chunk range — so results over disjoint ranges
 * still combine without counting it twice.
 *
 * All counts are exact.  Every term is exact (the product of two 24-bit
 * significands fits in 53 bits).  The sums are any-order f64 sums — products
 * accumulated per tile, tiles added with f64 atomics in whatever order they
 * finish — and NOT bitwise reproducible from run to run.  Each is a chain of
 * f64 roundings over its terms: for annotations of any sign
 *     |score[i][c] - exact| <= n 2^-52 sum |term|,
 * n the site's term count (partners[i], + 1 with the self term) and the sum
 * over the absolute values of its terms.
 *
 * wld_annot_scores_merge adds `from` into `into`: counts, scores, partners and
 * tiles by addition, kernel_ms the larger.  Results over disjoint chunk ranges
 * merge to the whole run's (counts exactly, scores to the bound above).
 * WLD_E_ARG when n_sites, n_annot or flags differ.
 *
 * On a device group (wld_create_multi) the range is sharded exactly as
 * wld_run_summary shards it, the members run concurrently and their results
 * are merged on the host in member order.
 *
 * WLD_E_ARG: n_annot == 0 or > WLD_ANNOT_MAX; annot NULL; a non-finite
 * annotation value (the message names the first offending site and column);
 * unknown flag bits; chunk_begin > chunk_end; non-finite weights (a load that
 * takes the row path's select loop).  WLD_E_STATE: before a load, or while a
 * run is in flight.  WLD_E_OOM leaves the context usable.  The call keeps its
 * tile list, image and accumulators in buffers of its own: it changes nothing
 * a later row run depends on, and wld_last_stats and the last run's rows stay
 * as they were.  No progress callback. */
#define WLD_ANNOT_MAX 128
#define WLD_ANNOT_SELF 1 /* flags: every site with both symbols also counts r2(i, i) = 1 */
typedef struct {
    uint64_t n_sites;
    uint32_t n_annot;
    int flags;
    uint64_t pairs, none_pairs, nonfinite_pairs, counted_pairs;
    double *score;      /* n_sites*n_annot, row-major [site*n_annot + c], LOADED site index */
    uint32_t *partners; /* n_sites */
    uint64_t tiles;     /* 64x64 tiles launched */
    double kernel_ms;   /* HIP-event time of the launch (device group: slowest member) */
} wld_annot_scores;
int wld_run_annot_scores(wld_ctx *ctx, const float *annot /* n_sites*n_annot, row-major, host */, uint32_t n_annot,
                         int flags, uint32_t chunk_begin, uint32_t chunk_end, wld_annot_scores *out);
int wld_annot_scores_merge(wld_annot_scores *into, const wld_annot_scores *from);
void wld_annot_scores_free(wld_annot_scores *s);

/* ---- LD matrix: dense r, r2, D or D' of a site rectangle (not in the
 * reference; PLINK's --r square / --r2 square, LDstore, LDlink's LDmatrix: what
 * fine-mapping, summary-statistic imputation, conditional analysis and PRS
 * samplers start from) ----
 *
 * Rectangle.  Rows [row_begin,row_end) and columns [col_begin,col_end) are
 * LOADED site indices (wld_loaded_sites); an end of 0 means the loaded site
 * count.  Entry (i, j) is dst[i * ld + j] (ld in elements, >= the width) and
 * belongs to the sites u = row_begin + i, v = col_begin + j.  The rectangle may
 * lie above, below or across the diagonal and need not be aligned to anything.
 *
 * Off the diagonal, with a = min(u, v), b = max(u, v):
 *   * pair (a, b) in the context's window (wld_set_window; none: every pair):
 *     the value is computed from the f32 d, d', r2 that the default row path
 *     (WLD_OPT_REF_SUMS 1) puts in the row of pair (a, b), bit for bit.  Pair
 *     (b, a) is never evaluated (the row path's f32 values are not symmetric
 *     in their arguments): entries (u, v) and (v, u) hold the same bits.
 *       WLD_MATRIX_R2, _D, _DPRIME   that r2, d, d';
 *       WLD_MATRIX_R   s = sqrtf(r2), correctly rounded, r = (d > 0) ? -s : s.
 *     d carries the REFERENCE's sign, expected minus observed (lib.rs:502),
 *     the opposite of the textbook D; WLD_MATRIX_R undoes that: r is the
 *     weighted Pearson correlation of the two sites' major-allele indicators
 *     over the sequences in the pair's mask (both sites major or minor).
 *     WLD_MATRIX_D and _DPRIME keep the reference's sign.  r2 is not clamped:
 *     rounding can leave it a few ulps above 1 (1.0000001), and r with it.
 *   * a none pair (a site without a major or a minor symbol): NaN;
 *   * a nonfinite pair: what the arithmetic gave (NaN or +-inf);
 *   * out of the window: +0.0 (the matrix is banded).
 * On the diagonal: 1.0 for _R2 and _R where the site has a major and a minor
 * symbol, NaN otherwise; NaN for _D and _DPRIME.
 * WLD_MATRIX_ZERO_MISSING (flags): every entry that would be NaN or +-inf
 * becomes +0.0, except the _R / _R2 diagonal, which becomes 1.0.
 * WLD_MATRIX_F16: the f32 value rounded to nearest-even to IEEE binary16,
 * subnormal results kept (numpy's astype(float16)).
 *
 * Info.  pairs, none_pairs, nonfinite_pairs, counted_pairs: the distinct pairs
 * a < b in the window with an entry in the rectangle — a pair with both
 * orientations inside counts once — classified as wld_run_summary classifies
 * them (by r2); for the full square they equal the summary's for the same
 * window.  tiles: the 64x64 tiles launched.  kernel_ms: HIP-event time of the
 * fill and pair launches (wld_run_matrix: summed over its bands).
 *
 * Every element inside the rectangle is written; nothing outside it is
 * touched, the ld - width elements between rows included.  No value goes
 * through an atomic: two calls give identical bytes.
 *
 * wld_run_matrix_device: d_dst is device memory of the context's device (a
 * torch tensor's, say); the call returns after its work has completed.
 * wld_run_matrix: h_dst is host memory, written through bands of whole rows
 * from a device buffer the call owns, at most WLD_OPT_MATRIX_BATCH_BYTES
 * (tiles whose two images fall into different bands are computed once per
 * band).  WLD_OPT_REF_SUMS, the kernel choice and the screen options do not
 * apply.
 *
 * WLD_E_ARG: an empty or out-of-range rectangle; an unknown stat, dtype or
 * flag bit; ld below the width; a null destination; non-finite weights (a load
 * that takes the row path's select loop).  WLD_E_STATE: before a load, while a
 * run is in flight, on a device group.  WLD_E_OOM leaves the context usable.
 * The calls keep their tile lists, counters and events to themselves:
 * wld_last_stats, the last run's rows and the row path's cached tile list stay
 * as they were. */
#define WLD_MATRIX_R2 0
#define WLD_MATRIX_R 1 /* signed */
#define WLD_MATRIX_D 2
#define WLD_MATRIX_DPRIME 3
#define WLD_MATRIX_F32 0
#define WLD_MATRIX_F16 1
#define WLD_MATRIX_ZERO_MISSING 1 /* flags */
typedef struct {
    uint32_t row_begin, row_end, col_begin, col_end; /* as resolved */
    int stat, dtype, flags;
    uint64_t pairs, none_pairs, nonfinite_pairs, counted_pairs;
    uint64_t tiles;   /* 64x64 tiles launched */
    double kernel_ms; /* HIP-event time of the launches */
} wld_matrix_info;
int wld_run_matrix_device(wld_ctx *ctx, uint32_t row_begin, uint32_t row_end, uint32_t col_begin, uint32_t col_end,
                          int stat, int dtype, int flags, void *d_dst, size_t ld /* elements */, wld_matrix_info *out);
int wld_run_matrix(wld_ctx *ctx, uint32_t row_begin, uint32_t row_end, uint32_t col_begin, uint32_t col_end, int stat,
                   int dtype, int flags, void *h_dst, size_t ld /* elements */, wld_matrix_info *out);

/* ---- Banded LD matrix: band storage of a windowed matrix, and its product
 * with a block of vectors (not in the reference; LAPACK's upper band storage
 * by rows: what fine-mapping, imputation and PRS sweeps multiply with, at the
 * band's size instead of the square's) ----
 *
 * Layout.  Rows [row_begin,row_end) are LOADED site indices (an end of 0 means
 * the loaded site count) and K = bandwidth.  For u in the rows and k = 0..K,
 * dst[(u - row_begin) * ld + k] (ld in elements, >= K + 1) is entry (u, u + k)
 * of the matrix wld_run_matrix_device defines under the context's current
 * window: the same stat (WLD_MATRIX_R2 / _R / _D / _DPRIME, the same signed-r
 * rule), at k = 0 the same diagonal rule, NaN for a none pair, +0.0 out of the
 * window, WLD_MATRIX_ZERO_MISSING and the WLD_MATRIX_F32 / _F16 rounding, bit
 * for bit.  Elements with u + k >= the loaded site count are +0.0.  Pair
 * (a, b), a < b, is evaluated once, as (a, b), and stored once, in row a; no
 * value goes through an atomic: two calls give identical bytes.  Every element
 * of the [rows] x [K + 1] block is written and nothing else is touched, the
 * ld - (K + 1) elements between rows included.
 *
 * Width.  wld_matrix_banded_width gives K_needed = max over a of hi[a] - a for
 * the window's limits hi (wld_window_limits_copy's; a max_distance-only window
 * too); without a window, the loaded site count - 1.  bandwidth < K_needed is
 * refused (WLD_E_ARG, the message names the width needed): a band that drops
 * in-window pairs is never produced.  bandwidth > K_needed is allowed; the
 * surplus is +0.0.
 *
 * Info.  pairs, none_pairs, nonfinite_pairs, counted_pairs: the in-window
 * pairs a < b with a in [row_begin,row_end), classified as wld_run_summary
 * classifies them; for all rows they equal the summary's for the same window.
 * tiles: the 64x64 tiles launched.  kernel_ms: HIP-event time of the fill and
 * pair launches (wld_run_matrix_banded: summed over its strips).
 *
 * wld_run_matrix_banded_device: d_dst is device memory of the context's
 * device; the call returns after its work has completed.
 * wld_run_matrix_banded: h_dst is host memory, written through strips of
 * whole rows from a device buffer the call owns, at most
 * WLD_OPT_MATRIX_BATCH_BYTES (64 rows at least); a pair belongs to the strip of
 * its row a, so a tile is computed once per strip it meets.
 *
 * Tile indices are 16-bit: more than 4,194,304 loaded sites are refused.
 * Refusals and state rules are wld_run_matrix_device's (WLD_E_ARG: an empty or
 * out-of-range row range, an unknown stat, dtype or flag bit, ld < K + 1, a
 * null destination, a short bandwidth, non-finite weights; WLD_E_STATE: before
 * a load, while a run is in flight, on a device group).  The calls keep their
 * lists, counters and events to themselves: wld_last_stats, the last run's
 * rows and the row path's cached tile list stay as they were. */
typedef struct {
    uint32_t row_begin, row_end; /* as resolved */
    uint32_t bandwidth;
    int stat, dtype, flags;
    uint64_t pairs, none_pairs, nonfinite_pairs, counted_pairs;
    uint64_t tiles;   /* 64x64 tiles launched */
    double kernel_ms; /* HIP-event time of the launches */
} wld_matrix_banded_info;
int wld_matrix_banded_width(wld_ctx *ctx, uint32_t *bandwidth_needed);
int wld_run_matrix_banded_device(wld_ctx *ctx, uint32_t row_begin, uint32_t row_end, uint32_t bandwidth, int stat,
                                 int dtype, int flags, void *d_dst, size_t ld /* elements */,
                                 wld_matrix_banded_info *out);
int wld_run_matrix_banded(wld_ctx *ctx, uint32_t row_begin, uint32_t row_end, uint32_t bandwidth, int stat, int dtype,
                          int flags, void *h_dst, size_t ld /* elements */, wld_matrix_banded_info *out);

/* Band product.  Y = S X for the symmetric n_sites x n_sites matrix S whose
 * upper band is d_band in the layout above with ALL rows present (row_begin
 * 0, row_end n_sites): for every site i and column c,
 *
 *   Y[i][c] = sum_{k=0..K, i+k<n} B[i][k] X[i+k][c]
 *           + sum_{k=1..min(K,i)}  B[i-k][k] X[i-k][c]
 *
 * d_band: WLD_MATRIX_F32 or _F16 (band_dtype), ld >= K + 1 elements per row.
 * d_x: WLD_APPLY_X_F32 or _F64 (x_dtype), row-major [n_sites][ldx], ldx >=
 * n_cols.  d_y: double, [n_sites][ldy], ldy >= n_cols, overwritten (only its
 * n_cols columns).  n_cols >= 1 with no upper limit.  All three are device
 * memory of the context's device and must not overlap; the context supplies
 * the device and the stream only: no load is needed and n_sites is the
 * caller's.  The call returns after its work has completed.
 *
 * Deterministic: every Y element is summed by one owner in a fixed order, in
 * f64, without atomics; two calls give identical bytes.  With float X every
 * product is exact and |Y - exact| <= n 2^-52 sum|term| (n the element's term
 * count); with double X each product is rounded once.
 * Band elements with i + k >= n_sites are never read.  The device data is not
 * validated: a non-finite band value propagates by IEEE rules to the rows i
 * and i + k it belongs to (WLD_MATRIX_ZERO_MISSING avoids them), and X must be
 * finite: the product runs on 64x64 blocks padded with zeros, so a non-finite
 * X entry can reach any output within 64 + K sites of it.
 *
 * WLD_E_ARG: a null pointer, n_sites or n_cols 0, ld < K + 1, ldx or ldy <
 * n_cols, an unknown dtype.  WLD_E_STATE: while a run is in flight, on a device
 * group. */
#define WLD_APPLY_X_F32 0
#define WLD_APPLY_X_F64 1
int wld_banded_apply_device(wld_ctx *ctx, const void *d_band, int band_dtype, size_t ld, uint32_t n_sites,
                            uint32_t bandwidth, const void *d_x, int x_dtype, size_t ldx, uint32_t n_cols, double *d_y,
                            size_t ldy);

/* The banded Cholesky factorisation and its triangular solves, on the device.
 * Like wld_banded_apply_device the context supplies only the device and the
 * stream; no load is needed, n_sites is the caller's, every pointer is device
 * memory of the context's device, and each call returns after its work has
 * completed.
 *
 * Matrix.  A is the symmetric matrix of the band d_band as wld_banded_apply_
 * device reads it (WLD_MATRIX_F32 or _F16, ld >= K + 1, elements with i + k >=
 * n_sites never read), every element converted to f64, with the diagonal
 * fl(fl(B[i][0] + ridge) + d_diag[i]) (the second addition skipped when d_diag
 * is NULL).  That rounded value is the definition of A.
 *
 * Factor.  A = U^T U, U upper triangular with U[i][i] > 0, in the same band
 * layout in f64: d_factor[i * ldf + k] = U(i, i + k), ldf >= K + 1.  Every
 * element of [n_sites] x [K + 1] is written, those with i + k >= n_sites with
 * +0.0; nothing else is touched, the padding between rows included.  d_factor
 * must not overlap the band.  Every element is produced by one owner in a
 * fixed order without atomics: two calls give identical bytes.
 *
 * A matrix that is not positive definite is a result, not an error: where a
 * pivot is not > 0 (NaN included) the call returns WLD_OK with first_bad = that
 * row; the factor's rows [0, 64 * floor(first_bad / 64)) are the valid factor
 * rows of the leading block, the rest is unspecified.  No pivot is replaced.
 *
 * Solve.  wld_banded_solve_device overwrites the n_cols columns of d_b
 * ([n_sites][ldb] f64, ldb >= n_cols, n_cols >= 1 with no upper limit) with the
 * solution of U^T y = b (WLD_SOLVE_FORWARD), U x = y (_BACKWARD) or A x = b
 * (_FULL: forward, then backward).  Diagonal blocks are solved by
 * substitution, never through an inverse.  Neither the factor nor b is
 * validated; non-finite values propagate (the solve runs on 64x64 blocks
 * padded with zeros, so a non-finite entry can reach any row within 64 + K
 * sites of it).  Deterministic as above.  For e ~ N(0, I) the _BACKWARD
 * solution has covariance A^-1; the _FORWARD solution of b ~ N(0, A) is white.
 *
 * WLD_E_ARG: a null pointer, n_sites or n_cols 0, ld or ldf < K + 1, ldb <
 * n_cols, an unknown dtype or mode, a non-finite ridge, d_factor overlapping
 * d_band.  WLD_E_STATE: while a run is in flight, on a device group.
 * wld_last_stats, the last run's rows and every cached list stay as they were. */
typedef struct {
    uint32_t n_sites, bandwidth;
    uint32_t first_bad; /* n_sites: positive definite; else the first row whose pivot was not > 0 (NaN included) */
    double min_pivot;   /* smallest U[i][0] over the rows factored (a conditioning hint) */
    double kernel_ms;   /* HIP-event time of the launches */
} wld_banded_chol_info;

int wld_banded_cholesky_device(wld_ctx *ctx, const void *d_band, int band_dtype, size_t ld, uint32_t n_sites,
                               uint32_t bandwidth, double ridge, const double *d_diag /* n_sites, may be NULL */,
                               double *d_factor, size_t ldf, wld_banded_chol_info *out);

#define WLD_SOLVE_FULL 0     /* A x = b   */
#define WLD_SOLVE_FORWARD 1  /* U^T y = b */
#define WLD_SOLVE_BACKWARD 2 /* U x = y   */
int wld_banded_solve_device(wld_ctx *ctx, const double *d_factor, size_t ldf, uint32_t n_sites, uint32_t bandwidth,
                            int mode, double *d_b /* [n_sites][ldb], overwritten by the solution */, size_t ldb,
                            uint32_t n_cols, double *kernel_ms /* may be NULL */);

/* ---- Sweep scan: Kim and Nielsen's omega and Kelly's ZnS from an r2 band (not
 * in the reference; OmegaPlus) ----
 * Every value below is one fixed sequence of IEEE f64 operations; the numpy
 * twins of the Python package (banded_pairsum_host, banded_omega_host) perform
 * the same sequence, and the device results equal them bit for bit.
 *
 * Pair sums.  wld_banded_pairsum_device reads a band as wld_banded_apply_device
 * does (WLD_MATRIX_F32 or _F16, ld >= K + 1; elements with j + k >= n_sites and
 * column 0 are never read) and writes the table M in the same layout in f64
 * (d_sums[j * lds_ + k] = M[j][k], lds_ >= K + 1).  With b(j, k) = f64(B[j][k])
 * where that is finite, else +0.0:
 *   P[j][0] = 0,  P[j][k] = P[j][k-1] + b(j, k)   k = 1..K in that order,
 *   M[j][0] = 0,  M[j][k] = M[j+1][k-1] + P[j][k],
 * so M[j][k] is the sum of the entries (u, v), j <= u < v <= j + k.  Elements
 * with j + k >= n_sites are +0.0.  Every element of [n_sites] x [K + 1] is
 * written, nothing else, the padding between rows included; d_sums must not
 * overlap the band.  Each element has one owner and one order: two calls give
 * identical bytes.  Like wld_banded_apply_device the context supplies only the
 * device and the stream; no load is needed.
 *
 * Scan.  wld_banded_omega_device takes such a table and n_splits splits; entry
 * g is the split between the sites c = d_split[g] and c + 1, its left flank the
 * sites a..c with d_lo[g] <= a, its right flank c+1..b with b <= d_hi[g], both
 * flanks at least min_side >= 2 sites.  For a candidate (a, b), l = c - a + 1,
 * r = b - c:
 *   SL = M[a][c-a]   SR = M[c+1][b-c-1]   ST = M[a][b-a]   X = (ST - SL) - SR
 *   t1 = (SL + SR) / f64(l(l-1)/2 + r(r-1)/2)     t2 = X / f64(l r) + eps
 *   omega = t1 / t2, the candidate skipped (and counted) unless t2 > 0.
 * d_omega[g] is the largest omega of the split's candidates, d_left[g] and
 * d_right[g] its (a, b); among equal omega the smallest a wins, then the
 * smallest b.  A split without an unskipped candidate gives NaN, UINT32_MAX,
 * UINT32_MAX.  d_zns[g] = M[lo][hi-lo] / f64(w(w-1)/2), w = hi - lo + 1.  Splits
 * may repeat and come in any order.  The device arrays are validated by a small
 * launch before the scan: every split needs lo <= c < hi < n_sites and hi - lo
 * <= bandwidth, else WLD_E_ARG naming the first offender, and nothing is
 * written.  The table's values are not validated.  The outputs must not overlap
 * the table or the split arrays (not checked).
 *
 * WLD_E_ARG: a null pointer, n_sites or n_splits 0, ld or lds_ < K + 1, an
 * unknown dtype, d_sums overlapping d_band, min_side < 2, eps negative or not
 * finite, a bad split.  WLD_E_STATE: while a run is in flight, on a device
 * group.  wld_last_stats, the last run's rows and every cached list stay as
 * they were. */
typedef struct {
    uint32_t n_sites, bandwidth;
    uint64_t nonfinite; /* band elements (k >= 1, i + k < n_sites) that were NaN or +-inf and counted as 0 */
    double kernel_ms;
} wld_banded_pairsum_info;
int wld_banded_pairsum_device(wld_ctx *ctx, const void *d_band, int band_dtype, size_t ld, uint32_t n_sites,
                              uint32_t bandwidth, double *d_sums, size_t lds_, wld_banded_pairsum_info *out);

typedef struct {
    uint32_t n_splits;
    uint64_t evaluated, skipped; /* candidate border pairs with t2 > 0 / without */
    double kernel_ms;
} wld_banded_omega_info;
int wld_banded_omega_device(wld_ctx *ctx, const double *d_sums, size_t lds_, uint32_t n_sites, uint32_t bandwidth,
                            const uint32_t *d_split, const uint32_t *d_lo, const uint32_t *d_hi, uint32_t n_splits,
                            uint32_t min_side, double eps, double *d_omega, uint32_t *d_left, uint32_t *d_right,
                            double *d_zns, wld_banded_omega_info *out);

/* The splits of a scan from coordinates; host only, no device.  site_map: the
 * n_sites >= 2 coordinates, non-decreasing as wld_set_window requires (NULL:
 * site_map[i] = i).  n_grid 0: every split c = 0..n_sites-2 at position
 * site_map[c]; n_grid >= 1: the equidistant positions x_g = site_map[0] +
 * floor(span g / (n_grid - 1)) (n_grid 1: the midpoint), c the last site with
 * coordinate <= x_g, clamped to [0, n_sites - 2].  lo = max(c - max_side + 1,
 * first site with coordinate >= x_g - max_distance), at most c; hi = min(c +
 * max_side, last site with coordinate <= x_g + max_distance, n_sites - 1), at
 * least c + 1; max_distance 0: no distance limit.  Writes wld_omega_n_splits
 * entries of each output.  WLD_E_ARG: a null output, n_sites < 2, max_side 0, a
 * descending site_map. */
uint64_t wld_omega_n_splits(uint32_t n_sites, uint32_t n_grid);
int wld_omega_splits(const uint64_t *site_map, uint32_t n_sites, uint32_t n_grid, uint32_t max_side,
                     uint64_t max_distance, uint64_t *position, uint32_t *split, uint32_t *lo, uint32_t *hi);

/* The whole scan on a loaded single-device context: the splits from the load's
 * site_map (wld_omega_splits), an r2 band with WLD_MATRIX_ZERO_MISSING of width
 * wld_matrix_banded_width under the context's CURRENT window in a buffer the
 * call owns, its pair sums, the scan, and the results on the host (malloc'ed;
 * wld_omega_free).  A split whose sites lo..hi are not all in each other's
 * window is refused with WLD_E_ARG (the window would drop pairs the scan
 * needs): a window of max_sites >= 2 max_side - 1 (and no max_distance) always
 * suffices, and the message names that number.  WLD_E_OOM leaves the context
 * usable.  wld_last_stats and the last run's rows stay as they were. */
typedef struct {
    uint32_t n_sites, bandwidth, n_splits, min_side;
    uint64_t *position;            /* [n_splits] the splits' coordinates */
    uint32_t *split, *lo, *hi;     /* [n_splits] loaded site indices */
    double *omega;                 /* [n_splits] NaN: no candidate */
    uint32_t *left, *right;        /* [n_splits] the best borders, UINT32_MAX: none */
    double *zns;                   /* [n_splits] */
    wld_matrix_banded_info band;   /* the band fill: its pair counts and time */
    wld_banded_pairsum_info sums;
    wld_banded_omega_info scan;
} wld_omega;
int wld_run_omega(wld_ctx *ctx, uint32_t n_grid, uint32_t max_side, uint32_t min_side, uint64_t max_distance, double eps,
                  int band_dtype, wld_omega *out);
void wld_omega_free(wld_omega *o);

/* ---- LD pruning: a greedy r2-independent site set with tags (not in the
 * reference; PLINK's --indep-pairwise, bcftools +prune) ----
 *
 * Graph.  The vertices are the loaded sites 0..L-1.  {a, b} is an edge iff the
 * context, as configured now (window, kernel choice, WLD_OPT_REF_SUMS and every
 * other option), would return a row for that pair from
 * wld_run_host(ctx, r2_threshold, ...): the pair is in the window,
 * single_weighted_ld_pair gives Some, and r2 > r2_threshold strictly (NaN is
 * never an edge).  A site without a statistic has no edge.
 *
 * Order.  priority is NULL (index order) or n_sites floats: site u comes
 * before v iff priority[u] > priority[v], or they compare equal (-0.0 and 0.0
 * do) and u < v.  +-inf are allowed; a NaN gives WLD_E_ARG naming the first
 * offending index.  The host turns the order into ranks (0 = first) with a
 * stable sort; the device compares ranks only.
 *
 * Result.  The kept set is what sequential greedy selection gives — the
 * lexicographically first maximal independent set under the order: visit the
 * sites by rank, keep a site iff none of its neighbours has been kept.
 *   keep[i]  1 kept, 0 removed; a site without edges is kept;
 *   tag[i]   i for a kept site; for a removed site the LOADED index of its kept
 *            neighbour with the smallest rank (one always exists and ranks
 *            before i);
 *   n_kept   the number of kept sites; edges: the rows at this threshold and
 *            window;
 *   rounds   decide launches enqueued (0 iff edges == 0); depends on
 *            scheduling, not reproducible;
 *   pair_ms  HIP-event time of the row passes (pair phase + ordering, summed
 *            over the batches); prune_ms: of the CSR build, the rounds and
 *            the tags (wld_prune_times splits it).
 * keep, tag, n_kept and edges are a function of the graph and the order alone:
 * identical from run to run and independent of batch sizes
 * (WLD_OPT_HOST_BATCH_PAIRS), staging capacity, the screen chosen and
 * scheduling.  The device runs the parallel form of sequential greedy (rounds
 * of separate launches over a CSR of each site's better-ranked neighbours;
 * DESIGN.md 4.8) and copies back O(n_sites) numbers; no row leaves the device.
 *
 * The edges come from the row path: the chunk sequence runs in wld_run_host's
 * batches, the rows' site columns staying on the device as loaded indices.
 * Afterwards the context holds no rows (wld_rows_* return WLD_E_STATE until
 * the next run, whose rows carry parent indices again) and wld_last_stats
 * describes the last batch's row run.
 *
 * WLD_E_STATE: before a load, while a run is in flight, on a device group.
 * WLD_E_ARG: a NaN priority; more than 2^31 - 1 edges (raise the threshold or
 * narrow the window).  WLD_E_OOM: the edge buffers (12 bytes per edge) cannot
 * be allocated; the context stays usable.  No progress callback.  Release
 * keep/tag with wld_prune_free. */
typedef struct {
    uint64_t n_sites, n_kept, edges;   /* edges = rows at this threshold and window */
    uint32_t rounds;                   /* decide launches enqueued; 0 iff edges == 0; not reproducible */
    uint8_t  *keep;                    /* n_sites */
    uint32_t *tag;                     /* n_sites, loaded indices */
    double pair_ms, prune_ms;          /* HIP-event time: the row passes; CSR build + rounds + tags */
} wld_prune;
int  wld_run_prune(wld_ctx *ctx, float r2_threshold, const float *priority, wld_prune *out);
/* The loaded set's site count — the length of priority, keep and tag (0 before
 * a load; a device group: its members'). */
size_t wld_loaded_sites(const wld_ctx *ctx);
void wld_prune_free(wld_prune *p);
/* The last wld_run_prune's prune_ms by phase (HIP-event time; 0 when it had no
 * edge): the CSR build, the rounds (with the host's reads of the undecided
 * count between them), the tags.  Any pointer may be NULL. */
int wld_prune_times(wld_ctx *ctx, double *csr_ms, double *rounds_ms, double *tags_ms);

/* ---- Target sites: the rows of chosen sites against every in-window partner
 * (not in the reference; PLINK's --ld-snp / --ld-snps / --ld-snp-list, a proxy
 * search, the r2 track of a regional plot) ----
 *
 * targets: n_targets LOADED indices of the loaded set, in any order, without
 * repeats.  For target t and every loaded site s != t, with a = min(s, t) and
 * b = max(s, t), there is a row iff the pair (a, b) is in the context's
 * current window (wld_set_window; symmetric about a target),
 * single_weighted_ld_pair gives Some, and r2 > r2_threshold strictly (NaN
 * never passes).  d, d_prime and r2 are, bit for bit, what the default row
 * path (WLD_OPT_REF_SUMS 1) puts in the row of pair (a, b), whichever side of
 * the target the partner lies on: the result always comes from lib.rs's
 * summation order; the kernel choice, WLD_OPT_REF_SUMS and the screen options
 * do not apply.  The work is n_targets x n_sites pairs (one pass over the
 * resident codes per 16 targets), not the triangle.
 *
 * Rows are ordered by position in the caller's list, then by the partner's
 * loaded index ascending; target k's rows are [offset[k], offset[k + 1]).  A
 * pair of two targets appears once under each.  site_target / site_partner
 * are PARENT indices, target[] the list position k.
 *   items     work items launched: the (block of 16 targets in loaded order,
 *             64-site partner tile) pairs whose tile holds an in-window
 *             partner of a target of the block;
 *   batches   the staging's batches (WLD_OPT_TARGET_BATCH_SLOTS);
 *   kernel_ms HIP-event time of the pair launches, summed over the batches.
 * Everything but kernel_ms is a function of the load, the window, the list and
 * the threshold: identical from run to run and across batch sizes.  The call
 * changes nothing a later row run depends on; the last run's rows and
 * wld_last_stats stay as they were.
 *
 * n_targets == 0: WLD_OK, no rows (offset[0] = 0).  WLD_E_ARG, naming the
 * first offending list position: a target >= the loaded site count; a repeated
 * target.  WLD_E_ARG also: targets == NULL with n_targets > 0; non-finite
 * weights (a load that takes the row path's select loop); n_targets x
 * (n_sites - 1) > 2^32 - 1 (split the list).  WLD_E_STATE: before a load,
 * while a run is in flight, on a device group.  WLD_E_OOM leaves the context
 * usable.  No progress callback.  Release with wld_target_rows_free. */
typedef struct {
    uint64_t n;             /* rows */
    uint32_t n_targets;
    uint64_t *offset;       /* n_targets + 1: target k's rows are [offset[k], offset[k+1]) */
    uint32_t *target;       /* n: index k into the caller's list */
    uint32_t *site_target;  /* n: PARENT index of the target  */
    uint32_t *site_partner; /* n: PARENT index of the partner */
    float *d, *d_prime, *r2;
    uint64_t items;         /* work items launched */
    uint32_t batches;
    double kernel_ms;       /* HIP-event time of the pair launches, summed over batches */
} wld_target_rows;
int  wld_run_targets(wld_ctx *ctx, const uint32_t *targets, uint32_t n_targets,
                     float r2_threshold, wld_target_rows *out);
void wld_target_rows_free(wld_target_rows *r);

/* ---- Best partners: the k strongest in-window LD partners of every site
 * (not in the reference; the all-sites form of a proxy search: tag-SNP
 * selection, imputation-panel design, the k-nearest-neighbour graph that
 * clustering sites by LD starts from) ----
 *
 * wld_run_partners(ctx, k, r2_threshold, chunk_begin, chunk_end, &out) with
 * 1 <= k <= WLD_PARTNERS_MAX_K.  For LOADED site s, a site p != s is a
 * candidate iff the pair (a, b) = (min(s, p), max(s, p))
 *   - lies in the linear chunk range [chunk_begin,chunk_end) (end 0 = all, as
 *     wld_run_summary; a pair belongs to chunk (a/256, b/256)),
 *   - lies in the context's current window (wld_set_window),
 *   - has a statistic (single_weighted_ld_pair gives Some), and
 *   - has r2 > r2_threshold strictly; NaN never passes, +inf does.
 * That is the pass test of the default row path: p is a candidate of s iff
 * the row path would emit the pair's row.
 *
 * Order.  The candidates of s are ordered by r2 descending under the total
 * order of the f32 bit patterns (-0 sorts below +0; the heat map's max uses
 * the same order), then by partner loaded index ascending.  Site s gets the
 * first min(k, number of candidates) of them.
 *
 * Values.  d, d_prime and r2 are, bit for bit, the f32 values the default row
 * path (WLD_OPT_REF_SUMS 1) puts in the row of pair (a, b); they are listed
 * identically under both sites, d with the sign it has for the ordered pair
 * (a, b).  The sums always run in lib.rs's order: the kernel choice,
 * WLD_OPT_REF_SUMS and the screen options do not apply, and every 64x64 tile
 * of the range and window is computed.
 *
 * Outputs (library-allocated; release with wld_partners_free), lists
 * row-major [site * k + rank]:
 *   n_sites, k  the shape of the lists;
 *   count[n_sites]      the entries filled per site;
 *   partner[n_sites*k]  LOADED indices; 0xFFFFFFFF past count;
 *   d, d_prime, r2 [n_sites*k]  the pair's values; NaN past count;
 *   pairs, none_pairs, passing_pairs  the considered pairs (in range and
 *              window), those without a statistic, and those that pass (each
 *              passing pair is a candidate of both of its sites); exact;
 *   tiles      the 64x64 tiles launched;
 *   kernel_ms  HIP-event time of the pair launch(es), summed over the batches;
 *   merge_ms   HIP-event time of the merge launch(es), summed likewise
 *              (device group: the slowest member's, both).
 * The result is a pure function of the considered pairs: no value goes through
 * an atomic, and everything but the two times is bitwise identical from run to
 * run, across splits of the chunk range, across batch sizes
 * (WLD_OPT_PARTNERS_BATCH_BYTES) and across device groups.
 *
 * wld_partners_merge(into, from) combines two results of the same shape over
 * disjoint chunk ranges into the result of the union of the ranges: the lists
 * merge under the same order, counters and tiles add, the times become the
 * larger of the two.  On a device group (wld_create_multi) the range is
 * sharded exactly as wld_run_summary shards it, the members run concurrently
 * and their results are merged on the host in member order.
 *
 * WLD_E_ARG: k == 0 or k > WLD_PARTNERS_MAX_K; a NaN threshold; chunk_begin >
 * chunk_end; non-finite weights (a load that takes the row path's select
 * loop); wld_partners_merge on results of different shapes.  WLD_E_STATE:
 * before a load, or while a run is in flight.  WLD_E_OOM leaves the context
 * usable.  The call changes nothing a later row run depends on — it keeps its
 * tile list in a buffer of its own — and wld_last_stats and the last run's
 * rows stay as they were.  No progress callback. */
#define WLD_PARTNERS_MAX_K 64
#define WLD_PARTNERS_NONE 0xFFFFFFFFu
typedef struct {
    uint64_t n_sites;
    uint32_t k;
    uint32_t *count;   /* n_sites */
    uint32_t *partner; /* n_sites*k, LOADED indices; WLD_PARTNERS_NONE past count */
    float *d, *d_prime, *r2; /* n_sites*k; NaN past count */
    uint64_t pairs, none_pairs, passing_pairs;
    uint64_t tiles;    /* 64x64 tiles launched */
    double kernel_ms;  /* HIP-event time of the pair launch(es) */
    double merge_ms;   /* HIP-event time of the merge launch(es) */
} wld_partners;
int wld_run_partners(wld_ctx *ctx, uint32_t k, float r2_threshold, uint32_t chunk_begin, uint32_t chunk_end,
                     wld_partners *out);
int wld_partners_merge(wld_partners *into, const wld_partners *from);
void wld_partners_free(wld_partners *p);

/* ---- LD blocks: maximal runs of consecutive sites without a weak pair (not in
 * the reference; Haploview's blocks, PLINK's --blocks, the segments behind
 * tag-SNP selection and region-wise analyses) ----
 *
 * Pairs and classes.  A pair a < b of LOADED sites is considered iff it lies in
 * the linear chunk range [chunk_begin,chunk_end) (end 0 = all, as
 * wld_run_summary; a pair belongs to chunk (a/256, b/256)) and in the
 * context's current window (wld_set_window).  Every considered pair is in
 * exactly one class:
 *   none        single_weighted_ld_pair gives None;
 *   nonfinite   Some, but the chosen value is NaN or +-inf;
 *   informative everything else.
 * The value is, bit for bit, the f32 the default row path (WLD_OPT_REF_SUMS 1)
 * puts in the pair's row: r2 (WLD_BLOCKS_R2) or fabsf(d_prime)
 * (WLD_BLOCKS_ABS_DPRIME).  d_prime is the row path's value, which is the
 * reference's and not the textbook |D'|: two sites that are copies of each
 * other have r2 = 1 but |d_prime| near 0.5, so conventions phrased in D' do
 * not transfer and r2 is the statistic to use by default.  An informative pair
 * is strong iff value >= strong_min (an f32 compare), else weak.  none and
 * nonfinite pairs never break a block.  The sums always run in lib.rs's order:
 * the kernel choice, WLD_OPT_REF_SUMS and the screen options do not apply.
 *
 * Breaks (pass 1: wld_run_block_breaks, every in-window tile of the range).
 * Per loaded site:
 *   fwd_weak[a]  the smallest b of the weak considered pairs (a, b);
 *   bwd_weak[b]  the largest a of the weak considered pairs (a, b);
 *                WLD_BLOCKS_NONE where there is no such pair;
 *   last[a]      the last in-window partner of a (the window's limit; n_sites
 *                - 1 without a window), filled for the whole set whatever the
 *                chunk range;
 *   pairs, none_pairs, nonfinite_pairs, strong_pairs, weak_pairs
 *                pairs = none + nonfinite + strong + weak =
 *                wld_window_pairs_in_chunks(range);
 *   tiles        the 64x64 tiles launched;
 *   kernel_ms    HIP-event time of the launch (device group: the slowest
 *                member's).
 * wld_block_breaks_merge(into, from) combines breaks over disjoint chunk
 * ranges into those of the union: fwd_weak by min, bwd_weak by max, totals and
 * tiles by addition, kernel_ms the larger.  WLD_E_ARG when n_sites, stat,
 * strong_min (as bits) or last differ.
 *
 * Validity of a run [s, e] of consecutive sites (every pair of it must be in
 * the window: e <= last[s]):
 *   WLD_BLOCKS_ALL    no pair of the run is weak;
 *   WLD_BLOCKS_SPINE  (Haploview's solid spine) no pair (s, k) and no pair
 *                     (k, e) of the run is weak; interior pairs may be.
 * A single site is always valid.
 *
 * Partition.  Start at s = 0; e is the largest index in [s, last[s]] for which
 * [s, e] is valid; the next s is e + 1.  Runs of at least min_sites (>= 2)
 * sites are reported as blocks, in site order:
 *   n_blocks, first[k], last[k]   LOADED indices, inclusive;
 *   site_block[i]                 the block of site i, or -1.
 * wld_blocks_partition computes this on the host from a breaks result (no
 * device needed) and leaves the statistics NULL.
 *
 * Block statistics (pass 2: wld_blocks_from_breaks, only the tiles that hold a
 * pair of a reported block).  Per block, over its considered pairs — all
 * chunks, the current window:
 *   pairs, informative, strong   counts (under WLD_BLOCKS_ALL strong ==
 *                informative when the breaks cover every chunk);
 *   value_sum    f64 sum of (double) value over the informative pairs;
 *   value_min    their smallest value, ordered as floats over ALL finite
 *                values; NaN when informative is 0;
 *   tiles, kernel_ms   of pass 2.
 * wld_run_blocks runs both passes over every chunk; the pass-1 totals, tiles
 * and time are then in break_* (zero from wld_blocks_from_breaks, which takes
 * them from nowhere).
 *
 * No value goes through a floating-point atomic on the way to a boundary: the
 * counts, value_min, the break arrays and therefore the partition are
 * identical from run to run, across splits of the chunk range and across
 * device groups.  value_sum is NOT bitwise reproducible: tiles add to a block
 * with f64 atomics in whatever order they finish.  Every term is exact
 * ((double) of an f32), so each sum is within the rounding of an any-order f64
 * sum of its terms: relative error at most about n 2^-53 for n nonnegative
 * terms (the heat map's wording and bound).
 *
 * On a device group (wld_create_multi) pass 1 is sharded exactly as
 * wld_run_summary shards it and merged on the host in member order; pass 2
 * runs on member 0.
 *
 * WLD_E_ARG: an unknown stat or rule; a non-finite strong_min; min_sites < 2;
 * non-finite weights (a load that takes the row path's select loop);
 * chunk_begin > chunk_end; breaks whose n_sites is not the loaded set's (or
 * with a NULL array).  WLD_E_STATE: before a load, or while a run is in
 * flight.  WLD_E_OOM leaves the context usable.  A blocks run changes nothing
 * a later row run depends on — it keeps its tile lists and accumulators in
 * buffers of its own — and wld_last_stats and the last run's rows stay as they
 * were.  No progress callback. */
#define WLD_BLOCKS_R2 0         /* value = r2 */
#define WLD_BLOCKS_ABS_DPRIME 1 /* value = fabsf(d_prime) */
#define WLD_BLOCKS_ALL 0
#define WLD_BLOCKS_SPINE 1
#define WLD_BLOCKS_NONE 0xFFFFFFFFu
typedef struct {
    uint64_t n_sites;
    int stat;
    float strong_min;
    uint32_t *fwd_weak; /* n_sites; WLD_BLOCKS_NONE: no weak pair (i, b) */
    uint32_t *bwd_weak; /* n_sites; WLD_BLOCKS_NONE: no weak pair (a, i) */
    uint32_t *last;     /* n_sites: the last in-window partner */
    uint64_t pairs, none_pairs, nonfinite_pairs, strong_pairs, weak_pairs;
    uint64_t tiles;     /* 64x64 tiles launched */
    double kernel_ms;   /* HIP-event time of the launch (device group: slowest member) */
} wld_block_breaks;
typedef struct {
    uint64_t n_sites;
    uint32_t n_blocks;
    int stat, rule;
    float strong_min;
    uint32_t min_sites;
    uint32_t *first, *last; /* n_blocks: LOADED indices, inclusive */
    int32_t *site_block;    /* n_sites: block id or -1 */
    /* n_blocks each; all NULL from wld_blocks_partition */
    uint64_t *pairs, *informative, *strong;
    double *value_sum;
    float *value_min;       /* NaN where informative == 0 */
    uint64_t tiles;         /* pass 2: 64x64 tiles launched */
    double kernel_ms;       /* pass 2: HIP-event time of the launch */
    /* pass 1 (wld_run_blocks only) */
    uint64_t break_pairs, break_none_pairs, break_nonfinite_pairs, break_strong_pairs, break_weak_pairs;
    uint64_t break_tiles;
    double break_kernel_ms;
} wld_blocks;
int wld_run_block_breaks(wld_ctx *ctx, int stat, float strong_min, uint32_t chunk_begin, uint32_t chunk_end,
                         wld_block_breaks *out);
int wld_block_breaks_merge(wld_block_breaks *into, const wld_block_breaks *from);
void wld_block_breaks_free(wld_block_breaks *b);
int wld_blocks_partition(const wld_block_breaks *breaks, int rule, uint32_t min_sites, wld_blocks *out);
int wld_blocks_from_breaks(wld_ctx *ctx, const wld_block_breaks *breaks, int rule, uint32_t min_sites,
                           wld_blocks *out);
int wld_run_blocks(wld_ctx *ctx, int stat, float strong_min, int rule, uint32_t min_sites, wld_blocks *out);
void wld_blocks_free(wld_blocks *b);

#ifdef __cplusplus
}
#endif
#endif /* WEIGHTEDLD_H */
