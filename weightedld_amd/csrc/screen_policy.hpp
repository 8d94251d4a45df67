// The pair pass's screen policy (capi.hip launch_pairs / fp6_sample /
// run_complete; pair_mfma.hip launch_pair_mfma switches on the Route): which
// of eight routes a pass takes, the thresholds the auto policy learns from the
// passes it has seen, and what a route reports in wld_run_stats.  This is the
// one place the policy lives.  Header-only and free of HIP types so the host
// test (tests/cpp/screen_policy_check.cpp) checks the same code; its functions
// have internal linkage, so the library's exported symbols are not touched.
//
// Every comparison against a learned threshold is written as the pass needs
// it for a NaN threshold: `thr > bad` is false for NaN (no screen), `!(thr >
// bad)` true, `thr >= good` false.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace wld {
namespace screen_policy {

// The path a pass takes through the pair kernels.
enum class Route : uint8_t {
    F32Plain,        // the plain f32 kernel on every tile (pair_valu.hip)
    F32RefOrder,     // lib.rs's summation order on every tile (the f32 kernel, lane-class layout)
    IntAll,          // the integer (MFMA) kernel on every tile, with or without the per-pair bound test
    Fp6Screen,       // the one-plane screen on fp6 x fp4 MFMA, then the candidate tiles
    I8PairScreen,    // the i8 one-plane screen on tile pairs (pre-multiplied images), then the candidates
    I8TileScreen,    // the i8 one-plane screen on single tiles, then the candidates
    TwoPlaneScreen,  // the screen on the top two digit planes, then the candidates
    CandidatePairs,  // every tile on the integer kernel, the pairs its bound cannot reject summed in lib.rs's order
};

// --- break-evens ---------------------------------------------------------
// A screen that leaves more than 1/k of what it looked at does not pay at that
// threshold, nor at any lower one.

// The fp6 screen hands over to the i8 one (a tighter bound at twice the cost)
// once it leaves more than a sixteenth of the tiles; in auto it gives the pass
// up on reaching that many, and its sample run judges by the same ratio.
constexpr uint64_t kFp6Keep = 16;
// A threshold at which even the i8 screen leaves more than half the tiles is
// not screened from then on: the screen costs a third of the full three-plane
// kernel, the candidates as much again; in lib.rs's order the exact candidate
// pairs take over there (a screened tile with one uncertain 16x16 sub-block
// costs ~0.12 us on the f32 kernel: half the C4 tiles ~3 ms over the 0.9 ms
// screen, about the exact candidate pairs' cost).
constexpr uint64_t kOnePlaneKeep = 2;
// The two-plane screen (0.8 of the full kernel's time at BASELINE config 4,
// archive/profiles_r01_r03/r02s2/) that leaves more than a fifth goes to the
// full kernel (the exact mode; lib.rs's order takes the two-plane screen only
// when asked, WLD_OPT_SCREEN 3).
constexpr uint64_t kTwoPlaneKeep = 5;
// Exact candidate pairs, each summed alone in lib.rs's order (~1 ms per
// million at C4 size): past a tenth of all pairs the full f32 kernel (27.8 ms
// for every tile at C4) is cheaper.
constexpr uint64_t kCandidatePairsKeep = 10;
// Tile lists shorter than this take the fp6 pass itself as the test (it gives
// up past a sixteenth); longer ones are sampled first.
constexpr uint32_t kSampleMinTiles = 2048;
// The tile-pair fp6 screen on three masked sums per pair runs the stage loop
// a second time (a quarter of the MFMAs again, with every copy and barrier)
// for an entry with a pair the three sums leave in doubt.  By MFMA count it
// breaks even with the four-sum kernel near 0.45 of the entries; auto takes
// it only where the sample run found the second pass on at most an eighth of
// its entries: a cap well inside the break-even, not a tuned value.
constexpr uint64_t kFp6ThreeKeep = 8;
// The three-sum screen's quick test rejects a lane's 16 pairs of a row block
// together at about half the full test's vector operations; a row block where
// some lane cannot be rejected pays the quick test on top of the full one.  By
// operation count it breaks even near 0.4 of the row blocks falling through;
// auto takes it only where the sample run found at most a quarter.
constexpr uint64_t kFp6QuickKeep = 4;
// (a 64 x 64 tile is four row blocks of 16 sites)
constexpr uint64_t kFp6RowBlocksPerTile = 4;

// What the auto policy has learned on this load, window and option set.
struct Learned {
    // the largest threshold at which the one-plane screen left > half the tiles
    float screen_bad = -1.0f;
    // ... and at which the two-plane screen left > a fifth
    float screen2_bad = -1.0f;
    // lib.rs's order: the largest threshold at which the exact candidate pairs
    // were more than a tenth of all pairs (then the full f32 kernel)
    float ref_pairs_bad = -1.0f;
    // the largest threshold at which the fp6 screen left more than a sixteenth
    // of the tiles (there and below, the i8 screen's tighter bound)
    float fp6_bad = -1.0f;
    // the smallest threshold at which the fp6 screen's sample run found few
    // enough candidate tiles (there and above no sample run is needed)
    float fp6_good = INFINITY;
    // the smallest threshold at which the sample run found the three-sum
    // screen's second pass on at most an eighth of its entries (there and
    // above the screen runs on three sums: a higher threshold leaves fewer
    // pairs in doubt)
    float fp6_three_good = INFINITY;
    // the smallest threshold at which the sample run, on three sums with the
    // quick test, found at most a quarter of its row blocks falling through to
    // the full test (there and above the quick test runs: a higher threshold
    // lets it reject more)
    float fp6_quick_good = INFINITY;

    void reset() { *this = Learned{}; }
};

struct Options {
    int screen;  // WLD_OPT_SCREEN: 0 never, 1 auto, 2 always, 3 two-plane, 4 exact candidate pairs
    int fp6;     // WLD_OPT_SCREEN_FP6: 0 off, 1 auto, 2 whenever it applies, 3 auto without the sample run
    bool ref_sums, prefilter, i8_pairs;
    // WLD_OPT_FP6_THREE: 0 four sums, 1 auto (where a sample run allowed it),
    // 2 three sums wherever the tile-pair fp6 screen runs
    int fp6_three = 1;
    // WLD_OPT_FP6_QUICK: 0 off, 1 auto (where a sample run allowed it), 2
    // wherever the three-sum kernel runs
    int fp6_quick = 1;
};
struct LoadFacts {
    bool mfma;            // the load runs on the integer kernel (WLD_KERNEL_MFMA)
    bool use_frag;        // ... in the fragment-major layout (not site-major)
    bool nonneg;          // every weight >= 0
    uint64_t NP;          // padded sequences
    unsigned plane_mask;  // the active weight-digit planes
    bool fp6_ok, fp6_better;  // fp6 operands exist; their residual is within twice the i8 top digit's
};
struct PassFacts {
    bool have_pairs;   // the tile list has its tile-pair list
    uint32_t n_tiles;
    float thr;
    bool dense;        // dense stats (wld_dense), not rows
    bool prog_pass;    // the pass reports per-chunk progress
    bool count_out;    // the caller gave a device count word
};

struct Plan {
    Route route = Route::F32Plain;
    // IntAll and the screens: the per-pair bound test is on (a positive
    // threshold is needed to reject anything)
    bool bound_test = false;
    // Fp6Screen: give the pass up past this many candidate tiles (0: never)
    uint32_t fp6_bail = 0;
    // I8PairScreen: the pass needs the pre-multiplied images (settle_i8)
    bool i8_images = false;
    // Fp6Screen on the tile-pair list: three masked sums per pair, the fourth
    // only for entries with a pair in doubt (the same candidates either way)
    bool fp6_three = false;
    // ... with the lane-shared quick test in front of the three-sum test (the
    // same verdicts either way)
    bool fp6_quick = false;
};

// Whether a tile-pair fp6 screen at thr runs on three sums.  Auto needs a
// sample run's word for this threshold or a lower one: lists that are never
// sampled (fewer than kSampleMinTiles tiles, WLD_OPT_SCREEN_FP6 2 or 3) stay
// on four sums.  (NaN thresholds compare false: four sums.)
static inline bool fp6_three(const Options &o, const PassFacts &p, const Learned &s) {
    if (!p.have_pairs) return false;
    return o.fp6_three == 2 || (o.fp6_three == 1 && p.thr >= s.fp6_three_good);
}

// Whether a screen on three sums runs the quick test first.  Auto needs a
// sample run's word, as fp6_three: lists that are not sampled stay off.
static inline bool fp6_quick(const Options &o, const PassFacts &p, const Learned &s) {
    return o.fp6_quick == 2 || (o.fp6_quick == 1 && p.thr >= s.fp6_quick_good);
}

static inline Plan decide(const Options &o, const LoadFacts &l, const PassFacts &p, const Learned &s) {
    Plan plan;
    const float thr = p.thr;
    const bool bound = o.prefilter && thr > 0.0f;
    // lib.rs's order with a screen in front: the integer kernel's fragment
    // layout, rows, a bound that can reject, and a screen not switched off
    const bool ref_screen = o.ref_sums && l.mfma && !p.dense && l.use_frag && bound && o.screen != 0;
    if (o.ref_sums && !ref_screen) {
        plan.route = Route::F32RefOrder;
        return plan;
    }
    if (!l.mfma) return plan;  // F32Plain
    plan.route = Route::IntAll;
    plan.bound_test = bound;
    // no screen without a bound to screen with, for dense stats, or site-major
    if (!bound || p.dense || !l.use_frag) return plan;

    // auto: below a threshold at which the screen left more than half the
    // tiles as candidates, every tile goes straight to the full kernel ...
    const bool one = o.screen == 2 || o.screen == 3 || (o.screen == 1 && thr > s.screen_bad);
    // ... where the one-plane screen proved ineffective, the two-plane one
    // unless it proved ineffective too (in lib.rs's order the exact candidate
    // pairs instead); with one or two active planes there is no such screen
    const bool two = __builtin_popcount(l.plane_mask & 15) >= 3 &&
                     (o.screen == 3 || (o.screen == 1 && !one && !ref_screen && thr > s.screen2_bad));
    if (two) {
        plan.route = Route::TwoPlaneScreen;
    } else if (one) {
        // the one-plane screen on fp6 x fp4 MFMA where the load allows it
        const bool fp6_auto = o.fp6 == 1 || o.fp6 == 3;
        if (l.fp6_ok && (o.fp6 == 2 || (fp6_auto && l.fp6_better && thr > s.fp6_bad))) {
            plan.route = Route::Fp6Screen;
            plan.fp6_three = fp6_three(o, p, s);
            plan.fp6_quick = plan.fp6_three && fp6_quick(o, p, s);
            // auto: past a sixteenth of the tiles as candidates the fp6 screen
            // gives the pass up and the pass is re-run on the i8 screen (not
            // with per-chunk progress, which a re-run does not report again,
            // nor with a caller's count word, which a collective may read
            // before the re-run rewrites it)
            if (fp6_auto && !p.prog_pass && !p.count_out)
                plan.fp6_bail = std::max<uint32_t>(p.n_tiles / (uint32_t)kFp6Keep, 1);
        } else if (o.i8_pairs && p.have_pairs && l.nonneg && l.NP <= 16384) {
            // (doubled f32 sums: non-negative weights, NP <= 16384)
            plan.route = Route::I8PairScreen;
            plan.i8_images = true;
        } else {
            plan.route = Route::I8TileScreen;
        }
    } else if (ref_screen) {
        // where the screen does not pay: every tile on all planes, the pairs
        // the bound cannot reject summed one by one in lib.rs's order, unless
        // that proved to be most pairs (then the full kernel)
        if (!((o.screen == 1 && thr > s.ref_pairs_bad) || o.screen == 4)) return Plan{Route::F32RefOrder};
        plan.route = Route::CandidatePairs;
    }
    return plan;
}

// The top active digit plane (no active plane counts as all four).
static inline uint32_t top_plane(unsigned plane_mask) {
    unsigned mask = plane_mask & 15;
    if (!mask) mask = 15;
    return 31u - (uint32_t)__builtin_clz(mask);
}

// The tile-pair i8 screen multiplies by images of one digit plane, built once
// per load: they serve while that plane is still the top active one.  After
// WLD_OPT_ALL_PLANES has moved the top plane the pass screens single tiles.
static inline Route settle_i8(Route planned, uint32_t image_plane, unsigned plane_mask) {
    if (planned == Route::I8PairScreen && image_plane != top_plane(plane_mask)) return Route::I8TileScreen;
    return planned;
}

// Whether a sample run of the fp6 screen should precede the pass (auto,
// WLD_OPT_SCREEN_FP6 1): the pass would screen on fp6, its list is long enough
// for a sample to be cheaper than a given-up pass, and no earlier sample or
// pass has settled this threshold.  Samples precede row passes only (dense is
// ignored), and WLD_OPT_SCREEN 3 samples as 2 does: the two-plane screen it
// forces with three or more planes never reads the verdict, but the sample has
// always run there and wld_run_stats.fp6_sampled reports it.
static inline bool wants_sample(Options o, const LoadFacts &l, PassFacts p, const Learned &s) {
    if (o.screen == 3) o.screen = 2;
    p.dense = false;
    return o.fp6 == 1 && decide(o, l, p, s).route == Route::Fp6Screen && p.n_tiles >= kSampleMinTiles &&
           !(p.thr >= s.fp6_good);
}

// The sample run's verdict: of `sampled` tiles, `candidates` hold a pair the
// fp6 bound cannot reject.
// three: the sample ran on three sums (the tile-pair list, WLD_OPT_FP6_THREE
// not 0) and `rechecked` of its entries took the second pass.  An entry holds
// at most two tiles, so (sampled + 1) / 2 is a lower bound of the sampled
// entries: the eighth is taken of that.
// quick: the sample ran the quick test as well (WLD_OPT_FP6_QUICK not 0) and
// `quick_full` of its 4 x sampled row blocks fell through to the full test.
struct Sample {
    float thr;
    uint64_t candidates, sampled;
    bool three = false;
    uint64_t rechecked = 0;
    bool quick = false;
    uint64_t quick_full = 0;
};
static inline void learn(Learned &s, const Sample &r) {
    if (r.candidates * kFp6Keep > r.sampled) {
        s.fp6_bad = std::max(s.fp6_bad, r.thr);
        return;
    }
    s.fp6_good = std::min(s.fp6_good, r.thr);
    if (r.three && r.sampled && r.rechecked * kFp6ThreeKeep <= (r.sampled + 1) / 2)
        s.fp6_three_good = std::min(s.fp6_three_good, r.thr);
    if (r.three && r.quick && r.sampled && r.quick_full * kFp6QuickKeep <= r.sampled * kFp6RowBlocksPerTile)
        s.fp6_quick_good = std::min(s.fp6_quick_good, r.thr);
}

// A completed pass.
struct Outcome {
    Route route;
    float thr;
    bool abandoned;            // the fp6 screen gave the pass up (the counts below mean nothing)
    uint64_t candidate_tiles;  // tiles the screen left
    uint64_t n_tiles;
    uint64_t candidate_pairs;  // CandidatePairs: the pairs staged
    uint64_t pairs;            // the run's pairs
};
static inline void learn(Learned &s, const Outcome &r) {
    if (r.abandoned) {
        // this threshold (and any lower one) screens on i8 from now on
        s.fp6_bad = std::max(s.fp6_bad, r.thr);
        return;
    }
    const bool i8 = r.route == Route::I8PairScreen || r.route == Route::I8TileScreen;
    if (r.route == Route::Fp6Screen && r.candidate_tiles * kFp6Keep > r.n_tiles)
        s.fp6_bad = std::max(s.fp6_bad, r.thr);
    else if ((r.route == Route::Fp6Screen || i8) && r.candidate_tiles * kOnePlaneKeep > r.n_tiles)
        s.screen_bad = std::max(s.screen_bad, r.thr);
    if (r.route == Route::TwoPlaneScreen && r.candidate_tiles * kTwoPlaneKeep > r.n_tiles)
        s.screen2_bad = std::max(s.screen2_bad, r.thr);
    if (r.route == Route::CandidatePairs && r.candidate_pairs * kCandidatePairsKeep > r.pairs)
        s.ref_pairs_bad = std::max(s.ref_pairs_bad, r.thr);
}

// --- what a route reports (wld_run_stats) --------------------------------

// A screen ran in front of the candidates: the pass has a screen phase
// (screen_ms) and candidate counts.
static inline bool ran_screen(Route r) {
    return r == Route::Fp6Screen || r == Route::I8PairScreen || r == Route::I8TileScreen ||
           r == Route::TwoPlaneScreen || r == Route::CandidatePairs;
}
// wld_run_stats.screened
static inline int stat_screened(Route r) {
    return r == Route::CandidatePairs ? 4 : r == Route::TwoPlaneScreen ? 3 : ran_screen(r) ? 1 : 0;
}
// wld_run_stats.screen_fp6 of a pass that was not given up
static inline int stat_screen_fp6(Route r) { return r == Route::Fp6Screen ? 1 : 0; }
// wld_run_stats.fp6_three of a pass that was not given up
static inline int stat_fp6_three(const Plan &p) { return p.route == Route::Fp6Screen && p.fp6_three ? 1 : 0; }
// wld_run_stats.fp6_quick of a pass that was not given up
static inline int stat_fp6_quick(const Plan &p) { return stat_fp6_three(p) && p.fp6_quick ? 1 : 0; }
// wld_run_stats.pair_kernel_launches of a pass with tiles (exact candidate
// pairs: the i8 pass, ref_sums_kernel, ref_compact_kernel)
static inline int stat_launches(Route r) { return r == Route::CandidatePairs ? 3 : ran_screen(r) ? 2 : 1; }

}  // namespace screen_policy
}  // namespace wld
