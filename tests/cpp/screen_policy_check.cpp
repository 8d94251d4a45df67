// Host check of weightedld_amd/csrc/screen_policy.hpp (stand-alone; built
// plain and with -fsanitize=address,undefined by tests/test_screen_policy.py).
//
// The reference (namespace frozen) is a literal transcription of the policy
// as commit e6794c9 had it, spread over capi.hip and pair_mfma.hip: the flag
// computation of launch_pairs, the if-ladder of launch_pair_mfma, the
// preconditions of fp6_sample, and the learning and stats mapping of
// run_complete, condition for condition over the same plain inputs.  They are
// frozen copies kept as the reference: do not tidy them.
//
//   - decide / wants_sample against the transcription over the full product of
//     the options, load facts, pass facts and learned-threshold classes;
//   - learn against the transcription on both sides of every break-even, for
//     every route, abandoned or not, below / at / above the stored threshold;
//   - the stats mapping for every route;
//   - the route sequences of the GPU policy tests replayed through both.
//
// Thinned: n_tiles only.  The reset state runs with all six n_tiles values at
// every thr; inside the 4^5 learned-threshold classes (thr 0.05) each
// combination runs with one n_tiles value, rotating through the six (n_tiles
// enters the decision only through the give-up count and the sample's 2,048).
// The product (0.86e9 points) is split over up to 16 threads.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "screen_policy.hpp"

using namespace wld::screen_policy;

namespace {

std::atomic<int> g_fail{0};
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) {                       \
            if (++g_fail <= 20) {            \
                printf("FAIL %s: ", #cond);  \
                printf(__VA_ARGS__);         \
                printf("\n");                \
            }                                \
        }                                    \
    } while (0)

namespace frozen {  // commit e6794c9, condition for condition

constexpr uint32_t kScrF32MaxNP = 16384;  // pair_mfma.hip
constexpr int WLD_KERNEL_MFMA = 2;        // any id other than the VALU's

struct Ctx {  // the wld_ctx fields the policy read
    int opt_screen, opt_fp6;
    bool opt_ref_sums, opt_prefilter, opt_i8_pairs;
    int kernel;
    bool use_frag;
    int nonneg;
    uint64_t NP;
    unsigned plane_mask;
    bool fp6_ok, fp6_better;
    uint32_t f6_n_pairs, n_tiles;
    bool prog_pass, count_out;
    float screen_bad_thr, screen2_bad_thr, ref_pairs_bad_thr, fp6_bad_thr, fp6_good_thr;
    // the last pass
    bool screened, screened2, fp6_pass, ref_pairs_pass;
};

enum Launched {
    kValuPlain,      // launch_pair_valu, the context's own codes
    kValuRef,        // launch_pair_valu(rv ...)
    kRowsDense,      // pair_mfma_rows_kernel<kModeDense> (site-major)
    kRowsPrefilter,
    kRowsAll,
    kLdsDense,
    kLdsAll,
    kLdsPrefilter,
    kRefPairs,       // kModeRefPairs + launch_ref_rows
    kScreen2,
    kFp6,
    kI8Pairs,
    kI8Tile,
};

struct Mfma {  // the MfmaLaunch fields that encoded the route
    bool frag, prefilter, screen, screen2, fp6, f6_pairs, i8img, ref_valu, ref_rows;
    uint32_t fp6_bail;
    unsigned plane_mask;
    int nonneg;
    uint64_t NP;
    float thr;
    uint32_t i8img_digit_plane;
};

// launch_pair_mfma's ladder; returns its bool ("a screen ran")
bool launch_pair_mfma(const Mfma &m, bool dense, Launched &k) {
    const bool prefilter = !dense && m.prefilter && m.thr > 0.0f;
    if (!m.frag) {
        if (dense)
            k = kRowsDense;
        else if (prefilter)
            k = kRowsPrefilter;
        else
            k = kRowsAll;
        return false;
    }
    unsigned mask = m.plane_mask & 15;
    if (!mask) mask = 15;
    uint32_t idx = 0, n = 0, top = 0;
    for (uint32_t p = 0; p < 4; ++p)
        if (mask >> p & 1) idx |= p << (2 * n++), top = p;
    if (n == 3 && idx != (0u | (1u << 2) | (2u << 4))) n = 4;
    if (dense) {
        k = kLdsDense;
        return false;
    }
    if (!prefilter) {
        k = kLdsAll;
        return false;
    }
    if (m.ref_rows) {
        k = kRefPairs;
        return true;
    }
    if (!m.screen) {
        k = kLdsPrefilter;
        return false;
    }
    if (m.screen2 && n >= 3) {
        k = kScreen2;
        return true;
    }
    if (m.fp6) {
        k = kFp6;
        return true;
    }
    const int f32 = m.nonneg ? (m.NP <= kScrF32MaxNP ? 2 : m.NP <= 32768 ? 1 : 0) : 0;
    if (f32 == 2 && m.i8img && m.f6_pairs && m.i8img_digit_plane == top) {
        k = kI8Pairs;
        return true;
    }
    k = kI8Tile;
    return true;
}

struct Pass {
    Launched k;
    bool sc;            // *screened
    bool in_mfma;       // the MfmaLaunch was filled (its flags mean something)
    Mfma m;
    bool i8img_wanted;  // i8img_prepare would have run (if not yet for this load)
};

// launch_pairs: the flags, the launch, the per-pass bools on the context.
// image_plane: the digit plane the i8 images hold once prepared.
Pass launch_pairs(Ctx *c, float thr, bool dense, uint32_t image_plane) {
    Pass out{};
    bool sc = false;
    c->fp6_pass = false;
    c->ref_pairs_pass = false;
    const bool ref_screen = c->opt_ref_sums && c->kernel == WLD_KERNEL_MFMA && !dense && c->use_frag &&
                            c->opt_prefilter && thr > 0.0f && c->opt_screen != 0;
    if (c->opt_ref_sums && !ref_screen) {
        out.k = kValuRef;
    } else if (c->kernel == WLD_KERNEL_MFMA) {
        Mfma m{};
        out.in_mfma = true;
        m.frag = c->use_frag;
        m.thr = thr;
        m.plane_mask = c->plane_mask;
        m.NP = c->NP;
        m.nonneg = c->nonneg;
        m.prefilter = c->opt_prefilter && thr > 0.0f;
        m.screen = m.prefilter && (c->opt_screen == 2 || c->opt_screen == 3 ||
                                   (c->opt_screen == 1 && thr > c->screen_bad_thr));
        if (m.prefilter && !m.screen && c->opt_screen == 1 && !ref_screen && thr > c->screen2_bad_thr)
            m.screen = m.screen2 = true;
        if (c->opt_screen == 3) m.screen2 = true;
        if (m.screen2 && __builtin_popcount(c->plane_mask & 15) < 3) {
            m.screen2 = false;
            m.screen = c->opt_screen == 2 || c->opt_screen == 3;
        }
        c->screened2 = m.screen && m.screen2;
        const bool fp6_auto = c->opt_fp6 == 1 || c->opt_fp6 == 3;
        m.fp6 = c->fp6_ok && (c->opt_fp6 == 2 || (fp6_auto && c->fp6_better && thr > c->fp6_bad_thr)) ? true : false;
        m.fp6_bail = fp6_auto && !c->prog_pass && !c->count_out ? std::max<uint32_t>(c->n_tiles / 16, 1) : 0;
        m.f6_pairs = c->f6_n_pairs ? true : false;
        if (!dense && m.prefilter && m.screen && !m.screen2 && !m.fp6 && c->opt_i8_pairs && c->f6_n_pairs &&
            c->use_frag && c->nonneg && c->NP <= 16384) {
            out.i8img_wanted = true;
            m.i8img = true;
            m.i8img_digit_plane = image_plane;
        }
        if (ref_screen) {
            m.ref_valu = true;
            if (!m.screen && ((c->opt_screen == 1 && thr > c->ref_pairs_bad_thr) || c->opt_screen == 4)) {
                m.ref_rows = true;
                c->ref_pairs_pass = true;
            }
        }
        if (ref_screen && !m.screen && !m.ref_rows) {
            out.k = kValuRef;
        } else {
            sc = launch_pair_mfma(m, dense, out.k);
            c->fp6_pass = sc && m.fp6 && !m.screen2 && !m.ref_rows;
        }
        out.m = m;
    } else {
        out.k = kValuPlain;
    }
    out.sc = sc;
    return out;
}

// enqueue_pass around launch_pairs
Pass enqueue_pass(Ctx *c, float thr, uint32_t image_plane) {
    c->screened = c->screened2 = false;
    Pass p{};
    if (c->n_tiles) {
        p = launch_pairs(c, thr, false, image_plane);
        c->screened = p.sc;
    }
    return p;
}

// fp6_sample's preconditions: true where the sample run was launched
bool fp6_sample_runs(const Ctx *c, float thr) {
    if (c->opt_fp6 != 1 || !c->fp6_ok || !c->fp6_better || !(thr > c->fp6_bad_thr) || thr >= c->fp6_good_thr)
        return false;
    if (c->kernel != WLD_KERNEL_MFMA || !c->use_frag || !c->opt_prefilter || !(thr > 0.0f) || c->opt_screen == 0 ||
        c->n_tiles < 2048)
        return false;
    if (!(c->opt_screen == 2 || c->opt_screen == 3 || (c->opt_screen == 1 && thr > c->screen_bad_thr)))
        return false;
    return true;
}
// ... and its verdict on the counts h
void fp6_sample_verdict(Ctx *c, float thr, const unsigned h[2]) {
    if ((uint64_t)h[0] * 16 > h[1])
        c->fp6_bad_thr = std::max(c->fp6_bad_thr, thr);
    else
        c->fp6_good_thr = std::min(c->fp6_good_thr, thr);
}

// run_complete: the abandoned pass
void abandoned(Ctx *c, float thr) { c->fp6_bad_thr = std::max(c->fp6_bad_thr, thr); }

// run_complete: the learning (h: the scan's {cursor, rows, candidate tiles, sub-blocks})
void learn(Ctx *c, float thr, const unsigned long long h[4], uint64_t pairs) {
    if (c->fp6_pass && h[2] * 16 > c->n_tiles) {
        c->fp6_bad_thr = std::max(c->fp6_bad_thr, thr);
    } else if (c->screened && !c->ref_pairs_pass && !c->screened2 && h[2] * 2 > c->n_tiles) {
        c->screen_bad_thr = std::max(c->screen_bad_thr, thr);
    }
    if (c->screened && c->screened2 && h[2] * 5 > c->n_tiles) c->screen2_bad_thr = std::max(c->screen2_bad_thr, thr);
    if (c->ref_pairs_pass && h[0] * 10 > pairs) c->ref_pairs_bad_thr = std::max(c->ref_pairs_bad_thr, thr);
}

// run_complete: the stats mapping
struct Stats {
    int pair_kernel_launches, screened, screen_fp6;
    bool times_screened;
};
Stats stats(const Ctx *c, bool was_abandoned) {
    Stats s{};
    s.pair_kernel_launches = c->n_tiles ? (c->ref_pairs_pass ? 3 : c->screened ? 2 : 1) : 0;
    s.screened = c->ref_pairs_pass ? 4 : c->screened ? (c->screened2 ? 3 : 1) : 0;
    s.screen_fp6 = c->fp6_pass ? 1 : was_abandoned ? 2 : 0;
    s.times_screened = c->screened;
    return s;
}

}  // namespace frozen

// ---- the two sides over the same plain inputs ----------------------------

struct Inputs {
    Options o;
    LoadFacts l;
    PassFacts p;
};

frozen::Ctx frozen_ctx(const Inputs &in, const Learned &s) {
    frozen::Ctx c{};
    c.opt_screen = in.o.screen;
    c.opt_fp6 = in.o.fp6;
    c.opt_ref_sums = in.o.ref_sums;
    c.opt_prefilter = in.o.prefilter;
    c.opt_i8_pairs = in.o.i8_pairs;
    c.kernel = in.l.mfma ? frozen::WLD_KERNEL_MFMA : 1;
    c.use_frag = in.l.use_frag;
    c.nonneg = in.l.nonneg;
    c.NP = in.l.NP;
    c.plane_mask = in.l.plane_mask;
    c.fp6_ok = in.l.fp6_ok;
    c.fp6_better = in.l.fp6_better;
    c.f6_n_pairs = in.p.have_pairs ? (in.p.n_tiles + 1) / 2 + 1 : 0;
    c.n_tiles = in.p.n_tiles;
    c.prog_pass = in.p.prog_pass;
    c.count_out = in.p.count_out;
    c.screen_bad_thr = s.screen_bad;
    c.screen2_bad_thr = s.screen2_bad;
    c.ref_pairs_bad_thr = s.ref_pairs_bad;
    c.fp6_bad_thr = s.fp6_bad;
    c.fp6_good_thr = s.fp6_good;
    return c;
}

bool same_f(float a, float b) { return (std::isnan(a) && std::isnan(b)) || a == b; }
bool same_state(const frozen::Ctx &c, const Learned &s) {
    return same_f(c.screen_bad_thr, s.screen_bad) && same_f(c.screen2_bad_thr, s.screen2_bad) &&
           same_f(c.ref_pairs_bad_thr, s.ref_pairs_bad) && same_f(c.fp6_bad_thr, s.fp6_bad) &&
           same_f(c.fp6_good_thr, s.fp6_good);
}

// the route a frozen launch amounts to
Route route_of(frozen::Launched k) {
    switch (k) {
        case frozen::kValuPlain: return Route::F32Plain;
        case frozen::kValuRef: return Route::F32RefOrder;
        case frozen::kRowsDense:
        case frozen::kRowsPrefilter:
        case frozen::kRowsAll:
        case frozen::kLdsDense:
        case frozen::kLdsAll:
        case frozen::kLdsPrefilter: return Route::IntAll;
        case frozen::kRefPairs: return Route::CandidatePairs;
        case frozen::kScreen2: return Route::TwoPlaneScreen;
        case frozen::kFp6: return Route::Fp6Screen;
        case frozen::kI8Pairs: return Route::I8PairScreen;
        case frozen::kI8Tile: return Route::I8TileScreen;
    }
    return Route::F32Plain;
}

const Route kRoutes[] = {Route::F32Plain,     Route::F32RefOrder,  Route::IntAll,         Route::Fp6Screen,
                         Route::I8PairScreen, Route::I8TileScreen, Route::TwoPlaneScreen, Route::CandidatePairs};

// the per-pass bools commit e6794c9 kept for a route (checked against the
// transcription at every point of the product below)
void set_pass_bools(frozen::Ctx &c, Route r) {
    c.screened = ran_screen(r);
    c.screened2 = r == Route::TwoPlaneScreen;
    c.fp6_pass = r == Route::Fp6Screen;
    c.ref_pairs_pass = r == Route::CandidatePairs;
}

std::atomic<uint64_t> g_points{0};

void report_point(const Inputs &in, const Learned &s, frozen::Ctx c);

// One point of the product: decide, wants_sample and the reporting against
// the transcription.  c: frozen_ctx(in, s), with the pass bools of an earlier
// point (every one of them is written before it is read).
inline void check_point(const Inputs &in, const Learned &s, frozen::Ctx &c, uint32_t top) {
    // (launch_pairs as enqueue_pass and wld_dense call it: with tiles or without)
    c.screened = c.screened2 = false;
    const frozen::Pass ref = frozen::launch_pairs(&c, in.p.thr, in.p.dense, top);
    c.screened = ref.sc;
    const Plan plan = decide(in.o, in.l, in.p, s);
    const Route want = route_of(ref.k);
    bool ok = plan.route == want;
    // the bound test wherever the MFMA launcher read it
    const bool mfma_launch = want != Route::F32Plain && want != Route::F32RefOrder;
    if (mfma_launch) ok = ok && plan.bound_test == ref.m.prefilter;
    // the give-up count as the fp6 screen received it (read nowhere else)
    ok = ok && plan.fp6_bail == (ref.k == frozen::kFp6 ? ref.m.fp6_bail : 0u);
    ok = ok && plan.i8_images == ref.i8img_wanted;
    // kRowsPrefilter / kLdsPrefilter against kRowsAll / kLdsAll: the bound test
    if (ref.k == frozen::kRowsPrefilter || ref.k == frozen::kLdsPrefilter) ok = ok && plan.bound_test;
    if (ref.k == frozen::kRowsAll || ref.k == frozen::kLdsAll) ok = ok && !plan.bound_test;
    // the per-pass bools (set_pass_bools) and the stats they gave
    ok = ok && ran_screen(plan.route) == c.screened &&
         (!c.screened || (plan.route == Route::TwoPlaneScreen) == c.screened2) &&
         (plan.route == Route::Fp6Screen) == c.fp6_pass && (plan.route == Route::CandidatePairs) == c.ref_pairs_pass;
    const frozen::Stats st = frozen::stats(&c, false);
    ok = ok && st.screened == stat_screened(plan.route) && st.screen_fp6 == stat_screen_fp6(plan.route) &&
         st.pair_kernel_launches == (c.n_tiles ? stat_launches(plan.route) : 0) &&
         st.times_screened == ran_screen(plan.route);
    ok = ok && wants_sample(in.o, in.l, in.p, s) == frozen::fp6_sample_runs(&c, in.p.thr);
    if (!ok) report_point(in, s, c);
}

void report_point(const Inputs &in, const Learned &s, frozen::Ctx c) {
    const frozen::Pass ref = frozen::launch_pairs(&c, in.p.thr, in.p.dense, top_plane(in.l.plane_mask));
    const Plan plan = decide(in.o, in.l, in.p, s);
    const Route want = route_of(ref.k);
    CHECK(false,
              "screen %d fp6 %d ref %d pre %d i8p %d mfma %d frag %d nonneg %d NP %llu mask %x ok %d better %d pairs %d "
              "dense %d prog %d cnt %d tiles %u thr %g state {%g %g %g %g %g}: route %d (frozen launch %d -> %d), "
              "bound %d/%d bail %u/%u img %d/%d sample %d/%d",
              in.o.screen, in.o.fp6, in.o.ref_sums, in.o.prefilter, in.o.i8_pairs, in.l.mfma, in.l.use_frag,
              in.l.nonneg, (unsigned long long)in.l.NP, in.l.plane_mask, in.l.fp6_ok, in.l.fp6_better, in.p.have_pairs,
              in.p.dense, in.p.prog_pass, in.p.count_out, in.p.n_tiles, in.p.thr, s.screen_bad, s.screen2_bad,
              s.ref_pairs_bad, s.fp6_bad, s.fp6_good, (int)plan.route, (int)ref.k, (int)want, plan.bound_test,
              ref.m.prefilter, plan.fp6_bail, ref.m.fp6_bail, plan.i8_images, ref.i8img_wanted,
              wants_sample(in.o, in.l, in.p, s), frozen::fp6_sample_runs(&c, in.p.thr));
}

const uint32_t kTiles[] = {0, 15, 16, 2047, 2048, 100000};

// worker w of n: its share of the product
void check_decisions(unsigned w, unsigned n) {
    // the learned states: reset alone (every thr), and at thr 0.05 each of the
    // five thresholds at {reset, just below thr, thr, just above}
    const float t = 0.05f, below = std::nextafterf(t, -1.0f), above = std::nextafterf(t, 1.0f);
    const float other[] = {NAN, -0.5f, 0.0f};
    std::vector<Learned> classes;
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b)
            for (int c = 0; c < 4; ++c)
                for (int d = 0; d < 4; ++d)
                    for (int e = 0; e < 4; ++e) {
                        const float v[4] = {-1.0f, below, t, above};
                        Learned s;
                        s.screen_bad = v[a];
                        s.screen2_bad = v[b];
                        s.ref_pairs_bad = v[c];
                        s.fp6_bad = v[d];
                        s.fp6_good = e ? v[e] : INFINITY;
                        classes.push_back(s);
                    }
    const unsigned masks[] = {0b0001, 0b0011, 0b0111, 0b1011, 0b1111};
    const uint64_t NPs[] = {16384, 16448};
    uint32_t rot = w % 6;
    uint64_t points = 0;
    Inputs in{};
    for (in.o.screen = 0; in.o.screen <= 4; ++in.o.screen)
    for (in.o.fp6 = 0; in.o.fp6 <= 3; ++in.o.fp6)
    for (unsigned bits = w; bits < (1u << 13); bits += n) {
        in.o.ref_sums = bits & 1;
        in.o.prefilter = bits >> 1 & 1;
        in.o.i8_pairs = bits >> 2 & 1;
        in.l.mfma = bits >> 3 & 1;
        in.l.use_frag = bits >> 4 & 1;
        in.l.nonneg = bits >> 5 & 1;
        in.l.NP = NPs[bits >> 6 & 1];
        in.l.fp6_ok = bits >> 7 & 1;
        in.l.fp6_better = bits >> 8 & 1;
        in.p.have_pairs = bits >> 9 & 1;
        in.p.dense = bits >> 10 & 1;
        in.p.prog_pass = bits >> 11 & 1;
        in.p.count_out = bits >> 12 & 1;
        for (unsigned mask : masks) {
            in.l.plane_mask = mask;
            const uint32_t top = top_plane(mask);
            for (uint32_t nt : kTiles) {  // the reset state: every n_tiles at every thr
                in.p.n_tiles = nt;
                frozen::Ctx c = frozen_ctx(in, Learned{});
                for (float th : other) {
                    in.p.thr = th;
                    check_point(in, Learned{}, c, top);
                }
                in.p.thr = t;
                check_point(in, Learned{}, c, top);
            }
            in.p.thr = t;
            frozen::Ctx c = frozen_ctx(in, Learned{});
            for (const Learned &s : classes) {  // (n_tiles thinned: one of the six per combination, rotating)
                in.p.n_tiles = c.n_tiles = kTiles[rot];
                rot = rot == 5 ? 0 : rot + 1;
                c.screen_bad_thr = s.screen_bad;
                c.screen2_bad_thr = s.screen2_bad;
                c.ref_pairs_bad_thr = s.ref_pairs_bad;
                c.fp6_bad_thr = s.fp6_bad;
                c.fp6_good_thr = s.fp6_good;
                check_point(in, s, c, top);
            }
            points += 4 * 6 + classes.size();
        }
    }
    g_points += points;
}

// the images' plane against the top active plane: pairs only while they match
void check_settle() {
    for (unsigned mask = 0; mask < 16; ++mask) {
        unsigned m = mask ? mask : 15;
        uint32_t top = 0;
        for (uint32_t p = 0; p < 4; ++p)
            if (m >> p & 1) top = p;
        CHECK(top_plane(mask) == top, "mask %x", mask);
        for (uint32_t img = 0; img < 4; ++img) {
            // launch_pair_mfma: `m.i8img->digit_plane == top` or the single-tile screen
            frozen::Mfma fm{};
            fm.frag = fm.prefilter = fm.screen = fm.f6_pairs = fm.i8img = true;
            fm.thr = 0.05f;
            fm.plane_mask = mask;
            fm.nonneg = 1;
            fm.NP = 16384;
            fm.i8img_digit_plane = img;
            frozen::Launched k;
            frozen::launch_pair_mfma(fm, false, k);
            CHECK(settle_i8(Route::I8PairScreen, img, mask) == route_of(k), "mask %x image plane %u", mask, img);
            for (Route r : kRoutes)
                if (r != Route::I8PairScreen) CHECK(settle_i8(r, img, mask) == r, "route %d", (int)r);
        }
    }
}

// learn on both sides of every break-even, for every route, abandoned or
// not, with the stored thresholds below, at and above the pass's
void check_learning() {
    const float thr = 0.01f;
    const float stored[] = {-1.0f, std::nextafterf(thr, -1.0f), thr, std::nextafterf(thr, 1.0f), 0.5f, NAN};
    const uint64_t ks[] = {16, 2, 5, 10};
    for (Route r : kRoutes)
        for (float st : stored)
            for (float good : {st, INFINITY})
                for (uint64_t k : ks)
                    for (uint64_t q : {(uint64_t)0, (uint64_t)1, (uint64_t)7, (uint64_t)6250})
                        for (int side = 0; side < 2; ++side)
                            for (int ab = 0; ab < 2; ++ab) {
                                // k c == n (not more than 1/k) and k c == n + 1 (more)
                                const uint64_t cnt = q + (uint64_t)side, n = k * cnt - (uint64_t)side;
                                if (side && !cnt) continue;
                                Learned s;
                                s.screen_bad = s.screen2_bad = s.ref_pairs_bad = s.fp6_bad = st;
                                s.fp6_good = good;
                                Inputs in{};
                                in.p.n_tiles = (uint32_t)n;
                                frozen::Ctx c = frozen_ctx(in, s);
                                set_pass_bools(c, r);
                                // tiles and pairs at the boundary together: each test reads its own count
                                const unsigned long long h[4] = {cnt, 0, cnt, 0};
                                if (ab) {
                                    frozen::abandoned(&c, thr);
                                    learn(s, Outcome{r, thr, true, cnt, n, cnt, n});
                                } else {
                                    frozen::learn(&c, thr, h, n);
                                    learn(s, Outcome{r, thr, false, cnt, n, cnt, n});
                                }
                                CHECK(same_state(c, s), "route %d stored %g k %llu count %llu of %llu abandoned %d",
                                      (int)r, st, (unsigned long long)k, (unsigned long long)cnt,
                                      (unsigned long long)n, ab);
                                // the sample's verdict: 16 h0 == h1 and 16 h0 == h1 + 1
                                if (k == 16 && !ab && r == Route::Fp6Screen) {
                                    Learned s2;
                                    s2.fp6_bad = st;
                                    s2.fp6_good = good;
                                    frozen::Ctx c2 = frozen_ctx(in, s2);
                                    const unsigned hs[2] = {(unsigned)cnt, (unsigned)n};
                                    frozen::fp6_sample_verdict(&c2, thr, hs);
                                    learn(s2, Sample{thr, cnt, n});
                                    CHECK(same_state(c2, s2), "sample stored %g good %g: %llu of %llu", st, good,
                                          (unsigned long long)cnt, (unsigned long long)n);
                                }
                            }
}

// ---- replays: a context driven through decide / learn and through the
// transcription, pass by pass ----------------------------------------------

struct Replay {
    Inputs in{};
    Learned s;
    frozen::Ctx c{};
    const char *name;

    Replay(const char *nm, const Inputs &i) : in(i), c(frozen_ctx(i, Learned{})), name(nm) {}

    // run_enqueue's sample (h0 of h1 sampled tiles candidates), if wanted
    bool sample(float thr, unsigned h0, unsigned h1) {
        in.p.thr = thr;
        const bool want = wants_sample(in.o, in.l, in.p, s), ref = frozen::fp6_sample_runs(&c, thr);
        CHECK(want == ref, "%s: sample at %g wanted %d, frozen %d", name, thr, want, ref);
        if (want) {
            const unsigned h[2] = {h0, h1};
            frozen::fp6_sample_verdict(&c, thr, h);
            learn(s, Sample{thr, h0, h1});
        }
        CHECK(same_state(c, s), "%s: state after the sample at %g", name, thr);
        return want;
    }
    // one pass at thr leaving cand_tiles (and cand_pairs of pairs); give_up:
    // the fp6 screen abandons it first.  Returns wld_run_stats.screened.
    int pass(float thr, uint64_t cand_tiles, uint64_t cand_pairs = 0, uint64_t pairs = 1999000, bool give_up = false,
             int *screen_fp6 = nullptr) {
        in.p.thr = thr;
        bool was_abandoned = false;
        for (;;) {
            Plan plan = decide(in.o, in.l, in.p, s);
            plan.route = settle_i8(plan.route, top_plane(in.l.plane_mask), in.l.plane_mask);
            const frozen::Pass ref = frozen::enqueue_pass(&c, thr, top_plane(in.l.plane_mask));
            CHECK(plan.route == route_of(ref.k), "%s: thr %g route %d, frozen %d", name, thr, (int)plan.route,
                  (int)route_of(ref.k));
            if (give_up && !was_abandoned) {
                CHECK(plan.route == Route::Fp6Screen && plan.fp6_bail, "%s: nothing to give up at %g", name, thr);
                was_abandoned = true;
                frozen::abandoned(&c, thr);
                learn(s, Outcome{plan.route, thr, true, 0, in.p.n_tiles, 0, pairs});
                continue;
            }
            const unsigned long long h[4] = {cand_pairs, 0, cand_tiles, 0};
            const frozen::Stats st = frozen::stats(&c, was_abandoned);
            frozen::learn(&c, thr, h, pairs);
            learn(s, Outcome{plan.route, thr, false, cand_tiles, in.p.n_tiles, cand_pairs, pairs});
            CHECK(same_state(c, s), "%s: state after the pass at %g", name, thr);
            const int fp6 = stat_screen_fp6(plan.route) ? 1 : was_abandoned ? 2 : 0;
            CHECK(st.screened == stat_screened(plan.route) && st.screen_fp6 == fp6, "%s: stats at %g", name, thr);
            if (screen_fp6) *screen_fp6 = fp6;
            return st.screened;
        }
    }
};

void check_replays() {
    Inputs base{};
    base.o = Options{1, 0, false, true, true};
    base.l = LoadFacts{true, true, true, 2048, 7, false, false};
    base.p = PassFacts{true, 528, 0.0f, false, false, false};
    {  // test_screen_auto_policy: 2000 x 2000, 528 tiles, the i8 tiers
        Replay r("auto policy", base);
        int seen[6];
        seen[0] = r.pass(0.002f, 265);  // more than half
        seen[1] = r.pass(0.002f, 106);  // two planes: more than a fifth
        seen[2] = r.pass(0.001f, 528);
        seen[3] = r.pass(0.05f, 0);
        seen[4] = r.pass(0.001f, 528);
        seen[5] = r.pass(0.003f, 264);  // not more than half
        const int want[6] = {1, 3, 0, 1, 0, 1};
        for (int i = 0; i < 6; ++i) CHECK(seen[i] == want[i], "auto policy step %d: screened %d", i, seen[i]);
    }
    {  // test_ref_screen_policy: lib.rs's order, 1 -> 4 -> 0, then 1 at 0.05
        Inputs in = base;
        in.o.ref_sums = true;
        Replay r("ref policy", in);
        CHECK(r.pass(0.002f, 265) == 1, "ref policy: first pass");
        CHECK(r.pass(0.002f, 528, 199900, 1999000) == 4, "ref policy: candidate pairs");  // a tenth: not more
        CHECK(r.pass(0.002f, 528, 199901, 1999000) == 4, "ref policy: candidate pairs again");  // more than a tenth
        CHECK(r.pass(0.002f, 528) == 0, "ref policy: the full kernel");
        CHECK(r.pass(0.0005f, 528) == 0, "ref policy: lower stays");
        CHECK(r.pass(0.05f, 0) == 1, "ref policy: higher screens");
    }
    Inputs fp6 = base;
    fp6.o.fp6 = 1;
    fp6.l.fp6_ok = fp6.l.fp6_better = true;
    {  // the fp6 screen hands over to i8 after a pass that leaves more than 1/16
        Replay r("fp6 handover", fp6);
        int f = 0;
        CHECK(!r.sample(0.01f, 0, 0), "fp6 handover: 528 tiles are not sampled");
        CHECK(r.pass(0.01f, 33, 0, 1999000, false, &f) == 1 && f == 1, "fp6 handover: 33 of 528 on fp6");
        CHECK(r.pass(0.01f, 33, 0, 1999000, false, &f) == 1 && f == 1, "fp6 handover: 16 x 33 == 528 stays");
        CHECK(r.pass(0.01f, 34, 0, 1999000, false, &f) == 1 && f == 1, "fp6 handover: the pass that leaves more");
        CHECK(r.pass(0.01f, 34, 0, 1999000, false, &f) == 1 && f == 0, "fp6 handover: then i8");
        CHECK(r.pass(0.005f, 34, 0, 1999000, false, &f) == 1 && f == 0, "fp6 handover: lower too");
        CHECK(r.pass(0.02f, 0, 0, 1999000, false, &f) == 1 && f == 1, "fp6 handover: higher on fp6");
    }
    fp6.p.n_tiles = 20100;
    {  // a sample that goes bad: i8 at once, and no second sample there or below
        Replay r("fp6 bad sample", fp6);
        int f = 0;
        CHECK(r.sample(0.01f, 20, 314), "fp6 bad sample: wanted");
        CHECK(r.pass(0.01f, 9000, 0, 1999000, false, &f) == 1 && f == 0, "fp6 bad sample: i8");
        CHECK(!r.sample(0.01f, 0, 314) && !r.sample(0.005f, 0, 314), "fp6 bad sample: settled");
        CHECK(r.sample(0.02f, 19, 314), "fp6 bad sample: above it another sample");
    }
    {  // a sample that goes good, then none at a higher thr
        Replay r("fp6 good sample", fp6);
        int f = 0;
        CHECK(r.sample(0.01f, 19, 304), "fp6 good sample: wanted");  // 16 x 19 == 304: not more
        CHECK(r.pass(0.01f, 100, 0, 1999000, false, &f) == 1 && f == 1, "fp6 good sample: fp6");
        CHECK(!r.sample(0.01f, 0, 0) && !r.sample(0.02f, 0, 0), "fp6 good sample: not wanted again");
        CHECK(r.sample(0.009f, 0, 314), "fp6 good sample: below it another sample");
    }
    {  // an abandoned pass (auto without the sample run): re-run on i8, screen_fp6 2
        Inputs in = fp6;
        in.o.fp6 = 3;
        Replay r("fp6 abandoned", in);
        int f = 0;
        CHECK(!r.sample(0.01f, 0, 0), "fp6 abandoned: no sample with WLD_OPT_SCREEN_FP6 3");
        CHECK(r.pass(0.01f, 9000, 0, 1999000, true, &f) == 1 && f == 2, "fp6 abandoned: given up, i8");
        CHECK(r.pass(0.01f, 9000, 0, 1999000, false, &f) == 1 && f == 0, "fp6 abandoned: i8 from then on");
        CHECK(r.pass(0.02f, 10, 0, 1999000, false, &f) == 1 && f == 1, "fp6 abandoned: higher on fp6");
    }
}

}  // namespace

int main() {
    check_settle();
    check_learning();
    check_replays();
    const unsigned n = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<std::thread> workers;
    for (unsigned w = 0; w < n; ++w) workers.emplace_back(check_decisions, w, n);
    for (std::thread &t : workers) t.join();
    printf("%llu decision points\n", (unsigned long long)g_points.load());
    if (g_fail) {
        printf("%d failures\n", g_fail.load());
        return 1;
    }
    printf("OK\n");
    return 0;
}
