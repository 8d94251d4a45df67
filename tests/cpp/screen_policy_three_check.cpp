// Host check of the three-sum rule in weightedld_amd/csrc/screen_policy.hpp
// (stand-alone; built plain and with -fsanitize=address,undefined by
// tests/test_screen_policy_three.py).
//
//   - WLD_OPT_FP6_THREE changes nothing of a plan but Plan::fp6_three, over
//     the product of the options, load facts, pass facts and learned
//     thresholds below; fp6_three is set only on the Fp6Screen route with a
//     tile-pair list;
//   - option 0 never, option 2 always there, option 1 (auto) only at or above
//     a threshold a sample run has allowed;
//   - the sample's rule: three sums where the second pass ran on at most an
//     eighth of the sampled entries (an entry holds at most two tiles), learned
//     monotonically in the threshold, never from a four-sum sample, never from
//     a sample that sends the threshold to the i8 screen;
//   - lists without a sample (fewer than 2,048 tiles, WLD_OPT_SCREEN_FP6 2 or
//     3) stay on four sums in auto, and so does a NaN threshold;
//   - the stats mapping, and reset.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "screen_policy.hpp"

using namespace wld::screen_policy;

namespace {
int g_fail = 0;
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

Options opts(int screen, int fp6, int three) {
    Options o{screen, fp6, false, true, true};
    o.fp6_three = three;
    return o;
}
const LoadFacts kLoad{true, true, true, 2048, 1u, true, true};
PassFacts pass(uint32_t n_tiles, float thr, bool have_pairs = true) { return {have_pairs, n_tiles, thr, false, false, false}; }

uint64_t product_part() {
    uint64_t points = 0;
    const float thrs[] = {0.0f, 0.01f, 0.05f, 0.3f, NAN};
    const float goods[] = {INFINITY, 0.05f, 0.01f};
    for (int screen = 0; screen <= 4; ++screen)
        for (int fp6 = 0; fp6 <= 3; ++fp6)
            for (int ref = 0; ref < 2; ++ref)
                for (int i8 = 0; i8 < 2; ++i8)
                    for (int ok = 0; ok < 4; ++ok)
                        for (int mfma = 0; mfma < 2; ++mfma)
                            for (unsigned planes : {1u, 7u})
                                for (int hp = 0; hp < 2; ++hp)
                                    for (uint32_t n_tiles : {100u, 2047u, 2048u, 50000u})
                                        for (float thr : thrs)
                                            for (float bad : {-1.0f, 0.05f})
                                                for (float good : goods) {
                                                    Learned s;
                                                    s.fp6_bad = bad;
                                                    s.fp6_three_good = good;
                                                    const LoadFacts l{mfma != 0, true, true, 2048, planes, (ok & 1) != 0, (ok & 2) != 0};
                                                    const PassFacts p = pass(n_tiles, thr, hp != 0);
                                                    Plan plan[3];
                                                    for (int three = 0; three < 3; ++three) {
                                                        Options o{screen, fp6, ref != 0, true, i8 != 0};
                                                        o.fp6_three = three;
                                                        plan[three] = decide(o, l, p, s);
                                                        const Plan &q = plan[three];
                                                        CHECK(q.route == plan[0].route && q.bound_test == plan[0].bound_test &&
                                                                  q.fp6_bail == plan[0].fp6_bail && q.i8_images == plan[0].i8_images,
                                                              "option %d moved the plan (screen %d fp6 %d thr %g)", three, screen, fp6, thr);
                                                        const bool fp6_pairs = q.route == Route::Fp6Screen && hp;
                                                        const bool want = fp6_pairs && (three == 2 || (three == 1 && thr >= good));
                                                        CHECK(q.fp6_three == want, "fp6_three %d, not %d (option %d thr %g good %g pairs %d route %d)",
                                                              (int)q.fp6_three, (int)want, three, thr, good, hp, (int)q.route);
                                                        CHECK(stat_fp6_three(q) == (want ? 1 : 0), "stat");
                                                        ++points;
                                                    }
                                                    CHECK(!plan[0].fp6_three, "option 0 on three sums");
                                                }
    return points;
}

void learn_part() {
    // 400 sampled tiles are at least 200 entries: an eighth is 25
    Learned s;
    learn(s, Sample{0.05f, 0, 400, true, 26});
    CHECK(s.fp6_good == 0.05f && s.fp6_three_good == INFINITY, "26 of >= 200 entries taken: %g", s.fp6_three_good);
    learn(s, Sample{0.05f, 0, 400, true, 25});
    CHECK(s.fp6_three_good == 0.05f, "25 of >= 200 entries refused: %g", s.fp6_three_good);
    // (an odd tile count: 401 tiles are at least 201 entries)
    s.reset();
    learn(s, Sample{0.05f, 0, 401, true, 25});
    CHECK(s.fp6_three_good == 0.05f, "25 of >= 201 refused");
    // monotone: a higher threshold's sample does not raise it, a lower one's lowers it, a bad one leaves it
    learn(s, Sample{0.1f, 0, 400, true, 0});
    CHECK(s.fp6_three_good == 0.05f, "raised to %g", s.fp6_three_good);
    learn(s, Sample{0.02f, 0, 400, true, 100});
    CHECK(s.fp6_three_good == 0.05f && s.fp6_good == 0.02f, "a refused sample moved it: %g", s.fp6_three_good);
    learn(s, Sample{0.01f, 0, 400, true, 3});
    CHECK(s.fp6_three_good == 0.01f, "not lowered: %g", s.fp6_three_good);
    // never from a four-sum sample (option 0, or no pair list) ...
    s.reset();
    learn(s, Sample{0.05f, 0, 400});
    learn(s, Sample{0.05f, 0, 400, false, 0});
    CHECK(s.fp6_good == 0.05f && s.fp6_three_good == INFINITY, "a four-sum sample taught three sums");
    // ... nor from a sample that leaves more than a sixteenth of the tiles, nor from an empty one
    s.reset();
    learn(s, Sample{0.05f, 26, 400, true, 0});
    CHECK(s.fp6_bad == 0.05f && s.fp6_good == INFINITY && s.fp6_three_good == INFINITY, "a bad sample taught three sums");
    s.reset();
    learn(s, Sample{0.05f, 0, 0, true, 0});
    CHECK(s.fp6_three_good == INFINITY, "an empty sample taught three sums");
    // what the pass then does, and reset
    s.reset();
    learn(s, Sample{0.05f, 1, 400, true, 2});
    const Options a = opts(1, 1, 1);
    CHECK(decide(a, kLoad, pass(50000, 0.05f), s).fp6_three, "auto at the sampled threshold");
    CHECK(decide(a, kLoad, pass(50000, 0.3f), s).fp6_three, "auto above it");
    CHECK(!decide(a, kLoad, pass(50000, 0.04f), s).fp6_three, "auto below it");
    CHECK(!decide(a, kLoad, pass(50000, NAN), s).fp6_three, "auto at NaN");
    CHECK(!decide(a, kLoad, pass(50000, 0.05f, false), s).fp6_three, "auto without a pair list");
    CHECK(!wants_sample(a, kLoad, pass(50000, 0.05f), s), "sampled again at a settled threshold");
    s.reset();
    CHECK(s.fp6_three_good == INFINITY && !decide(a, kLoad, pass(50000, 0.05f), s).fp6_three, "reset");
}

void unsampled_part() {
    const Learned fresh;
    // fewer than 2,048 tiles: no sample, so auto stays on four sums; option 2 does not
    for (uint32_t n_tiles : {1u, 136u, 2047u}) {
        CHECK(!wants_sample(opts(1, 1, 1), kLoad, pass(n_tiles, 0.05f), fresh), "%u tiles sampled", n_tiles);
        const Plan p = decide(opts(1, 1, 1), kLoad, pass(n_tiles, 0.05f), fresh);
        CHECK(p.route == Route::Fp6Screen && !p.fp6_three, "%u tiles: auto on three sums", n_tiles);
        CHECK(decide(opts(1, 1, 2), kLoad, pass(n_tiles, 0.05f), fresh).fp6_three, "%u tiles: option 2 on four", n_tiles);
        CHECK(!decide(opts(1, 1, 0), kLoad, pass(n_tiles, 0.05f), fresh).fp6_three, "%u tiles: option 0 on three", n_tiles);
    }
    // WLD_OPT_SCREEN_FP6 2 (forced) and 3 (auto without the sample run): never sampled
    for (int fp6 : {2, 3}) {
        CHECK(!wants_sample(opts(1, fp6, 1), kLoad, pass(50000, 0.05f), fresh), "fp6 %d sampled", fp6);
        const Plan p = decide(opts(1, fp6, 1), kLoad, pass(50000, 0.05f), fresh);
        CHECK(p.route == Route::Fp6Screen && !p.fp6_three, "fp6 %d: auto on three sums", fp6);
        CHECK(decide(opts(1, fp6, 2), kLoad, pass(50000, 0.05f), fresh).fp6_three, "fp6 %d: option 2 on four", fp6);
    }
    // a long list in auto is sampled first
    CHECK(wants_sample(opts(1, 1, 1), kLoad, pass(2048, 0.05f), fresh), "2,048 tiles not sampled");
    CHECK(!decide(opts(1, 1, 1), kLoad, pass(2048, 0.05f), fresh).fp6_three, "three sums before any sample");
    // a pass's outcome teaches the other thresholds, never this one
    Learned s;
    learn(s, Outcome{Route::Fp6Screen, 0.05f, false, 0, 50000, 0, 1});
    learn(s, Outcome{Route::Fp6Screen, 0.05f, true, 0, 50000, 0, 1});
    CHECK(s.fp6_three_good == INFINITY, "an outcome taught three sums");
    CHECK(stat_fp6_three(Plan{Route::I8PairScreen, true, 0, true, true}) == 0, "stat of another route");
}
}  // namespace

int main() {
    const uint64_t points = product_part();
    printf("plans: %llu points\n", (unsigned long long)points);
    learn_part();
    unsampled_part();
    if (g_fail) {
        printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("OK\n");
    return 0;
}
