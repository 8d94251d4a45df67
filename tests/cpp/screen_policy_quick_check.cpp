// Host check of the quick-test rule in weightedld_amd/csrc/screen_policy.hpp
// (stand-alone; built plain and with -fsanitize=address,undefined by
// tests/test_screen_policy_quick.py).
//
//   - WLD_OPT_FP6_QUICK changes nothing of a plan but Plan::fp6_quick, and
//     fp6_quick is set only where fp6_three is (the Fp6Screen route on a
//     tile-pair list, on three sums);
//   - option 0 never, option 2 wherever the three-sum kernel runs, option 1
//     (auto) only at or above a threshold a sample run has allowed;
//   - the sample's rule: the quick test where at most a quarter of the sampled
//     row blocks (four per tile) fell through, learned monotonically in the
//     threshold, never from a sample without the quick test or on four sums,
//     never from a sample that sends the threshold to the i8 screen;
//   - lists without a sample stay off in auto, and so does a NaN threshold;
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

Options opts(int screen, int fp6, int three, int quick) {
    Options o{screen, fp6, false, true, true};
    o.fp6_three = three;
    o.fp6_quick = quick;
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
            for (int three = 0; three <= 2; ++three)
                for (int hp = 0; hp < 2; ++hp)
                    for (uint32_t n_tiles : {100u, 2048u, 50000u})
                        for (float thr : thrs)
                            for (float good3 : goods)
                                for (float goodq : goods) {
                                    Learned s;
                                    s.fp6_three_good = good3;
                                    s.fp6_quick_good = goodq;
                                    Plan plan[3];
                                    for (int quick = 0; quick <= 2; ++quick) {
                                        const Plan q = decide(opts(screen, fp6, three, quick), kLoad, pass(n_tiles, thr, hp), s);
                                        plan[quick] = q;
                                        ++points;
                                        const bool want = q.fp6_three && (quick == 2 || (quick == 1 && thr >= goodq));
                                        CHECK(q.fp6_quick == want, "fp6_quick %d, not %d (option %d three %d thr %g good %g)",
                                              (int)q.fp6_quick, (int)want, quick, three, thr, goodq);
                                        CHECK(!q.fp6_quick || (q.route == Route::Fp6Screen && q.fp6_three && hp), "quick without three sums");
                                        CHECK(stat_fp6_quick(q) == (want ? 1 : 0), "stat");
                                    }
                                    for (int quick = 1; quick <= 2; ++quick)
                                        CHECK(plan[quick].route == plan[0].route && plan[quick].bound_test == plan[0].bound_test &&
                                                  plan[quick].fp6_bail == plan[0].fp6_bail && plan[quick].i8_images == plan[0].i8_images &&
                                                  plan[quick].fp6_three == plan[0].fp6_three,
                                              "option %d moved the plan", quick);
                                    CHECK(!plan[0].fp6_quick, "option 0 ran the quick test");
                                }
    return points;
}

void learn_part() {
    Learned s;
    // 1,000 tiles sampled: 4,000 row blocks, a quarter is 1,000
    learn(s, Sample{0.05f, 10, 1000, true, 3, true, 1001});
    CHECK(s.fp6_good == 0.05f && s.fp6_three_good == 0.05f && s.fp6_quick_good == INFINITY, "1,001 of 4,000 taken: %g", s.fp6_quick_good);
    learn(s, Sample{0.05f, 10, 1000, true, 3, true, 1000});
    CHECK(s.fp6_quick_good == 0.05f, "1,000 of 4,000 refused: %g", s.fp6_quick_good);
    learn(s, Sample{0.1f, 0, 1000, true, 0, true, 0});
    CHECK(s.fp6_quick_good == 0.05f, "raised to %g", s.fp6_quick_good);
    learn(s, Sample{0.02f, 10, 1000, true, 3, true, 4000});
    CHECK(s.fp6_quick_good == 0.05f && s.fp6_good == 0.02f, "a refused sample moved it: %g", s.fp6_quick_good);
    learn(s, Sample{0.01f, 10, 1000, true, 3, true, 0});
    CHECK(s.fp6_quick_good == 0.01f, "not lowered: %g", s.fp6_quick_good);
    s.reset();
    learn(s, Sample{0.05f, 10, 1000, true, 3, false, 0});
    CHECK(s.fp6_three_good == 0.05f && s.fp6_quick_good == INFINITY, "a sample without the quick test taught it");
    s.reset();
    learn(s, Sample{0.05f, 10, 1000, false, 0, true, 0});
    CHECK(s.fp6_quick_good == INFINITY, "a four-sum sample taught it");
    s.reset();
    learn(s, Sample{0.05f, 100, 1000, true, 3, true, 0});
    CHECK(s.fp6_bad == 0.05f && s.fp6_quick_good == INFINITY, "a bad sample taught it");
    learn(s, Sample{0.05f, 0, 0, true, 0, true, 0});
    CHECK(s.fp6_quick_good == INFINITY, "an empty sample taught it");
    // the three-sum sample that allows the quick test but not three sums leaves it unused
    s.reset();
    learn(s, Sample{0.05f, 10, 1000, true, 500, true, 10});
    CHECK(s.fp6_three_good == INFINITY && s.fp6_quick_good == 0.05f, "learned apart");
    CHECK(!decide(opts(1, 1, 1, 1), kLoad, pass(50000, 0.05f), s).fp6_quick, "auto without three sums");
    // auto
    s.reset();
    learn(s, Sample{0.05f, 10, 1000, true, 3, true, 10});
    const Options a = opts(1, 1, 1, 1);
    CHECK(decide(a, kLoad, pass(50000, 0.05f), s).fp6_quick, "auto at the sampled threshold");
    CHECK(decide(a, kLoad, pass(50000, 0.3f), s).fp6_quick, "auto above it");
    CHECK(!decide(a, kLoad, pass(50000, 0.04f), s).fp6_quick, "auto below it");
    CHECK(!decide(a, kLoad, pass(50000, NAN), s).fp6_quick, "auto at NaN");
    CHECK(!decide(a, kLoad, pass(50000, 0.05f, false), s).fp6_quick, "auto without a pair list");
    CHECK(!decide(opts(1, 1, 0, 2), kLoad, pass(50000, 0.05f), s).fp6_quick, "option 2 on four sums");
    s.reset();
    CHECK(s.fp6_quick_good == INFINITY && !decide(a, kLoad, pass(50000, 0.05f), s).fp6_quick, "reset");
    // lists that are not sampled stay off in auto
    const Learned fresh;
    for (int fp6 : {2, 3}) {
        CHECK(!decide(opts(1, fp6, 2, 1), kLoad, pass(50000, 0.05f), fresh).fp6_quick, "fp6 %d: auto ran the quick test", fp6);
        CHECK(decide(opts(1, fp6, 2, 2), kLoad, pass(50000, 0.05f), fresh).fp6_quick, "fp6 %d: option 2 did not", fp6);
    }
    CHECK(!decide(opts(1, 1, 2, 1), kLoad, pass(100, 0.05f), fresh).fp6_quick, "a short list before any sample");
    // a pass's outcome teaches nothing here
    s.reset();
    learn(s, Outcome{Route::Fp6Screen, 0.05f, false, 0, 50000, 0, 1});
    CHECK(s.fp6_quick_good == INFINITY, "an outcome taught the quick test");
    Plan other;
    other.route = Route::I8PairScreen;
    other.fp6_three = other.fp6_quick = true;
    CHECK(stat_fp6_quick(other) == 0, "stat of another route");
}
}  // namespace

int main() {
    const uint64_t points = product_part();
    learn_part();
    printf("%llu plans\n", (unsigned long long)points);
    if (g_fail) {
        printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("OK\n");
    return 0;
}
