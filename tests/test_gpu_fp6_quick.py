"""The quick test in front of the three-sum fp6 screen's per-pair test
(WLD_OPT_FP6_QUICK, "fp6_quick"): pair_fp6_screen2w_kernel<., true, true>
first tries to reject a lane's 16 pairs of a row block together, from one
numerator maximum and marginal bounds shared by the lane (pair_common.hpp
f6q_pair / f6q_lane_terms), and runs today's per-pair test only for the row
blocks where some lane cannot.  A row block the quick test rejects holds no
pair the per-pair test keeps, so for every case here option 0 (off) and option
2 (wherever the three-sum kernel runs), both under "fp6_three" 2, must give
the oracle's rows bit for bit and equal candidate tiles, sub-blocks and second
passes, with wld_run_stats.fp6_quick 0 and 1.

The cases are test_gpu_fp6_three.py's: the planted 1,024 x 2,000 case (unit
weights: the shared image) and the small shapes (the three formats, one and
two stages, a padded last tile, a filtered site, diagonal tiles).
fp6_quick_full counts the row blocks (16 sites x a 64-site tile) that fell
through to the per-pair test.  A diagonal tile never takes the quick test (its
row blocks hold pairs of a site with itself) and is not counted, so the planted
case has 4 x 120 row blocks that can fall through, of its 4 x 136.  At 0.05 the
planted pairs' row blocks do and most of the background's do not; at 0.5 on the
background alone none does; at 0.005 the background's noise (r2 ~ 1 / 1,600 per
pair against a bound whose worst ratio to 0.05 is already 0.8) leaves no lane
rejected: at least 9/10 of the 480 must fall through.
"""
import numpy as np
import pytest

import _oracle as O
import test_gpu_fp6_three as T

pytestmark = pytest.mark.gpu

L_PLANTED = 1024
TILES = (L_PLANTED // 64) * (L_PLANTED // 64 + 1) // 2
ROW_BLOCKS = 4 * TILES                                # 544
ROW_BLOCKS_OFF = 4 * (TILES - L_PLANTED // 64)        # 480: off the diagonal


@pytest.fixture(scope="module")
def W():
    import weightedld_amd as W
    return W


def _run(W, buf, w, refs, quick, kind=None):
    return T._run(W, buf, w, refs, 2, kind, opts=(("screen_fp6", 2), ("fp6_quick", quick)))


def _same_verdicts(label, off, on):
    for thr in off:
        a, b = off[thr], on[thr]
        print("%s thr %g: rows %d, candidate tiles / sub-blocks / rechecked %d / %d / %d (off), %d / %d / %d (quick), "
              "row blocks fallen through %d"
              % (label, thr, b["rows"], a["candidate_tiles"], a["candidate_blocks"], a["fp6_rechecked"],
                 b["candidate_tiles"], b["candidate_blocks"], b["fp6_rechecked"], b["fp6_quick_full"]))
        for st in (a, b):
            assert st["screened"] == 1 and st["screen_fp6"] == 1 and st["fp6_three"] == 1, st
        assert a["fp6_quick"] == 0 and a["fp6_quick_full"] == 0, a
        assert b["fp6_quick"] == 1, b
        assert (a["candidate_tiles"], a["candidate_blocks"], a["fp6_rechecked"]) == \
               (b["candidate_tiles"], b["candidate_blocks"], b["fp6_rechecked"]), (a, b)


@pytest.fixture(scope="module")
def planted_runs(W):
    buf, w, refs = T._planted_case()
    off, on = _run(W, buf, w, refs, 0, "unit"), _run(W, buf, w, refs, 2, "unit")
    _same_verdicts("planted", off, on)
    return refs, on


def test_quick_option_round_trip(W):
    c = W.Context(0)
    assert c.get_option("fp6_quick") == 1
    for v in (0, 2, 1):
        c.set_option("fp6_quick", v)
        assert c.get_option("fp6_quick") == v
    with pytest.raises(W.WldError):
        c.set_option("fp6_quick", 3)
    c.close()


def test_quick_planted_both_paths(planted_runs):
    """thr 0.05: some row blocks fall through (the planted pairs'), not all."""
    refs, on = planted_runs
    st = on[0.05]
    assert 0 < st["fp6_quick_full"] < ROW_BLOCKS, st
    # every entry in doubt holds a row block that fell through, unless it is diagonal
    assert st["fp6_quick_full"] <= ROW_BLOCKS_OFF, st


def test_quick_planted_low_threshold(planted_runs):
    """thr 0.005: nearly every row block off the diagonal falls through."""
    refs, on = planted_runs
    st = on[0.005]
    assert ROW_BLOCKS_OFF * 9 // 10 <= st["fp6_quick_full"] <= ROW_BLOCKS_OFF, st


def test_quick_background_high_threshold(W):
    """thr 0.5 on the background alone: no row block falls through."""
    import bench
    buf = bench.synth(L_PLANTED, 2000)
    w = T._weights("unit", 2000)
    ref = {0.5: O.all_pairs(buf, w, np.float32(0.5))}
    assert len(ref[0.5]["site_a"]) == 0
    off, on = _run(W, buf, w, ref, 0, "unit"), _run(W, buf, w, ref, 2, "unit")
    _same_verdicts("background", off, on)
    assert on[0.5]["fp6_quick_full"] == 0 and on[0.5]["fp6_rechecked"] == 0 and on[0.5]["candidate_tiles"] == 0, on[0.5]


@pytest.mark.parametrize("kind", sorted(T.FORMAT))
@pytest.mark.parametrize("L,N,dropped", T.SHAPES)
def test_quick_small_shapes(W, L, N, dropped, kind):
    import bench
    buf = T._plant(bench.synth(L, N, seed=0x73 + 5 * L + N), [p for p in T.SMALL_PLANTED if p[1] < L], L + N)
    if dropped:
        for i, s in enumerate(T.DROPPED):
            buf[s] = i
    w = T._weights(kind, N)
    refs = {thr: O.all_pairs(buf, w, np.float32(thr)) for thr in (0.05, 0.5)}
    assert len(refs[0.5]["site_a"]) > 0
    off, on = _run(W, buf, w, refs, 0, kind), _run(W, buf, w, refs, 2, kind)
    _same_verdicts("L %d N %d %s%s" % (L, N, kind, " dropped" if dropped else ""), off, on)
    tiles = ((L + 63) // 64) * ((L + 63) // 64 + 1) // 2
    for thr in refs:
        assert on[thr]["fp6_quick_full"] <= 4 * (tiles - (L + 63) // 64), (thr, on[thr])


def _stats(W, buf, w, thr, opts):
    c = W.Context(0)
    for k, v in opts:
        c.set_option(k, v)
    c.load(buf, w)
    n = c.run(thr)
    st = c.stats()
    c.close()
    return n, st


def test_quick_auto(W):
    """Auto (the default) on C4-like data: 2,080 tiles of random background
    with unit weights, so the sample run decides.  At 0.3 (N = 256: a pair's
    r2 is ~ 1 / 200) nothing falls through in the sample: the pass runs the
    quick test, with the verdicts of the pass without it.  A list without a
    sample (WLD_OPT_SCREEN_FP6 3) stays off, and so does four sums
    (WLD_OPT_FP6_THREE 0).  Linkage blocks at 0.05: the sample sends the pass
    to the i8 screen, and the quick test is not chosen."""
    import bench
    L, N = 4096, 256
    w = T._weights("unit", N)
    buf = bench.synth(L, N)
    n, st = _stats(W, buf, w, 0.3, ())
    print("auto, background:", st)
    assert st["screen_fp6"] == 1 and st["fp6_sampled"] == 1 and st["fp6_three"] == 1 and st["fp6_quick"] == 1, st
    assert st["fp6_quick_full"] <= st["tiles"], st  # (a quarter of the row blocks, four per tile)
    n0, st0 = _stats(W, buf, w, 0.3, (("fp6_quick", 0),))
    assert st0["fp6_three"] == 1 and st0["fp6_quick"] == 0 and st0["fp6_quick_full"] == 0, st0
    assert (n0, st0["candidate_tiles"], st0["candidate_blocks"], st0["fp6_rechecked"]) == \
           (n, st["candidate_tiles"], st["candidate_blocks"], st["fp6_rechecked"]), (st0, st)
    n3, st3 = _stats(W, buf, w, 0.3, (("screen_fp6", 3),))
    assert n3 == n and st3["screen_fp6"] == 1 and st3["fp6_sampled"] == 0 and st3["fp6_quick"] == 0, st3
    n4, st4 = _stats(W, buf, w, 0.3, (("fp6_three", 0), ("fp6_quick", 2)))
    assert n4 == n and st4["fp6_three"] == 0 and st4["fp6_quick"] == 0 and st4["fp6_quick_full"] == 0, st4
    buf = bench.ld_blocks(L, N)
    nb, stb = _stats(W, buf, w, 0.05, ())
    print("auto, linkage blocks:", stb)
    assert stb["fp6_quick"] == 0 and stb["fp6_quick_full"] == 0, stb
