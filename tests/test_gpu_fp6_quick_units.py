"""The tile-pair fp6 screen's three-sum tests on per-load site records, in
count units where the load's one weight code is a power of two, with the quick
test on the one-sided cap (pair_common.hpp F6RowRec, f6q_pair1;
pair_fp6_screen2w_kernel<., true, ., kCounts>).  Nothing of this may change a
verdict: for every case here "fp6_quick" 0 and 2 (under "fp6_three" 2) must
give the oracle's rows bit for bit and equal candidate tiles, sub-blocks and
second passes.

Cases: test_gpu_fp6_quick.py's small shapes (one and two stages, a padded last
tile, a filtered site, diagonal tiles) in the three formats, and the planted
1,024 x 2,000 case.  The shared format runs in both of its units: unit weights
land on the code of 4.0 (count units), and every weight 0.9 lands on the code
of 4.5, which is no power of two (the scaled path: with one weight value every
scale has a residual of rounding size only, and for 0.9 the smallest is not
the median's).  The codes are asserted.  One windowed pass, and two loads on
one context whose codes differ, so that the second load's records replace the
first's (units and values both change).
"""
import numpy as np
import pytest

import _oracle as O
import test_gpu_fp6_complement as C
import test_gpu_fp6_quick as Q
import test_gpu_fp6_three as T

pytestmark = pytest.mark.gpu

# kind: (fp6_shared, fp6_a4 or None, the load's single code or None)
CODE_4, CODE_4_5 = 24, 25  # e2m3 codes of 4.0 and 4.5
KINDS = {"unit": (1, None, CODE_4), "nine": (1, None, CODE_4_5), "two": (0, 1, None), "spread": (0, 0, None)}


@pytest.fixture(scope="module")
def W():
    import weightedld_amd as W
    return W


def _weights(kind, N):
    return np.full(N, 0.9, dtype=np.float32) if kind == "nine" else T._weights(kind, N)


def _check_format(W, buf, w, kind, stats):
    shared, a4, code = KINDS[kind]
    for st in stats.values():
        assert st["fp6_shared"] == shared and (a4 is None or st["fp6_a4"] == a4), (kind, st)
    if code is not None:
        c = W.Context(0)
        c.set_option("screen_fp6", 2)
        c.load(buf, w)
        codes = set(c.fp6_weight_codes(buf.shape[1])[0].tolist())
        c.close()
        assert codes == {code}, (kind, sorted(codes))


def _both(W, label, buf, w, refs, kind):
    off, on = Q._run(W, buf, w, refs, 0), Q._run(W, buf, w, refs, 2)
    Q._same_verdicts(label, off, on)
    _check_format(W, buf, w, kind, on)
    return on


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("L,N,dropped", T.SHAPES)
def test_units_small_shapes(W, L, N, dropped, kind):
    import bench
    buf = T._plant(bench.synth(L, N, seed=0x73 + 5 * L + N), [p for p in T.SMALL_PLANTED if p[1] < L], L + N)
    if dropped:
        for i, s in enumerate(T.DROPPED):
            buf[s] = i
    w = _weights(kind, N)
    refs = {thr: O.all_pairs(buf, w, np.float32(thr)) for thr in (0.05, 0.5)}
    assert len(refs[0.5]["site_a"]) > 0
    on = _both(W, "L %d N %d %s%s" % (L, N, kind, " dropped" if dropped else ""), buf, w, refs, kind)
    tiles = ((L + 63) // 64) * ((L + 63) // 64 + 1) // 2
    for thr in refs:
        assert on[thr]["fp6_quick_full"] <= 4 * (tiles - (L + 63) // 64), (thr, on[thr])


_cache = {}


def _planted(kind):
    """The planted case's buffer, weights and oracle rows at 0.05 (unit weights: test_gpu_fp6_three's, shared)."""
    if kind == "unit":
        buf, w, refs = T._planted_case()
        return buf, w, {0.05: refs[0.05]}
    if kind not in _cache:
        buf = T._planted_case()[0]
        w = _weights(kind, buf.shape[1])
        _cache[kind] = (buf, w, {0.05: O.all_pairs(buf, w, np.float32(0.05))})
    return _cache[kind]


@pytest.mark.parametrize("kind", ["unit", "nine"])
def test_units_planted(W, kind):
    """thr 0.05 in both units of the shared format: the planted pairs' row
    blocks fall through the quick test, the background's mostly do not."""
    buf, w, refs = _planted(kind)
    on = _both(W, "planted %s" % kind, buf, w, refs, kind)
    st = on[0.05]
    assert 0 < st["fp6_quick_full"] <= Q.ROW_BLOCKS_OFF // 2, st
    assert 0 < st["fp6_rechecked"] < T.n_entries(Q.L_PLANTED), st


def test_units_window(W):
    """A windowed pass (b - a <= 300 sites) on the planted case: the oracle's rows inside the window, quick off and on."""
    buf, w, refs = _planted("unit")
    ref = refs[0.05]
    keep = (ref["site_b"].astype(np.int64) - ref["site_a"].astype(np.int64)) <= 300
    assert keep.any() and not keep.all()
    exp = {k: v[keep] for k, v in ref.items() if isinstance(v, np.ndarray) and len(v) == len(keep)}
    got = {}
    for quick in (0, 2):
        c = W.Context(0)
        for k, v in (("screen_fp6", 2), ("fp6_three", 2), ("fp6_quick", quick)):
            c.set_option(k, v)
        c.set_window(max_sites=300)
        c.load(buf, w)
        n = c.run(0.05)
        st = c.stats()
        assert n == int(keep.sum()), (n, int(keep.sum()))
        C._bits_equal(c.rows(), exp)
        assert st["screen_fp6"] == 1 and st["fp6_three"] == 1 and st["fp6_quick"] == (1 if quick else 0), st
        got[quick] = st
        c.close()
    a, b = got[0], got[2]
    print("window: candidate tiles / sub-blocks / rechecked %d / %d / %d, row blocks fallen through %d"
          % (b["candidate_tiles"], b["candidate_blocks"], b["fp6_rechecked"], b["fp6_quick_full"]))
    assert (a["candidate_tiles"], a["candidate_blocks"], a["fp6_rechecked"]) == \
           (b["candidate_tiles"], b["candidate_blocks"], b["fp6_rechecked"]), (a, b)


def test_units_two_loads_one_context(W):
    """Two loads on one context, the second with other weights and another
    code (4.0 then 4.5, then the several codes of the fp6 A image): each pass
    reads its own load's records."""
    import bench
    L, N = 200, 130
    buf = T._plant(bench.synth(L, N, seed=0x73 + 5 * L + N), [p for p in T.SMALL_PLANTED if p[1] < L], L + N)
    buf2 = T._plant(bench.synth(L, N, seed=0x99), [p for p in T.SMALL_PLANTED if p[1] < L], 7)
    loads = [(buf, _weights("unit", N), "unit"), (buf2, _weights("nine", N), "nine"), (buf, _weights("spread", N), "spread"),
             (buf2, _weights("unit", N), "unit")]
    refs = [{thr: O.all_pairs(b, w, np.float32(thr)) for thr in (0.05, 0.5)} for b, w, _ in loads]
    stats = {}
    for quick in (0, 2):
        c = W.Context(0)
        for k, v in (("screen_fp6", 2), ("fp6_three", 2), ("fp6_quick", quick)):
            c.set_option(k, v)
        for i, (b, w, kind) in enumerate(loads):
            c.load(b, w)
            for thr, ref in refs[i].items():
                n = c.run(thr)
                st = c.stats()
                assert n == len(ref["site_a"]), (quick, i, thr, n, len(ref["site_a"]))
                C._bits_equal(c.rows(), ref)
                assert st["screen_fp6"] == 1 and st["fp6_three"] == 1 and st["fp6_shared"] == KINDS[kind][0], (kind, st)
                stats[(quick, i, thr)] = st
            if KINDS[kind][2] is not None:
                assert set(c.fp6_weight_codes(N)[0].tolist()) == {KINDS[kind][2]}, kind
        c.close()
    for (quick, i, thr), st in stats.items():
        if quick == 2:
            a = stats[(0, i, thr)]
            assert (a["candidate_tiles"], a["candidate_blocks"], a["fp6_rechecked"]) == \
                   (st["candidate_tiles"], st["candidate_blocks"], st["fp6_rechecked"]), (i, thr, a, st)
