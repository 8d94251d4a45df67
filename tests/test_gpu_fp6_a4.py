"""The fp6 screen's fp4 A image (WLD_OPT_FP6_A4, "fp6_a4"): where every rounded
weight of a load is also an e2m1 value (fp6_scale.hpp fp6_codes_fit_fp4) the A
operand image is fp4 nibbles, read by pair_fp6_screen2w_kernel<true>,
pair_fp6_screen_kernel<true> and the sample run.  Every product is exact in
either format, so the sums, the verdicts and the candidate sets are the fp6
image's bit for bit: beside rows, order and every bit of d, d', r2 against the
oracle, candidate tiles must be equal between "fp6_a4" 0 and 1, and on the unit
and Henikoff cases equal tests/test_gpu_fp6_complement.py's PARENT_CANDIDATES.

Inputs are that module's (L = 160: one pair entry, single entries, three
diagonal tiles, a padded last tile; N = 130 two K stages with 126 padded
sequences, 128 one, 1 a single sequence; with and without dropped sites).
Weights: unit, {1, 0.5} and {1, 0.75} (codes 24 / 16 and 24 / 20: fp4),
{1, 0.875} (24 / 22: stays fp6), Henikoff (whatever the scale rule gives: the
field is checked against the predicate on the load's own codes).  With N = 1
a two-valued set is its first value alone, one code on 4.0, and fits.
"""
import numpy as np
import pytest

import _oracle as O
import test_gpu_fp6_complement as C

pytestmark = pytest.mark.gpu

WEIGHTS = ("unit", "half", "threeq", "seveneighths", "henikoff")
SECOND = {"half": 0.5, "threeq": 0.75, "seveneighths": 0.875}
# two-valued sets with both values present: does the committed scale rule leave them on e2m1 values?
FITS = {"unit": True, "half": True, "threeq": True, "seveneighths": False}


@pytest.fixture(scope="module")
def W():
    import weightedld_amd as W
    return W


def _weights(W, buf, kind):
    if kind in ("unit", "henikoff"):
        return C._weights(W, buf, kind)
    w = np.ones(buf.shape[1], dtype=np.float32)
    w[1::2] = SECOND[kind]
    return w


_cache = {}


def _case(W, N, weights, dropped):
    """(buf, w, {thr: oracle rows}), computed once per input (the complement module's own where it has them)."""
    if weights in ("unit", "henikoff"):
        return C._small_case(W, N, weights, dropped)
    key = (N, weights, dropped)
    if key not in _cache:
        buf = C._small_input(N, dropped)
        w = _weights(W, buf, weights)
        _cache[key] = (buf, w, {thr: O.all_pairs(buf, w, np.float32(thr)) for thr in C.THRESHOLDS})
    return _cache[key]


def _check_pass(c, n, ref, forced, a4, fits):
    st = c.stats()
    fp6 = st["screened"] == 1 and st["screen_fp6"] == 1
    if forced:
        assert fp6, st
    assert n == len(ref["site_a"])
    C._bits_equal(c.rows(), ref)
    if st["screened"] == 1:
        assert st["candidate_tiles"] >= len(C._row_tiles(ref)), (st, sorted(C._row_tiles(ref)))
    assert st["fp6_a4"] == (1 if fp6 and a4 and fits else 0), (st, a4, fits)
    return st["candidate_tiles"] if fp6 else -1


@pytest.mark.parametrize("dropped", [False, True])
@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("N", C.SIZES)
def test_fp6_a4_small_shapes(W, N, weights, dropped):
    buf, w, refs = _case(W, N, weights, dropped)
    got = {}
    fits_seen = set()
    for mode, opts in C.MODES:
        for a4 in (0, 1):
            c = W.Context(0)
            for k, v in opts.items():
                c.set_option(k, v)
            c.set_option("fp6_a4", a4)
            assert c.get_option("fp6_a4") == a4
            c.load(buf, w)
            codes, fits = c.fp6_weight_codes(N)
            assert fits == bool(np.all(codes % 4 == 0)), codes
            if weights in FITS:
                assert fits == (FITS[weights] or N == 1), (weights, sorted(set(codes.tolist())))
            fits_seen.add(fits)
            for thr in C.THRESHOLDS:
                n = c.run(thr)
                got[(mode, thr, a4)] = _check_pass(c, n, refs[thr], bool(opts), a4, fits)
            c.close()
    assert len(fits_seen) == 1
    for mode, _ in C.MODES:
        for thr in C.THRESHOLDS:
            key = "%d/%s/%d/%s/%g" % (N, weights, int(dropped), mode, thr)
            print("candidate tiles %s: fp6 A %d, fp4 A %d, fits %s" % (key, got[(mode, thr, 0)], got[(mode, thr, 1)],
                                                                         fits_seen))
    for mode, _ in C.MODES:
        for thr in C.THRESHOLDS:
            key = "%d/%s/%d/%s/%g" % (N, weights, int(dropped), mode, thr)
            assert got[(mode, thr, 0)] == got[(mode, thr, 1)], (key, got[(mode, thr, 0)], got[(mode, thr, 1)])
            if weights in ("unit", "henikoff"):
                assert got[(mode, thr, 1)] == C.PARENT_CANDIDATES[key], (key, got[(mode, thr, 1)])


def test_fp6_a4_reload(W):
    """One context through an fp4 load, an fp6 load and an fp4 load again: each
    load builds its own A image, and an option change discards a built one."""
    N = 130
    c = W.Context(0)
    c.set_option("screen_fp6", 2)
    for weights in ("unit", "seveneighths", "unit"):
        buf, w, refs = _case(W, N, weights, False)
        c.load(buf, w)
        fits = c.fp6_weight_codes(N)[1]
        assert fits == FITS[weights]
        for thr in C.THRESHOLDS:
            _check_pass(c, c.run(thr), refs[thr], True, 1, fits)
    # the same load, the option off and on again
    thr = C.THRESHOLDS[0]
    for a4 in (0, 1):
        c.set_option("fp6_a4", a4)
        _check_pass(c, c.run(thr), refs[thr], True, a4, True)
    c.close()


def test_fp6_a4_random_background(W):
    """Random background alone (L 1024, N 2000, unit weights, thr 0.05): no
    row, and the same candidate tiles from either A image."""
    import bench
    L, N, thr = 1024, 2000, 0.05
    buf = bench.synth(L, N)
    w = np.ones(N, dtype=np.float32)
    ref = O.all_pairs(buf, w, np.float32(thr))
    assert len(ref["site_a"]) == 0
    cand = []
    for a4 in (0, 1):
        c = W.Context(0)
        c.set_option("screen_fp6", 2)
        c.set_option("fp6_a4", a4)
        c.load(buf, w)
        assert c.run(thr) == 0
        st = c.stats()
        print("random background, fp6_a4 %d: candidate tiles %d of %d" % (a4, st["candidate_tiles"], st["tiles"]))
        assert st["screened"] == 1 and st["screen_fp6"] == 1 and st["fp6_a4"] == a4, st
        C._bits_equal(c.rows(), ref)
        cand.append(st["candidate_tiles"])
        c.close()
    assert cand[0] == cand[1], cand
