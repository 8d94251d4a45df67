"""The fp6 screen's complement coding (pair_mfma.hip frag6_kernel: A channels
w6 [missing] and w6 [minor], B nibbles 2.0 missing / 1.0 minor / 0 major; the
epilogue restores the direct coding's sums from per-site marginals,
pair_common.hpp f6c_direct) at the smallest shapes that reach every path of
pair_fp6_screen2w_kernel and pair_fp6_screen_kernel.

L = 160 is three tile columns, the last half padding: one pair entry, single
entries, three diagonal tiles and a padded last tile.  N = 130 is two K
stages (126 padded sequences in the second, which read as missing and must
weigh nothing), N = 128 exactly one, N = 1 a single sequence.  Site 50 is
missing in 90% of the sequences, site 90 in none; with `dropped`, three sites
carry one symbol only and the filter drops them.  Weights: Henikoff, unit,
and a set spread over 2^4 so that several e2m3 codes occur.

The restored sums are the direct coding's bit for bit, so every verdict is
the parent build's: beside rows, order and every bit of d, d', r2 against the
oracle, and every tile holding an oracle row being a candidate, the candidate
tile counts must equal the parent build's on the same inputs.  (The scale
rule of fp6_scale.hpp moves R by at most its 1% condition; the counts below
held with it as well, and the random background keeps the limit of
tests/test_gpu_fp6_operands.py, the parent's count plus 2.)
"""
import numpy as np
import pytest

import _oracle as O
from conftest import REPO  # noqa: F401

pytestmark = pytest.mark.gpu

L_SMALL = 160
PLANTED = (
    (3, 40),     # tile (0, 0): diagonal, first half of the pair entry
    (10, 69),    # tile (0, 1): second half of the pair entry
    (20, 135),   # tile (0, 2): single entry, the padded last column
    (70, 100),   # tile (1, 1): diagonal single entry
    (140, 150),  # tile (2, 2): diagonal, padded rows and columns
)
DROPPED = (17, 77, 130)  # one symbol only: no minor, so the filter drops them
MOSTLY_MISSING, NEVER_MISSING = 50, 90
THRESHOLDS = (0.5, 0.05)
SIZES = (130, 128, 1)
WEIGHTS = ("henikoff", "unit", "spread")
# (kernel, options): both fp6 kernels forced, then the automatic choice
MODES = (("pairs", {"screen_fp6": 2}), ("tiles", {"screen_fp6": 2, "fp6_pairs_min_tiles": 1 << 30}), ("auto", {}))

# Candidate tiles of the parent build (commit 90f1150: A channels "in" and
# minor, B minor + 2 major, no marginals) on _small_input's inputs, by
# "N/weights/dropped/mode/threshold", measured once on an MI355X by running
# measure_candidates() below against that build's library; -1 where the pass
# did not screen on fp6 (the automatic choice on lists this small).
PARENT_CANDIDATES = {
    "1/henikoff/0/auto/0.05": 0, "1/henikoff/0/auto/0.5": 0, "1/henikoff/0/pairs/0.05": 0,
    "1/henikoff/0/pairs/0.5": 0, "1/henikoff/0/tiles/0.05": 0, "1/henikoff/0/tiles/0.5": 0,
    "1/henikoff/1/auto/0.05": 0, "1/henikoff/1/auto/0.5": 0, "1/henikoff/1/pairs/0.05": 0,
    "1/henikoff/1/pairs/0.5": 0, "1/henikoff/1/tiles/0.05": 0, "1/henikoff/1/tiles/0.5": 0,
    "1/spread/0/auto/0.05": 0, "1/spread/0/auto/0.5": 0, "1/spread/0/pairs/0.05": 0, "1/spread/0/pairs/0.5": 0,
    "1/spread/0/tiles/0.05": 0, "1/spread/0/tiles/0.5": 0, "1/spread/1/auto/0.05": 0, "1/spread/1/auto/0.5": 0,
    "1/spread/1/pairs/0.05": 0, "1/spread/1/pairs/0.5": 0, "1/spread/1/tiles/0.05": 0, "1/spread/1/tiles/0.5": 0,
    "1/unit/0/auto/0.05": 0, "1/unit/0/auto/0.5": 0, "1/unit/0/pairs/0.05": 0, "1/unit/0/pairs/0.5": 0,
    "1/unit/0/tiles/0.05": 0, "1/unit/0/tiles/0.5": 0, "1/unit/1/auto/0.05": 0, "1/unit/1/auto/0.5": 0,
    "1/unit/1/pairs/0.05": 0, "1/unit/1/pairs/0.5": 0, "1/unit/1/tiles/0.05": 0, "1/unit/1/tiles/0.5": 0,
    "128/henikoff/0/auto/0.05": -1, "128/henikoff/0/auto/0.5": 5, "128/henikoff/0/pairs/0.05": 6,
    "128/henikoff/0/pairs/0.5": 5, "128/henikoff/0/tiles/0.05": 6, "128/henikoff/0/tiles/0.5": 5,
    "128/henikoff/1/auto/0.05": -1, "128/henikoff/1/auto/0.5": 5, "128/henikoff/1/pairs/0.05": 6,
    "128/henikoff/1/pairs/0.5": 5, "128/henikoff/1/tiles/0.05": 6, "128/henikoff/1/tiles/0.5": 5,
    "128/spread/0/auto/0.05": -1, "128/spread/0/auto/0.5": -1, "128/spread/0/pairs/0.05": 6,
    "128/spread/0/pairs/0.5": 6, "128/spread/0/tiles/0.05": 6, "128/spread/0/tiles/0.5": 6,
    "128/spread/1/auto/0.05": -1, "128/spread/1/auto/0.5": -1, "128/spread/1/pairs/0.05": 6,
    "128/spread/1/pairs/0.5": 6, "128/spread/1/tiles/0.05": 6, "128/spread/1/tiles/0.5": 6,
    "128/unit/0/auto/0.05": -1, "128/unit/0/auto/0.5": 5, "128/unit/0/pairs/0.05": 6, "128/unit/0/pairs/0.5": 5,
    "128/unit/0/tiles/0.05": 6, "128/unit/0/tiles/0.5": 5, "128/unit/1/auto/0.05": -1, "128/unit/1/auto/0.5": 5,
    "128/unit/1/pairs/0.05": 6, "128/unit/1/pairs/0.5": 5, "128/unit/1/tiles/0.05": 6, "128/unit/1/tiles/0.5": 5,
    "130/henikoff/0/auto/0.05": -1, "130/henikoff/0/auto/0.5": 5, "130/henikoff/0/pairs/0.05": 6,
    "130/henikoff/0/pairs/0.5": 5, "130/henikoff/0/tiles/0.05": 6, "130/henikoff/0/tiles/0.5": 5,
    "130/henikoff/1/auto/0.05": -1, "130/henikoff/1/auto/0.5": 5, "130/henikoff/1/pairs/0.05": 6,
    "130/henikoff/1/pairs/0.5": 5, "130/henikoff/1/tiles/0.05": 6, "130/henikoff/1/tiles/0.5": 5,
    "130/spread/0/auto/0.05": -1, "130/spread/0/auto/0.5": -1, "130/spread/0/pairs/0.05": 6,
    "130/spread/0/pairs/0.5": 5, "130/spread/0/tiles/0.05": 6, "130/spread/0/tiles/0.5": 5,
    "130/spread/1/auto/0.05": -1, "130/spread/1/auto/0.5": -1, "130/spread/1/pairs/0.05": 6,
    "130/spread/1/pairs/0.5": 5, "130/spread/1/tiles/0.05": 6, "130/spread/1/tiles/0.5": 5,
    "130/unit/0/auto/0.05": -1, "130/unit/0/auto/0.5": 5, "130/unit/0/pairs/0.05": 6, "130/unit/0/pairs/0.5": 5,
    "130/unit/0/tiles/0.05": 6, "130/unit/0/tiles/0.5": 5, "130/unit/1/auto/0.05": -1, "130/unit/1/auto/0.5": 5,
    "130/unit/1/pairs/0.05": 6, "130/unit/1/pairs/0.5": 5, "130/unit/1/tiles/0.05": 6, "130/unit/1/tiles/0.5": 5,
}
# ... and on the 1024 x 2000 random background (tests/test_gpu_fp6_operands.py
# PARENT_CANDIDATES; re-measured with the counts above): 87 of 136.  The
# complement coding alone gave exactly 87, and so did the scale rule on top.
PARENT_BACKGROUND = 87


@pytest.fixture(scope="module")
def W():
    import weightedld_amd as W
    return W


def _bits_equal(store, ref):
    assert len(store) == len(ref["site_a"]), (len(store), len(ref["site_a"]))
    assert np.array_equal(store.site_a.astype(np.uint64), ref["site_a"].astype(np.uint64))
    assert np.array_equal(store.site_b.astype(np.uint64), ref["site_b"].astype(np.uint64))
    for f in ("d", "d_prime", "r2"):
        x, y = getattr(store, f), np.asarray(ref[f], dtype=np.float32)
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f


def _small_input(N, dropped):
    import bench
    buf = bench.synth(L_SMALL, N, seed=0xC6 + N)
    rng = np.random.default_rng(23 + N)
    for a, b in PLANTED:
        row = buf[a].copy()
        flip = rng.random(N) < 0.04  # a little noise: r2 high, not 1
        row[flip] = buf[b][flip]
        buf[b] = row
    if N > 1:
        buf[MOSTLY_MISSING, rng.random(N) < 0.9] = 4
        gone = buf[NEVER_MISSING] == 4
        buf[NEVER_MISSING, gone] = buf[NEVER_MISSING][~gone][0]
    if dropped:
        for i, s in enumerate(DROPPED):
            buf[s] = i
    return buf


def _weights(W, buf, kind):
    N = buf.shape[1]
    if kind == "henikoff":
        return W.henikoff_weights(W.SiteSet.from_buffer(buf))
    if kind == "unit":
        return np.ones(N, dtype=np.float32)
    return np.exp2(-4.0 * np.random.default_rng(5 + N).random(N)).astype(np.float32)


_cache = {}


def _small_case(W, N, weights, dropped):
    """(buf, w, {thr: oracle rows}), computed once per input."""
    key = (N, weights, dropped)
    if key not in _cache:
        buf = _small_input(N, dropped)
        w = _weights(W, buf, weights)
        _cache[key] = (buf, w, {thr: O.all_pairs(buf, w, np.float32(thr)) for thr in THRESHOLDS})
    return _cache[key]


def _row_tiles(ref):
    return set(zip((ref["site_a"] // 64).tolist(), (ref["site_b"] // 64).tolist()))


def _run_modes(W, buf, w, refs, check):
    """{mode/thr: candidate tiles, -1 where the pass did not screen on fp6}"""
    out = {}
    for mode, opts in MODES:
        c = W.Context(0)
        for k, v in opts.items():
            c.set_option(k, v)
        c.load(buf, w)
        for thr in THRESHOLDS:
            n = c.run(thr)
            st = c.stats()
            fp6 = st["screened"] == 1 and st["screen_fp6"] == 1
            out["%s/%g" % (mode, thr)] = st["candidate_tiles"] if fp6 else -1
            if check:
                ref = refs[thr]
                if opts:
                    assert fp6, st
                assert n == len(ref["site_a"])
                _bits_equal(c.rows(), ref)
                if st["screened"] == 1:
                    assert st["candidate_tiles"] >= len(_row_tiles(ref)), (st, sorted(_row_tiles(ref)))
        c.close()
    return out


def measure_candidates(W):
    """Every small case's candidate counts, as PARENT_CANDIDATES holds them."""
    out = {}
    for N in SIZES:
        for weights in WEIGHTS:
            for dropped in (False, True):
                buf, w, refs = _small_case(W, N, weights, dropped)
                for k, v in _run_modes(W, buf, w, refs, check=False).items():
                    out["%d/%s/%d/%s" % (N, weights, int(dropped), k)] = v
    return out


@pytest.mark.parametrize("dropped", [False, True])
@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("N", SIZES)
def test_fp6_complement_small_shapes(W, N, weights, dropped):
    buf, w, refs = _small_case(W, N, weights, dropped)
    if N > 1 and weights != "spread":
        # the planted rows are there at the high threshold
        pairs = set(zip(refs[0.5]["site_a"].tolist(), refs[0.5]["site_b"].tolist()))
        assert set(PLANTED) <= pairs
    got = _run_modes(W, buf, w, refs, check=True)
    for k, v in sorted(got.items()):
        key = "%d/%s/%d/%s" % (N, weights, int(dropped), k)
        print("candidate tiles %s: %d (parent %d)" % (key, v, PARENT_CANDIDATES[key]))
    for k, v in got.items():
        key = "%d/%s/%d/%s" % (N, weights, int(dropped), k)
        assert v == PARENT_CANDIDATES[key], (key, v, PARENT_CANDIDATES[key])


def test_fp6_complement_random_background(W):
    """Random background alone (L 1024, N 2000, thr 0.05): no oracle row, and
    no more candidate tiles than the parent build's count plus 2 (the scale
    rule may move R within its 1% condition; the coding alone moves nothing)."""
    import bench
    L, N, thr = 1024, 2000, 0.05
    buf = bench.synth(L, N)
    w = W.henikoff_weights(W.SiteSet.from_buffer(buf))
    ref = O.all_pairs(buf, w, np.float32(thr))
    assert len(ref["site_a"]) == 0
    for forced in (True, False):
        c = W.Context(0)
        if forced:
            c.set_option("screen_fp6", 2)
        c.load(buf, w)
        assert c.run(thr) == 0
        st = c.stats()
        print("random background, %s: candidate tiles %d of %d (parent %d), screen_fp6 %d"
              % ("forced" if forced else "auto", st["candidate_tiles"], st["tiles"], PARENT_BACKGROUND,
                 st["screen_fp6"]))
        if forced:
            assert st["screened"] == 1 and st["screen_fp6"] == 1, st
        if st["screen_fp6"] == 1:
            assert st["candidate_tiles"] <= PARENT_BACKGROUND + 2, st
        _bits_equal(c.rows(), ref)
        c.close()
