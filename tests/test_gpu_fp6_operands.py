"""The fp6 screen's operand images (pair_mfma.hip frag6_kernel: A channels
"in" and minor, B fp4 codes) and its stage loop, at the smallest shapes that
reach every path of pair_fp6_screen2w_kernel and pair_fp6_screen_kernel.

L = 160 is three tile columns, the last half padding: tile row 0 is one pair
entry (tiles (0, 0) and (0, 1)) plus one single entry ((0, 2)), rows 1 and 2
are single entries, and (0, 0), (1, 1), (2, 2) are diagonal tiles.  N = 130
is two K stages, the second holding two real sequences; N = 128 exactly one
(the stage that takes a constant-zero C, and no other); N = 1 a single
sequence.  A screen only decides which tiles the candidate launch computes:
rows, their order and every bit of d, d', r2 must equal the oracle's
(lib.rs:482-520, :660, :623-683), and every tile that holds an oracle row
must have been a candidate.
"""
import numpy as np
import pytest

import _oracle as O
from conftest import REPO  # noqa: F401

pytestmark = pytest.mark.gpu

L_SMALL = 160
# planted (a, b): b's row a noisy copy of a's, one pair in each of
PLANTED = (
    (3, 40),     # tile (0, 0): diagonal, first half of the pair entry
    (10, 69),    # tile (0, 1): second half of the pair entry
    (20, 135),   # tile (0, 2): single entry, the padded last column
    (70, 100),   # tile (1, 1): diagonal single entry
    (140, 150),  # tile (2, 2): diagonal, padded rows and columns
)
PLANTED_TILES = {(0, 0), (0, 1), (0, 2), (1, 1), (2, 2)}
DROPPED = (17, 77, 130)  # one symbol only: no minor, so the filter drops them (site_ok 0)


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
    buf = bench.synth(L_SMALL, N, seed=0xF6 + N)
    rng = np.random.default_rng(11 + N)
    for a, b in PLANTED:
        row = buf[a].copy()
        flip = rng.random(N) < 0.04  # a little noise: r2 high, not 1
        row[flip] = buf[b][flip]
        buf[b] = row
    if dropped:
        for i, s in enumerate(DROPPED):
            buf[s] = i
    return buf


_cache = {}


def _small_case(W, N, weights, dropped):
    """(buf, w, {thr: oracle rows}), computed once per input."""
    key = (N, weights, dropped)
    if key not in _cache:
        buf = _small_input(N, dropped)
        if weights == "henikoff":
            w = W.henikoff_weights(W.SiteSet.from_buffer(buf))
        else:
            w = np.ones(N, dtype=np.float32)
        refs = {thr: O.all_pairs(buf, w, np.float32(thr)) for thr in (0.5, 0.05)}
        _cache[key] = (buf, w, refs)
    return _cache[key]


def _row_tiles(ref):
    return set(zip((ref["site_a"] // 64).tolist(), (ref["site_b"] // 64).tolist()))


def _check(W, buf, w, refs, forced, pairs_min=None):
    c = W.Context(0)
    if forced:
        c.set_option("screen_fp6", 2)
    if pairs_min is not None:
        c.set_option("fp6_pairs_min_tiles", pairs_min)
    c.load(buf, w)
    for thr, ref in refs.items():
        n = c.run(thr)
        st = c.stats()
        if forced:
            assert st["screen_fp6"] == 1, st
        assert n == len(ref["site_a"])
        _bits_equal(c.rows(), ref)
        if st["screened"] == 1:
            assert st["candidate_tiles"] >= len(_row_tiles(ref)), (st, sorted(_row_tiles(ref)))
    c.close()


@pytest.mark.parametrize("dropped", [False, True])
@pytest.mark.parametrize("weights", ["henikoff", "unit"])
@pytest.mark.parametrize("N", [130, 128, 1])
def test_fp6_operands_small_shapes(W, N, weights, dropped):
    """The tile-pair kernel forced, then auto.  dropped: three sites the
    filter drops, in three tiles, so the general (not all-valid) epilogue
    runs beside the diagonal and padded tiles'."""
    buf, w, refs = _small_case(W, N, weights, dropped)
    if N > 1:
        # the planted rows are there at the high threshold, in all five tiles
        assert PLANTED_TILES <= _row_tiles(refs[0.5]), sorted(_row_tiles(refs[0.5]))
        pairs = set(zip(refs[0.5]["site_a"].tolist(), refs[0.5]["site_b"].tolist()))
        assert set(PLANTED) <= pairs
    _check(W, buf, w, refs, forced=True)
    _check(W, buf, w, refs, forced=False)


@pytest.mark.parametrize("N", [130, 128])
def test_fp6_operands_single_tile_kernel(W, N):
    """The same image through pair_fp6_screen_kernel (fp6_pairs_min_tiles above
    the tile count)."""
    buf, w, refs = _small_case(W, N, "henikoff", True)
    _check(W, buf, w, refs, forced=True, pairs_min=1 << 30)


# Candidate tiles of the parent build (A channels "in" and major) on the input
# below, measured before the A image changed: 87 of 136, forced and auto (at
# 1,024 sites the Henikoff weights spread more than at C4's 20,000, so the fp6
# rounding keeps many tiles; profiles/r07a/candidates_1024x2000.jsonl).
PARENT_CANDIDATES = 87


def test_fp6_operands_random_background_rejects(W):
    """Random background alone (L 1024, N 2000, thr 0.05): no oracle row, and
    the screen still rejects: no more candidate tiles than the parent build's
    count plus 2 (0 if the parent's was 0)."""
    import bench
    L, N, thr = 1024, 2000, 0.05
    buf = bench.synth(L, N)
    w = W.henikoff_weights(W.SiteSet.from_buffer(buf))
    ref = O.all_pairs(buf, w, np.float32(thr))
    assert len(ref["site_a"]) == 0
    limit = PARENT_CANDIDATES + 2 if PARENT_CANDIDATES else 0
    for forced in (True, False):
        c = W.Context(0)
        if forced:
            c.set_option("screen_fp6", 2)
        c.load(buf, w)
        assert c.run(thr) == 0
        st = c.stats()
        print("random background, %s: candidate tiles %d of %d (parent %d), screen_fp6 %d"
              % ("forced" if forced else "auto", st["candidate_tiles"], st["tiles"], PARENT_CANDIDATES,
                 st["screen_fp6"]))
        if forced:
            assert st["screened"] == 1 and st["screen_fp6"] == 1, st
        if st["screen_fp6"] == 1:
            assert st["candidate_tiles"] <= limit, (st, limit)
        _bits_equal(c.rows(), ref)
        c.close()
