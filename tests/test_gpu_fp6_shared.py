"""The fp6 screen's shared code image (WLD_OPT_FP6_SHARED, "fp6_shared"): where
every rounded weight of a load is the same code (fp6_scale.hpp fp6_shared_code:
unit weights here) no A image is built, and pair_fp6_screen2w_kernel<kF6Shared>,
pair_fp6_screen_kernel<kF6Shared> and the sample run read the row tile from the
B code image, mask it into the two A channels and scale the restored sums by
the one weight value (pair_common.hpp f6s_direct).  The scaled sums are the
parent coding's bit for bit, so beside rows, order and every bit of d, d', r2
against the oracle, the candidate tiles and sub-blocks must be equal between
"fp6_shared" 0 and 1, on both kernels ("fp6_pairs_min_tiles" 0 and 2^30).

Shapes: L 64 (one diagonal tile), 65 (a single entry whose second tile is all
padding but one site), 130 (a pair entry and a padded last tile), 200 (an odd
tile row: pair and single entries); N 1, 100 (28 padded sequences inside one
128-block, which the shared image must code 0), 128 (none), 129 (127 padded in
a second block), 200 (56 padded).  The background misses 10% of the symbols;
one shape misses 60%, so that the missing channel's products dominate.
Correlated pairs are planted in every tile kind, so the passes have rows.
Henikoff weights of a small alignment have several codes: the mode stays off
and the parent's kernels run.
"""
import numpy as np
import pytest

import _oracle as O
import test_gpu_fp6_complement as C

pytestmark = pytest.mark.gpu

LS = (64, 65, 130, 200)
NS = (1, 100, 128, 129, 200)
THRESHOLDS = (0.05, 0.3)
# (a, b) kept where b < L: diagonal tiles, the pair entry's halves, single entries, padded last tiles
PLANTED = ((3, 40), (10, 64), (20, 129), (70, 100), (60, 199), (140, 150), (130, 195))
KERNELS = (("pairs", 0), ("tiles", 1 << 30))


@pytest.fixture(scope="module")
def W():
    import weightedld_amd as W
    return W


def _input(L, N, p_missing=0.1):
    import bench
    buf = bench.synth(L, N, seed=0x5A + 7 * L + N)
    rng = np.random.default_rng(31 * L + N)
    if p_missing > 0.1:  # synth misses 0.1: the rest on top
        buf[rng.random(buf.shape) < (p_missing - 0.1) / 0.9] = 4
    for a, b in PLANTED:
        if b >= L:
            continue
        row = buf[a].copy()
        flip = rng.random(N) < 0.04  # a little noise: r2 high, not 1
        row[flip] = buf[b][flip]
        buf[b] = row
    return buf


_cache = {}


def _case(L, N, p_missing=0.1, weights="unit", W=None):
    """(buf, w, {thr: oracle rows}), computed once per input."""
    key = (L, N, p_missing, weights)
    if key not in _cache:
        buf = _input(L, N, p_missing)
        w = np.ones(N, dtype=np.float32) if weights == "unit" else W.henikoff_weights(W.SiteSet.from_buffer(buf))
        _cache[key] = (buf, w, {thr: O.all_pairs(buf, w, np.float32(thr)) for thr in THRESHOLDS})
    return _cache[key]


def _run(W, buf, w, refs, min_tiles, shared, want_shared):
    """{thr: (candidate tiles, candidate sub-blocks)} of the forced fp6 screen, rows checked against the oracle."""
    c = W.Context(0)
    c.set_option("screen_fp6", 2)
    c.set_option("fp6_pairs_min_tiles", min_tiles)
    c.set_option("fp6_shared", shared)
    assert c.get_option("fp6_shared") == shared
    c.load(buf, w)
    out = {}
    for thr in THRESHOLDS:
        n = c.run(thr)
        st = c.stats()
        assert st["screened"] == 1 and st["screen_fp6"] == 1, st
        assert st["fp6_shared"] == want_shared, (st, shared)
        assert n == len(refs[thr]["site_a"]), (n, len(refs[thr]["site_a"]))
        C._bits_equal(c.rows(), refs[thr])
        assert st["candidate_tiles"] >= len(C._row_tiles(refs[thr])), (st, sorted(C._row_tiles(refs[thr])))
        out[thr] = (st["candidate_tiles"], st["candidate_blocks"])
    c.close()
    return out


def _both_modes(W, buf, w, refs, qualifies, label):
    for kernel, min_tiles in KERNELS:
        got = {s: _run(W, buf, w, refs, min_tiles, s, 1 if s and qualifies else 0) for s in (0, 1)}
        for thr in THRESHOLDS:
            print("%s %s thr %g: rows %d, candidate tiles / sub-blocks: option 0 %r, option 1 %r"
                  % (label, kernel, thr, len(refs[thr]["site_a"]), got[0][thr], got[1][thr]))
        for thr in THRESHOLDS:
            assert got[0][thr] == got[1][thr], (label, kernel, thr, got[0][thr], got[1][thr])


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("L", LS)
def test_fp6_shared_small_shapes(W, L, N):
    buf, w, refs = _case(L, N)
    if N >= 100:
        # the planted rows are there at the high threshold
        pairs = set(zip(refs[0.3]["site_a"].tolist(), refs[0.3]["site_b"].tolist()))
        assert {p for p in PLANTED if p[1] < L} <= pairs
    _both_modes(W, buf, w, refs, True, "L %d N %d" % (L, N))


def test_fp6_shared_mostly_missing(W):
    """60% of the symbols missing: the missing channel (the 0x4 mask) carries most products."""
    L, N = 130, 200
    buf, w, refs = _case(L, N, p_missing=0.6)
    assert abs(float(np.mean(buf == 4)) - 0.6) < 0.03
    assert len(refs[0.05]["site_a"]) > 0
    _both_modes(W, buf, w, refs, True, "L %d N %d, 60%% missing" % (L, N))


def test_fp6_shared_henikoff_stays_off(W):
    """Henikoff weights of a small alignment round to several codes: no shared image, the same rows."""
    L, N = 130, 100
    buf, w, refs = _case(L, N, weights="henikoff", W=W)
    c = W.Context(0)
    c.set_option("screen_fp6", 2)
    c.load(buf, w)
    codes = c.fp6_weight_codes(N)[0]
    c.close()
    assert len(set(codes.tolist())) > 1, sorted(set(codes.tolist()))
    _both_modes(W, buf, w, refs, False, "L %d N %d Henikoff" % (L, N))


def test_fp6_shared_reload(W):
    """One context through a shared load, a several-code load and a shared load again, then the option off and on."""
    L, N = 130, 129
    c = W.Context(0)
    c.set_option("screen_fp6", 2)
    for weights, want in (("unit", 1), ("henikoff", 0), ("unit", 1)):
        buf, w, refs = _case(L, N, weights=weights, W=W)
        c.load(buf, w)
        for thr in THRESHOLDS:
            assert c.run(thr) == len(refs[thr]["site_a"])
            assert c.stats()["fp6_shared"] == want, c.stats()
            C._bits_equal(c.rows(), refs[thr])
    for shared in (0, 1):
        c.set_option("fp6_shared", shared)
        assert c.run(THRESHOLDS[0]) == len(refs[THRESHOLDS[0]]["site_a"])
        assert c.stats()["fp6_shared"] == shared, c.stats()
        C._bits_equal(c.rows(), refs[THRESHOLDS[0]])
    c.close()


def test_fp6_shared_random_background(W):
    """Random background alone (L 1024, N 2000, unit weights, thr 0.05): no
    row, and the same candidate tiles and sub-blocks with and without the
    shared image."""
    import bench
    L, N, thr = 1024, 2000, 0.05
    buf = bench.synth(L, N)
    w = np.ones(N, dtype=np.float32)
    ref = O.all_pairs(buf, w, np.float32(thr))
    assert len(ref["site_a"]) == 0
    cand = []
    for shared in (0, 1):
        c = W.Context(0)
        c.set_option("screen_fp6", 2)
        c.set_option("fp6_shared", shared)
        c.load(buf, w)
        assert c.run(thr) == 0
        st = c.stats()
        print("random background, fp6_shared %d: candidate tiles %d of %d, sub-blocks %d"
              % (shared, st["candidate_tiles"], st["tiles"], st["candidate_blocks"]))
        assert st["screened"] == 1 and st["screen_fp6"] == 1 and st["fp6_shared"] == shared, st
        C._bits_equal(c.rows(), ref)
        cand.append((st["candidate_tiles"], st["candidate_blocks"]))
        c.close()
    assert cand[0] == cand[1], cand
