"""The tile-pair fp6 screen on three masked sums (WLD_OPT_FP6_THREE,
"fp6_three"): pair_fp6_screen2w_kernel<., true> leaves the missing-by-missing
sum out of its stage loop, decides every pair it can on the interval the other
three leave for it (pair_common.hpp r2_screen_terms_xy2_t) and runs the loop a
second time, for that sum alone, for the entries with a pair in doubt.  A pair
the three sums reject is rejected on four, and the second pass completes the
very sums of the four-sum kernel, so for every case here option 0 (four sums)
and option 2 (three sums wherever the tile-pair screen runs) must give the
oracle's rows bit for bit and equal candidate tiles and sub-blocks, with
wld_run_stats.fp6_three 0 and 1.

The planted case (1,024 sites x 2,000 sequences, unit weights: the headline's
shared image) holds ten pairs with r2 from 1 down to just under 0.05 in nine
of its 72 entries: first halves, second halves, both halves of one entry, a
single entry and diagonal tiles.  At 0.05 the planted entries take the second
pass and the background's do not (0 < fp6_rechecked < entries, one launch on
both paths); at 0.005 the background's noise (r2 ~ 1 / 1,600 per pair, 4,096
pairs per tile) puts every entry in doubt; at 0.5 only planted entries can be
in doubt (a pair that passes makes its tile a candidate, and a candidate needs
the fourth sum: the entries that hold a row are rechecked at any threshold),
and on the background alone none is.
"""
import numpy as np
import pytest

import _oracle as O
import test_gpu_fp6_complement as C

pytestmark = pytest.mark.gpu

# (a, b, share of b's column re-drawn): r2 about (1 - share)^2
PLANTED = (
    (5, 70, 0.0),       # entry (0, 0-1), second half
    (130, 300, 0.03),   # entry (2, 4-5), first half
    (200, 710, 0.1),    # entry (3, 10-11), second half
    (260, 270, 0.2),    # entry (4, 4-5), first half: a diagonal tile
    (330, 1000, 0.35),  # entry (5, 14-15), second half
    (400, 401, 0.5),    # entry (6, 6-7), first half: a diagonal tile
    (450, 460, 0.6),    # tile (7, 7): a single entry on the diagonal
    (520, 900, 0.7),    # entry (8, 14-15), first half ...
    (530, 980, 0.76),   # ... and its second half
    (600, 660, 0.8),    # entry (9, 10-11), first half: just under 0.05
)


@pytest.fixture(scope="module")
def W():
    import weightedld_amd as W
    return W


def n_entries(L):
    """Entries of the fp6 screen's pair list over every tile (tile_order.hpp fp6_pair_list)."""
    T, n = (L + 63) // 64, 0
    for ta in range(T):
        tb = ta
        while tb < T:
            step = 2 if tb % 2 == 0 and tb + 1 < T else 1
            n, tb = n + 1, tb + step
    return n


def entry_of(a, b):
    return (a // 64, b // 64 // 2)


def _weights(kind, N):
    rng = np.random.default_rng(77 + N)
    if kind == "unit":  # one code: the shared image
        return np.ones(N, dtype=np.float32)
    if kind == "two":  # two e2m1 codes: the fp4 A image
        return np.where(rng.random(N) < 0.5, 1.0, 0.5).astype(np.float32)
    return np.exp2(-4.0 * rng.random(N)).astype(np.float32)  # several e2m3 codes: the fp6 A image


FORMAT = {"unit": (1, None), "two": (0, 1), "spread": (0, 0)}  # kind: (fp6_shared, fp6_a4)


def _plant(buf, pairs, seed):
    rng = np.random.default_rng(seed)
    N = buf.shape[1]
    for a, b, share in pairs:
        row = buf[a].copy()
        redo = rng.random(N) < share
        row[redo] = rng.permutation(buf[a])[redo]
        buf[b] = row
    return buf


_cache = {}


def _planted_case():
    if "planted" not in _cache:
        import bench
        L, N = 1024, 2000
        buf = _plant(bench.synth(L, N), PLANTED, 0x3A)
        w = _weights("unit", N)
        _cache["planted"] = (buf, w, {thr: O.all_pairs(buf, w, np.float32(thr)) for thr in (0.05, 0.005, 0.5)})
    return _cache["planted"]


def _run(W, buf, w, refs, three, kind=None, opts=(("screen_fp6", 2),)):
    """{thr: stats} of the pass with "fp6_three" = three, rows checked against the oracle."""
    c = W.Context(0)
    for k, v in opts:
        c.set_option(k, v)
    c.set_option("fp6_three", three)
    assert c.get_option("fp6_three") == three
    c.load(buf, w)
    out = {}
    for thr, ref in refs.items():
        n = c.run(thr)
        st = c.stats()
        assert n == len(ref["site_a"]), (thr, n, len(ref["site_a"]))
        C._bits_equal(c.rows(), ref)
        if kind is not None:
            shared, a4 = FORMAT[kind]
            assert st["fp6_shared"] == shared and (a4 is None or st["fp6_a4"] == a4), (kind, st)
        out[thr] = st
    c.close()
    return out


def _same_verdicts(label, four, three):
    for thr in four:
        a, b = four[thr], three[thr]
        print("%s thr %g: rows %d, candidate tiles / sub-blocks %d / %d (four sums), %d / %d (three), rechecked %d"
              % (label, thr, b["rows"], a["candidate_tiles"], a["candidate_blocks"], b["candidate_tiles"],
                 b["candidate_blocks"], b["fp6_rechecked"]))
        assert a["screened"] == 1 and a["screen_fp6"] == 1 and b["screened"] == 1 and b["screen_fp6"] == 1, (a, b)
        assert a["fp6_three"] == 0 and a["fp6_rechecked"] == 0, a
        assert b["fp6_three"] == 1, b
        assert (a["candidate_tiles"], a["candidate_blocks"]) == (b["candidate_tiles"], b["candidate_blocks"]), (a, b)


@pytest.fixture(scope="module")
def planted_runs(W):
    buf, w, refs = _planted_case()
    four, three = _run(W, buf, w, refs, 0, "unit"), _run(W, buf, w, refs, 2, "unit")
    _same_verdicts("planted", four, three)
    return refs, three


def _row_entries(ref):
    return {entry_of(a, b) for a, b in zip(ref["site_a"].tolist(), ref["site_b"].tolist())}


def test_three_planted_both_paths(planted_runs):
    """thr 0.05: the planted entries are rechecked, the background's are not."""
    refs, three = planted_runs
    rows = set(zip(refs[0.05]["site_a"].tolist(), refs[0.05]["site_b"].tolist()))
    assert {(a, b) for a, b, share in PLANTED if share <= 0.6} <= rows, sorted(rows)
    st = three[0.05]
    assert len(_row_entries(refs[0.05])) <= st["fp6_rechecked"] < n_entries(1024), (st, n_entries(1024))
    assert st["fp6_rechecked"] > 0


def test_three_planted_every_entry(planted_runs):
    """thr 0.005: every entry is rechecked."""
    refs, three = planted_runs
    assert three[0.005]["fp6_rechecked"] == n_entries(1024) == 72, three[0.005]


def test_three_planted_high_threshold(planted_runs, W):
    """thr 0.5: the entries that hold a row are rechecked, no entry without a
    planted pair is; on the background alone, none at all."""
    refs, three = planted_runs
    planted = {entry_of(a, b) for a, b, share in PLANTED}
    assert len(_row_entries(refs[0.5])) <= three[0.5]["fp6_rechecked"] <= len(planted), (three[0.5], sorted(planted))
    import bench
    buf = bench.synth(1024, 2000)
    w = _weights("unit", 2000)
    ref = {0.5: O.all_pairs(buf, w, np.float32(0.5))}
    assert len(ref[0.5]["site_a"]) == 0
    four, bg = _run(W, buf, w, ref, 0, "unit"), _run(W, buf, w, ref, 2, "unit")
    _same_verdicts("background", four, bg)
    assert bg[0.5]["fp6_rechecked"] == 0 and bg[0.5]["candidate_tiles"] == 0, bg[0.5]


# pairs planted in every kind of tile of the small shapes, kept where b < L
SMALL_PLANTED = ((3, 40, 0.04), (10, 64, 0.3), (20, 129, 0.04), (70, 100, 0.5), (60, 191, 0.04), (140, 150, 0.7),
                 (130, 195, 0.04))
DROPPED = (17, 77, 131)  # one symbol only: the filter drops them (row and column tiles keep a hole)
# N 100: one stage (the peeled one alone); N 130: two, the second mostly padding;
# L 192: three tiles (pair and single entries, the diagonal); L 200: a padded last tile
SHAPES = ((130, 100, False), (130, 130, False), (192, 200, False), (200, 130, False), (200, 200, True))


@pytest.mark.parametrize("kind", sorted(FORMAT))
@pytest.mark.parametrize("L,N,dropped", SHAPES)
def test_three_small_shapes(W, L, N, dropped, kind):
    import bench
    buf = _plant(bench.synth(L, N, seed=0x73 + 5 * L + N), [p for p in SMALL_PLANTED if p[1] < L], L + N)
    if dropped:
        for i, s in enumerate(DROPPED):
            buf[s] = i
    w = _weights(kind, N)
    refs = {thr: O.all_pairs(buf, w, np.float32(thr)) for thr in (0.05, 0.5)}
    assert len(refs[0.5]["site_a"]) > 0
    four, three = _run(W, buf, w, refs, 0, kind), _run(W, buf, w, refs, 2, kind)
    _same_verdicts("L %d N %d %s%s" % (L, N, kind, " dropped" if dropped else ""), four, three)
    for thr in refs:
        assert three[thr]["fp6_rechecked"] >= len(_row_entries(refs[thr])) > 0, (thr, three[thr])


def test_three_single_tile_kernel_keeps_four(W):
    """One tile per workgroup (no pair list): four sums whatever the option."""
    buf, w, refs = _planted_case()
    st = _run(W, buf, w, {0.05: refs[0.05]}, 2, "unit", opts=(("screen_fp6", 2), ("fp6_pairs_min_tiles", 1 << 30)))
    assert st[0.05]["screen_fp6"] == 1 and st[0.05]["fp6_three"] == 0 and st[0.05]["fp6_rechecked"] == 0, st


def test_three_auto(W):
    """Auto (the default): 2,080 tiles, so the sample run decides.  Random
    background with unit weights at 0.3 (N = 256: a pair's r2 is ~ 1 / 200, no
    pair near 0.3, nothing in doubt): three sums.  Linkage blocks at 0.05: the
    sample sends the pass to the i8 screen, no fp6 pass at all.  A list
    without a sample (WLD_OPT_SCREEN_FP6 3) stays on four sums."""
    import bench
    L, N = 4096, 256
    assert (L // 64) * (L // 64 + 1) // 2 == 2080
    w = _weights("unit", N)
    buf = bench.synth(L, N)
    ref = {0.3: O.all_pairs(buf, w, np.float32(0.3))}
    st = _run(W, buf, w, ref, 1, opts=())[0.3]
    print("auto, background:", st)
    assert st["screen_fp6"] == 1 and st["fp6_sampled"] == 1 and st["fp6_three"] == 1 and st["fp6_rechecked"] == 0, st
    st0 = _run(W, buf, w, ref, 0, opts=())[0.3]
    assert st0["screen_fp6"] == 1 and st0["fp6_three"] == 0, st0
    assert (st0["candidate_tiles"], st0["candidate_blocks"]) == (st["candidate_tiles"], st["candidate_blocks"])
    st3 = _run(W, buf, w, ref, 1, opts=(("screen_fp6", 3),))[0.3]
    assert st3["screen_fp6"] == 1 and st3["fp6_sampled"] == 0 and st3["fp6_three"] == 0, st3
    buf = bench.ld_blocks(L, N)
    ref = {0.05: O.all_pairs(buf, w, np.float32(0.05))}
    st = _run(W, buf, w, ref, 1, opts=())[0.05]
    print("auto, linkage blocks:", st)
    assert st["fp6_three"] == 0 and st["fp6_rechecked"] == 0, st
