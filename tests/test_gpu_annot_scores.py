"""Partitioned LD scores (wld_run_annot_scores / Context.run_annot_scores /
ld_annot_scores / the CLI's --annot-input, --annot-score-output, --annot-self):
    score[i][c] = sum over site i's counted pairs {i, k} of r2(i, k) annot[k][c]
reduced on the device, with no rows.

Expected values: the CPU oracle's dense f32 r2 and `valid` per pair
(O.all_pairs_dense), reduced here in numpy.  The class counts and partners
must be equal.  Each score is compared with math.fsum of its terms — every
term (double) r2 * (double) annot is an exact f64 product of two 24-bit
significands — under the header's bound for an any-order chain of f64 adds
over signed terms:
    |got - ref| <= n 2^-52 sum |term|,   n = partners (+ 1 with the self term).
One r2 off by an f32 ulp moves a score by ~2^-24 of a term — orders of
magnitude past that — so the bound also pins every pair's r2 to the oracle's
bits, and a product that lands in the wrong row or column misses it by whole
terms (the annotations are mixed-sign random values, asymmetric in both
indices).
"""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import CLI, FIXTURES
from test_gpu_summary import Case, case1, case1_map, chunk_linear, shape_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def W():
    import weightedld_amd as W
    return W


def annot_random(L, C, seed):
    """Mixed-sign f32 values with a few exact zeros."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((L, C)).astype(np.float32)
    a[rng.random((L, C)) < 0.1] = 0.0
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def annot_sparse600():
    """600 sites x 40 columns (three 16-column chunks over ten 64-site tiles):
    columns 0..9 one-hot over cells of 60 sites; columns 16..31 zero for the
    sites below 320 (whole 64 x 16 zero blocks: tiles 0..4) and random above;
    columns 32..39 zero but for one value (nine all-zero blocks)."""
    a = np.zeros((600, 40), dtype=np.float32)
    a[np.arange(600), np.arange(600) // 60] = 1.0
    a[320:, 16:32] = annot_random(280, 16, 0xA5)
    a[437, 35] = -2.5
    a.setflags(write=False)
    return a


def pair_mask(L, pos=None, D=0, K=0, chunks=None):
    """[L, L] bool, upper triangle: the pairs of the window and chunk range."""
    a, b = np.triu_indices(L, 1)
    p = np.arange(L, dtype=np.int64) if pos is None else np.asarray(pos, dtype=np.int64)
    keep = np.ones(a.size, dtype=bool)
    if D:
        keep &= p[b] - p[a] <= D
    if K:
        keep &= b - a <= K
    if chunks is not None:
        lin = chunk_linear((L + 255) // 256, a // 256, b // 256)
        keep &= (lin >= chunks[0]) & (lin < chunks[1])
    m = np.zeros((L, L), dtype=bool)
    m[a[keep], b[keep]] = True
    return m


_expected = {}


def expected(case, annot, pos=None, D=0, K=0, chunks=None, self_term=False):
    """The oracle's pairs of the range and window, reduced (once per set of
    arguments): the class counts, partners, and per (site, column) the fsum
    of the exact terms (ref), the sum of their absolute values (mag, rounded
    down: the bound is never wider than stated) and the term count (n)."""
    key = (id(case), annot.shape, annot.tobytes(), None if pos is None else pos.tobytes(), D, K, chunks, self_term)
    if key not in _expected:
        _expected[key] = _reduce(case, annot, pos, D, K, chunks, self_term)
    return _expected[key]


def _reduce(case, annot, pos, D, K, chunks, self_term):
    L = case.L
    m = pair_mask(L, pos, D, K, chunks)
    fin = np.isfinite(case.r2)
    cnt = m & case.valid & fin
    X = np.where(cnt, case.r2, np.float32(0)).astype(np.float64)
    X = X + X.T  # site i's terms: row i
    partners = cnt.sum(axis=1) + cnt.sum(axis=0)
    e = {"pairs": int(m.sum()), "none_pairs": int((m & ~case.valid).sum()),
         "nonfinite_pairs": int((m & case.valid & ~fin).sum()), "counted_pairs": int(cnt.sum()),
         "partners": partners}
    A = np.asarray(annot, dtype=np.float64)
    n = partners.astype(np.int64).copy()
    own = np.zeros(L, dtype=bool)
    if self_term:
        # (valid[a, b] = both sites have a major and a minor symbol)
        ok = (case.valid | case.valid.T).any(axis=1)
        lo, hi = chunks if chunks is not None else (0, 1 << 62)
        rows = np.arange(L) // 256
        diag = chunk_linear((L + 255) // 256, rows, rows)
        own = ok & (diag >= lo) & (diag < hi)
        n += own
    ref = np.zeros(A.shape)
    mag = np.zeros(A.shape)
    for c in range(A.shape[1]):
        nz = np.flatnonzero(A[:, c])  # (a zero annotation's terms are exact zeros)
        P = X[:, nz] * A[nz, c][None, :]  # exact: 24-bit x 24-bit significands
        for i, row in enumerate(P.tolist()):
            if own[i]:
                row.append(float(A[i, c]))
            ref[i, c] = math.fsum(row)
        mag[:, c] = (np.abs(P).sum(axis=1) + np.where(own, np.abs(A[:, c]), 0.0)) * (1 - 2.0 ** -40)
    e.update(ref=ref, mag=mag, n=n)
    return e


def assert_counts(s, e, what=""):
    for f in ("pairs", "none_pairs", "nonfinite_pairs", "counted_pairs"):
        assert getattr(s, f) == e[f], (what, f, getattr(s, f), e[f])
    assert s.pairs == s.none_pairs + s.nonfinite_pairs + s.counted_pairs
    assert np.array_equal(s.partners.astype(np.int64), e["partners"]), what
    assert int(s.partners.sum(dtype=np.uint64)) == 2 * s.counted_pairs


def assert_scores(score, e, what="", slack=1):
    assert score.shape == e["ref"].shape and score.dtype == np.float64
    bound = slack * e["n"][:, None] * 2.0 ** -52 * e["mag"]
    diff = np.abs(score - e["ref"])
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = np.nanmax(np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0)))
    print("%s: worst |diff|/bound %.3g over %d scores" % (what, worst, score.size))
    bad = np.argwhere(diff > bound)
    assert bad.size == 0, (what, bad[:5].tolist(), [(score[i, c], e["ref"][i, c], int(e["n"][i])) for i, c in bad[:5]])


def assert_result(s, e, what="", slack=1):
    assert_counts(s, e, what)
    assert_scores(s.score, e, what, slack)


def loaded(W, case, pos=None, **kw):
    ctx = W.Context(0, **kw)
    ctx.load(case.buf, case.w, pos)
    return ctx


# ------------------------------------------------------------------ 1. shapes and column counts
@pytest.mark.parametrize("C", [1, 5, 16, 17, 128])
@pytest.mark.parametrize("N", [7, 64])
def test_shapes(W, N, C):
    """130 sites (three tiles a side, the last partial: diagonal and
    off-diagonal tiles, ragged rows and columns); N: the sequence tail only /
    one whole stage.  C: one column, a partial chunk, a whole one, one past
    it, the most."""
    c = shape_case(N)
    a = annot_random(130, C, 0xC0 + C)
    ctx = loaded(W, c)
    s = ctx.run_annot_scores(a)
    assert_result(s, expected(c, a), "N=%d C=%d" % (N, C))
    assert s.kernel_ms > 0 and s.tiles == 6 and not s.self_term
    s = ctx.run_annot_scores(a, self_term=True)
    assert s.self_term
    assert_result(s, expected(c, a, self_term=True), "N=%d C=%d self" % (N, C))
    ctx.close()


# ------------------------------------------------------------------ 2. every class, three chunk rows
@pytest.mark.parametrize("self_term", [False, True], ids=["pairs", "self"])
def test_awkward_alignment(W, self_term):
    c = case1()
    a = annot_random(600, 17, 0x17)
    e = expected(c, a, self_term=self_term)
    assert e["none_pairs"] > 0 and e["nonfinite_pairs"] > 0, "every class must occur in the oracle"
    ctx = loaded(W, c)
    s = ctx.run_annot_scores(a, self_term)
    assert_result(s, e, "case 1")
    assert s.pairs == ctx.window_pairs_in_chunks(0, W.Context.chunks(c.L))
    # the summary's counts and partners, exactly
    u = ctx.run_summary()
    assert (s.pairs, s.none_pairs, s.nonfinite_pairs, s.counted_pairs) == \
        (u.pairs, u.none_pairs, u.nonfinite_pairs, u.counted_pairs)
    assert np.array_equal(s.partners, u.partners)
    if self_term:
        # the sites without both symbols take no self term: their scores are their pairs' alone
        plain = ctx.run_annot_scores(a)
        assert np.array_equal(plain.score[[5, 300]], np.zeros((2, 17))) and np.array_equal(s.score[[5, 300]], plain.score[[5, 300]])
    ctx.close()


def test_zero_chunks_and_one_hot(W):
    """The skip path: whole 64-site x 16-column zero blocks on either side of a
    tile, one-hot columns, a column with a single value."""
    c, a = case1(), annot_sparse600()
    ctx = loaded(W, c)
    assert_result(ctx.run_annot_scores(a), expected(c, a), "sparse")
    assert_result(ctx.run_annot_scores(a, True), expected(c, a, self_term=True), "sparse self")
    # the free function: loads and scores
    ss = W.SiteSet.from_buffer(c.buf)
    r = W.ld_annot_scores(ss, c.w, a, names=["c%d" % k for k in range(40)], ctx=ctx)
    assert_result(r, expected(c, a), "ld_annot_scores")
    assert r.names[39] == "c39"
    ctx.close()


# ------------------------------------------------------------------ 3. windows
@pytest.mark.parametrize("with_map,D,K", [(True, 100, 0), (False, 0, 70), (True, 100, 50)],
                         ids=["dist100_map", "sites70", "dist100_map_sites50"])
def test_windows(W, with_map, D, K):
    c = case1()
    pos = case1_map() if with_map else None
    a = annot_random(600, 5, 0x55)
    e = expected(c, a, pos, D, K, self_term=True)
    assert 0 < e["counted_pairs"] < 178228, "counted pairs on both sides of the window"
    ctx = loaded(W, c, pos)
    ctx.set_window(D, K)
    s = ctx.run_annot_scores(a, True)
    assert_result(s, e, "window D=%d K=%d" % (D, K))
    assert s.pairs == ctx.window_pairs_in_chunks(0, W.Context.chunks(c.L))
    ctx.close()
    if with_map and not K:
        ss = W.SiteSet.from_buffer(c.buf, site_map=pos)
        ctx = W.Context(0)
        assert_result(W.ld_annot_scores(ss, c.w, a, self_term=True, max_distance=D, ctx=ctx), e, "ld_annot_scores window")
        assert ctx.window() == (0, 0)
        ctx.close()


# ------------------------------------------------------------------ 4. chunk ranges
@pytest.mark.parametrize("self_term", [False, True], ids=["pairs", "self"])
def test_chunk_ranges_merge(W, self_term):
    c = case1()
    a = annot_random(600, 16, 0x16)
    assert W.Context.chunks(c.L) == 6
    ctx = loaded(W, c)
    whole = expected(c, a, self_term=self_term)
    parts = []
    for rng in ((0, 2), (2, 3), (3, 6)):
        s = ctx.run_annot_scores(a, self_term, rng[0], rng[1])
        assert_result(s, expected(c, a, chunks=rng, self_term=self_term), "chunks [%d,%d)" % rng)
        assert s.pairs == ctx.window_pairs_in_chunks(*rng)
        parts.append(s)
    m = parts[0].merge(parts[1]).merge(parts[2])
    assert m is parts[0]
    assert_result(m, whole, "merged", slack=2)
    assert m.tiles == 55
    # an empty range: all zero, also with the self term
    z = ctx.run_annot_scores(a, self_term, 3, 3)
    assert (z.pairs, z.counted_pairs) == (0, 0) and not z.partners.any() and not z.score.any()
    with pytest.raises(ValueError):
        m.merge(ctx.run_annot_scores(a[:, :3], self_term))
    with pytest.raises(ValueError):
        m.merge(ctx.run_annot_scores(a, not self_term, 3, 3))
    ctx.close()


# ------------------------------------------------------------------ 5. device group
@pytest.mark.parametrize("K", [0, 70], ids=["nowindow", "sites70"])
def test_device_group(W, K):
    c = case1()
    a = annot_random(600, 5, 0x56)
    grp = W.Context(devices=[0, 0])
    grp.load(c.buf, c.w)
    grp.set_window(0, K)
    for self_term in (False, True):
        assert_result(grp.run_annot_scores(a, self_term), expected(c, a, K=K, self_term=self_term),
                      "group self=%d" % self_term, slack=2)
    assert_result(grp.run_annot_scores(a, True, 1, 5), expected(c, a, K=K, chunks=(1, 5), self_term=True),
                  "group [1,5)", slack=2)
    grp.close()


# ------------------------------------------------------------------ 6. cross-checks
def test_all_ones_is_the_ld_score(W):
    c = case1()
    ctx = loaded(W, c)
    s = ctx.run_annot_scores(np.ones((600, 1), dtype=np.float32))
    u = ctx.run_summary()
    assert np.array_equal(s.partners, u.partners)
    # both are any-order f64 sums of the same n nonnegative-up-to-rounding terms
    mag = expected(c, np.ones((600, 1), dtype=np.float32))["mag"][:, 0]
    assert np.all(np.abs(s.score[:, 0] - u.score) <= 2 * u.partners * 2.0 ** -52 * mag)
    ctx.close()


def test_one_hot_cells_against_the_heat_map(W):
    """Column d one-hot over cell d: the scores of cell g's sites in column d
    add up to the heat map's sum of cell pair {g, d} (twice the diagonal's)."""
    c, a = case1(), annot_sparse600()
    cells = (np.arange(600) // 60).astype(np.int32)
    ctx = loaded(W, c)
    s = ctx.run_annot_scores(a)
    h = ctx.run_heatmap(cells, 10)
    got = np.zeros((10, 10))
    np.add.at(got, cells, s.score[:, :10])
    up = np.triu(h.sum)
    want = up + up.T
    n = np.triu(h.count.astype(np.float64))
    n = n + n.T
    mag = np.zeros((10, 10))
    np.add.at(mag, cells, expected(c, a[:, :10])["mag"])
    assert np.all(np.abs(got - want) <= 2 * n * 2.0 ** -52 * mag), np.abs(got - want).max()
    ctx.close()


def _rows(ctx, thr=0.05):
    n = ctx.run(thr)
    r = ctx.rows()
    assert n == len(r)
    return [r.site_a.copy(), r.site_b.copy(), r.d.view(np.uint32).copy(), r.d_prime.view(np.uint32).copy(),
            r.r2.view(np.uint32).copy()]


def _same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


def test_rows_undisturbed(W):
    c = case1()
    a = annot_random(600, 5, 0x57)
    ref, ctx = loaded(W, c), loaded(W, c)  # ref never runs the call
    before = _rows(ctx)
    stats = ctx.stats()
    ctx.run_annot_scores(a, True)
    for f in ("rows", "pairs", "kernel"):
        assert ctx.stats()[f] == stats[f], "wld_last_stats still describes the row run"
    after = ctx.rows()
    assert np.array_equal(after.site_a, before[0]) and np.array_equal(after.r2.view(np.uint32), before[4])
    assert _same(_rows(ctx), before) and _same(before, _rows(ref))
    for K in (64, 0):  # a windowed list, a sub-range: other tile lists between the row runs
        ref.set_window(0, K)
        ctx.set_window(0, K)
        want = _rows(ref)
        ctx.run_annot_scores(a)
        assert _same(_rows(ctx), want), K
        ctx.run_annot_scores(a, False, 0, 2)
        assert _same(_rows(ctx), want), K
    h0, h1 = ref.run_host(0.05), (ctx.run_annot_scores(a), ctx.run_host(0.05))[1]
    assert np.array_equal(h0.site_a, h1.site_a) and np.array_equal(h0.site_b, h1.site_b)
    assert np.array_equal(h0.r2.view(np.uint32), h1.r2.view(np.uint32))
    ref.close()
    ctx.close()


# ------------------------------------------------------------------ 7. errors
def test_errors(W):
    import ctypes

    from weightedld_amd._lib import AnnotScoresC, lib

    c = case1()
    a = annot_random(600, 5, 0x58)
    ctx = W.Context(0)

    def raw(on, annot, n_annot, flags=0, lb=0, le=0):
        """The C call itself (the Python wrapper refuses most of these first)."""
        out = AnnotScoresC()
        p = None if annot is None else annot.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        st = lib().wld_run_annot_scores(on._h, p, n_annot, flags, lb, le, ctypes.byref(out))
        msg = lib().wld_last_error().decode()
        lib().wld_annot_scores_free(ctypes.byref(out))
        return st, msg

    E_ARG, E_STATE = -1, -7
    assert raw(ctx, a, 5)[0] == E_STATE  # before a load
    ctx.load(c.buf, c.w)
    assert raw(ctx, a, 0)[0] == E_ARG
    wide = np.zeros((600, 129), dtype=np.float32)
    assert raw(ctx, wide, 129)[0] == E_ARG
    assert raw(ctx, None, 5)[0] == E_ARG
    assert raw(ctx, a, 5, flags=2)[0] == E_ARG
    assert raw(ctx, a, 5, lb=4, le=2)[0] == E_ARG
    bad = a.copy()
    bad[301, 3] = np.nan
    bad[400, 0] = np.inf
    st, msg = raw(ctx, bad, 5)
    assert st == E_ARG and "site 301" in msg and "column 3" in msg, msg
    with pytest.raises(ValueError):
        ctx.run_annot_scores(bad)
    with pytest.raises(ValueError):
        ctx.run_annot_scores(a[:599])
    ctx.run_chunks_async(0.05)
    assert raw(ctx, a, 5)[0] == E_STATE  # a run in flight
    assert ctx.run_wait() == len(ctx.rows())
    e = expected(c, a)
    assert_result(ctx.run_annot_scores(a), e, "after the refusals")
    w = c.w.copy()
    w[7] = np.inf  # non-finite weights: the row path's select loop
    ctx.load(c.buf, w)
    with pytest.raises(W.WldError) as ei:
        ctx.run_annot_scores(a)
    assert ei.value.name == "WLD_E_ARG"
    grp = W.Context(devices=[0, 0])
    assert raw(grp, a, 5)[0] == E_STATE
    grp.load(c.buf, c.w)
    assert raw(grp, bad, 5)[0] == E_ARG
    assert_result(grp.run_annot_scores(a), e, "group after a refusal", slack=2)
    grp.close()
    ctx.load(c.buf, c.w)
    assert_result(ctx.run_annot_scores(a), e, "after every refusal")
    ctx.close()


# ------------------------------------------------------------------ 8. CLI
def test_cli_vcf(W, tmp_path):
    """t7_1000genome.vcf with an annotation file written here: rows for
    coordinates no site has are skipped, repeated POS take their rows in
    order.  (VCF input takes no site filter; site index = POS.)"""
    path = os.path.join(FIXTURES, "t7_1000genome.vcf")
    vcf = W.read_vcf(path)
    L = vcf.n_sites()
    a = annot_random(L, 3, 0x7C)
    parent = [vcf.parent_site_index(i) for i in range(L)]
    lines = ["site\tcoding\tmaf bin\tcons"]
    for i in range(L):
        if i % 7 == 0 and parent[i] >= 1 and parent[i] - 1 not in set(parent):
            lines.append("%d\t9\t9\t9" % (parent[i] - 1))  # a filtered-out site's row: skipped
        lines.append("%d\t%s" % (parent[i], "\t".join(repr(float(x)) for x in a[i])))
    assert len(lines) > L + 1
    annot_file, out_file = str(tmp_path / "annot.tsv"), str(tmp_path / "l2.tsv")
    with open(annot_file, "w") as f:
        f.write("\n".join(lines) + "\n")
    for extra, window in (([], (None, None)), (["--max-distance", "100", "--max-sites", "3", "--annot-self"], (100, 3))):
        out = subprocess.run([CLI, "--vcf-input", path, "--annot-input", annot_file, "--annot-score-output", out_file,
                              *extra], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        buf = np.ascontiguousarray(vcf.buffer)
        c = Case(buf, W.henikoff_weights(vcf))
        pos = np.asarray(parent, dtype=np.uint64)
        e = expected(c, a, pos, window[0] or 0, window[1] or 0, self_term=bool(extra))
        with open(out_file) as f:
            head = f.readline().rstrip("\n").split("\t")
            rows = [ln.rstrip("\n").split("\t") for ln in f]
        assert head == ["site", "partners", "coding_l2", "maf bin_l2", "cons_l2"] and len(rows) == L
        assert e["counted_pairs"] > 0
        for i, row in enumerate(rows):
            assert int(row[0]) == parent[i] and int(row[1]) == e["partners"][i]
            for k in range(3):
                # %.9g: half a unit of the ninth digit, on top of the sum's own bound
                tol = 5.1e-9 * abs(e["ref"][i, k]) + e["n"][i] * 2.0 ** -52 * e["mag"][i, k]
                assert abs(float(row[2 + k]) - e["ref"][i, k]) <= tol, (i, k, row[2 + k], e["ref"][i, k])
