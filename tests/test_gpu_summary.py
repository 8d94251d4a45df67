"""LD summaries (wld_run_summary / Context.run_summary / ld_summary / the CLI's
--ld-score-output and --decay-output): every in-window pair of a chunk range
classified (none / nonfinite / counted) and reduced on the device — class
counts, r2_sum, per-site score and partner count, the decay histogram — with
no rows.

Expected values: the CPU oracle's dense f32 r2 and `valid` per pair
(O.all_pairs_dense), reduced here in numpy.  Counts must be equal.  Each f64
sum is compared with math.fsum of its f64-converted terms (correctly rounded):
    |got - ref| <= n 2^-52 ref,     n = the number of terms,
the bound of an any-order f64 sum of n nonnegative terms (first order
(n - 1) 2^-53, doubled for the higher-order term).  One r2 off by an f32 ulp
moves a sum by ~2^-24 of a term — orders of magnitude past that — so the
bound also pins every pair's r2 to the oracle's bits.
"""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
from conftest import CLI, FIXTURES, REPO, SYNTH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def W():
    import weightedld_amd as W
    return W


def _bench():
    import sys
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import bench
    return bench


def _henikoff(buf):
    import weightedld_amd as W
    return W.henikoff_weights(W.SiteSet.from_buffer(buf))


class Case:
    """A data set with its oracle (computed once, left unchanged)."""

    def __init__(self, buf, w):
        self.buf, self.w = buf, w
        self.L = buf.shape[0]
        _, _, r2, valid = O.all_pairs_dense(buf, w)
        self.r2, self.valid = r2, valid != 0
        for a in (self.buf, self.w, self.r2, self.valid):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case1():
    """ld_blocks(600, 203) with a site without symbols (None pairs), a
    one-symbol site, and three sites whose minor allele sits in few sequences."""
    buf = _bench().ld_blocks(600, 203).copy()
    buf[5, :] = 0
    buf[300, :] = 4
    buf[64, :100] = 5
    buf[470, 100:] = 5
    buf[129, 3:] = 5
    return Case(buf, _henikoff(buf))


@functools.lru_cache(maxsize=None)
def case1_map():
    """POS with repeats: a cumulative sum of steps 0..3."""
    rng = np.random.default_rng(0x5117)
    m = np.cumsum(rng.integers(0, 4, size=600)).astype(np.uint64)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def shape_case(N):
    buf = _bench().synth(130, N, seed=0x130 + N)
    return Case(buf, _henikoff(buf))


@functools.lru_cache(maxsize=None)
def case5():
    buf = _bench().synth(5000, 40)
    return Case(buf, _henikoff(buf))


def chunk_linear(n, row, col):
    rf = n - 1 - row
    return rf * (rf + 1) // 2 + (col - row)


def expected(case, pos=None, D=0, K=0, bin_width=0, n_bins=0, chunks=None, scores=True):
    """The oracle's pairs of the range and window, reduced: a dict of the
    class counts, the exact integer arrays, and per sum (ref, n_terms)."""
    L = case.L
    a, b = np.triu_indices(L, 1)
    p = np.arange(L, dtype=np.int64) if pos is None else np.asarray(pos, dtype=np.int64)
    keep = np.ones(a.size, dtype=bool)
    if D:
        keep &= p[b] - p[a] <= D
    if K:
        keep &= b - a <= K
    if chunks is not None:
        n = (L + 255) // 256
        lin = chunk_linear(n, a // 256, b // 256)
        keep &= (lin >= chunks[0]) & (lin < chunks[1])
    a, b = a[keep], b[keep]
    r = case.r2[a, b]
    v = case.valid[a, b]
    fin = np.isfinite(r)
    cnt = v & fin
    ca, cb, x = a[cnt], b[cnt], r[cnt].astype(np.float64)
    e = {"pairs": int(a.size), "none_pairs": int((~v).sum()), "nonfinite_pairs": int((v & ~fin).sum()),
         "counted_pairs": int(cnt.sum()), "nan": int((v & np.isnan(r)).sum()),
         "r2_sum": (math.fsum(x.tolist()), x.size),
         "partners": np.bincount(ca, minlength=L) + np.bincount(cb, minlength=L)}

    if scores:
        # a site's terms: its row and column of the symmetric matrix of counted
        # r2 (the zeros of the other pairs add nothing to an exact sum)
        X = np.zeros((L, L))
        X[ca, cb] = x
        X[cb, ca] = x
        e["score"] = [(math.fsum(X[i].tolist()), int(e["partners"][i])) for i in range(L)]
    if bin_width:
        k = np.minimum((p[cb] - p[ca]) // bin_width, n_bins - 1)
        e["bin_pairs"] = np.bincount(k, minlength=n_bins)
        e["bin_r2_sum"] = [(math.fsum(x[k == j].tolist()), int(e["bin_pairs"][j])) for j in range(n_bins)]
    return e


def assert_sum(got, ref_n, what):
    ref, n = ref_n
    print("%s: got %.17g ref %.17g n %d |diff|/bound %.3g" %
          (what, got, ref, n, abs(got - ref) / (n * 2.0 ** -52 * ref) if n and ref else 0.0))
    assert abs(got - ref) <= n * 2.0 ** -52 * ref, (what, got, ref, n)


def assert_summary(s, e, what=""):
    for f in ("pairs", "none_pairs", "nonfinite_pairs", "counted_pairs"):
        assert getattr(s, f) == e[f], (what, f, getattr(s, f), e[f])
    assert s.pairs == s.none_pairs + s.nonfinite_pairs + s.counted_pairs
    assert np.array_equal(s.partners.astype(np.int64), e["partners"]), what
    assert int(s.partners.sum(dtype=np.uint64)) == 2 * s.counted_pairs
    assert_sum(s.r2_sum, e["r2_sum"], what + " r2_sum")
    if "score" in e:
        assert s.score.shape == (len(e["score"]),)
        for i, ref_n in enumerate(e["score"]):
            ref, n = ref_n
            assert abs(s.score[i] - ref) <= n * 2.0 ** -52 * ref, (what, "score", i, s.score[i], ref, n)
    if "bin_pairs" in e:
        assert np.array_equal(s.bin_pairs.astype(np.int64), e["bin_pairs"]), what
        assert int(s.bin_pairs.sum(dtype=np.uint64)) == s.counted_pairs
        for k, ref_n in enumerate(e["bin_r2_sum"]):
            ref, n = ref_n
            assert abs(s.bin_r2_sum[k] - ref) <= n * 2.0 ** -52 * ref, (what, "bin", k, s.bin_r2_sum[k], ref, n)
    else:
        assert s.bin_pairs is None and s.bin_r2_sum is None


def loaded(W, case, pos=None, **kw):
    ctx = W.Context(0, **kw)
    ctx.load(case.buf, case.w, pos)
    return ctx


# ------------------------------------------------------------------ 1. awkward alignment
@pytest.mark.parametrize("with_map", [False, True], ids=["index", "site_map"])
def test_awkward_alignment(W, with_map):
    c = case1()
    pos = case1_map() if with_map else None
    e = expected(c, pos, bin_width=8, n_bins=32)
    assert e["pairs"] == 600 * 599 // 2
    assert e["none_pairs"] > 0 and e["nonfinite_pairs"] > 0, "every class must occur in the oracle"
    assert e["bin_pairs"][31] > 0 and (e["bin_pairs"][:31] > 0).sum() >= 2, "overflow bin and two others"
    ctx = loaded(W, c, pos)
    s = ctx.run_summary(8, 32)
    assert_summary(s, e, "case 1")
    assert s.pairs == ctx.window_pairs_in_chunks(0, W.Context.chunks(c.L))
    assert s.kernel_ms > 0
    # without bins: the same counts and scores, no bin arrays
    s0 = ctx.run_summary()
    assert_summary(s0, expected(c, pos), "case 1, no bins")
    # the free function: loads and summarizes
    ss = W.SiteSet.from_buffer(c.buf, site_map=pos) if with_map else W.SiteSet.from_buffer(c.buf)
    assert_summary(W.ld_summary(ss, c.w, bin_width=8, n_bins=32, ctx=ctx), e, "ld_summary")
    ctx.close()


def test_case1_oracle_counts():
    """The counts the data set was built for (a change of bench.ld_blocks would show here first)."""
    e = expected(case1(), scores=False)
    assert (e["pairs"], e["none_pairs"], e["nan"], e["nonfinite_pairs"], e["counted_pairs"]) == \
        (179700, 1197, 275, 275, 178228)


# ------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize("N", [5, 8, 64, 203, 520])
def test_shapes(W, N):
    """130 sites (three tiles a side, the last partial); N: a tail only, no
    tail, one stage, tail + partial stage, several stages per lane class."""
    c = shape_case(N)
    ctx = loaded(W, c)
    assert_summary(ctx.run_summary(3, 16), expected(c, bin_width=3, n_bins=16), "N=%d" % N)
    ctx.close()


@pytest.mark.parametrize("L", [1, 2, 65])
def test_tiny_sets(W, L):
    """One site (no pair), one pair, and one site past a tile."""
    buf = _bench().synth(L, 12, seed=0x71 + L)
    c = Case(buf, _henikoff(buf))
    ctx = loaded(W, c)
    assert_summary(ctx.run_summary(1, 4), expected(c, bin_width=1, n_bins=4), "L=%d" % L)
    ctx.close()


# ------------------------------------------------------------------ 3. windows
@pytest.mark.parametrize("with_map,D,K", [(False, 0, 70), (False, 100, 0), (True, 100, 0), (True, 100, 50)],
                         ids=["sites70", "dist100", "dist100_map", "dist100_map_sites50"])
def test_windows(W, with_map, D, K):
    c = case1()
    pos = case1_map() if with_map else None
    e, full = expected(c, pos, D, K, bin_width=8, n_bins=32), expected(c, pos, scores=False)
    assert 0 < e["counted_pairs"] < full["counted_pairs"], "counted pairs on both sides of the window"
    ctx = loaded(W, c, pos)
    ctx.set_window(D, K)
    s = ctx.run_summary(8, 32)
    assert_summary(s, e, "window D=%d K=%d" % (D, K))
    assert s.pairs == ctx.window_pairs_in_chunks(0, W.Context.chunks(c.L))
    ctx.close()


# ------------------------------------------------------------------ 4. chunk ranges
def test_chunk_ranges_add_up(W):
    c = case1()
    assert W.Context.chunks(c.L) == 6
    ctx = loaded(W, c)
    whole = expected(c, bin_width=8, n_bins=32)
    parts = []
    for rng in ((0, 2), (2, 6)):
        s = ctx.run_summary(8, 32, rng[0], rng[1])
        assert_summary(s, expected(c, bin_width=8, n_bins=32, chunks=rng), "chunks [%d,%d)" % rng)
        assert s.pairs == ctx.window_pairs_in_chunks(*rng)
        parts.append(s)
    p, q = parts
    for f in ("pairs", "none_pairs", "nonfinite_pairs", "counted_pairs"):
        assert getattr(p, f) + getattr(q, f) == whole[f], f
    assert np.array_equal(p.partners.astype(np.int64) + q.partners, whole["partners"])
    assert np.array_equal(p.bin_pairs.astype(np.int64) + q.bin_pairs.astype(np.int64), whole["bin_pairs"])
    assert_sum(p.r2_sum + q.r2_sum, whole["r2_sum"], "r2_sum of the parts")
    for i, (ref, n) in enumerate(whole["score"]):
        assert abs(p.score[i] + q.score[i] - ref) <= n * 2.0 ** -52 * ref, i
    for k, (ref, n) in enumerate(whole["bin_r2_sum"]):
        assert abs(p.bin_r2_sum[k] + q.bin_r2_sum[k] - ref) <= n * 2.0 ** -52 * ref, k
    # an empty range: all zero
    z = ctx.run_summary(8, 32, 3, 3)
    assert (z.pairs, z.counted_pairs, z.r2_sum) == (0, 0, 0.0) and not z.partners.any() and not z.bin_pairs.any()
    ctx.close()


# ------------------------------------------------------------------ 5. past the row path's size switch
def test_past_the_row_paths_switch(W):
    """5,000 sites: 3,081 tiles, past the 3,072 at which the row path goes from
    16-row items to whole-tile workgroups (the shapes above are below it).  The
    summary launches whole-tile workgroups at every size."""
    c = case5()
    e = expected(c, bin_width=64, n_bins=40)
    assert e["nan"] > 0
    ctx = loaded(W, c)
    assert_summary(ctx.run_summary(64, 40), e, "5000 sites")
    ctx.close()


# ------------------------------------------------------------------ 6. device group
@pytest.mark.parametrize("K", [0, 70], ids=["nowindow", "sites70"])
def test_device_group(W, K):
    c = case1()
    e = expected(c, K=K, bin_width=8, n_bins=32)
    one = loaded(W, c)
    grp = W.Context(devices=[0, 0, 0])
    grp.load(c.buf, c.w)
    for ctx in (one, grp):
        ctx.set_window(0, K)
    s1, s3 = one.run_summary(8, 32), grp.run_summary(8, 32)
    assert_summary(s1, e, "single")
    assert_summary(s3, e, "group of three")
    # ... and over a sub-range of the chunks
    assert_summary(grp.run_summary(8, 32, 1, 5), expected(c, K=K, bin_width=8, n_bins=32, chunks=(1, 5)), "group [1,5)")
    one.close()
    grp.close()


# ------------------------------------------------------------------ 7. rows undisturbed
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
    ref, ctx = loaded(W, c), loaded(W, c)  # ref never runs a summary
    before = _rows(ctx)
    stats = ctx.stats()
    ctx.run_summary(8, 32)
    assert ctx.stats()["rows"] == stats["rows"] and ctx.stats()["pairs"] == stats["pairs"]  # still the row run's
    assert _same(_rows(ctx), before) and _same(before, _rows(ref))
    # no window -> max_sites 64 -> none, a summary (whole, and of a sub-range:
    # another tile list) before and between the row runs of each state
    for K in (64, 0):
        ref.set_window(0, K)
        ctx.set_window(0, K)
        want = _rows(ref)
        ctx.run_summary(8, 32)
        assert _same(_rows(ctx), want), K
        ctx.run_summary(0, 0, 0, 2)
        assert _same(_rows(ctx), want), K
    ref.close()
    ctx.close()


# ------------------------------------------------------------------ 8. errors
def test_errors(W):
    c = case1()
    ctx = W.Context(0)

    def refused(status, *args, on=None):
        with pytest.raises(W.WldError) as ei:
            (on or ctx).run_summary(*args)
        assert ei.value.name == status, (ei.value, args)
        return str(ei.value)

    refused("WLD_E_STATE")  # before a load
    ctx.load(c.buf, c.w)
    refused("WLD_E_ARG", 8, 1025)
    refused("WLD_E_ARG", 0, 1025)
    refused("WLD_E_ARG", 8, 0)
    refused("WLD_E_ARG", 0, 0, 4, 2)  # begin > end
    ctx.run_chunks_async(0.05)
    refused("WLD_E_STATE", 8, 32)  # a run in flight
    n = ctx.run_wait()
    assert n == len(ctx.rows())
    e = expected(c, bin_width=8, n_bins=32, scores=False)
    assert_summary(ctx.run_summary(8, 32), e, "after the refusals")
    # a site_map that descends: no bins (the window's rule); without bins it runs
    pos = case1_map().copy()
    pos[200] = pos[199] - 1
    ctx.load(c.buf, c.w, pos)
    assert "non-decreasing site_map" in refused("WLD_E_ARG", 8, 32) and "site_map[200]" in refused("WLD_E_ARG", 8, 32)
    assert_summary(ctx.run_summary(), expected(c, scores=False), "descending map, no bins")
    # non-finite weights: the row path's select loop has no summary
    w = c.w.copy()
    w[7] = np.inf
    ctx.load(c.buf, w)
    refused("WLD_E_ARG")
    # a group: the same refusals
    grp = W.Context(devices=[0, 0])
    refused("WLD_E_STATE", on=grp)
    grp.load(c.buf, c.w)
    refused("WLD_E_ARG", 8, 1025, on=grp)
    assert_summary(grp.run_summary(8, 32), e, "group after a refusal")
    grp.close()
    ctx.load(c.buf, c.w)
    assert_summary(ctx.run_summary(8, 32), e, "after every refusal")
    ctx.close()


# ------------------------------------------------------------------ 9. CLI
def _read_tsv(path):
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        rows = [line.rstrip("\n").split("\t") for line in f]
    return head, rows


def _cli_case(W, tmp_path, args, loaded_set, window):
    """Runs the CLI with both summary outputs and compares them with the API's
    result on the set the CLI loads (loaded_set), Henikoff weights, the window."""
    score, decay, pairs = (str(tmp_path / n) for n in ("score.tsv", "decay.tsv", "pairs.tsv"))
    cmd = [CLI, *args, "--pair-output", pairs, "--ld-score-output", score, "--decay-output", decay,
           "--decay-bin-width", "7", "--decay-bins", "12"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    ctx = W.Context(0)
    s = W.ld_summary(loaded_set, W.henikoff_weights(loaded_set), bin_width=7, n_bins=12, max_distance=window[0],
                     max_sites=window[1], ctx=ctx)
    ctx.close()
    assert s.counted_pairs > 0
    head, rows = _read_tsv(score)
    assert head == ["site", "partners", "ld_score"] and len(rows) == loaded_set.n_sites()
    for i, (site, partners, sc) in enumerate(rows):
        assert int(site) == loaded_set.parent_site_index(i) and int(partners) == s.partners[i]
        assert float(sc) == pytest.approx(s.score[i], rel=1e-8, abs=0)
    head, rows = _read_tsv(decay)
    assert head == ["bin_start", "pairs", "r2_sum", "mean_r2"] and len(rows) == 12
    mean = s.mean_r2()
    for k, (start, n, rsum, m) in enumerate(rows):
        assert int(start) == 7 * k and int(n) == s.bin_pairs[k]
        assert float(rsum) == pytest.approx(s.bin_r2_sum[k], rel=1e-8, abs=0)
        if s.bin_pairs[k]:
            assert float(m) == pytest.approx(mean[k], rel=1e-8, abs=0)
        else:
            assert m == "nan"
    return s


def test_cli_fasta(W, tmp_path):
    path = os.path.join(SYNTH, "synth_n200_l24.fasta")
    _cli_case(W, tmp_path, ["--fasta-input", path], W.read_fasta(path).filter_sites_of_interest(0.8, 0.02, 0.5),
              (None, None))


def test_cli_vcf_window(W, tmp_path):
    """(VCF input takes no site filter; site index = POS, the window's and the bins' coordinate)"""
    path = os.path.join(FIXTURES, "t7_1000genome.vcf")
    vcf = W.read_vcf(path)
    s = _cli_case(W, tmp_path, ["--vcf-input", path, "--max-distance", "100", "--max-sites", "3"], vcf, (100, 3))
    ctx = W.Context(0)
    full = W.ld_summary(vcf, W.henikoff_weights(vcf), ctx=ctx)
    ctx.close()
    assert s.pairs < full.pairs, "the window must cut pairs"
