"""Best partners (wld_run_partners / Context.run_partners / ld_partners / the
CLI's --partners-output): for every loaded site its k strongest in-window LD
partners — the pairs the default row path would emit a row for (in the chunk
range and the window, a statistic, r2 > threshold strictly), ordered by r2
descending under the total order of the f32 bit patterns, then by partner
ascending.

Expected values: the CPU oracle's dense f32 d, d', r2 and `valid` per pair
(O.all_pairs_dense), selected here in numpy by a stable sort on the uint32 key
(the order of heatmap_plan.hpp's float_key), ties to the lower partner.  count,
partner, the bit patterns of d, d' and r2 and the three counters must be equal.
No tolerance applies anywhere.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
from conftest import CLI, FIXTURES, REPO, SYNTH

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


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


def float_key(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


class Case:
    """A data set with its oracle as symmetric [L, L] matrices (entry [s, p] is
    the pair (min, max)'s value; computed once, left unchanged)."""

    def __init__(self, buf, w):
        self.buf, self.w = buf, w
        L = self.L = buf.shape[0]
        d, dp, r2, valid = O.all_pairs_dense(buf, w)
        up = np.triu(np.ones((L, L), dtype=bool), 1)

        def sym(m):
            m = np.where(up, m, 0)
            return m + m.T

        self.d, self.dp, self.r2 = (sym(np.asarray(x, dtype=np.float32).view(np.uint32)).view(np.float32)
                                    for x in (d, dp, r2))
        self.valid = sym((np.asarray(valid) != 0).astype(np.uint8)).astype(bool)
        self.key = float_key(self.r2).astype(np.int64)
        a, b = np.minimum.outer(np.arange(L), np.arange(L)), np.maximum.outer(np.arange(L), np.arange(L))
        n = (L + 255) // 256
        rf = n - 1 - a // 256
        self.lin = rf * (rf + 1) // 2 + (b // 256 - a // 256)
        self.a, self.b = a, b
        for x in (self.buf, self.w, self.d, self.dp, self.r2, self.valid, self.key, self.lin, self.a, self.b):
            x.setflags(write=False)


def expected(case, k, thr, pos=None, D=0, K=0, chunks=None):
    """The oracle's considered pairs and per site the first k candidates."""
    L = case.L
    keep = case.a != case.b
    if D:
        p = np.arange(L, dtype=np.int64) if pos is None else np.asarray(pos, dtype=np.int64)
        keep &= p[case.b] - p[case.a] <= D
    if K:
        keep &= case.b - case.a <= K
    if chunks is not None:
        keep &= (case.lin >= chunks[0]) & (case.lin < chunks[1])
    with np.errstate(invalid="ignore"):
        cand = keep & case.valid & (case.r2 > np.float32(thr))  # (NaN never passes)
    skey = np.where(cand, case.key, -1)
    order = np.argsort(-skey, axis=1, kind="stable")  # key descending, ties to the lower partner
    n_cand = cand.sum(axis=1)
    count = np.minimum(n_cand, k).astype(np.uint32)
    kk = min(k, L)
    top = order[:, :kk]
    filled = np.arange(kk)[None, :] < count[:, None]
    rows = np.arange(L)[:, None]

    def take(m, fill, dt):
        out = np.full((L, k), fill, dtype=dt)
        out[:, :kk] = np.where(filled, m[rows, top], fill)
        return out

    nan = np.uint32(0x7FC00000)
    return {"count": count, "n_cand": n_cand, "order": order, "skey": skey,
            "partner": take(np.broadcast_to(np.arange(L), (L, L)), NONE, np.uint32),
            "d": take(case.d.view(np.uint32), nan, np.uint32), "d_prime": take(case.dp.view(np.uint32), nan, np.uint32),
            "r2": take(case.r2.view(np.uint32), nan, np.uint32),
            "pairs": int(keep.sum()) // 2, "none_pairs": int((keep & ~case.valid).sum()) // 2,
            "passing_pairs": int(cand.sum()) // 2}


def assert_partners(p, e, what=""):
    for f in ("pairs", "none_pairs", "passing_pairs"):
        print("%s: %s got %d expected %d" % (what, f, getattr(p, f), e[f]))
    print("%s: listed %d of %d candidates" % (what, int(p.count.sum()), int(e["n_cand"].sum())))
    for f in ("pairs", "none_pairs", "passing_pairs"):
        assert getattr(p, f) == e[f], (what, f, getattr(p, f), e[f])
    assert p.count.dtype == np.uint32 and np.array_equal(p.count, e["count"]), what
    assert p.partner.shape == e["partner"].shape, what
    bad = np.argwhere(p.partner != e["partner"])
    assert bad.size == 0, (what, "partner", bad[:5].tolist())
    filled = p.partner != NONE
    for f in ("d", "d_prime", "r2"):
        got = getattr(p, f)
        assert got.dtype == np.float32
        bad = np.argwhere((got.view(np.uint32) != e[f]) & filled)
        assert bad.size == 0, (what, f, bad[:5].tolist())
        assert np.isnan(got[~filled]).all(), (what, f, "NaN past count")


def same(x, y):
    return (all(np.array_equal(getattr(x, f).view(np.uint32), getattr(y, f).view(np.uint32))
                for f in ("count", "partner", "d", "d_prime", "r2"))
            and all(getattr(x, f) == getattr(y, f) for f in ("pairs", "none_pairs", "passing_pairs")))


def loaded(W, case, pos=None, **kw):
    ctx = W.Context(0, **kw)
    ctx.load(case.buf, case.w, pos)
    return ctx


@functools.lru_cache(maxsize=None)
def tie_case():
    """ld_blocks(300, 77): five tiles a side, the last ragged; rows equal to
    row 10 in other tiles (bit-equal r2 across tiles), a site without symbols,
    a one-symbol site and a site with few symbols."""
    buf = _bench().ld_blocks(300, 77).copy()
    for r in (11, 70, 131, 290):
        buf[r, :] = buf[10, :]
    buf[5, :] = 0
    buf[200, :] = 4
    buf[64, :40] = 5
    return Case(buf, _henikoff(buf))


@functools.lru_cache(maxsize=None)
def shape_case(N):
    buf = _bench().synth(130, N, seed=0x130 + N)
    return Case(buf, _henikoff(buf))


@functools.lru_cache(maxsize=None)
def case600():
    buf = _bench().ld_blocks(600, 203).copy()
    buf[5, :] = 0
    buf[300, :] = 4
    buf[64, :100] = 5
    return Case(buf, _henikoff(buf))


@functools.lru_cache(maxsize=None)
def map600():
    """POS with repeats and gaps: a cumulative sum of steps 0..3, every 37th step 60."""
    rng = np.random.default_rng(0x4EA7)
    step = rng.integers(0, 4, size=600)
    step[::37] = 60
    m = np.cumsum(step).astype(np.uint64)
    m.setflags(write=False)
    return m


def cross_tile_ties(e, k):
    """Sites whose k-th and (k + 1)-th candidates have equal keys and lie in different 64-site tiles."""
    L = e["order"].shape[0]
    if k >= L:
        return 0
    s = np.arange(L)
    p0, p1 = e["order"][:, k - 1], e["order"][:, k]
    tie = (e["n_cand"] > k) & (e["skey"][s, p0] == e["skey"][s, p1]) & (p0 // 64 != p1 // 64)
    return int(tie.sum())


# ------------------------------------------------------------------ 1. ties and degenerate sites
MUST_TIE = {(1, -1.0), (3, -1.0), (5, 0.0), (8, 0.2), (64, -1.0)}


@pytest.mark.parametrize("thr", [-1.0, 0.0, 0.2])
@pytest.mark.parametrize("k", [1, 3, 5, 8, 64])
def test_ties_and_degenerate_sites(W, k, thr):
    c = tie_case()
    e = expected(c, k, thr)
    ties = cross_tile_ties(e, k)
    print("k %d thr %g: %d sites with a cross-tile tie at the cut" % (k, thr, ties))
    if (k, thr) in MUST_TIE:
        assert ties > 0, "the tie-break and the cross-tile merge must be exercised"
    assert (e["n_cand"] == 0).any(), "a site without a candidate"
    if thr == 0.2 and k >= 8:  # (below that every site with a candidate has dozens)
        assert ((e["n_cand"] > 0) & (e["n_cand"] < k)).any(), "a site with fewer than k candidates"
    ctx = loaded(W, c)
    p = ctx.run_partners(k, thr)
    ctx.close()
    assert p.k == k and p.n_sites == c.L and p.tiles == 15
    assert_partners(p, e, "ties k %d thr %g" % (k, thr))


# ------------------------------------------------------------------ 2. sequence shapes
@pytest.mark.parametrize("N", [5, 8, 64, 203, 520])
def test_sequence_shapes(W, N):
    c = shape_case(N)
    ctx = loaded(W, c)
    for thr in (-1.0, 0.05):
        assert_partners(ctx.run_partners(5, thr), expected(c, 5, thr), "N %d thr %g" % (N, thr))
    ctx.close()


# ------------------------------------------------------------------ 3. fewer sites than k
def test_fewer_sites_than_k(W):
    full = shape_case(64)
    c = Case(full.buf[:40].copy(), full.w.copy())
    e = expected(c, 64, -1.0)
    assert (e["count"] < 64).all() and np.array_equal(e["count"], e["n_cand"])
    ctx = loaded(W, c)
    p = ctx.run_partners(64, -1.0)
    ctx.close()
    assert_partners(p, e, "L 40 k 64")
    assert np.array_equal(p.count, e["n_cand"])


# ------------------------------------------------------------------ 4. windows
@pytest.mark.parametrize("D,K", [(0, 64), (100, 0), (100, 20)])
def test_windows(W, D, K):
    c, pos = case600(), map600()
    ctx = loaded(W, c, pos)
    ctx.set_window(D, K)
    for k, thr in ((4, -1.0), (8, 0.1)):
        e = expected(c, k, thr, pos=pos, D=D, K=K)
        p = ctx.run_partners(k, thr)
        assert_partners(p, e, "window (%d, %d) k %d" % (D, K, k))
        s, r = np.nonzero(p.partner != NONE)
        q = p.partner[s, r].astype(np.int64)
        lo, hi = np.minimum(s, q), np.maximum(s, q)
        if K:
            assert (hi - lo <= K).all()
        if D:
            assert (pos[hi].astype(np.int64) - pos[lo].astype(np.int64) <= D).all()
    ctx.close()


# ------------------------------------------------------------------ 5. chunk ranges
def test_chunk_ranges_merge(W):
    c = case600()  # 3 chunk rows: 6 linear chunks
    ctx = loaded(W, c)
    for k, thr in ((5, -1.0), (8, 0.2)):
        whole = ctx.run_partners(k, thr)
        assert_partners(whole, expected(c, k, thr), "whole")
        for cuts in ([(i, i + 1) for i in range(6)], [(0, 2), (2, 6)]):
            acc = None
            for rng in cuts:
                part = ctx.run_partners(k, thr, rng[0], rng[1])
                assert_partners(part, expected(c, k, thr, chunks=rng), "chunks [%d,%d)" % rng)
                acc = part if acc is None else acc.merge(part)
            assert same(acc, whole), cuts
            assert acc.tiles == whole.tiles
    z = ctx.run_partners(3, 0.0, 4, 4)  # an empty range
    assert (z.pairs, z.passing_pairs, z.tiles) == (0, 0, 0) and not z.count.any() and (z.partner == NONE).all()
    ctx.close()


# ------------------------------------------------------------------ 6. batches
def test_batches(W):
    c = case600()
    ctx = loaded(W, c)
    k = 5
    one = ctx.run_partners(k, -1.0)
    assert_partners(one, expected(c, k, -1.0), "one batch")
    tile_bytes = 128 * (16 * k + 4)
    for tiles_per_batch in (20, 1):  # 55 tiles: 3 batches, then one tile per batch
        ctx.set_option("partners_batch_bytes", tile_bytes * tiles_per_batch if tiles_per_batch > 1 else 1)
        assert -(-one.tiles // tiles_per_batch) >= 3
        assert same(ctx.run_partners(k, -1.0), one), tiles_per_batch
    assert ctx.get_option("partners_batch_bytes") == 1
    ctx.close()


# ------------------------------------------------------------------ 7. device group
@pytest.mark.parametrize("K", [0, 64], ids=["nowindow", "sites64"])
def test_device_group(W, K):
    c = case600()
    one = loaded(W, c)
    grp = W.Context(devices=[0, 0, 0])
    grp.load(c.buf, c.w)
    for ctx in (one, grp):
        ctx.set_window(0, K)
    e = expected(c, 6, 0.05, K=K)
    p1, p3 = one.run_partners(6, 0.05), grp.run_partners(6, 0.05)
    assert_partners(p1, e, "single")
    assert_partners(p3, e, "group of three")
    assert same(p1, p3) and p1.tiles == p3.tiles
    assert_partners(grp.run_partners(6, 0.05, 1, 5), expected(c, 6, 0.05, K=K, chunks=(1, 5)), "group [1,5)")
    one.close()
    grp.close()


# ------------------------------------------------------------------ 8. two GPU paths against each other
def test_against_targets_and_rows(W):
    c = case600()
    ctx = loaded(W, c)
    k, thr = 8, 0.2
    p = ctx.run_partners(k, thr)
    targets = np.array([0, 5, 10, 63, 64, 65, 127, 128, 200, 255, 256, 300, 301, 511, 598, 599], dtype=np.uint32)
    t = ctx.run_targets(targets, thr)  # (no site_map: parent = loaded index)
    for i, s in enumerate(targets.tolist()):
        lo, hi = int(t.offset[i]), int(t.offset[i + 1])
        part, r2 = t.site_partner[lo:hi].astype(np.int64), t.r2[lo:hi]
        order = np.lexsort((part, -float_key(r2).astype(np.int64)))[:k]
        n = order.size
        assert p.count[s] == n == min(k, hi - lo), s
        assert np.array_equal(p.partner[s, :n], part[order]), s
        for f in ("d", "d_prime", "r2"):
            assert np.array_equal(getattr(p, f)[s, :n].view(np.uint32), getattr(t, f)[lo:hi][order].view(np.uint32)), (s, f)
    assert p.passing_pairs == len(ctx.run_host(thr))
    ctx.close()


# ------------------------------------------------------------------ 9. rows undisturbed
def _bits(r):
    return [r.site_a.copy(), r.site_b.copy(), r.d.view(np.uint32).copy(), r.d_prime.view(np.uint32).copy(),
            r.r2.view(np.uint32).copy()]


def _rows(ctx, thr=0.05):
    n = ctx.run(thr)
    r = ctx.rows()
    assert n == len(r)
    return _bits(r)


def _same_rows(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


def test_rows_undisturbed(W):
    c = case600()
    ref, ctx = loaded(W, c), loaded(W, c)  # ref never runs partners
    before = _rows(ctx)
    stats = ctx.stats()
    dev = ctx.rows_device()
    ctx.run_partners(8, 0.1)
    ctx.run_partners(3, -1.0, 0, 2)
    after = ctx.stats()
    for f in ("rows", "pairs", "tiles", "kernel", "ref_sums", "screened"):
        assert after[f] == stats[f], f  # still the row run's
    assert ctx.rows_device() == dev, "the device views of the row run's rows are the same"
    assert _same_rows(_bits(ctx.rows()), before), "rows() after partners returns the row run's rows"
    assert _same_rows(_rows(ctx), before) and _same_rows(before, _rows(ref))
    for K in (64, 0):
        ref.set_window(0, K)
        ctx.set_window(0, K)
        want = _rows(ref)
        ctx.run_partners(8, 0.1)
        assert _same_rows(_rows(ctx), want), K
        st = ctx.stats()
        ctx.run_partners(2, 0.3, 0, 2)
        assert ctx.stats()["rows"] == st["rows"] and ctx.stats()["pairs"] == st["pairs"], K
        assert _same_rows(_bits(ctx.rows()), want), K
        assert _same_rows(_rows(ctx), want), K
    ref.close()
    ctx.close()


# ------------------------------------------------------------------ 10. errors
def test_errors(W):
    c = case600()
    ctx = W.Context(0)

    def refused(status, *args, on=None):
        with pytest.raises(W.WldError) as ei:
            (on or ctx).run_partners(*args)
        assert ei.value.name == status, (ei.value, args)
        return str(ei.value)

    refused("WLD_E_STATE", 4, 0.1)  # before a load
    ctx.load(c.buf, c.w)
    refused("WLD_E_ARG", 0, 0.1)
    refused("WLD_E_ARG", 65, 0.1)
    refused("WLD_E_ARG", 4, float("nan"))
    refused("WLD_E_ARG", 4, 0.1, 4, 2)  # begin > end
    ctx.run_chunks_async(0.05)
    refused("WLD_E_STATE", 4, 0.1)  # a run in flight
    n = ctx.run_wait()
    assert n == len(ctx.rows())
    e = expected(c, 4, 0.1)
    assert_partners(ctx.run_partners(4, 0.1), e, "after the refusals")
    w = c.w.copy()
    w[7] = np.inf
    ctx.load(c.buf, w)
    assert "finite weights" in refused("WLD_E_ARG", 4, 0.1)
    grp = W.Context(devices=[0, 0])
    refused("WLD_E_STATE", 4, 0.1, on=grp)
    grp.load(c.buf, c.w)
    refused("WLD_E_ARG", 65, 0.1, on=grp)
    refused("WLD_E_ARG", 4, float("nan"), on=grp)
    assert_partners(grp.run_partners(4, 0.1), e, "group after a refusal")
    grp.close()
    ctx.load(c.buf, c.w)
    p = ctx.run_partners(4, 0.1)
    assert_partners(p, e, "after every refusal")
    # merging results of different shapes
    with pytest.raises(W.WldError) as ei:
        p.merge(ctx.run_partners(5, 0.1, 0, 0))
    assert ei.value.name == "WLD_E_ARG"
    ctx.close()


# ------------------------------------------------------------------ 11. CLI
def _read_tsv(path):
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        rows = [line.rstrip("\n").split("\t") for line in f]
    return head, rows


def _fmt3(x):
    """The pair TSV's number format (Rust's {:.3} of the f32's exact value)."""
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    return "%.3f" % x


def _cli_case(W, tmp_path, args, loaded_set, k, thr, window, default_thr=0.1):
    """Runs the CLI with a best-partner output and compares the TSV with
    ld_partners on the set the CLI loads.  thr None: no --partners-r2, the
    threshold is --r2-threshold's (default_thr)."""
    out_path = str(tmp_path / "partners.tsv")
    extra = [] if thr is None else ["--partners-r2", repr(thr)]
    out = subprocess.run([CLI, *args, "--partners-output", out_path, "--partners-k", str(k), *extra],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    ctx = W.Context(0)
    p = W.ld_partners(loaded_set, W.henikoff_weights(loaded_set), k, default_thr if thr is None else thr,
                      max_distance=window[0], max_sites=window[1], ctx=ctx)
    ctx.close()
    assert p.count.sum() > 0
    head, rows = _read_tsv(out_path)
    assert head == ["site", "partner", "rank", "d", "d'", "r2"]
    site, part, rank, d, dp, r2 = p.rows(p.site_map)
    assert len(rows) == site.size > 0
    got = np.array([[int(r[0]), int(r[1]), int(r[2])] for r in rows], dtype=np.int64)
    assert np.array_equal(got[:, 0], site.astype(np.int64)) and np.array_equal(got[:, 1], part.astype(np.int64))
    assert np.array_equal(got[:, 2], rank.astype(np.int64))
    for col, want in ((3, d), (4, dp), (5, r2)):
        assert [r[col] for r in rows] == [_fmt3(x) for x in want.tolist()], col
    return p


def test_cli_fasta(W, tmp_path):
    """(a FASTA set's parent coordinate is the column in the unfiltered alignment)"""
    path = os.path.join(SYNTH, "synth_n200_l24.fasta")
    kept = W.read_fasta(path).filter_sites_of_interest(0.8, 0.02, 0.5)
    parent = np.array([kept.parent_site_index(i) for i in range(kept.n_sites())], dtype=np.uint64)
    loaded_set = W.SiteSet.from_buffer(kept.buffer, site_map=parent)
    _cli_case(W, tmp_path, ["--fasta-input", path, "--r2-threshold", "0.005"], loaded_set, 3, None, (None, None),
              default_thr=0.005)
    _cli_case(W, tmp_path, ["--fasta-input", path, "--pair-output", str(tmp_path / "pairs.tsv")], loaded_set, 2, 0.0,
              (None, None))


def test_cli_vcf_window(W, tmp_path):
    path = os.path.join(FIXTURES, "t7_1000genome.vcf")
    vcf = W.read_vcf(path)
    p = _cli_case(W, tmp_path, ["--vcf-input", path, "--max-distance", "100", "--max-sites", "3", "--devices", "0,0"],
                  vcf, 4, 0.0, (100, 3))
    assert (p.count <= 4).all() and p.count.max() > 0
