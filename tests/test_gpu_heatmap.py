"""LD heat map (wld_run_heatmap / Context.run_heatmap / ld_heatmap / the CLI's
--heatmap-output): every considered pair of a chunk range — in the window,
both sites on a cell — classified (none / nonfinite / counted) and reduced on
the device over a caller-defined grid of cells: count, sum and max per cell,
with no rows.

Expected values: the CPU oracle's dense f32 r2, d' and `valid` per pair
(O.all_pairs_dense), reduced here in numpy.  Counts must be equal; max must be
bit-equal to the max of the cell's f32 values.  Each f64 sum is compared with
math.fsum of its f64-converted terms (correctly rounded):
    |got - ref| <= n 2^-52 |ref|,     n = the number of terms,
the bound of an any-order f64 sum of n nonnegative terms (first order
(n - 1) 2^-53, doubled for the higher-order term; |ref| because a one-term
cell may hold an r2 that f32 rounded below zero — its sum is then exact).  One
value off by an f32 ulp moves a sum by ~2^-24 of a term — orders of magnitude
past that — so the bound also pins every pair's value to the oracle's bits.
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

G = 1024  # heatmap_plan::kGridCells: a tile's cell rectangle up to this is reduced in LDS


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
        _, dp, r2, valid = O.all_pairs_dense(buf, w)
        self.a, self.b = np.triu_indices(self.L, 1)
        self.val = {"r2": r2[self.a, self.b], "dprime": np.abs(dp[self.a, self.b])}
        self.valid = (valid != 0)[self.a, self.b]
        n = (self.L + 255) // 256
        rf = n - 1 - self.a // 256
        self.lin = rf * (rf + 1) // 2 + (self.b // 256 - self.a // 256)
        for x in (self.buf, self.w, self.a, self.b, self.val["r2"], self.val["dprime"], self.valid, self.lin):
            x.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case1():
    """ld_blocks(600, 203) — 10 x 10 tiles, the last ragged, 6 chunks — with a
    site without symbols (None pairs), a one-symbol site, and three sites
    whose minor allele sits in few sequences."""
    buf = _bench().ld_blocks(600, 203).copy()
    buf[5, :] = 0
    buf[300, :] = 4
    buf[64, :100] = 5
    buf[470, 100:] = 5
    buf[129, 3:] = 5
    return Case(buf, _henikoff(buf))


@functools.lru_cache(maxsize=None)
def case1_map():
    """POS with repeats and gaps: a cumulative sum of steps 0..3, every 37th
    step 60 (so equal coordinate bins leave cells without a site)."""
    rng = np.random.default_rng(0x4EA7)
    step = rng.integers(0, 4, size=600)
    step[::37] = 60
    m = np.cumsum(step).astype(np.uint64)
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


def expected(case, site_cell, n_cells, stat, pos=None, D=0, K=0, chunks=None):
    """The oracle's considered pairs, reduced: the class counts, count and max
    per cell, and per touched cell (fsum of the terms, their number)."""
    a, b = case.a, case.b
    sc = np.asarray(site_cell, dtype=np.int64)
    keep = (sc[a] >= 0) & (sc[b] >= 0)
    if D:
        p = np.arange(case.L, dtype=np.int64) if pos is None else np.asarray(pos, dtype=np.int64)
        keep &= p[b] - p[a] <= D
    if K:
        keep &= b - a <= K
    if chunks is not None:
        keep &= (case.lin >= chunks[0]) & (case.lin < chunks[1])
    x, v = case.val[stat][keep], case.valid[keep]
    cell = sc[a[keep]] * n_cells + sc[b[keep]]
    fin = np.isfinite(x)
    cnt = v & fin
    x, cell = x[cnt], cell[cnt]
    count = np.bincount(cell, minlength=n_cells * n_cells).reshape(n_cells, n_cells)
    mx = np.full(n_cells * n_cells, -np.inf, dtype=np.float32)
    np.maximum.at(mx, cell, x)
    mx[count.reshape(-1) == 0] = np.nan
    order = np.argsort(cell, kind="stable")
    xs, cs = x[order].astype(np.float64), cell[order]
    cut = np.flatnonzero(np.diff(cs)) + 1
    starts, ends = np.concatenate(([0], cut)), np.concatenate((cut, [cs.size]))
    sums = {}
    if cs.size:
        for s, e in zip(starts.tolist(), ends.tolist()):
            sums[int(cs[s])] = (float(xs[s]) if e - s == 1 else math.fsum(xs[s:e].tolist()), e - s)
    return {"pairs": int(keep.sum()), "none_pairs": int((~v).sum()), "nonfinite_pairs": int((v & ~fin).sum()),
            "counted_pairs": int(cnt.sum()), "count": count, "max": mx.reshape(n_cells, n_cells), "sum": sums,
            "neg": int((x < 0).sum())}


def sum_ok(got, ref, n):
    return abs(got - ref) <= n * 2.0 ** -52 * abs(ref)


def assert_heatmap(h, e, what=""):
    for f in ("pairs", "none_pairs", "nonfinite_pairs", "counted_pairs"):
        assert getattr(h, f) == e[f], (what, f, getattr(h, f), e[f])
    assert h.pairs == h.none_pairs + h.nonfinite_pairs + h.counted_pairs
    n = e["count"].shape[0]
    assert h.count.shape == h.sum.shape == h.max.shape == (n, n) and h.n_cells == n
    assert np.array_equal(h.count.astype(np.int64), e["count"]), what
    assert int(h.count.sum(dtype=np.uint64)) == h.counted_pairs
    assert not np.tril(h.count, -1).any(), "the lower triangle stays empty"
    assert np.array_equal(h.max.view(np.uint32)[e["count"] > 0], e["max"].view(np.uint32)[e["count"] > 0]), what
    assert np.isnan(h.max[e["count"] == 0]).all() and not h.sum[e["count"] == 0].any(), what
    worst = 0.0
    flat = h.sum.reshape(-1)
    for cell, (ref, k) in e["sum"].items():
        if ref:
            worst = max(worst, abs(flat[cell] - ref) / (k * 2.0 ** -52 * abs(ref)))
        assert sum_ok(flat[cell], ref, k), (what, "sum", divmod(cell, n), flat[cell], ref, k)
    print("%s: %d cells with pairs, %d counted, worst |diff|/bound %.3g" % (what, len(e["sum"]), h.counted_pairs, worst))


def loaded(W, case, pos=None, **kw):
    ctx = W.Context(0, **kw)
    ctx.load(case.buf, case.w, pos)
    return ctx


def plan_tiles(site_cell, L):
    """Tiles (ta <= tb) whose row block and column block both hold a site with a cell (no window)."""
    sc = np.asarray(site_cell)
    flag = [bool((sc[t * 64:(t + 1) * 64] >= 0).any()) for t in range((L + 63) // 64)]
    return sum(1 for ta in range(len(flag)) for tb in range(ta, len(flag)) if flag[ta] and flag[tb])


def rect_cells(site_cell, L):
    """The largest cell rectangle a 64 x 64 tile touches."""
    sc = np.asarray(site_cell)
    span = []
    for t in range((L + 63) // 64):
        on = sc[t * 64:(t + 1) * 64]
        on = on[on >= 0]
        span.append(int(on[-1] - on[0] + 1) if on.size else 0)
    return max(span) ** 2


# the cell layouts of the 600-site case: name -> (site_cell, n_cells)
def layouts():
    s = np.arange(600)
    gene = np.full(600, -1)
    gene[40:150] = 0
    gene[400:520] = 2  # (cell 1 has no site)
    region = np.full(600, -1)
    region[130:390] = (np.arange(260) // 20)
    return {
        "sites50": (s // 50, 12),               # cuts off the tile edges: coarse
        "one_site": (s, 600),                   # 64 x 64 cells per tile: fine
        "one_cell": (np.zeros(600, int), 1),
        "region": (region, 13),                 # sites 130..389
        "gene_x_gene": (gene, 3),
        "rect_at_G": (s // 2, 300),             # 32 x 32 = G cells per tile: the last coarse size
        "rect_past_G": ((s + 1) // 2, 301),     # 33 x 33 on whole tiles (fine), less on the ragged ones (coarse)
    }


# ------------------------------------------------------------------ 1. cell layouts
@pytest.mark.parametrize("stat", ["r2", "dprime"])
@pytest.mark.parametrize("name", list(layouts()))
def test_cell_layouts(W, name, stat):
    c = case1()
    site_cell, n_cells = layouts()[name]
    e = expected(c, site_cell, n_cells, stat)
    assert e["counted_pairs"] > 0
    ctx = loaded(W, c)
    h = ctx.run_heatmap(site_cell, n_cells, stat)
    assert_heatmap(h, e, "%s %s" % (name, stat))
    assert h.stat == stat and h.kernel_ms > 0
    assert h.tiles == plan_tiles(site_cell, c.L)
    if name in ("sites50", "one_site", "one_cell"):
        assert h.pairs == 600 * 599 // 2 and h.tiles == 55
        assert e["none_pairs"] > 0 and (stat == "dprime" or e["nonfinite_pairs"] > 0)
    if name == "one_site":
        assert int(h.count.max()) == 1
    if name == "region":
        assert h.tiles == 15 < 55
    if name == "rect_at_G":
        assert rect_cells(site_cell, c.L) == G
    if name == "rect_past_G":
        assert rect_cells(site_cell, c.L) == 33 * 33 > G
    # mean and the mirrored image
    m = h.mean()
    on = h.count > 0
    assert np.isnan(m[~on]).all() and np.array_equal(m[on], h.sum[on] / h.count[on])
    sym = h.symmetric("count")
    assert np.array_equal(sym, sym.T) and np.array_equal(np.triu(sym), h.count)
    ctx.close()


def test_coordinate_bins(W):
    """Equal bins of a site_map with repeats; some cells have no site."""
    c, pos = case1(), case1_map()
    site_cell, n_cells, cell_start = W.heatmap_cells(pos, cell_width=16)
    assert np.setdiff1d(np.arange(n_cells), site_cell).size > 0, "some cells must be empty"
    ctx = loaded(W, c, pos)
    for stat in ("r2", "dprime"):
        assert_heatmap(ctx.run_heatmap(site_cell, n_cells, stat), expected(c, site_cell, n_cells, stat), "bins " + stat)
    # the free function: builds the same cells, loads and runs
    ss = W.SiteSet.from_buffer(c.buf, site_map=pos)
    h = W.ld_heatmap(ss, c.w, cell_width=16, ctx=ctx)
    assert_heatmap(h, expected(c, site_cell, n_cells, "r2"), "ld_heatmap")
    assert np.array_equal(h.cell_start, cell_start) and np.array_equal(h.site_cell, site_cell)
    ctx.close()


def test_case1_oracle_counts():
    """The counts the data set was built for (a change of bench.ld_blocks would show here first)."""
    e = expected(case1(), np.zeros(600, int), 1, "r2")
    assert (e["pairs"], e["none_pairs"], e["nonfinite_pairs"], e["counted_pairs"]) == (179700, 1197, 275, 178228)


# ------------------------------------------------------------------ 2. windows
@pytest.mark.parametrize("D,K", [(0, 64), (100, 0), (100, 20)], ids=["sites64", "dist100", "dist100_sites20"])
@pytest.mark.parametrize("layout", ["sites50", "bins"])
def test_windows(W, layout, D, K):
    c, pos = case1(), case1_map()
    site_cell, n_cells = layouts()["sites50"] if layout == "sites50" else W.heatmap_cells(pos, cell_width=16)[:2]
    ctx = loaded(W, c, pos)
    ctx.set_window(D, K)
    for stat in ("r2", "dprime"):
        e, full = expected(c, site_cell, n_cells, stat, pos, D, K), expected(c, site_cell, n_cells, stat)
        assert 0 < e["counted_pairs"] < full["counted_pairs"], "counted pairs on both sides of the window"
        h = ctx.run_heatmap(site_cell, n_cells, stat)
        assert_heatmap(h, e, "%s window D=%d K=%d %s" % (layout, D, K, stat))
        assert h.pairs == ctx.window_pairs_in_chunks(0, W.Context.chunks(c.L))  # (every site has a cell)
        assert h.tiles < 55
    ctx.close()


# ------------------------------------------------------------------ 3. sequence counts
@pytest.mark.parametrize("N", [5, 8, 64, 203, 520])
def test_shapes(W, N):
    """130 sites (three tiles a side, the last partial), 16-site cells; N: a
    tail only, no tail, one stage, tail + partial stage, several stages per
    lane class."""
    c = shape_case(N)
    site_cell, n_cells = np.arange(130) // 16, 9
    ctx = loaded(W, c)
    for stat in ("r2", "dprime"):
        assert_heatmap(ctx.run_heatmap(site_cell, n_cells, stat), expected(c, site_cell, n_cells, stat),
                       "N=%d %s" % (N, stat))
    ctx.close()


# ------------------------------------------------------------------ 4. a larger set
def test_larger_set(W):
    """5,000 sites (a tile list past 3,072 tiles and past one wave of
    workgroups), 64 cells of 79 sites."""
    c = case5()
    site_cell, n_cells, _ = W.heatmap_cells(None, 5000, sites_per_cell=79)
    assert n_cells == 64
    ctx = loaded(W, c)
    h = ctx.run_heatmap(site_cell, n_cells)
    assert_heatmap(h, expected(c, site_cell, n_cells, "r2"), "5000 sites")
    assert h.tiles == plan_tiles(site_cell, c.L) == 79 * 80 // 2
    ctx.close()


# ------------------------------------------------------------------ 5. chunk ranges
def _combine(parts):
    count = sum(p.count.astype(np.int64) for p in parts)
    with np.errstate(invalid="ignore"):
        mx = functools.reduce(np.fmax, [p.max for p in parts])
    return count, mx, sum(p.sum for p in parts)


@pytest.mark.parametrize("split", [[(i, i + 1) for i in range(6)], [(0, 2), (2, 6)]], ids=["single_chunks", "2+4"])
def test_chunk_ranges_combine(W, split):
    c = case1()
    assert W.Context.chunks(c.L) == 6
    site_cell, n_cells = layouts()["sites50"]
    ctx = loaded(W, c)
    for stat in ("r2", "dprime"):
        whole = expected(c, site_cell, n_cells, stat)
        parts = []
        for rng in split:
            h = ctx.run_heatmap(site_cell, n_cells, stat, rng[0], rng[1])
            assert_heatmap(h, expected(c, site_cell, n_cells, stat, chunks=rng), "chunks [%d,%d) %s" % (*rng, stat))
            parts.append(h)
        for f in ("pairs", "none_pairs", "nonfinite_pairs", "counted_pairs"):
            assert sum(getattr(p, f) for p in parts) == whole[f], f
        count, mx, sm = _combine(parts)
        assert np.array_equal(count, whole["count"])
        on = whole["count"] > 0
        assert np.array_equal(mx.view(np.uint32)[on], whole["max"].view(np.uint32)[on]) and np.isnan(mx[~on]).all()
        for cell, (ref, k) in whole["sum"].items():
            assert sum_ok(sm.reshape(-1)[cell], ref, k), (cell, ref, k)
    # an empty range: all empty
    z = ctx.run_heatmap(site_cell, n_cells, "r2", 3, 3)
    assert (z.pairs, z.counted_pairs, z.tiles) == (0, 0, 0) and not z.count.any() and np.isnan(z.max).all()
    ctx.close()


# ------------------------------------------------------------------ 6. device group
@pytest.mark.parametrize("K", [0, 64], ids=["nowindow", "sites64"])
def test_device_group(W, K):
    c = case1()
    one = loaded(W, c)
    grp = W.Context(devices=[0, 0, 0])
    grp.load(c.buf, c.w)
    for ctx in (one, grp):
        ctx.set_window(0, K)
    for name in ("sites50", "rect_past_G"):
        site_cell, n_cells = layouts()[name]
        e = expected(c, site_cell, n_cells, "r2", K=K)
        h1, h3 = one.run_heatmap(site_cell, n_cells), grp.run_heatmap(site_cell, n_cells)
        assert_heatmap(h1, e, "single " + name)
        assert_heatmap(h3, e, "group of three " + name)
        assert np.array_equal(h1.count, h3.count) and np.array_equal(h1.max.view(np.uint32), h3.max.view(np.uint32))
        assert h1.tiles == h3.tiles
    # ... and over a sub-range of the chunks
    site_cell, n_cells = layouts()["sites50"]
    assert_heatmap(grp.run_heatmap(site_cell, n_cells, "dprime", 1, 5),
                   expected(c, site_cell, n_cells, "dprime", K=K, chunks=(1, 5)), "group [1,5)")
    one.close()
    grp.close()


# ------------------------------------------------------------------ 7. rows undisturbed
def _rows(ctx, thr=0.05):
    n = ctx.run(thr)
    r = ctx.rows()
    assert n == len(r)
    return _bits(r)


def _bits(r):
    return [r.site_a.copy(), r.site_b.copy(), r.d.view(np.uint32).copy(), r.d_prime.view(np.uint32).copy(),
            r.r2.view(np.uint32).copy()]


def _same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


def test_rows_undisturbed(W):
    c = case1()
    site_cell, n_cells = layouts()["sites50"]
    part, n_part = layouts()["region"]
    ref, ctx = loaded(W, c), loaded(W, c)  # ref never runs a heat map
    before = _rows(ctx)
    stats = ctx.stats()
    ctx.run_heatmap(site_cell, n_cells)
    ctx.run_heatmap(part, n_part, "dprime", 0, 2)
    after = ctx.stats()
    for f in ("rows", "pairs", "tiles", "kernel", "ref_sums", "screened"):
        assert after[f] == stats[f], f  # still the row run's
    assert _same(_bits(ctx.rows()), before), "rows() after the heat map returns the row run's rows"
    assert _same(_rows(ctx), before) and _same(before, _rows(ref))
    # no window -> max_sites 64 -> none, a heat map (whole, and of a sub-range
    # of another layout: another tile list) before and between the row runs
    for K in (64, 0):
        ref.set_window(0, K)
        ctx.set_window(0, K)
        want = _rows(ref)
        ctx.run_heatmap(site_cell, n_cells)
        assert _same(_rows(ctx), want), K
        st = ctx.stats()
        ctx.run_heatmap(part, n_part, "r2", 0, 2)
        assert ctx.stats()["rows"] == st["rows"] and ctx.stats()["pairs"] == st["pairs"], K
        assert _same(_bits(ctx.rows()), want), K
        assert _same(_rows(ctx), want), K
    ref.close()
    ctx.close()


# ------------------------------------------------------------------ 8. errors
def test_errors(W):
    c = case1()
    site_cell, n_cells = layouts()["sites50"]
    ctx = W.Context(0)

    def refused(status, *args, on=None):
        with pytest.raises(W.WldError) as ei:
            (on or ctx).run_heatmap(*args)
        assert ei.value.name == status, (ei.value, args[1:])
        return str(ei.value)

    refused("WLD_E_STATE", site_cell, n_cells)  # before a load
    ctx.load(c.buf, c.w)
    refused("WLD_E_ARG", site_cell, 0)
    refused("WLD_E_ARG", site_cell, 4097)
    refused("WLD_E_ARG", site_cell, n_cells, 2)  # an unknown stat
    refused("WLD_E_ARG", None, n_cells)
    bad = site_cell.copy()
    bad[77] = 12
    assert "site_cell[77]" in refused("WLD_E_ARG", bad, n_cells)  # an id >= n_cells
    bad = site_cell.copy()
    bad[[30, 91]] = -2
    assert "site_cell[30]" in refused("WLD_E_ARG", bad, n_cells)  # an id < -1: the first
    bad = site_cell.copy()
    bad[300] = -1
    bad[301] = 5  # (site 299 is on cell 5, site 300 on none: an equal id after a gap is fine)
    assert ctx.run_heatmap(bad, n_cells).pairs == 599 * 598 // 2
    bad[301] = 4
    msg = refused("WLD_E_ARG", bad, n_cells)  # a descending id, across a -1 gap
    assert "site_cell[301]" in msg and "site_cell[299]" in msg
    refused("WLD_E_ARG", site_cell, n_cells, "r2", 4, 2)  # begin > end
    ctx.run_chunks_async(0.05)
    refused("WLD_E_STATE", site_cell, n_cells)  # a run in flight
    n = ctx.run_wait()
    assert n == len(ctx.rows())
    e = expected(c, site_cell, n_cells, "r2")
    assert_heatmap(ctx.run_heatmap(site_cell, n_cells), e, "after the refusals")
    # non-finite weights: the row path's select loop has no heat map
    w = c.w.copy()
    w[7] = np.inf
    ctx.load(c.buf, w)
    assert "finite weights" in refused("WLD_E_ARG", site_cell, n_cells)
    # a group: the same refusals
    grp = W.Context(devices=[0, 0])
    refused("WLD_E_STATE", site_cell, n_cells, on=grp)
    grp.load(c.buf, c.w)
    refused("WLD_E_ARG", site_cell, 4097, on=grp)
    bad = site_cell.copy()
    bad[599] = 3
    assert "site_cell[599]" in refused("WLD_E_ARG", bad, n_cells, on=grp)
    assert_heatmap(grp.run_heatmap(site_cell, n_cells), e, "group after a refusal")
    grp.close()
    ctx.load(c.buf, c.w)
    assert_heatmap(ctx.run_heatmap(site_cell, n_cells), e, "after every refusal")
    # the Python layer's own checks
    with pytest.raises(ValueError):
        ctx.run_heatmap(site_cell[:-1], n_cells)
    with pytest.raises(ValueError):
        ctx.run_heatmap(site_cell, n_cells, "r")
    ctx.close()


# ------------------------------------------------------------------ 9. CLI
def _read_tsv(path):
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        rows = [line.rstrip("\n").split("\t") for line in f]
    return head, rows


def _cli_case(W, tmp_path, args, loaded_set, cells, stat, window):
    """Runs the CLI with a heat-map output and compares the TSV with
    ld_heatmap on the set the CLI loads (loaded_set; parent coordinates as
    its site_map), Henikoff weights, the same cells and window."""
    heat, pairs = str(tmp_path / "heat.tsv"), str(tmp_path / "pairs.tsv")
    out = subprocess.run([CLI, *args, "--pair-output", pairs, "--heatmap-output", heat], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    ctx = W.Context(0)
    h = W.ld_heatmap(loaded_set, W.henikoff_weights(loaded_set), stat=stat, max_distance=window[0],
                     max_sites=window[1], ctx=ctx, **cells)
    ctx.close()
    assert h.counted_pairs > 0
    head, rows = _read_tsv(heat)
    assert head == ["cell_a_start", "cell_b_start", "pairs", "sum", "mean", "max"]
    want = [(i, j) for i in range(h.n_cells) for j in range(i, h.n_cells) if h.count[i, j]]
    assert len(rows) == len(want) > 0
    mean = h.mean()
    for (i, j), (sa, sb, n, s, m, mx) in zip(want, rows):
        assert (int(sa), int(sb), int(n)) == (int(h.cell_start[i]), int(h.cell_start[j]), int(h.count[i, j]))
        assert float(s) == pytest.approx(h.sum[i, j], rel=1e-8, abs=0)
        assert float(m) == pytest.approx(mean[i, j], rel=1e-8, abs=0)
        assert np.float32(float(mx)) == h.max[i, j]
    return h


def test_cli_fasta(W, tmp_path):
    """(a FASTA set's parent coordinate is the column in the unfiltered alignment)"""
    path = os.path.join(SYNTH, "synth_n200_l24.fasta")
    kept = W.read_fasta(path).filter_sites_of_interest(0.8, 0.02, 0.5)
    parent = np.array([kept.parent_site_index(i) for i in range(kept.n_sites())], dtype=np.uint64)
    loaded_set = W.SiteSet.from_buffer(kept.buffer, site_map=parent)
    h = _cli_case(W, tmp_path, ["--fasta-input", path, "--heatmap-cell-sites", "5", "--heatmap-stat", "dprime"],
                  loaded_set, {"sites_per_cell": 5}, "dprime", (None, None))
    assert h.n_cells == (kept.n_sites() + 4) // 5 > 1
    lo, hi = int(parent[2]), int(parent[-3])
    h = _cli_case(W, tmp_path, ["--fasta-input", path, "--heatmap-cell-width", "3", "--heatmap-region",
                                "%d:%d" % (lo, hi)], loaded_set, {"cell_width": 3, "region": (lo, hi)}, "r2", (None, None))
    assert h.pairs < kept.n_sites() * (kept.n_sites() - 1) // 2, "the region must cut pairs"


def test_cli_vcf_window(W, tmp_path):
    """(VCF input takes no site filter; site index = POS, the window's and the cells' coordinate)"""
    path = os.path.join(FIXTURES, "t7_1000genome.vcf")
    vcf = W.read_vcf(path)
    h = _cli_case(W, tmp_path, ["--vcf-input", path, "--max-distance", "100", "--max-sites", "3",
                                "--heatmap-cell-width", "40", "--devices", "0,0"], vcf, {"cell_width": 40}, "r2", (100, 3))
    ctx = W.Context(0)
    full = W.ld_heatmap(vcf, W.henikoff_weights(vcf), cell_width=40, ctx=ctx)
    ctx.close()
    assert h.pairs < full.pairs, "the window must cut pairs"
