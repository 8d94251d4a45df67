"""LD blocks (wld_run_block_breaks / wld_blocks_from_breaks / wld_run_blocks,
Context.run_block_breaks / blocks_from_breaks / run_blocks, ld_blocks, the
CLI's --blocks-output): every considered pair of a chunk range classified
(none / nonfinite / strong / weak) on the device, the weak pairs reduced to the
per-site break arrays, the site axis partitioned on the host, and the pairs
inside the reported blocks reduced to per-block statistics.

Expected values: the CPU oracle's dense f32 r2, d' and `valid` per pair
(O.all_pairs_dense), reduced here in numpy straight from the definitions (the
partition from the weak MATRIX, not from break arrays).  Class counts, break
arrays, partition, per-block counts and value_min (bit for bit) must be equal.
Each f64 value_sum is compared with math.fsum of its f64-converted terms:
    |got - ref| <= n 2^-52 |ref|,     n = the number of terms,
the heat-map test's bound of an any-order f64 sum of n exact terms, for its
reason: one value off by an f32 ulp moves a sum by ~2^-24 of a term.

The generator, the oracle reduction and the non-vacuity checks touch no device
(tests/test_blocks_api.py reuses them on the CPU)."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
from conftest import CLI, FIXTURES, REPO, SYNTH

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
STRONG_R2, STRONG_DP = 0.55, 0.45
SEED = 0xB10C5


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
    return O.henikoff_weights(buf)


def planted(L=600, N=203, seed=SEED):
    """Planted LD blocks: runs of 1-150 sites, each a copy of one random 0/1
    pattern (minor share 0.3-0.5) with a random per-site major/minor swap and
    5 % missing.  In about half of the runs of >= 6 sites two interior sites
    are flipped in disjoint tenths of the sequences: they stay strong with the
    rest of the run and are weak with each other, so the two rules differ.
    Then a site without symbols, a one-symbol site and a site with symbol 5 in
    half the sequences.  Returns (buf, the planted runs' [first, last])."""
    rng = np.random.Generator(np.random.PCG64(seed))
    buf = np.empty((L, N), dtype=np.uint8)
    runs = []
    s0 = 0
    while s0 < L:
        n = int(rng.integers(1, 13)) if rng.random() < 0.5 else int(rng.integers(13, 151))
        s1 = min(L, s0 + n)
        n = s1 - s0
        pat = np.zeros(N, dtype=bool)
        pat[rng.permutation(N)[:int(round(rng.uniform(0.3, 0.5) * N))]] = True
        allele = np.repeat(pat[None, :], n, axis=0) ^ (rng.random((n, 1)) < 0.5)
        if n >= 6 and rng.random() < 0.5:
            i1, i2 = sorted(rng.choice(np.arange(1, n - 1), size=2, replace=False).tolist())
            tenth = rng.permutation(N)
            k = N // 10
            allele[i1, tenth[:k]] ^= True
            allele[i2, tenth[k:2 * k]] ^= True
        maj = rng.integers(0, 4, size=n)
        mnr = (maj + rng.integers(1, 4, size=n)) % 4
        col = np.where(allele, mnr[:, None], maj[:, None])
        buf[s0:s1] = np.where(rng.random((n, N)) < 0.05, 4, col)
        runs.append((s0, s1 - 1))
        s0 = s1
    return buf, runs


class Case:
    """A data set with its oracle (computed once, left unchanged): the dense
    upper-triangle values, `valid` and each pair's linear chunk."""

    def __init__(self, buf, w):
        self.buf, self.w = buf, w
        self.L = L = buf.shape[0]
        _, dp, r2, valid = O.all_pairs_dense(buf, w)
        up = np.triu(np.ones((L, L), dtype=bool), 1)
        self.up = up
        self.val = {"r2": np.where(up, r2, np.float32(0)).astype(np.float32),
                    "dprime": np.where(up, np.abs(dp), np.float32(0)).astype(np.float32)}
        self.valid = (valid != 0) & up
        n = (L + 255) // 256
        a, b = np.indices((L, L))
        rf = n - 1 - a // 256
        self.lin = rf * (rf + 1) // 2 + (b // 256 - a // 256)
        for x in (self.buf, self.w, self.up, self.val["r2"], self.val["dprime"], self.valid, self.lin):
            x.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case1():
    buf, _ = planted()
    buf = buf.copy()
    buf[300, :] = 4      # a site without symbols
    buf[5, :] = 0        # a one-symbol site
    buf[64, :100] = 5    # symbol 5 in half the sequences
    buf[129, 3:] = 5     # three sequences left: non-finite values
    return Case(buf, _henikoff(buf))


@functools.lru_cache(maxsize=None)
def case1_map():
    """POS with repeats and gaps: a cumulative sum of steps 0..3, every 37th step 60."""
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


def window_last(L, pos=None, D=0, K=0):
    """last[a]: the last b <= min(L - 1, a + K) (K == 0: L - 1) with pos[b] - pos[a] <= D (D == 0: no limit)."""
    p = np.arange(L, dtype=np.int64) if pos is None else np.asarray(pos, dtype=np.int64)
    last = np.empty(L, dtype=np.int64)
    for a in range(L):
        hi = min(L - 1, a + K) if K else L - 1
        if D:
            hi = min(hi, int(np.searchsorted(p, p[a] + D, side="right")) - 1)
        last[a] = max(hi, a)
    return last


def classes(case, stat, strong_min, last, chunks=None):
    """Boolean L x L matrices of the considered pairs and their classes."""
    L = case.L
    b = np.arange(L)[None, :]
    con = case.up & (b <= last[:, None])
    if chunks is not None:
        con = con & (case.lin >= chunks[0]) & (case.lin < chunks[1])
    x = case.val[stat]
    fin = np.isfinite(x)
    none = con & ~case.valid
    nonfin = con & case.valid & ~fin
    inf = con & case.valid & fin
    strong = inf & (x >= np.float32(strong_min))
    return {"con": con, "none": none, "nonfinite": nonfin, "inf": inf, "strong": strong, "weak": inf & ~strong}


def break_arrays(weak):
    """fwd_weak / bwd_weak of a weak matrix, by the definition."""
    L = weak.shape[0]
    fwd = np.full(L, NONE, dtype=np.uint32)
    bwd = np.full(L, NONE, dtype=np.uint32)
    rows = weak.any(axis=1)
    fwd[rows] = weak.argmax(axis=1)[rows]
    cols = weak.any(axis=0)
    bwd[cols] = (L - 1 - weak[::-1, :].argmax(axis=0))[cols]
    return fwd, bwd


def run_valid(weak, s, e, rule):
    if rule == "all":
        return not weak[s:e + 1, s:e + 1].any()
    return not weak[s, s:e + 1].any() and not weak[s:e + 1, e].any()


def partition(weak, last, rule, min_sites=2):
    """The partition straight from the definition, on the weak matrix: the
    runs (first, last, whether the run ends at last[first] < L - 1), the
    reported blocks and site_block."""
    L = weak.shape[0]
    runs, s = [], 0
    while s < L:
        e = next(c for c in range(int(last[s]), s - 1, -1) if c == s or run_valid(weak, s, c, rule))
        runs.append((s, e))
        s = e + 1
    first = np.array([r[0] for r in runs if r[1] - r[0] + 1 >= min_sites], dtype=np.uint32)
    lst = np.array([r[1] for r in runs if r[1] - r[0] + 1 >= min_sites], dtype=np.uint32)
    site_block = np.full(L, -1, dtype=np.int32)
    for k, (f, l) in enumerate(zip(first.tolist(), lst.tolist())):
        site_block[f:l + 1] = k
    return {"first": first, "last": lst, "site_block": site_block}


def expected(case, stat, strong_min, rule, min_sites=2, pos=None, D=0, K=0):
    """Everything a whole blocks run must return, from the oracle."""
    last = window_last(case.L, pos, D, K)
    cl = classes(case, stat, strong_min, last)
    fwd, bwd = break_arrays(cl["weak"])
    p = partition(cl["weak"], last, rule, min_sites)
    x = case.val[stat]
    stats = []
    for f, l in zip(p["first"].tolist(), p["last"].tolist()):
        sl = (slice(f, l + 1), slice(f, l + 1))
        inf = cl["inf"][sl]
        v = x[sl][inf]
        stats.append({"pairs": int(cl["con"][sl].sum()), "informative": int(inf.sum()),
                      "strong": int(cl["strong"][sl].sum()),
                      "sum": math.fsum(v.astype(np.float64).tolist()), "n": int(v.size),
                      "min": v.min() if v.size else np.float32("nan")})
    tot = {k: int(cl[k].sum()) for k in ("con", "none", "nonfinite", "strong", "weak")}
    return {"last": last.astype(np.uint32), "fwd": fwd, "bwd": bwd, "tot": tot, "stats": stats, **p}


def sum_ok(got, ref, n):
    return abs(got - ref) <= n * 2.0 ** -52 * abs(ref)


def assert_breaks(b, case, stat, strong_min, last, chunks=None, what=""):
    cl = classes(case, stat, strong_min, last, chunks)
    fwd, bwd = break_arrays(cl["weak"])
    got = (b.pairs, b.none_pairs, b.nonfinite_pairs, b.strong_pairs, b.weak_pairs)
    want = tuple(int(cl[k].sum()) for k in ("con", "none", "nonfinite", "strong", "weak"))
    print("%s: classes %s" % (what, got))
    assert got == want, (what, got, want)
    assert b.pairs == b.none_pairs + b.nonfinite_pairs + b.strong_pairs + b.weak_pairs
    assert np.array_equal(b.fwd_weak, fwd), (what, "fwd_weak", np.flatnonzero(b.fwd_weak != fwd)[:5])
    assert np.array_equal(b.bwd_weak, bwd), (what, "bwd_weak", np.flatnonzero(b.bwd_weak != bwd)[:5])
    assert np.array_equal(b.last, last.astype(np.uint32)), (what, "last")
    assert b.stat == stat and b.strong_min == float(np.float32(strong_min))


def assert_blocks(r, e, what=""):
    assert np.array_equal(r.first, e["first"]) and np.array_equal(r.last, e["last"]), \
        (what, r.first.tolist(), e["first"].tolist())
    assert np.array_equal(r.site_block, e["site_block"]), what
    assert r.n_blocks == len(e["stats"]) and r.n_sites == e["site_block"].size
    worst = 0.0
    for k, s in enumerate(e["stats"]):
        got = (int(r.pairs[k]), int(r.informative[k]), int(r.strong[k]))
        assert got == (s["pairs"], s["informative"], s["strong"]), (what, k, got, s)
        if s["n"]:
            assert r.value_min[k:k + 1].view(np.uint32)[0] == np.float32(s["min"]).view(np.uint32), (what, k, "min")
            if s["sum"]:
                worst = max(worst, abs(r.value_sum[k] - s["sum"]) / (s["n"] * 2.0 ** -52 * abs(s["sum"])))
            assert sum_ok(r.value_sum[k], s["sum"], s["n"]), (what, k, "sum", r.value_sum[k], s["sum"], s["n"])
        else:
            assert np.isnan(r.value_min[k]) and r.value_sum[k] == 0.0, (what, k)
    m = r.mean
    inf = r.informative > 0
    assert np.array_equal(m[inf], r.value_sum[inf] / r.informative[inf]) and np.isnan(m[~inf]).all()
    print("%s: %d blocks, sizes %s, worst |diff|/bound %.3g" % (what, r.n_blocks, r.sites.tolist(), worst))


def non_vacuous(case):
    """The planted case is worth running: checked on the oracle alone."""
    L = case.L
    e_all, e_sp = expected(case, "r2", STRONG_R2, "all"), expected(case, "r2", STRONG_R2, "spine")
    for e in (e_all, e_sp):
        assert int(((e["last"].astype(int) - e["first"].astype(int) + 1) >= 3).sum()) >= 5, "blocks of >= 3 sites"
        assert any(f <= 255 and l >= 256 for f, l in zip(e["first"].tolist(), e["last"].tolist())), \
            "a block across sites 255/256 (two chunks)"
    assert not (np.array_equal(e_all["first"], e_sp["first"]) and np.array_equal(e_all["last"], e_sp["last"])), \
        "the two rules give different partitions"
    assert e_all["tot"]["none"] > 0
    # a boundary that only weak pairs across two 64-site blocks decide: the run
    # [s, e] ends before its window does, and every weak pair (i, e + 1) with
    # s <= i <= e has i in another 64-site block than e + 1
    weak = classes(case, "r2", STRONG_R2, window_last(L))["weak"]
    crossing = 0
    for s, e in zip(e_all["first"].tolist(), e_all["last"].tolist()):
        if e + 1 < L:
            i = np.flatnonzero(weak[s:e + 1, e + 1]) + s
            crossing += bool(i.size and (i // 64 != (e + 1) // 64).all())
    assert crossing >= 1, "a boundary decided across 64-site blocks"
    # under max_sites 40 a block ends at the cap
    for rule in ("all", "spine"):
        e = expected(case, "r2", STRONG_R2, rule, K=40)
        capped = sum(1 for f, l in zip(e["first"].tolist(), e["last"].tolist()) if l == f + 40 and l < L - 1)
        assert capped >= 1, "a block that ends at last[s]"
    return e_all, e_sp


def loaded(W, case, pos=None, **kw):
    ctx = W.Context(0, **kw)
    ctx.load(case.buf, case.w, pos)
    return ctx


# ------------------------------------------------------------------ 1. rules and statistics
@pytest.mark.parametrize("stat,strong_min", [("r2", STRONG_R2), ("dprime", STRONG_DP)])
@pytest.mark.parametrize("rule", ["all", "spine"])
def test_rules_and_stats(W, rule, stat, strong_min):
    c = case1()
    if stat == "r2":
        non_vacuous(c)
    e = expected(c, stat, strong_min, rule)
    ctx = loaded(W, c)
    b = ctx.run_block_breaks(strong_min, stat)
    assert_breaks(b, c, stat, strong_min, window_last(c.L), what="breaks %s" % stat)
    assert b.pairs == 600 * 599 // 2 == ctx.window_pairs_in_chunks(0, W.Context.chunks(c.L))
    assert b.tiles == 55 and b.kernel_ms > 0
    r = ctx.run_blocks(strong_min, stat, rule)
    assert_blocks(r, e, "%s %s" % (rule, stat))
    assert (r.stat, r.rule, r.min_sites) == (stat, rule, 2) and r.kernel_ms > 0
    assert (r.break_pairs, r.break_weak_pairs, r.break_tiles) == (b.pairs, b.weak_pairs, 55)
    assert 0 < r.tiles < 55, "pass 2 launches only the tiles the blocks touch"
    if rule == "all":
        assert np.array_equal(r.strong, r.informative)
    # the host-only partition of the same breaks, and larger minimum sizes
    p = b.partition(rule)
    assert np.array_equal(p.first, r.first) and np.array_equal(p.last, r.last) and p.pairs is None and p.mean is None
    for m in (3, 5):
        assert_blocks(ctx.blocks_from_breaks(b, rule, m), expected(c, stat, strong_min, rule, m), "min_sites %d" % m)
    # the blocks as a heat map's cells: the diagonal cells are the blocks
    h = ctx.run_heatmap(r.site_cell(), r.n_blocks, stat)
    d = np.arange(r.n_blocks)
    assert np.array_equal(h.count[d, d], r.informative)
    ctx.close()


# ------------------------------------------------------------------ 2. windows
@pytest.mark.parametrize("D,K", [(0, 40), (100, 0), (100, 20)], ids=["sites40", "dist100", "dist100_sites20"])
def test_windows(W, D, K):
    c, pos = case1(), case1_map()
    ctx = loaded(W, c, pos)
    ctx.set_window(D, K)
    last = window_last(c.L, pos, D, K)
    b = ctx.run_block_breaks(STRONG_R2)
    assert_breaks(b, c, "r2", STRONG_R2, last, what="window D=%d K=%d" % (D, K))
    assert b.pairs == ctx.window_pairs_in_chunks(0, W.Context.chunks(c.L)) < 600 * 599 // 2 and b.tiles < 55
    for rule in ("all", "spine"):
        e = expected(c, "r2", STRONG_R2, rule, pos=pos, D=D, K=K)
        r = ctx.run_blocks(STRONG_R2, "r2", rule)
        assert_blocks(r, e, "window D=%d K=%d %s" % (D, K, rule))
        assert (r.last.astype(int) <= last[r.first.astype(int)]).all()
        first, lst = r.parents(pos)
        assert np.array_equal(first, pos[r.first.astype(int)]) and np.array_equal(lst, pos[r.last.astype(int)])
    ctx.close()


# ------------------------------------------------------------------ 3. sequence counts
@pytest.mark.parametrize("N", [5, 8, 64, 203])
def test_shapes(W, N):
    """130 sites (three tiles a side, the last partial); N: a tail only, no
    tail, one stage, tail + partial stage.  The threshold is the median of the
    oracle's finite values, so both classes are large."""
    c = shape_case(N)
    ctx = loaded(W, c)
    for stat in ("r2", "dprime"):
        x = c.val[stat][c.valid & np.isfinite(c.val[stat])]
        thr = float(np.median(x))
        b = ctx.run_block_breaks(thr, stat)
        assert_breaks(b, c, stat, thr, window_last(c.L), what="N=%d %s" % (N, stat))
        assert b.weak_pairs > 0 and b.strong_pairs > 0
        for rule in ("all", "spine"):
            assert_blocks(ctx.run_blocks(thr, stat, rule), expected(c, stat, thr, rule), "N=%d %s %s" % (N, stat, rule))
    ctx.close()


# ------------------------------------------------------------------ 4. chunk ranges
@pytest.mark.parametrize("split", [[(i, i + 1) for i in range(6)], [(0, 2), (2, 6)]], ids=["single_chunks", "2+4"])
def test_chunk_ranges_merge(W, split):
    c = case1()
    assert W.Context.chunks(c.L) == 6
    ctx = loaded(W, c)
    last = window_last(c.L)
    whole = ctx.run_block_breaks(STRONG_R2)
    merged = None
    for rng in split:
        b = ctx.run_block_breaks(STRONG_R2, "r2", rng[0], rng[1])
        assert_breaks(b, c, "r2", STRONG_R2, last, chunks=rng, what="chunks [%d,%d)" % rng)
        merged = b if merged is None else merged.merge(b)
    for f in ("fwd_weak", "bwd_weak", "last"):
        assert np.array_equal(getattr(merged, f), getattr(whole, f)), f
    for f in ("pairs", "none_pairs", "nonfinite_pairs", "strong_pairs", "weak_pairs", "tiles"):
        assert getattr(merged, f) == getattr(whole, f), f
    for rule in ("all", "spine"):
        a, r = ctx.blocks_from_breaks(merged, rule), ctx.run_blocks(STRONG_R2, "r2", rule)
        assert_blocks(a, expected(c, "r2", STRONG_R2, rule), "merged " + rule)
        for f in ("first", "last", "site_block", "pairs", "informative", "strong"):
            assert np.array_equal(getattr(a, f), getattr(r, f)), f
        assert np.array_equal(a.value_min.view(np.uint32), r.value_min.view(np.uint32))
    # an empty range: no pair, no break
    z = ctx.run_block_breaks(STRONG_R2, "r2", 3, 3)
    assert (z.pairs, z.tiles) == (0, 0) and (z.fwd_weak == NONE).all() and (z.bwd_weak == NONE).all()
    assert np.array_equal(z.last, whole.last)
    ctx.close()


# ------------------------------------------------------------------ 5. device group
@pytest.mark.parametrize("K", [0, 40], ids=["nowindow", "sites40"])
def test_device_group(W, K):
    c = case1()
    one = loaded(W, c)
    grp = W.Context(devices=[0, 0])
    grp.load(c.buf, c.w)
    for ctx in (one, grp):
        ctx.set_window(0, K)
    last = window_last(c.L, K=K)
    b1, b2 = one.run_block_breaks(STRONG_R2), grp.run_block_breaks(STRONG_R2)
    assert_breaks(b2, c, "r2", STRONG_R2, last, what="group of two")
    for f in ("fwd_weak", "bwd_weak", "last"):
        assert np.array_equal(getattr(b1, f), getattr(b2, f)), f
    assert b1.tiles == b2.tiles
    assert_breaks(grp.run_block_breaks(STRONG_R2, "r2", 1, 5), c, "r2", STRONG_R2, last, chunks=(1, 5), what="group [1,5)")
    for rule in ("all", "spine"):
        r1, r2 = one.run_blocks(STRONG_R2, "r2", rule), grp.run_blocks(STRONG_R2, "r2", rule)
        assert_blocks(r2, expected(c, "r2", STRONG_R2, rule, K=K), "group " + rule)
        for f in ("first", "last", "site_block", "pairs", "informative", "strong"):
            assert np.array_equal(getattr(r1, f), getattr(r2, f)), f
        assert np.array_equal(r1.value_min.view(np.uint32), r2.value_min.view(np.uint32))
    one.close()
    grp.close()


# ------------------------------------------------------------------ 6. run to run
def test_two_runs_identical(W):
    c = case1()
    ctx = loaded(W, c)
    for stat, thr in (("r2", STRONG_R2), ("dprime", STRONG_DP)):
        b = [ctx.run_block_breaks(thr, stat) for _ in range(2)]
        for f in ("fwd_weak", "bwd_weak", "last"):
            assert getattr(b[0], f).tobytes() == getattr(b[1], f).tobytes(), f
        for f in ("pairs", "none_pairs", "nonfinite_pairs", "strong_pairs", "weak_pairs"):
            assert getattr(b[0], f) == getattr(b[1], f), f
        for rule in ("all", "spine"):
            r = [ctx.run_blocks(thr, stat, rule) for _ in range(2)]
            for f in ("first", "last", "site_block", "pairs", "informative", "strong", "value_min"):
                assert getattr(r[0], f).tobytes() == getattr(r[1], f).tobytes(), (stat, rule, f)
    ctx.close()


# ------------------------------------------------------------------ 7. rows undisturbed
def _bits(r):
    return [r.site_a.copy(), r.site_b.copy(), r.d.view(np.uint32).copy(), r.d_prime.view(np.uint32).copy(),
            r.r2.view(np.uint32).copy()]


def _rows(ctx, thr=0.05):
    n = ctx.run(thr)
    r = ctx.rows()
    assert n == len(r)
    return _bits(r)


def _same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


def test_rows_undisturbed(W):
    c = case1()
    ref, ctx = loaded(W, c), loaded(W, c)  # ref never runs a blocks call
    before = _rows(ctx)
    stats = ctx.stats()
    ctx.run_blocks(STRONG_R2)
    ctx.run_block_breaks(STRONG_DP, "dprime", 0, 2)
    after = ctx.stats()
    for f in ("rows", "pairs", "tiles", "kernel", "ref_sums", "screened"):
        assert after[f] == stats[f], f  # still the row run's
    assert _same(_bits(ctx.rows()), before), "rows() after a blocks run returns the row run's rows"
    assert _same(_rows(ctx), before) and _same(before, _rows(ref))
    for K in (40, 0):
        ref.set_window(0, K)
        ctx.set_window(0, K)
        want = _rows(ref)
        ctx.run_blocks(STRONG_R2, "r2", "spine")
        assert _same(_rows(ctx), want), K
        st = ctx.stats()
        ctx.run_block_breaks(STRONG_R2, "r2", 0, 2)
        assert ctx.stats()["rows"] == st["rows"] and ctx.stats()["pairs"] == st["pairs"], K
        assert _same(_bits(ctx.rows()), want), K
        assert _same(_rows(ctx), want), K
    ref.close()
    ctx.close()


# ------------------------------------------------------------------ 8. errors
def test_errors(W):
    c = case1()
    ctx = W.Context(0)

    def refused(status, call, *args):
        with pytest.raises(W.WldError) as ei:
            call(*args)
        assert ei.value.name == status, (ei.value, args)
        return str(ei.value)

    refused("WLD_E_STATE", ctx.run_block_breaks, 0.5)  # before a load
    refused("WLD_E_STATE", ctx.run_blocks, 0.5)
    ctx.load(c.buf, c.w)
    good = ctx.run_block_breaks(STRONG_R2)
    refused("WLD_E_ARG", ctx.run_block_breaks, 0.5, 2)  # an unknown stat
    refused("WLD_E_ARG", ctx.run_blocks, 0.5, "r2", 2)  # an unknown rule
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused("WLD_E_ARG", ctx.run_block_breaks, bad)
        refused("WLD_E_ARG", ctx.run_blocks, bad)
    for m in (0, 1):
        refused("WLD_E_ARG", ctx.run_blocks, 0.5, "r2", "all", m)
        refused("WLD_E_ARG", ctx.blocks_from_breaks, good, "all", m)
    refused("WLD_E_ARG", ctx.run_block_breaks, 0.5, "r2", 4, 2)  # begin > end
    # breaks of another set, of another threshold or statistic
    small = shape_case(8)
    other = loaded(W, small)
    foreign = other.run_block_breaks(STRONG_R2)
    assert "sites" in refused("WLD_E_ARG", ctx.blocks_from_breaks, foreign)
    refused("WLD_E_ARG", good.merge, foreign)
    refused("WLD_E_ARG", good.merge, ctx.run_block_breaks(0.5))
    refused("WLD_E_ARG", good.merge, ctx.run_block_breaks(STRONG_R2, "dprime"))
    ctx.set_window(0, 40)
    refused("WLD_E_ARG", good.merge, ctx.run_block_breaks(STRONG_R2))  # another window: another last
    ctx.set_window(0, 0)
    other.close()
    ctx.run_chunks_async(0.05)
    refused("WLD_E_STATE", ctx.run_block_breaks, 0.5)  # a run in flight
    refused("WLD_E_STATE", ctx.run_blocks, 0.5)
    refused("WLD_E_STATE", ctx.blocks_from_breaks, good)
    n = ctx.run_wait()
    assert n == len(ctx.rows())
    e = expected(c, "r2", STRONG_R2, "all")
    assert_blocks(ctx.run_blocks(STRONG_R2), e, "after the refusals")
    # non-finite weights: the row path's select loop has no blocks
    w = c.w.copy()
    w[7] = np.inf
    ctx.load(c.buf, w)
    assert "finite weights" in refused("WLD_E_ARG", ctx.run_block_breaks, 0.5)
    assert "finite weights" in refused("WLD_E_ARG", ctx.run_blocks, 0.5)
    # a group: the same refusals
    grp = W.Context(devices=[0, 0])
    refused("WLD_E_STATE", grp.run_blocks, 0.5)
    grp.load(c.buf, c.w)
    refused("WLD_E_ARG", grp.run_blocks, 0.5, "r2", "all", 1)
    refused("WLD_E_ARG", grp.run_block_breaks, float("nan"))
    assert_blocks(grp.run_blocks(STRONG_R2), e, "group after a refusal")
    grp.close()
    ctx.load(c.buf, c.w)
    assert_blocks(ctx.run_blocks(STRONG_R2), e, "after every refusal")
    # the Python layer's own checks
    with pytest.raises(ValueError):
        ctx.run_blocks(0.5, "r")
    with pytest.raises(ValueError):
        ctx.run_blocks(0.5, "r2", "solid")
    ctx.close()


# ------------------------------------------------------------------ 9. CLI
def _read_tsv(path):
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        rows = [line.rstrip("\n").split("\t") for line in f]
    return head, rows


def _cli_case(W, tmp_path, args, loaded_set, strong_min, stat, rule, min_sites, window, pair=True):
    """Runs the CLI with a blocks output and compares the TSV with ld_blocks
    on the set the CLI loads (parent coordinates as its site_map), Henikoff
    weights, the same threshold, rule and window."""
    blocks, pairs = str(tmp_path / "blocks.tsv"), str(tmp_path / "pairs.tsv")
    out = subprocess.run([CLI, *args, *(["--pair-output", pairs] if pair else []), "--blocks-output", blocks],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    ctx = W.Context(0)
    r = W.ld_blocks(loaded_set, W.henikoff_weights(loaded_set), strong_min, stat, rule, min_sites,
                    max_distance=window[0], max_sites=window[1], ctx=ctx)
    ctx.close()
    head, rows = _read_tsv(blocks)
    assert head == ["block", "first", "last", "sites", "pairs", "informative", "strong", "mean", "min"]
    assert len(rows) == r.n_blocks > 0
    first, last = r.parents()
    for k, row in enumerate(rows):
        assert [int(x) for x in row[:7]] == [k, int(first[k]), int(last[k]), int(r.sites[k]), int(r.pairs[k]),
                                             int(r.informative[k]), int(r.strong[k])], (k, row)
        assert row[7:] == [_fmt3(float(np.float32(r.mean[k]))), _fmt3(float(r.value_min[k]))], (k, row, r.mean[k])
    return r


def _fmt3(x):
    """The pair TSV's number format (Rust's {:.3} of the f32's exact value)."""
    if x != x:
        return "NaN"
    return "%.3f" % x


def test_cli_fasta(W, tmp_path):
    """(a FASTA set's parent coordinate is the column in the unfiltered alignment)"""
    path = os.path.join(SYNTH, "synth_n200_l24.fasta")
    kept = W.read_fasta(path).filter_sites_of_interest(0.8, 0.02, 0.5)
    parent = np.array([kept.parent_site_index(i) for i in range(kept.n_sites())], dtype=np.uint64)
    loaded_set = W.SiteSet.from_buffer(kept.buffer, site_map=parent)
    _cli_case(W, tmp_path, ["--fasta-input", path, "--blocks-r2", "0.001"], loaded_set, 0.001, "r2", "all", 2,
              (None, None))
    _cli_case(W, tmp_path, ["--fasta-input", path, "--blocks-dprime", "0.05", "--blocks-rule", "spine",
                            "--blocks-min-sites", "3"], loaded_set, 0.05, "dprime", "spine", 3, (None, None), pair=False)


def test_cli_vcf_window(W, tmp_path):
    """(VCF input takes no site filter; site index = POS, the window's coordinate)"""
    path = os.path.join(FIXTURES, "t7_1000genome.vcf")
    vcf = W.read_vcf(path)
    r = _cli_case(W, tmp_path, ["--vcf-input", path, "--max-distance", "100", "--max-sites", "3", "--blocks-r2", "0.01",
                                "--devices", "0,0"], vcf, 0.01, "r2", "all", 2, (100, 3))
    assert (r.sites <= 4).all(), "max_sites 3 caps a block at four sites"
