"""LD pruning (wld_run_prune / Context.run_prune / ld_prune / the CLI's
--prune-output): the greedy r2-independent site set with tags, computed on the
device from the row path's rows.

Expected values: sequential greedy selection restated here in numpy (greedy())
on the graph the CPU oracle's dense f32 r2 and `valid` give
(O.all_pairs_dense: edge iff in the window, valid and r2 > threshold) — not
the library's plan.  The result is a discrete function of graph and order, so
keep, tag, n_kept and edges are compared for exact equality.  The edge and
kept counts asserted on the expected values were computed on the CPU with the
oracle.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
from conftest import CLI, REPO, SYNTH

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
    """test_gpu_summary.py's case 1: ld_blocks(600, 203) with a site without
    symbols (site 5: None pairs only), a one-symbol site, and three sites whose
    minor allele sits in few sequences; Henikoff weights."""
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
def chain_case():
    """300 copies of one polymorphic 64-sequence site with a few '-': every
    pair has r2 exactly 1.0 in the oracle."""
    site = np.array([0] * 40 + [2] * 20 + [4] * 4, dtype=np.uint8)
    np.random.default_rng(0xC4A1).shuffle(site)
    buf = np.repeat(site[None, :], 300, axis=0).copy()
    c = Case(buf, _henikoff(buf))
    iu = np.triu_indices(300, 1)
    assert c.valid[iu].all() and (c.r2[iu] == np.float32(1.0)).all()
    return c


def edges_of(case, thr, pos=None, D=0, K=0):
    """The oracle's graph: the pairs a < b in the window with a statistic and r2 > thr."""
    a, b = np.triu_indices(case.L, 1)
    p = np.arange(case.L, dtype=np.int64) if pos is None else np.asarray(pos, dtype=np.int64)
    e = case.valid[a, b] & (case.r2[a, b] > np.float32(thr))
    if D:
        e &= p[b] - p[a] <= D
    if K:
        e &= b - a <= K
    return a[e], b[e]


def greedy(L, ea, eb, priority=None):
    """Sequential greedy selection: visit the sites by priority (larger first,
    ties to the lower index; None: index order), keep a site iff none of its
    neighbours is kept; tag = the kept neighbour that came first."""
    order = np.arange(L) if priority is None else np.argsort(-np.asarray(priority, dtype=np.float32), kind="stable")
    rank = np.empty(L, dtype=np.int64)
    rank[order] = np.arange(L)
    adj = np.zeros((L, L), dtype=bool)
    adj[ea, eb] = True
    adj[eb, ea] = True
    keep = np.zeros(L, dtype=bool)
    tag = np.arange(L, dtype=np.uint32)
    for v in order:
        nb = np.flatnonzero(adj[v] & keep)
        if nb.size:
            tag[v] = nb[np.argmin(rank[nb])]
        else:
            keep[v] = True
    return keep, tag


def assert_pruned(p, L, ea, eb, priority=None, what=""):
    keep, tag = greedy(L, ea, eb, priority)
    assert p.edges == ea.size, (what, p.edges, ea.size)
    assert p.keep.dtype == np.bool_ and p.keep.shape == (L,) and p.tag.dtype == np.uint32 and p.tag.shape == (L,)
    assert np.array_equal(p.keep, keep), (what, np.flatnonzero(p.keep != keep)[:8])
    assert np.array_equal(p.tag, tag), (what, np.flatnonzero(p.tag != tag)[:8])
    assert p.n_kept == int(keep.sum()), what
    assert np.array_equal(p.tag[p.keep], np.flatnonzero(p.keep)), "tag[i] == i for kept sites"
    assert (p.rounds == 0) == (ea.size == 0), (what, p.rounds)
    return keep, tag


def loaded(W, case, pos=None, **kw):
    ctx = W.Context(0, **kw)
    ctx.load(case.buf, case.w, pos)
    return ctx


# ------------------------------------------------------------------ 1. block data
@pytest.mark.parametrize("thr,n_edges,n_kept", [(0.1, 15510, 116), (0.5, 4048, 192)])
def test_block_data(W, thr, n_edges, n_kept):
    c = case1()
    ea, eb = edges_of(c, thr)
    assert ea.size == n_edges
    ctx = loaded(W, c)
    p = ctx.run_prune(thr)
    keep, _ = assert_pruned(p, c.L, ea, eb, what="thr %g" % thr)
    assert int(keep.sum()) == n_kept and p.n_kept == n_kept
    assert not c.valid[5].any() and not c.valid[:, 5].any() and p.keep[5] and p.tag[5] == 5
    assert p.pair_ms > 0 and p.prune_ms > 0
    assert sum(ctx.prune_times()) <= p.prune_ms * 1.001 + 1e-3
    # the same context again: the same set
    q = ctx.run_prune(thr)
    assert np.array_equal(q.keep, p.keep) and np.array_equal(q.tag, p.tag) and q.edges == p.edges
    ctx.close()


# ------------------------------------------------------------------ 2. ties
def test_ties(W):
    c = case1()
    pr = np.random.default_rng(0x71E5).integers(0, 8, 600).astype(np.float32)
    ea, eb = edges_of(c, 0.2)
    ctx = loaded(W, c)
    p = ctx.run_prune(0.2, pr)
    keep, _ = assert_pruned(p, c.L, ea, eb, pr, "ties")
    keep0, _ = greedy(c.L, ea, eb)
    assert not np.array_equal(keep, keep0), "the priority must change the set"
    # -0.0 == 0.0 and +-inf: still the lower index among equals, inf first
    pr2 = pr.copy()
    pr2[pr2 == 3] = -0.0
    pr2[pr2 == 4] = 0.0
    pr2[10], pr2[400], pr2[77] = np.inf, np.inf, -np.inf
    assert_pruned(ctx.run_prune(0.2, pr2), c.L, ea, eb, pr2, "signed zeros and infinities")
    ctx.close()


# ------------------------------------------------------------------ 3. windows
@pytest.mark.parametrize("D,K,n_edges", [(60, 0, 5955), (0, 37, 5417)], ids=["dist60_map", "sites37"])
def test_windows(W, D, K, n_edges):
    c = case1()
    pos = case1_map() if D else None
    ea, eb = edges_of(c, 0.2, pos, D, K)
    assert ea.size == n_edges
    ctx = loaded(W, c, pos)
    ctx.set_window(D, K)
    p = ctx.run_prune(0.2)
    assert_pruned(p, c.L, ea, eb, what="window D=%d K=%d" % (D, K))  # (keep, tag: loaded indices)
    assert p.tag.max() < c.L
    ctx.close()


# ------------------------------------------------------------------ 4. dependency chain
def test_dependency_chain(W):
    c = chain_case()
    L = c.L
    ctx = loaded(W, c)
    # a path across the chunk boundary at 256: a synchronous schedule needs 300 rounds
    ctx.set_window(0, 1)
    ea, eb = edges_of(c, 0.5, K=1)
    assert ea.size == L - 1
    p = ctx.run_prune(0.5)
    assert_pruned(p, L, ea, eb, what="path")
    idx = np.arange(L)
    assert np.array_equal(p.keep, idx % 2 == 0) and np.array_equal(p.tag[1::2], idx[1::2] - 1)
    print("path of %d: %d rounds" % (L, p.rounds))
    ctx.set_window(0, 2)
    ea, eb = edges_of(c, 0.5, K=2)
    p = ctx.run_prune(0.5)
    assert_pruned(p, L, ea, eb, what="max_sites 2")
    assert np.array_equal(np.flatnonzero(p.keep), idx[::3])
    # no window: a clique; the site of the largest priority stands for all
    ctx.set_window(0, 0)
    ea, eb = edges_of(c, 0.5)
    assert ea.size == L * (L - 1) // 2
    pr = np.zeros(L, dtype=np.float32)
    pr[137] = 1.0
    p = ctx.run_prune(0.5, pr)
    assert_pruned(p, L, ea, eb, pr, "clique")
    assert np.array_equal(np.flatnonzero(p.keep), [137]) and (p.tag == 137).all()
    ctx.close()


# ------------------------------------------------------------------ 5. shapes
@pytest.mark.parametrize("N", [5, 64, 203])
def test_shapes(W, N):
    """130 sites (not a multiple of 64); N = 5 takes the row path's tail-only sums."""
    c = shape_case(N)
    ea, eb = edges_of(c, 0.05)
    ctx = loaded(W, c)
    p = ctx.run_prune(0.05)
    assert_pruned(p, c.L, ea, eb, what="N=%d" % N)
    if N == 64:
        assert (p.edges, p.n_kept) == (900, 25)
    ctx.close()


# ------------------------------------------------------------------ 6. batching
def test_batches_and_staging_regrowth(W):
    c = case1()
    ea, eb = edges_of(c, 0.2)
    ref = loaded(W, c)
    want = ref.run_prune(0.2)
    assert_pruned(want, c.L, ea, eb, what="default")
    ctx = W.Context(0)
    ctx.set_option("host_batch_pairs", 20000)
    ctx.set_option("staging_rows", 64)
    ctx.load(c.buf, c.w)
    assert W.Context.pairs_in_chunks(c.L, 0, W.Context.chunks(c.L)) > 3 * 20000, "several batches"
    p = ctx.run_prune(0.2)
    assert p.edges == want.edges and p.n_kept == want.n_kept
    assert np.array_equal(p.keep, want.keep) and np.array_equal(p.tag, want.tag)
    ref.close()
    ctx.close()


# ------------------------------------------------------------------ 7. other row paths
@pytest.mark.parametrize("kind", ["valu", "mfma", "exact_sums"])
def test_other_row_paths(W, kind):
    """The graph is the context's own rows (identity map: loaded indices), not the oracle's."""
    c = case1()
    kw = {"valu": dict(kernel=W.KERNEL_VALU), "mfma": dict(kernel=W.KERNEL_MFMA), "exact_sums": dict(ref_sums=False)}[kind]
    ctx = loaded(W, c, **kw)
    rows = ctx.run_host(0.2)
    assert len(rows) > 1000
    ea, eb = rows.site_a.astype(np.int64), rows.site_b.astype(np.int64)
    p = ctx.run_prune(0.2)
    assert_pruned(p, c.L, ea, eb, what=kind)
    ctx.close()


# ------------------------------------------------------------------ 8. no leak into the row path
def _host_rows(ctx, thr):
    r = ctx.run_host(thr)
    return [r.site_a, r.site_b, r.d.view(np.uint32), r.d_prime.view(np.uint32), r.r2.view(np.uint32)]


def test_no_leak_into_the_row_path(W):
    c = case1()
    pos = (case1_map() * 3 + 11).astype(np.uint64)  # not the identity
    fresh, ctx = loaded(W, c, pos), loaded(W, c, pos)
    assert ctx.run(0.2) > 0 and len(ctx.rows()) > 0  # rows before the prune: gone after it
    ea, eb = edges_of(c, 0.2)
    assert_pruned(ctx.run_prune(0.2), c.L, ea, eb, what="with a map")
    a = np.zeros(ea.size, dtype=np.uint32)
    st = W.lib().wld_rows_copy(ctx._h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None, None, None, None)
    assert st == -7, "wld_rows_copy after a prune: WLD_E_STATE"
    with pytest.raises(W.WldError) as ei:
        ctx.rows()
    assert ei.value.name == "WLD_E_STATE"
    got, want = _host_rows(ctx, 0.2), _host_rows(fresh, 0.2)
    assert len(want[0]) == ea.size
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
    assert set(zip(got[0].tolist(), got[1].tolist())) == set(zip(pos[ea].tolist(), pos[eb].tolist())), "parent indices"
    # ... and the staged run's rows as well
    n = ctx.run(0.2)
    r = ctx.rows()
    assert n == ea.size and np.array_equal(r.site_a, want[0]) and np.array_equal(r.site_b, want[1])
    fresh.close()
    ctx.close()


# ------------------------------------------------------------------ 9. edge cases and errors
def test_edge_cases_and_errors(W):
    c = case1()
    ctx = W.Context(0)
    with pytest.raises(W.WldError) as ei:
        ctx.run_prune(0.2)
    assert ei.value.name == "WLD_E_STATE"  # before a load
    ctx.load(c.buf, c.w)
    p = ctx.run_prune(2.0)  # no r2 exceeds 2: no edge
    assert (p.edges, p.n_kept, p.rounds) == (0, c.L, 0) and p.keep.all() and np.array_equal(p.tag, np.arange(c.L))
    pr = np.zeros(c.L, dtype=np.float32)
    pr[17] = pr[400] = np.nan
    with pytest.raises(W.WldError) as ei:
        ctx.run_prune(0.2, pr)
    assert ei.value.name == "WLD_E_ARG" and "priority[17]" in str(ei.value)
    with pytest.raises(ValueError):
        ctx.run_prune(0.2, pr[:10])
    ctx.run_chunks_async(0.2)
    with pytest.raises(W.WldError) as ei:
        ctx.run_prune(0.2)
    assert ei.value.name == "WLD_E_STATE"  # a run in flight
    ctx.run_wait()
    ea, eb = edges_of(c, 0.2)
    assert_pruned(ctx.run_prune(0.2), c.L, ea, eb, what="after the refusals")
    # one site
    ctx.load(c.buf[:1], c.w)
    p = ctx.run_prune(0.0)
    assert (p.edges, p.n_kept, p.rounds) == (0, 1, 0) and p.keep.tolist() == [True] and p.tag.tolist() == [0]
    ctx.close()
    grp = W.Context(devices=[0, 0])
    grp.load(c.buf, c.w)
    with pytest.raises(W.WldError) as ei:
        grp.run_prune(0.2)
    assert ei.value.name == "WLD_E_STATE"
    grp.close()


# ------------------------------------------------------------------ 10. Python and CLI
def _maf(buf):
    """minor / (major + minor) of the oracle's major and minor symbols, in double, as float32."""
    out = np.zeros(buf.shape[0], dtype=np.float32)
    for i in range(buf.shape[0]):
        h = O.histogram(buf[i])
        major, minor = O.major_minor(h)
        if major is not None and minor is not None:
            out[i] = np.float32(float(h[minor]) / (float(h[major]) + float(h[minor])))
    return out


def test_ld_prune_maf(W):
    c = case1()
    pos = case1_map()
    pr = _maf(c.buf)
    assert np.unique(pr).size > 10 and pr[5] == 0.0
    ea, eb = edges_of(c, 0.2, pos, 0, 37)
    ss = W.SiteSet.from_buffer(c.buf, site_map=pos)
    assert np.array_equal(W.maf_priority(ss), pr)
    ctx = W.Context(0)
    ctx.set_window(0, 5)
    p = W.ld_prune(ss, c.w, 0.2, priority="maf", max_sites=37, ctx=ctx)
    assert ctx.window() == (0, 5), "the context's own window is restored"
    keep, _ = assert_pruned(p, c.L, ea, eb, pr, "ld_prune maf")
    assert np.array_equal(p.kept_sites, pos[np.flatnonzero(keep)])
    assert not np.array_equal(keep, greedy(c.L, ea, eb)[0])
    # an array priority, no window
    pr2 = np.random.default_rng(3).random(c.L).astype(np.float32)
    ea, eb = edges_of(c, 0.2)
    ctx.set_window(0, 0)
    assert_pruned(W.ld_prune(ss, c.w, 0.2, priority=pr2, ctx=ctx), c.L, ea, eb, pr2, "ld_prune array")
    ctx.close()


def _cli_expected(W, path, thr, maf, K):
    ss = W.read_fasta(path).filter_sites_of_interest(0.8, 0.02, 0.5)
    buf = ss.buffer
    c = Case(buf, O.henikoff_weights(buf))
    ea, eb = edges_of(c, thr, K=K)
    keep, tag = greedy(c.L, ea, eb, _maf(buf) if maf else None)
    parent = [ss.parent_site_index(i) for i in range(c.L)]
    assert 0 < keep.sum() < c.L, "kept and removed sites"
    return ["site\tkept\ttag"] + ["%d\t%d\t%d" % (parent[i], keep[i], parent[tag[i]]) for i in range(c.L)]


@pytest.mark.parametrize("maf,K", [(False, 0), (True, 9)], ids=["index", "maf_sites9"])
def test_cli(W, tmp_path, maf, K):
    path = os.path.join(SYNTH, "synth_n500_l40.fasta")
    want = _cli_expected(W, path, 0.004, maf, K)
    out, pairs = str(tmp_path / "prune.tsv"), str(tmp_path / "pairs.tsv")
    cmd = [CLI, "--fasta-input", path, "--pair-output", pairs, "--prune-output", out, "--prune-r2", "0.004"]
    if maf:
        cmd += ["--prune-priority", "maf", "--max-sites", str(K)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    with open(out) as f:
        assert f.read().split("\n") == want + [""]


def test_cli_missing_flags(tmp_path):
    base = [CLI, "--fasta-input", os.path.join(SYNTH, "synth_n200_l24.fasta"), "--pair-output", str(tmp_path / "p.tsv")]
    for extra, needle in ((["--prune-output", str(tmp_path / "x.tsv")], "--prune-r2 <prune-r2>"),
                          (["--prune-r2", "0.2"], "--prune-output <prune-output>"),
                          (["--prune-output", str(tmp_path / "x.tsv"), "--prune-r2", "0.2", "--prune-priority", "mad"],
                           "--prune-priority")):
        res = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert res.returncode == 1 and res.stderr.startswith("error:") and needle in res.stderr, res.stderr
        assert not os.path.exists(str(tmp_path / "x.tsv")) and not os.path.exists(str(tmp_path / "p.tsv"))
