"""Target-site LD (wld_run_targets / Context.run_targets / ld_targets / the CLI's
--ld-sites*): the rows of chosen sites against every in-window partner.

Expected values come from the CPU oracle: O.all_pairs_dense, entry (min, max)
of target and partner.  A row exists iff the pair is in the window, the oracle
has a statistic (valid) and r2 > threshold strictly; rows come by list position,
then partner ascending.  d, d' and r2 are compared as uint32 views: bit for bit.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
from conftest import CLI, FIXTURES, REPO

pytestmark = pytest.mark.gpu

TARGETS_A = [63, 64, 0, 599, 5, 300, 129, 255, 256, 470]  # (unsorted: list order is not loaded order)


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
        self.buf, self.w = buf, np.ascontiguousarray(w, dtype=np.float32)
        self.L = buf.shape[0]
        self.d, self.dp, self.r2, valid = O.all_pairs_dense(buf, self.w)
        self.valid = valid != 0
        for a in (self.buf, self.w, self.d, self.dp, self.r2, self.valid):
            a.setflags(write=False)


def _set_a_buf():
    buf = _bench().ld_blocks(600, 203).copy()
    buf[5, :] = 0
    buf[300, :] = 4
    buf[64, :100] = 5
    buf[470, 100:] = 5
    buf[129, 3:] = 5
    return buf


@functools.lru_cache(maxsize=None)
def set_a():
    """Set A: ld_blocks(600, 203) with a site without symbols, a one-symbol
    site and three sites whose minor allele sits in few sequences; Henikoff
    weights.  10 tiles and 3 chunk rows a side, a 3-sequence tail and a partial
    stage."""
    buf = _set_a_buf()
    return Case(buf, _henikoff(buf))


@functools.lru_cache(maxsize=None)
def set_a_unit():
    buf = _set_a_buf()
    return Case(buf, np.ones(buf.shape[1], dtype=np.float32))


@functools.lru_cache(maxsize=None)
def set_a_wide():
    """weights spanning 2^-20 .. 1"""
    buf = _set_a_buf()
    rng = np.random.default_rng(0x7A6)
    w = np.exp2(-rng.integers(0, 21, size=buf.shape[1]).astype(np.float64)).astype(np.float32)
    w[0], w[1] = 1.0, 2.0 ** -20
    return Case(buf, w)


@functools.lru_cache(maxsize=None)
def map_a():
    """POS with repeats: a cumulative sum of steps 0..3."""
    rng = np.random.default_rng(0x5117)
    m = np.cumsum(rng.integers(0, 4, size=600)).astype(np.uint64)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def shape_case(N):
    buf = _bench().synth(130, N, seed=0x130 + N)
    return Case(buf, _henikoff(buf))


def window_matrix(L, pos=None, D=0, K=0):
    """in_window[s, t] for s != t, symmetric (the window is symmetric about a target)."""
    i = np.arange(L, dtype=np.int64)
    p = i if pos is None else np.asarray(pos, dtype=np.int64)
    m = i[:, None] != i[None, :]
    if D:
        m &= np.abs(p[:, None] - p[None, :]) <= D
    if K:
        m &= np.abs(i[:, None] - i[None, :]) <= K
    return m


def expected(case, targets, thr, pos=None, D=0, K=0):
    """The contract restated on the oracle's dense matrices."""
    L = case.L
    win = window_matrix(L, pos, D, K)
    parent = np.arange(L, dtype=np.uint32) if pos is None else np.asarray(pos).astype(np.uint32)
    s = np.arange(L)
    cols = {k: [] for k in ("target", "site_target", "site_partner", "partner", "d", "d_prime", "r2")}
    offset = [0]
    for k, t in enumerate(targets):
        a, b = np.minimum(s, t), np.maximum(s, t)
        with np.errstate(invalid="ignore"):
            keep = win[s, t] & case.valid[a, b] & (case.r2[a, b] > np.float32(thr))
        sk = s[keep]
        ak, bk = a[keep], b[keep]
        cols["target"].append(np.full(sk.size, k, dtype=np.uint32))
        cols["site_target"].append(np.full(sk.size, parent[t], dtype=np.uint32))
        cols["site_partner"].append(parent[sk])
        cols["partner"].append(sk.astype(np.uint32))
        cols["d"].append(case.d[ak, bk])
        cols["d_prime"].append(case.dp[ak, bk])
        cols["r2"].append(case.r2[ak, bk])
        offset.append(offset[-1] + sk.size)
    out = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in cols.items()}
    out["offset"] = np.asarray(offset, dtype=np.uint64)
    return out


def assert_rows(got, want, what=""):
    assert len(got) == int(want["offset"][-1]), what
    assert np.array_equal(got.offset, want["offset"]), what
    for f in ("target", "site_target", "site_partner"):
        assert np.array_equal(getattr(got, f).astype(np.uint64), want[f].astype(np.uint64)), (what, f)
    for f in ("d", "d_prime", "r2"):
        g, r = getattr(got, f), np.ascontiguousarray(want[f], dtype=np.float32)
        assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), (what, f)


def same_rows(x, y):
    return (np.array_equal(x.offset, y.offset) and
            all(np.array_equal(getattr(x, f).view(np.uint32), getattr(y, f).view(np.uint32))
                for f in ("target", "site_target", "site_partner", "d", "d_prime", "r2")) and x.items == y.items)


@pytest.fixture(scope="module")
def ctx_a(W):
    ctx = W.Context(0)
    c = set_a()
    ctx.load(c.buf, c.w)
    yield ctx
    ctx.close()


# ------------------------------------------------------------------ oracle preconditions
def test_oracle_preconditions():
    c = set_a()
    table = {(0, -1.0): (0, 596), (599, -1.0): (596, 0), (5, -1.0): (0, 0), (300, -1.0): (0, 0),
             (63, 0.2): (37, 44), (64, 0.2): (41, 49), (470, 0.2): (16, 25), (255, 0.2): (1, 9), (256, 0.2): (1, 23),
             (129, 0.2): (74, 249)}
    for (t, thr), (below, above) in table.items():
        e = expected(c, [t], thr)
        assert (int((e["partner"] < t).sum()), int((e["partner"] > t).sum())) == (below, above), (t, thr)
    # the statistic is not symmetric in its arguments: with the roles swapped
    # the oracle's bits differ for at least one row below a target
    differs = 0
    for t in (63, 64, 129, 470):
        e = expected(c, [t], 0.2)
        for s in e["partner"][e["partner"] < t].tolist():
            sw = np.asarray(O.single_pair(c.buf[t], c.buf[s], c.w), dtype=np.float32)
            dense = np.asarray([c.d[s, t], c.dp[s, t], c.r2[s, t]], dtype=np.float32)
            differs += not np.array_equal(sw.view(np.uint32), dense.view(np.uint32))
    assert differs > 0


# ------------------------------------------------------------------ 1. both sides, bit exact
@pytest.mark.parametrize("thr", [-1.0, 0.0, 0.2])
def test_both_sides_bit_exact(ctx_a, thr):
    got = ctx_a.run_targets(TARGETS_A, thr)
    assert_rows(got, expected(set_a(), TARGETS_A, thr), "thr %g" % thr)
    assert got.batches == 1 and got.kernel_ms >= 0.0


# ------------------------------------------------------------------ 2. equal to the row path
@pytest.mark.parametrize("thr", [0.2, -1.0])
def test_equal_to_row_path(W, thr):
    c, pos = set_a(), map_a()
    ctx = W.Context(0)
    ctx.load(c.buf, c.w)
    plain = ctx.run_host(thr)  # loaded indices: the row order does not depend on the map
    ctx.load(c.buf, c.w, pos)
    rows = ctx.run_host(thr)
    a, b = plain.site_a.astype(np.int64), plain.site_b.astype(np.int64)
    assert np.array_equal(rows.site_a.astype(np.uint64), pos[a]) and np.array_equal(rows.site_b.astype(np.uint64), pos[b])
    got = ctx.run_targets(TARGETS_A, thr)
    ctx.close()
    at = 0
    for k, t in enumerate(TARGETS_A):
        sel = np.flatnonzero((a == t) | (b == t))
        partner = np.where(a[sel] == t, b[sel], a[sel])
        sel = sel[np.argsort(partner, kind="stable")]
        partner = np.sort(partner)
        n = sel.size
        assert int(got.offset[k]) == at and int(got.offset[k + 1]) == at + n
        sl = slice(at, at + n)
        assert np.all(got.target[sl] == k) and np.all(got.site_target[sl] == pos[t])
        assert np.array_equal(got.site_partner[sl].astype(np.uint64), pos[partner])
        for f in ("d", "d_prime", "r2"):
            assert np.array_equal(getattr(got, f)[sl].view(np.uint32), getattr(rows, f)[sel].view(np.uint32)), (t, f)
        at += n
    assert len(got) == at


# ------------------------------------------------------------------ 3. shapes
@pytest.mark.parametrize("N", [5, 8, 64, 203, 520])
def test_shapes(W, N):
    """tail only; no tail; one stage; tail plus a partial stage; several stages per class"""
    c = shape_case(N)
    ctx = W.Context(0)
    ctx.load(c.buf, c.w)
    t = [0, 15, 16, 64, 129]
    got = ctx.run_targets(t, -1.0)
    ctx.close()
    assert_rows(got, expected(c, t, -1.0), "N %d" % N)
    assert len(got) > 0


# ------------------------------------------------------------------ 4. tiny sets
@pytest.mark.parametrize("L", [1, 2, 65])
def test_tiny_sets(W, L):
    buf = _bench().synth(L, 37, seed=0x717 + L)
    c = Case(buf, _henikoff(buf))
    ctx = W.Context(0)
    ctx.load(c.buf, c.w)
    t = list(range(L))[::-1]
    got = ctx.run_targets(t, -1.0)
    ctx.close()
    assert_rows(got, expected(c, t, -1.0), "L %d" % L)
    if L == 1:
        assert len(got) == 0 and got.items == 0


# ------------------------------------------------------------------ 5. target counts
@pytest.mark.parametrize("Q", [1, 16, 17, 33])
def test_target_counts(ctx_a, Q):
    rng = np.random.default_rng(0x9 + Q)
    t = rng.permutation(600)[:Q].tolist()
    got = ctx_a.run_targets(t, 0.2)
    assert_rows(got, expected(set_a(), t, 0.2), "Q %d" % Q)


def test_all_sites_as_targets(ctx_a):
    t = list(range(600))
    got = ctx_a.run_targets(t, 0.2)
    assert_rows(got, expected(set_a(), t, 0.2), "all sites")
    rows = ctx_a.run_host(0.2)
    assert len(got) == 2 * len(rows)
    a, b = rows.site_a.astype(np.int64), rows.site_b.astype(np.int64)
    both = np.concatenate([a * 600 + b, b * 600 + a])
    mine = got.site_target.astype(np.int64) * 600 + got.site_partner.astype(np.int64)
    assert np.array_equal(np.sort(both), np.sort(mine)) and np.unique(mine).size == mine.size


# ------------------------------------------------------------------ 6. windows
def items_restated(L, targets, win):
    """Blocks of 16 targets in loaded order x 64-site tiles holding an
    in-window partner of a target of the block."""
    st = np.sort(np.asarray(targets))
    n = 0
    for b0 in range(0, st.size, 16):
        blk = st[b0:b0 + 16]
        for t0 in range(0, L, 64):
            n += bool(win[t0:min(L, t0 + 64)][:, blk].any())
    return n


@pytest.mark.parametrize("use_map,D,K", [(False, 0, 70), (True, 100, 0), (True, 100, 50)])
def test_windows(W, use_map, D, K):
    c = set_a()
    pos = map_a() if use_map else None
    ctx = W.Context(0)
    ctx.load(c.buf, c.w, pos)
    # two blocks in the set's first two thirds (a list spread over the whole
    # set reaches every tile under any window), both sides of every target
    t = [63, 64, 129, 300, 320, 5] + list(range(250, 264))
    free = ctx.run_targets(t, -1.0)
    ctx.set_window(D or None, K or None)
    got = ctx.run_targets(t, -1.0)
    got2 = ctx.run_targets(t, 0.2)
    ctx.close()
    assert_rows(got, expected(c, t, -1.0, pos, D, K), "window")
    assert_rows(got2, expected(c, t, 0.2, pos, D, K), "window, thr 0.2")
    assert got.items == items_restated(600, t, window_matrix(600, pos, D, K))
    assert free.items == items_restated(600, t, window_matrix(600))
    assert got.items < free.items and len(got) < len(free)


# ------------------------------------------------------------------ 7. batches
def test_batches(W):
    c = set_a()
    rng = np.random.default_rng(0xBA7)
    t = rng.permutation(600)[:33].tolist()
    ctx = W.Context(0)
    ctx.load(c.buf, c.w)
    one = ctx.run_targets(t, 0.0)
    ctx.set_option("target_batch_slots", 1)
    assert ctx.get_option("target_batch_slots") == 1
    many = ctx.run_targets(t, 0.0)
    ctx.close()
    assert one.batches == 1 and many.batches >= 3
    assert same_rows(one, many)
    assert_rows(many, expected(c, t, 0.0), "three batches")


# ------------------------------------------------------------------ 8. weights
@pytest.mark.parametrize("which", ["unit", "wide"])
def test_weights(W, which):
    c = set_a_unit() if which == "unit" else set_a_wide()
    ctx = W.Context(0)
    ctx.load(c.buf, c.w)
    if which == "wide":
        assert ctx.stats()["kernel"] == W.KERNEL_VALU  # (the range does not fit the fixed-point planes)
    for thr in (-1.0, 0.2):
        assert_rows(ctx.run_targets(TARGETS_A, thr), expected(c, TARGETS_A, thr), "%s thr %g" % (which, thr))
    ctx.close()


# ------------------------------------------------------------------ 9. rows undisturbed
def test_rows_undisturbed(W):
    c = set_a()
    ctx = W.Context(0)
    ctx.load(c.buf, c.w)
    n = ctx.run(0.2)
    before, st = ctx.rows(), ctx.stats()
    ctx.run_targets(TARGETS_A, 0.0)
    after = ctx.rows()
    assert ctx.stats() == st and len(after) == n
    for f in ("site_a", "site_b", "d", "d_prime", "r2"):
        assert np.array_equal(getattr(before, f).view(np.uint32), getattr(after, f).view(np.uint32)), f
    assert ctx.run(0.2) == n
    again = ctx.rows()
    for f in ("site_a", "site_b", "d", "d_prime", "r2"):
        assert np.array_equal(getattr(before, f).view(np.uint32), getattr(again, f).view(np.uint32)), f
    ctx.close()


# ------------------------------------------------------------------ 10. errors
def test_errors(W):
    import ctypes
    from weightedld_amd import _lib
    c = set_a()
    ctx = W.Context(0)

    def refused(name, targets, on=None):
        with pytest.raises(W.WldError) as e:
            (on or ctx).run_targets(targets, 0.2)
        assert e.value.name == name, str(e.value)
        return str(e.value)

    refused("WLD_E_STATE", [1])  # before a load
    ctx.load(c.buf, c.w)
    assert "targets[2]" in refused("WLD_E_ARG", [3, 4, 600, 700])
    assert "targets[3]" in refused("WLD_E_ARG", [3, 4, 5, 4, 4])
    assert "targets[1]" in refused("WLD_E_ARG", [3, 3, 600])  # the first offending position, whatever its kind
    out = _lib.TargetRowsC()
    assert _lib.lib().wld_run_targets(ctx._h, None, 3, 0.2, ctypes.byref(out)) == -1  # WLD_E_ARG
    empty = ctx.run_targets([], 0.2)
    assert len(empty) == 0 and empty.offset.tolist() == [0] and empty.items == 0
    ctx.run_chunks_async(0.2)
    refused("WLD_E_STATE", [1])  # a run in flight
    ctx.run_wait()
    w = c.w.copy()
    w[7] = np.inf
    ctx.load(c.buf, w)
    assert "finite weights" in refused("WLD_E_ARG", [1])
    # n_targets x (L - 1) past 2^32 - 1
    big = _bench().synth(66000, 8, seed=0xB16)
    ctx.load(big, np.ones(8, dtype=np.float32))
    assert "split the list" in refused("WLD_E_ARG", np.arange(65100))
    got = ctx.run_targets([65999], 0.9)  # (the same load is usable)
    assert got.offset.size == 2
    grp = W.Context(devices=[0, 0])
    grp.load(c.buf, c.w)
    refused("WLD_E_STATE", [1], on=grp)
    grp.close()
    ctx.load(c.buf, c.w)
    assert_rows(ctx.run_targets(TARGETS_A, 0.2), expected(c, TARGETS_A, 0.2), "after every refusal")
    ctx.close()


# ------------------------------------------------------------------ 11. ld_targets
def test_ld_targets(W):
    c, pos = set_a(), map_a()
    ss = W.SiteSet.from_buffer(c.buf, pos)
    ctx = W.Context(0)
    # a coordinate several sites carry: all of them, in loaded order
    vals, counts = np.unique(pos, return_counts=True)
    rep = int(vals[np.argmax(counts >= 2)])
    single = int(vals[np.argmax(counts == 1)])
    want_t = np.flatnonzero(pos == single).tolist() + np.flatnonzero(pos == rep).tolist()
    assert len(want_t) >= 3
    got = W.ld_targets(ss, c.w, 0.2, parents=[single, rep], ctx=ctx)
    assert got.targets.tolist() == want_t
    assert_rows(got, expected(c, want_t, 0.2, pos), "parents")
    got = W.ld_targets(ss, c.w, 0.2, targets=[64, 63], max_sites=70, ctx=ctx)
    assert_rows(got, expected(c, [64, 63], 0.2, pos, 0, 70), "targets under a window")
    assert ctx.window() == (0, 0)
    absent = int(pos.max()) + 5
    with pytest.raises(ValueError, match=str(absent)):
        W.ld_targets(ss, c.w, 0.2, parents=[single, absent], ctx=ctx)
    with pytest.raises(ValueError):
        W.ld_targets(ss, c.w, 0.2, targets=[1], parents=[single], ctx=ctx)
    with pytest.raises(ValueError):
        W.ld_targets(ss, c.w, 0.2, ctx=ctx)
    ctx.close()


# ------------------------------------------------------------------ 12. CLI
def _fmt3(x):
    x = float(x)
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    return "%.3f" % x


def _tsv_lines(rows):
    return ["target\tsite\td\td'\tr2"] + [
        "%d\t%d\t%s\t%s\t%s" % (a, b, _fmt3(d), _fmt3(dp), _fmt3(r2))
        for a, b, d, dp, r2 in zip(rows.site_target.tolist(), rows.site_partner.tolist(), rows.d, rows.d_prime, rows.r2)]


def test_cli_fasta(W, tmp_path):
    path = os.path.join(FIXTURES, "example.fasta")
    loaded = W.read_fasta(path).filter_sites_of_interest(0.8, 0.02, 0.5)
    L = loaded.n_sites()
    assert L >= 2
    coords = [loaded.parent_site_index(L - 1), loaded.parent_site_index(0)]  # (not in loaded order)
    ctx = W.Context(0)
    want = W.ld_targets(loaded, W.henikoff_weights(loaded), -1.0, parents=coords, ctx=ctx)
    want_pair = W.ld_targets(loaded, W.henikoff_weights(loaded), 0.1, parents=coords, ctx=ctx)
    ctx.close()
    assert len(want) > 0
    out, listf = str(tmp_path / "t.tsv"), str(tmp_path / "sites.txt")
    with open(listf, "w") as f:
        f.write("\n%d\n" % coords[1])
    # without --pair-output: the list, then the file; its own threshold
    res = subprocess.run([CLI, "--fasta-input", path, "--ld-sites", str(coords[0]), "--ld-sites-file", listf,
                          "--ld-sites-output", out, "--ld-sites-r2=-1"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "target sites" in res.stderr
    with open(out) as f:
        assert f.read().split("\n") == _tsv_lines(want) + [""]
    # with --pair-output; the threshold defaults to --r2-threshold's
    pairs = str(tmp_path / "p.tsv")
    res = subprocess.run([CLI, "--fasta-input", path, "--pair-output", pairs, "--ld-sites",
                          ",".join(str(x) for x in coords), "--ld-sites-output", out],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    with open(out) as f:
        assert f.read().split("\n") == _tsv_lines(want_pair) + [""]
    assert os.path.getsize(pairs) > 0


def test_cli_vcf_window(W, tmp_path):
    """(VCF input takes no site filter; site index = POS, the window's coordinate)"""
    path = os.path.join(FIXTURES, "t7_1000genome.vcf")
    vcf = W.read_vcf(path)
    L = vcf.n_sites()
    coords = sorted({vcf.parent_site_index(i) for i in (0, L // 3, L - 1)})
    ctx = W.Context(0)
    w = W.henikoff_weights(vcf)
    want = W.ld_targets(vcf, w, -1.0, parents=coords, max_distance=100, ctx=ctx)
    free = W.ld_targets(vcf, w, -1.0, parents=coords, ctx=ctx)
    ctx.close()
    assert 0 < len(want) < len(free), "the window must cut rows"
    out = str(tmp_path / "t.tsv")
    res = subprocess.run([CLI, "--vcf-input", path, "--ld-sites", ",".join(str(x) for x in coords),
                          "--ld-sites-output", out, "--ld-sites-r2=-1", "--max-distance", "100"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    with open(out) as f:
        assert f.read().split("\n") == _tsv_lines(want) + [""]


def test_cli_errors(W, tmp_path):
    path = os.path.join(FIXTURES, "example.fasta")
    loaded = W.read_fasta(path).filter_sites_of_interest(0.8, 0.02, 0.5)
    known = loaded.parent_site_index(0)
    absent = max(loaded.parent_site_index(i) for i in range(loaded.n_sites())) + 7
    out = str(tmp_path / "t.tsv")
    res = subprocess.run([CLI, "--fasta-input", path, "--ld-sites", "%d,%d" % (known, absent), "--ld-sites-output", out],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and str(absent) in res.stderr and not os.path.exists(out), res.stderr
    for extra, needle in ((["--ld-sites", str(known)], "--ld-sites-output <ld-sites-output>"),
                          (["--ld-sites-output", out], "--ld-sites <ld-sites>"),
                          (["--ld-sites", str(known), "--ld-sites-output", out, "--devices", "2"], "--devices")):
        res = subprocess.run([CLI, "--fasta-input", path, "--pair-output", str(tmp_path / "p.tsv"), *extra],
                             capture_output=True, text=True, timeout=60)
        assert res.returncode == 1 and res.stderr.startswith("error:") and needle in res.stderr, res.stderr
        assert not os.path.exists(out)
