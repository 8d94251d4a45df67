"""The window (wld_set_window: max_distance D in parent coordinates, max_sites K
in loaded sites): a windowed run gives exactly the rows of the same run
without a window whose pair a < b is in the window,
    (D == 0 or pos[b] - pos[a] <= D) and (K == 0 or b - a <= K),
in the same order with the same parent indices and the same bits, on every
row-emitting kernel path; its stats, progress, batches and shards count
in-window pairs.  Expected rows: the CPU oracle's (loaded indices), filtered
in numpy by the predicate.  Every row-comparing case asserts that the oracle
has rows on both sides of the window, so the mask is exercised.

The exact-sum paths (WLD_OPT_REF_SUMS 0) are not the oracle's arithmetic (the
suite holds them to 1e-5 of it, not to its bits: at 700 x 200 their unwindowed
rows are the oracle's pairs, with r2 differing in the last bits in 213,521 of
244,650 rows at threshold 0 and 20,752 of 24,830 at 0.05, measured on MI355X),
so their expected rows are their own unwindowed run's, filtered the same way,
bit for bit; the paths in lib.rs's order are held to the oracle's bits.
"""
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

import _oracle as O
from conftest import CLI, FIXTURES, REPO, SYNTH

pytestmark = pytest.mark.gpu

FIELDS = ("d", "d_prime", "r2")


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


@functools.lru_cache(maxsize=None)
def data(kind, L, N):
    """(buffer, Henikoff weights) of bench.synth / bench.ld_blocks, built once."""
    import weightedld_amd as W
    buf = getattr(_bench(), kind)(L, N)
    buf.setflags(write=False)
    w = W.henikoff_weights(W.SiteSet.from_buffer(buf))
    w.setflags(write=False)
    return buf, w


@functools.lru_cache(maxsize=None)
def oracle(kind, L, N, thr):
    """The oracle's rows in LOADED indices (no site_map), computed once and left unchanged."""
    buf, w = data(kind, L, N)
    ref = O.all_pairs(buf, w, np.float32(thr))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def in_window(a, b, pos, D, K):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    p = np.arange(0) if pos is None else np.asarray(pos, dtype=np.int64)
    dist = (b - a) if pos is None else (p[b] - p[a])
    return ((D == 0) | (dist <= D)) & ((K == 0) | (b - a <= K))


def window_matrix(L, pos, D, K):
    """[L, L] bool: pair (a, b), a < b, is in the window."""
    a, b = np.triu_indices(L, 1)
    m = np.zeros((L, L), dtype=bool)
    m[a, b] = in_window(a, b, pos, D, K)
    return m


def blocks_any(m, side):
    """per side x side block of m: the in-window pairs it holds"""
    L = m.shape[0]
    P = (L + side - 1) // side * side
    q = np.zeros((P, P), dtype=np.int64)
    q[:L, :L] = m
    return q.reshape(P // side, side, P // side, side).sum(axis=(1, 3))


def chunk_counts(m):
    """in-window pairs per chunk in linear (triu_index) order"""
    c = blocks_any(m, 256)
    n = c.shape[0]
    out = []
    for i in range(n * (n + 1) // 2):
        row, col = O.triu_index(n, i)
        out.append(int(c[row, col]))
    return out


def expected(ref, pos, D, K, need_both=True):
    """The oracle's rows (loaded indices) inside the window, as parent indices."""
    keep = in_window(ref["site_a"], ref["site_b"], pos, D, K)
    if need_both:
        assert keep.any() and not keep.all(), "the case must have rows on both sides of the window"
    a, b = ref["site_a"][keep].astype(np.int64), ref["site_b"][keep].astype(np.int64)
    if pos is not None:
        a, b = np.asarray(pos)[a], np.asarray(pos)[b]
    return {"site_a": a, "site_b": b, **{f: ref[f][keep] for f in FIELDS}}


def assert_rows(got, exp, what=""):
    assert len(got) == len(exp["site_a"]), (what, len(got), len(exp["site_a"]))
    assert np.array_equal(got.site_a.astype(np.int64), exp["site_a"]), what
    assert np.array_equal(got.site_b.astype(np.int64), exp["site_b"]), what
    for f in FIELDS:
        assert np.array_equal(getattr(got, f).view(np.uint32), np.asarray(exp[f]).view(np.uint32)), (what, f)


def store_as_ref(store):
    return {"site_a": store.site_a.astype(np.uint64), "site_b": store.site_b.astype(np.uint64),
            **{f: getattr(store, f).copy() for f in FIELDS}}


# ------------------------------------------------------------------ 3. every emitting path, K windows
L3, N3 = 700, 200
KS = [1, 63, 64, 65, 255, 256, 300, 700]
# (kernel, ref_sums, options, threshold, data): the issue's five paths in
# lib.rs's order (bit-equal to the oracle), then the exact-sum kernels behind
# the same switches (pair_valu_kernel's VALU and MFMA loops, the integer
# kernels' epilogues), held to their own unwindowed rows
PATHS = {
    "default_thr0": ("auto", None, {}, 0.0, "synth", True),
    "exact_thr0": ("auto", False, {}, 0.0, "synth", False),
    "kernel_valu": ("valu", None, {}, 0.05, "ld_blocks", True),
    "valu_plain": ("auto", None, {"valu_plain": 1}, 0.05, "ld_blocks", True),
    "mfma_layout": ("auto", None, {"mfma_layout": 1}, 0.05, "ld_blocks", True),
    "exact_valu": ("valu", False, {}, 0.05, "ld_blocks", False),
    "exact_valu_plain": ("valu", False, {"valu_plain": 1}, 0.0, "synth", False),
    "exact_mfma_layout": ("mfma", False, {"mfma_layout": 1}, 0.05, "ld_blocks", False),
    "exact_mfma_prefilter": ("mfma", False, {}, 0.05, "ld_blocks", False),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_every_emitting_path_site_windows(W, path):
    kernel, ref_sums, opts, thr, kind, bit_oracle = PATHS[path]
    buf, w = data(kind, L3, N3)
    ctx = W.Context(0, {"auto": W.KERNEL_AUTO, "valu": W.KERNEL_VALU, "mfma": W.KERNEL_MFMA}[kernel],
                    ref_sums=ref_sums)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.load(buf, w)
    assert ctx.window() == (0, 0)
    ctx.run(thr)
    full = ctx.rows()
    ref = oracle(kind, L3, N3, thr) if bit_oracle else store_as_ref(full)
    if bit_oracle:
        assert_rows(full, expected(ref, None, 0, 0, need_both=False), path)
    else:  # (measured, not asserted: how far this path's unwindowed rows are from the oracle's bits)
        o = oracle(kind, L3, N3, thr)
        same = len(full) == len(o["r2"]) and np.array_equal(full.site_a, o["site_a"])
        print(path, "unwindowed rows", len(full), "oracle", len(o["r2"]), "same pairs", same, "r2 bit mismatches",
              int((full.r2.view(np.uint32) != o["r2"].view(np.uint32)).sum()) if same else -1)
    for K in KS:
        ctx.set_window(max_sites=K)
        assert ctx.window() == (0, K)
        n = ctx.run(thr)
        got = ctx.rows()
        assert_rows(got, expected(ref, None, 0, K, need_both=K < L3), (path, K))
        m = window_matrix(L3, None, 0, K)
        st = ctx.stats()
        print(path, K, "rows", n, "pairs", st["pairs"], "tiles", st["tiles"])
        assert st["pairs"] == int(m.sum()), (path, K, st)
        assert st["tiles"] == int((blocks_any(m, 64) > 0).sum()), (path, K, st)
        assert ctx.window_pairs_in_chunks(0, ctx.chunks(L3)) == int(m.sum())
    # K >= L: the unwindowed run's rows, bit for bit
    assert_rows(ctx.rows(), store_as_ref(full), (path, "K >= L"))
    ctx.close()


def test_device_limits_equal_brute_force(W):
    """window_limits_kernel's hi[] (from the resident site_map) against numpy."""
    buf, w = data("ld_blocks", L3, N3)
    pos = gappy_map(L3)
    ctx = W.Context(0)
    ctx.load(buf, w, site_map=pos)
    for D, K in [(0, 1), (0, 64), (0, 700), (100, 0), (1000, 0), (4999, 64), (5000, 0), (2 ** 40, 0), (1, 1)]:
        ctx.set_window(D, K)
        m = window_matrix(L3, pos, D, K)
        want = np.where(m.any(axis=1), L3 - 1 - np.argmax(m[:, ::-1], axis=1), np.arange(L3))
        assert np.array_equal(ctx.window_limits(L3).astype(np.int64), want), (D, K)
    ctx.close()


# ------------------------------------------------------------------ 4. screened paths
@pytest.mark.parametrize("thr,screen,fp6", [(0.05, 1, 0), (0.002, 4, 0), (0.05, 1, 2)],
                         ids=["screen_items", "candidate_pairs", "fp6_screen"])
def test_screened_paths_site_windows(W, thr, screen, fp6):
    L, N = 3000, 600  # (the shape of test_progress_once_per_chunk_screened: known to engage them)
    buf, w = data("ld_blocks", L, N)
    ref = oracle("ld_blocks", L, N, thr)
    ctx = W.Context(0)
    ctx.set_option("screen", screen)
    ctx.set_option("screen_fp6", fp6)
    ctx.load(buf, w)
    for K in (100, 300):
        ctx.set_window(max_sites=K)
        ctx.run(thr)
        st = ctx.stats()
        print(thr, screen, fp6, K, st)
        assert st["screened"] == screen and st["candidate_tiles"] > 0, st
        assert st["screen_fp6"] == (1 if fp6 else 0), st
        assert_rows(ctx.rows(), expected(ref, None, 0, K), (thr, screen, fp6, K))
    ctx.close()


# ------------------------------------------------------------------ 5. distance windows
def gappy_map(L):
    """A gappy, duplicate-bearing non-decreasing map: the cumulative sum of
    increments in [0, 40) (seed 7), six of them raised by 5,000, plus 3."""
    rng = np.random.default_rng(7)
    inc = rng.integers(0, 40, size=L)
    inc[np.linspace(L // 7, L - L // 7, 6).astype(int)] += 5000
    pos = (np.cumsum(inc) + 3).astype(np.uint64)
    assert (np.diff(pos.astype(np.int64)) == 0).sum() >= 5  # equal neighbours (multi-allelic lines)
    return pos


@pytest.mark.parametrize("D,K", [(100, 0), (1000, 0), (4999, 0), (100, 64), (1000, 64), (4999, 64)])
def test_distance_windows_gappy_map(W, D, K):
    buf, w = data("ld_blocks", L3, N3)
    pos = gappy_map(L3)
    ref = oracle("ld_blocks", L3, N3, 0.05)
    ctx = W.Context(0)
    ctx.set_window(D, K)  # the window first, then the load
    ctx.load(buf, w, site_map=pos)
    ctx.run(0.05)
    assert_rows(ctx.rows(), expected(ref, pos, D, K), (D, K))
    m = window_matrix(L3, pos, D, K)
    st = ctx.stats()
    assert st["pairs"] == int(m.sum()) and st["tiles"] == int((blocks_any(m, 64) > 0).sum()), st
    ctx.close()


def test_distance_window_after_load_filtered(W):
    """The kept map of the device pre-pass (parent columns of the kept sites) under max_distance."""
    buf = np.array(data("ld_blocks", L3, N3)[0])
    buf[::7] = 0  # invariant sites: filtered out
    buf[5::31] = 4
    raw_map = gappy_map(L3)
    ctx = W.Context(0)
    n_kept = ctx.load_filtered(buf, site_map=raw_map)
    keep = O.site_mask(buf)
    assert 0 < n_kept == int(keep.sum()) < L3
    kept_map = ctx.site_map()
    assert np.array_equal(kept_map, raw_map[keep])
    ref = O.all_pairs(buf[keep], ctx.weights(), np.float32(0.05))
    for D, K in [(1000, 0), (4999, 50)]:
        ctx.set_window(D, K)  # the load first, then the window
        ctx.run(0.05)
        assert_rows(ctx.rows(), expected(ref, kept_map, D, K), (D, K))
    ctx.close()


def test_descending_map_fails_distance_window_only(W):
    buf, w = data("ld_blocks", L3, N3)
    bad = gappy_map(L3)
    bad[300] = bad[299] - 1
    bad[500] = 0
    ref = oracle("ld_blocks", L3, N3, 0.05)
    # the window first: the load fails
    ctx = W.Context(0)
    ctx.set_window(max_distance=100)
    with pytest.raises(W.WldError) as e:
        ctx.load(buf, w, site_map=bad)
    assert e.value.name == "WLD_E_ARG" and "site_map[300]" in str(e.value), str(e.value)
    # the load first: the window is refused and stays as it was
    ctx.set_window(0, 64)
    ctx.load(buf, w, site_map=bad)
    with pytest.raises(W.WldError) as e:
        ctx.set_window(100, 64)
    assert e.value.name == "WLD_E_ARG" and "site_map[300]" in str(e.value), str(e.value)
    assert ctx.window() == (0, 64)
    # max_sites alone needs no order in the map
    ctx.run(0.05)
    exp = expected(ref, None, 0, 64)
    exp["site_a"], exp["site_b"] = bad[exp["site_a"]].astype(np.int64), bad[exp["site_b"]].astype(np.int64)
    assert_rows(ctx.rows(), exp, "K only")
    ctx.close()


# ------------------------------------------------------------------ 6. run-to-run sequence on one context
def test_window_sequence_on_one_context(W):
    """no window -> K=300 -> K=64 -> D=1000 -> no window on one context:
    stale segment counts of tiles a narrower window leaves out, the tile
    list's cache key, the gather enqueued behind the scan, and a staging
    overflow with its re-run (the first step: 24,830 rows into 1,000)."""
    buf, w = data("ld_blocks", L3, N3)
    ref = oracle("ld_blocks", L3, N3, 0.05)
    ctx = W.Context(0)
    ctx.set_option("staging_rows", 1000)
    pos = gappy_map(L3)  # (so that D = 1000 cuts: in site counts it would admit all 700 sites)
    ctx.load(buf, w, site_map=pos)
    assert len(ref["r2"]) > 1000
    first = None
    for D, K in [(0, 0), (0, 300), (0, 64), (1000, 0), (0, 0)]:
        ctx.set_window(D, K)
        ctx.run(0.05)
        got = ctx.rows()
        assert_rows(got, expected(ref, pos, D, K, need_both=bool(D or K)), (D, K))
        if first is None:
            first = got
    assert_rows(got, store_as_ref(first), "the last step equals the first")
    ctx.close()


# ------------------------------------------------------------------ 7. chunk ranges, batches, device groups
def test_window_shards_batches_and_groups(W):
    buf, w = data("ld_blocks", L3, N3)
    ref = oracle("ld_blocks", L3, N3, 0.05)
    K = 64
    exp = expected(ref, None, 0, K)
    ctx = W.Context(0)
    ctx.load(buf, w)
    ctx.set_window(max_sites=K)
    m = ctx.chunks(L3)
    counts = chunk_counts(window_matrix(L3, None, 0, K))
    total = sum(counts)
    assert [ctx.window_pairs_in_chunks(i, i + 1) for i in range(m)] == counts
    # three shards, balanced by in-window pairs, concatenated in descending shard order
    ranges = [ctx.shard_chunks_window(3, k) for k in range(3)]
    assert ranges[2][0] == 0 and ranges[0][1] == m and all(ranges[k][0] == ranges[k + 1][1] for k in range(2))
    parts = []
    for b, e in reversed(ranges):
        assert sum(counts[b:e]) <= total / 3 + max(counts)
        if e > b:
            ctx.run_chunks(0.05, b, e)
            assert ctx.stats()["pairs"] == sum(counts[b:e])
            parts.append(store_as_ref(ctx.rows()))
    cat = {f: np.concatenate([p[f] for p in parts]) for f in ("site_a", "site_b") + FIELDS}
    cat["site_a"], cat["site_b"] = cat["site_a"].astype(np.int64), cat["site_b"].astype(np.int64)
    ctx.run_chunks(0.05)
    assert_rows(ctx.rows(), cat, "shards")
    assert_rows(ctx.rows(), exp, "whole run")
    # the two-call run obeys the window too, and the window cannot change under it
    ctx.run_chunks_async(0.05)
    with pytest.raises(W.WldError) as e:
        ctx.set_window(max_sites=K + 1)
    assert e.value.name == "WLD_E_STATE"
    assert ctx.run_wait() == len(exp["r2"]) and ctx.window() == (0, K)
    assert_rows(ctx.rows(), exp, "async run")
    # at least three host batches
    before = ctx.get_option("host_batch_pairs")
    limit = total // 4
    ctx.set_option("host_batch_pairs", limit)
    batches, held = 0, None  # wld_run_host's rule: whole chunks, at most `limit` pairs unless a single chunk has more
    for c in counts:
        if held is None or held + c > limit:
            batches, held = batches + 1, 0
        held += c
    assert batches >= 3
    try:
        assert_rows(ctx.run_host(0.05), exp, "batches")
        assert ctx.stats()["pairs"] == total
    finally:
        ctx.set_option("host_batch_pairs", before)
    ctx.close()
    # a device group: the window forwarded to every member, the shards balanced by in-window pairs
    grp = W.Context(0, devices=[0, 0, 0])
    store = W.all_weighted_ld_pairs(W.SiteSet.from_buffer(buf), w, 0.05, ctx=grp, max_sites=K)
    assert grp.window() == (0, 0)  # restored
    assert_rows(store, exp, "device group")
    assert grp.stats()["pairs"] == total
    grp.close()


# ------------------------------------------------------------------ 8. progress
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_window_progress_once_per_live_chunk(W, devices):
    L, N, K = 2000, 500, 300
    buf, w = data("synth", L, N)
    counts = chunk_counts(window_matrix(L, None, 0, K))
    live = [c for c in counts if c]
    assert 0 < len(live) < len(counts)
    ctx = W.Context(0, devices=devices) if devices else W.Context(0)
    seen, threads = [], set()

    def cb(n):
        seen.append(n)
        threads.add(threading.get_ident())
    store = W.all_weighted_ld_pairs(W.SiteSet.from_buffer(buf), w, 0.0, progress_report=cb, ctx=ctx, max_sites=K)
    assert len(seen) == 1 + len(live), (len(seen), len(live))
    assert seen[0] == 0 and seen[1] == 0 and seen == sorted(seen)
    assert sorted(np.diff(seen[1:]).tolist() + [sum(live) - seen[-1]]) == sorted(live)
    assert ctx.stats()["progress_filled"] == 0
    assert threads == {threading.get_ident()}
    ref = oracle("synth", L, N, 0.0)
    assert_rows(store, expected(ref, None, 0, K), "progress run")
    ctx.close()


# ------------------------------------------------------------------ 9. CLI
def _run_cli(args, out):
    r = subprocess.run([CLI, *args, "--pair-output", str(out), "--r2-threshold", "0"], capture_output=True, text=True,
                       timeout=120)
    return r, (open(out, "rb").read().splitlines(keepends=True) if r.returncode == 0 else [])


def test_cli_max_distance_vcf(tmp_path):
    vcf = ["--vcf-input", os.path.join(FIXTURES, "t7_1000genome.vcf")]
    r, full = _run_cli(vcf, tmp_path / "full.tsv")
    assert r.returncode == 0 and len(full) > 2, r.stderr
    ab = np.array([[int(x) for x in ln.split(b"\t")[:2]] for ln in full[1:]])
    D = int(np.median(ab[:, 1] - ab[:, 0]))  # VCF: site indices are POS, the window's coordinates
    keep = ab[:, 1] - ab[:, 0] <= D
    assert keep.any() and not keep.all()
    want = [full[0]] + [ln for ln, k in zip(full[1:], keep) if k]
    for extra in ([], ["--devices", "0,0"]):
        r, got = _run_cli(vcf + ["--max-distance", str(D)] + extra, tmp_path / "win.tsv")
        assert r.returncode == 0, r.stderr
        assert got == want, extra
    r, _ = _run_cli(vcf + ["--max-distance", "x"], tmp_path / "bad.tsv")
    assert r.returncode != 0 and "--max-distance" in r.stderr


@pytest.mark.parametrize("prepass", [False, True], ids=["host_prepass", "gpu_prepass"])
def test_cli_max_sites_fasta(tmp_path, W, prepass):
    path = os.path.join(SYNTH, "synth_n500_l40.fasta")
    fa = ["--fasta-input", path] + (["--gpu-prepass"] if prepass else [])
    r, full = _run_cli(fa, tmp_path / "full.tsv")
    assert r.returncode == 0 and len(full) > 2, r.stderr
    kept = W.read_fasta(path).filter_sites_of_interest(0.8, 0.02, 0.5).site_map  # parent column of each site of interest
    at = {int(p): i for i, p in enumerate(kept)}
    ab = np.array([[at[int(x)] for x in ln.split(b"\t")[:2]] for ln in full[1:]])
    K = int(np.median(ab[:, 1] - ab[:, 0]))  # --max-sites counts sites of interest
    keep = ab[:, 1] - ab[:, 0] <= K
    assert keep.any() and not keep.all()
    r, got = _run_cli(fa + ["--max-sites", str(K)], tmp_path / "win.tsv")
    assert r.returncode == 0, r.stderr
    assert got == [full[0]] + [ln for ln, k in zip(full[1:], keep) if k]


def test_cli_descending_map_with_max_distance(tmp_path):
    """A VCF whose POS column descends: --max-distance prints the library's message and fails; --max-sites runs."""
    src = open(os.path.join(FIXTURES, "t7_1000genome.vcf")).read().splitlines(keepends=True)
    rows = [i for i, ln in enumerate(src) if not ln.startswith("#")]
    cols = src[rows[2]].split("\t")
    cols[1] = "1000"
    src[rows[2]] = "\t".join(cols)
    bad = tmp_path / "desc.vcf"
    bad.write_text("".join(src))
    r, _ = _run_cli(["--vcf-input", str(bad), "--max-distance", "50"], tmp_path / "a.tsv")
    assert r.returncode != 0 and "non-decreasing site_map" in r.stderr and "site_map[2]" in r.stderr, r.stderr
    r, got = _run_cli(["--vcf-input", str(bad), "--max-sites", "2"], tmp_path / "b.tsv")
    assert r.returncode == 0 and len(got) > 1, r.stderr
