"""The dense LD matrix (wld_run_matrix_device / wld_run_matrix /
Context.run_matrix / ld_matrix / the CLI's --matrix-output): r, r2, d or d' of a
site rectangle, symmetric bit for bit, banded under a window, float32 or
float16, left on the device or copied to the host in bands.

Expected matrices: the CPU oracle's dense d, d', r2 and `valid`
(O.all_pairs_dense, upper triangle) assembled in numpy by the contract
(matrix_expected.py: mirrored, diagonal rule, window mask, stat; r built with
np.sqrt on float32; float16 by astype).  Every comparison is by bit pattern,
with the NaN positions equal; NaN payloads are not compared.  The class counts
must equal the oracle's over the distinct pairs with an entry in the
rectangle, and run_summary's for the full square.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
from conftest import CLI, FIXTURES, SYNTH
from matrix_expected import STATS, Dense, assert_same_bits, expected_counts, expected_matrix
from test_gpu_summary import case1, case1_map, shape_case

pytestmark = pytest.mark.gpu

SENTINEL = -777.25  # exact in float16 and float32; no LD statistic of these inputs


@pytest.fixture(scope="module")
def W():
    import weightedld_amd as W
    return W


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def dense(name, N=0):
    c = case1() if name == "case1" else shape_case(N)
    return Dense(c.buf, c.w)


def loaded(W, dn, pos=None):
    ctx = W.Context(0)
    ctx.load(dn.buf, dn.w, pos)
    return ctx


def counts_of(info):
    return {k: getattr(info, k) for k in ("pairs", "none_pairs", "nonfinite_pairs", "counted_pairs")}


def device_call(torch, ctx, rows, cols, stat, dtype, zero_missing=False, pad=5):
    """run_matrix into a row-strided view (ld = width + pad) of a sentinel-filled
    tensor with one guard row: returns (the view's values, info) after
    checking that nothing outside the view was written."""
    h, w = rows[1] - rows[0], cols[1] - cols[0]
    t = torch.full((h + 1, w + pad), SENTINEL, dtype=getattr(torch, dtype), device="cuda:0")
    out, info = ctx.run_matrix(rows, cols, stat, dtype, zero_missing, out=t[:h, :w])
    assert out.data_ptr() == t.data_ptr()
    full = t.cpu().numpy()
    assert np.all(full[h] == SENTINEL), "the guard row after the matrix was written"
    assert np.all(full[:h, w:] == SENTINEL), "the elements between the rows were written"
    return full[:h, :w].copy(), info


# ------------------------------------------------------------------ 1. full square
@pytest.mark.parametrize("N", [7, 64])
def test_full_square_all_stats_and_dtypes(W, torch, N):
    """130 sites: three tiles a side, the last holding 2 sites; 7 sequences is the scalar tail only."""
    dn = dense("shape", N)
    assert dn.L == 130
    ctx = loaded(W, dn)
    e = expected_counts(dn, (0, 130), (0, 130))
    if N == 7:
        assert e["none_pairs"] == 510 and e["nonfinite_pairs"] == 435
    else:
        assert e["counted_pairs"] == e["pairs"] == 130 * 129 // 2
    for stat in STATS:
        for dtype in ("float32", "float16"):
            got, info = device_call(torch, ctx, (0, 130), (0, 130), stat, dtype)
            assert_same_bits(got, expected_matrix(dn, stat, dtype=np.dtype(dtype)), (N, stat, dtype))
            assert counts_of(info) == e and info.tiles == 6
            assert (info.rows, info.cols, info.stat, info.dtype) == ((0, 130), (0, 130), stat, dtype)
    ctx.close()


# ------------------------------------------------------------------ 2. every class
def test_every_class(W, torch):
    dn = dense("case1")
    ctx = loaded(W, dn)
    e = expected_counts(dn, (0, 600), (0, 600))
    assert e == {"pairs": 179700, "none_pairs": 1197, "nonfinite_pairs": 275, "counted_pairs": 178228}
    iu = np.triu_indices(600, 1)
    cnt = dn.valid[iu] & np.isfinite(dn.r2[iu])
    assert (dn.d[iu][cnt] > 0).sum() == 91384 and (dn.d[iu][cnt] < 0).sum() == 86844
    s = ctx.run_summary()
    for stat in STATS:
        for dtype in ("float32",) + (("float16",) if stat in ("r", "r2") else ()):
            for zm in (False, True):
                got, info = device_call(torch, ctx, (0, 600), (0, 600), stat, dtype, zm)
                exp = expected_matrix(dn, stat, zero_missing=zm, dtype=np.dtype(dtype))
                assert_same_bits(got, exp, (stat, dtype, zm))
                assert np.isnan(exp).any() != zm, "the oracle must hold NaN entries"
                assert counts_of(info) == e
                assert counts_of(info) == {k: getattr(s, k) for k in e}, "the summary's counts"
    ctx.close()


# ------------------------------------------------------------------ 3. the sign's meaning
def test_sign_is_the_correlations(W):
    """sign(r) = the sign of the f64 weighted covariance of the two sites'
    major-allele indicators over the pair's mask, computed from the buffer and
    the weights (not from d)."""
    dn = dense("shape", 64)
    ctx = loaded(W, dn)
    r, _ = ctx.run_matrix(stat="r")
    ctx.close()
    L = dn.L
    maj = np.zeros(L, dtype=np.int64)
    mnr = np.zeros(L, dtype=np.int64)
    for s in range(L):
        maj[s], mnr[s] = O.major_minor(O.histogram(dn.buf[s]))
    A = (dn.buf == maj[:, None]).astype(np.float64)                      # major
    M = A + (dn.buf == mnr[:, None]).astype(np.float64)                  # major or minor: in the mask
    w = dn.w.astype(np.float64)
    T, SA, SB, SAB = (M * w) @ M.T, (A * w) @ M.T, (M * w) @ A.T, (A * w) @ A.T
    cov = SAB / T - (SA / T) * (SB / T)
    big = (np.abs(r) > 0.05) & ~np.eye(L, dtype=bool)
    assert big.sum() > 1000 and (r[big] > 0).any() and (r[big] < 0).any()
    assert np.array_equal(np.sign(r[big]), np.sign(cov[big]))
    assert np.abs(np.abs(r[big]) - np.abs(cov[big] / np.sqrt((SA / T) * (1 - SA / T) * (SB / T) * (1 - SB / T))[big])).max() < 1e-4


# ------------------------------------------------------------------ 4. symmetry
def test_bitwise_symmetry(W):
    """(fails if (b, a) is evaluated on its own: the oracle's (a, b) and (b, a) differ on these inputs)"""
    dn = dense("case1")
    ctx = loaded(W, dn)
    for stat in STATS:
        m, _ = ctx.run_matrix(stat=stat)
        assert m.tobytes() == np.ascontiguousarray(m.T).tobytes(), stat
    ctx.close()


# ------------------------------------------------------------------ 5. rectangles
RECTS_130 = [((3, 129), (61, 70)), ((70, 130), (0, 60)), ((50, 100), (60, 130)), ((64, 65), (64, 65)),
             ((5, 6), (100, 101)), ((129, 130), (129, 130))]


def test_rectangles(W, torch):
    dn = dense("shape", 7)
    ctx = loaded(W, dn)
    full = {s: expected_matrix(dn, s) for s in ("r", "dprime")}
    for rows, cols in RECTS_130:
        for stat in ("r", "dprime"):
            got, info = device_call(torch, ctx, rows, cols, stat, "float32")
            assert_same_bits(got, full[stat][rows[0]:rows[1], cols[0]:cols[1]], (rows, cols, stat))
            assert counts_of(info) == expected_counts(dn, rows, cols), (rows, cols)
    _, info = ctx.run_matrix((70, 130), (0, 60))
    assert info.pairs == 60 * 60 and info.tiles == 2, "strictly below the diagonal: mirrored images only"
    _, info = ctx.run_matrix((50, 100), (60, 130))
    assert info.pairs == 50 * 70 - 40 - 40 * 39 // 2, "a pair with both orientations inside counts once"
    ctx.close()


def test_single_row_and_column(W, torch):
    dn = dense("case1")
    ctx = loaded(W, dn)
    full = expected_matrix(dn, "r")
    for rows, cols in (((77, 78), (0, 600)), ((0, 600), (333, 334))):
        got, info = device_call(torch, ctx, rows, cols, "r", "float32")
        assert_same_bits(got, full[rows[0]:rows[1], cols[0]:cols[1]], (rows, cols))
        assert counts_of(info) == expected_counts(dn, rows, cols) and info.pairs == 599 and info.tiles == 10
    ctx.close()


# ------------------------------------------------------------------ 6. windows
@pytest.mark.parametrize("window", [(0, 40), (25, 0), (25, 12)], ids=["max_sites", "max_distance", "both"])
def test_windows(W, torch, window):
    dn = dense("case1")
    D, K = window
    pos = case1_map() if D else None
    ctx = loaded(W, dn, pos)
    _, unwindowed = ctx.run_matrix()
    assert unwindowed.tiles == 55
    ctx.set_window(D, K)
    s = ctx.run_summary()
    for stat, dtype in (("r", "float32"), ("r2", "float16")):
        got, info = device_call(torch, ctx, (0, 600), (0, 600), stat, dtype)
        exp = expected_matrix(dn, stat, pos, D, K, dtype=np.dtype(dtype))
        assert_same_bits(got, exp, (window, stat))
        assert (exp == 0).sum() > 600 * 400, "most of the matrix is out of the window"
        e = expected_counts(dn, (0, 600), (0, 600), pos, D, K)
        assert counts_of(info) == e == {k: getattr(s, k) for k in e}
        assert 0 < info.tiles < unwindowed.tiles
    # a rectangle far from the diagonal: no tile at all, all +0.0
    got, info = device_call(torch, ctx, (0, 100), (400, 600), "r", "float32")
    assert info.tiles == 0 and info.pairs == 0 and got.tobytes() == np.zeros((100, 200), np.float32).tobytes()
    # ... and one across tile boundaries under the window
    got, info = device_call(torch, ctx, (100, 333), (90, 301), "dprime", "float32")
    assert_same_bits(got, expected_matrix(dn, "dprime", pos, D, K)[100:333, 90:301], window)
    assert counts_of(info) == expected_counts(dn, (100, 333), (90, 301), pos, D, K)
    ctx.close()


# ------------------------------------------------------------------ 7. host call and bands
def test_host_call_bands(W, torch):
    dn = dense("case1")
    ctx = loaded(W, dn)
    assert ctx.get_option("matrix_batch_bytes") == 1 << 30
    one, info1 = ctx.run_matrix(stat="r")
    dev, infod = device_call(torch, ctx, (0, 600), (0, 600), "r", "float32")
    ctx.set_option("matrix_batch_bytes", 1)  # the minimum of 64 rows applies: 10 bands
    many, infom = ctx.run_matrix(stat="r")
    ctx.set_option("matrix_batch_bytes", 250 * 600 * 4)  # 250 + 250 + 100 rows
    three, info3 = ctx.run_matrix(stat="r")
    assert one.tobytes() == dev.tobytes() == many.tobytes() == three.tobytes()
    assert_same_bits(one, expected_matrix(dn, "r"))
    assert counts_of(info1) == counts_of(infod) == counts_of(infom) == counts_of(info3)
    assert info1.tiles == 55 and infom.tiles == 10 * 10 and info3.tiles > 55  # (a band lists the tiles of its images)
    # a strided numpy destination, a rectangle, float16, bands
    big = np.full((301, 80), SENTINEL, dtype=np.float16)
    out, info = ctx.run_matrix((100, 400), (530, 600), "r2", "float16", out=big[:300, :70])
    assert np.all(big[300] == SENTINEL) and np.all(big[:300, 70:] == SENTINEL)
    assert_same_bits(big[:300, :70], expected_matrix(dn, "r2", dtype=np.float16)[100:400, 530:600])
    assert counts_of(info) == expected_counts(dn, (100, 400), (530, 600))
    ctx.close()


# ------------------------------------------------------------------ 8. torch destinations
def test_torch_destinations(W, torch):
    dn = dense("case1")
    ctx = loaded(W, dn)
    t16 = torch.empty((600, 600), dtype=torch.float16, device="cuda:0")
    out, _ = ctx.run_matrix(stat="r", dtype="float16", out=t16)
    assert out is t16
    assert_same_bits(t16.cpu().numpy(), expected_matrix(dn, "r", dtype=np.float16))
    parent = torch.full((700, 640), SENTINEL, dtype=torch.float32, device="cuda:0")
    view = parent[50:650, 20:620]
    ctx.run_matrix(stat="r2", out=view)
    p = parent.cpu().numpy()
    assert_same_bits(p[50:650, 20:620], expected_matrix(dn, "r2"))
    p[50:650, 20:620] = SENTINEL
    assert np.all(p == SENTINEL), "elements of the parent tensor outside the view changed"
    # refused before any device call
    with pytest.raises(ValueError):
        ctx.run_matrix(out=torch.empty((600, 600), dtype=torch.float32))  # on the CPU
    with pytest.raises(ValueError):
        ctx.run_matrix(out=t16)  # dtype float32 asked
    with pytest.raises(ValueError):
        ctx.run_matrix(out=parent[:600, :1200:2])  # last stride 2
    with pytest.raises(ValueError):
        ctx.run_matrix((0, 10), out=parent[:600, :600])  # shape
    ctx.close()


# ------------------------------------------------------------------ 9. determinism
def test_two_calls_identical(W):
    dn = dense("case1")
    ctx = loaded(W, dn, case1_map())
    ctx.set_window(25, 40)
    for stat, dtype in (("r", "float32"), ("dprime", "float16")):
        a, ia = ctx.run_matrix(stat=stat, dtype=dtype)
        b, ib = ctx.run_matrix(stat=stat, dtype=dtype)
        assert a.tobytes() == b.tobytes() and counts_of(ia) == counts_of(ib)
    ctx.close()


# ------------------------------------------------------------------ 10. undisturbed state
def _rows_now(ctx):
    r = ctx.rows()
    return [r.site_a.copy(), r.site_b.copy(), r.d.view(np.uint32).copy(), r.d_prime.view(np.uint32).copy(),
            r.r2.view(np.uint32).copy()]


def _same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


def test_rows_undisturbed(W, torch):
    dn = dense("case1")
    ref, ctx = loaded(W, dn), loaded(W, dn)  # ref never runs a matrix
    n = ctx.run_chunks(0.05)
    before, stats = _rows_now(ctx), ctx.stats()
    assert n == len(before[0]) > 0
    ctx.run_matrix(stat="r")
    ctx.run_matrix((3, 200), (100, 600), out=torch.empty((197, 500), dtype=torch.float32, device="cuda:0"))
    assert ctx.stats() == stats, "wld_last_stats changed"
    assert _same(_rows_now(ctx), before), "the last run's rows changed"
    # no window -> max_sites 64 -> none: a matrix (whole, and a rectangle: other
    # lists) before the row runs of each state leaves them the reference's
    for K in (64, 0):
        ref.set_window(0, K)
        ctx.set_window(0, K)
        ref.run_chunks(0.05)
        want = _rows_now(ref)
        ctx.run_matrix()
        ctx.run_matrix((0, 70), (500, 600))
        ctx.run_chunks(0.05)
        assert _same(_rows_now(ctx), want), K
    ref.close()
    ctx.close()


# ------------------------------------------------------------------ 11. refusals
def test_refusals(W, torch):
    from weightedld_amd._lib import MatrixInfoC, lib
    L = lib()
    dn = dense("shape", 64)
    dst = torch.zeros((130, 130), dtype=torch.float32, device="cuda:0")
    host = np.zeros((130, 130), dtype=np.float32)
    ARG, STATE = -1, -7

    def both(ctx, rb, re, cb, ce, stat, dtype, flags, ld, null=False):
        info = MatrixInfoC()
        d = L.wld_run_matrix_device(ctx._h, rb, re, cb, ce, stat, dtype, flags,
                                    None if null else ctypes.c_void_p(dst.data_ptr()), ld, ctypes.byref(info))
        h = L.wld_run_matrix(ctx._h, rb, re, cb, ce, stat, dtype, flags,
                             None if null else ctypes.c_void_p(host.ctypes.data), ld, ctypes.byref(info))
        assert d == h, (d, h)
        return d

    ctx = W.Context(0)
    assert both(ctx, 0, 0, 0, 0, 1, 0, 0, 130) == STATE, "before a load"
    ctx.load(dn.buf, dn.w)
    assert both(ctx, 0, 0, 0, 0, 1, 0, 0, 130) == 0
    assert both(ctx, 5, 5, 0, 0, 1, 0, 0, 130) == ARG, "empty rows"
    assert both(ctx, 0, 0, 9, 3, 1, 0, 0, 130) == ARG, "reversed columns"
    assert both(ctx, 130, 0, 0, 0, 1, 0, 0, 130) == ARG, "rows begin at the site count"
    assert both(ctx, 0, 131, 0, 0, 1, 0, 0, 130) == ARG, "row end out of range"
    assert both(ctx, 0, 0, 0, 500, 1, 0, 0, 500) == ARG, "column end out of range"
    assert both(ctx, 0, 0, 0, 0, 4, 0, 0, 130) == ARG, "unknown stat"
    assert both(ctx, 0, 0, 0, 0, -1, 0, 0, 130) == ARG, "unknown stat"
    assert both(ctx, 0, 0, 0, 0, 1, 2, 0, 130) == ARG, "unknown dtype"
    assert both(ctx, 0, 0, 0, 0, 1, 0, 2, 130) == ARG, "unknown flag bit"
    assert both(ctx, 0, 0, 0, 0, 1, 0, 0, 129) == ARG, "ld below the width"
    assert both(ctx, 0, 0, 10, 20, 1, 0, 0, 9) == ARG, "ld below the width"
    assert both(ctx, 0, 0, 0, 0, 1, 0, 0, 130, null=True) == ARG, "null destination"
    ctx.run_chunks_async(0.05)
    assert both(ctx, 0, 0, 0, 0, 1, 0, 0, 130) == STATE, "during a run"
    ctx.run_wait()
    assert both(ctx, 0, 0, 0, 0, 1, 0, 0, 130) == 0, "the context stays usable"
    w = dn.w.copy()
    w[3] = np.inf
    ctx.load(dn.buf, w)
    assert both(ctx, 0, 0, 0, 0, 1, 0, 0, 130) == ARG, "non-finite weights"
    with pytest.raises(W.WldError) as ei:
        ctx.run_matrix()
    assert ei.value.name == "WLD_E_ARG"
    ctx.close()
    grp = W.Context(devices=[0, 0])
    grp.load(dn.buf, dn.w)
    assert both(grp, 0, 0, 0, 0, 1, 0, 0, 130) == STATE, "a device group"
    grp.close()
    with pytest.raises(W.WldError) as ei:
        W.Context(0).run_matrix()
    assert ei.value.name == "WLD_E_STATE"


# ------------------------------------------------------------------ 12. CLI
def _read_tsv(path):
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        rows = [ln.rstrip("\n").split("\t") for ln in f]
    assert head[0] == "site"
    sites = np.array([int(x) for x in head[1:]], dtype=np.uint64)
    assert [int(r[0]) for r in rows] == sites.tolist()
    return sites, np.array([[np.float32(float(x)) for x in r[1:]] for r in rows], dtype=np.float32)


def _cli_case(W, tmp_path, args, site_set, region, stat, window, zero_missing=False):
    ctx = W.Context(0)
    want, info, sites = W.ld_matrix(site_set, W.henikoff_weights(site_set), region, stat, zero_missing=zero_missing,
                                    max_distance=window[0], max_sites=window[1], ctx=ctx)
    ctx.close()
    tsv, npy = str(tmp_path / "m.tsv"), str(tmp_path / "m.npy")
    base = [CLI, *args, "--matrix-stat", stat] + (["--matrix-zero-missing"] if zero_missing else [])
    if region is not None:
        base += ["--matrix-region", "%d:%d" % region]
    out = subprocess.run(base + ["--matrix-output", tsv], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got_sites, got = _read_tsv(tsv)
    assert np.array_equal(got_sites, sites)
    assert_same_bits(got, want, "tsv")
    out = subprocess.run(base + ["--matrix-output", npy, "--matrix-format", "npy"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    with open(npy, "rb") as f:
        assert f.read(8) == b"\x93NUMPY\x01\x00"
    m = np.load(npy)
    assert m.dtype == np.dtype("<f4") and m.flags.c_contiguous
    assert_same_bits(m, want, "npy")
    assert np.array_equal(np.loadtxt(npy + ".sites", dtype=np.uint64, ndmin=1), sites)
    return want, info


def test_cli_fasta(W, tmp_path):
    """(a FASTA set's parent coordinate is the column in the unfiltered alignment)"""
    path = os.path.join(SYNTH, "synth_n200_l24.fasta")
    kept = W.read_fasta(path).filter_sites_of_interest(0.8, 0.02, 0.5)
    parent = np.array([kept.parent_site_index(i) for i in range(kept.n_sites())], dtype=np.uint64)
    loaded_set = W.SiteSet.from_buffer(kept.buffer, site_map=parent)
    m, _ = _cli_case(W, tmp_path, ["--fasta-input", path], loaded_set, None, "r", (None, None))
    assert m.shape == (kept.n_sites(),) * 2
    lo, hi = int(parent[2]), int(parent[-3])
    m, _ = _cli_case(W, tmp_path, ["--fasta-input", path], loaded_set, (lo, hi), "dprime", (None, None), True)
    assert m.shape == (kept.n_sites() - 5,) * 2


def test_cli_vcf_window(W, tmp_path):
    """(VCF input takes no site filter; site index = POS, the window's coordinate)"""
    path = os.path.join(FIXTURES, "t7_1000genome.vcf")
    vcf = W.read_vcf(path)
    m, info = _cli_case(W, tmp_path, ["--vcf-input", path, "--max-distance", "100", "--max-sites", "3"], vcf, None,
                        "r2", (100, 3))
    L = vcf.n_sites()
    assert m.shape == (L, L) and info.pairs < L * (L - 1) // 2, "the window must cut pairs"
    assert (m == 0).any()
