"""The banded LD matrix (wld_matrix_banded_width / wld_run_matrix_banded_device /
wld_run_matrix_banded / Context.run_matrix_banded / ld_banded / the CLI's
--matrix-banded): the windowed LD matrix in band storage — element [u - r0, k]
is entry (u, u + k) of the dense matrix, +0.0 past the last site.

Expected bands: the dense expected matrix of tests/matrix_expected.py (the CPU
oracle's d, d', r2 assembled by the contract) skewed into the band in numpy
(banded_from_dense).  Every comparison is by bit pattern, with the NaN
positions equal.  The class counts must equal the oracle's over the in-window
pairs a < b with a in the rows, and run_summary's for all rows.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import CLI, FIXTURES
from matrix_expected import STATS, Dense, assert_same_bits, expected_matrix, in_window
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


def needed_width(L, pos=None, D=0, K=0):
    """max over a of (a's last in-window partner) - a, from the window's definition."""
    if not (D or K):
        return L - 1
    up = np.triu(in_window(L, pos, D, K), 1)
    return int(max((np.flatnonzero(up[a]).max() - a) if up[a].any() else 0 for a in range(L)))


def expected_band(W, dn, rows, bandwidth, stat, pos=None, D=0, K=0, zero_missing=False, dtype=np.float32):
    m = expected_matrix(dn, stat, pos, D, K, zero_missing, dtype)
    return W.banded_from_dense(m, bandwidth)[rows[0]:rows[1]]


def expected_row_counts(dn, rows, pos=None, D=0, K=0):
    """The class counts over the in-window pairs a < b with a in rows."""
    L = dn.L
    has = np.triu(in_window(L, pos, D, K), 1)
    has[:rows[0]] = False
    has[rows[1]:] = False
    v, fin = dn.valid[has], np.isfinite(dn.r2[has])
    return {"pairs": int(has.sum()), "none_pairs": int((~v).sum()), "nonfinite_pairs": int((v & ~fin).sum()),
            "counted_pairs": int((v & fin).sum())}


def band_call(torch, ctx, rows, bandwidth, stat, dtype, zero_missing=False, pad=5):
    """run_matrix_banded into a row-strided view (ld = bandwidth + 1 + pad) of a
    sentinel-filled tensor with one guard row: returns (the view's values,
    info) after checking that nothing outside the view was written."""
    h, w = rows[1] - rows[0], bandwidth + 1
    t = torch.full((h + 1, w + pad), SENTINEL, dtype=getattr(torch, dtype), device="cuda:0")
    out, info = ctx.run_matrix_banded(rows, bandwidth, stat, dtype, zero_missing, out=t[:h, :w])
    assert out.data_ptr() == t.data_ptr()
    full = t.cpu().numpy()
    assert np.all(full[h] == SENTINEL), "the guard row after the band was written"
    assert np.all(full[:h, w:] == SENTINEL), "the elements between the rows were written"
    assert not np.any(full[:h, :w] == SENTINEL), "an element of the block was not written"
    return full[:h, :w].copy(), info


# ------------------------------------------------------------------ 1. tile edges
@pytest.mark.parametrize("N", [7, 64])
def test_tile_edges_all_stats_and_dtypes(W, torch, N):
    """130 sites: three tiles a side, the last holding 2 sites; 7 sequences produce none and nonfinite pairs."""
    dn = dense("shape", N)
    assert dn.L == 130
    ctx = loaded(W, dn)
    assert ctx.matrix_banded_width() == 129
    e = expected_row_counts(dn, (0, 130))
    if N == 7:
        assert e["none_pairs"] == 510 and e["nonfinite_pairs"] == 435
    else:
        assert e["counted_pairs"] == e["pairs"] == 130 * 129 // 2
    for stat in STATS:
        for dtype in ("float32", "float16"):
            got, info = band_call(torch, ctx, (0, 130), 129, stat, dtype)
            assert_same_bits(got, expected_band(W, dn, (0, 130), 129, stat, dtype=np.dtype(dtype)), (N, stat, dtype))
            assert counts_of(info) == e and info.tiles == 6
            assert (info.rows, info.bandwidth, info.stat, info.dtype) == ((0, 130), 129, stat, dtype)
    ctx.close()


# ------------------------------------------------------------------ 2. every class, every window
WINDOWS = [(0, 1), (0, 63), (0, 64), (0, 65), (0, 200), (25, 0), (25, 12)]


@pytest.mark.parametrize("window", WINDOWS, ids=["k1", "k63", "k64", "k65", "k200", "distance", "both"])
def test_every_class_under_windows(W, torch, window):
    dn = dense("case1")
    D, K = window
    pos = case1_map() if D else None
    ctx = loaded(W, dn, pos)
    ctx.set_window(D, K)
    need = needed_width(600, pos, D, K)
    assert ctx.matrix_banded_width() == need
    hi = ctx.window_limits(600)
    assert need == int((hi.astype(np.int64) - np.arange(600)).max()), "the width of wld_window_limits_copy's limits"
    if not D:
        assert need == K
    e = expected_row_counts(dn, (0, 600), pos, D, K)
    s = ctx.run_summary()
    assert e == {k: getattr(s, k) for k in e}, "the summary's counts"
    assert e["none_pairs"] > 0 and e["counted_pairs"] > 0
    for stat, dtype in (("r", "float32"), ("r2", "float16"), ("dprime", "float32")):
        for zm in (False, True):
            got, info = band_call(torch, ctx, (0, 600), need, stat, dtype, zm)
            exp = expected_band(W, dn, (0, 600), need, stat, pos, D, K, zm, np.dtype(dtype))
            assert_same_bits(got, exp, (window, stat, dtype, zm))
            assert np.isnan(exp).any() != zm, "the oracle must hold NaN entries"
            assert counts_of(info) == e, (window, stat)
    ctx.close()


def test_no_window_every_class(W, torch):
    dn = dense("case1")
    ctx = loaded(W, dn)
    e = expected_row_counts(dn, (0, 600))
    assert e == {"pairs": 179700, "none_pairs": 1197, "nonfinite_pairs": 275, "counted_pairs": 178228}
    for stat in STATS:
        got, info = band_call(torch, ctx, (0, 600), 599, stat, "float32")
        assert_same_bits(got, expected_band(W, dn, (0, 600), 599, stat), stat)
        assert counts_of(info) == e and info.tiles == 55
    ctx.close()


# ------------------------------------------------------------------ 3. row ranges
ROWS = [(37, 201), (64, 128), (599, 600)]


@pytest.mark.parametrize("window", [(0, 0), (0, 65), (25, 0)], ids=["none", "k65", "distance"])
def test_row_ranges(W, torch, window):
    dn = dense("case1")
    D, K = window
    pos = case1_map() if D else None
    ctx = loaded(W, dn, pos)
    ctx.set_window(D, K)
    need = ctx.matrix_banded_width()
    for rows in ROWS:
        for stat, dtype in (("r", "float32"), ("d", "float16")):
            got, info = band_call(torch, ctx, rows, need, stat, dtype)
            assert_same_bits(got, expected_band(W, dn, rows, need, stat, pos, D, K, dtype=np.dtype(dtype)), (rows, stat))
            assert counts_of(info) == expected_row_counts(dn, rows, pos, D, K), rows
            assert info.rows == rows
    _, info = ctx.run_matrix_banded((599, 600))
    assert info.pairs == 0 and info.tiles == 1, \
        "the last site has no partner; its row tile's diagonal tile (listed for the other rows' pairs) supplies its k = 0"
    ctx.close()


# ------------------------------------------------------------------ 4. bandwidth
def test_surplus_and_short_bandwidth(W, torch):
    from weightedld_amd._lib import MatrixBandedInfoC, last_error, lib
    dn = dense("case1")
    pos = case1_map()
    for D, K in ((0, 65), (25, 0), (0, 0)):
        ctx = loaded(W, dn, pos)
        ctx.set_window(D, K)
        need = ctx.matrix_banded_width()
        exact, info0 = band_call(torch, ctx, (0, 600), need, "r", "float32")
        got, info = band_call(torch, ctx, (0, 600), need + 7, "r", "float32")
        assert got[:, :need + 1].tobytes() == exact.tobytes()
        assert got[:, need + 1:].tobytes() == np.zeros((600, 7), np.float32).tobytes(), "the surplus is +0.0"
        assert counts_of(info) == counts_of(info0) and info.bandwidth == need + 7
        got, _ = band_call(torch, ctx, (37, 201), need + 400, "r2", "float16")
        assert_same_bits(got, expected_band(W, dn, (37, 201), need + 400, "r2", pos, D, K, dtype=np.float16), (D, K))
        # short: refused, the needed width named
        with pytest.raises(ValueError, match="needs bandwidth %d" % need):
            ctx.run_matrix_banded(bandwidth=need - 1)
        dst = torch.zeros((600, need + 1), dtype=torch.float32, device="cuda:0")
        st = lib().wld_run_matrix_banded_device(ctx._h, 0, 0, need - 1, 1, 0, 0, ctypes.c_void_p(dst.data_ptr()), need + 1,
                                                ctypes.byref(MatrixBandedInfoC()))
        assert st == -1 and "needs bandwidth %d" % need in last_error(), last_error()
        assert not dst.any().item(), "a refused call wrote"
        ctx.close()


# ------------------------------------------------------------------ 5. host call and strips
def test_host_call_strips(W, torch):
    dn = dense("case1")
    ctx = loaded(W, dn)
    ctx.set_window(0, 65)
    dev, infod = band_call(torch, ctx, (0, 600), 65, "r", "float32")
    one, info1 = ctx.run_matrix_banded(stat="r")
    ctx.set_option("matrix_batch_bytes", 200 * 66 * 4)  # 200 + 200 + 200 rows
    three, info3 = ctx.run_matrix_banded(stat="r")
    ctx.set_option("matrix_batch_bytes", 1)  # the minimum of 64 rows applies: 10 strips
    many, infom = ctx.run_matrix_banded(stat="r")
    assert one.shape == (600, 66) and one.dtype == np.float32
    assert one.tobytes() == dev.tobytes() == three.tobytes() == many.tobytes()
    assert counts_of(info1) == counts_of(infod) == counts_of(info3) == counts_of(infom)
    # row tiles 3 (sites 192..255) and 6 (384..447) meet two of the three strips: their three tiles run once
    # per strip; strips of 64 rows from row 0 are the row tiles themselves
    assert info1.tiles == infod.tiles == infom.tiles == 27 and info3.tiles == 27 + 2 * 3
    # a strided numpy destination, a row range, float16, strips
    big = np.full((165, 80), SENTINEL, dtype=np.float16)
    ctx.set_option("matrix_batch_bytes", 70 * 66 * 2)
    out, info = ctx.run_matrix_banded((37, 201), 65, "r2", "float16", out=big[:164, :66])
    assert np.all(big[164] == SENTINEL) and np.all(big[:164, 66:] == SENTINEL)
    assert_same_bits(big[:164, :66], expected_band(W, dn, (37, 201), 65, "r2", K=65, dtype=np.float16))
    assert counts_of(info) == expected_row_counts(dn, (37, 201), K=65)
    ctx.close()


# ------------------------------------------------------------------ 6. against run_matrix, determinism
def test_agrees_with_run_matrix_and_two_calls_identical(W, torch):
    dn = dense("case1")
    ctx = loaded(W, dn, case1_map())
    for D, K in ((25, 40), (0, 64), (0, 0)):
        ctx.set_window(D, K)
        need = ctx.matrix_banded_width()
        for stat, dtype, zm in (("r", "float32", False), ("dprime", "float16", True)):
            m, im = ctx.run_matrix(stat=stat, dtype=dtype, zero_missing=zm)
            a, ia = ctx.run_matrix_banded(stat=stat, dtype=dtype, zero_missing=zm)
            b, ib = ctx.run_matrix_banded(stat=stat, dtype=dtype, zero_missing=zm)
            assert a.tobytes() == b.tobytes() and counts_of(ia) == counts_of(ib)
            assert_same_bits(a, W.banded_from_dense(m, need), (D, K, stat))
            assert counts_of(ia) == counts_of(im)
            t = torch.empty((600, need + 1), dtype=getattr(torch, dtype), device="cuda:0")
            ctx.run_matrix_banded(stat=stat, dtype=dtype, zero_missing=zm, out=t)
            assert t.cpu().numpy().tobytes() == a.tobytes(), "the device call and the host call"
    ctx.close()


def test_ld_banded(W):
    dn = dense("case1")
    ss = W.SiteSet.from_buffer(dn.buf, site_map=case1_map())
    ctx = W.Context(0)
    ctx.set_window(0, 7)
    band, info, sites = W.ld_banded(ss, dn.w, stat="r2", max_distance=25, ctx=ctx)
    assert ctx.window() == (0, 7), "the context's own window is restored"
    need = needed_width(600, case1_map(), 25, 0)
    assert band.shape == (600, need + 1) and info.bandwidth == need and np.array_equal(sites, case1_map())
    assert_same_bits(band, expected_band(W, dn, (0, 600), need, "r2", case1_map(), 25, 0))
    with pytest.raises(ValueError):
        W.ld_banded(ss, dn.w, stat="rho", ctx=ctx)
    ctx.close()


# ------------------------------------------------------------------ 7. undisturbed state
def _rows_now(ctx):
    r = ctx.rows()
    return [r.site_a.copy(), r.site_b.copy(), r.d.view(np.uint32).copy(), r.d_prime.view(np.uint32).copy(),
            r.r2.view(np.uint32).copy()]


def _same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


def test_rows_undisturbed(W, torch):
    dn = dense("case1")
    ref, ctx = loaded(W, dn), loaded(W, dn)  # ref never runs a banded matrix
    n = ctx.run_chunks(0.05)
    before, stats = _rows_now(ctx), ctx.stats()
    assert n == len(before[0]) > 0
    ctx.run_matrix_banded(stat="r")
    ctx.run_matrix_banded((3, 200), out=torch.empty((197, 600), dtype=torch.float32, device="cuda:0"))
    assert ctx.stats() == stats, "wld_last_stats changed"
    assert _same(_rows_now(ctx), before), "the last run's rows changed"
    for K in (64, 0):
        ref.set_window(0, K)
        ctx.set_window(0, K)
        ref.run_chunks(0.05)
        want = _rows_now(ref)
        ctx.run_matrix_banded()
        ctx.run_matrix_banded((0, 70))
        ctx.run_chunks(0.05)
        assert _same(_rows_now(ctx), want), K
    ref.close()
    ctx.close()


# ------------------------------------------------------------------ 8. refusals
def test_refusals(W, torch):
    from weightedld_amd._lib import MatrixBandedInfoC, lib
    L = lib()
    dn = dense("shape", 64)
    dst = torch.zeros((130, 140), dtype=torch.float32, device="cuda:0")
    host = np.zeros((130, 140), dtype=np.float32)
    ARG, STATE = -1, -7

    def both(ctx, rb, re, K, stat, dtype, flags, ld, null=False):
        info = MatrixBandedInfoC()
        d = L.wld_run_matrix_banded_device(ctx._h, rb, re, K, stat, dtype, flags,
                                           None if null else ctypes.c_void_p(dst.data_ptr()), ld, ctypes.byref(info))
        h = L.wld_run_matrix_banded(ctx._h, rb, re, K, stat, dtype, flags,
                                    None if null else ctypes.c_void_p(host.ctypes.data), ld, ctypes.byref(info))
        assert d == h, (d, h)
        return d

    k = ctypes.c_uint32(0)
    ctx = W.Context(0)
    assert both(ctx, 0, 0, 129, 1, 0, 0, 130) == STATE, "before a load"
    assert L.wld_matrix_banded_width(ctx._h, ctypes.byref(k)) == STATE
    ctx.load(dn.buf, dn.w)
    assert L.wld_matrix_banded_width(ctx._h, ctypes.byref(k)) == 0 and k.value == 129
    assert L.wld_matrix_banded_width(ctx._h, None) == ARG
    assert both(ctx, 0, 0, 129, 1, 0, 0, 130) == 0
    assert both(ctx, 0, 0, 139, 1, 0, 0, 140) == 0, "a surplus bandwidth"
    assert both(ctx, 0, 0, 128, 1, 0, 0, 130) == ARG, "a short bandwidth"
    assert both(ctx, 5, 5, 129, 1, 0, 0, 130) == ARG, "empty rows"
    assert both(ctx, 9, 3, 129, 1, 0, 0, 130) == ARG, "reversed rows"
    assert both(ctx, 130, 0, 129, 1, 0, 0, 130) == ARG, "rows begin at the site count"
    assert both(ctx, 0, 131, 129, 1, 0, 0, 130) == ARG, "row end out of range"
    assert both(ctx, 0, 0, 129, 4, 0, 0, 130) == ARG, "unknown stat"
    assert both(ctx, 0, 0, 129, -1, 0, 0, 130) == ARG, "unknown stat"
    assert both(ctx, 0, 0, 129, 1, 2, 0, 130) == ARG, "unknown dtype"
    assert both(ctx, 0, 0, 129, 1, 0, 2, 130) == ARG, "unknown flag bit"
    assert both(ctx, 0, 0, 129, 1, 0, 0, 129) == ARG, "ld below bandwidth + 1"
    assert both(ctx, 0, 0, 129, 1, 0, 0, 130, null=True) == ARG, "null destination"
    assert L.wld_run_matrix_banded_device(ctx._h, 0, 0, 129, 1, 0, 0, ctypes.c_void_p(dst.data_ptr()), 130, None) == ARG
    ctx.run_chunks_async(0.05)
    assert both(ctx, 0, 0, 129, 1, 0, 0, 130) == STATE, "during a run"
    ctx.run_wait()
    assert both(ctx, 0, 0, 129, 1, 0, 0, 130) == 0, "the context stays usable"
    # Python: refused before any device call
    for kw in ({"rows": (0, 131)}, {"stat": "rho"}, {"dtype": "float64"}, {"bandwidth": 128},
               {"out": torch.empty((130, 130), dtype=torch.float32)},                      # on the CPU
               {"out": torch.empty((130, 130), dtype=torch.float16, device="cuda:0")},     # dtype float32 asked
               {"out": torch.empty((130, 260), dtype=torch.float32, device="cuda:0")[:, ::2]},
               {"out": torch.empty((130, 129), dtype=torch.float32, device="cuda:0")}):
        with pytest.raises(ValueError):
            ctx.run_matrix_banded(**kw)
    w = dn.w.copy()
    w[3] = np.inf
    ctx.load(dn.buf, w)
    assert both(ctx, 0, 0, 129, 1, 0, 0, 130) == ARG, "non-finite weights"
    with pytest.raises(W.WldError) as ei:
        ctx.run_matrix_banded()
    assert ei.value.name == "WLD_E_ARG"
    ctx.close()
    grp = W.Context(devices=[0, 0])
    grp.load(dn.buf, dn.w)
    assert both(grp, 0, 0, 129, 1, 0, 0, 130) == STATE, "a device group"
    assert L.wld_matrix_banded_width(grp._h, ctypes.byref(k)) == STATE
    grp.close()
    with pytest.raises(W.WldError) as ei:
        W.Context(0).run_matrix_banded()
    assert ei.value.name == "WLD_E_STATE"


# ------------------------------------------------------------------ 9. CLI
def test_cli_vcf_window(W, tmp_path):
    """(VCF input takes no site filter; site index = POS, the window's coordinate)"""
    path = os.path.join(FIXTURES, "t7_1000genome.vcf")
    vcf = W.read_vcf(path)
    for zm in (False, True):
        ctx = W.Context(0)
        want, info, sites = W.ld_banded(vcf, W.henikoff_weights(vcf), stat="r2", zero_missing=zm, max_sites=3, ctx=ctx)
        ctx.close()
        assert want.shape == (vcf.n_sites(), 4) and info.bandwidth == 3
        npy = str(tmp_path / "b.npy")
        out = subprocess.run([CLI, "--vcf-input", path, "--max-sites", "3", "--matrix-stat", "r2", "--matrix-banded",
                              "--matrix-format", "npy", "--matrix-output", npy] + (["--matrix-zero-missing"] if zm else []),
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        b = np.load(npy)
        assert b.dtype == np.dtype("<f4") and b.flags.c_contiguous
        assert_same_bits(b, want, "npy")
        assert np.array_equal(np.loadtxt(npy + ".sites", dtype=np.uint64, ndmin=1), sites)
        assert (b[:, 1:] != 0).any() and not b[-1, 1:].any(), "the last site's row holds its diagonal alone"
