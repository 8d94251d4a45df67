"""The sweep scan on the device (wld_banded_pairsum_device,
wld_banded_omega_device, wld_run_omega; Context.banded_pairsum, banded_omega,
run_omega, ld_omega and the CLI's --omega-output).

Every device value is compared with the numpy twins (banded_pairsum_host,
banded_omega_host: the definition) BYTE FOR BYTE: the table, omega and zns as
float64 bit patterns, the borders and the evaluated / skipped counts exactly.
The twins themselves are checked against brute force in
tests/test_banded_omega_api.py.  Bands and outputs are strided or offset views
with NaN in the band's padding and sentinels around every output: nothing
outside the views may be written.  The end-to-end test also holds the table of
case1's r2 band within the summation bound gamma_{m-1} of an fsum over
run_matrix's dense r2 (m the window's pair count; see the API test).
"""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import CLI, FIXTURES, SYNTH
from test_banded_omega_api import (PAIRSUM_SHAPES, every_split, gamma, r2_band_case, sweep_case, tie_case,
                                   zero_cross_case)
from test_gpu_heatmap import case1_map
from test_gpu_summary import case1

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
ISENT = 0x5A5A5A5A


@pytest.fixture(scope="module")
def W():
    import weightedld_amd as W
    return W


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx(W):
    c = W.Context(0)  # neither device call needs a load
    yield c
    c.close()


def pairsum_strided(torch, ctx, B, bandwidth=None):
    """banded_pairsum on row-strided views with NaN / sentinel padding: returns
    (M as numpy, info, the device table view) after the layout checks."""
    n, Wd = B.shape
    K = Wd - 1 if bandwidth is None else bandwidth
    tb = torch.full((n, Wd + 3), float("nan"), dtype=getattr(torch, B.dtype.name), device="cuda:0")
    tb[:, :Wd] = torch.from_numpy(np.array(B))
    keep = tb.clone()
    tf = torch.full((n + 1, K + 1 + 4), SENTINEL, dtype=torch.float64, device="cuda:0")
    out, info = ctx.banded_pairsum(tb[:, :Wd], out=tf[:n, :K + 1], bandwidth=bandwidth)
    assert out.data_ptr() == tf.data_ptr()
    full = tf.cpu().numpy()
    assert np.all(full[n] == SENTINEL) and np.all(full[:n, K + 1:] == SENTINEL), "written outside the table"
    assert keep.cpu().numpy().tobytes() == tb.cpu().numpy().tobytes(), "the band changed"
    again, info2 = ctx.banded_pairsum(tb[:, :Wd], bandwidth=bandwidth)
    M = full[:n, :K + 1].copy()
    assert again.is_contiguous() and again.cpu().numpy().tobytes() == M.tobytes(), "two calls differ"
    assert info2.nonfinite == info.nonfinite and info.bandwidth == K and info.kernel_ms > 0
    return M, info, out


def scan_padded(torch, ctx, tM, split, lo, hi, min_side, eps, device_splits=False):
    """banded_omega into sentinel-padded outputs: the LdOmega after the layout
    checks."""
    G = len(split)
    om = torch.full((G + 2,), SENTINEL, dtype=torch.float64, device="cuda:0")
    zn = torch.full((G + 2,), SENTINEL, dtype=torch.float64, device="cuda:0")
    le = torch.full((G + 2,), ISENT, dtype=torch.int32, device="cuda:0")
    ri = torch.full((G + 2,), ISENT, dtype=torch.int32, device="cuda:0")
    out = {"omega": om[1:G + 1], "zns": zn[1:G + 1], "left": le[1:G + 1], "right": ri[1:G + 1]}
    if device_splits:
        split, lo, hi = (torch.from_numpy(np.asarray(x, dtype=np.uint32).view(np.int32)).cuda() for x in (split, lo, hi))
    res = ctx.banded_omega(tM, split, lo, hi, min_side, eps, out=out)
    for t, s in ((om, SENTINEL), (zn, SENTINEL), (le, ISENT), (ri, ISENT)):
        h = t.cpu().numpy()
        assert h[0] == s and h[-1] == s, "written outside the outputs"
    assert res.kernel_ms > 0
    return res


def assert_same(got, want, what):
    assert got.omega.tobytes() == want.omega.tobytes(), (what, "omega", np.flatnonzero(
        got.omega.view(np.uint64) != want.omega.view(np.uint64))[:5].tolist())
    assert got.zns.tobytes() == want.zns.tobytes(), (what, "zns")
    assert np.array_equal(got.left, want.left) and np.array_equal(got.right, want.right), (what, "borders")
    assert (got.evaluated, got.skipped) == (want.evaluated, want.skipped), (what, "counts")
    for f in ("split", "lo", "hi"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), (what, f)


@functools.lru_cache(maxsize=None)
def host_table(n, K, dtype):
    import weightedld_amd as W
    M = W.banded_pairsum_host(r2_band_case(n, K, dtype)[0])
    M.setflags(write=False)
    return M


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("n,K", PAIRSUM_SHAPES)
def test_pairsum(W, torch, ctx, n, K, dtype):
    B, planted = r2_band_case(n, K, dtype)
    M, info, _ = pairsum_strided(torch, ctx, B)
    want = host_table(n, K, dtype)
    assert M.tobytes() == want.tobytes(), np.argwhere(M.view(np.uint64) != want.view(np.uint64))[:5].tolist()
    assert info.nonfinite == planted


def test_pairsum_narrower_bandwidth(W, torch, ctx):
    B, _ = r2_band_case(130, 129)
    for Kn in (0, 1, 20, 64):
        M, info, _ = pairsum_strided(torch, ctx, B, bandwidth=Kn)
        assert M.shape == (130, Kn + 1) and M.tobytes() == W.banded_pairsum_host(B[:, :Kn + 1]).tobytes()
        assert info.nonfinite == W.banded_nonfinite_host(B[:, :Kn + 1])


@pytest.mark.parametrize("n,K", [s for s in PAIRSUM_SHAPES if s[0] >= 2])
def test_scan_every_split(W, torch, ctx, n, K):
    B, _ = r2_band_case(n, K)
    M, _, tM = pairsum_strided(torch, ctx, B)
    assert M.tobytes() == host_table(n, K, "float32").tobytes()
    for max_side in (2, 3, 33, 100):
        split, lo, hi = every_split(n, K, max_side)
        for min_side in (2, 5):
            got = scan_padded(torch, ctx, tM, split, lo, hi, min_side, 1e-5)
            assert_same(got, W.banded_omega_host(M, split, lo, hi, min_side, 1e-5), (n, K, max_side, min_side))


def test_scan_eps_zero_and_skips(W, torch, ctx):
    B = zero_cross_case()
    M, info, tM = pairsum_strided(torch, ctx, B)
    assert info.nonfinite == 0 and M.tobytes() == W.banded_pairsum_host(B).tobytes()
    split, lo, hi = every_split(40, 39, 20)
    for eps in (1e-5, 0.0):
        got = scan_padded(torch, ctx, tM, split, lo, hi, 2, eps)
        assert_same(got, W.banded_omega_host(M, split, lo, hi, 2, eps), ("zero cross block", eps))
        if eps == 0.0:
            assert got.skipped > 0 and got.evaluated > 0
            assert np.isnan(got.omega[19]) and got.left[19] == W.OMEGA_NONE and got.right[19] == W.OMEGA_NONE
        else:
            assert got.skipped == 0


def test_scan_split_lists(W, torch, ctx):
    n, K = 600, 200
    B, _ = r2_band_case(n, K)
    M, _, tM = pairsum_strided(torch, ctx, B)
    split, lo, hi = every_split(n, K, 100)
    # one split; the split at c = 0 (no left flank of two sites: NaN)
    for g in (0, 311):
        got = scan_padded(torch, ctx, tM, split[g:g + 1], lo[g:g + 1], hi[g:g + 1], 2, 1e-5)
        assert_same(got, W.banded_omega_host(M, split[g:g + 1], lo[g:g + 1], hi[g:g + 1], 2, 1e-5), ("one split", g))
        assert np.isnan(got.omega[0]) == (g == 0) and (got.left[0] == W.OMEGA_NONE) == (g == 0)
    # 599 splits, unsorted with repeats, c = 0 among them, as device tensors
    rng = np.random.default_rng(0x599)
    pick = rng.integers(0, n - 1, size=599)
    pick[7] = pick[8] = 0
    pick[100:110] = 431
    got = scan_padded(torch, ctx, tM, split[pick], lo[pick], hi[pick], 5, 1e-5, device_splits=True)
    want = W.banded_omega_host(M, split[pick], lo[pick], hi[pick], 5, 1e-5)
    assert_same(got, want, "599 unsorted splits")
    assert np.isnan(got.omega[7]) and got.left[7] == W.OMEGA_NONE
    assert len(set(got.omega[100:110].tobytes()[i:i + 8] for i in range(0, 80, 8))) == 1, "repeated splits agree"


def test_scan_tie_and_planted_sweep(W, torch, ctx):
    M, _, tM = pairsum_strided(torch, ctx, tie_case())
    got = scan_padded(torch, ctx, tM, [9], [5], [14], 2, 1e-5)
    assert got.omega[0] == 0.5 / (0.5 + 1e-5) and (got.left[0], got.right[0]) == (5, 11)
    assert got.evaluated == 16 and got.skipped == 0 and got.zns[0] == 0.5
    assert_same(got, W.banded_omega_host(M, [9], [5], [14], 2, 1e-5), "tie")
    B = sweep_case()
    M, _, tM = pairsum_strided(torch, ctx, B)
    _, split, lo, hi = W.omega_splits(None, 120, 0, 40)
    got = scan_padded(torch, ctx, tM, split, lo, hi, 2, 1e-5)
    assert_same(got, W.banded_omega_host(M, split, lo, hi, 2, 1e-5), "planted sweep")
    assert split[int(np.nanargmax(got.omega))] == 59


def test_refusals_and_state(W, torch, ctx):
    from weightedld_amd._lib import BandedOmegaInfoC, BandedPairsumInfoC, lib
    Lb = lib()
    ARG, STATE = -1, -7
    n, K = 130, 20
    B = np.ascontiguousarray(r2_band_case(130, 129)[0][:, :K + 1])
    band = torch.from_numpy(B).cuda()
    S = torch.zeros((n, K + 1), dtype=torch.float64, device="cuda:0")
    pi, oi = BandedPairsumInfoC(), BandedOmegaInfoC()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    _, split, lo, hi = W.omega_splits(None, n, 0, 10)
    G = len(split)
    ts, tl, th = (torch.from_numpy(x.view(np.int32)).cuda() for x in (split, lo, hi))
    o_om, o_zn = (torch.full((G,), SENTINEL, dtype=torch.float64, device="cuda:0") for _ in range(2))
    o_le, o_ri = (torch.full((G,), ISENT, dtype=torch.int32, device="cuda:0") for _ in range(2))

    def ps(c=ctx, b=p(band), bd=0, ld=K + 1, nn=n, k=K, s=p(S), lds=K + 1, o=ctypes.byref(pi)):
        return Lb.wld_banded_pairsum_device(c._h, b, bd, ld, nn, k, s, lds, o)

    def om(c=ctx, s=p(S), lds=K + 1, nn=n, k=K, sp=p(ts), l=p(tl), h=p(th), g=G, ms=2, eps=1e-5, a=p(o_om), b=p(o_le),
           r=p(o_ri), z=p(o_zn), o=ctypes.byref(oi)):
        return Lb.wld_banded_omega_device(c._h, s, lds, nn, k, sp, l, h, g, ms, eps, a, b, r, z, o)

    assert ps() == 0 and pi.n_sites == n and pi.bandwidth == K and pi.nonfinite == W.banded_nonfinite_host(B)
    assert om() == 0 and oi.n_splits == G and oi.evaluated > 0
    assert ps(b=None) == ARG and ps(s=None) == ARG and ps(o=None) == ARG, "null pointers"
    assert ps(nn=0) == ARG and ps(ld=K) == ARG and ps(lds=K) == ARG
    assert ps(bd=2) == ARG and ps(bd=-1) == ARG, "unknown dtypes"
    both = torch.zeros(n * (K + 1) * 2 + 8, dtype=torch.float64, device="cuda:0")
    assert ps(b=ctypes.c_void_p(both.data_ptr() + 16), s=p(both)) == ARG, "the sums overlap the band"
    assert ps(b=p(both), s=ctypes.c_void_p(both.data_ptr() + 4 * ((n - 1) * (K + 1) + K))) == ARG, "by one element"
    assert ps(b=p(both), s=ctypes.c_void_p(both.data_ptr() + 8 * ((n * (K + 1) * 4 + 7) // 8))) == 0, "adjacent is fine"
    assert Lb.wld_banded_pairsum_device(None, p(band), 0, K + 1, n, K, p(S), K + 1, ctypes.byref(pi)) == ARG
    for kw in ({"s": None}, {"sp": None}, {"l": None}, {"h": None}, {"a": None}, {"b": None}, {"r": None}, {"z": None},
               {"o": None}, {"nn": 0}, {"g": 0}, {"lds": K}, {"ms": 1}, {"ms": 0}, {"eps": -1e-9}, {"eps": float("nan")},
               {"eps": float("inf")}):
        assert om(**kw) == ARG, kw
    # a bad split is found on the device, named, and nothing is written
    before = (o_om.clone(), o_le.clone())
    for what, arr, g, value in (("hi past the last site", th, 3, n), ("lo above the split", tl, 5, int(split[5]) + 1),
                                ("split at hi", ts, 9, int(hi[9])), ("wider than the band", tl, G - 1, 0)):
        keep = arr.clone()
        o_om.fill_(SENTINEL)
        arr[g] = value
        assert om() == ARG and ("split %d " % g) in Lb.wld_last_error().decode(), what
        assert bool((o_om == SENTINEL).all()), (what, "nothing is written")
        arr.copy_(keep)
    assert om() == 0 and o_om.cpu().numpy().tobytes() == before[0].cpu().numpy().tobytes()
    assert Lb.wld_banded_omega_device(None, p(S), K + 1, n, K, p(ts), p(tl), p(th), G, 2, 1e-5, p(o_om), p(o_le), p(o_ri),
                                      p(o_zn), ctypes.byref(oi)) == ARG

    c = case1()
    busy = W.Context(0)
    busy.load(c.buf, c.w)
    n_rows = busy.run(0.05)
    rows, stats = busy.rows(), busy.stats()
    assert ps(c=busy) == 0 and om(c=busy) == 0
    after = busy.rows()
    assert len(after) == n_rows and busy.stats() == stats, "wld_last_stats stays"
    for f in ("site_a", "site_b", "d", "d_prime", "r2"):
        assert np.array_equal(getattr(after, f), getattr(rows, f)), f
    busy.run_chunks_async(0.05)
    assert ps(c=busy) == STATE and om(c=busy) == STATE, "during a run"
    with pytest.raises(W.WldError):
        busy.run_omega(max_side=10)
    busy.run_wait()
    assert ps(c=busy) == 0 and om(c=busy) == 0
    busy.close()
    grp = W.Context(devices=[0, 0])
    assert ps(c=grp) == STATE and om(c=grp) == STATE, "a device group"
    grp.load(c.buf, c.w)
    with pytest.raises(W.WldError):
        grp.run_omega(max_side=10)
    grp.close()
    # Python: refused before any device call
    for args, kw in (((band.cpu(),), {}), ((band.double(),), {}), ((band[:, ::2],), {}), ((band[0],), {}),
                     ((band,), {"bandwidth": K + 1}), ((band,), {"out": torch.zeros((n, K + 1), device="cuda:0")}),
                     ((band,), {"out": torch.zeros((n, K), dtype=torch.float64, device="cuda:0")})):
        with pytest.raises(ValueError):
            ctx.banded_pairsum(*args, **kw)
    for args, kw in (((S.float(), split, lo, hi), {}), ((S.cpu(), split, lo, hi), {}), ((S[:, ::2], split, lo, hi), {}),
                     ((S, split, lo, hi + 200), {}), ((S, split[:-1], lo, hi), {}), ((S, ts, lo, hi), {}),
                     ((S, ts.long(), tl.long(), th.long()), {}), ((S, split, lo, hi), {"min_side": 1}),
                     ((S, split, lo, hi), {"eps": -1.0}), ((S, ts, tl, th), {"min_side": 1}),
                     ((S, split, lo, hi), {"out": {"omega": o_om}}),
                     ((S, split, lo, hi), {"out": {"omega": o_om, "zns": o_zn, "left": o_le, "right": o_ri[:-1]}})):
        with pytest.raises(ValueError):
            ctx.banded_omega(*args, **kw)


def test_case1_end_to_end(W, torch):
    c, pos = case1(), case1_map()
    ctx = W.Context(0)
    ctx.load(c.buf, c.w, pos)
    n_rows = ctx.run(0.05)
    rows, stats = ctx.rows(), ctx.stats()
    ctx.set_window(0, 65)
    band, binfo = ctx.run_matrix_banded(stat="r2", zero_missing=True)
    assert band.shape == (600, 66) and np.isfinite(band).all()
    assert not band[5, 1:].any() and not band[np.arange(0, 5), 5 - np.arange(0, 5)].any(), "the None-pair site 5 gives 0"
    M = W.banded_pairsum_host(band)
    for n_grid, D in ((0, None), (50, None), (0, 40)):
        res = ctx.run_omega(n_grid, 33, 2, D, 1e-5)
        position, split, lo, hi = W.omega_splits(pos, None, n_grid, 33, D)
        assert np.array_equal(res.position, position) and res.n_sites == 600 and res.bandwidth == 65
        want = W.banded_omega_host(M, split, lo, hi, 2, 1e-5)
        assert_same(res, want, ("run_omega", n_grid, D))
        assert res.band.pairs == binfo.pairs and res.band.none_pairs == binfo.none_pairs
        assert res.band.counted_pairs == binfo.counted_pairs and res.sums.nonfinite == 0 and res.sums.bandwidth == 65
        assert res.kernel_ms > 0 and res.band.kernel_ms > 0 and res.sums.kernel_ms > 0
    # float16 storage of the band: the table of the rounded band
    band16, _ = ctx.run_matrix_banded(stat="r2", zero_missing=True, dtype="float16")
    _, split, lo, hi = W.omega_splits(pos, None, 0, 33)
    assert_same(ctx.run_omega(0, 33, dtype="float16"),
                W.banded_omega_host(W.banded_pairsum_host(band16), split, lo, hi), "float16 band")
    # the device table against an fsum over run_matrix's dense r2 (None pairs: 0)
    ctx.set_window(0, 0)
    dense, _ = ctx.run_matrix(stat="r2", zero_missing=True)
    ctx.set_window(0, 65)
    D64 = np.triu(dense.astype(np.float64), 1)
    assert not D64[5].any() and not D64[:, 5].any()
    tM, _ = ctx.banded_pairsum(torch.from_numpy(band).cuda())
    Md = tM.cpu().numpy()
    assert Md.tobytes() == M.tobytes()
    worst = 0.0
    for j in range(0, 600, 7):
        for k in (1, 2, 33, 65):
            if j + k >= 600:
                continue
            exact = math.fsum(D64[j:j + k + 1, j:j + k + 1].ravel().tolist())
            bound = gamma((k + 1) * k // 2 - 1) * exact
            assert abs(Md[j, k] - exact) <= bound, (j, k, Md[j, k], exact)
            worst = max(worst, abs(Md[j, k] - exact) / bound if bound else 0.0)
    print("case1: worst |M - fsum| / bound = %.4f" % worst)
    # a window that is too narrow is refused, and the message names the width needed
    ctx.set_window(0, 64)
    with pytest.raises(W.WldError, match="max_sites 65"):
        ctx.run_omega(0, 33)
    ctx.set_window(0, 0)
    # rows and wld_last_stats are undisturbed, and the next row run is unaffected
    after = ctx.rows()
    assert len(after) == n_rows and ctx.stats() == stats
    for f in ("site_a", "site_b", "d", "d_prime", "r2"):
        assert np.array_equal(getattr(after, f), getattr(rows, f)), f
    assert ctx.run(0.05) == n_rows
    again = ctx.rows()
    for f in ("site_a", "site_b", "d", "d_prime", "r2"):
        assert np.array_equal(getattr(again, f), getattr(rows, f)), f
    # ld_omega sets the window itself and restores the context's own
    ss = W.SiteSet.from_buffer(c.buf, site_map=pos)
    ctx.set_window(0, 7)
    res = W.ld_omega(ss, c.w, 0, 33, ctx=ctx)
    assert ctx.window() == (0, 7)
    position, split, lo, hi = W.omega_splits(pos, None, 0, 33)
    assert_same(res, W.banded_omega_host(M, split, lo, hi), "ld_omega")
    assert np.array_equal(res.site_map, pos) and np.array_equal(res.position, position)
    pa, pb = res.parents(pos)
    ok = ~np.isnan(res.omega)
    assert np.array_equal(pa[ok], pos[res.left[ok].astype(np.int64)]) and np.all(pa[~ok] == np.uint64(2 ** 64 - 1))
    ctx.close()


def _cli_rows(tmp_path, args, want, site_map):
    """The CLI's TSV for `args` against an LdOmega: every line after a %.17g
    round trip; returns the count of lines with a value."""
    tsv = str(tmp_path / "o.tsv")
    out = subprocess.run([CLI, *args, "--omega-output", tsv], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = open(tsv).read().splitlines()
    os.remove(tsv)
    assert lines[0].split("\t") == ["position", "left", "right", "omega", "zns"]
    rows = want.rows(site_map)
    assert len(lines) == 1 + len(rows)
    valued = 0
    for line, (pos, a, b, om, zn) in zip(lines[1:], rows):
        f = line.split("\t")
        assert int(f[0]) == pos
        if math.isnan(om):
            assert f[1:4] == ["NA", "NA", "nan"]
        else:
            valued += 1
            assert (int(f[1]), int(f[2])) == (a, b)
            assert np.float64(f[3]).tobytes() == np.float64(om).tobytes() and f[3] == "%.17g" % om
        assert np.float64(f[4]).tobytes() == np.float64(zn).tobytes() and f[4] == "%.17g" % zn
    return valued


def test_cli_tsv_vcf(W, tmp_path):
    """(VCF input takes no site filter; the fixture holds five sites, so flanks of up to three)"""
    path = os.path.join(FIXTURES, "t7_1000genome.vcf")
    vcf = W.read_vcf(path)
    w = W.henikoff_weights(vcf)
    ctx = W.Context(0)
    assert vcf.n_sites() == 5
    base = ["--vcf-input", path, "--omega-max-side", "3"]
    assert _cli_rows(tmp_path, base, W.ld_omega(vcf, w, max_side=3, ctx=ctx), vcf.site_map) >= 2
    # flanks of three do not exist among five sites: every line is NA
    want = W.ld_omega(vcf, w, n_grid=9, max_side=3, min_side=3, max_distance=400, eps=0.001, ctx=ctx)
    assert np.isnan(want.omega).all()
    assert _cli_rows(tmp_path, base + ["--omega-grid", "9", "--omega-min-side", "3", "--omega-max-distance", "400",
                                       "--omega-eps", "0.001"], want, vcf.site_map) == 0
    # --max-sites given and too narrow: the library's refusal, no file
    tsv = str(tmp_path / "o.tsv")
    out = subprocess.run([CLI, *base, "--omega-output", tsv, "--max-sites", "3"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "max_sites 5" in out.stderr and not os.path.exists(tsv)
    ctx.close()


def test_cli_tsv_fasta(W, tmp_path):
    """A 500 x 40 alignment with a constant column after every third one: the
    filter drops those, so parent coordinates differ from site indices (a FASTA
    set's parent coordinate is the column in the unfiltered alignment)."""
    src, path = os.path.join(SYNTH, "synth_n500_l40.fasta"), str(tmp_path / "gapped.fasta")
    with open(src) as f, open(path, "w") as g:
        for line in f:
            t = line.rstrip("\n")
            g.write((t if t.startswith(">") else "".join(ch + ("A" if i % 3 == 2 else "") for i, ch in enumerate(t))) + "\n")
    kept = W.read_fasta(path).filter_sites_of_interest(0.8, 0.02, 0.5)
    parent = np.array([kept.parent_site_index(i) for i in range(kept.n_sites())], dtype=np.uint64)
    assert kept.n_sites() == 40 and np.any(np.diff(parent.astype(np.int64)) > 1)
    loaded_set = W.SiteSet.from_buffer(kept.buffer, site_map=parent)
    w = W.henikoff_weights(kept)
    ctx = W.Context(0)
    base = ["--fasta-input", path, "--omega-max-side", "8"]
    # every split: 39 lines, all but the first and the last with a value
    assert _cli_rows(tmp_path, base, W.ld_omega(loaded_set, w, max_side=8, ctx=ctx), parent) == 37
    want = W.ld_omega(loaded_set, w, n_grid=25, max_side=8, min_side=3, max_distance=9, eps=0.0, ctx=ctx)
    assert _cli_rows(tmp_path, base + ["--omega-grid", "25", "--omega-min-side", "3", "--omega-max-distance", "9",
                                       "--omega-eps", "0"], want, parent) == np.count_nonzero(~np.isnan(want.omega)) > 0
    # beside the pair output, with --gpu-prepass, and with a window the scan fits in
    pairs = str(tmp_path / "p.tsv")
    assert _cli_rows(tmp_path, base + ["--pair-output", pairs, "--gpu-prepass", "--max-sites", "15"],
                     W.ld_omega(loaded_set, w, max_side=8, ctx=ctx), parent) == 37
    assert os.path.getsize(pairs) > 0
    ctx.close()
