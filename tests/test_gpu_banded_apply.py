"""The band product (wld_banded_apply_device / Context.banded_apply): Y = S X on
the device for the symmetric matrix S of a band in run_matrix_banded's layout.

Bands are synthetic random values uploaded through torch, so the product is
tested apart from the pair pass; one case takes its band from
run_matrix_banded.  Every Y element is compared with math.fsum of its terms
(the f64 products, exact for float32 X, rounded once for float64 X) under

    float32 X:  |Y - exact| <=  n      2^-52 sum|term|
    float64 X:  |Y - exact| <= (n + 2) 2^-52 sum|term|

with n the element's term count.  X is mixed-sign and asymmetric in both
indices, so a misplaced or transposed block misses by whole terms.  NaN is
planted at every band position past the last site (i + k >= L) and in the
padding between rows: none may reach Y.
"""
import ctypes
import functools
import math

import numpy as np
import pytest

from test_gpu_summary import case1
from test_matrix_banded_api import band_case, cg_case, x_case

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
SHAPES = [(1, 0), (63, 5), (64, 64), (65, 63), (130, 129), (130, 400), (600, 65), (600, 200)]
COLS = [1, 5, 16, 17, 33]


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
    c = W.Context(0)  # the product needs no load
    yield c
    c.close()


def exact_product(S, X, K):
    """Per element of S X (S dense, symmetric, only |i - j| <= K used): the
    correctly rounded sum of its f64 products, the sum of their magnitudes
    and the term count."""
    L, C = X.shape
    S, X = S.astype(np.float64), X.astype(np.float64)
    exact, mag, n = np.zeros((L, C)), np.zeros((L, C)), np.zeros((L, 1))
    for i in range(L):
        lo, hi = max(0, i - K), min(L, i + K + 1)
        T = S[i, lo:hi, None] * X[lo:hi]  # one rounding per product
        n[i] = hi - lo
        for c in range(C):
            t = T[:, c].tolist()
            exact[i, c], mag[i, c] = math.fsum(t), math.fsum(map(abs, t))
    return exact, mag, n


@functools.lru_cache(maxsize=None)
def reference(W, L, K, xdt):
    """The band (float32; its values are exact in float16 too), X with the most
    columns, and exact_product of them: computed once per shape and X dtype."""
    B = band_case(L, K, 1000 * L + K)
    X = x_case(L, max(COLS), L + K, np.dtype(xdt))
    out = (B, X) + exact_product(W.banded_to_dense(B), X, K)
    for a in out:
        a.setflags(write=False)
    return out


def apply_strided(torch, ctx, B, X, bandwidth=None):
    """banded_apply on row-strided views with NaN / sentinel padding: returns Y
    (numpy) after checking that nothing outside Y's view was written."""
    L, Wd = B.shape
    C = X.shape[1]
    tb = torch.full((L, Wd + 3), float("nan"), dtype=getattr(torch, B.dtype.name), device="cuda:0")
    tb[:, :Wd] = torch.from_numpy(B)
    tx = torch.full((L, C + 2), float("nan"), dtype=getattr(torch, X.dtype.name), device="cuda:0")
    tx[:, :C] = torch.from_numpy(X)
    ty = torch.full((L + 1, C + 4), SENTINEL, dtype=torch.float64, device="cuda:0")
    out = ctx.banded_apply(tb[:, :Wd], tx[:, :C], out=ty[:L, :C], bandwidth=bandwidth)
    assert out.data_ptr() == ty.data_ptr()
    full = ty.cpu().numpy()
    assert np.all(full[L] == SENTINEL) and np.all(full[:L, C:] == SENTINEL), "written outside Y"
    again = ctx.banded_apply(tb[:, :Wd], tx[:, :C], bandwidth=bandwidth)
    assert again.is_contiguous() and again.cpu().numpy().tobytes() == full[:L, :C].tobytes(), "two calls differ"
    return full[:L, :C].copy()


def check(Y, exact, mag, n, extra, what):
    assert np.isfinite(Y).all(), (what, "a NaN past the last site reached Y")
    bound = (n + extra) * 2.0 ** -52 * mag
    diff = np.abs(Y - exact)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))
    print("%s: worst |diff| / bound = %.4f" % (what, ratio.max()))
    assert np.all(diff <= bound), (what, np.argwhere(diff > bound)[:5].tolist(), float(ratio.max()))


@pytest.mark.parametrize("n_cols", COLS)
@pytest.mark.parametrize("xdt", ["float32", "float64"])
@pytest.mark.parametrize("bdt", ["float32", "float16"])
@pytest.mark.parametrize("L,K", SHAPES)
def test_product_against_fsum(W, torch, ctx, L, K, bdt, xdt, n_cols):
    B, X, exact, mag, n = reference(W, L, K, xdt)
    Bt = B.astype(bdt)
    assert np.array_equal(Bt.astype(np.float32), B, equal_nan=True), "the band's values are exact in float16"
    Y = apply_strided(torch, ctx, Bt, X[:, :n_cols].copy())
    check(Y, exact[:, :n_cols], mag[:, :n_cols], n, 0 if xdt == "float32" else 2, (L, K, bdt, xdt, n_cols))
    assert np.abs(Y).max() > 0 or L == 1


def test_vector_and_narrower_bandwidth(W, torch, ctx):
    B, X, exact, mag, n = reference(W, 130, 129, "float32")
    tb, tx = torch.from_numpy(B.copy()).cuda(), torch.from_numpy(X[:, 3].copy()).cuda()
    y = ctx.banded_apply(tb, tx)
    assert y.shape == (130,) and y.dtype == torch.float64
    check(y.cpu().numpy()[:, None], exact[:, 3:4], mag[:, 3:4], n, 0, "a 1-D X")
    # bandwidth 20 of the same tensor: the first 21 columns, the rest ignored
    e20, m20, n20 = exact_product(W.banded_to_dense(B[:, :21]), X[:, :5], 20)
    Y = apply_strided(torch, ctx, B.copy(), X[:, :5].copy(), bandwidth=20)
    check(Y, e20, m20, n20, 0, "bandwidth 20 of 129")
    host = W.banded_matmul_host(B[:, :21], X[:, :5])
    assert np.abs(Y - host).max() <= 2 * (n20 * 2.0 ** -52 * m20).max()


def test_band_from_run_matrix_banded(W, torch):
    c = case1()
    ld_ctx = W.Context(0)
    ld_ctx.load(c.buf, c.w)
    ld_ctx.set_window(0, 65)
    band = torch.empty((600, 66), dtype=torch.float32, device="cuda:0")
    dense = torch.empty((600, 600), dtype=torch.float32, device="cuda:0")
    ld_ctx.run_matrix_banded(stat="r", zero_missing=True, out=band)
    ld_ctx.run_matrix(stat="r", zero_missing=True, out=dense)
    S = dense.cpu().numpy()
    assert np.isfinite(S).all() and np.array_equal(S, S.T)
    for xdt, extra in (("float32", 0), ("float64", 2)):
        X = x_case(600, 17, 9, np.dtype(xdt))
        Y = ld_ctx.banded_apply(band, torch.from_numpy(X).cuda()).cpu().numpy()
        exact, mag, n = exact_product(S, X, 65)
        check(Y, exact, mag, n, extra, ("case1 r, max_sites 65", xdt))
        assert np.abs(Y - S.astype(np.float64) @ X.astype(np.float64)).max() <= 2 * ((n + extra) * 2.0 ** -52 * mag).max()
    ld_ctx.close()


def test_cg_solve_on_the_device(W, torch, ctx):
    B, b, x_ref = cg_case()
    tb, tv = torch.from_numpy(B).cuda(), torch.from_numpy(b).cuda()
    x, it, res, ok = W.banded_cg_solve(ctx.banded_apply, tb, tv, tol=1e-10)
    assert ok and 0 < it < 300 and res <= 1e-10 and x.dtype == torch.float64 and x.is_cuda
    assert np.abs(x.cpu().numpy() - x_ref).max() <= 1e-9 * np.abs(x_ref).max()


def test_refusals(W, torch, ctx):
    from weightedld_amd._lib import lib
    Lb = lib()
    ARG, STATE = -1, -7
    band = torch.zeros((130, 21), dtype=torch.float32, device="cuda:0")
    X = torch.zeros((130, 5), dtype=torch.float32, device="cuda:0")
    Y = torch.zeros((130, 5), dtype=torch.float64, device="cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(c=ctx, b=p(band), bd=0, ld=21, n=130, K=20, x=p(X), xd=0, ldx=5, nc=5, y=p(Y), ldy=5):
        return Lb.wld_banded_apply_device(c._h, b, bd, ld, n, K, x, xd, ldx, nc, y, ldy)

    assert call() == 0
    assert call(b=None) == ARG and call(x=None) == ARG and call(y=None) == ARG, "null pointers"
    assert call(nc=0) == ARG and call(n=0) == ARG
    assert call(ld=20) == ARG, "ld below bandwidth + 1"
    assert call(ldx=4) == ARG and call(ldy=4) == ARG
    assert call(bd=2) == ARG and call(bd=-1) == ARG and call(xd=2) == ARG, "unknown dtypes"
    assert Lb.wld_banded_apply_device(None, p(band), 0, 21, 130, 20, p(X), 0, 5, 5, p(Y), 5) == ARG
    c = case1()
    busy = W.Context(0)
    busy.load(c.buf, c.w)
    busy.run_chunks_async(0.05)
    assert call(c=busy) == STATE, "during a run"
    busy.run_wait()
    assert call(c=busy) == 0
    busy.close()
    grp = W.Context(devices=[0, 0])
    assert call(c=grp) == STATE, "a device group"
    grp.close()
    # Python: refused before any device call
    for args, kw in (((band.cpu(), X), {}), ((band, X.cpu()), {}), ((band.double(), X), {}), ((band, X.half()), {}),
                     ((band, X[:100]), {}), ((band[:, ::2], X), {}), ((band, X[:, ::2]), {}), ((band[0], X), {}),
                     ((band, X), {"bandwidth": 21}), ((band, X), {"bandwidth": -1}),
                     ((band, X), {"out": torch.zeros((130, 5), dtype=torch.float32, device="cuda:0")}),
                     ((band, X), {"out": torch.zeros((130, 4), dtype=torch.float64, device="cuda:0")}),
                     ((band, X), {"out": torch.zeros((130, 5), dtype=torch.float64)}),
                     ((band.cpu().numpy(), X), {})):
        with pytest.raises(ValueError):
            ctx.banded_apply(*args, **kw)
