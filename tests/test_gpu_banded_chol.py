"""The banded Cholesky factorisation and its triangular solves on the device
(wld_banded_cholesky_device / wld_banded_solve_device; Context.banded_cholesky
and Context.banded_solve).

Matrices are built in numpy (tests/test_banded_chol_api.py: a diagonally
dominant random band, the band of a Gram matrix T^T T under a small ridge and
a random diag) or come from run_matrix_banded (case1's r under max_sites 65,
ridge max(0, -lambda_min) + 0.05 with lambda_min from numpy's eigvalsh of the
dense matrix).  With u = 2^-53, m the term count of an element or row and the
device's own U expanded to dense f64, the checks are

    factor      |A - U^T U|_ij <= (m_ij + 1) 2^-52 (|U|^T |U|)_ij   for |i - j| <= K
                (Higham, Theorem 10.3: gamma_{m+1} in any summation order, plus
                the m u of the test's own f64 product); outside the band U^T U
                is exactly 0 by structure
    half solves |b - U^T y| <= (m + 1) 2^-52 |U^T| |y|,  |y - U x| <= (m + 1) 2^-52 |U| |x|
                (Theorem 8.5, order independent, plus the test's product)
    full solve  |b - A x| <= (3 m + 3) 2^-52 |U^T| |U| |x|   (Theorem 10.4),
                m = min(n, K + 1), the longest inner product of the factorisation
                and of either solve

all derived, none measured.  b is mixed-sign and asymmetric (x_case), so a
misplaced block misses by whole terms.  Bands and outputs are strided views
with NaN past the last site and in the padding, and sentinels around the
outputs: nothing outside the views may be written.

Worst |diff| / bound seen on MI355X (printed per case): factor 0.46, forward
0.44, backward 0.46, full solve 0.16.
"""
import ctypes
import functools

import numpy as np
import pytest

from test_banded_chol_api import BAD, SHAPES, bad_case, dominant_case, gram_case, shifted_dense, upper_dense
from test_gpu_summary import case1
from test_matrix_banded_api import x_case

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
COLS = [1, 5, 17, 64, 65]
MODES = ["forward", "backward", "full"]


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
    c = W.Context(0)  # neither call needs a load
    yield c
    c.close()


def factor_strided(torch, ctx, B, ridge, diag, bandwidth=None):
    """banded_cholesky on row-strided views with NaN / sentinel padding: returns
    (U band as numpy, info, the device factor view) after the layout checks."""
    n, Wd = B.shape
    K = Wd - 1 if bandwidth is None else bandwidth
    tb = torch.full((n, Wd + 3), float("nan"), dtype=getattr(torch, B.dtype.name), device="cuda:0")
    tb[:, :Wd] = torch.from_numpy(B)
    keep = tb.clone()
    td = None if diag is None else torch.from_numpy(np.asarray(diag, dtype=np.float64)).cuda()
    tf = torch.full((n + 1, K + 1 + 4), SENTINEL, dtype=torch.float64, device="cuda:0")
    out, info = ctx.banded_cholesky(tb[:, :Wd], ridge, td, out=tf[:n, :K + 1], bandwidth=bandwidth)
    assert out.data_ptr() == tf.data_ptr()
    full = tf.cpu().numpy()
    assert np.all(full[n] == SENTINEL) and np.all(full[:n, K + 1:] == SENTINEL), "written outside the factor"
    assert keep.cpu().numpy().tobytes() == tb.cpu().numpy().tobytes(), "the band changed"
    again, info2 = ctx.banded_cholesky(tb[:, :Wd], ridge, td, bandwidth=bandwidth)
    U = full[:n, :K + 1].copy()
    assert info2.first_bad == info.first_bad
    if info.ok:
        assert again.is_contiguous() and again.cpu().numpy().tobytes() == U.tobytes(), "two calls differ"
        assert info2.min_pivot == info.min_pivot
    return U, info, out


def solve_strided(torch, ctx, tf, b, mode):
    """banded_solve into a strided view with sentinels: the solution (numpy)."""
    n, C = b.shape
    tb = torch.from_numpy(np.array(b)).cuda()
    tx = torch.full((n + 1, C + 3), SENTINEL, dtype=torch.float64, device="cuda:0")
    out = ctx.banded_solve(tf, tb, mode, out=tx[:n, :C])
    assert out.data_ptr() == tx.data_ptr()
    full = tx.cpu().numpy()
    assert np.all(full[n] == SENTINEL) and np.all(full[:n, C:] == SENTINEL), "written outside the solution"
    assert np.array_equal(tb.cpu().numpy(), b), "b changed"
    again = ctx.banded_solve(tf, tb, mode)
    assert again.is_contiguous() and again.dtype == torch.float64
    assert again.cpu().numpy().tobytes() == full[:n, :C].tobytes(), "two calls differ"
    return full[:n, :C].copy()


def worst(diff, bound, what):
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))
    print("%s: worst |diff| / bound = %.4f" % (what, ratio.max()))
    assert np.all(diff <= bound), (what, np.argwhere(diff > bound)[:5].tolist(), float(ratio.max()))


def check_factor(U, A, K, what):
    n = A.shape[0]
    r, k = np.arange(n)[:, None], np.arange(U.shape[1])[None, :]
    tails = U[r + k >= n]
    assert not tails.any() and not np.signbit(tails).any(), (what, "tails are +0.0")
    assert np.isfinite(U).all() and np.all(U[:, 0] > 0), (what, "U[i, 0] > 0")
    Ud = upper_dense(U)
    G, Gabs = Ud.T @ Ud, np.abs(Ud).T @ np.abs(Ud)
    i, j = np.indices((n, n))
    inside = np.abs(i - j) <= K
    assert not G[~inside].any(), (what, "U^T U is exactly 0 outside the band")
    m = np.minimum(i, j) - np.maximum(0, np.maximum(i, j) - K) + 1
    worst(np.abs(A - G)[inside], ((m + 1) * 2.0 ** -52 * Gabs)[inside], (what, "factor"))
    return Ud


def check_solves(torch, ctx, tf, Ud, A, K, b, what):
    n = A.shape[0]
    rows = np.arange(n)[:, None]
    m_fwd = rows - np.maximum(0, rows - K) + 1           # terms of row i of U^T
    m_bwd = np.minimum(n - 1, rows + K) - rows + 1       # terms of row i of U
    m_full = min(n, K + 1)
    aU = np.abs(Ud)
    for C in COLS:
        bc = np.ascontiguousarray(b[:, :C])
        y = solve_strided(torch, ctx, tf, bc, "forward")
        worst(np.abs(bc - Ud.T @ y), (m_fwd + 1) * 2.0 ** -52 * (aU.T @ np.abs(y)), (what, C, "forward"))
        x = solve_strided(torch, ctx, tf, y, "backward")
        worst(np.abs(y - Ud @ x), (m_bwd + 1) * 2.0 ** -52 * (aU @ np.abs(x)), (what, C, "backward"))
        full = solve_strided(torch, ctx, tf, bc, "full")
        assert full.tobytes() == x.tobytes(), (what, C, "full is forward, then backward")
        worst(np.abs(bc - A @ full), (3 * m_full + 3) * 2.0 ** -52 * (aU.T @ (aU @ np.abs(full))), (what, C, "full"))
        assert np.isfinite(full).all()


@functools.lru_cache(maxsize=None)
def rhs(n):
    b = x_case(n, max(COLS), n, np.float64)
    b.setflags(write=False)
    return b


@pytest.mark.parametrize("kind", ["dominant", "gram"])
@pytest.mark.parametrize("n,K", SHAPES)
def test_factor_and_solves(W, torch, ctx, n, K, kind):
    B, ridge, diag = dominant_case(n, K) if kind == "dominant" else gram_case(n, K)
    A = shifted_dense(B, ridge, diag)
    np.linalg.cholesky(A)  # the guard: the dense matrix is positive definite
    U, info, tf = factor_strided(torch, ctx, B, ridge, diag)
    assert info.ok and info.first_bad is None and info.kernel_ms > 0
    assert info.min_pivot == U[:, 0].min()
    Ud = check_factor(U, A, K, (n, K, kind))
    check_solves(torch, ctx, tf, Ud, A, K, rhs(n), (n, K, kind))
    host, none = W.banded_cholesky_host(B, ridge, diag)
    assert none is None and np.allclose(U, host, rtol=1e-6, atol=1e-9)
    assert abs(W.banded_logdet(tf) - W.banded_logdet(U)) <= 1e-9 * max(1.0, abs(W.banded_logdet(U)))


def test_float16_band_vector_and_narrower_bandwidth(W, torch, ctx):
    n, K = 130, 129
    B, ridge, _ = dominant_case(n, K)  # (its values are exact in float16)
    B16 = B.astype(np.float16)
    U32, _, _ = factor_strided(torch, ctx, B, ridge, None)
    U16, info, tf = factor_strided(torch, ctx, B16, ridge, None)
    assert info.ok and U16.tobytes() == U32.tobytes()
    # a 1-D float32 b: converted, a new float64 [n] tensor
    b = rhs(n)[:, 3].astype(np.float32)
    x = ctx.banded_solve(tf, torch.from_numpy(b).cuda())
    assert x.shape == (n,) and x.dtype == torch.float64
    ref = solve_strided(torch, ctx, tf, b.astype(np.float64)[:, None], "full")
    assert x.cpu().numpy().tobytes() == ref[:, 0].tobytes()
    # bandwidth 20 of the same tensor: the first 21 columns, the rest ignored
    B20 = B[:, :21]
    ridge20 = dominant_case(n, K)[1]
    U20, info20, tf20 = factor_strided(torch, ctx, B, ridge20, None, bandwidth=20)
    assert info20.ok and U20.shape == (n, 21)
    A20 = shifted_dense(B20, ridge20)
    Ud = check_factor(U20, A20, 20, "bandwidth 20 of 129")
    check_solves(torch, ctx, tf20, Ud, A20, 20, rhs(n), "bandwidth 20 of 129")


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_ld_band_and_cg(W, torch, dtype):
    c = case1()
    ld_ctx = W.Context(0)
    ld_ctx.load(c.buf, c.w)
    ld_ctx.set_window(0, 65)
    band, _ = ld_ctx.run_matrix_banded(stat="r", zero_missing=True, dtype=dtype,
                                       out=torch.empty((600, 66), dtype=getattr(torch, dtype), device="cuda:0"))
    B = band.cpu().numpy()
    S = W.banded_to_dense(B).astype(np.float64)
    assert np.isfinite(S).all()
    lam = np.linalg.eigvalsh(S)
    ridge = max(0.0, -float(lam[0])) + 0.05
    A = shifted_dense(B, ridge)
    np.linalg.cholesky(A)
    U, info, tf = factor_strided(torch, ld_ctx, B, ridge, None)
    assert info.ok
    Ud = check_factor(U, A, 65, ("case1 r, max_sites 65", dtype))
    check_solves(torch, ld_ctx, tf, Ud, A, 65, rhs(600), ("case1 r, max_sites 65", dtype))
    # against conjugate gradients on the device, one right-hand side: they agree
    # to CG's own reported residual times |A^-1| (x - x_cg = A^-1 (b - A x_cg)
    # for the exact x).  The second check needs no exact x: with both true
    # residuals recomputed on the host in f64, x - x_cg = A^-1 ((b - A x_cg) -
    # (b - A x)), each residual known to the rounding of its own product,
    # (m + 2) 2^-53 (|A| |x| + |b|) per element with m <= 2 K + 1 terms.
    bh = rhs(600)[:, 2].copy()
    b = torch.from_numpy(bh).cuda()
    x_cg, it, res, ok = W.banded_cg_solve(ld_ctx.banded_apply, band, b, ridge=ridge, tol=1e-10)
    assert ok and res <= 1e-10
    x = ld_ctx.banded_solve(tf, b)
    inv_norm = 1.0 / float(np.linalg.eigvalsh(A)[0])
    err = float((x - x_cg).norm())
    bound = res * float(b.norm()) * inv_norm
    xh, xch = x.cpu().numpy(), x_cg.cpu().numpy()
    own = sum(np.linalg.norm((2 * 65 + 3) * 2.0 ** -53 * (np.abs(A) @ np.abs(v) + np.abs(bh))) for v in (xh, xch))
    true = inv_norm * (np.linalg.norm(bh - A @ xch) + np.linalg.norm(bh - A @ xh) + own)
    print("chol vs cg (%s): |x - x_cg| = %.3e, residual x |A^-1| = %.3e, from both true residuals %.3e, %d iterations" %
          (dtype, err, bound, true, it))
    assert err <= bound
    assert err <= true
    ld_ctx.close()


@functools.lru_cache(maxsize=None)
def good_factor_bytes(n, K):
    import torch
    import weightedld_amd as W
    B, ridge, _ = dominant_case(n, K)
    c = W.Context(0)
    U, info = c.banded_cholesky(torch.from_numpy(B).cuda(), ridge)
    c.close()
    assert info.ok
    return U.cpu().numpy()


@pytest.mark.parametrize("n,K,p", BAD)
def test_not_positive_definite(W, torch, ctx, n, K, p):
    U_good = good_factor_bytes(n, K)
    for value in (-1.0, float("nan")):
        B, ridge, _ = bad_case(n, K, p, value)
        U, info, _ = factor_strided(torch, ctx, B, ridge, None)  # (WLD_OK: no exception)
        assert not info.ok and info.first_bad == p, (value, info)
        lead = 64 * (p // 64)
        assert U[:lead].tobytes() == U_good[:lead].tobytes(), "the rows of the leading blocks are the good matrix's"
        if lead:
            assert info.min_pivot <= U_good[:lead, 0].min()
    # the call after a failed one, on the good matrix, is unaffected
    B, ridge, _ = dominant_case(n, K)
    U, info, _ = factor_strided(torch, ctx, B, ridge, None)
    assert info.ok and U.tobytes() == U_good.tobytes()


def test_refusals_and_state(W, torch, ctx):
    from weightedld_amd._lib import BandedCholInfoC, lib
    Lb = lib()
    ARG, STATE = -1, -7
    n, K = 130, 20
    B, ridge, _ = dominant_case(n, K)
    band = torch.from_numpy(B).cuda()
    F = torch.zeros((n, K + 1), dtype=torch.float64, device="cuda:0")
    rhs_t = torch.ones((n, 5), dtype=torch.float64, device="cuda:0")
    info = BandedCholInfoC()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def fac(c=ctx, b=p(band), bd=0, ld=K + 1, nn=n, k=K, r=ridge, d=None, f=p(F), ldf=K + 1, o=ctypes.byref(info)):
        return Lb.wld_banded_cholesky_device(c._h, b, bd, ld, nn, k, r, d, f, ldf, o)

    def sol(c=ctx, f=p(F), ldf=K + 1, nn=n, k=K, mode=0, b=p(rhs_t), ldb=5, nc=5, ms=None):
        return Lb.wld_banded_solve_device(c._h, f, ldf, nn, k, mode, b, ldb, nc, ms)

    assert fac() == 0 and info.first_bad == n and info.n_sites == n and info.bandwidth == K
    ms = ctypes.c_double(-1.0)
    assert sol(ms=ctypes.byref(ms)) == 0 and ms.value > 0
    assert fac(b=None) == ARG and fac(f=None) == ARG and fac(o=None) == ARG, "null pointers"
    assert fac(nn=0) == ARG and fac(ld=K) == ARG and fac(ldf=K) == ARG
    assert fac(bd=2) == ARG and fac(bd=-1) == ARG, "unknown dtypes"
    assert fac(r=float("inf")) == ARG and fac(r=float("nan")) == ARG, "a non-finite ridge"
    both = torch.zeros(n * (K + 1) * 2 + 8, dtype=torch.float64, device="cuda:0")
    assert fac(b=ctypes.c_void_p(both.data_ptr() + 16), f=p(both)) == ARG, "the factor overlaps the band"
    assert fac(b=p(both), f=ctypes.c_void_p(both.data_ptr() + 4 * ((n - 1) * (K + 1) + K))) == ARG, "by one element"
    assert fac(b=p(both), f=ctypes.c_void_p(both.data_ptr() + 8 * ((n * (K + 1) * 4 + 7) // 8))) == 0, "adjacent is fine"
    assert Lb.wld_banded_cholesky_device(None, p(band), 0, K + 1, n, K, ridge, None, p(F), K + 1, ctypes.byref(info)) == ARG
    assert sol(f=None) == ARG and sol(b=None) == ARG, "null pointers"
    assert sol(nn=0) == ARG and sol(nc=0) == ARG and sol(ldf=K) == ARG and sol(ldb=4) == ARG
    assert sol(mode=3) == ARG and sol(mode=-1) == ARG, "unknown modes"
    assert Lb.wld_banded_solve_device(None, p(F), K + 1, n, K, 0, p(rhs_t), 5, 5, None) == ARG

    c = case1()
    busy = W.Context(0)
    busy.load(c.buf, c.w)
    n_rows = busy.run(0.05)
    rows, stats = busy.rows(), busy.stats()
    assert fac(c=busy) == 0 and sol(c=busy) == 0
    after = busy.rows()
    assert len(after) == n_rows and busy.stats() == stats, "wld_last_stats stays"
    for f in ("site_a", "site_b", "d", "d_prime", "r2"):
        assert np.array_equal(getattr(after, f), getattr(rows, f)), f
    busy.run_chunks_async(0.05)
    assert fac(c=busy) == STATE and sol(c=busy) == STATE, "during a run"
    busy.run_wait()
    assert fac(c=busy) == 0 and sol(c=busy) == 0
    busy.close()
    grp = W.Context(devices=[0, 0])
    assert fac(c=grp) == STATE and sol(c=grp) == STATE, "a device group"
    grp.close()
    # Python: refused before any device call
    for args, kw in (((band.cpu(),), {}), ((band.double(),), {}), ((band[:, ::2],), {}), ((band[0],), {}),
                     ((band,), {"ridge": float("inf")}), ((band,), {"bandwidth": K + 1}),
                     ((band,), {"diag": torch.zeros(n, device="cuda:0")}),
                     ((band,), {"diag": torch.zeros(n - 1, dtype=torch.float64, device="cuda:0")}),
                     ((band,), {"out": torch.zeros((n, K + 1), device="cuda:0")}),
                     ((band,), {"out": torch.zeros((n, K), dtype=torch.float64, device="cuda:0")})):
        with pytest.raises(ValueError):
            ctx.banded_cholesky(*args, **kw)
    for args, kw in (((F, rhs_t), {"mode": "both"}), ((F.float(), rhs_t), {}), ((F, rhs_t[:100]), {}), ((F, rhs_t.cpu()), {}),
                     ((F, rhs_t.half()), {}), ((F[:, ::2], rhs_t), {}),
                     ((F, rhs_t), {"out": torch.zeros((n, 5), device="cuda:0")}),
                     ((F, rhs_t), {"out": torch.zeros((n, 4), dtype=torch.float64, device="cuda:0")})):
        with pytest.raises(ValueError):
            ctx.banded_solve(*args, **kw)
