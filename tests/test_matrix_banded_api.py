"""The banded LD matrix's host side of the Python API: banded_from_dense /
banded_to_dense, banded_matmul_host (the f64 reference of the device product)
against math.fsum of the dense form's terms, the argument checks of
Context.run_matrix_banded (banded_args: everything refused before a device
call) and banded_cg_solve with the host product.  No GPU.

band_case() and cg_case() are shared with tests/test_gpu_banded_apply.py."""
import math

import numpy as np
import pytest

from weightedld_amd import api


def band_case(L, K, seed, dtype=np.float32):
    """A random band [L, K + 1] (values exactly representable in float16, mixed
    sign) with NaN planted at every position past the last site (i + k >= L)."""
    rng = np.random.default_rng(seed)
    B = (rng.integers(-2048, 2049, size=(L, K + 1)) / 1024.0).astype(dtype)
    i, k = np.arange(L)[:, None], np.arange(K + 1)[None, :]
    B[i + k >= L] = np.nan
    return B


def x_case(L, C, seed, dtype=np.float32):
    """X mixed-sign and asymmetric in both indices."""
    rng = np.random.default_rng(seed + 77)
    i, c = np.arange(L)[:, None], np.arange(C)[None, :]
    return ((rng.random((L, C)) - 0.4) * (1.0 + 0.37 * c) + 0.013 * i - 0.05 * c * (i % 3)).astype(dtype)


def terms(B, X, i, c):
    """The products of element (i, c) of S X, rounded to f64 once each (exact
    for float32 X), in the formula's order."""
    L, W = B.shape
    t = [float(B[i, k]) * float(X[i + k, c]) for k in range(min(W, L - i))]
    t += [float(B[i - k, k]) * float(X[i - k, c]) for k in range(1, min(W - 1, i) + 1)]
    return t


def cg_case(L=300, K=20, seed=5):
    """A diagonally dominant random band, its right-hand side and the dense solution."""
    rng = np.random.default_rng(seed)
    B = (rng.random((L, K + 1)) - 0.5).astype(np.float32)
    B[:, 0] = 2.0 * K + 1.0
    i, k = np.arange(L)[:, None], np.arange(K + 1)[None, :]
    B[i + k >= L] = np.nan
    b = rng.standard_normal(L)
    x = np.linalg.solve(api.banded_to_dense(B).astype(np.float64), b)
    return B, b, x


@pytest.mark.parametrize("n,K", [(1, 0), (5, 0), (5, 2), (5, 4), (5, 9), (64, 63), (130, 17)])
def test_from_dense_to_dense_round_trip(n, K):
    rng = np.random.default_rng(n * 100 + K)
    M = rng.standard_normal((n, n)).astype(np.float32)
    M = M + M.T
    B = api.banded_from_dense(M, K)
    assert B.shape == (n, K + 1) and B.dtype == np.float32
    for i in range(n):
        for k in range(K + 1):
            assert B[i, k] == (M[i, i + k] if i + k < n else 0.0), (i, k)
    D = api.banded_to_dense(B)
    i, j = np.indices((n, n))
    inside = np.abs(i - j) <= K
    assert np.array_equal(D[inside], M[inside]) and not D[~inside].any()
    assert np.array_equal(api.banded_from_dense(D, K), B)
    # elements past the last site are not read
    Bn = B.copy()
    Bn[(np.arange(n)[:, None] + np.arange(K + 1)[None, :]) >= n] = np.nan
    assert np.array_equal(api.banded_to_dense(Bn, n), D)
    for bad in (lambda: api.banded_from_dense(M[:, :-1] if n > 1 else M[0], K), lambda: api.banded_from_dense(M, -1),
                lambda: api.banded_to_dense(B, n + 1), lambda: api.banded_to_dense(B[0])):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("L,K", [(1, 0), (63, 5), (65, 63), (130, 129), (130, 200)])
@pytest.mark.parametrize("xdt", [np.float32, np.float64])
def test_matmul_host_against_fsum(L, K, xdt):
    B, X = band_case(L, K, L + K), x_case(L, 3, L, xdt)
    Y = api.banded_matmul_host(B, X)
    assert Y.shape == X.shape and Y.dtype == np.float64 and np.isfinite(Y).all()
    D = api.banded_to_dense(B).astype(np.float64)
    for i in range(L):
        for c in range(3):
            t = terms(B, X, i, c)
            exact = math.fsum(t)
            assert exact == math.fsum(D[i, j] * float(X[j, c]) for j in range(L))  # the dense form's terms
            bound = (len(t) + 2) * 2.0 ** -52 * math.fsum(abs(v) for v in t)
            assert abs(Y[i, c] - exact) <= bound, (i, c, Y[i, c], exact, bound)
    y1 = api.banded_matmul_host(B, X[:, 1])
    assert y1.shape == (L,) and np.array_equal(y1, Y[:, 1])
    with pytest.raises(ValueError):
        api.banded_matmul_host(B, np.zeros(L + 1))
    with pytest.raises(ValueError):
        api.banded_matmul_host(B[0], X)


def test_banded_args():
    assert api.banded_args(130, 129) == ((0, 130), 129, 1, 0, None, 130)
    assert api.banded_args(600, 65, (37, 201), 72, "dprime", "float16") == ((37, 201), 72, 3, 1, None, 73)
    assert api.banded_args(600, 65, bandwidth=np.int64(65))[1] == 65
    out = np.zeros((164, 100), dtype=np.float32)
    assert api.banded_args(600, 65, (37, 201), out=out[:, :66])[4:] == ("numpy", 100)
    assert api.banded_args(600, 0, (599, 600), out=np.zeros((1, 1), np.float32))[4:] == ("numpy", 1)
    with pytest.raises(ValueError, match="needs bandwidth 65"):
        api.banded_args(600, 65, bandwidth=64)
    for kw in ({"rows": (5, 5)}, {"rows": (9, 3)}, {"rows": (0, 601)}, {"rows": (-1, 4)}, {"rows": 7}, {"bandwidth": -1},
               {"bandwidth": 65.5}, {"bandwidth": "wide"}, {"bandwidth": 2 ** 32}, {"stat": "rho"}, {"dtype": "float64"},
               {"out": np.zeros((600, 65), np.float32)}, {"out": np.zeros((600, 66), np.float64)},
               {"out": np.zeros((600, 132), np.float32)[:, ::2]}, {"out": np.zeros((66, 600), np.float32).T},
               {"out": [[0.0] * 66] * 600}, {"out": np.zeros((600, 66), np.float32), "dtype": "float16"}):
        with pytest.raises(ValueError):
            api.banded_args(600, 65, **kw)
    ro = np.zeros((600, 66), np.float32)
    ro.setflags(write=False)
    with pytest.raises(ValueError):
        api.banded_args(600, 65, out=ro)

    class FakeTensor:  # a tensor on the wrong kind of device: refused without importing torch
        shape, dtype = (600, 66), "torch.float32"

        class device:
            type, index = "cpu", None

        def data_ptr(self):
            raise AssertionError("no device call")

        def stride(self):
            return (80, 1)

    with pytest.raises(ValueError):
        api.banded_args(600, 65, out=FakeTensor())
    FakeTensor.device.type = "cuda"
    assert api.banded_args(600, 65, out=FakeTensor())[4:] == ("device", 80)


def test_cg_solve_host():
    B, b, x_ref = cg_case()
    x, it, res, ok = api.banded_cg_solve(api.banded_matmul_host, B, b, tol=1e-10)
    assert ok and 0 < it < 300 and res <= 1e-10
    A = api.banded_to_dense(B).astype(np.float64)
    assert np.linalg.norm(b - A @ x) <= 1e-10 * np.linalg.norm(b) * (1 + 1e-6)
    assert np.abs(x - x_ref).max() <= 1e-9 * np.abs(x_ref).max()
    # a ridge: (S + ridge I) x = b
    xr, _, res_r, ok_r = api.banded_cg_solve(api.banded_matmul_host, B, b.reshape(-1, 1), ridge=3.5)
    assert ok_r and res_r <= 1e-8 and xr.shape == (300, 1)
    assert np.abs(xr[:, 0] - np.linalg.solve(A + 3.5 * np.eye(300), b)).max() <= 1e-7 * np.abs(x_ref).max()
    # too few iterations: not converged, the residual reported
    _, it2, res2, ok2 = api.banded_cg_solve(api.banded_matmul_host, B, b, tol=1e-14, max_iter=2)
    assert not ok2 and it2 == 2 and res2 > 1e-14
    # b = 0
    x0, it0, res0, ok0 = api.banded_cg_solve(api.banded_matmul_host, B, np.zeros(300))
    assert ok0 and it0 == 0 and res0 == 0.0 and not x0.any()
    with pytest.raises(ValueError):
        api.banded_cg_solve(api.banded_matmul_host, B, np.zeros((300, 2)))
    with pytest.raises(ValueError):
        api.banded_cg_solve(api.banded_matmul_host, B, b, tol=0.0)


def test_cg_solve_flags_an_indefinite_band():
    L, K = 300, 20
    B = np.zeros((L, K + 1), dtype=np.float32)
    B[:, 0] = np.where(np.arange(L) % 2 == 0, 1.0, -1.0)  # diag(+1, -1, ...): indefinite
    b = np.ones(L)
    x, it, res, ok = api.banded_cg_solve(api.banded_matmul_host, B, b)
    assert not ok and it == 0 and res == 1.0 and not x.any()  # b.A b = 0: no positive curvature
    # definite again under a ridge
    x, it, res, ok = api.banded_cg_solve(api.banded_matmul_host, B, b, ridge=2.0)
    assert ok and res <= 1e-8 and np.allclose(x, 1.0 / (B[:, 0] + 2.0))
