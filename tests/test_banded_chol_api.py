"""The banded Cholesky factorisation's host side of the Python API:
banded_cholesky_host against numpy.linalg.cholesky of the dense matrix,
banded_solve_host round trips in each mode, banded_logdet against
numpy.linalg.slogdet, first_bad on matrices that are not positive definite, and
the argument checks of Context.banded_cholesky / Context.banded_solve
(banded_chol_args, banded_solve_args: everything refused before a device call).
No GPU.

The case builders are shared with tests/test_gpu_banded_chol.py.  Every matrix
is built in numpy from a seed and rounded to float32 before anything else is
derived from it."""
import numpy as np
import pytest

from test_matrix_banded_api import band_case, x_case
from weightedld_amd import api

SHAPES = [(1, 0), (63, 5), (64, 63), (65, 64), (130, 129), (130, 400), (600, 65), (600, 200)]
BAD = [(600, 200, p) for p in (0, 63, 64, 200)] + [(130, 400, p) for p in (0, 63, 64)]


def shifted_dense(B, ridge=0.0, diag=None):
    """The dense float64 matrix A of the band B with the diagonal
    fl(fl(B[i, 0] + ridge) + diag[i]): the definition the device uses."""
    Bd = np.asarray(B).astype(np.float64)
    Bd[:, 0] = Bd[:, 0] + np.float64(ridge)
    if diag is not None:
        Bd[:, 0] = Bd[:, 0] + np.asarray(diag, dtype=np.float64)
    return api.banded_to_dense(Bd)


def upper_dense(U_band):
    """The dense upper triangular matrix of a factor in band layout (elements
    with i + k >= n not read)."""
    U_band = np.asarray(U_band)
    n = U_band.shape[0]
    U = np.zeros((n, n), dtype=U_band.dtype)
    for k in range(min(U_band.shape[1], n)):
        U[np.arange(n - k), np.arange(n - k) + k] = U_band[:n - k, k]
    return U


def dominant_case(n, K, seed=None):
    """band_case with a ridge that makes the matrix diagonally dominant:
    (band float32 with NaN past the last site, ridge, None)."""
    B = band_case(n, K, 1000 * n + K if seed is None else seed)
    S = api.banded_to_dense(B).astype(np.float64)
    ridge = 1.0 + float(np.abs(S).sum(axis=1).max())
    return B, ridge, None


def gram_case(n, K, seed=None, ridge=1e-3):
    """The upper band of T^T T for a random upper-banded T of bandwidth K with
    entries in [-1, 1] and a diagonal in [0.05, 1], rounded to float32, NaN past
    the last site; ridge 1e-3 and a random diag in [0, 0.1]."""
    rng = np.random.default_rng(7000 * n + K if seed is None else seed)
    T = np.triu(rng.uniform(-1.0, 1.0, size=(n, n)))
    i, j = np.indices((n, n))
    T[j - i > K] = 0.0
    T[np.arange(n), np.arange(n)] = rng.uniform(0.05, 1.0, size=n)
    B = api.banded_from_dense(T.T @ T, K).astype(np.float32)
    r, k = np.arange(n)[:, None], np.arange(K + 1)[None, :]
    B[r + k >= n] = np.nan
    return B, ridge, rng.uniform(0.0, 0.1, size=n)


def bad_case(n, K, p, value=-1.0):
    """The dominant case with the shifted diagonal of row p equal to `value`
    (-1, or NaN): the band holds value - ridge there, which float32 holds
    exactly (the band's values and the ridge are multiples of 2^-10 below
    2^13).  Everything subtracted from pivot p is a square, and the pivots
    before p depend on earlier rows only, so first_bad == p exactly."""
    B, ridge, _ = dominant_case(n, K)
    B = B.copy()
    B[p, 0] = np.float32(value - ridge)
    if not np.isnan(value):
        assert np.float64(B[p, 0]) + ridge == value
    return B, ridge, None


@pytest.mark.parametrize("kind", ["dominant", "gram"])
@pytest.mark.parametrize("n,K", SHAPES)
def test_cholesky_host_against_numpy(n, K, kind):
    # well conditioned for this comparison: the gram case takes a ridge of 0.5
    B, ridge, diag = dominant_case(n, K) if kind == "dominant" else gram_case(n, K, ridge=0.5)
    A = shifted_dense(B, ridge, diag)
    ref = np.linalg.cholesky(A).T
    U, bad = api.banded_cholesky_host(B, ridge, diag)
    assert bad is None and U.shape == (n, K + 1) and U.dtype == np.float64
    r, k = np.arange(n)[:, None], np.arange(K + 1)[None, :]
    assert not U[r + k >= n].any() and not np.signbit(U[r + k >= n]).any(), "tails are +0.0"
    assert np.all(U[:, 0] > 0)
    # (atol: elements that cancel to near zero carry the absolute error of their row, a few ulps of the largest entry)
    atol = 1e-12 * np.abs(ref).max()
    assert np.allclose(upper_dense(U), ref, rtol=1e-10, atol=atol)
    assert np.allclose(api.banded_from_dense(ref, K), U, rtol=1e-10, atol=atol)
    # the log-determinant
    sign, logdet = np.linalg.slogdet(A)
    assert sign == 1.0 and abs(api.banded_logdet(U) - logdet) <= 1e-10 * max(1.0, abs(logdet))


@pytest.mark.parametrize("n,K", [(1, 0), (63, 5), (65, 64), (130, 400), (600, 65)])
def test_solve_host_round_trips(n, K):
    B, ridge, diag = gram_case(n, K, ridge=0.5)
    A = shifted_dense(B, ridge, diag)
    U, bad = api.banded_cholesky_host(B, ridge, diag)
    assert bad is None
    Ud = upper_dense(U)
    b = x_case(n, 3, n + K, np.float64)
    scale = np.abs(b).max() * np.linalg.cond(A)
    y = api.banded_solve_host(U, b, "forward")
    x = api.banded_solve_host(U, y, "backward")
    full = api.banded_solve_host(U, b, "full")
    assert y.shape == b.shape and y.dtype == np.float64
    assert np.abs(Ud.T @ y - b).max() <= 1e-12 * scale
    assert np.abs(Ud @ x - y).max() <= 1e-12 * scale
    assert np.array_equal(full, x), "full is forward, then backward"
    assert np.abs(A @ full - b).max() <= 1e-12 * scale
    assert np.abs(full - np.linalg.solve(A, b)).max() <= 1e-10 * scale
    v = api.banded_solve_host(U, b[:, 1])
    assert v.shape == (n,) and np.abs(v - full[:, 1]).max() <= 1e-12 * scale  # (numpy's dot order depends on the shape)
    # float32 right-hand sides are converted, not modified
    b32 = b.astype(np.float32)
    keep = b32.copy()
    assert np.array_equal(api.banded_solve_host(U, b32), api.banded_solve_host(U, b32.astype(np.float64)))
    assert np.array_equal(b32, keep)
    for bad_call in (lambda: api.banded_solve_host(U, b, "both"), lambda: api.banded_solve_host(U, b[:-1] if n > 1 else b[:0]),
                     lambda: api.banded_solve_host(U[0], b)):
        with pytest.raises(ValueError):
            bad_call()


@pytest.mark.parametrize("n,K,p", BAD)
def test_first_bad_host(n, K, p):
    good, ridge, _ = dominant_case(n, K)
    U_good, none = api.banded_cholesky_host(good, ridge)
    assert none is None
    for value in (-1.0, float("nan")):
        B, ridge, _ = bad_case(n, K, p, value)
        U, bad = api.banded_cholesky_host(B, ridge)
        assert bad == p
        assert np.array_equal(U[:p], U_good[:p]), "the rows before the bad pivot are the good matrix's"


def test_host_argument_checks():
    B, ridge, diag = gram_case(63, 5)
    for call in (lambda: api.banded_cholesky_host(B[0]), lambda: api.banded_cholesky_host(B, float("inf")),
                 lambda: api.banded_cholesky_host(B, float("nan")), lambda: api.banded_cholesky_host(B, 0.0, diag[:-1]),
                 lambda: api.banded_logdet(np.zeros(4))):
        with pytest.raises(ValueError):
            call()
    assert api.banded_logdet(np.array([[2.0, 9.0], [4.0, 0.0]])) == pytest.approx(2.0 * np.log(8.0))


class FakeTensor:
    """A device tensor by duck typing: the checks run without a GPU."""

    def __init__(self, shape, dtype="float32", stride=None, dev="cuda", index=0):
        self.shape, self.dtype = tuple(shape), "torch." + dtype
        self._stride = tuple(stride) if stride is not None else tuple(
            int(np.prod(shape[i + 1:])) for i in range(len(shape)))
        self.device = type("device", (), {"type": dev, "index": index})()

    def stride(self):
        return self._stride

    def data_ptr(self):
        raise AssertionError("no device call")


def test_banded_chol_args():
    T = FakeTensor
    assert api.banded_chol_args(T((600, 66))) == (600, 65, 0, 66, None)
    assert api.banded_chol_args(T((600, 66), "float16", (80, 1)), 0.5, T((600,), "float64"),
                                T((600, 21), "float64", (30, 1)), 20, device=0) == (600, 20, 1, 80, 30)
    assert api.banded_chol_args(T((1, 1)), out=T((1, 1), "float64")) == (1, 0, 0, 1, 1)
    good = dict(band=T((600, 66)), ridge=0.0, diag=None, out=None, bandwidth=None)
    for kw in ({"band": T((600, 66), "float64")}, {"band": T((600, 66), dev="cpu")}, {"band": T((600,))},
               {"band": T((600, 66), stride=(132, 2))}, {"band": T((600, 66), stride=(65, 1))}, {"band": np.zeros((600, 66))},
               {"band": T((0, 66))}, {"bandwidth": 66}, {"bandwidth": -1}, {"bandwidth": "wide"},
               {"ridge": float("inf")}, {"ridge": float("nan")}, {"ridge": "big"},
               {"diag": T((600,), "float32")}, {"diag": T((599,), "float64")}, {"diag": T((600,), "float64", (2,))},
               {"diag": T((600,), "float64", dev="cpu")}, {"diag": np.zeros(600)},
               {"out": T((600, 66), "float32")}, {"out": T((600, 65), "float64")}, {"out": T((600, 66), "float64", (65, 1))},
               {"out": T((600, 66), "float64", (132, 2))}, {"out": T((600, 66), "float64", dev="cpu")}):
        with pytest.raises(ValueError):
            api.banded_chol_args(**dict(good, **kw))
    with pytest.raises(ValueError):
        api.banded_chol_args(T((600, 66), index=1), device=0)


def test_banded_solve_args():
    T = FakeTensor
    F = T((600, 66), "float64", (70, 1))
    assert api.banded_solve_args(F, T((600,), "float32")) == (600, 65, 70, 0, 1)
    assert api.banded_solve_args(F, T((600, 17), "float64", (20, 1)), "forward", T((600, 17), "float64")) == (600, 65, 70, 1, 17)
    assert api.banded_solve_args(F, T((600, 1), "float64"), "backward")[3:] == (2, 1)
    good = dict(factor=F, b=T((600, 5), "float64"), mode="full", out=None)
    for kw in ({"mode": "both"}, {"mode": 0}, {"factor": T((600, 66), "float32")}, {"factor": T((600, 66), "float64", (65, 1))},
               {"factor": T((600, 66), "float64", (132, 2))}, {"factor": T((600,), "float64")},
               {"factor": T((600, 66), "float64", dev="cpu")}, {"b": T((599, 5), "float64")}, {"b": T((600, 5), "float16")},
               {"b": T((600, 5, 1), "float64")}, {"b": T((600, 5), "float64", dev="cpu")},
               {"b": np.zeros((600, 5))}, {"out": T((600, 5), "float32")}, {"out": T((600, 4), "float64")},
               {"out": T((600, 5), "float64", (4, 1))}, {"out": T((600, 5), "float64", (10, 2))}):
        with pytest.raises(ValueError):
            api.banded_solve_args(**dict(good, **kw))
