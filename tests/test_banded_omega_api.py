"""The sweep scan's host side of the Python API: the numpy twins
banded_pairsum_host and banded_omega_host (the definition of what the device
computes) against brute force, omega_splits (wld_omega_splits, host only)
against a brute-force search, every argument refusal that needs no device, a
planted sweep and an exact tie.  No GPU.

The pair-sum reference is math.fsum over the dense matrix, the exactly rounded
sum.  M[j, k] adds m = w (w - 1) / 2 non-negative terms (w = k + 1 sites), each
through at most m - 1 additions, so in ANY summation order
    |M - exact| <= gamma_{m-1} exact,   gamma_q = q u / (1 - q u),  u = 2^-53
(Higham, Accuracy and Stability, section 4.2): derived, not measured.  omega is
compared bit for bit with a plain double loop over the same formula in Python
floats.

The case builders are shared with tests/test_gpu_banded_omega.py."""
import functools
import math

import numpy as np
import pytest

from test_banded_chol_api import FakeTensor
from test_gpu_heatmap import case1_map
from weightedld_amd import api

U = 2.0 ** -53
PAIRSUM_SHAPES = [(1, 0), (2, 1), (5, 4), (63, 10), (64, 63), (65, 64), (130, 129), (130, 400), (600, 65), (600, 200)]


def gamma(q):
    return q * U / (1.0 - q * U)


@functools.lru_cache(maxsize=None)
def r2_band_case(n, K, dtype="float32", seed=None):
    """(band [n, K + 1] of `dtype` with values in [0, 1), planted): a few NaN,
    +inf and -inf inside the band (k >= 1, j + k < n; `planted` of them), NaN in
    column 0 and where j + k >= n."""
    rng = np.random.default_rng(31 * n + K if seed is None else seed)
    B = rng.random((n, K + 1)).astype(np.float32).astype(dtype)
    j, k = np.arange(n)[:, None], np.arange(K + 1)[None, :]
    inside = np.argwhere((k >= 1) & (j + k < n))
    pick = inside[rng.choice(len(inside), size=min(7, len(inside)), replace=False)] if len(inside) else inside
    for t, (r, c) in enumerate(pick):
        B[r, c] = (np.nan, np.inf, -np.inf)[t % 3]
    B[:, 0] = np.nan
    B[j + k >= n] = np.nan
    B.setflags(write=False)
    return B, len(pick)


def dense_r2(B):
    """The dense symmetric float64 matrix the table sums: finite in-band values,
    0 elsewhere and on the diagonal."""
    B = np.asarray(B)
    n = B.shape[0]
    D = np.zeros((n, n))
    for k in range(1, min(B.shape[1], n)):
        v = B[:n - k, k].astype(np.float64)
        v[~np.isfinite(v)] = 0.0
        D[np.arange(n - k), np.arange(n - k) + k] = v
    return D + D.T


def exact_pairsum(D, j, i):
    """fsum of D[u, v] over j <= u < v <= i."""
    return math.fsum(np.triu(D[j:i + 1, j:i + 1], 1).ravel().tolist())


def omega_brute(M, split, lo, hi, min_side, eps):
    """The scan by a plain double loop in Python floats: (omega, left, right,
    zns, evaluated, skipped)."""
    om, left, right, zns, ev, sk = [], [], [], [], 0, 0
    for c, l0, h0 in zip(split, lo, hi):
        c, l0, h0 = int(c), int(l0), int(h0)
        w = h0 - l0 + 1
        zns.append(float(M[l0, h0 - l0]) / float(w * (w - 1) // 2))
        best = None
        for a in range(l0, c - min_side + 2):
            for b in range(c + min_side, h0 + 1):
                l, r = c - a + 1, b - c
                SL, SR, ST = float(M[a, c - a]), float(M[c + 1, b - c - 1]), float(M[a, b - a])
                X = (ST - SL) - SR
                t1 = (SL + SR) / float(l * (l - 1) // 2 + r * (r - 1) // 2)
                t2 = X / float(l * r) + eps
                if not t2 > 0:
                    sk += 1
                    continue
                ev += 1
                wv = t1 / t2
                if best is None or wv > best[0]:  # (a, b ascending: the first of equal ones stays)
                    best = (wv, a, b)
        om.append(float("nan") if best is None else best[0])
        left.append(api.OMEGA_NONE if best is None else best[1])
        right.append(api.OMEGA_NONE if best is None else best[2])
    return np.array(om), np.array(left, dtype=np.uint32), np.array(right, dtype=np.uint32), np.array(zns), ev, sk


def every_split(n, K, max_side):
    """Every split c = 0 .. n - 2 with flanks of up to max_side sites, max_side
    clipped so that hi - lo <= K."""
    ms = max(1, min(max_side, (K + 1) // 2))
    _, split, lo, hi = api.omega_splits(None, n, 0, ms)
    assert np.all(hi - lo <= K)
    return split, lo, hi


@functools.lru_cache(maxsize=None)
def tie_case():
    """A 20 x 11 band of 0.5: at split 9 with lo 5 and hi 14 all 16 candidates
    give the same omega, 0.5 / (0.5 + 1e-5)."""
    B = np.full((20, 11), 0.5, dtype=np.float32)
    B.setflags(write=False)
    return B


@functools.lru_cache(maxsize=None)
def sweep_case():
    """n = 120, K = 79: background r2 uniform in [0, 0.05), the blocks [30, 60)
    and [60, 85) uniform in [0.7, 0.95): a sweep between the sites 59 and 60."""
    rng = np.random.default_rng(0x5EE9)
    n, K = 120, 79
    R = rng.uniform(0.0, 0.05, size=(n, n))
    for b0, b1 in ((30, 60), (60, 85)):
        R[b0:b1, b0:b1] = rng.uniform(0.7, 0.95, size=(b1 - b0, b1 - b0))
    R = np.triu(R, 1)
    B = api.banded_from_dense(R + R.T, K).astype(np.float32)
    B.setflags(write=False)
    return B


@functools.lru_cache(maxsize=None)
def zero_cross_case():
    """n = 40, K = 39: r2 a random multiple of 2^-10 inside the groups [0, 20)
    and [20, 40) and exactly 0 between them.  Every sum is exact, so X is exactly
    0 for a candidate whose cross block lies between the groups."""
    rng = np.random.default_rng(0xC405)
    n = 40
    R = rng.integers(1, 1024, size=(n, n)) / 1024.0
    R[:20, 20:] = 0.0
    R = np.triu(R, 1)
    B = api.banded_from_dense(R + R.T, n - 1).astype(np.float32)
    B.setflags(write=False)
    return B


@pytest.mark.parametrize("n,K", [(1, 0), (2, 1), (5, 4), (40, 39), (63, 10), (30, 50)])
def test_pairsum_host_against_fsum(n, K):
    B, planted = r2_band_case(n, K)
    assert api.banded_nonfinite_host(B) == planted
    M = api.banded_pairsum_host(B)
    assert M.shape == (n, K + 1) and M.dtype == np.float64
    r, k = np.arange(n)[:, None], np.arange(K + 1)[None, :]
    tails = M[(r + k >= n) | (k == 0)]
    assert not tails.any() and not np.signbit(tails).any(), "column 0 and the tails are +0.0"
    D = dense_r2(B)
    worst = 0.0
    for j in range(n):
        for kk in range(1, min(K, n - 1 - j) + 1):
            exact = exact_pairsum(D, j, j + kk)
            m = (kk + 1) * kk // 2
            bound = gamma(m - 1) * exact
            assert abs(M[j, kk] - exact) <= bound, (j, kk, M[j, kk], exact)
            worst = max(worst, abs(M[j, kk] - exact) / bound if bound else 0.0)
    print("n %d K %d: worst |M - exact| / bound = %.4f" % (n, K, worst))
    # float16 storage of the same values: the table of the rounded band
    B16 = B.astype(np.float16)
    assert np.array_equal(api.banded_pairsum_host(B16), api.banded_pairsum_host(B16.astype(np.float64)))
    with pytest.raises(ValueError):
        api.banded_pairsum_host(B[0])


@pytest.mark.parametrize("n,K", [(5, 4), (40, 39), (63, 10), (30, 50)])
@pytest.mark.parametrize("min_side", [2, 5])
def test_omega_host_against_double_loop(n, K, min_side):
    M = api.banded_pairsum_host(r2_band_case(n, K)[0])
    for max_side in (2, 3, 33):
        split, lo, hi = every_split(n, K, max_side)
        for eps in (1e-5, 0.0):
            got = api.banded_omega_host(M, split, lo, hi, min_side, eps)
            om, left, right, zns, ev, sk = omega_brute(M, split, lo, hi, min_side, eps)
            assert got.omega.tobytes() == om.tobytes() and got.zns.tobytes() == zns.tobytes()
            assert np.array_equal(got.left, left) and np.array_equal(got.right, right)
            assert (got.evaluated, got.skipped) == (ev, sk)
            assert got.n_splits == n - 1 and got.kernel_ms is None
            assert np.array_equal(np.isnan(got.omega), got.left == api.OMEGA_NONE)


def test_zero_cross_block_skips():
    B = zero_cross_case()
    M = api.banded_pairsum_host(B)
    split, lo, hi = every_split(40, 39, 20)
    with_eps = api.banded_omega_host(M, split, lo, hi, 2, 1e-5)
    assert with_eps.skipped == 0 and not np.isnan(with_eps.omega[19])
    none = api.banded_omega_host(M, split, lo, hi, 2, 0.0)
    om, left, right, zns, ev, sk = omega_brute(M, split, lo, hi, 2, 0.0)
    assert none.omega.tobytes() == om.tobytes() and (none.evaluated, none.skipped) == (ev, sk)
    assert none.skipped > 0 and none.evaluated > 0
    assert np.isnan(none.omega[19]) and none.left[19] == api.OMEGA_NONE and none.right[19] == api.OMEGA_NONE
    assert none.evaluated + none.skipped == with_eps.evaluated


def brute_splits(pos, n_grid, max_side, D):
    p = [int(x) for x in pos]
    n = len(p)
    if n_grid == 0:
        cs, xs = list(range(n - 1)), p[:-1]
    else:
        span = p[-1] - p[0]
        xs = [p[0] + span // 2] if n_grid == 1 else [p[0] + span * g // (n_grid - 1) for g in range(n_grid)]
        cs = [min(max(i for i in range(n) if p[i] <= x), n - 2) for x in xs]
    lo, hi = [], []
    for c, x in zip(cs, xs):
        l, h = max(c - max_side + 1, 0), min(c + max_side, n - 1)
        if D:
            l = max(l, min([i for i in range(n) if p[i] >= x - D], default=n))
            h = min(h, max(i for i in range(n) if p[i] <= x + D))
        lo.append(min(l, c))
        hi.append(max(h, c + 1))
    return np.array(xs, dtype=np.uint64), np.array(cs), np.array(lo), np.array(hi)


@pytest.mark.parametrize("which", ["case1_map", "increasing", "indices"])
@pytest.mark.parametrize("n_grid", [0, 1, 2, 7, 700])
def test_omega_splits_against_brute_force(which, n_grid):
    if which == "case1_map":
        pos = case1_map()
        assert np.any(np.diff(pos.astype(np.int64)) == 0), "repeated coordinates"
    elif which == "increasing":
        pos = np.cumsum(np.random.default_rng(9).integers(1, 50, size=130)).astype(np.uint64) + np.uint64(10 ** 12)
    else:
        pos = None
    n = 90 if pos is None else len(pos)
    ref_pos = np.arange(n) if pos is None else pos
    for max_side in (1, 2, 33, 1000):
        for D in (0, 5, 60):
            position, split, lo, hi = api.omega_splits(pos, None if pos is not None else n, n_grid, max_side, D or None)
            want = brute_splits(ref_pos, n_grid, max_side, D)
            assert position.dtype == np.uint64 and split.dtype == lo.dtype == hi.dtype == np.uint32
            for got, ref, what in zip((position, split, lo, hi), want, ("position", "split", "lo", "hi")):
                assert np.array_equal(got.astype(np.int64), ref.astype(np.int64)), (what, max_side, D)
            assert np.all(lo <= split) and np.all(split < hi) and np.all(hi < n)
            assert np.all(hi.astype(np.int64) - lo <= 2 * max_side - 1)
            assert len(split) == (n_grid or n - 1)


def test_refusals():
    M = api.banded_pairsum_host(tie_case())
    good = dict(M=M, split=[9], lo=[5], hi=[14], min_side=2, eps=1e-5)
    for kw in ({"M": M[0]}, {"split": [9, 9]}, {"split": []}, {"lo": [10]}, {"hi": [9]}, {"hi": [20]}, {"lo": [3]},
               {"lo": [-1]}, {"split": [9.5]}, {"min_side": 1}, {"min_side": 0}, {"min_side": "two"}, {"eps": -1e-9},
               {"eps": float("nan")}, {"eps": float("inf")}, {"eps": "small"}):
        with pytest.raises(ValueError):
            api.banded_omega_host(**dict(good, **kw))
    assert api.omega_args(20, 10, [9], [5], [14])[3:] == (2, 1e-5)
    sm = np.arange(10, dtype=np.uint64)
    for args, kw in (((None,), {"max_side": 3}), ((sm,), {}), ((sm,), {"max_side": 0}), ((sm[:1],), {"max_side": 3}),
                     ((sm[::-1],), {"max_side": 3}), ((sm, 9), {"max_side": 3}), ((sm,), {"max_side": 3, "n_grid": -1}),
                     ((sm,), {"max_side": 3, "max_distance": -1}), ((None, 1), {"max_side": 3})):
        with pytest.raises(ValueError):
            api.omega_splits(*args, **kw)
    T = FakeTensor
    assert api.banded_pairsum_args(T((600, 66))) == (600, 65, 0, 66, None)
    assert api.banded_pairsum_args(T((600, 66), "float16", (80, 1)), T((600, 21), "float64", (30, 1)), 20, device=0) == \
        (600, 20, 1, 80, 30)
    for kw in ({"band": T((600, 66), "float64")}, {"band": T((600, 66), dev="cpu")}, {"band": T((600,))},
               {"band": T((600, 66), stride=(65, 1))}, {"band": np.zeros((600, 66))}, {"bandwidth": 66}, {"bandwidth": -1},
               {"out": T((600, 66), "float32")}, {"out": T((600, 65), "float64")},
               {"out": T((600, 66), "float64", (65, 1))}, {"out": T((600, 66), "float64", dev="cpu")}):
        with pytest.raises(ValueError):
            api.banded_pairsum_args(**dict(dict(band=T((600, 66)), out=None, bandwidth=None), **kw))


def test_planted_sweep():
    B = sweep_case()
    M = api.banded_pairsum_host(B)
    position, split, lo, hi = api.omega_splits(None, 120, 0, 40)
    assert np.all(hi - lo <= 79)
    res = api.banded_omega_host(M, split, lo, hi, 2, 1e-5)
    g = int(np.nanargmax(res.omega))
    print("planted sweep: argmax split %d, omega %.4f, borders (%d, %d), zns %.4f" %
          (split[g], res.omega[g], res.left[g], res.right[g], res.zns[g]))
    assert split[g] == 59  # (the borders are not asserted: omega favours a short flank there)
    rows = res.rows(np.arange(1000, 1120))
    assert rows[g][0] == 1059 and rows[g][1] == 1000 + res.left[g] and rows[g][2] == 1000 + res.right[g]
    assert rows[g][3] == res.omega[g] and rows[g][4] == res.zns[g]


def test_exact_tie():
    M = api.banded_pairsum_host(tie_case())
    res = api.banded_omega_host(M, [9], [5], [14], 2, 1e-5)
    assert res.evaluated == 16 and res.skipped == 0
    assert res.omega[0] == 0.5 / (0.5 + 1e-5) and abs(res.omega[0] - 0.9999800004) < 1e-10
    assert (res.left[0], res.right[0]) == (5, 11)
    assert res.zns[0] == 0.5
    om = omega_brute(M, [9], [5], [14], 2, 1e-5)
    assert om[0][0] == res.omega[0] and (om[1][0], om[2][0]) == (5, 11)
    # a split without a left flank: NaN and no borders
    none = api.banded_omega_host(M, [0], [0], [9], 2, 1e-5)
    assert np.isnan(none.omega[0]) and none.left[0] == api.OMEGA_NONE and none.evaluated == none.skipped == 0
    pa, pb = none.parents()
    assert pa[0] == pb[0] == np.uint64(2 ** 64 - 1)
