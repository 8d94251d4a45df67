"""The LD matrix's Python-side argument checks (weightedld_amd.api.matrix_args,
matrix_region: everything refused before a device call) and the tests' own
expected-matrix helpers (matrix_expected.py) against the oracle's
single_weighted_ld_pair on a handful of pairs — one of them a pair whose
(a, b) and (b, a) bits differ, which is why the matrix mirrors pair (min, max)
instead of evaluating both.  No GPU."""
import numpy as np
import pytest

import _oracle as O
from matrix_expected import Dense, expected_counts, expected_matrix, signed_r
from test_gpu_summary import case1
from weightedld_amd import api


@pytest.fixture(scope="module")
def dn():
    c = case1()
    return Dense(c.buf, c.w)


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def test_expected_matrix_against_single_pair(dn):
    m = {s: expected_matrix(dn, s) for s in ("r2", "r", "d", "dprime")}
    asym = None
    rng = np.random.default_rng(0x3A7)
    pairs = [(0, 1), (63, 64), (128, 599), (5, 17), (17, 300), (64, 470)] + \
        [tuple(sorted(rng.choice(600, 2, replace=False).tolist())) for _ in range(60)]
    for a, b in pairs:
        fwd, rev = O.single_pair(dn.buf[a], dn.buf[b], dn.w), O.single_pair(dn.buf[b], dn.buf[a], dn.w)
        if fwd is None:  # a site without a major or minor symbol
            assert not (dn.ok[a] and dn.ok[b])
            for s in m:
                assert np.isnan(m[s][a, b]) and np.isnan(m[s][b, a]), (a, b, s)
            continue
        d, dp, r2 = (np.float32(x) for x in fwd)
        r = signed_r(np.array([d]), np.array([r2]))[0]
        for s, x in (("d", d), ("dprime", dp), ("r2", r2), ("r", r)):
            for u, v in ((a, b), (b, a)):
                got = m[s][u, v]
                assert (np.isnan(got) and np.isnan(x)) or _bits(got) == _bits(x), (a, b, s, got, x)
        if np.isfinite(r2) and r2 > 0 and d != 0:
            assert np.sign(r) == -np.sign(d)
        if rev is not None and any(_bits(p) != _bits(q) and not (np.isnan(p) and np.isnan(q)) for p, q in zip(fwd, rev)):
            asym = (a, b)
    assert asym is not None, "no pair whose (a, b) and (b, a) differ among the sampled ones"
    for s in m:
        assert m[s].tobytes() == np.ascontiguousarray(m[s].T).tobytes()


def test_expected_diagonal_window_and_flags(dn):
    r = expected_matrix(dn, "r")
    assert np.isnan(r[5, 5]) and np.isnan(r[300, 300]) and r[0, 0] == 1.0  # sites 5 and 300 have no two symbols
    assert np.isnan(expected_matrix(dn, "d")[0, 0])
    z = expected_matrix(dn, "r2", zero_missing=True)
    assert not np.isnan(z).any() and np.isfinite(z).all() and z[5, 5] == 1.0 and z[5, 6] == 0.0
    assert expected_matrix(dn, "dprime", zero_missing=True)[0, 0] == 0.0
    k = expected_matrix(dn, "r2", K=3)
    assert k[10, 13] == dn.r2[10, 13] and k[10, 14] == 0.0 and not np.signbit(k[10, 14]) and k[14, 10] == 0.0
    assert expected_matrix(dn, "r", dtype=np.float16).dtype == np.float16
    e = expected_counts(dn, (0, 600), (0, 600))
    assert e == {"pairs": 179700, "none_pairs": 1197, "nonfinite_pairs": 275, "counted_pairs": 178228}
    assert expected_counts(dn, (50, 100), (60, 130))["pairs"] == 50 * 70 - 40 - 40 * 39 // 2
    assert expected_counts(dn, (0, 600), (0, 600), K=1)["pairs"] == 599


def test_matrix_args():
    assert api.matrix_args(130) == ((0, 130), (0, 130), 1, 0, None, 130)
    assert api.matrix_args(130, (3, 129), (61, 70), "dprime", "float16") == ((3, 129), (61, 70), 3, 1, None, 9)
    assert api.matrix_args(130, stat="r2", dtype=np.float32)[2:4] == (0, 0)
    out = np.zeros((126, 20), dtype=np.float32)
    assert api.matrix_args(130, (3, 129), (61, 70), out=out[:, :9])[4:] == ("numpy", 20)
    assert api.matrix_args(130, (3, 4), (61, 62), out=np.zeros((1, 1), np.float32))[4:] == ("numpy", 1)
    for kw in ({"rows": (5, 5)}, {"rows": (9, 3)}, {"cols": (0, 131)}, {"rows": (-1, 4)}, {"rows": 7}, {"rows": (1, 2, 3)},
               {"stat": "rho"}, {"dtype": "float64"}, {"dtype": "bfloat16"},
               {"out": np.zeros((130, 129), np.float32)}, {"out": np.zeros((130, 130), np.float64)},
               {"out": np.zeros((130, 130), np.float16)}, {"out": np.zeros((130, 260), np.float32)[:, ::2]},
               {"out": np.zeros((130, 130), np.float32).T}, {"out": [[0.0] * 130] * 130},
               {"out": np.zeros((130, 130), np.float32), "dtype": "float16"}):
        with pytest.raises(ValueError):
            api.matrix_args(130, **kw)
    ro = np.zeros((130, 130), np.float32)
    ro.setflags(write=False)
    with pytest.raises(ValueError):
        api.matrix_args(130, out=ro)

    class FakeTensor:  # a tensor on the wrong kind of device: refused without importing torch
        shape, dtype = (130, 130), "torch.float32"

        class device:
            type, index = "cpu", None

        def data_ptr(self):
            raise AssertionError("no device call")

        def stride(self):
            return (130, 1)

    with pytest.raises(ValueError):
        api.matrix_args(130, out=FakeTensor())
    FakeTensor.device.type = "cuda"
    assert api.matrix_args(130, out=FakeTensor())[4:] == ("device", 130)


def test_matrix_region():
    pos = np.array([3, 3, 7, 10, 10, 10, 15, 40], dtype=np.uint64)
    assert api.matrix_region(pos, 8, (0, 100)) == (0, 8)
    assert api.matrix_region(pos, 8, (3, 10)) == (0, 3)
    assert api.matrix_region(pos, 8, (4, 11)) == (2, 6)
    assert api.matrix_region(None, 8, (2, 5)) == (2, 5)
    for bad in ((11, 15), (5, 3), (41, 50), (1,), "ab"):
        with pytest.raises(ValueError):
            api.matrix_region(pos, 8, bad)
    with pytest.raises(ValueError):
        api.matrix_region(np.array([1, 5, 4]), 3, (0, 9))
    with pytest.raises(ValueError):
        api.matrix_region(pos, 7, (0, 9))
