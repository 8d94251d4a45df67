"""The expected LD matrix of the tests (test_gpu_matrix.py, test_matrix_api.py),
assembled in numpy from the CPU oracle's dense d, d', r2 and `valid`
(O.all_pairs_dense, meaningful on the upper triangle) by the contract of
include/weightedld.h: the value of pair (min, max) mirrored, the diagonal rule,
the window mask, the stat, zero_missing, the dtype."""
import numpy as np

import _oracle as O

STATS = ("r2", "r", "d", "dprime")


def site_ok(buf):
    """True where the site has a major and a minor symbol."""
    ok = np.zeros(buf.shape[0], dtype=bool)
    for s in range(buf.shape[0]):
        a, b = O.major_minor(O.histogram(buf[s]))
        ok[s] = a is not None and b is not None
    return ok


class Dense:
    """The oracle's dense statistics of a data set (computed once, read-only)."""

    def __init__(self, buf, w):
        self.buf, self.w, self.L = buf, w, buf.shape[0]
        self.d, self.dp, self.r2, valid = O.all_pairs_dense(buf, w)
        self.valid = valid != 0
        self.ok = site_ok(buf)
        for a in (self.d, self.dp, self.r2, self.valid, self.ok):
            a.setflags(write=False)


def in_window(L, pos=None, D=0, K=0):
    """[L, L] bool, symmetric: the pair {u, v}, u != v, is in the window."""
    i = np.arange(L, dtype=np.int64)
    p = i if pos is None else np.asarray(pos, dtype=np.int64)
    keep = np.ones((L, L), dtype=bool)
    if D:
        keep &= np.abs(p[:, None] - p[None, :]) <= D
    if K:
        keep &= np.abs(i[:, None] - i[None, :]) <= K
    return keep


def signed_r(d, r2):
    """r = (d > 0) ? -sqrtf(r2) : sqrtf(r2) on float32 (numpy's sqrt is correctly rounded)."""
    with np.errstate(invalid="ignore"):
        s = np.sqrt(r2.astype(np.float32))
    return np.where(d > 0, -s, s).astype(np.float32)


def expected_matrix(dn, stat, pos=None, D=0, K=0, zero_missing=False, dtype=np.float32):
    """The full L x L matrix of the contract."""
    L = dn.L
    up = {"r2": dn.r2, "d": dn.d, "dprime": dn.dp}[stat] if stat != "r" else signed_r(dn.d, dn.r2)
    iu = np.triu_indices(L, 1)
    v = up[iu].astype(np.float32)
    v[~dn.valid[iu]] = np.nan  # none pairs
    if zero_missing:
        v[~np.isfinite(v)] = 0.0
    v[~in_window(L, pos, D, K)[iu]] = 0.0
    m = np.zeros((L, L), dtype=np.float32)
    m[iu] = v
    m[(iu[1], iu[0])] = v
    if stat in ("r", "r2"):
        diag = np.where(dn.ok | zero_missing, np.float32(1.0), np.float32(np.nan))
    else:
        diag = np.full(L, 0.0 if zero_missing else np.nan, dtype=np.float32)
    m[np.arange(L), np.arange(L)] = diag
    return m.astype(dtype)


def expected_counts(dn, rows, cols, pos=None, D=0, K=0):
    """The class counts over the distinct in-window pairs a < b with an entry in rows x cols."""
    L = dn.L
    e = np.zeros((L, L), dtype=bool)
    e[rows[0]:rows[1], cols[0]:cols[1]] = True
    iu = np.triu_indices(L, 1)
    has = ((e | e.T) & in_window(L, pos, D, K))[iu]
    v, fin = dn.valid[iu][has], np.isfinite(dn.r2[iu][has])
    return {"pairs": int(has.sum()), "none_pairs": int((~v).sum()), "nonfinite_pairs": int((v & ~fin).sum()),
            "counted_pairs": int((v & fin).sum())}


def assert_same_bits(got, exp, what=""):
    """Equal shapes, dtypes, NaN positions and — elsewhere — bit patterns."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    u = {4: np.uint32, 2: np.uint16}[got.dtype.itemsize]
    gn, en = np.isnan(got), np.isnan(exp)
    assert np.array_equal(gn, en), (what, "NaN positions differ at", np.argwhere(gn != en)[:5].tolist())
    gb, eb = np.ascontiguousarray(got).view(u), np.ascontiguousarray(exp).view(u)
    bad = (gb != eb) & ~gn
    assert not bad.any(), (what, int(bad.sum()), "entries differ, first at", np.argwhere(bad)[:5].tolist(),
                           got[bad][:5].tolist(), exp[bad][:5].tolist())
