"""The Python argument checks of the partitioned LD scores (annot_matrix,
Context.run_annot_scores, ld_annot_scores, LdAnnotScores.merge in
weightedld_amd/api.py): every refusal is raised before any device call, so
they are checked here without a device."""
import sys

import numpy as np
import pytest

from conftest import REPO

if REPO not in sys.path:
    sys.path.insert(0, REPO)

import weightedld_amd as W  # noqa: E402
from weightedld_amd.api import ANNOT_MAX, LdAnnotScores, annot_matrix, ld_annot_scores  # noqa: E402


class NoDevice:
    """Stands in for a Context: any use of it is a device call."""

    def __getattr__(self, name):
        raise AssertionError("device call: " + name)


def test_exports():
    assert ANNOT_MAX == 128 and W.ANNOT_MAX == 128
    for name in ("ld_annot_scores", "LdAnnotScores", "annot_matrix"):
        assert name in W.__all__ and hasattr(W, name)
    assert hasattr(W.Context, "run_annot_scores")


def test_accepted_matrices():
    a = np.arange(12, dtype=np.float32).reshape(4, 3)
    assert annot_matrix(a) is a or np.shares_memory(annot_matrix(a), a)
    t = annot_matrix(a.T[:3])  # not contiguous: copied, same values
    assert t.flags.c_contiguous and np.array_equal(t, a.T[:3])
    for exact in (np.eye(4, dtype=bool), np.eye(4, dtype=np.int64), np.full((4, 2), 0.25), np.full((4, 2), -3, dtype=np.int8)):
        got = annot_matrix(exact, 4)
        assert got.dtype == np.float32 and np.array_equal(got, exact.astype(np.float64))
    assert annot_matrix(np.zeros((0, 2), dtype=np.float32), 0).shape == (0, 2)
    assert annot_matrix(np.ones((3, ANNOT_MAX), dtype=np.float32)).shape == (3, 128)


@pytest.mark.parametrize("bad,exc", [
    (np.ones(4, dtype=np.float32), ValueError),                   # one dimension
    (np.ones((4, 2, 1), dtype=np.float32), ValueError),           # three
    (np.ones((4, 0), dtype=np.float32), ValueError),              # no column
    (np.ones((4, ANNOT_MAX + 1), dtype=np.float32), ValueError),  # too many
    (np.ones((5, 2), dtype=np.float32), ValueError),              # rows != sites
    (np.full((4, 2), 0.1), TypeError),                            # float64 that would round
    (np.full((4, 2), 2 ** 24 + 1), TypeError),                    # an integer that would round
    (np.full((4, 2), 1e60), TypeError),                           # would overflow to inf
    (np.ones((4, 2), dtype=np.complex64), TypeError),
    (np.array([["1", "2"]] * 4), TypeError),
    (np.array([[1.0, None]] * 4, dtype=object), TypeError),
    (np.array([[1.0, np.nan]] * 4, dtype=np.float32), ValueError),
    (np.array([[1.0, np.inf]] * 4, dtype=np.float32), ValueError),
    (np.array([[1.0, -np.inf]] * 4), ValueError),                 # exact in float32, still not finite
])
def test_refused_matrices(bad, exc):
    with pytest.raises(exc):
        annot_matrix(bad, 4)


def test_the_first_offending_value_is_named():
    a = np.zeros((6, 3), dtype=np.float32)
    a[4, 1] = np.nan
    a[2, 2] = np.inf
    with pytest.raises(ValueError, match=r"annot\[2, 2\]"):
        annot_matrix(a)


def test_ld_annot_scores_refuses_before_any_device_call():
    ss = W.SiteSet.from_buffer(np.zeros((4, 6), dtype=np.uint8))
    w = np.ones(6, dtype=np.float32)
    good = np.ones((4, 2), dtype=np.float32)
    for annot, kw, exc in ((np.ones((3, 2), dtype=np.float32), {}, ValueError),
                           (np.full((4, 2), 0.1), {}, TypeError),
                           (np.full((4, 2), np.nan, dtype=np.float32), {}, ValueError),
                           (np.ones((4, 129), dtype=np.float32), {}, ValueError),
                           (good, {"names": ["only one"]}, ValueError)):
        with pytest.raises(exc):
            ld_annot_scores(ss, w, annot, ctx=NoDevice(), **kw)
    with pytest.raises(ValueError):
        ld_annot_scores(ss, w[:5], good, ctx=NoDevice())


def made(seed, C=2, self_term=False):
    rng = np.random.default_rng(seed)
    return LdAnnotScores(score=rng.standard_normal((5, C)), partners=rng.integers(0, 9, 5).astype(np.uint32),
                         pairs=10 + seed, none_pairs=1, nonfinite_pairs=seed, counted_pairs=9, self_term=self_term,
                         tiles=3, kernel_ms=0.5 * seed)


def test_merge():
    a, b = made(1), made(2)
    score, partners = a.score + b.score, a.partners + b.partners
    assert a.merge(b) is a
    assert (a.pairs, a.none_pairs, a.nonfinite_pairs, a.counted_pairs, a.tiles, a.kernel_ms) == (23, 2, 3, 18, 6, 1.0)
    assert np.array_equal(a.score, score) and np.array_equal(a.partners, partners) and a.partners.dtype == np.uint32
    assert (a.n_sites, a.n_annot) == (5, 2)
    for other in (made(3, C=3), made(3, self_term=True)):
        with pytest.raises(ValueError):
            a.merge(other)
    assert a.pairs == 23
