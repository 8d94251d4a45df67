"""LdPartners.parents and LdPartners.rows (weightedld_amd/api.py) on hand-made
arrays: no library call, no device."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO

if REPO not in sys.path:
    sys.path.insert(0, REPO)

from weightedld_amd.api import PARTNERS_MAX_K, PARTNERS_NONE, LdPartners  # noqa: E402

NAN = np.float32("nan")


def made():
    """4 sites, k = 3: site 0 has two partners, site 1 three, site 2 none, site 3 one."""
    partner = np.array([[2, 1, PARTNERS_NONE], [0, 3, 2], [PARTNERS_NONE] * 3, [1, PARTNERS_NONE, PARTNERS_NONE]],
                       dtype=np.uint32)
    filled = partner != PARTNERS_NONE
    vals = np.arange(12, dtype=np.float32).reshape(4, 3)
    return LdPartners(count=filled.sum(axis=1).astype(np.uint32), partner=partner,
                      d=np.where(filled, -vals, NAN).astype(np.float32),
                      d_prime=np.where(filled, vals / 16, NAN).astype(np.float32),
                      r2=np.where(filled, 1 - vals / 16, NAN).astype(np.float32),
                      pairs=6, none_pairs=0, passing_pairs=3, tiles=1, kernel_ms=0.0, merge_ms=0.0)


def test_shape_and_constants():
    p = made()
    assert (p.n_sites, p.k) == (4, 3)
    assert PARTNERS_MAX_K == 64 and PARTNERS_NONE == 0xFFFFFFFF


def test_parents_identity_and_map():
    p = made()
    site, part = p.parents()
    assert site.dtype == part.dtype == np.uint64
    assert site.tolist() == [0, 1, 2, 3]
    top = np.iinfo(np.uint64).max
    assert part.tolist() == [[2, 1, top], [0, 3, 2], [top] * 3, [1, top, top]]
    sm = np.array([10, 10, 500, 2 ** 40], dtype=np.uint64)  # repeats and a coordinate past 32 bits
    site, part = p.parents(sm)
    assert site.tolist() == sm.tolist()
    assert part.tolist() == [[500, 10, top], [10, 2 ** 40, 500], [top] * 3, [10, top, top]]
    assert p.partner[0, 0] == 2, "the lists themselves stay in loaded indices"
    with pytest.raises(ValueError):
        p.parents(sm[:3])


def test_rows_by_site_then_rank():
    p = made()
    site, part, rank, d, dp, r2 = p.rows()
    assert site.tolist() == [0, 0, 1, 1, 1, 3]
    assert part.tolist() == [2, 1, 0, 3, 2, 1]
    assert rank.tolist() == [0, 1, 0, 1, 2, 0] and rank.dtype == np.uint32
    flat = [0, 1, 3, 4, 5, 9]
    assert np.array_equal(d, p.d.reshape(-1)[flat]) and np.array_equal(dp, p.d_prime.reshape(-1)[flat])
    assert np.array_equal(r2, p.r2.reshape(-1)[flat])
    assert len(site) == int(p.count.sum())
    sm = np.array([7, 9, 11, 13], dtype=np.uint64)
    site, part, rank2, *_ = p.rows(sm)
    assert site.tolist() == [7, 7, 9, 9, 9, 13] and part.tolist() == [11, 9, 7, 13, 11, 9]
    assert np.array_equal(rank, rank2)


def test_rows_of_an_empty_result():
    z = LdPartners(count=np.zeros(3, dtype=np.uint32), partner=np.full((3, 2), PARTNERS_NONE, dtype=np.uint32),
                   d=np.full((3, 2), NAN), d_prime=np.full((3, 2), NAN), r2=np.full((3, 2), NAN), pairs=0,
                   none_pairs=0, passing_pairs=0, tiles=0, kernel_ms=0.0, merge_ms=0.0)
    assert all(len(x) == 0 for x in z.rows())
    assert os.path.isdir(REPO)
