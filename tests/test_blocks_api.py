"""The LD blocks' host-only surface, no device: wld_blocks_partition and
wld_block_breaks_merge through ctypes (LdBlockBreaks.partition / .merge) on
break arrays computed in numpy from the CPU oracle on the planted case of
tests/test_gpu_blocks.py, their argument errors, and LdBlocks.site_cell /
parents / mean on hand-made arrays."""
import sys

import numpy as np
import pytest

from conftest import REPO

if REPO not in sys.path:
    sys.path.insert(0, REPO)

import test_gpu_blocks as T  # noqa: E402  (the generator and the oracle reduction; no device at import)
from weightedld_amd.api import BLOCKS_NONE, LdBlockBreaks, LdBlocks, WldError  # noqa: E402
from weightedld_amd._lib import HEAT_MAX_CELLS  # noqa: E402

NAN = np.float32("nan")


def oracle_breaks(case, stat, strong_min, last, chunks=None):
    cl = T.classes(case, stat, strong_min, last, chunks)
    fwd, bwd = T.break_arrays(cl["weak"])
    return LdBlockBreaks(fwd_weak=fwd, bwd_weak=bwd, last=last.astype(np.uint32), stat=stat,
                         strong_min=float(np.float32(strong_min)), pairs=int(cl["con"].sum()),
                         none_pairs=int(cl["none"].sum()), nonfinite_pairs=int(cl["nonfinite"].sum()),
                         strong_pairs=int(cl["strong"].sum()), weak_pairs=int(cl["weak"].sum()), tiles=1, kernel_ms=0.5)


def test_constants():
    assert BLOCKS_NONE == 0xFFFFFFFF == T.NONE


def test_planted_case_is_not_vacuous():
    T.non_vacuous(T.case1())


@pytest.mark.parametrize("K", [0, 40], ids=["nowindow", "sites40"])
@pytest.mark.parametrize("rule", ["all", "spine"])
def test_partition_of_oracle_breaks(rule, K):
    """The break-array partition (the library's) equals the partition straight
    from the weak matrix (the definition)."""
    c = T.case1()
    last = T.window_last(c.L, K=K)
    b = oracle_breaks(c, "r2", T.STRONG_R2, last)
    for m in (2, 3, 5):
        e = T.expected(c, "r2", T.STRONG_R2, rule, m, K=K)
        p = b.partition(rule, m)
        assert np.array_equal(p.first, e["first"]) and np.array_equal(p.last, e["last"]), (rule, K, m)
        assert np.array_equal(p.site_block, e["site_block"])
        assert (p.n_blocks, p.n_sites, p.rule, p.stat, p.min_sites) == (len(e["first"]), 600, rule, "r2", m)
        assert p.strong_min == b.strong_min
        assert p.pairs is None and p.informative is None and p.value_min is None and p.mean is None
        assert (p.sites >= m).all() and p.tiles == 0


def test_merge_of_oracle_breaks():
    """Breaks of the six chunks merge to the whole set's, exactly."""
    c = T.case1()
    last = T.window_last(c.L)
    whole = oracle_breaks(c, "r2", T.STRONG_R2, last)
    merged = None
    for k in range(6):
        b = oracle_breaks(c, "r2", T.STRONG_R2, last, chunks=(k, k + 1))
        merged = b if merged is None else merged.merge(b)
    for f in ("fwd_weak", "bwd_weak", "last"):
        assert np.array_equal(getattr(merged, f), getattr(whole, f)), f
    for f in ("pairs", "none_pairs", "nonfinite_pairs", "strong_pairs", "weak_pairs"):
        assert getattr(merged, f) == getattr(whole, f), f
    assert merged.tiles == 6 and merged.kernel_ms == 0.5 and merged.stat == "r2"


def small():
    """6 sites: weak pairs (0, 3), (1, 3) and (4, 5)."""
    fwd = np.array([3, 3, BLOCKS_NONE, BLOCKS_NONE, 5, BLOCKS_NONE], dtype=np.uint32)
    bwd = np.array([BLOCKS_NONE, BLOCKS_NONE, BLOCKS_NONE, 1, BLOCKS_NONE, 4], dtype=np.uint32)
    return LdBlockBreaks(fwd_weak=fwd, bwd_weak=bwd, last=np.full(6, 5, dtype=np.uint32), stat="r2", strong_min=0.5,
                         pairs=15, none_pairs=0, nonfinite_pairs=0, strong_pairs=12, weak_pairs=3, tiles=1,
                         kernel_ms=0.0)


def test_small_partition_by_hand():
    b = small()
    p = b.partition("all")
    assert p.first.tolist() == [0, 3] and p.last.tolist() == [2, 4] and p.site_block.tolist() == [0, 0, 0, 1, 1, -1]
    p = b.partition("spine")  # (0 is weak with 3; from 3, site 5 is weak with 4)
    assert p.first.tolist() == [0, 3] and p.last.tolist() == [2, 4]
    assert b.partition("all", 3).first.tolist() == [0]
    assert b.partition("all", 4).n_blocks == 0


def test_argument_errors():
    b = small()

    def refused(call, *args):
        with pytest.raises(WldError) as ei:
            call(*args)
        assert ei.value.name == "WLD_E_ARG", ei.value
        return str(ei.value)

    assert "rule" in refused(b.partition, 2)
    for m in (0, 1):
        assert "min_sites" in refused(b.partition, "all", m)
    with pytest.raises(ValueError):
        b.partition("solid")
    bad = small()
    bad.stat = 7
    assert "stat" in refused(bad.partition)
    bad = small()
    bad.strong_min = float("nan")
    assert "strong_min" in refused(bad.partition)
    # an index out of place: last before the site, a forward break at or before it, a backward one at or after it
    for field, site, value in (("last", 3, 2), ("last", 0, 6), ("fwd_weak", 2, 2), ("fwd_weak", 2, 9),
                               ("bwd_weak", 3, 3), ("bwd_weak", 0, 0)):
        bad = small()
        getattr(bad, field)[site] = value
        assert "site %d" % site in refused(bad.partition), (field, site)
    # merge: another set, statistic, threshold, window
    other = small()
    other.fwd_weak, other.bwd_weak, other.last = other.fwd_weak[:5], other.bwd_weak[:5], np.full(5, 4, dtype=np.uint32)
    other.fwd_weak[4] = BLOCKS_NONE
    refused(b.merge, other)
    for field, value in (("stat", "dprime"), ("strong_min", 0.25)):
        other = small()
        setattr(other, field, value)
        refused(b.merge, other)
    other = small()
    other.last = np.array([4, 5, 5, 5, 5, 5], dtype=np.uint32)
    refused(b.merge, other)
    m = b.merge(small())
    assert np.array_equal(m.fwd_weak, b.fwd_weak) and np.array_equal(m.bwd_weak, b.bwd_weak) and m.pairs == 30


def made():
    """9 sites, blocks [1, 3] and [5, 8]."""
    return LdBlocks(first=np.array([1, 5], dtype=np.uint32), last=np.array([3, 8], dtype=np.uint32),
                    site_block=np.array([-1, 0, 0, 0, -1, 1, 1, 1, 1], dtype=np.int32), stat="r2", rule="all",
                    strong_min=0.5, min_sites=2, pairs=np.array([3, 6], dtype=np.uint64),
                    informative=np.array([2, 0], dtype=np.uint64), strong=np.array([2, 0], dtype=np.uint64),
                    value_sum=np.array([1.5, 0.0]), value_min=np.array([0.7, NAN], dtype=np.float32), tiles=1,
                    kernel_ms=0.0)


def test_ldblocks_views():
    r = made()
    assert (r.n_blocks, r.n_sites) == (2, 9) and r.sites.tolist() == [3, 4]
    m = r.mean
    assert m[0] == 0.75 and np.isnan(m[1])
    sc = r.site_cell()
    assert sc.dtype == np.int32 and sc.tolist() == r.site_block.tolist()
    sc[0] = 5
    assert r.site_block[0] == -1, "site_cell returns a copy"
    first, last = r.parents()
    assert first.dtype == last.dtype == np.uint64 and first.tolist() == [1, 5] and last.tolist() == [3, 8]
    sm = np.array([10, 10, 11, 500, 500, 501, 2 ** 40, 2 ** 40, 2 ** 40 + 7], dtype=np.uint64)
    first, last = r.parents(sm)
    assert first.tolist() == [10, 501] and last.tolist() == [500, 2 ** 40 + 7]
    r.site_map = sm  # (as ld_blocks leaves it)
    assert r.parents()[1].tolist() == [500, 2 ** 40 + 7]
    with pytest.raises(ValueError):
        r.parents(sm[:4])
    many = HEAT_MAX_CELLS + 1
    big = LdBlocks(first=np.arange(many, dtype=np.uint32) * 2, last=np.arange(many, dtype=np.uint32) * 2 + 1,
                   site_block=np.repeat(np.arange(many, dtype=np.int32), 2), value_sum=None)
    with pytest.raises(ValueError):
        big.site_cell()
    assert big.mean is None
