"""heatmap_cells (weightedld_amd/api.py): the site -> cell map of an LD heat
map for each layout — equal runs of sites, equal coordinate bins, explicit
edges, a region — on a site_map with repeated positions, against the
definitions written out site by site.  Pure numpy: no GPU."""
import numpy as np
import pytest

from weightedld_amd.api import LdHeatmap, heatmap_cells

# parent coordinates with repeats (multi-allelic lines share a POS) and a gap
POS = np.array([100, 100, 103, 104, 104, 104, 110, 119, 120, 121, 150, 151, 151, 199, 200, 260], dtype=np.uint64)


def brute(pos, cell_of):
    """site_cell from a per-site rule (None: no cell)."""
    return np.array([-1 if cell_of(i, int(p)) is None else cell_of(i, int(p)) for i, p in enumerate(pos)],
                    dtype=np.int32)


def test_equal_runs_of_sites():
    sc, n, start = heatmap_cells(POS, sites_per_cell=5)
    assert sc.dtype == np.int32 and n == 4
    assert np.array_equal(sc, brute(POS, lambda i, p: i // 5))
    assert np.array_equal(start, POS[[0, 5, 10, 15]]) and start.dtype == np.uint64
    # without a map the coordinate is the site index; the last run is shorter
    sc, n, start = heatmap_cells(None, 11, sites_per_cell=4)
    assert n == 3 and np.array_equal(sc, np.arange(11) // 4) and np.array_equal(start, [0, 4, 8])
    # one site per cell, one cell for everything
    assert np.array_equal(heatmap_cells(POS, sites_per_cell=1)[0], np.arange(16))
    sc, n, _ = heatmap_cells(POS, sites_per_cell=100)
    assert n == 1 and not sc.any()


def test_coordinate_bins_with_repeats_and_empty_cells():
    sc, n, start = heatmap_cells(POS, cell_width=20)
    # bins on the multiples of 20 from the one at or below the first site
    assert np.array_equal(sc, brute(POS, lambda i, p: (p - 100) // 20))
    assert n == 9 and np.array_equal(start, 100 + 20 * np.arange(9))
    assert sc[0] == sc[1] and sc[3] == sc[4] == sc[5], "sites sharing a position share a cell"
    assert sorted(set(range(n)) - set(sc.tolist())) == [3, 6, 7], "cells without a site are kept"
    assert np.all(np.diff(sc) >= 0)
    # an origin that is not the first site: floor to the multiple of the width
    sc, n, start = heatmap_cells(POS + np.uint64(7), cell_width=20)
    assert start[0] == 100 and np.array_equal(sc, brute(POS + np.uint64(7), lambda i, p: (p - 100) // 20))


def test_edges_gene_boundaries():
    edges = [100, 104, 120, 150, 200]  # four genes; [150, 200) ends before site 14
    sc, n, start = heatmap_cells(POS, edges=edges)

    def cell(i, p):
        for c in range(4):
            if edges[c] <= p < edges[c + 1]:
                return c
        return None

    assert n == 4 and np.array_equal(start, edges[:-1])
    assert np.array_equal(sc, brute(POS, cell))
    assert sc[14] == -1 and sc[15] == -1 and sc[3] == 1 and sc[8] == 2
    # a gene without a site stays an empty cell
    sc, n, _ = heatmap_cells(POS, edges=[100, 122, 140, 300])
    assert n == 3 and 1 not in sc.tolist() and set(sc.tolist()) == {0, 2}


def test_region():
    # sites outside [104, 151) are on no cell; bins are relative to the region's start
    sc, n, start = heatmap_cells(POS, cell_width=10, region=(104, 151))
    assert np.array_equal(sc, brute(POS, lambda i, p: (p - 104) // 10 if 104 <= p < 151 else None))
    assert n == 5 and np.array_equal(start, 104 + 10 * np.arange(5)) and sc[2] == -1 and sc[11] == -1
    # equal runs of the region's sites only
    sc, n, start = heatmap_cells(POS, sites_per_cell=3, region=(104, 151))
    inside = [i for i, p in enumerate(POS) if 104 <= p < 151]
    want = np.full(16, -1, dtype=np.int32)
    want[inside] = np.arange(len(inside)) // 3
    assert np.array_equal(sc, want) and n == 3 and np.array_equal(start, POS[[3, 6, 9]])
    # edges cut by a region
    sc, n, _ = heatmap_cells(POS, edges=[100, 120, 300], region=(110, 200))
    assert n == 2 and np.array_equal(sc, brute(POS, lambda i, p: (0 if p < 120 else 1) if 110 <= p < 200 else None))


def test_siteset_like_inputs_and_sizes():
    with pytest.raises(ValueError):
        heatmap_cells(POS, 15, sites_per_cell=2)  # n_sites disagrees with the map
    sc, n, _ = heatmap_cells(POS, 16, sites_per_cell=2)
    assert n == 8 and sc.size == 16
    # exactly 4,096 cells is the limit
    sc, n, _ = heatmap_cells(None, 4096, sites_per_cell=1)
    assert n == 4096


@pytest.mark.parametrize("kw", [
    {},                                                   # no layout
    {"sites_per_cell": 2, "cell_width": 5},               # two layouts
    {"sites_per_cell": 0}, {"cell_width": 0},
    {"edges": [100]}, {"edges": [100, 100, 200]}, {"edges": [200, 100]},
    {"cell_width": 10, "region": (150, 104)},             # a region that ends before it starts
    {"cell_width": 10, "region": (300, 400)},             # no site in the region
    {"edges": [300, 400]},                                # no site on a cell
])
def test_argument_errors(kw):
    with pytest.raises(ValueError):
        heatmap_cells(POS, **kw)


def test_too_many_cells_and_descending_maps():
    with pytest.raises(ValueError, match="4096"):
        heatmap_cells(None, 4097, sites_per_cell=1)
    with pytest.raises(ValueError, match="4096"):
        heatmap_cells(np.array([0, 5000000], dtype=np.uint64), cell_width=1000)
    with pytest.raises(ValueError, match="4096"):
        heatmap_cells(POS, edges=np.arange(4098))
    with pytest.raises(ValueError):
        heatmap_cells(None, sites_per_cell=2)  # neither a map nor a size
    down = POS.copy()
    down[7] = 90  # a position that goes back across a bin edge
    with pytest.raises(ValueError, match="descend"):
        heatmap_cells(down, cell_width=10)
    with pytest.raises(ValueError, match="descend"):
        heatmap_cells(down, edges=[0, 100, 300])
    # equal runs of sites never look at the order of the positions
    assert np.array_equal(heatmap_cells(down, sites_per_cell=4)[0], np.arange(16) // 4)


def test_ldheatmap_mean_and_symmetric():
    count = np.array([[2, 1, 0], [0, 0, 4], [0, 0, 1]], dtype=np.uint64)
    s = np.array([[1.0, 0.25, 0.0], [0.0, 0.0, 2.0], [0.0, 0.0, 0.5]])
    mx = np.where(count > 0, np.float32(0.75), np.float32(np.nan)).astype(np.float32)
    h = LdHeatmap(count=count, sum=s, max=mx, n_cells=3)
    m = h.mean()
    assert np.array_equal(m[count > 0], [0.5, 0.25, 0.5, 0.5]) and np.isnan(m[count == 0]).all()
    for f in ("count", "sum", "max", "mean"):
        sym = h.symmetric(f)
        src = m if f == "mean" else getattr(h, f)
        assert np.array_equal(np.triu(sym), np.triu(src), equal_nan=True)
        assert np.array_equal(sym, sym.T, equal_nan=True)
    assert h.symmetric("count")[2, 1] == 4 and count[2, 1] == 0, "a copy: the map itself is unchanged"
    with pytest.raises(ValueError):
        h.symmetric("min")
