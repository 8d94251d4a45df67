"""Python mirror of the weighted_ld crate's public surface (rust/weighted_ld/src/lib.rs).

Same names, argument meaning and results as the Rust functions, implemented on
the C ABI of libweightedld.so: the host pre-pass (FASTA, site filter, Henikoff
weights) runs in the library's C++ host code, the all-pairs hot path on the
gfx950 GPU.  There is no CPU fallback for the hot path.
"""
import atexit
import ctypes
import weakref
import enum
from collections import namedtuple

import numpy as np

from ._lib import (ANNOT_MAX, ANNOT_SELF, AnnotScoresC, BLOCKS_ABS_DPRIME, BLOCKS_ALL, BLOCKS_NONE, BLOCKS_R2, BLOCKS_SPINE, BlockBreaksC, BlocksC,
                   HEAT_ABS_DPRIME, HEAT_MAX_CELLS, HEAT_R2, KERNEL_AUTO, KERNEL_MFMA, KERNEL_VALU, MATRIX_F16, MATRIX_F32,
                   MATRIX_STATS, MATRIX_ZERO_MISSING, APPLY_X_F32, APPLY_X_F64, SOLVE_MODES, BandedCholInfoC, BandedOmegaInfoC, BandedPairsumInfoC, OmegaC, MatrixBandedInfoC, MatrixInfoC, OPTIONS,
                   PARTNERS_MAX_K, PARTNERS_NONE, PROGRESS_FN, Heatmap, Pairs, PartnersC, Prune, RunStats, Summary,
                   TargetRowsC, WldError, check, lib)

__all__ = [
    "Symbol", "SymbolHistogram", "SiteSet", "LdStats", "PairStore", "read_fasta", "read_vcf",
    "is_site_of_interest", "henikoff_weights", "single_weighted_ld_pair", "all_weighted_ld_pairs",
    "ld_summary", "LdSummary", "ld_heatmap", "LdHeatmap", "heatmap_cells", "ld_annot_scores", "LdAnnotScores", "annot_matrix", "ANNOT_MAX", "ld_matrix", "LdMatrixInfo", "matrix_args", "matrix_region", "ld_banded", "LdBandedInfo", "banded_args", "banded_from_dense", "banded_to_dense", "banded_matmul_host", "banded_cg_solve", "banded_cholesky_host", "banded_solve_host", "banded_logdet", "banded_chol_args", "banded_solve_args", "LdBandedCholInfo", "banded_pairsum_host", "banded_nonfinite_host", "banded_omega_host", "banded_pairsum_args", "omega_args", "omega_splits", "ld_omega", "LdOmega", "LdPairsumInfo", "OMEGA_NONE", "ld_prune", "LdPrune", "maf_priority", "ld_targets", "TargetRows", "ld_partners", "LdPartners", "PARTNERS_MAX_K", "PARTNERS_NONE", "ld_blocks", "LdBlocks", "LdBlockBreaks", "BLOCKS_NONE", "Context", "default_context", "KERNEL_AUTO", "KERNEL_VALU", "KERNEL_MFMA", "OPTIONS", "WldError",
]


def _p(a, ct):
    return a.ctypes.data_as(ctypes.POINTER(ct))


class Symbol(enum.IntEnum):
    """lib.rs:20-29 (#[repr(u8)])."""
    A = 0
    C = 1
    G = 2
    T = 3
    Missing = 4
    Unknown = 5

    @staticmethod
    def from_char(c):
        """lib.rs:53-64."""
        return {"a": Symbol.A, "A": Symbol.A, "c": Symbol.C, "C": Symbol.C, "g": Symbol.G, "G": Symbol.G,
                "t": Symbol.T, "T": Symbol.T, "-": Symbol.Missing}.get(c, Symbol.Unknown)

    def is_acgt(self):
        return self <= Symbol.T

    def is_acgtm(self):
        return self <= Symbol.Missing


def symbols_from_str(s):
    return np.array([Symbol.from_char(c) for c in s], dtype=np.uint8)


class SymbolHistogram:
    """lib.rs:72-141."""

    def __init__(self, counts):
        self.data = np.asarray(counts, dtype=np.uint64).reshape(6)

    @staticmethod
    def from_slice(symbols):
        s = np.ascontiguousarray(symbols, dtype=np.uint8)
        h = np.zeros(6, dtype=np.uint64)
        check(lib().wld_histogram(_p(s, ctypes.c_uint8), s.size, _p(h, ctypes.c_uint64)), "histogram")
        return SymbolHistogram(h)

    def __getitem__(self, sym):
        return int(self.data[int(sym)])

    def major_minor_symbols(self):
        a, b = ctypes.c_int(), ctypes.c_int()
        h = np.ascontiguousarray(self.data)
        check(lib().wld_major_minor(_p(h, ctypes.c_uint64), ctypes.byref(a), ctypes.byref(b)), "major_minor")
        return (Symbol(a.value) if a.value >= 0 else None, Symbol(b.value) if b.value >= 0 else None)


class SiteSet:
    """lib.rs:158-275: site-major symbol buffer, optional site_map, histograms."""

    def __init__(self, handle):
        self._h = ctypes.c_void_p(handle)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and lib is not None:
            try:
                lib().wld_siteset_free(h)
            except Exception:
                pass
            self._h = None

    @staticmethod
    def from_buffer(site_major, site_map=None):
        """Builds a SiteSet from a [n_sites, n_seqs] uint8 array of Symbol codes."""
        buf = np.ascontiguousarray(site_major, dtype=np.uint8)
        if buf.ndim != 2:
            raise ValueError("site_major must be [n_sites, n_seqs]")
        sm = None if site_map is None else np.ascontiguousarray(site_map, dtype=np.uint64)
        out = ctypes.c_void_p()
        check(lib().wld_siteset_from_buffer(_p(buf, ctypes.c_uint8), buf.shape[0], buf.shape[1],
                                            None if sm is None else _p(sm, ctypes.c_uint64), ctypes.byref(out)),
              "siteset_from_buffer")
        return SiteSet(out.value)

    @staticmethod
    def from_strs(seqs):
        """lib.rs:208-228 (test helper): one string per sequence."""
        return SiteSet.from_buffer(np.stack([symbols_from_str(s) for s in seqs], axis=1))

    def n_sites(self):
        return lib().wld_siteset_n_sites(self._h)

    def n_seqs(self):
        return lib().wld_siteset_n_seqs(self._h)

    @property
    def buffer(self):
        """SiteSet.buffer as a [n_sites, n_seqs] uint8 array (copy)."""
        L, N = self.n_sites(), self.n_seqs()
        if L * N == 0:
            return np.zeros((L, N), dtype=np.uint8)
        p = lib().wld_siteset_buffer(self._h)
        return np.ctypeslib.as_array(p, shape=(L * N,)).reshape(L, N).copy()

    @property
    def site_map(self):
        p = lib().wld_siteset_site_map(self._h)
        if not p:
            return None
        return np.ctypeslib.as_array(p, shape=(self.n_sites(),)).copy()

    def parent_site_index(self, idx):
        return int(lib().wld_siteset_parent_site_index(self._h, idx))

    def site_symbols(self, index):
        return self.buffer[index]

    def site_histogram(self, index):
        h = np.zeros(6, dtype=np.uint64)
        check(lib().wld_siteset_histogram(self._h, index, _p(h, ctypes.c_uint64)), "site_histogram")
        return SymbolHistogram(h)

    def filter_sites_of_interest(self, min_acgt=0.8, min_minor=0.02, max_minor=0.5):
        """main.rs:139-143: filter_by(|s| is_site_of_interest(s, ceil(min_acgt*N), min_minor, max_minor))."""
        out = ctypes.c_void_p()
        check(lib().wld_siteset_filter_sites_of_interest(self._h, min_acgt, min_minor, max_minor,
                                                         ctypes.byref(out)), "filter_by")
        return SiteSet(out.value)


def read_fasta(path):
    """read_fasta + SiteSet::from_multiseq (lib.rs:277-307, 176-206)."""
    out = ctypes.c_void_p()
    check(lib().wld_read_fasta(str(path).encode(), ctypes.byref(out)), "read_fasta")
    return SiteSet(out.value)


def read_vcf(path):
    """VCF reader with WeightedLD.py handle_vcf semantics (WeightedLD.py:311-379)."""
    out = ctypes.c_void_p()
    check(lib().wld_read_vcf(str(path).encode(), ctypes.byref(out)), "read_vcf")
    return SiteSet(out.value)


def is_site_of_interest(site, min_acgt, min_minor, max_minor):
    """lib.rs:309-338 (min_acgt is a count)."""
    s = np.ascontiguousarray(site, dtype=np.uint8)
    return bool(lib().wld_is_site_of_interest(_p(s, ctypes.c_uint8), s.size, int(min_acgt), min_minor, max_minor))


def henikoff_weights(site_set):
    """lib.rs:340-380."""
    w = np.zeros(site_set.n_seqs(), dtype=np.float32)
    check(lib().wld_henikoff_weights(site_set._h, _p(w, ctypes.c_float)), "henikoff_weights")
    return w


LdStats = namedtuple("LdStats", ["r2", "d", "d_prime"])  # lib.rs:382-387


class PairStore:
    """PairStore<LdStats> (lib.rs:529-576) as structure-of-arrays in reference order."""

    def __init__(self, site_a, site_b, d, d_prime, r2):
        self.site_a, self.site_b, self.d, self.d_prime, self.r2 = site_a, site_b, d, d_prime, r2

    def __len__(self):
        return int(self.site_a.size)

    def len(self):
        return len(self)

    def iter(self):
        for i in range(len(self)):
            yield (int(self.site_a[i]), int(self.site_b[i]),
                   LdStats(float(self.r2[i]), float(self.d[i]), float(self.d_prime[i])))

    __iter__ = iter


class LdSummary:
    """wld_summary as numpy arrays and ints (Context.run_summary, ld_summary):
    the class counts (pairs = none_pairs + nonfinite_pairs + counted_pairs),
    r2_sum, per LOADED site score (sum of r2 over the site's counted pairs)
    and partners (their number), and with bins bin_pairs / bin_r2_sum
    (bin k: distances [k bin_width, (k + 1) bin_width), the last bin open
    ended; None without bins)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def mean_r2(self):
        """Per-bin mean r2 (nan for an empty bin); None without bins."""
        if self.bin_pairs is None:
            return None
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.bin_pairs > 0, self.bin_r2_sum / self.bin_pairs, np.nan)


class LdHeatmap:
    """wld_heatmap as numpy arrays and ints (Context.run_heatmap, ld_heatmap):
    count (uint64), sum (float64) and max (float32, NaN where count is 0) as
    (n_cells, n_cells) arrays — cell (i, j), i <= j, holds the counted pairs
    a < b with site a on cell i and site b on cell j; the lower triangle is
    empty — the class counts (pairs = none_pairs + nonfinite_pairs +
    counted_pairs), stat ("r2" or "dprime"), tiles and kernel_ms.  From
    ld_heatmap also cell_start, the parent coordinate each cell begins at."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def mean(self):
        """Per-cell mean of the value (NaN where count is 0)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.count > 0, self.sum / self.count, np.nan)

    def symmetric(self, field="mean"):
        """`field` ("count", "sum", "max" or "mean") with the upper triangle
        mirrored into the lower one: the square image of a heat-map plot."""
        if field not in ("count", "sum", "max", "mean"):
            raise ValueError("field must be \"count\", \"sum\", \"max\" or \"mean\"")
        a = (self.mean() if field == "mean" else getattr(self, field)).copy()
        lo = np.tril_indices(a.shape[0], -1)
        a[lo] = a.T[lo]
        return a


HEAT_STATS = {"r2": HEAT_R2, "dprime": HEAT_ABS_DPRIME}


class LdAnnotScores:
    """wld_annot_scores as numpy arrays and ints (Context.run_annot_scores,
    ld_annot_scores): score, the [n_sites, n_annot] float64 partitioned LD
    scores (row i: sum over site i's counted pairs of r2 times the partner's
    annotation row, plus the site's own row with self_term), partners (uint32,
    [n_sites], the counted pairs of each site), the class counts (pairs =
    none_pairs + nonfinite_pairs + counted_pairs), self_term, tiles and
    kernel_ms.  From ld_annot_scores also names, where given."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_sites(self):
        return int(self.score.shape[0])

    @property
    def n_annot(self):
        return int(self.score.shape[1])

    def merge(self, other):
        """Adds other — the result of a disjoint chunk range of the same load,
        annotations and self_term — into this one (wld_annot_scores_merge:
        counts, scores, partners and tiles add, kernel_ms is the larger);
        returns self.  ValueError when the shapes or self_term differ."""
        if self.score.shape != other.score.shape or bool(self.self_term) != bool(other.self_term):
            raise ValueError("results of different shapes or self_term do not merge")
        for f in ("pairs", "none_pairs", "nonfinite_pairs", "counted_pairs", "tiles"):
            setattr(self, f, getattr(self, f) + getattr(other, f))
        self.score = self.score + other.score
        self.partners = self.partners + other.partners
        self.kernel_ms = max(self.kernel_ms, other.kernel_ms)
        return self


LdMatrixInfo = namedtuple("LdMatrixInfo", ["rows", "cols", "stat", "dtype", "zero_missing", "pairs", "none_pairs",
                                           "nonfinite_pairs", "counted_pairs", "tiles", "kernel_ms"])
LdMatrixInfo.__doc__ = """wld_matrix_info (Context.run_matrix, ld_matrix): rows and cols, the (begin, end)
loaded-site ranges of the rectangle as resolved; stat ("r2", "r", "d", "dprime"), dtype ("float32", "float16"),
zero_missing; the class counts of the distinct in-window pairs with an entry in the rectangle; the 64x64 tiles
launched and kernel_ms.  From ld_matrix also sites, the parent coordinates of the rows."""

_MATRIX_DTYPES = {"float32": MATRIX_F32, "float16": MATRIX_F16}


def _site_range(x, n_sites, what):
    if x is None:
        return 0, int(n_sites)
    try:
        b, e = int(x[0]), int(x[1])
    except (TypeError, IndexError, ValueError):
        raise ValueError("%s must be None or a (begin, end) pair of loaded site indices" % what)
    if len(x) != 2 or b < 0 or e <= b or e > int(n_sites):
        raise ValueError("%s [%d, %d) must be a non-empty range within the %d loaded sites" % (what, b, e, int(n_sites)))
    return b, e


def matrix_args(n_sites, rows=None, cols=None, stat="r", dtype="float32", out=None):
    """Context.run_matrix's arguments checked before any device call: returns
    (rows, cols, stat id, dtype id, kind, ld) with rows / cols resolved (begin,
    end) pairs, kind None (no out), "numpy" or "device", and ld the row stride
    of out in elements (the width without out).  ValueError on anything the
    call would refuse: a range outside the n_sites loaded sites, an unknown
    stat or dtype, an out of the wrong shape, dtype, strides or device kind."""
    rows, cols = _site_range(rows, n_sites, "rows"), _site_range(cols, n_sites, "cols")
    if stat not in MATRIX_STATS:
        raise ValueError("stat must be one of %s" % ", ".join('"%s"' % k for k in MATRIX_STATS))
    name = np.dtype(dtype).name if not isinstance(dtype, str) else dtype
    if name not in _MATRIX_DTYPES:
        raise ValueError('dtype must be "float32" or "float16"')
    shape = (rows[1] - rows[0], cols[1] - cols[0])
    if out is None:
        return rows, cols, MATRIX_STATS[stat], _MATRIX_DTYPES[name], None, shape[1]
    if isinstance(out, np.ndarray):
        kind, oname, strides = "numpy", out.dtype.name, tuple(x // out.itemsize if x % out.itemsize == 0 else -1
                                                               for x in out.strides)
        if not out.flags.writeable:
            raise ValueError("out is read-only")
    elif all(hasattr(out, a) for a in ("data_ptr", "stride", "dtype", "shape", "device")):
        kind, oname, strides = "device", str(out.dtype).replace("torch.", ""), tuple(int(x) for x in out.stride())
        if getattr(out.device, "type", "") != "cuda":
            raise ValueError("a tensor out must be on the context's GPU, not on %s" % (out.device,))
    else:
        raise ValueError("out must be a numpy array or a device tensor (data_ptr, stride, dtype, shape, device)")
    if tuple(int(x) for x in out.shape) != shape:
        raise ValueError("out has shape %s; the rectangle is %s" % (tuple(out.shape), shape))
    if oname != name:
        raise ValueError("out has dtype %s; dtype is %s" % (oname, name))
    if strides[1] != 1 and shape[1] > 1:
        raise ValueError("out must have contiguous rows (last stride 1)")
    if strides[0] < shape[1] and shape[0] > 1:
        raise ValueError("out's row stride %d is below the width %d" % (strides[0], shape[1]))
    return rows, cols, MATRIX_STATS[stat], _MATRIX_DTYPES[name], kind, max(strides[0], shape[1])


def matrix_region(site_map, n_sites, region):
    """The loaded-site range [begin, end) of region = (start, stop), parent
    coordinates, start <= pos < stop (heatmap_cells' rule; site_map None:
    coordinate = site index).  ValueError: a malformed or empty region, or a
    site_map that descends (the region's sites would not be one range)."""
    pos = np.arange(int(n_sites), dtype=np.int64) if site_map is None else np.asarray(site_map).astype(np.int64).reshape(-1)
    if pos.size != int(n_sites):
        raise ValueError("site_map has %d entries for %d sites" % (pos.size, int(n_sites)))
    try:
        start, stop = int(region[0]), int(region[1])
    except (TypeError, IndexError, ValueError):
        raise ValueError("region must be (start, stop)")
    if len(region) != 2 or start < 0 or stop < start:
        raise ValueError("region must be (start, stop) with 0 <= start <= stop")
    if np.any(np.diff(pos) < 0):
        raise ValueError("a region needs a non-decreasing site_map")
    b, e = int(np.searchsorted(pos, start, side="left")), int(np.searchsorted(pos, stop, side="left"))
    if e <= b:
        raise ValueError("no site lies in the region [%d, %d)" % (start, stop))
    return b, e


LdBandedInfo = namedtuple("LdBandedInfo", ["rows", "bandwidth", "stat", "dtype", "zero_missing", "pairs", "none_pairs",
                                           "nonfinite_pairs", "counted_pairs", "tiles", "kernel_ms"])
LdBandedInfo.__doc__ = """wld_matrix_banded_info (Context.run_matrix_banded, ld_banded): rows, the (begin, end)
loaded-site range as resolved; bandwidth K (the band has K + 1 columns); stat, dtype, zero_missing; the class counts of
the in-window pairs a < b with a in rows; the 64x64 tiles launched and kernel_ms."""


def _out_layout(out, shape, name):
    """(kind, row stride in elements) of an out array of Context.run_matrix's kinds, checked against shape and
    the dtype name; ValueError otherwise."""
    if isinstance(out, np.ndarray):
        kind, oname, strides = "numpy", out.dtype.name, tuple(x // out.itemsize if x % out.itemsize == 0 else -1
                                                               for x in out.strides)
        if not out.flags.writeable:
            raise ValueError("out is read-only")
    elif all(hasattr(out, a) for a in ("data_ptr", "stride", "dtype", "shape", "device")):
        kind, oname, strides = "device", str(out.dtype).replace("torch.", ""), tuple(int(x) for x in out.stride())
        if getattr(out.device, "type", "") != "cuda":
            raise ValueError("a tensor out must be on the context's GPU, not on %s" % (out.device,))
    else:
        raise ValueError("out must be a numpy array or a device tensor (data_ptr, stride, dtype, shape, device)")
    if tuple(int(x) for x in out.shape) != tuple(shape):
        raise ValueError("out has shape %s; the call writes %s" % (tuple(out.shape), tuple(shape)))
    if oname != name:
        raise ValueError("out has dtype %s; dtype is %s" % (oname, name))
    if strides[1] != 1 and shape[1] > 1:
        raise ValueError("out must have contiguous rows (last stride 1)")
    if strides[0] < shape[1] and shape[0] > 1:
        raise ValueError("out's row stride %d is below the width %d" % (strides[0], shape[1]))
    return kind, max(strides[0], shape[1])


def banded_args(n_sites, needed, rows=None, bandwidth=None, stat="r", dtype="float32", out=None):
    """Context.run_matrix_banded's arguments checked before any device call:
    returns (rows, bandwidth, stat id, dtype id, kind, ld) with rows a resolved
    (begin, end) pair, bandwidth resolved (None: needed, the width the window
    needs — Context.matrix_banded_width), kind None (no out), "numpy" or
    "device", and ld the row stride of out in elements (bandwidth + 1 without
    out).  ValueError on anything the call would refuse: a range outside the
    n_sites loaded sites, a bandwidth below needed, an unknown stat or dtype, an
    out of the wrong shape ([rows, bandwidth + 1]), dtype, strides or kind."""
    rows = _site_range(rows, n_sites, "rows")
    if stat not in MATRIX_STATS:
        raise ValueError("stat must be one of %s" % ", ".join('"%s"' % k for k in MATRIX_STATS))
    name = np.dtype(dtype).name if not isinstance(dtype, str) else dtype
    if name not in _MATRIX_DTYPES:
        raise ValueError('dtype must be "float32" or "float16"')
    needed = int(needed)
    if bandwidth is None:
        bandwidth = needed
    try:
        K = int(bandwidth)
    except (TypeError, ValueError):
        raise ValueError("bandwidth must be None or an integer")
    if K != bandwidth or K < 0 or K > 0xFFFFFFFF:
        raise ValueError("bandwidth must be None or an integer in [0, 2^32)")
    if K < needed:
        raise ValueError("bandwidth %d would drop in-window pairs; the window needs bandwidth %d" % (K, needed))
    shape = (rows[1] - rows[0], K + 1)
    if out is None:
        return rows, K, MATRIX_STATS[stat], _MATRIX_DTYPES[name], None, shape[1]
    kind, ld = _out_layout(out, shape, name)
    return rows, K, MATRIX_STATS[stat], _MATRIX_DTYPES[name], kind, ld


def banded_from_dense(M, K):
    """The upper band of the square matrix M in the banded layout: B[i, k] =
    M[i, i + k] for k = 0..K, 0 where i + k >= n.  numpy, M's dtype."""
    M = np.asarray(M)
    if M.ndim != 2 or M.shape[0] != M.shape[1]:
        raise ValueError("M must be a square matrix")
    K = int(K)
    if K < 0:
        raise ValueError("K must be >= 0")
    n = M.shape[0]
    B = np.zeros((n, K + 1), dtype=M.dtype)
    for k in range(min(K, n - 1) + 1):
        B[:n - k, k] = M.diagonal(k)
    return B


def banded_to_dense(B, n=None):
    """The symmetric n x n matrix of the band B ([n, K + 1]; n None: B's rows):
    D[i, i + k] = D[i + k, i] = B[i, k] for i + k < n, 0 beyond the band.
    Elements with i + k >= n are not read.  numpy, B's dtype."""
    B = np.asarray(B)
    if B.ndim != 2 or B.shape[1] < 1:
        raise ValueError("B must be a [n, K + 1] band")
    n = B.shape[0] if n is None else int(n)
    if n != B.shape[0]:
        raise ValueError("B has %d rows for %d sites" % (B.shape[0], n))
    D = np.zeros((n, n), dtype=B.dtype)
    i = np.arange(n)
    for k in range(min(B.shape[1], n)):
        D[i[:n - k], i[:n - k] + k] = B[:n - k, k]
        D[i[:n - k] + k, i[:n - k]] = B[:n - k, k]
    return D


def banded_matmul_host(B, X):
    """The f64 reference of Context.banded_apply on the host: Y = S X for the
    symmetric matrix S of the band B ([n, K + 1]) and X ([n] or [n, n_cols]),
    in float64: Y[i] = sum_k B[i, k] X[i + k] + sum_{k >= 1} B[i - k, k] X[i - k].
    Elements with i + k >= n are not read.  numpy."""
    B = np.asarray(B)
    X = np.asarray(X)
    if B.ndim != 2 or B.shape[1] < 1:
        raise ValueError("B must be a [n, K + 1] band")
    n = B.shape[0]
    if X.ndim not in (1, 2) or X.shape[0] != n:
        raise ValueError("X must be [n] or [n, n_cols] with n = %d" % n)
    Bd = B.astype(np.float64)
    Xd = X.astype(np.float64).reshape(n, -1)
    Y = np.zeros_like(Xd)
    for k in range(min(B.shape[1], n)):
        b = Bd[:n - k, k:k + 1]
        Y[:n - k] += b * Xd[k:]
        if k:
            Y[k:] += b * Xd[:n - k]
    return Y.reshape(X.shape)


def banded_cg_solve(apply, B, b, ridge=0.0, tol=1e-8, max_iter=None):
    """Plain conjugate gradients for (S + ridge I) x = b, S the symmetric
    matrix of the band B and apply(B, v) its product with a vector (on whatever
    array type apply takes: Context.banded_apply on device tensors,
    banded_matmul_host on numpy arrays).  b is one right-hand side ([n] or
    [n, 1]).  Returns (x, iterations, relative residual |b - A x| / |b|,
    converged): converged is True once the residual, recomputed from x, is <=
    tol within max_iter iterations (None: 10 n).

    The band of a weighted, pairwise-masked correlation matrix need NOT be
    positive definite (every pair has its own mask, and a window cuts the
    matrix): where the curvature p.A p of a search direction is not positive
    the iteration stops with converged False and the best x so far; a ridge
    makes the system definite."""
    def f64(a):
        return a.double() if hasattr(a, "double") else np.asarray(a, dtype=np.float64)

    def dot(u, v):
        return float((u * v).sum())

    b = f64(b)
    if len(b.shape) not in (1, 2) or (len(b.shape) == 2 and b.shape[1] != 1):
        raise ValueError("b must be one right-hand side, [n] or [n, 1]")
    n = int(b.shape[0])
    if not (tol > 0):
        raise ValueError("tol must be > 0")
    max_iter = 10 * n if max_iter is None else int(max_iter)
    ridge = float(ridge)

    def A(v):
        return f64(apply(B, v)) + ridge * v

    x = b.new_zeros(b.shape) if hasattr(b, "new_zeros") else np.zeros_like(b)
    bnorm = dot(b, b) ** 0.5
    if bnorm == 0.0:
        return x, 0, 0.0, True
    r = b + 0.0
    p = r
    rs = dot(r, r)
    it = 0
    while it < max_iter:
        Ap = A(p)
        curv = dot(p, Ap)
        if not curv > 0.0:  # (also NaN)
            return x, it, rs ** 0.5 / bnorm, False
        it += 1
        alpha = rs / curv
        x = x + alpha * p
        r = r - alpha * Ap
        rs_new = dot(r, r)
        if rs_new ** 0.5 <= tol * bnorm:
            r = b - A(x)  # the residual itself, not its recurrence
            rs_new = dot(r, r)
            if rs_new ** 0.5 <= tol * bnorm:
                return x, it, rs_new ** 0.5 / bnorm, True
            p, rs = r, rs_new  # restart from it
            continue
        p = r + (rs_new / rs) * p
        rs = rs_new
    return x, it, rs ** 0.5 / bnorm, False


LdBandedCholInfo = namedtuple("LdBandedCholInfo", ["ok", "first_bad", "min_pivot", "kernel_ms"])
LdBandedCholInfo.__doc__ = """wld_banded_chol_info (Context.banded_cholesky): ok, True when every pivot was > 0;
first_bad, None when ok, else the first row whose pivot was not > 0 (NaN included); min_pivot, the smallest U[i, 0] of the
rows factored (a conditioning hint); kernel_ms."""


def _band_f64(B, ridge, diag):
    """(A's band in float64 with the shifted diagonal, n, K) of the host twins: the diagonal is
    fl(fl(B[i, 0] + ridge) + diag[i]), the device's own rounding."""
    B = np.asarray(B)
    if B.ndim != 2 or B.shape[0] < 1 or B.shape[1] < 1:
        raise ValueError("B must be a [n, K + 1] band")
    ridge = float(ridge)
    if not np.isfinite(ridge):
        raise ValueError("ridge must be finite")
    n = B.shape[0]
    A = B.astype(np.float64)
    A[:, 0] = A[:, 0] + ridge
    if diag is not None:
        diag = np.asarray(diag, dtype=np.float64)
        if diag.shape != (n,):
            raise ValueError("diag must be [n] with n = %d" % n)
        A[:, 0] = A[:, 0] + diag
    return A, n, B.shape[1] - 1


def banded_cholesky_host(B, ridge=0.0, diag=None):
    """The host twin of Context.banded_cholesky, in float64: the plain
    row-oriented Cholesky factorisation A = U^T U of the symmetric matrix A of
    the band B ([n, K + 1]) with the diagonal fl(fl(B[i, 0] + ridge) +
    diag[i]).  Returns (U_band, first_bad): U_band [n, K + 1] float64 in the
    same layout (U_band[i, k] = U[i, i + k], +0.0 where i + k >= n), first_bad
    None when every pivot was > 0, else the first row whose pivot was not (the
    rows before it are valid, the rest is zero).  Elements with i + k >= n are
    not read.  numpy."""
    A, n, K = _band_f64(B, ridge, diag)
    Kc = min(K, n - 1)
    U = np.zeros((n, K + 1), dtype=np.float64)
    for i in range(n):
        m = min(Kc, n - 1 - i)
        row = A[i, :m + 1].copy()
        for p in range(max(0, i - Kc), i):
            d = i - p
            ln = min(m + 1, Kc + 1 - d)
            row[:ln] -= U[p, d] * U[p, d:d + ln]
        if not row[0] > 0.0:  # (also NaN)
            return U, i
        U[i, 0] = np.sqrt(row[0])
        U[i, 1:m + 1] = row[1:] / U[i, 0]
    return U, None


def banded_solve_host(U_band, b, mode="full"):
    """The host twin of Context.banded_solve, in float64, by substitution:
    mode "forward" solves U^T y = b, "backward" U x = b, "full" A x = b (forward,
    then backward) for the factor U_band ([n, K + 1]) of banded_cholesky_host or
    Context.banded_cholesky and b ([n] or [n, n_cols]).  Returns a new float64
    array of b's shape.  numpy."""
    if mode not in SOLVE_MODES:
        raise ValueError('mode must be "full", "forward" or "backward"')
    U = np.asarray(U_band, dtype=np.float64)
    b = np.asarray(b)
    if U.ndim != 2 or U.shape[0] < 1 or U.shape[1] < 1:
        raise ValueError("U_band must be a [n, K + 1] band")
    n = U.shape[0]
    if b.ndim not in (1, 2) or b.shape[0] != n:
        raise ValueError("b must be [n] or [n, n_cols] with n = %d" % n)
    Kc = min(U.shape[1] - 1, n - 1)
    x = b.astype(np.float64).reshape(n, -1).copy()
    if mode != "backward":
        for i in range(n):
            m = min(Kc, n - 1 - i)
            x[i] = x[i] / U[i, 0]
            x[i + 1:i + m + 1] -= U[i, 1:m + 1, None] * x[i]
    if mode != "forward":
        for i in range(n - 1, -1, -1):
            m = min(Kc, n - 1 - i)
            x[i] = (x[i] - U[i, 1:m + 1] @ x[i + 1:i + m + 1]) / U[i, 0]
    return x.reshape(b.shape)


def banded_logdet(U_band):
    """log det A = 2 sum_i log U[i, 0] for the factor U_band ([n, K + 1], a numpy
    array or a torch tensor) of A = U^T U.  A float."""
    if hasattr(U_band, "data_ptr"):
        return 2.0 * float(U_band[:, 0].double().log().sum())
    U = np.asarray(U_band, dtype=np.float64)
    if U.ndim != 2 or U.shape[1] < 1:
        raise ValueError("U_band must be a [n, K + 1] band")
    return 2.0 * float(np.log(U[:, 0]).sum())


def _dev_tensor(t, what, names, device=None):
    """t checked as a device tensor of one of the dtype names; its dtype name."""
    if not all(hasattr(t, a) for a in ("data_ptr", "stride", "dtype", "shape", "device")):
        raise ValueError("%s must be a device tensor" % what)
    if getattr(t.device, "type", "") != "cuda":
        raise ValueError("%s must be on the context's GPU, not on %s" % (what, t.device))
    if device is not None and t.device.index is not None and t.device.index != device:
        raise ValueError("%s is on device %d; the context runs on %d" % (what, t.device.index, device))
    name = str(t.dtype).replace("torch.", "")
    if name not in names:
        raise ValueError("%s has dtype %s; it must be one of %s" % (what, name, ", ".join(names)))
    return name


def _row_stride(t, width, what):
    """The row stride in elements of a [n] or [n, width] tensor with contiguous rows."""
    shape, strides = tuple(int(x) for x in t.shape), tuple(int(x) for x in t.stride())
    if len(shape) == 2 and shape[1] > 1 and strides[1] != 1:
        raise ValueError("%s must have contiguous rows (last stride 1)" % what)
    ld = strides[0] if shape[0] > 1 else max(width, 1)
    if ld < width:
        raise ValueError("%s's row stride %d is below its width %d" % (what, ld, width))
    return ld


def _band_out_args(band, out, bandwidth, device):
    """What the calls that read a band and write a float64 array of its shape
    share: band a float32 or float16 [n, >= K + 1] device tensor with contiguous
    rows, bandwidth inside its columns, out (or None) a float64 [n, K + 1] device
    tensor with contiguous rows.  Returns (n, K, dtype id, ld, out's row stride
    or None); ValueError otherwise."""
    name = _dev_tensor(band, "band", ("float32", "float16"), device)
    shape = tuple(int(x) for x in band.shape)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError("band must be a [n, bandwidth + 1] tensor")
    n = shape[0]
    try:
        K = shape[1] - 1 if bandwidth is None else int(bandwidth)
    except (TypeError, ValueError):
        raise ValueError("bandwidth must be None or an integer")
    if K < 0 or K > shape[1] - 1:
        raise ValueError("bandwidth %d does not fit the band's %d columns" % (K, shape[1]))
    ld = _row_stride(band, shape[1], "band")
    ldo = None
    if out is not None:
        _dev_tensor(out, "out", ("float64",), device)
        if tuple(int(x) for x in out.shape) != (n, K + 1):
            raise ValueError("out has shape %s; the call writes %s" % (tuple(out.shape), (n, K + 1)))
        ldo = _row_stride(out, K + 1, "out")
    return n, K, _MATRIX_DTYPES[name], ld, ldo


def banded_chol_args(band, ridge=0.0, diag=None, out=None, bandwidth=None, device=None):
    """Context.banded_cholesky's arguments checked before any device call:
    returns (n, K, dtype id, ld, ldf) with ldf None without out.  ValueError on
    anything the call would refuse: band not a float32 or float16 [n, >= K + 1]
    device tensor with contiguous rows, a bandwidth outside the band's columns,
    a non-finite ridge, diag not a contiguous float64 [n] device tensor, out not
    a float64 [n, K + 1] device tensor with contiguous rows."""
    n, K, dt, ld, ldf = _band_out_args(band, out, bandwidth, device)
    try:
        ridge = float(ridge)
    except (TypeError, ValueError):
        raise ValueError("ridge must be a number")
    if not np.isfinite(ridge):
        raise ValueError("ridge must be finite")
    if diag is not None:
        _dev_tensor(diag, "diag", ("float64",), device)
        if tuple(int(x) for x in diag.shape) != (n,):
            raise ValueError("diag must be [n] with n = %d, not %s" % (n, tuple(diag.shape)))
        if n > 1 and int(diag.stride()[0]) != 1:
            raise ValueError("diag must be contiguous")
    return n, K, dt, ld, ldf


def banded_solve_args(factor, b, mode="full", out=None, device=None):
    """Context.banded_solve's arguments checked before any device call: returns
    (n, K, ldf, mode id, n_cols).  ValueError on anything the call would refuse:
    an unknown mode, factor not a float64 [n, K + 1] device tensor with
    contiguous rows, b not a float32 or float64 [n] or [n, n_cols] device
    tensor, out not a float64 device tensor of b's shape with contiguous rows."""
    if mode not in SOLVE_MODES:
        raise ValueError('mode must be "full", "forward" or "backward"')
    _dev_tensor(factor, "factor", ("float64",), device)
    shape = tuple(int(x) for x in factor.shape)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError("factor must be a [n, bandwidth + 1] tensor")
    n, K = shape[0], shape[1] - 1
    ldf = _row_stride(factor, K + 1, "factor")
    _dev_tensor(b, "b", ("float32", "float64"), device)
    bshape = tuple(int(x) for x in b.shape)
    if len(bshape) not in (1, 2) or bshape[0] != n or (len(bshape) == 2 and bshape[1] < 1):
        raise ValueError("b must be [n] or [n, n_cols] with n = %d, not %s" % (n, bshape))
    n_cols = 1 if len(bshape) == 1 else bshape[1]
    if out is not None:
        _dev_tensor(out, "out", ("float64",), device)
        if tuple(int(x) for x in out.shape) != bshape:
            raise ValueError("out has shape %s; b has %s" % (tuple(out.shape), bshape))
        _row_stride(out, n_cols, "out")
    return n, K, ldf, SOLVE_MODES[mode], n_cols


LdPairsumInfo = namedtuple("LdPairsumInfo", ["bandwidth", "nonfinite", "kernel_ms"])
LdPairsumInfo.__doc__ = """wld_banded_pairsum_info (Context.banded_pairsum): bandwidth; nonfinite, the band elements
(k >= 1, i + k < n) that were NaN or +-inf and counted as 0; kernel_ms."""

OMEGA_NONE = 0xFFFFFFFF


class LdOmega:
    """A sweep scan (Context.banded_omega, Context.run_omega, ld_omega,
    banded_omega_host) as numpy arrays, one entry per split: split, lo, hi
    (uint32 site indices of the scanned table), omega (float64, NaN where no
    candidate had t2 > 0), left and right (uint32, the best borders a and b,
    OMEGA_NONE where omega is NaN), zns (float64, Kelly's ZnS of the sites
    lo..hi), and the ints min_side, evaluated and skipped (candidate border
    pairs with t2 > 0 / without), eps and kernel_ms (None from the host twin).
    run_omega and ld_omega add position (uint64, the splits' coordinates),
    n_sites, bandwidth and the infos band (LdBandedInfo) and sums
    (LdPairsumInfo)."""

    FIELDS = ("split", "lo", "hi", "omega", "left", "right", "zns")

    def __init__(self, **kw):
        self.position = None
        self.__dict__.update(kw)

    @property
    def n_splits(self):
        return int(self.split.shape[0])

    def parents(self, site_map=None):
        """(left, right) in parent coordinates as uint64: site_map[a] and
        site_map[b] of the best borders (None: the indices themselves), 2^64 -
        1 where the split has none."""
        none = self.left == OMEGA_NONE
        a, b = np.where(none, 0, self.left).astype(np.int64), np.where(none, 0, self.right).astype(np.int64)
        if site_map is None:
            pa, pb = a.astype(np.uint64), b.astype(np.uint64)
        else:
            sm = np.asarray(site_map, dtype=np.uint64).reshape(-1)
            if a.size and max(int(a.max()), int(b.max())) >= sm.size:
                raise ValueError("site_map has %d entries; the borders reach site %d" % (sm.size, int(b.max())))
            pa, pb = sm[a], sm[b]
        full = np.uint64(0xFFFFFFFFFFFFFFFF)
        return np.where(none, full, pa), np.where(none, full, pb)

    def rows(self, site_map=None):
        """The scan as a list of (position, left parent, right parent, omega,
        zns) tuples, the CLI's columns; position is the split's own coordinate
        (site_map[split]) where the scan has none."""
        pa, pb = self.parents(site_map)
        if self.position is not None:
            pos = self.position
        elif site_map is None:
            pos = self.split.astype(np.uint64)
        else:
            pos = np.asarray(site_map, dtype=np.uint64).reshape(-1)[self.split.astype(np.int64)]
        return [(int(p), int(x), int(y), float(w), float(z)) for p, x, y, w, z in zip(pos, pa, pb, self.omega, self.zns)]


def banded_pairsum_host(B):
    """The host twin, and the definition, of Context.banded_pairsum: the
    pair-sum table M ([n, K + 1] float64) of the band B ([n, K + 1], any float
    dtype).  With b = float64(B) where that is finite, else +0.0, b[:, 0] and
    the elements with j + k >= n taken as +0.0:
    P = cumsum(b) along k (P[j, k] = P[j, k - 1] + b[j, k]), then M[j, 0] = 0 and
    M[j, k] = M[j + 1, k - 1] + P[j, k] for j + k < n, +0.0 elsewhere — so M[j, k]
    is the sum of the entries (u, v) with j <= u < v <= j + k.  The device gives
    the same bytes.  numpy."""
    B = np.asarray(B)
    if B.ndim != 2 or B.shape[0] < 1 or B.shape[1] < 1:
        raise ValueError("B must be a [n, K + 1] band")
    n, width = B.shape
    b = B.astype(np.float64)
    j, k = np.arange(n)[:, None], np.arange(width)[None, :]
    b[~np.isfinite(b) | (k == 0) | (j + k >= n)] = 0.0
    P = np.cumsum(b, axis=1)
    M = np.zeros((n, width), dtype=np.float64)
    for kk in range(1, min(width, n)):
        M[:n - kk, kk] = M[1:n - kk + 1, kk - 1] + P[:n - kk, kk]
    return M


def banded_nonfinite_host(B):
    """The count Context.banded_pairsum reports as nonfinite: the elements of
    the band B with k >= 1 and j + k < n that are NaN or +-inf.  numpy."""
    B = np.asarray(B)
    n, width = B.shape
    j, k = np.arange(n)[:, None], np.arange(width)[None, :]
    return int(np.count_nonzero(~np.isfinite(B.astype(np.float64)) & (k >= 1) & (j + k < n)))


def omega_args(n, K, split, lo, hi, min_side=2, eps=1e-5):
    """The scan's arguments checked before any device call: returns (split, lo,
    hi) as uint32 arrays and min_side, eps.  ValueError on anything
    wld_banded_omega_device would refuse: arrays of different lengths or none,
    a split without lo <= split < hi < n or with hi - lo > K, min_side < 2, eps
    negative or not finite."""
    try:
        arrs = [np.asarray(x).reshape(-1) for x in (split, lo, hi)]
    except Exception:
        raise ValueError("split, lo and hi must be integer arrays")
    for x in arrs:
        if x.dtype.kind not in "iu" and x.size:
            raise ValueError("split, lo and hi must be integer arrays")
    c, l, h = [x.astype(np.int64) for x in arrs]
    if not (c.size == l.size == h.size) or c.size < 1:
        raise ValueError("split, lo and hi must have the same length, at least 1")
    bad = np.flatnonzero(~((l >= 0) & (l <= c) & (c < h) & (h < n) & (h - l <= K)))
    if bad.size:
        g = int(bad[0])
        raise ValueError("split %d (lo %d, split %d, hi %d) breaks lo <= split < hi < %d sites or hi - lo <= bandwidth %d"
                         % (g, l[g], c[g], h[g], n, K))
    try:
        min_side, eps = int(min_side), float(eps)
    except (TypeError, ValueError):
        raise ValueError("min_side must be an integer and eps a number")
    if min_side < 2 or min_side > 0xFFFFFFFF:
        raise ValueError("min_side must be at least 2")
    if not np.isfinite(eps) or eps < 0:
        raise ValueError("eps must be finite and >= 0")
    return c.astype(np.uint32), l.astype(np.uint32), h.astype(np.uint32), min_side, eps


def banded_omega_host(M, split, lo, hi, min_side=2, eps=1e-5):
    """The host twin, and the definition, of Context.banded_omega on a pair-sum
    table M ([n, K + 1] float64, banded_pairsum_host's).  Entry g is the split
    between the sites c = split[g] and c + 1; the left flank is a..c with lo[g]
    <= a, the right flank c+1..b with b <= hi[g], both at least min_side sites.
    Per candidate (a, b), l = c - a + 1, r = b - c:
        SL = M[a, c-a]   SR = M[c+1, b-c-1]   ST = M[a, b-a]   X = (ST - SL) - SR
        t1 = (SL + SR) / float(l(l-1)/2 + r(r-1)/2)     t2 = X / float(l r) + eps
        omega = t1 / t2, skipped (and counted) unless t2 > 0.
    The split's omega is the largest; among equal ones the smallest a, then the
    smallest b.  zns = M[lo, hi-lo] / float(w(w-1)/2), w = hi - lo + 1.  Returns an
    LdOmega.  numpy."""
    M = np.asarray(M, dtype=np.float64)
    if M.ndim != 2 or M.shape[0] < 1 or M.shape[1] < 1:
        raise ValueError("M must be a [n, K + 1] table")
    n, K = M.shape[0], M.shape[1] - 1
    cs, ls, hs, min_side, eps = omega_args(n, K, split, lo, hi, min_side, eps)
    G = cs.size
    omega = np.full(G, np.nan)
    left, right = np.full(G, OMEGA_NONE, dtype=np.uint32), np.full(G, OMEGA_NONE, dtype=np.uint32)
    zns = np.empty(G)
    evaluated = skipped = 0
    for g in range(G):
        c, l0, h0 = int(cs[g]), int(ls[g]), int(hs[g])
        w = h0 - l0 + 1
        zns[g] = M[l0, h0 - l0] / np.float64(w * (w - 1) // 2)
        a = np.arange(l0, c + 1 - min_side + 1, dtype=np.int64)
        b = np.arange(c + min_side, h0 + 1, dtype=np.int64)
        if a.size == 0 or b.size == 0:
            continue
        l, r = c - a + 1, b - c
        SL, SR = M[a, c - a][:, None], M[c + 1, b - c - 1][None, :]
        ST = M[a[:, None], b[None, :] - a[:, None]]
        X = (ST - SL) - SR
        den1 = ((l * (l - 1) // 2)[:, None] + (r * (r - 1) // 2)[None, :]).astype(np.float64)
        den2 = (l[:, None] * r[None, :]).astype(np.float64)
        t1 = (SL + SR) / den1
        t2 = X / den2 + np.float64(eps)
        ok = t2 > 0
        evaluated += int(np.count_nonzero(ok))
        skipped += int(ok.size - np.count_nonzero(ok))
        if not ok.any():
            continue
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            om = t1 / np.where(ok, t2, 1.0)
        best = om[ok].max()
        flat = int(np.flatnonzero((ok & (om == best)).reshape(-1))[0])  # row-major: smallest a, then smallest b
        omega[g] = best
        left[g], right[g] = a[flat // b.size], b[flat % b.size]
    return LdOmega(split=cs, lo=ls, hi=hs, omega=omega, left=left, right=right, zns=zns, min_side=min_side, eps=eps,
                   evaluated=evaluated, skipped=skipped, kernel_ms=None)


def omega_splits(site_map, n_sites=None, n_grid=0, max_side=None, max_distance=None):
    """wld_omega_splits (host only): the splits of a sweep scan from
    coordinates.  site_map: the sites' non-decreasing coordinates (None: the
    indices 0..n_sites-1).  n_grid 0: every split c = 0..n-2 at position
    site_map[c]; n_grid >= 1: the equidistant positions x_g = site_map[0] +
    floor(span g / (n_grid - 1)) (n_grid 1: the midpoint), c the last site with
    coordinate <= x_g, clamped to [0, n - 2].  lo = max(c - max_side + 1, first
    site with coordinate >= x_g - max_distance), at most c; hi = min(c +
    max_side, last site with coordinate <= x_g + max_distance, n - 1), at least
    c + 1; max_distance None or 0: no distance limit.  Returns (position
    uint64, split, lo, hi uint32).  ValueError where the library refuses."""
    if site_map is None:
        if n_sites is None:
            raise ValueError("give site_map or n_sites")
        sm, n = None, int(n_sites)
    else:
        sm = np.ascontiguousarray(np.asarray(site_map).reshape(-1), dtype=np.uint64)
        n = int(sm.size)
        if n_sites is not None and int(n_sites) != n:
            raise ValueError("site_map has %d entries for %d sites" % (n, int(n_sites)))
    if max_side is None:
        raise ValueError("max_side is required")
    n_grid, max_side, D = int(n_grid), int(max_side), int(max_distance or 0)
    if n < 2 or n > 0xFFFFFFFF:
        raise ValueError("a split needs two sites, not %d" % n)
    if n_grid < 0 or n_grid > 0xFFFFFFFF or max_side < 1 or max_side > 0xFFFFFFFF or D < 0 or D >= 1 << 64:
        raise ValueError("n_grid, max_side (at least 1) and max_distance must be non-negative integers")
    G = int(lib().wld_omega_n_splits(n, n_grid))
    position = np.empty(G, dtype=np.uint64)
    split, lo, hi = (np.empty(G, dtype=np.uint32) for _ in range(3))
    st = lib().wld_omega_splits(None if sm is None else ctypes.c_void_p(sm.ctypes.data), n, n_grid, max_side, D,
                                ctypes.c_void_p(position.ctypes.data), ctypes.c_void_p(split.ctypes.data),
                                ctypes.c_void_p(lo.ctypes.data), ctypes.c_void_p(hi.ctypes.data))
    if st == -1:
        raise ValueError(lib().wld_last_error().decode())
    check(st, "wld_omega_splits")
    return position, split, lo, hi


def banded_pairsum_args(band, out=None, bandwidth=None, device=None):
    """Context.banded_pairsum's arguments checked before any device call:
    returns (n, K, dtype id, ld, lds) with lds None without out.  ValueError on
    anything the call would refuse: band not a float32 or float16 [n, >= K + 1]
    device tensor with contiguous rows, a bandwidth outside the band's columns,
    out not a float64 [n, K + 1] device tensor with contiguous rows."""
    return _band_out_args(band, out, bandwidth, device)


def annot_matrix(annot, n_sites=None):
    """The annotation matrix of Context.run_annot_scores as a C-contiguous
    float32 [n_sites, n_annot] array, checked before any device call: two
    dimensions, 1 to ANNOT_MAX columns, n_sites rows where given, every value
    finite.  float32 input is taken as it is; bool, integer and float64 input
    only where every value is a float32 (no silent rounding: TypeError
    otherwise, as for every other dtype).  Shape and value errors raise
    ValueError."""
    a = np.asarray(annot)
    if a.ndim != 2:
        raise ValueError("annot must be a [n_sites, n_annot] matrix, not %d-dimensional" % a.ndim)
    if a.shape[1] < 1 or a.shape[1] > ANNOT_MAX:
        raise ValueError("annot has %d columns; 1 to %d are supported" % (a.shape[1], ANNOT_MAX))
    if n_sites is not None and a.shape[0] != int(n_sites):
        raise ValueError("annot has %d rows for %d sites" % (a.shape[0], int(n_sites)))
    if a.dtype != np.float32:
        if a.dtype.kind not in "biuf":
            raise TypeError("annot must be float32 (or exactly convertible numbers), not %s" % a.dtype)
        with np.errstate(over="ignore", invalid="ignore"):
            f = a.astype(np.float32)
        same = (f.astype(a.dtype) == a) | ((a != a) & (f != f)) if a.dtype.kind == "f" else f.astype(np.float64) == a
        if not bool(np.all(same)):
            raise TypeError("annot of dtype %s does not convert to float32 exactly; pass float32" % a.dtype)
        a = f
    bad = np.argwhere(~np.isfinite(a))
    if bad.size:
        raise ValueError("annot[%d, %d] = %r is not finite" % (bad[0][0], bad[0][1], float(a[bad[0][0], bad[0][1]])))
    return np.ascontiguousarray(a)


class LdPartners:
    """wld_partners as numpy arrays and ints (Context.run_partners,
    ld_partners): count (uint32, [L]) and the [L, k] lists partner (uint32
    LOADED indices, PARTNERS_NONE past count), d, d_prime and r2 (float32, NaN
    past count) — row s holds site s's best partners, r2 descending then
    partner ascending — the counters pairs, none_pairs and passing_pairs,
    tiles, kernel_ms and merge_ms."""

    FIELDS = ("count", "partner", "d", "d_prime", "r2")

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_sites(self):
        return int(self.count.shape[0])

    @property
    def k(self):
        return int(self.partner.shape[1])

    def parents(self, site_map=None):
        """(site, partner) in parent coordinates: site [L] and partner [L, k]
        as uint64, site_map[i] for loaded index i (None: the indices
        themselves); partner is 2^64 - 1 past count."""
        L = self.n_sites
        sm = np.arange(L, dtype=np.uint64) if site_map is None else np.asarray(site_map, dtype=np.uint64).reshape(-1)
        if sm.size != L:
            raise ValueError("site_map has %d entries for %d sites" % (sm.size, L))
        filled = self.partner != PARTNERS_NONE
        part = np.full(self.partner.shape, np.iinfo(np.uint64).max, dtype=np.uint64)
        part[filled] = sm[self.partner[filled].astype(np.int64)]
        return sm.copy(), part

    def rows(self, site_map=None):
        """The flattened table (site, partner, rank, d, d_prime, r2) of the
        filled entries, by site then rank (rank 0 = the best partner); site
        and partner in parent coordinates when site_map is given."""
        site, part = self.parents(site_map)
        s, rank = np.nonzero(self.partner != PARTNERS_NONE)  # (row-major: by site, then rank)
        return (site[s], part[s, rank], rank.astype(np.uint32), self.d[s, rank], self.d_prime[s, rank],
                self.r2[s, rank])

    def _to_c(self):
        c = PartnersC()
        keep = [np.ascontiguousarray(self.count, dtype=np.uint32),
                np.ascontiguousarray(self.partner, dtype=np.uint32),
                np.ascontiguousarray(self.d, dtype=np.float32), np.ascontiguousarray(self.d_prime, dtype=np.float32),
                np.ascontiguousarray(self.r2, dtype=np.float32)]
        keep = [a.copy() for a in keep]
        c.n_sites, c.k = self.n_sites, self.k
        c.count, c.partner = _p(keep[0], ctypes.c_uint32), _p(keep[1], ctypes.c_uint32)
        c.d, c.d_prime, c.r2 = (_p(a, ctypes.c_float) for a in keep[2:])
        c.pairs, c.none_pairs, c.passing_pairs = self.pairs, self.none_pairs, self.passing_pairs
        c.tiles, c.kernel_ms, c.merge_ms = self.tiles, self.kernel_ms, self.merge_ms
        return c, keep

    def merge(self, other):
        """wld_partners_merge: the result over the union of this result's and
        other's (disjoint) chunk ranges, as a new LdPartners."""
        a, keep = self._to_c()
        b, keep_b = other._to_c()
        check(lib().wld_partners_merge(ctypes.byref(a), ctypes.byref(b)), "wld_partners_merge")
        L, k = self.n_sites, self.k
        return LdPartners(count=keep[0], partner=keep[1].reshape(L, k), d=keep[2].reshape(L, k),
                          d_prime=keep[3].reshape(L, k), r2=keep[4].reshape(L, k), pairs=int(a.pairs),
                          none_pairs=int(a.none_pairs), passing_pairs=int(a.passing_pairs), tiles=int(a.tiles),
                          kernel_ms=float(a.kernel_ms), merge_ms=float(a.merge_ms))


BLOCK_STATS = {"r2": BLOCKS_R2, "dprime": BLOCKS_ABS_DPRIME}
BLOCK_RULES = {"all": BLOCKS_ALL, "spine": BLOCKS_SPINE}


def _block_code(table, what, value):
    if isinstance(value, str):
        if value not in table:
            raise ValueError("%s must be one of %s" % (what, ", ".join("\"%s\"" % k for k in table)))
        return table[value]
    return int(value)


def _block_name(table, code):
    return next((k for k, v in table.items() if v == int(code)), int(code))


class LdBlockBreaks:
    """wld_block_breaks as numpy arrays and ints (Context.run_block_breaks):
    fwd_weak, bwd_weak (uint32, BLOCKS_NONE where a site has no weak pair) and
    last (uint32) per LOADED site, stat ("r2" or "dprime"), strong_min, the
    class totals pairs = none_pairs + nonfinite_pairs + strong_pairs +
    weak_pairs, tiles and kernel_ms."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_sites(self):
        return int(self.fwd_weak.shape[0])

    def _to_c(self):
        c = BlockBreaksC()
        keep = [np.ascontiguousarray(a, dtype=np.uint32).copy() for a in (self.fwd_weak, self.bwd_weak, self.last)]
        c.n_sites, c.stat, c.strong_min = self.n_sites, _block_code(BLOCK_STATS, "stat", self.stat), self.strong_min
        c.fwd_weak, c.bwd_weak, c.last = (_p(a, ctypes.c_uint32) for a in keep)
        c.pairs, c.none_pairs, c.nonfinite_pairs = self.pairs, self.none_pairs, self.nonfinite_pairs
        c.strong_pairs, c.weak_pairs, c.tiles, c.kernel_ms = self.strong_pairs, self.weak_pairs, self.tiles, self.kernel_ms
        return c, keep

    @staticmethod
    def _from_c(c, arrays):
        return LdBlockBreaks(fwd_weak=arrays[0], bwd_weak=arrays[1], last=arrays[2],
                             stat=_block_name(BLOCK_STATS, c.stat), strong_min=float(c.strong_min),
                             pairs=int(c.pairs), none_pairs=int(c.none_pairs),
                             nonfinite_pairs=int(c.nonfinite_pairs), strong_pairs=int(c.strong_pairs),
                             weak_pairs=int(c.weak_pairs), tiles=int(c.tiles), kernel_ms=float(c.kernel_ms))

    def merge(self, other):
        """wld_block_breaks_merge: the breaks over the union of this result's
        and other's (disjoint) chunk ranges, as a new LdBlockBreaks."""
        a, keep = self._to_c()
        b, keep_b = other._to_c()
        check(lib().wld_block_breaks_merge(ctypes.byref(a), ctypes.byref(b)), "wld_block_breaks_merge")
        return LdBlockBreaks._from_c(a, keep)

    def partition(self, rule="all", min_sites=2):
        """wld_blocks_partition: the blocks of these breaks, on the host (no
        device); an LdBlocks without statistics."""
        a, keep = self._to_c()
        out = BlocksC()
        check(lib().wld_blocks_partition(ctypes.byref(a), _block_code(BLOCK_RULES, "rule", rule), int(min_sites),
                                         ctypes.byref(out)), "wld_blocks_partition")
        return _take_blocks(out)


class LdBlocks:
    """wld_blocks as numpy arrays and ints (Context.run_blocks,
    Context.blocks_from_breaks, LdBlockBreaks.partition, ld_blocks): first and
    last (uint32 LOADED indices, inclusive) per block in site order,
    site_block (int32 per site: its block or -1), stat, rule, strong_min,
    min_sites; the per-block statistics pairs, informative, strong (uint64),
    value_sum (float64) and value_min (float32, NaN without an informative
    pair) — None after a host-only partition — with pass 2's tiles and
    kernel_ms and, from run_blocks, pass 1's break_* totals."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_sites(self):
        return int(self.site_block.shape[0])

    @property
    def n_blocks(self):
        return int(self.first.shape[0])

    @property
    def sites(self):
        """Sites per block."""
        return (self.last.astype(np.int64) - self.first.astype(np.int64) + 1).astype(np.uint32)

    @property
    def mean(self):
        """Per-block mean of the value over the informative pairs (NaN where
        there is none); None without statistics."""
        if self.value_sum is None:
            return None
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.informative > 0, self.value_sum / self.informative, np.nan)

    def parents(self, site_map=None):
        """(first, last) in parent coordinates as uint64: site_map[i] for
        loaded index i (None: this result's site_map if it has one, else the
        indices themselves)."""
        if site_map is None:
            site_map = getattr(self, "site_map", None)
        L = self.n_sites
        sm = np.arange(L, dtype=np.uint64) if site_map is None else np.asarray(site_map, dtype=np.uint64).reshape(-1)
        if sm.size != L:
            raise ValueError("site_map has %d entries for %d sites" % (sm.size, L))
        return sm[self.first.astype(np.int64)], sm[self.last.astype(np.int64)]

    def site_cell(self):
        """The blocks as a heat map's cells: the int32 site -> cell map
        Context.run_heatmap accepts (with n_cells = n_blocks), for up to
        HEAT_MAX_CELLS blocks."""
        if self.n_blocks > HEAT_MAX_CELLS:
            raise ValueError("%d blocks; a heat map has at most %d cells per side" % (self.n_blocks, HEAT_MAX_CELLS))
        return np.ascontiguousarray(self.site_block, dtype=np.int32).copy()


def _take_blocks(out):
    """Library-allocated wld_blocks -> LdBlocks (copies, then frees)."""
    L, nb = int(out.n_sites), int(out.n_blocks)

    def grab(p, n, dt):
        return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)

    have = bool(out.pairs)
    res = LdBlocks(first=grab(out.first, nb, np.uint32), last=grab(out.last, nb, np.uint32),
                   site_block=grab(out.site_block, L, np.int32), stat=_block_name(BLOCK_STATS, out.stat),
                   rule=_block_name(BLOCK_RULES, out.rule), strong_min=float(out.strong_min),
                   min_sites=int(out.min_sites),
                   pairs=grab(out.pairs, nb, np.uint64) if have else None,
                   informative=grab(out.informative, nb, np.uint64) if have else None,
                   strong=grab(out.strong, nb, np.uint64) if have else None,
                   value_sum=grab(out.value_sum, nb, np.float64) if have else None,
                   value_min=grab(out.value_min, nb, np.float32) if have else None,
                   tiles=int(out.tiles), kernel_ms=float(out.kernel_ms), break_pairs=int(out.break_pairs),
                   break_none_pairs=int(out.break_none_pairs), break_nonfinite_pairs=int(out.break_nonfinite_pairs),
                   break_strong_pairs=int(out.break_strong_pairs), break_weak_pairs=int(out.break_weak_pairs),
                   break_tiles=int(out.break_tiles), break_kernel_ms=float(out.break_kernel_ms))
    lib().wld_blocks_free(ctypes.byref(out))
    return res


def heatmap_cells(site_map_or_siteset, n_sites=None, *, sites_per_cell=None, cell_width=None, edges=None,
                  region=None):
    """The site -> cell map of a heat map (Context.run_heatmap): returns
    (site_cell, n_cells, cell_start) — site_cell int32 per site (-1: on no
    cell), cell_start uint64 per cell, the parent coordinate the cell begins at.

    The first argument is a SiteSet, a site_map (parent coordinate per site)
    or None with n_sites (coordinate = site index).  Exactly one layout:
      sites_per_cell=S  equal runs of S sites (the last may be shorter);
                        cell_start is the coordinate of the run's first site;
      cell_width=W      equal bins of the coordinate: cell (pos - origin) // W,
                        origin = the region's start, or without a region the
                        multiple of W at or below the first site;
      edges=[e0..ek]    k cells [e_c, e_c+1) (gene boundaries; strictly
                        ascending); sites outside [e0, ek) are on no cell.
    region=(start, stop), parent coordinates, start <= pos < stop: every site
    outside is on no cell.  Pure numpy.  ValueError: more than 4,096 cells, no
    site on any cell, or (coordinate layouts) a site_map that descends."""
    if isinstance(site_map_or_siteset, SiteSet):
        n_sites = site_map_or_siteset.n_sites()
        site_map_or_siteset = site_map_or_siteset.site_map
    if site_map_or_siteset is None:
        if n_sites is None:
            raise ValueError("give a SiteSet, a site_map or n_sites")
        pos = np.arange(int(n_sites), dtype=np.int64)
    else:
        pos = np.asarray(site_map_or_siteset).astype(np.int64).reshape(-1)
        if n_sites is not None and int(n_sites) != pos.size:
            raise ValueError("site_map has %d entries for %d sites" % (pos.size, int(n_sites)))
    if sum(x is not None for x in (sites_per_cell, cell_width, edges)) != 1:
        raise ValueError("give exactly one of sites_per_cell, cell_width and edges")
    inside = np.ones(pos.size, dtype=bool)
    if region is not None:
        start, stop = int(region[0]), int(region[1])
        if start < 0 or stop < start:
            raise ValueError("region must be (start, stop) with 0 <= start <= stop")
        inside = (pos >= start) & (pos < stop)
    cell = np.full(pos.size, -1, dtype=np.int64)
    if sites_per_cell is not None:
        S = int(sites_per_cell)
        if S < 1:
            raise ValueError("sites_per_cell must be at least 1")
        idx = np.flatnonzero(inside)
        cell[idx] = np.arange(idx.size) // S
        n_cells = (idx.size + S - 1) // S
        cell_start = pos[idx[::S]].astype(np.uint64)
    elif cell_width is not None:
        W = int(cell_width)
        if W < 1:
            raise ValueError("cell_width must be at least 1")
        if not inside.any():
            n_cells, cell_start = 0, np.zeros(0, dtype=np.uint64)
        else:
            origin = int(region[0]) if region is not None else int(pos[inside].min()) // W * W
            cell[inside] = (pos[inside] - origin) // W
            n_cells = int(cell.max()) + 1
            cell_start = (origin + W * np.arange(min(n_cells, HEAT_MAX_CELLS + 1), dtype=np.int64)).astype(np.uint64)
    else:
        e = np.asarray(edges).astype(np.int64).reshape(-1)
        if e.size < 2 or np.any(np.diff(e) <= 0) or e[0] < 0:
            raise ValueError("edges must be at least two strictly ascending coordinates")
        inside &= (pos >= e[0]) & (pos < e[-1])
        cell[inside] = np.searchsorted(e, pos[inside], side="right") - 1
        n_cells = e.size - 1
        cell_start = e[:-1].astype(np.uint64)
    if n_cells > HEAT_MAX_CELLS:
        raise ValueError("%d cells; a heat map has at most %d per side" % (n_cells, HEAT_MAX_CELLS))
    if n_cells == 0 or not (cell >= 0).any():
        raise ValueError("no site is on a cell")
    on = cell[cell >= 0]
    if np.any(np.diff(on) < 0):
        raise ValueError("the cells descend along the sites: a coordinate layout needs a non-decreasing site_map")
    return cell.astype(np.int32), int(n_cells), cell_start


class LdPrune:
    """wld_prune as numpy arrays and ints (Context.run_prune, ld_prune): keep
    (bool per LOADED site), tag (uint32, loaded indices: a kept site's own
    index, else its kept neighbour of the smallest rank), n_kept, edges (the
    rows at the threshold and window), rounds, pair_ms and prune_ms.  From
    ld_prune also kept_sites: the parent indices of the kept sites."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class TargetRows:
    """wld_target_rows as numpy arrays and numbers (Context.run_targets,
    ld_targets): offset (uint64, one more than the targets: target k's rows are
    [offset[k], offset[k + 1])), target (the list position k), site_target and
    site_partner (PARENT indices), d, d_prime, r2 (float32), in list order then
    by partner; items, batches and kernel_ms.  From ld_targets also targets:
    the loaded indices the rows' `target` column indexes."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __len__(self):
        return int(self.r2.size)


def maf_priority(site_set):
    """The "maf" priority of ld_prune: per site minor / (major + minor) of
    the counts of its major and minor symbols (wld_major_minor on the site's
    histogram), in double, cast to float32; 0 for a site without both."""
    buf = site_set.buffer
    L = buf.shape[0]
    hist = np.stack([(buf == s).sum(axis=1) for s in range(6)], axis=1).astype(np.uint64) if L else \
        np.zeros((0, 6), dtype=np.uint64)
    out = np.zeros(L, dtype=np.float32)
    a, b = ctypes.c_int(), ctypes.c_int()
    for i in range(L):
        h = np.ascontiguousarray(hist[i])
        check(lib().wld_major_minor(_p(h, ctypes.c_uint64), ctypes.byref(a), ctypes.byref(b)), "major_minor")
        if a.value >= 0 and b.value >= 0:
            major, minor = float(h[a.value]), float(h[b.value])
            out[i] = np.float32(minor / (major + minor))
    return out


# Live contexts, closed (newest first) by an exit handler while the HIP
# runtime and torch are still up: a context left to its finalizer at
# interpreter shutdown would destroy its stream and buffers in arbitrary order
# against torch objects that may still reference them (events, pinned-memory
# copies recorded on a stream the context ran on).
_LIVE = weakref.WeakValueDictionary()
_SEQ = [0]


@atexit.register
def _close_live_contexts():
    for k in sorted(list(_LIVE.keys()), reverse=True):
        c = _LIVE.get(k)
        if c is not None:
            try:
                c.close()
            except Exception:
                pass


class Context:
    """One device context (wld_ctx): HIP stream, device buffers, results."""

    def __init__(self, device=0, kernel=KERNEL_AUTO, devices=None, ref_sums=None):
        """devices (a list of HIP ordinals, repeats allowed): a multi-device
        context (wld_create_multi) that shards load/run_host/all-pairs calls.
        ref_sums (WLD_OPT_REF_SUMS): None keeps the library default (lib.rs's
        own f32 summation order, bit-identical rows); False: exact sums."""
        self._borrowers = weakref.WeakSet()  # contexts running on this one's stream (set_stream)
        self._stream_owner = None
        h = ctypes.c_void_p()
        self._lib = lib()  # kept: module globals may be gone when __del__ runs at exit
        if devices is not None:
            arr = (ctypes.c_int * len(devices))(*devices)
            check(self._lib.wld_create_multi(arr, len(devices), ctypes.byref(h)), "wld_create_multi")
            device = devices[0]
        else:
            check(self._lib.wld_create(device, ctypes.byref(h)), "wld_create")
        self._h = h
        self.device = device
        _SEQ[0] += 1
        _LIVE[_SEQ[0]] = self
        if kernel != KERNEL_AUTO:
            self.set_kernel(kernel)
        if ref_sums is not None:
            self.set_option("ref_sums", int(bool(ref_sums)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            # contexts running on this one's stream get their own back first
            # (wld_set_stream waits for their queued work)
            for b in list(getattr(self, "_borrowers", ())):
                if getattr(b, "_h", None) is not None and b._h.value:
                    b.set_stream(None)
            owner = getattr(self, "_stream_owner", None)
            if owner is not None:
                owner._borrowers.discard(self)
                self._stream_owner = None
            self._lib.wld_destroy(self._h)
            self._h = None

    __del__ = close

    def n_devices(self):
        return int(lib().wld_n_devices(self._h))

    def set_kernel(self, kernel):
        check(lib().wld_set_kernel(self._h, kernel), "wld_set_kernel")

    def set_option(self, name, value):
        """wld_set_option: name is a key of OPTIONS ("prefilter", "screen",
        "tile_order", "all_planes", "mfma_layout", "valu_plain", "staging_rows",
        "host_batch_pairs", "ref_sums", "fused_scan", "screen_fp6", "fp6_a4", "fp6_shared", ...); only "ref_sums" changes a result."""
        check(lib().wld_set_option(self._h, OPTIONS[name], int(value)), "wld_set_option")

    def get_option(self, name):
        v = ctypes.c_int64()
        check(lib().wld_get_option(self._h, OPTIONS[name], ctypes.byref(v)), "wld_get_option")
        return int(v.value)

    def fp6_weight_codes(self, n_seqs):
        """(e2m3 codes of the loaded set's n_seqs rounded weights, whether all
        are e2m1 values: the "fp6_a4" image's condition) (wld_fp6_weight_codes)."""
        codes, fits = np.zeros(n_seqs, dtype=np.uint8), ctypes.c_int()
        check(lib().wld_fp6_weight_codes(self._h, _p(codes, ctypes.c_uint8), ctypes.byref(fits)), "wld_fp6_weight_codes")
        return codes, bool(fits.value)

    def set_window(self, max_distance=None, max_sites=None):
        """wld_set_window: later runs compute only the pairs a < b with
        site_map[b] - site_map[a] <= max_distance (parent coordinates) and
        b - a <= max_sites (loaded sites); None or 0: no limit.  Persists
        across loads; dense() and single_weighted_ld_pair ignore it."""
        check(lib().wld_set_window(self._h, int(max_distance or 0), int(max_sites or 0)), "wld_set_window")

    def window(self):
        """(max_distance, max_sites) of wld_get_window; 0 = no limit."""
        d, k = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().wld_get_window(self._h, ctypes.byref(d), ctypes.byref(k)), "wld_get_window")
        return int(d.value), int(k.value)

    def window_pairs_in_chunks(self, begin, end):
        """In-window pairs of the loaded set's linear chunks [begin, end) (wld_window_pairs_in_chunks)."""
        n = ctypes.c_uint64()
        check(lib().wld_window_pairs_in_chunks(self._h, begin, end, ctypes.byref(n)), "wld_window_pairs_in_chunks")
        return int(n.value)

    def shard_chunks_window(self, n_shards, shard):
        """Linear chunk range [begin, end) of `shard`, balanced by in-window pairs (wld_shard_chunks_window)."""
        b, e = ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().wld_shard_chunks_window(self._h, n_shards, shard, ctypes.byref(b), ctypes.byref(e)),
              "wld_shard_chunks_window")
        return int(b.value), int(e.value)

    def window_limits(self, n_sites):
        """The device's per-site limits hi[] under the window (wld_window_limits_copy; tests)."""
        hi = np.zeros(n_sites, dtype=np.uint32)
        check(lib().wld_window_limits_copy(self._h, _p(hi, ctypes.c_uint32)), "wld_window_limits_copy")
        return hi

    def load(self, site_major, weights, site_map=None):
        buf = np.ascontiguousarray(site_major, dtype=np.uint8)
        w = np.ascontiguousarray(weights, dtype=np.float32)
        if buf.ndim != 2 or w.size != buf.shape[1]:
            raise ValueError("site_major must be [n_sites, n_seqs] and weights n_seqs long")
        sm = None if site_map is None else np.ascontiguousarray(site_map, dtype=np.uint64)
        check(lib().wld_load(self._h, _p(buf, ctypes.c_uint8), buf.shape[0], buf.shape[1],
                             None if sm is None else _p(sm, ctypes.c_uint64), _p(w, ctypes.c_float)), "wld_load")

    def load_device(self, d_sites_ptr, n_sites, n_seqs, d_weights_ptr, site_map=None):
        sm = None if site_map is None else np.ascontiguousarray(site_map, dtype=np.uint64)
        check(lib().wld_load_device(self._h, ctypes.c_void_p(d_sites_ptr), n_sites, n_seqs,
                                    None if sm is None else _p(sm, ctypes.c_uint64),
                                    ctypes.c_void_p(d_weights_ptr)), "wld_load_device")

    def load_filtered(self, buffer, min_acgt=0.8, min_minor=0.02, max_minor=0.5, unweighted=False, site_map=None):
        """Device pre-pass (main.rs:139-156 on the GPU): filter the UNFILTERED
        [n_sites, n_seqs] Symbol buffer with is_site_of_interest, compute
        Henikoff (or unit) weights on the kept sites and load them.  Returns the
        kept site count; weights() and site_map() give the pre-pass results."""
        buf = np.ascontiguousarray(buffer, dtype=np.uint8)
        L, N = buf.shape
        sm = None if site_map is None else np.ascontiguousarray(site_map, dtype=np.uint64)
        n = ctypes.c_size_t()
        check(lib().wld_load_filtered(self._h, _p(buf, ctypes.c_uint8), L, N,
                                      None if sm is None else _p(sm, ctypes.c_uint64), min_acgt, min_minor, max_minor,
                                      int(bool(unweighted)), ctypes.byref(n)), "wld_load_filtered")
        self._n_seqs, self._n_kept = N, int(n.value)
        return self._n_kept

    def load_filtered_device(self, d_sites_ptr, n_sites, n_seqs, min_acgt=0.8, min_minor=0.02, max_minor=0.5,
                             unweighted=False, site_map=None):
        sm = None if site_map is None else np.ascontiguousarray(site_map, dtype=np.uint64)
        n = ctypes.c_size_t()
        check(lib().wld_load_filtered_device(self._h, ctypes.c_void_p(d_sites_ptr), n_sites, n_seqs,
                                             None if sm is None else _p(sm, ctypes.c_uint64), min_acgt,
                                             min_minor, max_minor, int(bool(unweighted)), ctypes.byref(n)),
              "wld_load_filtered_device")
        self._n_seqs, self._n_kept = n_seqs, int(n.value)
        return self._n_kept

    def weights(self):
        w = np.zeros(self._n_seqs, dtype=np.float32)
        check(lib().wld_weights_copy(self._h, _p(w, ctypes.c_float)), "wld_weights_copy")
        return w

    def site_map(self):
        m = np.zeros(self._n_kept, dtype=np.uint64)
        check(lib().wld_site_map_copy(self._h, _p(m, ctypes.c_uint64)), "wld_site_map_copy")
        return m

    def run(self, r2_threshold, row_begin=0, row_end=0):
        n = ctypes.c_uint64()
        check(lib().wld_run(self._h, r2_threshold, row_begin, row_end, ctypes.byref(n)), "wld_run")
        return int(n.value)

    def run_chunks(self, r2_threshold, chunk_begin=0, chunk_end=0):
        """wld_run_chunks: pairs of the linear chunk range [chunk_begin, chunk_end) (end 0 = all)."""
        n = ctypes.c_uint64()
        check(lib().wld_run_chunks(self._h, r2_threshold, chunk_begin, chunk_end, ctypes.byref(n)), "wld_run_chunks")
        return int(n.value)

    def run_chunks_async(self, r2_threshold, chunk_begin=0, chunk_end=0, d_count_ptr=None):
        """wld_run_chunks_async: enqueue the run on the context's stream; the row
        total lands in the device uint64 at d_count_ptr (if given).  Complete
        it with run_wait() before any other call on this context."""
        check(lib().wld_run_chunks_async(self._h, r2_threshold, chunk_begin, chunk_end,
                                         ctypes.c_void_p(d_count_ptr) if d_count_ptr else None),
              "wld_run_chunks_async")

    def run_wait(self):
        """wld_run_wait: completes the run started by run_chunks_async; returns its row count."""
        n = ctypes.c_uint64()
        check(lib().wld_run_wait(self._h, ctypes.byref(n)), "wld_run_wait")
        return int(n.value)

    def run_after(self, prev):
        """wld_run_after: this context's next run waits on the device for the
        pair kernels of prev's run in flight (no host wait)."""
        check(lib().wld_run_after(self._h, prev._h), "wld_run_after")

    def run_host(self, r2_threshold, progress_report=None):
        """wld_run_host: every pair of the loaded set, in batches of <= 2^31
        pairs, rows to host in reference order (a PairStore)."""
        cb = PROGRESS_FN(lambda n, _u: progress_report(int(n))) if progress_report else PROGRESS_FN()
        out = Pairs()
        check(lib().wld_run_host(self._h, r2_threshold, cb, None, ctypes.byref(out)), "wld_run_host")
        return _take_pairs(out)

    def run_summary(self, bin_width=0, n_bins=0, chunk_begin=0, chunk_end=0):
        """wld_run_summary: every in-window pair of the linear chunk range
        (end 0 = all) reduced on the device to an LdSummary — no rows.  With
        bin_width > 0 also the r2 decay histogram over n_bins distance bins."""
        out = Summary()
        check(lib().wld_run_summary(self._h, chunk_begin, chunk_end, int(bin_width or 0), int(n_bins or 0),
                                    ctypes.byref(out)), "wld_run_summary")
        L, nb = int(out.n_sites), int(out.n_bins)

        def grab(p, n, dt):
            return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)

        res = LdSummary(pairs=int(out.pairs), none_pairs=int(out.none_pairs),
                        nonfinite_pairs=int(out.nonfinite_pairs), counted_pairs=int(out.counted_pairs),
                        r2_sum=float(out.r2_sum), score=grab(out.score, L, np.float64),
                        partners=grab(out.partners, L, np.uint32),
                        bin_width=int(out.bin_width), n_bins=nb,
                        bin_pairs=grab(out.bin_pairs, nb, np.uint64) if nb else None,
                        bin_r2_sum=grab(out.bin_r2_sum, nb, np.float64) if nb else None,
                        kernel_ms=float(out.kernel_ms))
        lib().wld_summary_free(ctypes.byref(out))
        return res

    def run_heatmap(self, site_cell, n_cells, stat="r2", chunk_begin=0, chunk_end=0):
        """wld_run_heatmap: every in-window pair of the linear chunk range
        (end 0 = all) whose two sites have a cell, reduced on the device over
        the n_cells x n_cells grid to an LdHeatmap — no rows.  site_cell: one
        int32 per LOADED site, -1 or a cell id, non-decreasing over the sites
        that have one (heatmap_cells builds the usual layouts).  stat: "r2"
        or "dprime" (|D'|)."""
        if isinstance(stat, str):
            if stat not in HEAT_STATS:
                raise ValueError("stat must be \"r2\" or \"dprime\"")
            stat = HEAT_STATS[stat]
        sc = None
        if site_cell is not None:
            sc = np.ascontiguousarray(site_cell, dtype=np.int32)
            if sc.ndim != 1:
                raise ValueError("site_cell must be one cell id per loaded site")
            n = int(lib().wld_loaded_sites(self._h))
            if n and sc.size != n:  # (not loaded: the library refuses the call)
                raise ValueError("site_cell has %d entries for %d loaded sites" % (sc.size, n))
        out = Heatmap()
        check(lib().wld_run_heatmap(self._h, None if sc is None else _p(sc, ctypes.c_int32), int(n_cells), int(stat),
                                    chunk_begin, chunk_end, ctypes.byref(out)), "wld_run_heatmap")
        nc = int(out.n_cells)

        def grab(p, dt):
            return np.ctypeslib.as_array(p, shape=(nc, nc)).astype(dt, copy=True)

        res = LdHeatmap(n_cells=nc, stat="dprime" if int(out.stat) == HEAT_ABS_DPRIME else "r2",
                        pairs=int(out.pairs), none_pairs=int(out.none_pairs),
                        nonfinite_pairs=int(out.nonfinite_pairs), counted_pairs=int(out.counted_pairs),
                        count=grab(out.count, np.uint64), sum=grab(out.sum, np.float64),
                        max=grab(out.max, np.float32), tiles=int(out.tiles), kernel_ms=float(out.kernel_ms))
        lib().wld_heatmap_free(ctypes.byref(out))
        return res

    def run_annot_scores(self, annot, self_term=False, chunk_begin=0, chunk_end=0):
        """wld_run_annot_scores: the partitioned LD scores of every LOADED
        site — score[i, c] = sum over site i's counted in-window pairs {i, k}
        of the linear chunk range (end 0 = all) of r2(i, k) annot[k, c] —
        reduced on the device to an LdAnnotScores; no rows.  annot: a float32
        [n_sites, n_annot] matrix (annot_matrix checks it before any device
        call).  self_term: every site with a major and a minor symbol also
        counts r2(i, i) = 1, as LDSC does."""
        n = int(lib().wld_loaded_sites(self._h))
        a = annot_matrix(annot, n if n else None)  # (not loaded: the library refuses the call)
        flags = ANNOT_SELF if self_term else 0
        out = AnnotScoresC()
        check(lib().wld_run_annot_scores(self._h, _p(a, ctypes.c_float), int(a.shape[1]), flags, chunk_begin,
                                         chunk_end, ctypes.byref(out)), "wld_run_annot_scores")
        L, C = int(out.n_sites), int(out.n_annot)
        res = LdAnnotScores(
            score=(np.ctypeslib.as_array(out.score, shape=(L, C)).astype(np.float64, copy=True) if L
                   else np.zeros((0, C), dtype=np.float64)),
            partners=(np.ctypeslib.as_array(out.partners, shape=(L,)).astype(np.uint32, copy=True) if L
                      else np.zeros(0, dtype=np.uint32)),
            pairs=int(out.pairs), none_pairs=int(out.none_pairs), nonfinite_pairs=int(out.nonfinite_pairs),
            counted_pairs=int(out.counted_pairs), self_term=bool(int(out.flags) & ANNOT_SELF), tiles=int(out.tiles),
            kernel_ms=float(out.kernel_ms))
        lib().wld_annot_scores_free(ctypes.byref(out))
        return res

    def run_matrix(self, rows=None, cols=None, stat="r", dtype="float32", zero_missing=False, out=None):
        """wld_run_matrix / wld_run_matrix_device: the dense LD matrix of the
        loaded-site rectangle rows x cols ((begin, end) pairs; None: every
        site) under the context's window: stat "r" (signed: the weighted
        correlation of the major-allele indicators), "r2", "d" or "dprime" (the
        reference's sign), float32 or float16, symmetric bit for bit, +0.0 out
        of the window, NaN for pairs without a value (zero_missing: 0.0, and
        1.0 on the r / r2 diagonal).  Without out: returns (numpy array,
        LdMatrixInfo).  out a numpy array (C-contiguous rows; a row stride is
        kept): filled through the host call.  out a device tensor (data_ptr,
        stride, dtype, shape, device — a torch tensor on the context's GPU,
        last stride 1): filled in place on the device; its pending work is
        synchronised first.  With out: returns (out, LdMatrixInfo).  Shape,
        dtype and range mismatches raise ValueError before any device call."""
        n = int(lib().wld_loaded_sites(self._h))
        if not n:
            check(lib().wld_run_matrix(self._h, 0, 0, 0, 0, 0, 0, 0, None, 0, ctypes.byref(MatrixInfoC())),
                  "wld_run_matrix")  # (not loaded: the library's own refusal)
        rows, cols, st, dt, kind, ld = matrix_args(n, rows, cols, stat, dtype, out)
        flags = MATRIX_ZERO_MISSING if zero_missing else 0
        info = MatrixInfoC()
        if kind is None:
            out = np.empty((rows[1] - rows[0], cols[1] - cols[0]), dtype=np.float16 if dt == MATRIX_F16 else np.float32)
            kind = "numpy"
        if kind == "numpy":
            check(lib().wld_run_matrix(self._h, rows[0], rows[1], cols[0], cols[1], st, dt, flags,
                                       ctypes.c_void_p(out.ctypes.data), ld, ctypes.byref(info)), "wld_run_matrix")
        else:
            import torch  # (only here: a device tensor was passed)
            if out.device.index is not None and out.device.index != self.device:
                raise ValueError("out is on device %d; the context runs on %d" % (out.device.index, self.device))
            torch.cuda.synchronize(out.device)
            check(lib().wld_run_matrix_device(self._h, rows[0], rows[1], cols[0], cols[1], st, dt, flags,
                                              ctypes.c_void_p(int(out.data_ptr())), ld, ctypes.byref(info)),
                  "wld_run_matrix_device")
        return out, LdMatrixInfo(rows=(int(info.row_begin), int(info.row_end)), cols=(int(info.col_begin), int(info.col_end)),
                                 stat=stat, dtype="float16" if dt == MATRIX_F16 else "float32",
                                 zero_missing=bool(zero_missing), pairs=int(info.pairs), none_pairs=int(info.none_pairs),
                                 nonfinite_pairs=int(info.nonfinite_pairs), counted_pairs=int(info.counted_pairs),
                                 tiles=int(info.tiles), kernel_ms=float(info.kernel_ms))

    def matrix_banded_width(self):
        """wld_matrix_banded_width: the bandwidth the context's window needs,
        max over a of hi[a] - a for the window's limits (no window: the loaded
        site count - 1).  run_matrix_banded refuses a smaller bandwidth."""
        k = ctypes.c_uint32(0)
        check(lib().wld_matrix_banded_width(self._h, ctypes.byref(k)), "wld_matrix_banded_width")
        return int(k.value)

    def run_matrix_banded(self, rows=None, bandwidth=None, stat="r", dtype="float32", zero_missing=False, out=None):
        """wld_run_matrix_banded / wld_run_matrix_banded_device: the LD matrix
        of run_matrix under the context's window in band storage: a
        [rows, bandwidth + 1] array whose element [u - rows[0], k] is entry
        (u, u + k) — the same bits as run_matrix's, +0.0 where u + k is past
        the last site.  rows: a (begin, end) pair of loaded sites (None: every
        site); bandwidth None: the width the window needs
        (matrix_banded_width), a smaller one is refused, a larger one pads
        with +0.0.  out as in run_matrix (a numpy array through the host call,
        a device tensor in place).  Returns (array, LdBandedInfo).  Argument
        errors raise ValueError before any device call."""
        n = int(lib().wld_loaded_sites(self._h))
        if not n:
            check(lib().wld_run_matrix_banded(self._h, 0, 0, 0, 0, 0, 0, None, 0, ctypes.byref(MatrixBandedInfoC())),
                  "wld_run_matrix_banded")  # (not loaded: the library's own refusal)
        rows, K, st, dt, kind, ld = banded_args(n, self.matrix_banded_width(), rows, bandwidth, stat, dtype, out)
        flags = MATRIX_ZERO_MISSING if zero_missing else 0
        info = MatrixBandedInfoC()
        if kind is None:
            out = np.empty((rows[1] - rows[0], K + 1), dtype=np.float16 if dt == MATRIX_F16 else np.float32)
            kind = "numpy"
        if kind == "numpy":
            check(lib().wld_run_matrix_banded(self._h, rows[0], rows[1], K, st, dt, flags,
                                              ctypes.c_void_p(out.ctypes.data), ld, ctypes.byref(info)),
                  "wld_run_matrix_banded")
        else:
            import torch  # (only here: a device tensor was passed)
            if out.device.index is not None and out.device.index != self.device:
                raise ValueError("out is on device %d; the context runs on %d" % (out.device.index, self.device))
            torch.cuda.synchronize(out.device)
            check(lib().wld_run_matrix_banded_device(self._h, rows[0], rows[1], K, st, dt, flags,
                                                     ctypes.c_void_p(int(out.data_ptr())), ld, ctypes.byref(info)),
                  "wld_run_matrix_banded_device")
        return out, LdBandedInfo(rows=(int(info.row_begin), int(info.row_end)), bandwidth=int(info.bandwidth), stat=stat,
                                 dtype="float16" if dt == MATRIX_F16 else "float32", zero_missing=bool(zero_missing),
                                 pairs=int(info.pairs), none_pairs=int(info.none_pairs),
                                 nonfinite_pairs=int(info.nonfinite_pairs), counted_pairs=int(info.counted_pairs),
                                 tiles=int(info.tiles), kernel_ms=float(info.kernel_ms))

    def banded_apply(self, band, X, out=None, bandwidth=None):
        """wld_banded_apply_device: Y = S X on the device for the symmetric
        matrix S whose upper band is `band` — a [n, W] float32 or float16
        device tensor in run_matrix_banded's layout with every row present
        (last stride 1; bandwidth None: W - 1, else the first bandwidth + 1
        columns) — and X a [n] or [n, n_cols] float32 or float64 device tensor
        (last stride 1).  Returns a float64 tensor of X's shape (out: such a
        tensor, overwritten).  Every element is summed by one owner in a fixed
        order in f64: two calls give identical bytes.  Band elements past the
        last site (i + k >= n) are never read; X must be finite.  The tensors'
        pending work is synchronised first; needs no load."""
        import torch

        def dev(t, what, dtypes):
            if not all(hasattr(t, a) for a in ("data_ptr", "stride", "dtype", "shape", "device")):
                raise ValueError("%s must be a device tensor" % what)
            if getattr(t.device, "type", "") != "cuda":
                raise ValueError("%s must be on the context's GPU, not on %s" % (what, t.device))
            if t.device.index is not None and t.device.index != self.device:
                raise ValueError("%s is on device %d; the context runs on %d" % (what, t.device.index, self.device))
            if t.dtype not in dtypes:
                raise ValueError("%s has dtype %s; it must be one of %s" % (what, t.dtype, ", ".join(map(str, dtypes))))

        def stride_of(t, width, what):
            # rows `ld` elements apart, contiguous inside a row
            if t.dim() == 2 and t.shape[1] > 1 and t.stride(1) != 1:
                raise ValueError("%s must have contiguous rows (last stride 1)" % what)
            ld = int(t.stride(0)) if t.shape[0] > 1 else width
            if ld < width:
                raise ValueError("%s's row stride %d is below its width %d" % (what, ld, width))
            return ld

        dev(band, "band", (torch.float32, torch.float16))
        dev(X, "X", (torch.float32, torch.float64))
        if band.dim() != 2 or band.shape[0] < 1 or band.shape[1] < 1:
            raise ValueError("band must be a [n, bandwidth + 1] tensor")
        n = int(band.shape[0])
        K = int(band.shape[1]) - 1 if bandwidth is None else int(bandwidth)
        if K < 0 or K > int(band.shape[1]) - 1:
            raise ValueError("bandwidth %d does not fit the band's %d columns" % (K, int(band.shape[1])))
        if X.dim() not in (1, 2) or int(X.shape[0]) != n or (X.dim() == 2 and X.shape[1] < 1):
            raise ValueError("X must be [n] or [n, n_cols] with n = %d, not %s" % (n, tuple(X.shape)))
        n_cols = 1 if X.dim() == 1 else int(X.shape[1])
        if out is None:
            out = torch.empty(tuple(X.shape), dtype=torch.float64, device=X.device)
        else:
            dev(out, "out", (torch.float64,))
            if tuple(out.shape) != tuple(X.shape):
                raise ValueError("out has shape %s; X has %s" % (tuple(out.shape), tuple(X.shape)))
        ld = stride_of(band, int(band.shape[1]), "band")
        ldx, ldy = stride_of(X, n_cols, "X"), stride_of(out, n_cols, "out")
        torch.cuda.synchronize(X.device)
        check(lib().wld_banded_apply_device(
            self._h, ctypes.c_void_p(int(band.data_ptr())), MATRIX_F16 if band.dtype == torch.float16 else MATRIX_F32, ld,
            n, K, ctypes.c_void_p(int(X.data_ptr())), APPLY_X_F64 if X.dtype == torch.float64 else APPLY_X_F32, ldx,
            n_cols, ctypes.c_void_p(int(out.data_ptr())), ldy), "wld_banded_apply_device")
        return out

    def banded_cholesky(self, band, ridge=0.0, diag=None, out=None, bandwidth=None):
        """wld_banded_cholesky_device: the Cholesky factor U (A = U^T U, upper
        triangular, U[i, i] > 0) of the symmetric matrix A whose upper band is
        `band` — a [n, W] float32 or float16 device tensor as banded_apply
        takes it (bandwidth None: W - 1) — with the diagonal fl(fl(band[i, 0] +
        ridge) + diag[i]) (diag: a float64 [n] device tensor or None).  Returns
        (factor, LdBandedCholInfo): factor a float64 [n, K + 1] device tensor in
        the same layout (factor[i, k] = U[i, i + k], +0.0 where i + k >= n; out:
        such a tensor, rows may be strided, overwritten).  About n K^2 flops on
        f64 MFMAs; every element has one owner and a fixed order, so two calls
        give identical bytes.

        A band that is not positive definite is a result, not an error:
        info.ok is False, info.first_bad the first row whose pivot was not > 0,
        and only the factor's rows below 64 * (first_bad // 64) are valid; no
        pivot is ever replaced.  banded_logdet(factor) gives log det A.

        Sampling: for e ~ N(0, I), banded_solve(factor, e, "backward") has
        covariance A^-1 (a draw from N(0, A^-1)); U^T e, i.e. the inverse of
        the "forward" solve, has covariance A.  Whitening: for z ~ N(0, A),
        banded_solve(factor, z, "forward") is N(0, I).  The tensors' pending
        work is synchronised first; needs no load."""
        import torch

        n, K, dt, ld, ldf = banded_chol_args(band, ridge, diag, out, bandwidth, self.device)
        if out is None:
            out = torch.empty((n, K + 1), dtype=torch.float64, device=band.device)
            ldf = K + 1
        info = BandedCholInfoC()
        torch.cuda.synchronize(band.device)
        check(lib().wld_banded_cholesky_device(
            self._h, ctypes.c_void_p(int(band.data_ptr())), dt, ld, n, K, float(ridge),
            None if diag is None else ctypes.c_void_p(int(diag.data_ptr())), ctypes.c_void_p(int(out.data_ptr())), ldf,
            ctypes.byref(info)), "wld_banded_cholesky_device")
        ok = int(info.first_bad) == n
        return out, LdBandedCholInfo(ok=ok, first_bad=None if ok else int(info.first_bad),
                                     min_pivot=float(info.min_pivot), kernel_ms=float(info.kernel_ms))

    def banded_solve(self, factor, b, mode="full", out=None):
        """wld_banded_solve_device: the solution of A x = b (mode "full"), U^T y
        = b ("forward") or U x = b ("backward") for the factor of
        banded_cholesky (a float64 [n, K + 1] device tensor, rows may be
        strided) and b a [n] or [n, n_cols] float32 or float64 device tensor,
        which is converted to float64 and never modified.  Returns a new
        float64 tensor of b's shape (out: such a tensor, overwritten; it may be
        b itself).  Substitution throughout, one owner and a fixed order per
        element: two calls give identical bytes.  Neither argument is
        validated: non-finite values propagate.

        For e ~ N(0, I), "backward" gives a draw with covariance A^-1;
        "forward" whitens a draw from N(0, A)."""
        import torch

        n, K, ldf, md, n_cols = banded_solve_args(factor, b, mode, out, self.device)
        if out is None:
            out = torch.empty(tuple(b.shape), dtype=torch.float64, device=b.device)
        if out.data_ptr() != b.data_ptr() or b.dtype != torch.float64:
            out.copy_(b)
        ldb = _row_stride(out, n_cols, "out")
        torch.cuda.synchronize(out.device)
        check(lib().wld_banded_solve_device(self._h, ctypes.c_void_p(int(factor.data_ptr())), ldf, n, K, md,
                                            ctypes.c_void_p(int(out.data_ptr())), ldb, n_cols, None),
              "wld_banded_solve_device")
        return out

    def banded_pairsum(self, band, out=None, bandwidth=None):
        """wld_banded_pairsum_device: the pair-sum table M of `band` — a [n, W]
        float32 or float16 device tensor as banded_apply takes it (bandwidth
        None: W - 1; column 0 and the elements with j + k >= n are never read,
        NaN and +-inf count as 0) — as a float64 [n, K + 1] device tensor in
        the same layout: M[j, k] is the sum of the band's entries (u, v) with
        j <= u < v <= j + k, +0.0 where j + k >= n (out: such a tensor, rows may
        be strided, overwritten; it must not overlap the band).  The bytes are
        banded_pairsum_host's; two calls give identical bytes.  Returns (M,
        LdPairsumInfo).  The tensors' pending work is synchronised first; needs
        no load."""
        import torch

        n, K, dt, ld, lds = banded_pairsum_args(band, out, bandwidth, self.device)
        if out is None:
            out = torch.empty((n, K + 1), dtype=torch.float64, device=band.device)
            lds = K + 1
        info = BandedPairsumInfoC()
        torch.cuda.synchronize(band.device)
        check(lib().wld_banded_pairsum_device(self._h, ctypes.c_void_p(int(band.data_ptr())), dt, ld, n, K,
                                              ctypes.c_void_p(int(out.data_ptr())), lds, ctypes.byref(info)),
              "wld_banded_pairsum_device")
        return out, LdPairsumInfo(bandwidth=int(info.bandwidth), nonfinite=int(info.nonfinite),
                                  kernel_ms=float(info.kernel_ms))

    def banded_omega(self, M, split, lo, hi, min_side=2, eps=1e-5, out=None):
        """wld_banded_omega_device: the sweep scan of banded_omega_host on the
        device, with the same bytes.  M: banded_pairsum's table, a float64
        [n, K + 1] device tensor (rows may be strided).  split, lo, hi: uint32
        or int32 device tensors, or lists / numpy arrays (copied to the
        device); they are checked on the host before the call when they are
        host arrays, and by the library on the device in either case.  out: a
        dict of contiguous device tensors omega, zns (float64) and left, right
        (int32 or uint32 storage) of n_splits entries to write into.  Returns
        an LdOmega (numpy arrays)."""
        import torch

        _dev_tensor(M, "M", ("float64",), self.device)
        shape = tuple(int(x) for x in M.shape)
        if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
            raise ValueError("M must be a [n, bandwidth + 1] tensor")
        n, K = shape[0], shape[1] - 1
        lds = _row_stride(M, K + 1, "M")
        on_dev = [hasattr(x, "data_ptr") for x in (split, lo, hi)]
        if any(on_dev) and not all(on_dev):
            raise ValueError("split, lo and hi must all be device tensors or all host arrays")
        if all(on_dev):
            ts = []
            for x, what in ((split, "split"), (lo, "lo"), (hi, "hi")):
                _dev_tensor(x, what, ("int32", "uint32"), self.device)
                if x.dim() != 1 or (x.shape[0] > 1 and x.stride(0) != 1):
                    raise ValueError("%s must be a contiguous 1-D tensor" % what)
                ts.append(x)
            if not (ts[0].shape[0] == ts[1].shape[0] == ts[2].shape[0]) or ts[0].shape[0] < 1:
                raise ValueError("split, lo and hi must have the same length, at least 1")
            try:
                min_side, eps = int(min_side), float(eps)
            except (TypeError, ValueError):
                raise ValueError("min_side must be an integer and eps a number")
            if min_side < 2 or min_side > 0xFFFFFFFF or not np.isfinite(eps) or eps < 0:
                raise ValueError("min_side must be at least 2 and eps finite and >= 0")
        else:
            c, l, h, min_side, eps = omega_args(n, K, split, lo, hi, min_side, eps)
            ts = [torch.from_numpy(x.view(np.int32)).to(M.device) for x in (c, l, h)]
        G = int(ts[0].shape[0])
        if out is None:
            out = {"omega": torch.empty(G, dtype=torch.float64, device=M.device),
                   "zns": torch.empty(G, dtype=torch.float64, device=M.device),
                   "left": torch.empty(G, dtype=torch.int32, device=M.device),
                   "right": torch.empty(G, dtype=torch.int32, device=M.device)}
        else:
            for name, names in (("omega", ("float64",)), ("zns", ("float64",)), ("left", ("int32", "uint32")),
                                ("right", ("int32", "uint32"))):
                if name not in out:
                    raise ValueError("out needs the tensors omega, zns, left and right")
                _dev_tensor(out[name], "out[%r]" % name, names, self.device)
                if tuple(out[name].shape) != (G,) or (G > 1 and out[name].stride(0) != 1):
                    raise ValueError("out[%r] must be a contiguous [%d] tensor" % (name, G))
        info = BandedOmegaInfoC()
        torch.cuda.synchronize(M.device)
        p = lambda t: ctypes.c_void_p(int(t.data_ptr()))  # noqa: E731
        check(lib().wld_banded_omega_device(self._h, p(M), lds, n, K, p(ts[0]), p(ts[1]), p(ts[2]), G, min_side, eps,
                                            p(out["omega"]), p(out["left"]), p(out["right"]), p(out["zns"]),
                                            ctypes.byref(info)), "wld_banded_omega_device")
        u32 = lambda t: t.cpu().numpy().view(np.uint32).copy()  # noqa: E731
        return LdOmega(split=u32(ts[0]), lo=u32(ts[1]), hi=u32(ts[2]), omega=out["omega"].cpu().numpy(),
                       left=u32(out["left"]), right=u32(out["right"]), zns=out["zns"].cpu().numpy(), min_side=min_side,
                       eps=eps, evaluated=int(info.evaluated), skipped=int(info.skipped), kernel_ms=float(info.kernel_ms))

    def run_omega(self, n_grid=0, max_side=None, min_side=2, max_distance=None, eps=1e-5, dtype="float32"):
        """wld_run_omega: the whole sweep scan on the loaded set under the
        context's CURRENT window: the splits of omega_splits(site_map, n_grid,
        max_side, max_distance), an r2 band with zero_missing of the width the
        window needs (dtype "float32" or "float16"), its pair sums and the scan.
        A window that drops pairs some split needs is refused (WldError): a
        window of max_sites 2 max_side - 1 and no max_distance always
        suffices.  Returns an LdOmega with position, n_sites, bandwidth, band
        and sums."""
        if max_side is None:
            raise ValueError("max_side is required")
        if dtype not in _MATRIX_DTYPES:
            raise ValueError('dtype must be "float32" or "float16"')
        try:
            n_grid, max_side, min_side, D, eps = int(n_grid), int(max_side), int(min_side), int(max_distance or 0), float(eps)
        except (TypeError, ValueError):
            raise ValueError("n_grid, max_side, min_side and max_distance must be integers and eps a number")
        if n_grid < 0 or n_grid > 0xFFFFFFFF or max_side < 1 or max_side > 0xFFFFFFFF or D < 0 or D >= 1 << 64:
            raise ValueError("n_grid, max_side (at least 1) and max_distance must be non-negative integers")
        if min_side < 2 or min_side > 0xFFFFFFFF or not np.isfinite(eps) or eps < 0:
            raise ValueError("min_side must be at least 2 and eps finite and >= 0")
        o = OmegaC()
        check(lib().wld_run_omega(self._h, n_grid, max_side, min_side, D, eps, _MATRIX_DTYPES[dtype], ctypes.byref(o)),
              "wld_run_omega")
        G = int(o.n_splits)

        def grab(p, dt):
            return np.ctypeslib.as_array(p, shape=(G,)).astype(dt, copy=True)

        b = o.band
        res = LdOmega(position=grab(o.position, np.uint64), split=grab(o.split, np.uint32), lo=grab(o.lo, np.uint32),
                      hi=grab(o.hi, np.uint32), omega=grab(o.omega, np.float64), left=grab(o.left, np.uint32),
                      right=grab(o.right, np.uint32), zns=grab(o.zns, np.float64), min_side=min_side, eps=eps,
                      evaluated=int(o.scan.evaluated), skipped=int(o.scan.skipped), kernel_ms=float(o.scan.kernel_ms),
                      n_sites=int(o.n_sites), bandwidth=int(o.bandwidth),
                      band=LdBandedInfo(rows=(int(b.row_begin), int(b.row_end)), bandwidth=int(b.bandwidth), stat="r2",
                                        dtype=dtype, zero_missing=True, pairs=int(b.pairs), none_pairs=int(b.none_pairs),
                                        nonfinite_pairs=int(b.nonfinite_pairs), counted_pairs=int(b.counted_pairs),
                                        tiles=int(b.tiles), kernel_ms=float(b.kernel_ms)),
                      sums=LdPairsumInfo(bandwidth=int(o.sums.bandwidth), nonfinite=int(o.sums.nonfinite),
                                         kernel_ms=float(o.sums.kernel_ms)))
        lib().wld_omega_free(ctypes.byref(o))
        return res

    def run_partners(self, k, r2_threshold, chunk_begin=0, chunk_end=0):
        """wld_run_partners: for every LOADED site its best k partners (r2 >
        r2_threshold, r2 descending then partner ascending) among the pairs of
        the linear chunk range (end 0 = all) under the context's window, as an
        LdPartners; values bit-identical to the default row path's row of the
        pair.  1 <= k <= PARTNERS_MAX_K."""
        out = PartnersC()
        k = int(k)
        if k < 0 or k > 0xFFFFFFFF:
            raise ValueError("k must be between 1 and %d" % PARTNERS_MAX_K)
        check(lib().wld_run_partners(self._h, k, r2_threshold, chunk_begin, chunk_end, ctypes.byref(out)),
              "wld_run_partners")
        L, kk = int(out.n_sites), int(out.k)

        def grab(p, shape, dt):
            return (np.ctypeslib.as_array(p, shape=shape).astype(dt, copy=True) if L
                    else np.zeros(shape, dtype=dt))

        res = LdPartners(count=grab(out.count, (L,), np.uint32), partner=grab(out.partner, (L, kk), np.uint32),
                         d=grab(out.d, (L, kk), np.float32), d_prime=grab(out.d_prime, (L, kk), np.float32),
                         r2=grab(out.r2, (L, kk), np.float32), pairs=int(out.pairs), none_pairs=int(out.none_pairs),
                         passing_pairs=int(out.passing_pairs), tiles=int(out.tiles), kernel_ms=float(out.kernel_ms),
                         merge_ms=float(out.merge_ms))
        lib().wld_partners_free(ctypes.byref(out))
        return res

    def run_block_breaks(self, strong_min, stat="r2", chunk_begin=0, chunk_end=0):
        """wld_run_block_breaks: pass 1 of the LD blocks over the linear chunk
        range (end 0 = all) under the context's window, as an LdBlockBreaks.
        An informative pair is weak iff its value (stat: "r2", or "dprime" for
        the row path's |d_prime|) is below strong_min."""
        out = BlockBreaksC()
        check(lib().wld_run_block_breaks(self._h, _block_code(BLOCK_STATS, "stat", stat), strong_min, chunk_begin,
                                         chunk_end, ctypes.byref(out)), "wld_run_block_breaks")
        L = int(out.n_sites)
        arrays = [np.ctypeslib.as_array(p, shape=(L,)).astype(np.uint32, copy=True) if L
                  else np.zeros(0, dtype=np.uint32) for p in (out.fwd_weak, out.bwd_weak, out.last)]
        res = LdBlockBreaks._from_c(out, arrays)
        lib().wld_block_breaks_free(ctypes.byref(out))
        return res

    def blocks_from_breaks(self, breaks, rule="all", min_sites=2):
        """wld_blocks_from_breaks: the partition of an LdBlockBreaks of the
        loaded set and the statistics of its blocks (pass 2), as an LdBlocks."""
        a, keep = breaks._to_c()
        out = BlocksC()
        check(lib().wld_blocks_from_breaks(self._h, ctypes.byref(a), _block_code(BLOCK_RULES, "rule", rule),
                                           int(min_sites), ctypes.byref(out)), "wld_blocks_from_breaks")
        return _take_blocks(out)

    def run_blocks(self, strong_min, stat="r2", rule="all", min_sites=2):
        """wld_run_blocks: both passes over every chunk under the context's
        window, as an LdBlocks: maximal runs of consecutive LOADED sites
        without a weak pair (rule "all") or with a solid spine (rule "spine"),
        of at least min_sites sites, with their statistics."""
        out = BlocksC()
        check(lib().wld_run_blocks(self._h, _block_code(BLOCK_STATS, "stat", stat), strong_min,
                                   _block_code(BLOCK_RULES, "rule", rule), int(min_sites), ctypes.byref(out)),
              "wld_run_blocks")
        return _take_blocks(out)

    def run_prune(self, r2_threshold, priority=None):
        """wld_run_prune: the greedy r2-independent set of the loaded sites at
        this threshold under the context's window, as an LdPrune (keep, tag in
        LOADED indices).  priority: None (index order) or one float per loaded
        site, larger first, ties to the lower index; NaN is refused."""
        pr = None
        if priority is not None:
            pr = np.ascontiguousarray(priority, dtype=np.float32)
            if pr.ndim != 1:
                raise ValueError("priority must be one float per loaded site")
            n = int(lib().wld_loaded_sites(self._h))
            if n and pr.size != n:  # (not loaded: the library refuses the call)
                raise ValueError("priority has %d entries for %d loaded sites" % (pr.size, n))
        out = Prune()
        check(lib().wld_run_prune(self._h, r2_threshold, None if pr is None else _p(pr, ctypes.c_float),
                                  ctypes.byref(out)), "wld_run_prune")
        L = int(out.n_sites)

        def grab(p, dt):
            return np.ctypeslib.as_array(p, shape=(L,)).astype(dt, copy=True) if L else np.zeros(0, dtype=dt)

        res = LdPrune(keep=grab(out.keep, np.uint8).astype(bool), tag=grab(out.tag, np.uint32), n_kept=int(out.n_kept),
                      edges=int(out.edges), rounds=int(out.rounds), pair_ms=float(out.pair_ms),
                      prune_ms=float(out.prune_ms))
        lib().wld_prune_free(ctypes.byref(out))
        return res

    def run_targets(self, targets, r2_threshold):
        """wld_run_targets: the rows (r2 > r2_threshold) of the listed LOADED
        site indices against every in-window partner, as a TargetRows: by list
        position, then partner ascending; values bit-identical to the default
        row path's row of the pair."""
        t = np.ascontiguousarray(targets, dtype=np.int64).reshape(-1)
        if t.size and (t.min() < 0 or t.max() > 0xFFFFFFFF):
            raise ValueError("targets must be loaded site indices (32-bit, nonnegative)")
        t = t.astype(np.uint32)
        out = TargetRowsC()
        check(lib().wld_run_targets(self._h, _p(t, ctypes.c_uint32) if t.size else None, int(t.size), r2_threshold,
                                    ctypes.byref(out)), "wld_run_targets")
        n, q = int(out.n), int(out.n_targets)

        def grab(p, m, dt):
            return np.ctypeslib.as_array(p, shape=(m,)).astype(dt, copy=True) if m else np.zeros(0, dtype=dt)

        res = TargetRows(offset=grab(out.offset, q + 1, np.uint64), target=grab(out.target, n, np.uint32),
                         site_target=grab(out.site_target, n, np.uint32),
                         site_partner=grab(out.site_partner, n, np.uint32), d=grab(out.d, n, np.float32),
                         d_prime=grab(out.d_prime, n, np.float32), r2=grab(out.r2, n, np.float32),
                         items=int(out.items), batches=int(out.batches), kernel_ms=float(out.kernel_ms))
        lib().wld_target_rows_free(ctypes.byref(out))
        return res

    def prune_times(self):
        """wld_prune_times: the last run_prune's prune_ms by phase, (csr_ms, rounds_ms, tags_ms)."""
        t = [ctypes.c_double() for _ in range(3)]
        check(lib().wld_prune_times(self._h, *[ctypes.byref(x) for x in t]), "wld_prune_times")
        return tuple(float(x.value) for x in t)

    def stream_ptr(self):
        """The context's hipStream_t as an int (torch.cuda.ExternalStream)."""
        return int(lib().wld_stream(self._h) or 0)

    def set_stream(self, stream):
        """wld_set_stream: run on another context's stream (a Context), a
        hipStream_t given as an int, or None for the context's own.  A borrowed
        Context stream stays referenced here, and the owner hands this context
        back its own stream before its close() destroys the borrowed one."""
        ptr = stream.stream_ptr() if isinstance(stream, Context) else (stream or 0)
        check(lib().wld_set_stream(self._h, ctypes.c_void_p(ptr) if ptr else None), "wld_set_stream")
        old = getattr(self, "_stream_owner", None)
        if old is not None:
            old._borrowers.discard(self)
        self._stream_owner = stream if isinstance(stream, Context) else None
        if self._stream_owner is not None:
            self._stream_owner._borrowers.add(self)

    def rows(self):
        v = Pairs()
        check(lib().wld_rows_device(self._h, ctypes.byref(v)), "wld_rows_device")
        n = int(v.n)
        a = np.zeros(n, dtype=np.uint32)
        b = np.zeros(n, dtype=np.uint32)
        d = np.zeros(n, dtype=np.float32)
        dp = np.zeros(n, dtype=np.float32)
        r2 = np.zeros(n, dtype=np.float32)
        if n:
            check(lib().wld_rows_copy(self._h, _p(a, ctypes.c_uint32), _p(b, ctypes.c_uint32), _p(d, ctypes.c_float),
                                      _p(dp, ctypes.c_float), _p(r2, ctypes.c_float)), "wld_rows_copy")
        return PairStore(a, b, d, dp, r2)

    def rows_device(self):
        v = Pairs()
        check(lib().wld_rows_device(self._h, ctypes.byref(v)), "wld_rows_device")
        addr = lambda p: ctypes.cast(p, ctypes.c_void_p).value or 0  # noqa: E731
        return {"n": int(v.n), "site_a": addr(v.site_a), "site_b": addr(v.site_b), "d": addr(v.d),
                "d_prime": addr(v.d_prime), "r2": addr(v.r2)}

    def rows_copy_device(self, site_a, site_b, d, d_prime, r2):
        """Copies the last run's rows into caller device buffers (raw pointers, 0 = skip)."""
        vp = lambda x: ctypes.c_void_p(x or None)  # noqa: E731
        check(lib().wld_rows_copy_device(self._h, vp(site_a), vp(site_b), vp(d), vp(d_prime), vp(r2)),
              "wld_rows_copy_device")

    def dense(self, n_sites):
        d = np.zeros((n_sites, n_sites), dtype=np.float32)
        dp = np.zeros_like(d)
        r2 = np.zeros_like(d)
        valid = np.zeros((n_sites, n_sites), dtype=np.uint8)
        check(lib().wld_dense(self._h, _p(d, ctypes.c_float), _p(dp, ctypes.c_float), _p(r2, ctypes.c_float),
                              _p(valid, ctypes.c_uint8)), "wld_dense")
        return d, dp, r2, valid

    def stats(self):
        s = RunStats()
        check(lib().wld_last_stats(self._h, ctypes.byref(s)), "wld_last_stats")
        return {f: getattr(s, f) for f, _ in RunStats._fields_}

    @staticmethod
    def chunk_rows(n_sites):
        return int(lib().wld_chunk_rows(n_sites))

    @staticmethod
    def shard_chunk_rows(n_sites, n_shards, shard):
        b, e = ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().wld_shard_chunk_rows(n_sites, n_shards, shard, ctypes.byref(b), ctypes.byref(e)), "shard")
        return int(b.value), int(e.value)

    @staticmethod
    def chunks(n_sites):
        return int(lib().wld_chunks(n_sites))

    @staticmethod
    def shard_chunks(n_sites, n_shards, shard):
        """Linear chunk range [begin, end) of `shard` (wld_shard_chunks)."""
        b, e = ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().wld_shard_chunks(n_sites, n_shards, shard, ctypes.byref(b), ctypes.byref(e)), "shard_chunks")
        return int(b.value), int(e.value)

    @staticmethod
    def pairs_in_chunks(n_sites, begin, end):
        return int(lib().wld_pairs_in_chunks(n_sites, begin, end))


_default = {}


def default_context(device=0):
    if device not in _default:
        _default[device] = Context(device)
    return _default[device]


def single_weighted_ld_pair(a, a_hist, b, b_hist, weights, ctx=None):
    """lib.rs:390-521 -> LdStats or None.  a_hist/b_hist are accepted for
    signature parity; the device derives the same histograms from a and b."""
    ctx = ctx or default_context()
    av = np.ascontiguousarray(a, dtype=np.uint8)
    bv = np.ascontiguousarray(b, dtype=np.uint8)
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if not (av.size == bv.size == w.size):
        raise ValueError("a, b and weights must have the same length (lib.rs:397-398)")
    out = np.zeros(3, dtype=np.float32)
    r = check(lib().wld_single_weighted_ld_pair(ctx._h, _p(av, ctypes.c_uint8), _p(bv, ctypes.c_uint8),
                                                _p(w, ctypes.c_float), av.size, _p(out, ctypes.c_float)),
              "single_weighted_ld_pair")
    if r == 0:
        return None
    return LdStats(r2=float(out[2]), d=float(out[0]), d_prime=float(out[1]))


def all_weighted_ld_pairs(site_set, weights, r2_threshold, progress_report=None, ctx=None, max_distance=None,
                          max_sites=None):
    """lib.rs:578-684 -> PairStore in reference order (parent site indices).
    max_distance / max_sites (not in the reference): the window of
    Context.set_window for this call; the context's own window is restored
    afterwards."""
    ctx = ctx or default_context()
    if max_distance is not None or max_sites is not None:
        before = ctx.window()
        ctx.set_window(max_distance, max_sites)
        try:
            return all_weighted_ld_pairs(site_set, weights, r2_threshold, progress_report, ctx)
        finally:
            ctx.set_window(*before)
    buf = site_set.buffer
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.size != site_set.n_seqs():
        raise ValueError("weights must have n_seqs entries")
    sm = site_set.site_map
    cb = PROGRESS_FN(lambda n, _u: progress_report(int(n))) if progress_report else PROGRESS_FN()
    out = Pairs()
    check(lib().wld_all_weighted_ld_pairs(ctx._h, _p(buf, ctypes.c_uint8), buf.shape[0], buf.shape[1],
                                          None if sm is None else _p(sm, ctypes.c_uint64), _p(w, ctypes.c_float),
                                          r2_threshold, cb, None, ctypes.byref(out)), "all_weighted_ld_pairs")
    return _take_pairs(out)


def ld_summary(site_set, weights, bin_width=None, n_bins=None, max_distance=None, max_sites=None, ctx=None):
    """Per-site LD scores and (bin_width, n_bins given) the r2 decay by
    distance of every pair of site_set (not in the reference): loads the set
    and runs Context.run_summary under the window max_distance / max_sites
    (the context's own window is restored afterwards).  Returns an LdSummary
    indexed by the set's own site index; distances are in site_map
    coordinates."""
    ctx = ctx or default_context()
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.size != site_set.n_seqs():
        raise ValueError("weights must have n_seqs entries")
    before = ctx.window()
    if max_distance is not None or max_sites is not None:
        ctx.set_window(max_distance, max_sites)
    try:
        ctx.load(site_set.buffer, w, site_set.site_map)
        return ctx.run_summary(bin_width or 0, n_bins or 0)
    finally:
        ctx.set_window(*before)


def ld_heatmap(site_set, weights, stat="r2", sites_per_cell=None, cell_width=None, edges=None, region=None,
               max_distance=None, max_sites=None, ctx=None):
    """The LD heat map of site_set (not in the reference): builds the cells
    with heatmap_cells (exactly one of sites_per_cell, cell_width and edges;
    region optional), loads the set and runs Context.run_heatmap under the
    window max_distance / max_sites (the context's own window is restored
    afterwards).  Returns an LdHeatmap with cell_start, the parent coordinate
    each cell begins at, and site_cell."""
    ctx = ctx or default_context()
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.size != site_set.n_seqs():
        raise ValueError("weights must have n_seqs entries")
    site_cell, n_cells, cell_start = heatmap_cells(site_set, sites_per_cell=sites_per_cell, cell_width=cell_width,
                                                   edges=edges, region=region)
    before = ctx.window()
    if max_distance is not None or max_sites is not None:
        ctx.set_window(max_distance, max_sites)
    try:
        ctx.load(site_set.buffer, w, site_set.site_map)
        res = ctx.run_heatmap(site_cell, n_cells, stat)
    finally:
        ctx.set_window(*before)
    res.cell_start = cell_start
    res.site_cell = site_cell
    return res


def ld_annot_scores(site_set, weights, annot, self_term=False, names=None, max_distance=None, max_sites=None,
                    ctx=None):
    """Partitioned LD scores of site_set (not in the reference; LDSC's --l2
    --annot): checks annot (annot_matrix: a float32 [n_sites, n_annot] matrix
    indexed by the set's own site index) before any device call, loads the set
    and runs Context.run_annot_scores under the window max_distance /
    max_sites (the context's own window is restored afterwards).  names:
    optional column names, kept on the result.  Returns an LdAnnotScores."""
    a = annot_matrix(annot, site_set.n_sites())
    if names is not None:
        names = [str(x) for x in names]
        if len(names) != a.shape[1]:
            raise ValueError("%d names for %d annotation columns" % (len(names), a.shape[1]))
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.size != site_set.n_seqs():
        raise ValueError("weights must have n_seqs entries")
    ctx = ctx or default_context()
    before = ctx.window()
    if max_distance is not None or max_sites is not None:
        ctx.set_window(max_distance, max_sites)
    try:
        ctx.load(site_set.buffer, w, site_set.site_map)
        res = ctx.run_annot_scores(a, self_term)
    finally:
        ctx.set_window(*before)
    res.names = names
    return res


def ld_matrix(site_set, weights, region=None, stat="r", dtype="float32", zero_missing=False, max_distance=None,
              max_sites=None, out=None, ctx=None):
    """The LD matrix of site_set (not in the reference; PLINK's --r square,
    LDstore, LDlink's LDmatrix): loads the set and runs Context.run_matrix on
    the square of the sites in region = (start, stop), parent coordinates,
    start <= pos < stop (None: every site), under the window max_distance /
    max_sites (the context's own window is restored afterwards).  Returns
    (matrix, info, sites): the matrix (or out), its LdMatrixInfo and the parent
    coordinates of its rows and columns."""
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.size != site_set.n_seqs():
        raise ValueError("weights must have n_seqs entries")
    n = site_set.n_sites()
    sq = (0, n) if region is None else matrix_region(site_set.site_map, n, region)
    matrix_args(n, sq, sq, stat, dtype, out)  # (every refusal before the load)
    ctx = ctx or default_context()
    before = ctx.window()
    if max_distance is not None or max_sites is not None:
        ctx.set_window(max_distance, max_sites)
    try:
        ctx.load(site_set.buffer, w, site_set.site_map)
        m, info = ctx.run_matrix(sq, sq, stat, dtype, zero_missing, out)
    finally:
        ctx.set_window(*before)
    sm = site_set.site_map
    sites = (np.arange(sq[0], sq[1], dtype=np.uint64) if sm is None
             else np.asarray(sm, dtype=np.uint64)[sq[0]:sq[1]].copy())
    return m, info, sites


def ld_banded(site_set, weights, bandwidth=None, stat="r", dtype="float32", zero_missing=False, max_distance=None,
              max_sites=None, out=None, ctx=None):
    """The LD matrix of site_set in band storage (ld_matrix's matrix at the
    band's size: what a windowed matrix needs at chromosome scale): loads the
    set and runs Context.run_matrix_banded on every site under the window
    max_distance / max_sites (the context's own window is restored
    afterwards).  bandwidth None: the width the window needs.  Returns (band,
    info, sites): the [n_sites, bandwidth + 1] band (or out), its LdBandedInfo
    and the parent coordinates of its rows."""
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.size != site_set.n_seqs():
        raise ValueError("weights must have n_seqs entries")
    n = site_set.n_sites()
    banded_args(n, 0, None, None if bandwidth is None else bandwidth, stat, dtype,
                None if bandwidth is None else out)  # (what can be refused before the load)
    ctx = ctx or default_context()
    before = ctx.window()
    if max_distance is not None or max_sites is not None:
        ctx.set_window(max_distance, max_sites)
    try:
        ctx.load(site_set.buffer, w, site_set.site_map)
        m, info = ctx.run_matrix_banded(None, bandwidth, stat, dtype, zero_missing, out)
    finally:
        ctx.set_window(*before)
    sm = site_set.site_map
    sites = np.arange(n, dtype=np.uint64) if sm is None else np.asarray(sm, dtype=np.uint64).copy()
    return m, info, sites


def ld_omega(site_set, weights, n_grid=0, max_side=None, min_side=2, max_distance=None, eps=1e-5, dtype="float32",
             ctx=None):
    """A selective-sweep scan of site_set (not in the reference; OmegaPlus):
    Kim and Nielsen's omega, maximised per split over flanks of min_side to
    max_side sites, and Kelly's ZnS of each split's largest window.  Loads the
    set and runs Context.run_omega under the window max_sites = 2 max_side - 1,
    which it sets itself (the context's own window is restored afterwards).
    n_grid 0 scans every split, n_grid >= 1 that many equidistant positions;
    max_distance limits the flanks in coordinates as well.  Returns an LdOmega
    with site_map, the set's parent coordinates (None without a map)."""
    if max_side is None:
        raise ValueError("max_side is required")
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.size != site_set.n_seqs():
        raise ValueError("weights must have n_seqs entries")
    max_side = int(max_side)
    if max_side < 1 or max_side > 0x7FFFFFFF:
        raise ValueError("max_side must be at least 1")
    ctx = ctx or default_context()
    before = ctx.window()
    ctx.set_window(None, 2 * max_side - 1)
    try:
        sm = site_set.site_map
        ctx.load(site_set.buffer, w, sm)
        res = ctx.run_omega(n_grid, max_side, min_side, max_distance, eps, dtype)
    finally:
        ctx.set_window(*before)
    res.site_map = sm
    return res


def ld_prune(site_set, weights, r2_threshold, priority=None, max_distance=None, max_sites=None, ctx=None):
    """LD pruning (not in the reference; PLINK --indep-pairwise, bcftools
    +prune): loads site_set and runs Context.run_prune at r2_threshold under
    the window max_distance / max_sites (the context's own window is restored
    afterwards).  priority: None (index order), one float per site (larger
    first, ties to the lower index), or "maf" (maf_priority).  Returns an
    LdPrune indexed by the set's own site index, with kept_sites, the parent
    indices of the kept sites."""
    ctx = ctx or default_context()
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.size != site_set.n_seqs():
        raise ValueError("weights must have n_seqs entries")
    if isinstance(priority, str):
        if priority != "maf":
            raise ValueError("priority must be None, an array or \"maf\"")
        priority = maf_priority(site_set)
    before = ctx.window()
    if max_distance is not None or max_sites is not None:
        ctx.set_window(max_distance, max_sites)
    try:
        sm = site_set.site_map
        ctx.load(site_set.buffer, w, sm)
        res = ctx.run_prune(r2_threshold, priority)
    finally:
        ctx.set_window(*before)
    kept = np.flatnonzero(res.keep).astype(np.uint64)
    res.kept_sites = kept if sm is None else sm[kept]
    return res


def ld_targets(site_set, weights, r2_threshold, targets=None, parents=None, max_distance=None, max_sites=None,
               ctx=None):
    """Target-site LD (not in the reference; PLINK --ld-snp / --ld-snps): loads
    site_set and runs Context.run_targets at r2_threshold under the window
    max_distance / max_sites (the context's own window is restored
    afterwards).  Exactly one of targets (the set's own site indices) and
    parents (parent coordinates: each maps to every site of the set carrying
    it, in site order — multi-allelic VCF lines share a POS; one that no site
    carries raises ValueError) must be given.  Returns a TargetRows whose
    `targets` are the site indices the `target` column refers to."""
    if (targets is None) == (parents is None):
        raise ValueError("give exactly one of targets and parents")
    ctx = ctx or default_context()
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.size != site_set.n_seqs():
        raise ValueError("weights must have n_seqs entries")
    sm = site_set.site_map
    if parents is not None:
        pos = np.arange(site_set.n_sites(), dtype=np.uint64) if sm is None else np.asarray(sm, dtype=np.uint64)
        chosen = []
        for c in np.asarray(parents).reshape(-1).tolist():
            hit = np.flatnonzero(pos == np.uint64(c)) if c >= 0 else np.zeros(0, dtype=np.int64)
            if hit.size == 0:
                raise ValueError("no site of the set has parent coordinate %d" % c)
            chosen.extend(hit.tolist())
        targets = chosen
    targets = np.ascontiguousarray(targets, dtype=np.int64).reshape(-1)
    before = ctx.window()
    if max_distance is not None or max_sites is not None:
        ctx.set_window(max_distance, max_sites)
    try:
        ctx.load(site_set.buffer, w, sm)
        res = ctx.run_targets(targets, r2_threshold)
    finally:
        ctx.set_window(*before)
    res.targets = targets.astype(np.uint32)
    return res


def ld_partners(site_set, weights, k, r2_threshold, max_distance=None, max_sites=None, ctx=None):
    """Best partners (not in the reference; the all-sites form of a proxy
    search): loads site_set and runs Context.run_partners(k, r2_threshold)
    under the window max_distance / max_sites (the context's own window is
    restored afterwards).  Returns an LdPartners indexed by the set's own site
    index, with site_map, the set's parent coordinates (None without a map)."""
    ctx = ctx or default_context()
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.size != site_set.n_seqs():
        raise ValueError("weights must have n_seqs entries")
    before = ctx.window()
    if max_distance is not None or max_sites is not None:
        ctx.set_window(max_distance, max_sites)
    try:
        sm = site_set.site_map
        ctx.load(site_set.buffer, w, sm)
        res = ctx.run_partners(k, r2_threshold)
    finally:
        ctx.set_window(*before)
    res.site_map = sm
    return res


def ld_blocks(site_set, weights, strong_min, stat="r2", rule="all", min_sites=2, max_distance=None, max_sites=None,
              ctx=None):
    """LD blocks (not in the reference; Haploview's blocks, PLINK's --blocks):
    loads site_set and runs Context.run_blocks(strong_min, stat, rule,
    min_sites) under the window max_distance / max_sites (the context's own
    window is restored afterwards).  stat "dprime" is the row path's |d_prime|,
    not the textbook |D'|: r2 is the default.  Returns an LdBlocks indexed by
    the set's own site index, with site_map, the set's parent coordinates (None
    without a map)."""
    ctx = ctx or default_context()
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.size != site_set.n_seqs():
        raise ValueError("weights must have n_seqs entries")
    before = ctx.window()
    if max_distance is not None or max_sites is not None:
        ctx.set_window(max_distance, max_sites)
    try:
        sm = site_set.site_map
        ctx.load(site_set.buffer, w, sm)
        res = ctx.run_blocks(strong_min, stat, rule, min_sites)
    finally:
        ctx.set_window(*before)
    res.site_map = sm
    return res


def _take_pairs(out):
    """Library-allocated host wld_pairs -> PairStore (copies, then frees)."""
    n = int(out.n)

    def grab(p, dt):
        return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)

    store = PairStore(grab(out.site_a, np.uint32), grab(out.site_b, np.uint32), grab(out.d, np.float32),
                      grab(out.d_prime, np.float32), grab(out.r2, np.float32))
    lib().wld_pairs_free(ctypes.byref(out))
    return store
