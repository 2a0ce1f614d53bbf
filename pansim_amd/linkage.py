"""Linkage disequilibrium between loci over the C ABI (docs/LINKAGE_DISEQUILIBRIUM.md): what `Population.locus_ld`,
`Simulation.locus_ld` and `MultiSimulation.locus_ld` return, and the two host-only restatements.

All computation happens in the HIP library; this module only marshals buffers.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Ld, LdParams, check
from .population import _metric as _core_or_acc, _ptr, _u32


class LocusLd:
    """The result of `locus_ld` (ps_ld_t + the arrays): the summary fields as attributes (integers; `mean_r2` a float),
    `locus_index` and `locus_count` (`loci` uint32 each: the column and the ones of every selected locus), `hist` ((lag_bins,
    r2_bins) uint64) and `lag_sum_q` (lag_bins uint64)."""
    FIELDS = tuple(name for name, _ in Ld._fields_)

    def __init__(self, o, index, count, hist, lag_sum_q):
        for name in self.FIELDS:
            v = getattr(o, name)
            setattr(self, name, float(v) if name == "mean_r2" else int(v))
        self.locus_index, self.locus_count = index[:self.loci], count[:self.loci]
        self.hist = hist.reshape(self.lag_bins, self.r2_bins)
        self.lag_sum_q = lag_sum_q

    def summary(self):
        return {name: getattr(self, name) for name in self.FIELDS}


def _ld_params(r2_bins, lag_bins, min_minor, max_loci):
    return LdParams(int(r2_bins), int(lag_bins), int(min_minor), int(max_loci))


def _ld_call(fn, prm, loci, *head):
    """fn(*head, &params, loci, n_loci, &summary, index, count, hist, lag_sum_q) -> LocusLd"""
    o = Ld()
    lst = None if loci is None else _u32(loci).reshape(-1)
    room = max(1, min(int(prm.max_loci), 65536) if lst is None else lst.size)
    index, count = np.zeros(room, np.uint32), np.zeros(room, np.uint32)
    nb = max(1, min(int(prm.r2_bins) * int(prm.lag_bins), 16384))      # (the library rejects bad bins itself)
    hist, lag = np.zeros(nb, np.uint64), np.zeros(max(1, min(int(prm.lag_bins), 32)), np.uint64)
    check(fn(*head, C.byref(prm), _ptr(lst), 0 if lst is None else lst.size, C.byref(o), _ptr(index), _ptr(count), _ptr(hist), _ptr(lag)))
    return LocusLd(o, index, count, hist[:int(o.r2_bins * o.lag_bins)], lag[:int(o.lag_bins)])


def _metric(metric):
    return _core_or_acc(metric, _lib.PS_LD_CORE, _lib.PS_LD_ACC)


def ld_select_loci(ones, pop_size, min_minor=1, max_loci=4096):
    """the automatic selection of `locus_ld` from the ones of every column, on the host alone (ps_ld_select_loci; no
    device) -> (index, candidates)"""
    ones = _u32(ones).reshape(-1)
    index = np.zeros(max(1, min(int(max_loci), 65536)), np.uint32)
    n, cand = C.c_uint64(), C.c_uint64()
    check(_lib.load().ps_ld_select_loci(_ptr(ones), ones.size, int(pop_size), int(min_minor), int(max_loci), _ptr(index), C.byref(n),
                                        C.byref(cand)))
    return index[:n.value], int(cand.value)


def ld_from_counts(locus_index, locus_count, n11, pop_size, r2_bins=64, lag_bins=1):
    """`locus_ld` from the columns and ones of M loci and n11 of their M (M - 1) / 2 pairs (a, b), a < b, row-major, on the
    host alone (ps_ld_from_counts; no device) -> a LocusLd"""
    index, count, n11 = _u32(locus_index).reshape(-1), _u32(locus_count).reshape(-1), _u32(n11).reshape(-1)
    if index.size != count.size or n11.size != index.size * max(0, index.size - 1) // 2:
        raise ValueError("one count per locus and one n11 per pair")
    prm = _ld_params(r2_bins, lag_bins, 1, 1)
    o = Ld()
    nb = max(1, min(prm.r2_bins * prm.lag_bins, 16384))
    hist, lag = np.zeros(nb, np.uint64), np.zeros(max(1, min(prm.lag_bins, 32)), np.uint64)
    check(_lib.load().ps_ld_from_counts(_ptr(index), _ptr(count), _ptr(n11), index.size, int(pop_size), C.byref(prm), C.byref(o),
                                        _ptr(hist), _ptr(lag)))
    return LocusLd(o, index, count, hist[:int(o.r2_bins * o.lag_bins)], lag[:int(o.lag_bins)])


__all__ = ["LocusLd", "ld_from_counts", "ld_select_loci"]
