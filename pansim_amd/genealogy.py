"""The recorded genealogy of a run over the C ABI (docs/GENEALOGY.md): the comb that `Simulation.genealogy()` returns with its
host-only read-outs, and the clock histogram over all pairs by (divergence time, distance).

All computation happens in the HIP library; this module only marshals buffers.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import PS_GEN_BEYOND, Clock, ClockParams, GenClusters, Genealogy, check
from .population import _ptr, _u32


def genealogy_pairs(order, coal, r1, r2):
    """the divergence times of the pairs (r1[k], r2[k]) of rows under a comb (ps_genealogy_pairs; host only): uint32, 0 for a
    row with itself, PS_GEN_BEYOND without a common ancestor inside the record"""
    order, coal, r1, r2 = _u32(order), _u32(coal), _u32(r1).reshape(-1), _u32(r2).reshape(-1)
    if r1.size != r2.size:
        raise ValueError("one row of each list per pair")
    t = np.zeros(max(1, r1.size), np.uint32)
    check(_lib.load().ps_genealogy_pairs(_ptr(order), _ptr(coal), order.size, _ptr(r1), _ptr(r2), r1.size, _ptr(t)))
    return t[:r1.size]


def genealogy_pair(order, coal, i, j):
    """the divergence time of rows i and j under a comb (ps_genealogy_pair; host only)"""
    order, coal = _u32(order), _u32(coal)
    t = C.c_uint32()
    check(_lib.load().ps_genealogy_pair(_ptr(order), _ptr(coal), order.size, int(i), int(j), C.byref(t)))
    return t.value


def genealogy_clusters(order, coal, depth, t):
    """the true clusters at look-back t <= depth (ps_genealogy_clusters; host only) -> (labels, dict(clusters, largest,
    within_pairs)); labels[i] = the smallest row that shares row i's ancestor t generations back"""
    order, coal = _u32(order), _u32(coal)
    labels, out = np.zeros(max(1, order.size), np.uint32), GenClusters()
    check(_lib.load().ps_genealogy_clusters(_ptr(order), _ptr(coal), order.size, int(depth), int(t), _ptr(labels), C.byref(out)))
    return labels[:order.size], {name: int(getattr(out, name)) for name, _ in GenClusters._fields_}


def genealogy_newick(order, coal):
    """the trees of a comb as Newick text, one line per root (ps_genealogy_newick; host only)"""
    order, coal = _u32(order), _u32(coal)
    lib, need = _lib.load(), C.c_uint64()
    check(lib.ps_genealogy_newick(_ptr(order), _ptr(coal), order.size, None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    check(lib.ps_genealogy_newick(_ptr(order), _ptr(coal), order.size, buf, need.value, C.byref(need)))
    return buf.value.decode()


class GenealogyResult:
    """The result of `genealogy()` (ps_genealogy_t + the comb): the summary fields as integer attributes, `order` (pop_size
    uint32: the row stored at every internal row) and `coal` (pop_size - 1 uint32: the coalescence time of neighbouring
    internal rows, PS_GEN_BEYOND beyond the record)."""
    FIELDS = tuple(name for name, _ in Genealogy._fields_)

    def __init__(self, g, order, coal):
        for name in self.FIELDS:
            setattr(self, name, int(getattr(g, name)))
        self.order, self.coal = order, coal

    def pair(self, i, j):
        return genealogy_pair(self.order, self.coal, i, j)

    def pairs(self, r1, r2):
        return genealogy_pairs(self.order, self.coal, r1, r2)

    def clusters(self, t):
        return genealogy_clusters(self.order, self.coal, self.depth, t)

    def newick(self):
        return genealogy_newick(self.order, self.coal)

    def restrict(self, rows):
        """the genealogy of the sample `rows` of this generation (ps_genealogy_restrict; host only) -> a GenealogyResult over
        the rows of the handle `subset(rows)` makes: pair(a, b) of the result == pair(rows[a], rows[b]) of this one; pop_size,
        roots and tmrca follow from the restricted comb (docs/GENEALOGY.md), generation, capacity and depth are inherited"""
        from .samples import genealogy_restrict
        order, coal = genealogy_restrict(self.order, self.coal, rows)
        g = Genealogy(**{name: getattr(self, name) for name in self.FIELDS})
        beyond = int((coal == PS_GEN_BEYOND).sum())
        g.pop_size, g.roots, g.tmrca = order.size, 1 + beyond, 0 if beyond or not coal.size else int(coal.max())
        return GenealogyResult(g, order, coal)

    def merges(self):
        """(left, right, height): the comb as a merge list in scipy's numbering, equal times resolved left to right
        (ps_merges_from_genealogy); `tree_parsimony(*merges()[:2])`"""
        from .parsimony import merges_from_genealogy
        return merges_from_genealogy(self.order, self.coal)


def _genealogy_call(fn, pop_size, handle):
    g = Genealogy()
    order, coal = np.zeros(int(pop_size), np.uint32), np.zeros(max(1, int(pop_size) - 1), np.uint32)
    check(fn(handle, C.byref(g), _ptr(order), _ptr(coal)))
    return GenealogyResult(g, order, coal[:int(pop_size) - 1])


class ClockHistogram:
    """The result of `clock_histogram` (ps_clock_t + the arrays): the summary fields as integer attributes, `joint`
    ((time_bins + 1, dist_bins) uint64, the last row the pairs beyond the record) and `per_time` ((time_bins + 1, 3) uint64:
    pairs, sum of num, sum of den of every time row)."""
    FIELDS = tuple(name for name, _ in Clock._fields_)

    def __init__(self, c, joint, per_time):
        for name in self.FIELDS:
            setattr(self, name, int(getattr(c, name)))
        self.joint = joint.reshape(self.time_bins + 1, self.dist_bins)
        self.per_time = per_time.reshape(self.time_bins + 1, 3)

    def mean_distance(self):
        """sum of num / sum of den of every time row (NaN for an empty one)"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.per_time[:, 1].astype(np.float64) / self.per_time[:, 2].astype(np.float64)


def _clock_params(metric, time_bins, dist_bins, time_span, core_max, core_sites, core_span=None):
    if metric not in ("core", "acc"):
        raise ValueError("metric must be \"core\" or \"acc\"")
    prm = ClockParams(_lib.PS_KNN_CORE if metric == "core" else _lib.PS_KNN_ACC, int(time_bins), int(dist_bins), int(time_span or 0), 0)
    if core_span is not None:
        prm.core_span = int(core_span)
    elif core_max is not None:
        if not float(core_max) > 0.0:
            raise ValueError("core_max must be > 0.0")
        prm.core_span = max(1, int(np.ceil(float(core_max) * int(core_sites))))
    return prm


def _clock_call(fn, prm, *head):
    """fn(*head, &params, &summary, joint, per_time) -> ClockHistogram"""
    c = Clock()
    rows = prm.time_bins + 1
    joint, per_time = np.zeros(max(1, rows * prm.dist_bins), np.uint64), np.zeros(3 * rows, np.uint64)      # (the library rejects bad bins itself)
    check(fn(*head, C.byref(prm), C.byref(c), _ptr(joint), _ptr(per_time)))
    return ClockHistogram(c, joint[:rows * prm.dist_bins], per_time)


def clock_from_counts(tmrca, core_h, acc_inter, acc_union, depth, core_sites, core_genes, metric="core", time_bins=32, dist_bins=64,
                      time_span=None, core_max=None, core_span=None):
    """`Simulation.clock_histogram` from any list of pairs with their divergence times (`genealogy().pairs`) and numerators
    (`pairwise_counts`), on the host alone (ps_clock_from_counts; no device).  The numerators of the other metric may be None."""
    t = _u32(tmrca).reshape(-1)
    arrays = [None if a is None else _u32(a).reshape(-1) for a in (core_h, acc_inter, acc_union)]
    if any(a is not None and a.size != t.size for a in arrays):
        raise ValueError("one divergence time and one numerator of each kind per pair")
    prm = _clock_params(metric, time_bins, dist_bins, time_span, core_max, core_sites, core_span)
    return _clock_call(_lib.load().ps_clock_from_counts, prm, _ptr(t), *map(_ptr, arrays), t.size, int(depth), int(core_sites), int(core_genes))


__all__ = ["PS_GEN_BEYOND", "ClockHistogram", "GenealogyResult", "clock_from_counts", "genealogy_clusters", "genealogy_newick", "genealogy_pair",
           "genealogy_pairs"]
