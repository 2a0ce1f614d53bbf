"""Comparison of two trees over the C ABI (docs/TREE_COMPARISON.md): the result of `tree_compare()`, the host restatement and
the dense ranks of a tree's heights.

All computation happens in the HIP library; this module only marshals buffers.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import TreeCompare, TreeCompareParams, check
from .population import _ptr, _Summary, _u32

DOUBLES = tuple(name for name, kind in TreeCompare._fields_ if kind is C.c_double)


class TreeComparison(_Summary):
    """The result of `tree_compare` (ps_tree_compare_t + the arrays; docs/TREE_COMPARISON.md): the integer summary fields as
    attributes, the doubles `cophenetic_r`, `triplet_recall`, `triplet_precision`, `clade_recall`, `clade_precision`, `joint`
    ((bins_a + 1, bins_b + 1) uint64: the pairs by the bins of their two values, the last row / column the pairs A / B does not
    join), `in_b` (merges_a uint8: the clades of A that B has as well) and `in_a` (merges_b uint8)."""
    FIELDS = tuple(name for name, kind in TreeCompare._fields_ if kind is C.c_uint64)

    def __init__(self, t, joint, in_b, in_a):
        self._take(t)
        for name in DOUBLES:
            setattr(self, name, float(getattr(t, name)))
        self.joint = joint.reshape(self.bins_a + 1, self.bins_b + 1)
        self.in_b, self.in_a = in_b[:self.merges_a], in_a[:self.merges_b]

    def as_dict(self):
        out = self._head(*DOUBLES)
        out.update(joint=self.joint, in_b=self.in_b, in_a=self.in_a)
        return out


def levels_from_heights(num, den):
    """the dense ranks (uint32, from 1) of the non-decreasing heights num[k] / den[k] of a tree's merges under the linkage
    tree's integer comparison, den == 0 above every defined height (ps_levels_from_heights; host only) -- values that
    `tree_compare` takes"""
    num, den = np.ascontiguousarray(num, np.uint64).reshape(-1), np.ascontiguousarray(den, np.uint64).reshape(-1)
    if num.size != den.size:
        raise ValueError("one num and one den per merge")
    levels = np.zeros(max(1, num.size), np.uint32)
    check(_lib.load().ps_levels_from_heights(_ptr(num), _ptr(den), num.size, _ptr(levels), None))
    return levels[:num.size]


def _tree(t, val):
    """(left, right, val or None) of a tree given as a tuple or as one of the three result classes; `val` replaces its values"""
    if isinstance(t, (tuple, list)):
        if len(t) not in (2, 3):
            raise ValueError("a tree is (left, right) or (left, right, val)")
        left, right, own = t[0], t[1], t[2] if len(t) == 3 else None
    elif hasattr(t, "levels"):            # LinkageTree, UpgmaTree
        left, right = t.merges()[:2]
        own = t.levels() if val is None else None
    elif hasattr(t, "merges"):            # GenealogyResult: the coalescence times
        left, right, own = t.merges()
    else:
        raise TypeError("a tree is a (left, right[, val]) tuple, a LinkageTree, an UpgmaTree or a GenealogyResult")
    left, right = _u32(left).reshape(-1), _u32(right).reshape(-1)
    own = own if val is None else val
    own = None if own is None else _u32(own).reshape(-1)
    if left.size != right.size or (own is not None and own.size != left.size):
        raise ValueError("one left, one right and one value per merge")
    return left, right, own


def _compare_call(fn, head, a, b, bins, spans, triplets, values):
    """fn(head, tree a, tree b, &params, &summary, joint, in_b, in_a) -> TreeComparison"""
    va, vb = (None, None) if values is None else values
    la, ra, va = _tree(a, va)
    lb, rb, vb = _tree(b, vb)
    prm = TreeCompareParams(int(bins[0]), int(bins[1]), int(spans[0]), int(spans[1]), int(bool(triplets)))
    # (the library checks the bins before it writes: room for what it accepts)
    joint = np.zeros(min((prm.bins_a + 1) * (prm.bins_b + 1), 16384), np.uint64)
    in_b, in_a = np.zeros(max(1, la.size), np.uint8), np.zeros(max(1, lb.size), np.uint8)
    t = TreeCompare()
    check(fn(head, _ptr(la), _ptr(ra), _ptr(va), la.size, _ptr(lb), _ptr(rb), _ptr(vb), lb.size, C.byref(prm), C.byref(t), _ptr(joint),
             _ptr(in_b), _ptr(in_a)))
    return TreeComparison(t, joint[:(prm.bins_a + 1) * (prm.bins_b + 1)], in_b, in_a)


def tree_compare_from_merges(pop_size, a, b, bins=(32, 32), spans=(0, 0), triplets=True, values=None):
    """`Population.tree_compare` by the plain sequential walk over all pairs on the host alone (ps_tree_compare_from_merges; no
    device)"""
    return _compare_call(_lib.load().ps_tree_compare_from_merges, int(pop_size), a, b, bins, spans, triplets, values)


__all__ = ["TreeComparison", "levels_from_heights", "tree_compare_from_merges"]
