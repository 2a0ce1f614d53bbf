"""The neighbour-joining tree over the C ABI (docs/NEIGHBOUR_JOINING.md): what `Population.neighbour_joining`,
`Simulation.neighbour_joining` and `MultiSimulation.neighbour_joining` return, the host-only form and the Newick text.

All computation happens in the HIP library; this module only marshals buffers and walks the finished list.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Nj, check
from .population import _pair_arrays, _ptr, _Summary, _tree_params, _u32


class NeighbourJoiningTree(_Summary):
    """The result of `neighbour_joining` (ps_nj_t + the joins): the summary fields as integer attributes and the pop_size - 1
    joins in the order performed -- join k creates node pop_size + k (the leaves are the rows), `left`, `right` (uint32) its
    children, left the node with the smaller id, `len_left`, `len_right` (float64) the branches above them, in differing sites
    under the core metric and in the accessory distance's own unit under the other; negative lengths are reported as they are.
    The tree is unrooted: the last join's edge (`len_left` whole, `len_right` 0) is the artefact that makes the list binary."""
    FIELDS = tuple(name for name, _ in Nj._fields_)

    def __init__(self, t, left, right, len_left, len_right):
        self._take(t)
        n = self.joins
        self.left, self.right, self.len_left, self.len_right = left[:n], right[:n], len_left[:n], len_right[:n]

    def merges(self):
        """(left, right): the merge list in the numbering `tree_parsimony` and `parsimony_schedule` take"""
        return self.left, self.right

    @property
    def tree_length(self):
        """the sum of all branch lengths, accumulated from 0.0 join by join, len_left[k] before len_right[k]"""
        total = np.float64(0.0)
        for a, b in zip(self.len_left, self.len_right):
            total = (total + a) + b
        return float(total)

    def patristic(self, r1, r2):
        """float64 per pair: the length of the path between the rows r1[k] and r2[k], summed from r1[k] up to the common
        ancestor and then down to r2[k], in that order -- the tree's own distance of the pair, the counterpart of
        `UpgmaTree.cophenetic`.  A node's number is above its children's, so the lower of the two climbs until they meet."""
        n = self.pop_size
        parent, above = [0] * (n + self.joins), [np.float64(0.0)] * (n + self.joins)
        for k in range(self.joins):
            a, b = int(self.left[k]), int(self.right[k])
            parent[a] = parent[b] = n + k
            above[a], above[b] = self.len_left[k], self.len_right[k]
        r1, r2 = _u32(r1).reshape(-1), _u32(r2).reshape(-1)
        if r1.size != r2.size:
            raise ValueError("two rows per pair")
        out = np.zeros(r1.size, np.float64)
        for k, (a, b) in enumerate(zip(r1.tolist(), r2.tolist())):
            if a >= n or b >= n or a == b:
                raise ValueError("pair %d: two different rows below pop_size" % k)
            up, down = [], []
            while a != b:
                if a < b:
                    up.append(above[a])
                    a = parent[a]
                else:
                    down.append(above[b])
                    b = parent[b]
            total = np.float64(0.0)
            for x in up + down[::-1]:
                total = total + x
            out[k] = total
        return out

    def newick(self):
        """the tree as one line of Newick text in the unrooted form with three subtrees at the top (ps_nj_newick): leaves are rows,
        lengths in substitutions per site under the core metric (len / core_sites) and as they are under the accessory one"""
        scale = self.core_sites if self.metric == _lib.PS_TREE_CORE else 1
        return nj_newick(self.left, self.right, self.len_left, self.len_right, self.pop_size, scale)

    def as_dict(self):
        out = self._head()
        out.update(left=self.left, right=self.right, len_left=self.len_left, len_right=self.len_right, tree_length=self.tree_length)
        return out


def nj_newick(left, right, len_left, len_right, pop_size, scale=1.0):
    """the joins of a neighbour-joining tree as one line of Newick text, every length divided by `scale` (ps_nj_newick; host only)"""
    left, right = _u32(left).reshape(-1), _u32(right).reshape(-1)
    ll, lr = np.ascontiguousarray(len_left, np.float64).reshape(-1), np.ascontiguousarray(len_right, np.float64).reshape(-1)
    if not left.size == right.size == ll.size == lr.size == int(pop_size) - 1:
        raise ValueError("pop_size - 1 joins")
    lib, need = _lib.load(), C.c_uint64()
    check(lib.ps_nj_newick(_ptr(left), _ptr(right), _ptr(ll), _ptr(lr), int(pop_size), float(scale), None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    check(lib.ps_nj_newick(_ptr(left), _ptr(right), _ptr(ll), _ptr(lr), int(pop_size), float(scale), buf, need.value, C.byref(need)))
    return buf.value.decode()


def _nj_call(fn, prm, pop_size, *head):
    """fn(*head, &params, &summary, left, right, len_left, len_right) -> NeighbourJoiningTree"""
    t = Nj()
    n = max(1, int(pop_size))
    left, right = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    len_left, len_right = np.zeros(n, np.float64), np.zeros(n, np.float64)
    check(fn(*head, C.byref(prm), C.byref(t), _ptr(left), _ptr(right), _ptr(len_left), _ptr(len_right)))
    return NeighbourJoiningTree(t, left, right, len_left, len_right)


def nj_from_counts(r1, r2, core_h, acc_inter, acc_union, pop_size, core_sites, core_genes, metric="core"):
    """`Population.neighbour_joining` from the COMPLETE list of pairs (r1, r2), in any order and orientation, and their numerators
    (`pairwise_counts` of both matrices), by the plain O(pop_size^3) loop on the host alone (ps_nj_from_counts; no device).  The
    numerators of the other metric may be None."""
    arrays = _pair_arrays(r1, r2, core_h, acc_inter, acc_union)
    return _nj_call(_lib.load().ps_nj_from_counts, _tree_params(metric), pop_size, *map(_ptr, arrays), arrays[0].size, int(pop_size),
                    int(core_sites), int(core_genes))


__all__ = ["NeighbourJoiningTree", "nj_from_counts", "nj_newick"]
