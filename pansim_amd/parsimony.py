"""Parsimony of the two matrices on a tree over the C ABI (docs/TREE_PARSIMONY.md): the result of `tree_parsimony()`, the merge
lists of the three trees the package builds, the level schedule and the host restatement.

All computation happens in the HIP library; this module only marshals buffers.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import PS_PARS_BINS, PS_PARS_MAX_POP, Parsimony, check
from .population import _ptr, _Summary, _u32, fmt_f64


def _merge_list(left, right):
    left, right = _u32(left).reshape(-1), _u32(right).reshape(-1)
    if left.size != right.size:
        raise ValueError("one left and one right child per merge")
    return left, right


class TreeParsimony(_Summary):
    """The result of `tree_parsimony` (ps_parsimony_t + the arrays; docs/TREE_PARSIMONY.md): the integer summary fields as
    attributes, `ci`, the merge list `left`, `right` it was computed on, `site_hist` (64 uint64: sites by their changes) and,
    when asked for, `site_changes` (sites uint32), `branch_changes` (pop_size + merges uint64: the core sites that change on
    the branch above every node), `gene_changes`, `gene_gains`, `gene_losses` (genes uint32), `branch_gains`, `branch_losses`
    (pop_size + merges uint64).  What was not asked for is None."""
    FIELDS = tuple(name for name, kind in Parsimony._fields_ if kind is C.c_uint64)
    ARRAYS = ("site_changes", "site_hist", "branch_changes", "gene_changes", "gene_gains", "gene_losses", "branch_gains", "branch_losses")

    def __init__(self, p, left, right, **arrays):
        self._take(p)
        self.ci = float(p.ci)
        self.left, self.right = left, right
        for name in self.ARRAYS:
            setattr(self, name, arrays.get(name))

    @property
    def parent(self):
        """pop_size + merges int64: the node every node was merged into, -1 for a root"""
        out = np.full(self.pop_size + self.merges, -1, np.int64)
        k = np.arange(self.merges, dtype=np.int64) + self.pop_size
        out[self.left], out[self.right] = k, k
        return out

    def branch_length(self):
        """pop_size + merges float64 (needs branches): changes per site on the branch above every node, 0.0 for a root"""
        if self.branch_changes is None:
            raise ValueError("branch_length needs branches=True")
        return self.branch_changes.astype(np.float64) / float(self.sites) if self.sites else np.zeros(self.branch_changes.size)

    def newick(self, order=None):
        """the trees as Newick text (needs branches), one line per internal root in ascending node order, children as
        (left:len,right:len) with branch lengths in changes per site; leaf k is written as order[k] (None: k)"""
        n, parent, length = self.pop_size, self.parent, self.branch_length()
        names = [str(k) for k in range(n)] if order is None else [str(x) for x in order]
        if len(names) != n:
            raise ValueError("one name per leaf")
        out = []
        for root in range(n, n + self.merges):
            if parent[root] >= 0:
                continue
            stack = [(True, root)]
            while stack:
                is_node, x = stack.pop()
                if not is_node:
                    out.append(x)
                    continue
                tail = ":" + fmt_f64(length[x]) if parent[x] >= 0 else ""
                if x < n:
                    out.append(names[x] + tail)
                else:
                    out.append("(")
                    stack += [(False, ")" + tail), (True, int(self.right[x - n])), (False, ","), (True, int(self.left[x - n]))]
            out.append(";\n")
        return "".join(out)

    def as_dict(self):
        out = self._head("ci")
        out.update(left=self.left, right=self.right, parent=self.parent)
        out.update({name: getattr(self, name) for name in self.ARRAYS})
        return out


def _outputs(nodes, sites, genes, per_site, branches, with_genes):
    """the eight optional arrays of a call in the order of the C entries (None: not asked for)"""
    u32, u64 = (lambda n: np.zeros(max(1, int(n)), np.uint32)), (lambda n: np.zeros(max(1, int(n)), np.uint64))
    return dict(site_changes=u32(sites) if per_site else None, site_hist=u64(PS_PARS_BINS), branch_changes=u64(nodes) if branches else None,
                gene_changes=u32(genes) if with_genes else None, gene_gains=u32(genes) if with_genes else None,
                gene_losses=u32(genes) if with_genes else None, branch_gains=u64(nodes) if with_genes and branches else None,
                branch_losses=u64(nodes) if with_genes and branches else None)


def _pars_call(fn, left, right, pop_size, sites, genes, per_site, branches, with_genes, *head):
    """fn(*head, left, right, merges, &summary, the eight arrays) -> TreeParsimony"""
    left, right = _merge_list(left, right)
    N, M = int(pop_size), left.size
    a = _outputs(N + M, sites, genes, per_site, branches, with_genes)
    p = Parsimony()
    check(fn(*head, _ptr(left), _ptr(right), M, C.byref(p), *[_ptr(a[name]) for name in TreeParsimony.ARRAYS]))
    for name, n in (("site_changes", sites), ("gene_changes", genes), ("gene_gains", genes), ("gene_losses", genes)):
        if a[name] is not None:
            a[name] = a[name][:int(n)]
    return TreeParsimony(p, left, right, **a)


def parsimony_from_rows(rows, left, right, genes=False, per_site=True, branches=True):
    """`Population.tree_parsimony` of an individual-major (pop_size, cols) uint8 matrix by the sequential algorithm on the host
    alone (ps_parsimony_from_rows; no device).  `genes`: the bytes are presences (0 / non-zero) of accessory genes and the gene
    outputs are filled; else they are core cells and the core outputs are."""
    rows = np.ascontiguousarray(rows, np.uint8)
    if rows.ndim != 2:
        raise ValueError("rows must be (pop_size, cols)")
    left, right = _merge_list(left, right)
    N, cols, M = rows.shape[0], rows.shape[1], left.size
    if genes:
        a = _outputs(N + M, 0, cols, False, branches, True)
        a["site_hist"] = a["branch_changes"] = None
        if not branches:
            a["gene_gains"] = a["gene_losses"] = None
    else:
        a = _outputs(N + M, cols, 0, per_site, branches, False)
    p = Parsimony()
    check(_lib.load().ps_parsimony_from_rows(_ptr(rows), N, cols, int(bool(genes)), _ptr(left), _ptr(right), M, C.byref(p),
                                             *[_ptr(a[name]) for name in TreeParsimony.ARRAYS]))
    for name in ("site_changes", "gene_changes", "gene_gains", "gene_losses"):
        if a[name] is not None:
            a[name] = a[name][:cols]
    return TreeParsimony(p, left, right, **a)


def merges_from_tree(lo, hi, pop_size):
    """the merge list (left, right) of a linkage tree's edges in their given order (ps_merges_from_tree; host only): merge k
    joins the clusters of edge k, left the one with the smaller smallest row; nodes in scipy's numbering"""
    lo, hi = _merge_list(lo, hi)
    left, right = np.zeros(max(1, lo.size), np.uint32), np.zeros(max(1, lo.size), np.uint32)
    m = C.c_uint64()
    check(_lib.load().ps_merges_from_tree(_ptr(lo), _ptr(hi), lo.size, int(pop_size), _ptr(left), _ptr(right), C.byref(m)))
    return left[:m.value], right[:m.value]


def merges_from_genealogy(order, coal):
    """the merge list (left, right, height) of a comb (ps_merges_from_genealogy; host only): the positions inside the record in
    (time, position) order, left the left interval, leaves the rows order[r]; equal times are resolved left to right"""
    order, coal = _u32(order).reshape(-1), _u32(coal).reshape(-1)
    if coal.size != max(0, order.size - 1):
        raise ValueError("pop_size rows and pop_size - 1 times")
    n = max(1, order.size)
    left, right, height = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    m = C.c_uint64()
    check(_lib.load().ps_merges_from_genealogy(_ptr(order), _ptr(coal), order.size, _ptr(left), _ptr(right), _ptr(height), C.byref(m)))
    return left[:m.value], right[:m.value], height[:m.value]


def parsimony_schedule(left, right, pop_size):
    """(level_of, levels) of a merge list (ps_parsimony_schedule; host only): the level of a merge is 1 + the larger of its
    children's, leaves at 0 -- the order the kernel runs the merges in"""
    left, right = _merge_list(left, right)
    level_of, levels = np.zeros(max(1, left.size), np.uint32), C.c_uint32()
    check(_lib.load().ps_parsimony_schedule(_ptr(left), _ptr(right), left.size, int(pop_size), _ptr(level_of), C.byref(levels)))
    return level_of[:left.size], levels.value


__all__ = ["PS_PARS_BINS", "PS_PARS_MAX_POP", "TreeParsimony", "merges_from_genealogy", "merges_from_tree", "parsimony_from_rows",
           "parsimony_schedule"]
