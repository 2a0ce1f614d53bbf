"""Bootstrap support of the trees over the C ABI (docs/BOOTSTRAP_SUPPORT.md): what `Population.bootstrap_support`,
`Simulation.bootstrap_support` and `MultiSimulation.bootstrap_support` return, the draw rule restated and the counting alone.

All computation happens in the HIP library; this module only marshals buffers.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Bootstrap, BootstrapParams, check
from .population import _MergeCount, _ptr, _Summary, _u32

METHODS = {"linkage": _lib.PS_BOOT_LINKAGE, "upgma": _lib.PS_BOOT_UPGMA, "nj": _lib.PS_BOOT_NJ}


class BootstrapSupport(_Summary):
    """The result of `bootstrap_support` (ps_bootstrap_t + the arrays): the summary fields as integer attributes, the reference
    tree's merge list `left`, `right` (uint32, pop_size - 1: what the method's own call returns), `support` (uint32 per merge: the
    replicates whose tree holds the merge's leaf set -- under "nj" its split) and `shared` (uint32 per replicate: the reference
    merges found in it)."""
    FIELDS = tuple(name for name, _ in Bootstrap._fields_)

    def __init__(self, o, left, right, support, shared):
        self._take(o)
        n = self.merges
        self.left, self.right, self.support, self.shared = left[:n], right[:n], support[:n], shared[:self.replicates]
        # (the number of merges which, called, gives the merge list (left, right) as `tree_parsimony` takes it: `merges()` as
        # on the trees, without renaming the summary field -- UpgmaTree does the same)
        self.merges = _MergeCount(n, self.left, self.right)

    @property
    def fraction(self):
        """support / replicates, float64 per merge"""
        return self.support.astype(np.float64) / np.float64(self.replicates)

    def as_dict(self):
        out = self._head()
        out.update(left=self.left, right=self.right, support=self.support, shared=self.shared, fraction=self.fraction)
        return out


def _method(method):
    if method not in METHODS:
        raise ValueError('method must be "linkage", "upgma" or "nj"')
    return METHODS[method]


def _boot_params(method, replicates, seed, draws):
    return BootstrapParams(_method(method), int(replicates), 0 if draws is None else int(draws), int(seed))


def _boot_call(fn, pop_size, method, replicates, seed, draws, sites, *head):
    """fn(*head, &params, sites, &summary, left, right, support, shared) -> BootstrapSupport"""
    lst = None
    if sites is not None:
        lst = _u32(sites)
        if lst.ndim != 2 or lst.shape[0] != int(replicates) or lst.shape[1] < 1:
            raise ValueError("sites: one row of site indices per replicate")
        if draws is not None and int(draws) != lst.shape[1]:
            raise ValueError("draws is the length of the rows of sites")
        draws = lst.shape[1]
    prm = _boot_params(method, replicates, seed, draws)
    o = Bootstrap()
    n, r = max(1, int(pop_size)), max(1, min(int(replicates), 65535))
    left, right, support, shared = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(r, np.uint32)
    check(fn(*head, C.byref(prm), _ptr(lst), C.byref(o), _ptr(left), _ptr(right), _ptr(support), _ptr(shared)))
    return BootstrapSupport(o, left, right, support, shared)


def bootstrap_sites(seed, replicate, core_sites, draws=None, first=0, count=None):
    """the sites that `bootstrap_support(seed=seed)` draws for replicate `replicate` over `core_sites` sites: the draws [first,
    first + count) of `draws` (None: core_sites; count None: all behind `first`), uint32, on the host alone (ps_bootstrap_sites)"""
    draws = int(core_sites) if draws is None else int(draws)
    count = draws - int(first) if count is None else int(count)
    out = np.zeros(max(1, count), np.uint32)
    check(_lib.load().ps_bootstrap_sites(int(seed), int(replicate), int(core_sites), draws, int(first), count, _ptr(out)))
    return out[:count]


def bootstrap_from_merges(ref_left, ref_right, rep_left, rep_right, pop_size, unrooted=False):
    """the counting of `bootstrap_support` alone, on the host (ps_bootstrap_from_merges): the reference tree's merge list and
    those of the replicates' trees ((replicates, pop_size - 1) each) -> (support, shared), uint32"""
    n = int(pop_size)
    rl, rr = _u32(ref_left).reshape(-1), _u32(ref_right).reshape(-1)
    pl, pr = _u32(rep_left), _u32(rep_right)
    if rl.size != n - 1 or rr.size != n - 1 or pl.shape != pr.shape or pl.ndim != 2 or pl.shape[1] != n - 1:
        raise ValueError("pop_size - 1 merges per tree, one row per replicate")
    support, shared = np.zeros(max(1, n - 1), np.uint32), np.zeros(max(1, pl.shape[0]), np.uint32)
    check(_lib.load().ps_bootstrap_from_merges(_ptr(rl), _ptr(rr), _ptr(pl), _ptr(pr), pl.shape[0], n, int(bool(unrooted)), _ptr(support),
                                               _ptr(shared)))
    return support[:n - 1], shared[:pl.shape[0]]


__all__ = ["BootstrapSupport", "bootstrap_from_merges", "bootstrap_sites"]
