"""Gene-site association over the C ABI (docs/GENE_SITE_ASSOCIATION.md): what `Population.gene_site_ld`,
`Simulation.gene_site_ld` and `MultiSimulation.gene_site_ld` return, and the host-only restatement.

All computation happens in the HIP library; this module only marshals buffers.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import PS_GS_NONE, Gs, GsParams, GsSide, check
from .population import _ptr, _u32

SIDE_ARRAYS = ("index", "count", "best", "best_q", "strong", "best_sign")


class _Side:
    """the six arrays of one side and the ps_gs_side that points at them"""

    def __init__(self, room):
        room = max(1, int(room))
        self.arrays = {name: np.zeros(room, np.int32 if name == "best_sign" else np.uint32) for name in SIDE_ARRAYS}
        self.c = GsSide(*(a.ctypes.data for a in self.arrays.values()))


class GeneSiteLd:
    """The result of `gene_site_ld` (ps_gs_t + the arrays): the summary fields as attributes (integers; `mean_r2` a float), `hist`
    ((freq_bins, r2_bins) uint64), `freq_sum_q` (freq_bins uint64) and per side -- `site_` over the `sites` sites, `gene_` over
    the `genes` genes -- `index` (the column), `count` (its ones), `best_gene` / `best_site` (the column of the best tag, or
    PS_GS_NONE), `best_q`, `best_sign` (int32) and `strong` (its pairs with q >= strong_q)."""
    FIELDS = tuple(name for name, _ in Gs._fields_)
    NONE = PS_GS_NONE

    def __init__(self, o, site, gene, hist, freq_sum_q):
        for name in self.FIELDS:
            v = getattr(o, name)
            setattr(self, name, float(v) if name == "mean_r2" else int(v))
        for side, other, M, arrays in (("site", "gene", self.sites, site.arrays), ("gene", "site", self.genes, gene.arrays)):
            for name in SIDE_ARRAYS:
                setattr(self, "%s_%s" % (side, "best_" + other if name == "best" else name), arrays[name][:M])
        self.hist = hist.reshape(self.freq_bins, self.r2_bins)
        self.freq_sum_q = freq_sum_q

    def summary(self):
        return {name: getattr(self, name) for name in self.FIELDS}

    def as_dict(self):
        out = self.summary()
        out["hist"], out["freq_sum_q"] = self.hist, self.freq_sum_q
        for side, other in (("site", "gene"), ("gene", "site")):
            for name in ("index", "count", "best_" + other, "best_q", "strong", "best_sign"):
                out["%s_%s" % (side, name)] = getattr(self, "%s_%s" % (side, name))
        return out


def _gs_params(r2_bins, freq_bins, site_min_minor, gene_min_minor, max_sites, max_genes, strong_q):
    return GsParams(int(r2_bins), int(freq_bins), int(site_min_minor), int(gene_min_minor), int(max_sites), int(max_genes), int(strong_q))


def _bins(prm):
    """room for the bins and the frequency sums (the library rejects bad bins itself)"""
    nb = max(1, min(int(prm.r2_bins) * int(prm.freq_bins), 16384))
    return np.zeros(nb, np.uint64), np.zeros(max(1, min(int(prm.freq_bins), 16384)), np.uint64)


def _gs_call(fn, prm, sites, genes, *head):
    """fn(*head, &params, sites, n_sites, genes, n_genes, &summary, &site side, &gene side, hist, freq_sum_q) -> GeneSiteLd"""
    o = Gs()
    ls = None if sites is None else _u32(sites).reshape(-1)
    lg = None if genes is None else _u32(genes).reshape(-1)
    site = _Side(min(int(prm.max_sites), 65536) if ls is None else ls.size)
    gene = _Side(min(int(prm.max_genes), 65536) if lg is None else lg.size)
    hist, freq = _bins(prm)
    check(fn(*head, C.byref(prm), _ptr(ls), 0 if ls is None else ls.size, _ptr(lg), 0 if lg is None else lg.size, C.byref(o), C.byref(site.c),
             C.byref(gene.c), _ptr(hist), _ptr(freq)))
    return GeneSiteLd(o, site, gene, hist[:int(o.r2_bins * o.freq_bins)], freq[:int(o.freq_bins)])


def gene_site_from_counts(site_index, site_count, gene_index, gene_count, n11, pop_size, r2_bins=64, freq_bins=1, strong_q=32768):
    """`gene_site_ld` from the columns and ones of Ms sites and Mg genes and n11 of their pairs, (Mg, Ms) row-major, on the host
    alone (ps_gene_site_from_counts; no device) -> a GeneSiteLd whose columns and candidates are 0"""
    si, sc, gi, gc = (_u32(a).reshape(-1) for a in (site_index, site_count, gene_index, gene_count))
    n11 = _u32(n11).reshape(-1)
    if si.size != sc.size or gi.size != gc.size or n11.size != si.size * gi.size:
        raise ValueError("one count per locus and one n11 per (gene, site) pair")
    prm = _gs_params(r2_bins, freq_bins, 1, 1, 1, 1, strong_q)
    o, site, gene = Gs(), _Side(si.size), _Side(gi.size)
    site.arrays["index"][:si.size], site.arrays["count"][:si.size] = si, sc
    gene.arrays["index"][:gi.size], gene.arrays["count"][:gi.size] = gi, gc
    hist, freq = _bins(prm)
    check(_lib.load().ps_gene_site_from_counts(_ptr(si), _ptr(sc), si.size, _ptr(gi), _ptr(gc), gi.size, _ptr(n11), int(pop_size), C.byref(prm),
                                               C.byref(o), C.byref(site.c), C.byref(gene.c), _ptr(hist), _ptr(freq)))
    return GeneSiteLd(o, site, gene, hist[:int(o.r2_bins * o.freq_bins)], freq[:int(o.freq_bins)])


__all__ = ["GeneSiteLd", "gene_site_from_counts"]
