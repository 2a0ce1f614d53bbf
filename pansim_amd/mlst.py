"""Core allele profiles (cgMLST) over the C ABI (docs/ALLELE_PROFILES.md): what `Population.allele_profiles`,
`Simulation.allele_profiles` and `MultiSimulation.allele_profiles` return, and the host-only form.

All computation happens in the HIP library; this module only marshals buffers.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Mlst, MlstParams, check
from .population import _ptr, _u32

MAX_BINS = 16384


class AlleleProfiles:
    """The result of `allele_profiles` (ps_mlst_t + the arrays): the summary fields as attributes (integers; `mean_distance` a
    float), `locus_alleles` (n_loci uint32), `locus_same_pairs` (n_loci uint64), `st` and `complex` (pop_size uint32: the smallest
    output row of the individual's sequence type / clonal complex), `hist` (dist_bins uint64) and `profiles` ((pop_size, n_loci)
    uint16, or None when they were not asked for)."""
    FIELDS = tuple(name for name, _ in Mlst._fields_)
    ARRAYS = ("locus_alleles", "locus_same_pairs", "st", "complex", "hist", "profiles")

    def __init__(self, o, locus_alleles, locus_same_pairs, st, complex_of, hist, profiles):
        for name in self.FIELDS:
            v = getattr(o, name)
            setattr(self, name, float(v) if name == "mean_distance" else int(v))
        self.locus_alleles, self.locus_same_pairs, self.st, self.complex = locus_alleles, locus_same_pairs, st, complex_of
        self.hist, self.profiles = hist[:self.dist_bins], profiles

    def summary(self):
        return {name: getattr(self, name) for name in self.FIELDS}

    def as_dict(self):
        out = self.summary()
        out.update({name: getattr(self, name) for name in self.ARRAYS})
        return out


def _mlst_params(n_loci, dist_bins, complex_max, key_seed, key_bits):
    n_loci = int(n_loci)
    if dist_bins is None:
        dist_bins = min(n_loci + 1, MAX_BINS)
    return MlstParams(n_loci, int(dist_bins), int(complex_max), int(key_bits), int(key_seed))


def _mlst_call(fn, prm, pop_size, want_profiles, *head):
    """fn(*head, &params, *tail) with tail = &summary, locus_alleles, locus_same_pairs, st, complex, hist, profiles -> AlleleProfiles
    (the library rejects bad sizes itself: the arrays only have to be large enough for the call to say so)"""
    n, loci = max(1, int(pop_size)), max(1, int(prm.n_loci))
    o = Mlst()
    locus_alleles, locus_same = np.zeros(loci, np.uint32), np.zeros(loci, np.uint64)
    st, cx = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    hist = np.zeros(max(1, min(int(prm.dist_bins), MAX_BINS)), np.uint64)
    profiles = np.zeros((n, loci), np.uint16) if want_profiles and n * loci <= 1 << 30 else None
    check(fn(*head, C.byref(o), _ptr(locus_alleles), _ptr(locus_same), _ptr(st), _ptr(cx), _ptr(hist), _ptr(profiles)))
    return AlleleProfiles(o, locus_alleles, locus_same, st, cx, hist, profiles)


def _mlst_device_call(fn, handle, pop_size, n_loci, bounds, dist_bins, complex_max, want_profiles, key_seed, key_bits):
    """the device entries: fn(handle, &params, bounds, *tail)"""
    prm = _mlst_params(n_loci, dist_bins, complex_max, key_seed, key_bits)
    if bounds is not None:
        bounds = np.ascontiguousarray(bounds, np.uint64).reshape(-1)
        if bounds.size != int(prm.n_loci) + 1:
            raise ValueError("bounds holds n_loci + 1 sites")
    return _mlst_call(fn, prm, pop_size, want_profiles, handle, C.byref(prm), _ptr(bounds))


def profiles_from_alleles(alleles, dist_bins=None, complex_max=0, want_profiles=True):
    """`allele_profiles` from any (pop_size, n_loci) table of allele ids in output row order, on the host alone
    (ps_profiles_from_alleles; no device): the ids of a locus need not be dense and are renumbered by first appearance -> an
    AlleleProfiles whose core_sites, sites_covered and rounds are 0"""
    a = _u32(alleles)
    if a.ndim != 2:
        raise ValueError("one row of allele ids per individual")
    prm = _mlst_params(a.shape[1], dist_bins, complex_max, 0, 64)
    return _mlst_call(_lib.load().ps_profiles_from_alleles, prm, a.shape[0], want_profiles, _ptr(a), a.shape[0], C.byref(prm))


__all__ = ["AlleleProfiles", "profiles_from_alleles"]
