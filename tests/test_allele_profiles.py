"""Core allele profiles without a device (docs/ALLELE_PROFILES.md): the host-only ps_profiles_from_alleles against the plain
restatement (tests/allele_profiles_ref.py) on random tables of allele ids, the identities between its results, permutations of
the individuals, every PS_ERR_INVALID limit, the no-device error of the device entries, the bindings and the two run classes.
The device half is tests/test_gpu_allele_profiles.py.  Every comparison is an equality of integers; the one double is compared
bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import allele_profiles_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS_ERR_INVALID, PS_ERR_NO_DEVICE = -1, -2
NEW_SYMBOLS = ("ps_allele_profiles", "ps_sim_allele_profiles", "ps_multi_allele_profiles", "ps_profiles_from_alleles",
               "ps_allele_profiles_timing")
SHAPES = [(2, 1), (7, 30), (64, 5), (65, 257), (1000, 40)]


def _table(rng, N, M):
    """ids that are not dense: a few founders' profiles, copied and changed at a few loci, so that alleles, sequence types and
    complexes are shared; the values of a locus are drawn from all of u32"""
    founders = min(N, 4)
    ids = rng.integers(0, 1 << 32, (N, M), dtype=np.uint64).astype(np.uint32)
    for k in range(founders, N):
        ids[k] = ids[rng.integers(k)]
        loci = rng.choice(M, min(M, int(rng.integers(0, 3))), replace=False)
        ids[k, loci] = rng.integers(0, 1 << 32, loci.size, dtype=np.uint64).astype(np.uint32)
    return ids[rng.permutation(N)]


def _cases(M):
    return sorted({1, 2, 7, M + 1}), sorted({0, 1, M})


@pytest.fixture(scope="module")
def tables():
    return {(N, M): _table(np.random.default_rng(N + M), N, M) for N, M in SHAPES}


@pytest.mark.parametrize("N,M", SHAPES)
def test_from_alleles_equals_the_restatement(pa, tables, N, M):
    ids = tables[N, M]
    bins, maxes = _cases(M)
    for k, dist_bins in enumerate(bins):
        complex_max = maxes[k % len(maxes)]
        got = pa.profiles_from_alleles(ids, dist_bins=dist_bins, complex_max=complex_max)
        ref.assert_equal(got, ref.from_ids(ids, dist_bins=dist_bins, complex_max=complex_max), rounds=0)
    for complex_max in maxes:
        got = pa.profiles_from_alleles(ids, complex_max=complex_max, want_profiles=False)
        assert got.profiles is None and got.dist_bins == M + 1
        ref.assert_equal(got, ref.from_ids(ids, complex_max=complex_max), rounds=0)
    if N >= 64:
        assert 1 < got.sequence_types < N and got.identical_pairs > 0


@pytest.mark.parametrize("N,M", SHAPES)
def test_identities(pa, tables, N, M):
    ids = tables[N, M]
    zero, one, all_ = (pa.profiles_from_alleles(ids, complex_max=c) for c in (0, min(1, M), M))
    for got in (zero, one, all_):
        assert int(got.hist.sum()) == got.pairs == N * (N - 1) // 2
        assert got.sum_d == sum(got.pairs - int(s) for s in got.locus_same_pairs)
        sizes = np.bincount(got.st)
        assert got.identical_pairs == int((sizes * (sizes - 1) // 2).sum())
        assert got.alleles_total == int(got.locus_alleles.sum()) and got.max_alleles == int(got.locus_alleles.max())
        assert np.array_equal(got.profiles.max(0) + 1, got.locus_alleles)
    assert np.array_equal(zero.complex, zero.st) and zero.complexes == zero.sequence_types and zero.edges == zero.identical_pairs
    assert all_.complexes == 1 and all_.largest_complex == N and not all_.complex.any() and all_.edges == all_.pairs
    assert zero.complexes >= one.complexes >= 1 and zero.edges <= one.edges


@pytest.mark.parametrize("N,M", [(7, 30), (65, 257)])
def test_a_permutation_of_the_individuals_permutes_the_partitions(pa, tables, N, M):
    ids = tables[N, M]
    perm = np.random.default_rng(5).permutation(N)
    a, b = pa.profiles_from_alleles(ids, complex_max=1), pa.profiles_from_alleles(ids[perm], complex_max=1)
    assert {k: v for k, v in a.summary().items()} == {k: v for k, v in b.summary().items()}
    assert np.array_equal(a.hist, b.hist) and np.array_equal(a.locus_alleles, b.locus_alleles)
    assert np.array_equal(a.locus_same_pairs, b.locus_same_pairs)
    for name in ("st", "complex"):
        x, y = getattr(a, name)[perm], getattr(b, name)              # (the labels of the same individuals, in b's order)
        assert np.array_equal(x[:, None] == x[None, :], y[:, None] == y[None, :]), name
        assert np.array_equal(y, np.array([np.flatnonzero(y == v)[0] for v in y])), name       # the smallest row of the class


def _call(pa, fn, *args):
    rc = fn(*args)
    return rc, pa.load().ps_last_error().decode()


def test_limits_name_their_field(pa):
    lib = pa.load()
    o = pa._lib.Mlst()
    P = pa._lib.MlstParams
    big = np.zeros(1 << 16, np.uint64)

    def from_alleles(prm, N=4):
        ids = np.zeros(max(1, min(N, 8) * max(1, min(int(prm.n_loci), 8))), np.uint32)
        return _call(pa, lib.ps_profiles_from_alleles, ids.ctypes.data, N, C.byref(prm), C.byref(o), big.ctypes.data, big.ctypes.data, big.ctypes.data,
                     big.ctypes.data, big.ctypes.data, None)

    assert from_alleles(P(2, 3, 0, 64, 0))[0] == 0 and from_alleles(P(2, 1, 2, 1, 9))[0] == 0
    for prm, N, word in ((P(0, 1, 0, 64, 0), 4, "n_loci"), (P(65536, 1, 0, 64, 0), 4, "n_loci"), (P(16385, 1, 0, 64, 0), 65536, "n_loci x pop_size"),
                         (P(2, 0, 0, 64, 0), 4, "dist_bins"), (P(2, 16385, 0, 64, 0), 4, "dist_bins"), (P(2, 3, 3, 64, 0), 4, "complex_max"),
                         (P(2, 3, 0, 0, 0), 4, "key_bits"), (P(2, 3, 0, 65, 0), 4, "key_bits"), (P(2, 3, 0, 64, 0), 1, "pop_size"),
                         (P(2, 3, 0, 64, 0), 65537, "pop_size")):
        rc, msg = from_alleles(prm, N)
        assert rc == PS_ERR_INVALID and word in msg, (word, msg)
    rc, msg = _call(pa, lib.ps_profiles_from_alleles, None, 4, C.byref(P(2, 3, 0, 64, 0)), C.byref(o), None, None, None, None, None, None)
    assert rc == PS_ERR_INVALID and "null" in msg
    assert lib.ps_allele_profiles_timing(None, None, None, None, None, None) == PS_ERR_INVALID
    with pytest.raises(ValueError):
        pa.profiles_from_alleles(np.zeros(5, np.uint32))


def test_the_device_entries_need_a_device(pa):
    """without a device the device entries fail with PS_ERR_NO_DEVICE before they look at their arguments; with one, the same
    calls refuse their null handles"""
    lib = pa.load()
    o, prm = pa._lib.Mlst(), pa._lib.MlstParams(4, 5, 0, 64, 0)
    b = np.zeros(64, np.uint64)
    want = PS_ERR_NO_DEVICE if lib.ps_device_count() <= 0 else PS_ERR_INVALID
    tail = (C.byref(prm), None, C.byref(o), b.ctypes.data, b.ctypes.data, b.ctypes.data, b.ctypes.data, b.ctypes.data, None)
    for fn in (lib.ps_allele_profiles, lib.ps_sim_allele_profiles, lib.ps_multi_allele_profiles):
        assert fn(None, *tail) == want
    if want == PS_ERR_NO_DEVICE:
        assert "no HIP device" in lib.ps_last_error().decode()
        bad = pa._lib.MlstParams(0, 0, 0, 0, 0)                  # ... and before the parameters
        tail = (C.byref(bad), None, C.byref(o), None, None, None, None, None, None)
        for fn in (lib.ps_allele_profiles, lib.ps_sim_allele_profiles, lib.ps_multi_allele_profiles):
            assert fn(None, *tail) == PS_ERR_NO_DEVICE


def test_abi_header_and_bindings_agree(pa):
    lib = pa.load()
    hdr = open(os.path.join(ROOT, "include", "pansim_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in pa._lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
    assert lib.ps_abi_version() == 3
    for struct, cls in (("ps_mlst_params", pa._lib.MlstParams), ("ps_mlst_t", pa._lib.Mlst)):
        fields = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1)
        assert re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S)) == [n for n, _ in cls._fields_], struct
    assert C.sizeof(pa._lib.MlstParams) == 24 and C.sizeof(pa._lib.Mlst) == 22 * 8
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert "fn %s(" % name in integration, name
    assert os.path.exists(os.path.join(ROOT, "docs", "ALLELE_PROFILES.md"))
    assert pa.AlleleProfiles is pa.mlst.AlleleProfiles and pa.profiles_from_alleles is pa.mlst.profiles_from_alleles
    assert b"mlst_band" in [lib.ps_tuning_key(k) for k in range(64)] and '"mlst_band"' in hdr


def test_both_run_classes_ask_for_their_own_entry(pa):
    """written once beside _Readouts, not in it; no device: the library is an object that notes the first symbol asked for"""
    from pansim_amd import _lib, simulation

    class Asked(Exception):
        pass

    class Library:
        def __getattr__(self, name):
            raise Asked(name)

    assert "allele_profiles" not in vars(simulation._Readouts) and "allele_profiles" not in vars(simulation._Associations)
    for cls, symbol in ((pa.Simulation, "ps_sim_allele_profiles"), (pa.MultiSimulation, "ps_multi_allele_profiles")):
        assert hasattr(cls, "allele_profiles") and "allele_profiles" not in vars(cls)
        run = object.__new__(cls)
        run._lib, run._h, run.generation = Library(), None, 0
        run.params = _lib.SimParams(pop_size=8, core_size=100, pan_genes=60, core_genes=20, max_distances=10)
        with pytest.raises(Asked) as e:
            run.allele_profiles(n_loci=5)
        assert str(e.value) == symbol and symbol in _lib.SIGNATURES
