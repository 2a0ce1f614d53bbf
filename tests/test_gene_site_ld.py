"""Gene-site association without a device (docs/GENE_SITE_ASSOCIATION.md): the host-only ps_gene_site_from_counts against the
plain restatement (tests/gene_site_ref.py) on random tables, the rounding traps of q at N = 65536, ties of the best tags, every
PS_ERR_INVALID limit, the no-device error of the device entries, the bindings and the two run classes.  The device half is
tests/test_gpu_gene_site_ld.py.  Every comparison is an equality of integers; the one double is compared bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gene_site_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS_ERR_INVALID, PS_ERR_NO_DEVICE = -1, -2
NEW_SYMBOLS = ("ps_gene_site_ld", "ps_sim_gene_site_ld", "ps_multi_gene_site_ld", "ps_gene_site_from_counts", "ps_gene_site_ld_timing")


def _from_rows(pa, Xs, Xg, site_index=None, gene_index=None, **kw):
    """ps_gene_site_from_counts on explicit indicator rows -> (result, reference)"""
    Xs, Xg = np.asarray(Xs, np.int64), np.asarray(Xg, np.int64)
    N = Xs.shape[1]
    site_index = list(range(Xs.shape[0])) if site_index is None else site_index
    gene_index = list(range(Xg.shape[0])) if gene_index is None else gene_index
    sc, gc = Xs.sum(1), Xg.sum(1)
    n11 = Xg @ Xs.T
    got = pa.gene_site_from_counts(site_index, sc, gene_index, gc, n11, N, **kw)
    want = ref.from_counts(site_index, sc, gene_index, gc, lambda a, b: n11[a, b], N, **kw)
    return got, want


def _table(rng, N, M, mono=True):
    """M indicator rows over N individuals that share the structure of four base rows; with two monomorphic rows"""
    base = rng.random((4, N)) < 0.5
    X = np.array([base[rng.integers(4)] ^ (rng.random(N) < rng.choice([0.0, 0.02, 0.3])) for _ in range(M)], np.uint8)
    if mono and M >= 2:
        X[rng.integers(M)] = 0
        X[rng.integers(M)] = 1
    return X


@pytest.mark.parametrize("N,Ms,Mg,r2_bins,freq_bins,strong_q", [(2, 5, 4, 1, 1, 32768), (7, 30, 11, 64, 5, 1), (64, 40, 25, 7, 64, 65536),
                                                               (65, 25, 40, 512, 5, 32768), (1000, 12, 17, 256, 64, 20000)])
def test_from_counts_equals_the_restatement(pa, N, Ms, Mg, r2_bins, freq_bins, strong_q):
    rng = np.random.default_rng(N + Ms)
    Xs, Xg = _table(rng, N, Ms), _table(rng, N, Mg)
    Xg[0] = Xs[3]                        # (a copy and a complement, unless the draw made site 3 monomorphic)
    Xg[1] = 1 - Xs[3]
    si = np.sort(rng.choice(1 << 20, Ms, replace=False)).tolist()
    gi = np.sort(rng.choice(1 << 20, Mg, replace=False)).tolist()
    got, want = _from_rows(pa, Xs, Xg, si, gi, r2_bins=r2_bins, freq_bins=freq_bins, strong_q=strong_q)
    ref.assert_equal(got, want)
    assert got.pairs == got.defined_pairs + got.undefined_pairs == Ms * Mg
    assert got.undefined_pairs > 0 and got.site_columns == got.gene_columns == got.site_candidates == got.gene_candidates == 0
    assert got.hist.shape == (freq_bins, r2_bins) and int(got.hist.sum()) == got.defined_pairs and int(got.freq_sum_q.sum()) == got.sum_q
    d = got.as_dict()
    assert set(ref.FIELDS) <= set(d) and sum(k.startswith(("site_", "gene_")) and isinstance(d[k], np.ndarray) for k in d) == 12


def test_counts_near_the_ends_at_65536_individuals(pa):
    """N = 65536 with counts near 1, N / 2 and N - 1: the rounding traps of ps_ld_pair's f64 estimate; n11 drawn from what the
    two counts allow"""
    N = 65536
    rng = np.random.default_rng(65536)
    pool = [1, 2, 3, 32767, 32768, 32769, 65533, 65534, 65535, 16384, 49152, 0, N]
    sc, gc = rng.choice(pool, 40), rng.choice(pool, 30)
    n11 = np.array([[rng.integers(max(0, g + s - N), min(g, s) + 1) for s in sc] for g in gc], np.int64)
    n11[:, 0], n11[0, :] = np.maximum(0, gc + sc[0] - N), np.minimum(gc[0], sc)        # (the two ends of the allowed range)
    for freq_bins in (1, 5, 64):
        kw = dict(r2_bins=128, freq_bins=freq_bins, strong_q=65536)
        got = pa.gene_site_from_counts(np.arange(40), sc, np.arange(30), gc, n11, N, **kw)
        ref.assert_equal(got, ref.from_counts(list(range(40)), sc, list(range(30)), gc, lambda a, b: n11[a, b], N, **kw))
    assert got.defined_pairs > 500 and got.undefined_pairs > 0


def test_empty_sides(pa):
    """Ms = 0 or Mg = 0 is not an error: no pairs, every integer 0, the other side's loci without a tag"""
    X = _table(np.random.default_rng(3), 20, 6, mono=False)
    for Xs, Xg in ((X[:0], X), (X, X[:0]), (X[:0], X[:0])):
        got, want = _from_rows(pa, Xs, Xg)
        ref.assert_equal(got, want)
        assert got.pairs == got.defined_pairs == got.undefined_pairs == got.sum_q == got.genes_tagged == got.sites_tagging == 0
        assert got.mean_r2 == 0.0 and not got.hist.any()
        assert (got.gene_best_site == ref.NONE).all() and (got.site_best_gene == ref.NONE).all()
        assert not got.gene_best_q.any() and not got.site_best_sign.any()


def test_ties_go_to_the_lowest_column_and_q_zero_still_reports(pa):
    rows = {"a": "11110000", "b": "11001100", "not_a": "00001111", "mono": "11111111", "c": "11100000"}
    bits = lambda *names: np.array([[int(ch) for ch in rows[n]] for n in names], np.uint8)      # noqa: E731
    # sites 10 and 30 equal, 20 their complement: all three have q = 65536 with gene `a`; the lowest column wins, its sign counts
    got, want = _from_rows(pa, bits("not_a", "a", "a", "mono"), bits("a", "b", "mono"), [10, 20, 30, 40], [5, 6, 7])
    ref.assert_equal(got, want)
    assert got.gene_best_site.tolist() == [10, 10, ref.NONE] and got.gene_best_q.tolist() == [65536, 0, 0]
    assert got.gene_best_sign.tolist() == [-1, 0, 0]
    # gene `b` is independent of every site (q = 0): it still reports its lowest defined site, and tags nothing
    assert got.gene_strong.tolist() == [3, 0, 0] and got.genes_tagged == 1 and got.sites_tagging == 3
    assert got.site_best_gene.tolist() == [5, 5, 5, ref.NONE] and got.site_best_sign.tolist() == [-1, 1, 1, 0]
    assert got.complete_pairs == 3 and got.strong_pairs == 3 and got.undefined_pairs == 3 + 4 - 1
    # two identical genes: the site reports the lower one; a monomorphic site in front does not shift the tie
    got, want = _from_rows(pa, bits("mono", "c", "a"), bits("b", "a", "a"), [1, 2, 3], [100, 200, 300])
    ref.assert_equal(got, want)
    assert got.site_best_gene.tolist() == [ref.NONE, 200, 200] and got.site_best_q[2] == 65536
    assert got.gene_best_site.tolist() == [2, 3, 3]
    # strong_q = 1 counts every pair with q > 0; 65536 only the complete ones
    Xs, Xg = bits("c", "a", "b"), bits("a", "not_a", "c")
    qs = [ref.pair_q(8, int(g.sum()), int(s.sum()), int((g & s).sum()))[1] for g in Xg for s in Xs]
    for strong_q, n in ((1, sum(q > 0 for q in qs)), (65536, sum(q == 65536 for q in qs))):
        got, want = _from_rows(pa, Xs, Xg, strong_q=strong_q)
        ref.assert_equal(got, want)
        assert got.strong_pairs == n > 0


def _call(pa, fn, *args):
    rc = fn(*args)
    return rc, pa.load().ps_last_error().decode()


def test_invalid_arguments(pa):
    lib = pa.load()
    o = pa._lib.Gs()
    hist, freq = np.zeros(16384, np.uint64), np.zeros(16384, np.uint64)
    si, sc = np.array([0, 3, 9], np.uint32), np.array([2, 2, 2], np.uint32)
    gi, gc = np.array([1, 4], np.uint32), np.array([2, 1], np.uint32)
    n11 = np.array([1, 1, 1, 0, 1, 1], np.uint32)

    def from_counts(prm, si=si, sc=sc, gi=gi, gc=gc, n11=n11, N=4, n_sites=None, n_genes=None):
        return _call(pa, lib.ps_gene_site_from_counts, si.ctypes.data, sc.ctypes.data, si.size if n_sites is None else n_sites, gi.ctypes.data,
                     gc.ctypes.data, gi.size if n_genes is None else n_genes, n11.ctypes.data, N, C.byref(prm), C.byref(o), None, None,
                     hist.ctypes.data, freq.ctypes.data)

    P = pa._lib.GsParams
    assert from_counts(P(64, 1, 1, 1, 1, 1, 32768))[0] == 0
    for r2, fb, sq, word in ((0, 1, 1, "r2_bins"), (4, 0, 1, "freq_bins"), (16385, 1, 1, "exceeds"), (1024, 32, 1, "exceeds"), (4, 4, 0, "strong_q"),
                             (4, 4, 65537, "strong_q")):
        rc, msg = from_counts(P(r2, fb, 1, 1, 1, 1, sq))
        assert rc == PS_ERR_INVALID and word in msg, (r2, fb, sq, msg)
    prm = P(8, 2, 1, 1, 1, 1, 32768)
    for bad in ([0, 3, 3], [5, 3, 9]):
        rc, msg = from_counts(prm, si=np.array(bad, np.uint32))
        assert rc == PS_ERR_INVALID and "strictly ascending" in msg and "site" in msg
    rc, msg = from_counts(prm, gi=np.array([4, 4], np.uint32))
    assert rc == PS_ERR_INVALID and "strictly ascending" in msg and "gene" in msg
    rc, msg = from_counts(prm, sc=np.array([2, 5, 2], np.uint32))
    assert rc == PS_ERR_INVALID and "ones among" in msg
    rc, msg = from_counts(prm, gc=np.array([2, 5], np.uint32))
    assert rc == PS_ERR_INVALID and "ones among" in msg
    rc, msg = from_counts(prm, n11=np.array([3, 1, 1, 0, 1, 1], np.uint32))              # above both counts
    assert rc == PS_ERR_INVALID and "does not fit" in msg
    rc, msg = from_counts(prm, sc=np.array([3, 2, 2], np.uint32), gc=np.array([3, 1], np.uint32))      # 3 + 3 - 1 > 4
    assert rc == PS_ERR_INVALID and "does not fit" in msg
    rc, msg = from_counts(prm, N=65537)
    assert rc == PS_ERR_INVALID and "pop_size" in msg
    rc, msg = from_counts(prm, n_sites=65535, n_genes=2)                                   # (refused before a list is read)
    assert rc == PS_ERR_INVALID and "exceeds" in msg
    assert lib.ps_gene_site_ld_timing(None, None, None, None, None) == PS_ERR_INVALID


def test_the_device_entries_need_a_device(pa):
    """without a device the device entries fail with PS_ERR_NO_DEVICE before they look at their arguments; with one, the same
    calls refuse their null handles"""
    lib = pa.load()
    o, prm = pa._lib.Gs(), pa._lib.GsParams(64, 1, 1, 1, 4096, 4096, 32768)
    b = np.zeros(64, np.uint64)
    want = PS_ERR_NO_DEVICE if lib.ps_device_count() <= 0 else PS_ERR_INVALID
    tail = (C.byref(prm), None, 0, None, 0, C.byref(o), None, None, b.ctypes.data, b.ctypes.data)
    assert lib.ps_gene_site_ld(None, None, *tail) == want
    assert lib.ps_sim_gene_site_ld(None, *tail) == want
    assert lib.ps_multi_gene_site_ld(None, *tail) == want
    if want == PS_ERR_NO_DEVICE:
        assert "no HIP device" in lib.ps_last_error().decode()
        bad = pa._lib.GsParams(0, 0, 0, 0, 0, 0, 0)                # ... and before the parameters
        tail = (C.byref(bad), None, 0, None, 0, C.byref(o), None, None, None, None)
        assert lib.ps_gene_site_ld(None, None, *tail) == PS_ERR_NO_DEVICE
        assert lib.ps_sim_gene_site_ld(None, *tail) == PS_ERR_NO_DEVICE
        assert lib.ps_multi_gene_site_ld(None, *tail) == PS_ERR_NO_DEVICE


def test_abi_header_and_bindings_agree(pa):
    lib = pa.load()
    hdr = open(os.path.join(ROOT, "include", "pansim_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in pa._lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
    assert lib.ps_abi_version() == 3
    for struct, cls in (("ps_gs_params", pa._lib.GsParams), ("ps_gs_t", pa._lib.Gs), ("ps_gs_side", pa._lib.GsSide)):
        fields = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1)
        assert re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S)) == [n for n, _ in cls._fields_], struct
    assert re.search(r"#define PS_GS_NONE 0xFFFFFFFFu", hdr) and pa._lib.PS_GS_NONE == 0xFFFFFFFF == ref.NONE
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert "fn %s(" % name in integration, name
    assert os.path.exists(os.path.join(ROOT, "docs", "GENE_SITE_ASSOCIATION.md"))
    assert pa.GeneSiteLd is pa.association.GeneSiteLd and pa.gene_site_from_counts is pa.association.gene_site_from_counts


def test_both_run_classes_ask_for_their_own_entry(pa):
    """written once beside _Readouts, not in it; no device: the library is an object that notes the first symbol asked for"""
    from pansim_amd import _lib, simulation

    class Asked(Exception):
        pass

    class Library:
        def __getattr__(self, name):
            raise Asked(name)

    assert "gene_site_ld" not in vars(simulation._Readouts)
    for cls, symbol in ((pa.Simulation, "ps_sim_gene_site_ld"), (pa.MultiSimulation, "ps_multi_gene_site_ld")):
        assert hasattr(cls, "gene_site_ld") and "gene_site_ld" not in vars(cls)
        run = object.__new__(cls)
        run._lib, run._h, run.generation = Library(), None, 0
        run.params = _lib.SimParams(pop_size=8, core_size=100, pan_genes=60, core_genes=20, max_distances=10)
        with pytest.raises(Asked) as e:
            run.gene_site_ld()
        assert str(e.value) == symbol and symbol in _lib.SIGNATURES
