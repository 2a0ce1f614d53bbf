"""Nearest neighbours and lineages without a device (docs/NEAREST_NEIGHBOURS.md): ps_neighbours_from_counts and
ps_lineages_from_neighbours against the plain restatement (tests/nearest_neighbours_ref.py) on complete lists with ties and
undefined pairs and on incomplete lists, their error paths, the identities of the summary, the rank-1 edges inside the
existing ps_tree_from_counts, the no-device errors of the device entries and the CLI's flag checks and help texts.  The device
half is tests/test_gpu_nearest_neighbours.py.  Every comparison is an equality of integer arrays and integer fields."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nearest_neighbours_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_NO_DEVICE, PS_ERR_STATE = -1, -2, -6
NEW_SYMBOLS = ("ps_nearest_neighbours", "ps_sim_nearest_neighbours", "ps_multi_nearest_neighbours", "ps_neighbours_from_counts",
               "ps_lineages_from_neighbours", "ps_nearest_neighbours_timing")
METRICS = (("core", ref.CORE), ("acc", ref.ACC))


def numerators(rng, P, L, G):
    """h of either parity, intersections at most unions, unions at most G"""
    h = rng.integers(0, 2 * L + 2, P, dtype=np.uint32)
    u = rng.integers(0, G + 1, P, dtype=np.uint32)
    i = np.minimum((rng.random(P) * (u + 1)).astype(np.uint32), u)
    return h, i, u


def check(pa, r1, r2, h, i, u, N, L, cg, k, ranks=None):
    """both metrics against the restatement, the lineages at every rank (or those given) -> the two results"""
    out = []
    for name, metric in METRICS:
        got = pa.neighbours_from_counts(r1, r2, h, i, u, N, L, cg, k, metric=name)
        ref.assert_equal(got, ref.from_pairs(metric, r1, r2, h, i, u, N, L, cg, k))
        assert got.metric == metric and got.pairs == len(r1)
        counts = []
        for rank in ranks or range(1, k + 1):
            lin = got.lineages(rank)
            ref.assert_lineages(lin, got.nbr, rank)
            counts.append(lin[1]["lineages"])
        assert counts == sorted(counts, reverse=True)       # (more edges never split a lineage)
        ref.assert_lineages(got.lineages(), got.nbr, k)
        out.append(got)
    return out


def shuffled(rng, N):
    """the complete list in a shuffled order, either orientation"""
    r1, r2 = ref.all_pairs(N)
    order = rng.permutation(r1.size)
    swap = rng.random(r1.size) < 0.5
    return np.where(swap, r2, r1)[order].astype(np.uint32), np.where(swap, r1, r2)[order].astype(np.uint32)


@pytest.mark.parametrize("N,k", [(2, 1), (5, 4), (40, 1), (40, 7), (40, 39), (130, 128)])
def test_complete_lists_equal_the_restatement(pa, N, k):
    """random numerators over the complete list; few values: many ties; cg = 0 with small G: undefined accessory pairs"""
    rng = np.random.default_rng(N * 1000 + k)
    a, b = shuffled(rng, N)
    for L, G in ((300, 70), (3, 2)):
        h, i, u = numerators(rng, a.size, L, G)
        for cg in (0, 5):
            for got in check(pa, a, b, h, i, u, N, L, cg, k, ranks=None if k < 10 else (1, 2, k)):
                assert got.graph_edges + got.mutual_edges == N * k and (got.nbr != ref.NONE).all()
                assert (got.nbr != np.arange(N)[:, None]).all()
    # G = 2 without core genes: about a third of the pairs is undefined, and a full list (k = N - 1) holds every one twice
    got = pa.neighbours_from_counts(a, b, h, i, u, N, 3, 0, k, metric="acc")
    assert got.undefined_neighbours == int((got.den == 0).sum())
    if k == N - 1:
        assert got.undefined_neighbours == 2 * int((u == 0).sum())
    # the numerators of the other metric may be left out
    got = pa.neighbours_from_counts(a, b, h, None, None, N, 300, 5, k, metric="core")
    ref.assert_equal(got, ref.from_pairs(ref.CORE, a, b, h, i, u, N, 300, 5, k))
    got = pa.neighbours_from_counts(a, b, None, i, u, N, 300, 5, k, metric="acc")
    ref.assert_equal(got, ref.from_pairs(ref.ACC, a, b, h, i, u, N, 300, 5, k))


def test_all_ties_list_the_lowest_rows(pa):
    N, k = 9, 3
    a, b = shuffled(np.random.default_rng(3), N)
    c = np.full(a.size, 6, np.uint32)
    for got in check(pa, a, b, c, c // 2, c, N, 10, 4, k):
        for i in range(N):
            assert list(got.nbr[i]) == [j for j in range(N) if j != i][:k]
        # rows 0 .. 3 list each other; every later row lists 0, 1, 2 one way
        assert got.mutual_edges == 6 and got.graph_edges == N * k - 6
        assert got.lineages(1)[1]["lineages"] == 1 and list(got.lineages(1)[0]) == [0] * N
    assert pa.neighbours_from_counts(a, b, c, c // 2, c, N, 10, 4, k, metric="core").num[0, 0] == 3
    assert pa.neighbours_from_counts(a, b, c, c // 2, c, N, 10, 4, k, metric="acc").den[0, 0] == 10


def test_equal_ratios_tie_and_the_row_decides(pa):
    """seen from row 2: row 1 at 2 / 4 and row 0 at 1 / 2 are one distance, so row 0 comes first; 3 / 7 is nearer than both"""
    arr = lambda *v: np.array(v, np.uint32)
    r1, r2 = arr(1, 0, 0, 2), arr(2, 2, 1, 3)
    u, i = arr(4, 2, 5, 7), arr(2, 1, 2, 4)                  # a / b = 2 / 4, 1 / 2, 3 / 5, 3 / 7 with no core genes
    got = pa.neighbours_from_counts(r1, r2, None, i, u, 4, 10, 0, 3, metric="acc")
    ref.assert_equal(got, ref.from_pairs(ref.ACC, r1, r2, u, i, u, 4, 10, 0, 3))
    assert list(zip(got.nbr[2], got.num[2], got.den[2])) == [(3, 3, 7), (0, 1, 2), (1, 2, 4)]
    assert list(got.nbr[3]) == [2, ref.NONE, ref.NONE] and list(got.num[3]) == [3, 0, 0] and list(got.den[3]) == [7, 0, 0]
    assert got.undefined_neighbours == 0 and np.isnan(got.distance[3, 1])


def test_undefined_pairs_sort_last(pa):
    """U = 0 and no core genes: 0 / 0, above every defined distance -- 1 / 1 included -- and equal among themselves"""
    N = 6
    r1, r2 = ref.all_pairs(N)
    empty = (1, 4, 5)
    u = np.array([0 if (a in empty and b in empty) else 3 for a, b in zip(r1, r2)], np.uint32)
    i = np.zeros_like(u)                                     # every defined pair at 3 / 3
    _, got = check(pa, r1, r2, u, i, u, N, 10, 0, 5)
    for e in empty:
        others = [j for j in empty if j != e]
        assert list(got.nbr[e]) == [0, 2, 3] + others and list(got.den[e]) == [3, 3, 3, 0, 0] and list(got.num[e, 3:]) == [0, 0]
    assert got.undefined_neighbours == 6
    assert pa.neighbours_from_counts(r1, r2, None, i, u, N, 10, 0, 3, metric="acc").undefined_neighbours == 0
    assert pa.neighbours_from_counts(r1, r2, None, i, u, N, 10, 1, 5, metric="acc").undefined_neighbours == 0      # one core gene: 0 / 1


def test_incomplete_lists_leave_sentinels(pa):
    """two paths of 20 and 10 and five individuals in no pair: at most two partners each"""
    rng = np.random.default_rng(1)
    N, k = 35, 3
    order = rng.permutation(30).astype(np.uint32)
    r1 = np.concatenate([order[:19], order[20:29]])
    r2 = np.concatenate([order[1:20], order[21:30]])
    h, i, u = numerators(rng, r1.size, 300, 70)
    for got in check(pa, r1, r2, h, i, u, N, 300, 2, k):
        filled = (got.nbr != ref.NONE).sum(1)
        assert list(np.bincount(filled, minlength=3)) == [5, 4, 26] and (got.nbr[:, 2] == ref.NONE).all()
        assert not got.num[got.nbr == ref.NONE].any() and not got.den[got.nbr == ref.NONE].any()
        assert np.isnan(got.distance[got.nbr == ref.NONE]).all()
        assert got.graph_edges + got.mutual_edges == 2 * 28 and got.pairs == 28
        assert got.lineages()[1]["lineages"] == 7 and got.lineages()[1]["edges"] == 28
    # no pair at all
    e = np.zeros(0, np.uint32)
    got = pa.neighbours_from_counts(e, e, e, e, e, 5, 10, 1, 2)
    assert (got.nbr == ref.NONE).all() and got.graph_edges == 0 and got.mutual_edges == 0
    assert list(got.lineages()[0]) == [0, 1, 2, 3, 4] and got.lineages()[1]["lineages"] == 5


def test_duplicate_pairs_are_listed_once(pa):
    """every pair twice with different numerators: the nearer copy is listed, once"""
    rng = np.random.default_rng(2)
    N = 12
    r1, r2 = ref.all_pairs(N)
    r1, r2 = np.concatenate([r1, r2]), np.concatenate([r2, r1])
    h, i, u = numerators(rng, r1.size, 20, 9)
    for got in check(pa, r1, r2, h, i, u, N, 20, 1, 11):
        assert all(len(set(row)) == 11 for row in got.nbr.tolist())


def test_the_largest_cross_products_stay_exact(pa):
    """a = 65535 over b = 2^32 - 1 against 65534 over b - 1: the products pass 2^47 and differ in their last digits"""
    arr = lambda *v: np.array(v, np.uint32)
    cg = 2**32 - 65536 - 65535
    r1, r2, i, u = arr(0, 0, 1), arr(1, 2, 2), arr(0, 1, 0), arr(65535, 65535, 65535)
    got = pa.neighbours_from_counts(r1, r2, None, i, u, 3, 10, cg, 2, metric="acc")
    ref.assert_equal(got, ref.from_pairs(ref.ACC, r1, r2, u, i, u, 3, 10, cg, 2))
    assert list(got.nbr[0]) == [2, 1] and list(got.num[0]) == [65534, 65535]


@pytest.mark.parametrize("name,metric", METRICS)
def test_rank_one_edges_are_tree_edges(pa, name, metric):
    """the minimum edge at a vertex under a strict order is in the minimum spanning tree: every (i, nbr[i, 0]) of a complete
    list is an edge of the existing ps_tree_from_counts of the same list, with the same distance"""
    rng = np.random.default_rng(17)
    N = 60
    a, b = shuffled(rng, N)
    h, i, u = numerators(rng, a.size, 40, 12)                # (few values: the ties are what the orders must agree on)
    got = pa.neighbours_from_counts(a, b, h, i, u, N, 40, 0, 4, metric=name)
    tree = pa.tree_from_counts(a, b, h, i, u, N, 40, 0, metric=name)
    edges = {(int(x), int(y)): (int(n), int(d)) for x, y, n, d in zip(tree.lo, tree.hi, tree.num, tree.den)}
    for r in range(N):
        j = int(got.nbr[r, 0])
        assert edges.get((min(r, j), max(r, j))) == (int(got.num[r, 0]), int(got.den[r, 0])), r
    # ... and so the lineages at rank 1 are unions of tree edges: no fewer of them than N less the distinct rank-1 pairs
    lin = got.lineages(1)[1]
    assert lin["lineages"] == N - lin["edges"]


def test_error_paths_of_neighbours_from_counts(pa):
    lib = pa.load()
    P, T = pa._lib.KnnParams, pa._lib.Knn
    arr = lambda *v: np.array(v, np.uint32)
    base = dict(r1=arr(0, 1), r2=arr(1, 2), h=arr(4, 6), i=arr(1, 2), u=arr(3, 2), nbr=np.zeros(6, np.uint32), num=np.zeros(6, np.uint64),
                den=np.zeros(6, np.uint64))
    out = T()

    def call(prm, n=2, N=3, o=out, cg=1, **kw):
        a = dict(base, **kw)
        ptr = lambda x: None if x is None else x.ctypes.data
        return lib.ps_neighbours_from_counts(ptr(a["r1"]), ptr(a["r2"]), ptr(a["h"]), ptr(a["i"]), ptr(a["u"]), n, N, 10, cg,
                                             C.byref(prm) if prm is not None else None, C.byref(o) if o is not None else None,
                                             ptr(a["nbr"]), ptr(a["num"]), ptr(a["den"]))

    def fails(text, *args, **kw):
        assert call(*args, **kw) == PS_ERR_INVALID
        assert text in lib.ps_last_error().decode(), lib.ps_last_error().decode()

    core, acc = P(0, 2), P(1, 2)
    assert call(core) == 0 and call(acc) == 0
    for metric in (2, -1, 7):
        fails("PS_KNN_CORE (0) or PS_KNN_ACC (1)", P(metric, 2))
    for m in (0, 1):
        fails("1 <= k <= min(pop_size - 1, 128)", P(m, 0))
        fails("1 <= k <= min(pop_size - 1, 128)", P(m, 3))                   # k = N
        fails("1 <= k <= min(pop_size - 1, 128)", P(m, 129), N=1000)
    fails("pair 1: intersection 3 above union 2", acc, i=arr(1, 3))
    assert call(core, i=arr(1, 3)) == 0                         # (the accessory numerators are not looked at)
    fails("65535 accessory genes", acc, u=arr(3, 65536))
    assert call(acc, u=arr(3, 65535)) == 0
    for prm in (core, acc):
        fails("pair 1: index 3 is not below pop_size 3", prm, r2=arr(1, 3))
        fails("pair 0: index 7 is not below pop_size 3", prm, r1=arr(7, 1))
        fails("pair 1: both indices are 1", prm, r2=arr(1, 1))
        fails("pop_size", prm, N=1)
        for kw in (dict(r1=None), dict(r2=None), dict(nbr=None), dict(num=None), dict(den=None), dict(o=None)):
            fails("null", prm, **kw)
    fails("null", core, h=None)
    fails("null", acc, i=None)
    fails("null", acc, u=None)
    fails("null", None)
    # core_genes + 65535 must stay below 2^32 under the accessory metric only
    fails("core_genes + 65535 < 2^32", acc, cg=2**32 - 65535)
    assert call(acc, cg=2**32 - 65536) == 0
    assert call(core, cg=2**40) == 0
    with pytest.raises(ValueError):
        pa.neighbours_from_counts(base["r1"], base["r2"], base["h"], base["i"], base["u"], 3, 10, 1, 2, metric="joint")
    with pytest.raises(ValueError):
        pa.neighbours_from_counts(base["r1"], base["r2"][:-1], base["h"], base["i"], base["u"], 3, 10, 1, 2)
    with pytest.raises(pa.PansimError) as e:
        pa.neighbours_from_counts(base["r1"], base["r2"], base["h"], arr(1, 3), base["u"], 3, 10, 1, 2, metric="acc")
    assert e.value.code == PS_ERR_INVALID and "intersection 3 above union 2" in str(e.value)


def test_error_paths_of_lineages_from_neighbours(pa):
    lib = pa.load()
    out = pa._lib.Lineages()
    nbr = np.array([[1, 2], [0, 2], [0, ref.NONE]], np.uint32)
    labels = np.zeros(3, np.uint32)

    def call(a=nbr, N=3, k=2, rank=2, o=out, lab=labels):
        return lib.ps_lineages_from_neighbours(None if a is None else a.ctypes.data, N, k, rank, C.byref(o) if o is not None else None,
                                               None if lab is None else lab.ctypes.data)

    assert call() == 0 and out.lineages == 1 and out.edges == 3 and list(labels) == [0, 0, 0]
    assert call(rank=1) == 0 and out.edges == 2 and out.rank == 1
    for rank in (0, 3, 2**31):
        assert call(rank=rank) == PS_ERR_INVALID and "rank" in lib.ps_last_error().decode()
    assert call(a=np.array([[1, 2], [0, 3], [0, 1]], np.uint32)) == PS_ERR_INVALID
    assert "index 3 is not below pop_size 3" in lib.ps_last_error().decode()
    for kw in (dict(a=None), dict(o=None), dict(lab=None)):
        assert call(**kw) == PS_ERR_INVALID and "null" in lib.ps_last_error().decode()
    got = pa.neighbours_from_counts(np.array([0], np.uint32), np.array([1], np.uint32), np.array([4], np.uint32), None, None, 3, 10, 0, 2)
    with pytest.raises(pa.PansimError) as e:
        got.lineages(3)
    assert e.value.code == PS_ERR_INVALID
    assert list(got.lineages(1)[0]) == [0, 0, 2]


def test_every_new_symbol_is_exported_and_declared(pa):
    lib = C.CDLL(pa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pansim_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in pa._lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
    assert lib.ps_abi_version() == 3
    for struct, cls in (("ps_knn_t", pa._lib.Knn), ("ps_lineage_t", pa._lib.Lineages), ("ps_knn_params", pa._lib.KnnParams)):
        fields = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1)
        assert re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields)) == [n for n, _ in cls._fields_]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert "fn %s(" % name in integration, name


def test_the_device_entries_need_a_device(pa):
    """without a device the three device entries fail with PS_ERR_NO_DEVICE before they look at their arguments; with one,
    the same calls refuse their null arguments"""
    lib = pa.load()
    out, prm = pa._lib.Knn(), pa._lib.KnnParams(0, 1)
    nbr, num = np.zeros(16, np.uint32), np.zeros(16, np.uint64)
    tail = (C.byref(prm), C.byref(out), nbr.ctypes.data, num.ctypes.data, num.ctypes.data)
    want = PS_ERR_NO_DEVICE if lib.ps_device_count() <= 0 else PS_ERR_INVALID
    assert lib.ps_nearest_neighbours(None, None, *tail) == want
    assert lib.ps_sim_nearest_neighbours(None, *tail) == want
    assert lib.ps_multi_nearest_neighbours(None, *tail) == want
    if want == PS_ERR_NO_DEVICE:
        assert "no HIP device" in lib.ps_last_error().decode()
        bad = pa._lib.KnnParams(9, 0)                            # ... and before the parameters
        assert lib.ps_nearest_neighbours(None, None, C.byref(bad), *tail[1:]) == PS_ERR_NO_DEVICE
    assert lib.ps_nearest_neighbours_timing(None, None, None) == PS_ERR_INVALID


def cli(*args):
    return subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=60)


def test_cli_rejects_bad_values(pa):
    """checked before any device work; the metric whether or not --print_knn is given"""
    for extra in ((), ("--print_knn", 3)):
        r = cli("--knn_metric", "bogus", "--pan_genes", 3000, *extra)
        assert r.returncode == 101 and r.stdout == "" and "--knn_metric" in r.stderr and "core or acc" in r.stderr, (r.returncode, r.stderr)
    for value in ("0", "129", "-1", "x", "2.5", "1000"):                # (1000 = the default pop_size: k = N)
        r = cli("--pan_genes", 3000, "--print_knn=" + value)
        assert r.returncode == 101 and r.stdout == "" and "--print_knn" in r.stderr, (value, r.returncode, r.stderr)
    r = cli("--pan_genes", 3000, "--pop_size", 5, "--print_knn", 5)
    assert r.returncode == 101 and "pop_size - 1" in r.stderr
    r = cli("--print_knn")
    assert r.returncode == 2 and "requires a value" in r.stderr


def test_help_extensions_lists_the_knn_flags(pa):
    r = cli("--help-extensions")
    assert r.returncode == 0
    assert "--print_knn <print_knn>\n" in r.stdout and "--knn_metric <knn_metric>\n" in r.stdout
    for name in ("_knn.tsv", "_lineages.tsv", "_knn_summary.tsv"):
        assert name in r.stdout
    r = cli("--help")
    assert r.returncode == 0 and "knn" not in r.stdout
    assert r.stdout[r.stdout.index("USAGE:"):] == open(os.path.join(ROOT, "tests", "golden", "help_usage.txt")).read()
