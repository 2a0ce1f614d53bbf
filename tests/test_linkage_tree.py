"""The single-linkage tree without a device (docs/LINKAGE_TREE.md): ps_tree_from_counts against the plain-integer Kruskal
(tests/linkage_tree_ref.py), ties, forests, duplicates, undefined pairs, its error paths, cut / clusters_at against the existing
ps_clusters_from_counts, the no-device errors of the device entries and the CLI's flag checks and help texts.  The device
half is tests/test_gpu_linkage_tree.py.  Every comparison is an equality of integer arrays and integer fields."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import linkage_tree_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_NO_DEVICE, PS_ERR_STATE = -1, -2, -6
NEW_SYMBOLS = ("ps_linkage_tree", "ps_sim_linkage_tree", "ps_multi_linkage_tree", "ps_tree_from_counts", "ps_linkage_tree_timing")
METRICS = (("core", ref.CORE), ("acc", ref.ACC))


def numerators(rng, P, L, G):
    """h of either parity, intersections at most unions, unions at most G"""
    h = rng.integers(0, 2 * L + 2, P, dtype=np.uint32)
    u = rng.integers(0, G + 1, P, dtype=np.uint32)
    i = np.minimum((rng.random(P) * (u + 1)).astype(np.uint32), u)
    return h, i, u


def check(pa, r1, r2, h, i, u, N, L, cg, spanning=True):
    """both metrics against the reference -> the two results"""
    out = []
    for name, metric in METRICS:
        got = pa.tree_from_counts(r1, r2, h, i, u, N, L, cg, metric=name)
        ref.assert_equal(got, ref.tree(metric, r1, r2, h, i, u, N, L, cg), N)
        assert got.rounds == 0 and got.metric == metric
        if spanning:
            ref.assert_spanning(got, N)
        out.append(got)
    return out


@pytest.mark.parametrize("N", [2, 5, 40])
def test_complete_lists_equal_kruskal(pa, N):
    """random numerators over the complete list (in a shuffled order, either orientation), few values: many ties"""
    rng = np.random.default_rng(N)
    r1, r2 = ref.all_pairs(N)
    order = rng.permutation(r1.size)
    swap = rng.random(r1.size) < 0.5
    a, b = np.where(swap, r2, r1)[order].astype(np.uint32), np.where(swap, r1, r2)[order].astype(np.uint32)
    for L, G in ((300, 70), (3, 4)):
        h, i, u = numerators(rng, r1.size, L, G)
        for cg in (0, 5):
            check(pa, a, b, h, i, u, N, L, cg)
    # the numerators of the other metric may be left out
    h, i, u = numerators(rng, r1.size, 300, 70)
    got = pa.tree_from_counts(a, b, h, None, None, N, 300, 5, metric="core")
    ref.assert_equal(got, ref.tree(ref.CORE, a, b, h, i, u, N, 300, 5), N)
    got = pa.tree_from_counts(a, b, None, i, u, N, 300, 5, metric="acc")
    ref.assert_equal(got, ref.tree(ref.ACC, a, b, h, i, u, N, 300, 5), N)


def test_an_incomplete_list_leaves_a_forest(pa):
    """two paths of 20 and 10 and five individuals in no pair: 28 edges, the arrays cut to them"""
    rng = np.random.default_rng(1)
    N = 35
    order = rng.permutation(30).astype(np.uint32)
    r1 = np.concatenate([order[:19], order[20:29]])
    r2 = np.concatenate([order[1:20], order[21:30]])
    h, i, u = numerators(rng, r1.size, 300, 70)
    for got in check(pa, r1, r2, h, i, u, N, 300, 2, spanning=False):
        assert got.edges == 28 and got.lo.size == 28 and got.pairs == 28
        assert got.clusters_at(0, 0) == 7
    # no pair at all
    e = np.zeros(0, np.uint32)
    got = pa.tree_from_counts(e, e, e, e, e, 5, 10, 1)
    assert got.edges == 0 and got.distinct_heights == 0 and got.lo.size == 0 and list(got.cut(0, 0)) == [0, 1, 2, 3, 4]


def test_duplicate_pairs(pa):
    """every pair twice with different numerators: the smaller copy decides"""
    rng = np.random.default_rng(2)
    N = 12
    r1, r2 = ref.all_pairs(N)
    r1, r2 = np.concatenate([r1, r2]), np.concatenate([r2, r1])
    h, i, u = numerators(rng, r1.size, 20, 9)
    check(pa, r1, r2, h, i, u, N, 20, 1)


def test_all_ties_give_the_star_of_row_0(pa):
    N = 9
    r1, r2 = ref.all_pairs(N)
    rng = np.random.default_rng(3)
    order = rng.permutation(r1.size)
    c = np.full(r1.size, 6, np.uint32)
    for got in check(pa, r2[order], r1[order], c, c // 2, c, N, 10, 4):
        assert list(got.lo) == [0] * (N - 1) and list(got.hi) == list(range(1, N)) and got.distinct_heights == 1
    assert pa.tree_from_counts(r1, r2, c, c // 2, c, N, 10, 4, metric="core").num[0] == 3
    assert pa.tree_from_counts(r1, r2, c, c // 2, c, N, 10, 4, metric="acc").den[0] == 10


def test_equal_ratios_tie_and_the_rows_decide(pa):
    """1 / 2 and 2 / 4 are one height: with (1, 2) at 2 / 4 and (0, 2) at 1 / 2 the order is by rows, and (0, 1) at 3 / 5 loses"""
    arr = lambda *v: np.array(v, np.uint32)
    r1, r2 = arr(1, 0, 0), arr(2, 2, 1)
    u, i = arr(4, 2, 5), arr(2, 1, 2)                # a / b = 2 / 4, 1 / 2, 3 / 5 with no core genes
    got = pa.tree_from_counts(r1, r2, None, i, u, 3, 10, 0, metric="acc")
    ref.assert_equal(got, ref.tree(ref.ACC, r1, r2, u, i, u, 3, 10, 0), 3)
    assert list(zip(got.lo, got.hi, got.num, got.den)) == [(0, 2, 1, 2), (1, 2, 2, 4)]
    assert got.distinct_heights == 1 and got.undefined_edges == 0
    # ... whereas by numerators alone (1, 2) would have come second for another reason: make it the smaller row pair
    got = pa.tree_from_counts(arr(0, 1, 0), arr(1, 2, 2), None, arr(2, 1, 2), arr(4, 2, 5), 3, 10, 0, metric="acc")
    assert list(zip(got.lo, got.hi, got.num, got.den)) == [(0, 1, 2, 4), (1, 2, 1, 2)]
    # a strictly smaller ratio with larger numbers comes first: 3 / 7 < 1 / 2
    got = pa.tree_from_counts(arr(0, 1), arr(1, 2), None, arr(1, 4), arr(2, 7), 3, 10, 0, metric="acc")
    assert list(zip(got.lo, got.hi, got.num, got.den)) == [(1, 2, 3, 7), (0, 1, 1, 2)]


def test_undefined_pairs_sort_last(pa):
    """U = 0 and no core genes: 0 / 0, above every defined distance -- 1 / 1 included -- and equal among themselves"""
    N = 6
    r1, r2 = ref.all_pairs(N)
    empty = (1, 4, 5)
    u = np.array([0 if (a in empty and b in empty) else 3 for a, b in zip(r1, r2)], np.uint32)
    i = np.zeros_like(u)                              # every defined pair at 3 / 3
    (_, got) = check(pa, r1, r2, u, i, u, N, 10, 0)
    assert got.undefined_edges == 0 and got.distinct_heights == 1      # the empty rows are joined through the others
    # only the empty rows: every pair undefined, the star of row 0 at 0 / 0
    r1, r2 = ref.all_pairs(3)
    z = np.zeros(3, np.uint32)
    got = pa.tree_from_counts(r1, r2, None, z, z, 3, 10, 0, metric="acc")
    ref.assert_equal(got, ref.tree(ref.ACC, r1, r2, z, z, z, 3, 10, 0), 3)
    assert got.undefined_edges == 2 and got.distinct_heights == 1 and not got.num.any() and not got.den.any()
    assert np.isnan(got.distance).all() and list(got.hi) == [1, 2]
    # a defined and an undefined way to the same row: the defined one is taken, whatever its size
    got = pa.tree_from_counts(np.array([0, 0, 1], np.uint32), np.array([1, 2, 2], np.uint32), None, np.array([0, 0, 0], np.uint32),
                              np.array([0, 5, 5], np.uint32), 3, 10, 0, metric="acc")
    assert list(zip(got.lo, got.hi, got.num, got.den)) == [(0, 2, 5, 5), (1, 2, 5, 5)] and got.undefined_edges == 0
    assert pa.tree_from_counts(r1, r2, None, z, z, 3, 10, 1, metric="acc").undefined_edges == 0      # one core gene: 0 / 1


def test_error_paths(pa):
    lib = pa.load()
    P, T = pa._lib.TreeParams, pa._lib.Tree
    arr = lambda *v: np.array(v, np.uint32)
    base = dict(r1=arr(0, 1), r2=arr(1, 2), h=arr(4, 6), i=arr(1, 2), u=arr(3, 2), lo=np.zeros(3, np.uint32), hi=np.zeros(3, np.uint32),
                num=np.zeros(3, np.uint64), den=np.zeros(3, np.uint64))
    out = T()

    def call(prm, n=2, N=3, o=out, cg=1, **kw):
        a = dict(base, **kw)
        ptr = lambda x: None if x is None else x.ctypes.data
        return lib.ps_tree_from_counts(ptr(a["r1"]), ptr(a["r2"]), ptr(a["h"]), ptr(a["i"]), ptr(a["u"]), n, N, 10, cg,
                                       C.byref(prm) if prm is not None else None, C.byref(o) if o is not None else None, ptr(a["lo"]),
                                       ptr(a["hi"]), ptr(a["num"]), ptr(a["den"]))

    def fails(text, *args, **kw):
        assert call(*args, **kw) == PS_ERR_INVALID
        assert text in lib.ps_last_error().decode(), lib.ps_last_error().decode()

    core, acc = P(0), P(1)
    assert call(core) == 0 and call(acc) == 0
    for metric in (2, -1, 7):
        fails("PS_TREE_CORE (0) or PS_TREE_ACC (1)", P(metric))
    fails("pair 1: intersection 3 above union 2", acc, i=arr(1, 3))
    assert call(core, i=arr(1, 3)) == 0                         # (the accessory numerators are not looked at)
    fails("65535 accessory genes", acc, u=arr(3, 65536))
    assert call(acc, u=arr(3, 65535)) == 0
    for prm in (core, acc):
        fails("pair 1: index 3 is not below pop_size 3", prm, r2=arr(1, 3))
        fails("pair 0: index 7 is not below pop_size 3", prm, r1=arr(7, 1))
        fails("pair 1: both indices are 1", prm, r2=arr(1, 1))
        fails("pop_size", prm, N=1)
        for kw in (dict(r1=None), dict(r2=None), dict(lo=None), dict(hi=None), dict(num=None), dict(den=None), dict(o=None)):
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
        pa.tree_from_counts(base["r1"], base["r2"], base["h"], base["i"], base["u"], 3, 10, 1, metric="joint")
    with pytest.raises(ValueError):
        pa.tree_from_counts(base["r1"], base["r2"][:-1], base["h"], base["i"], base["u"], 3, 10, 1)
    with pytest.raises(pa.PansimError) as e:
        pa.tree_from_counts(base["r1"], base["r2"], base["h"], arr(1, 3), base["u"], 3, 10, 1, metric="acc")
    assert e.value.code == PS_ERR_INVALID and "intersection 3 above union 2" in str(e.value)


def test_the_largest_cross_products_stay_exact(pa):
    """a = 65535 over b = 2^32 - 1 against 65534 over b - 1: the products pass 2^47 and differ in their last digits"""
    arr = lambda *v: np.array(v, np.uint32)
    cg = 2**32 - 65536 - 65535
    r1, r2, i, u = arr(0, 0, 1), arr(1, 2, 2), arr(0, 1, 0), arr(65535, 65535, 65535)
    got = pa.tree_from_counts(r1, r2, None, i, u, 3, 10, cg, metric="acc")
    ref.assert_equal(got, ref.tree(ref.ACC, r1, r2, u, i, u, 3, 10, cg), 3)
    assert list(got.num) == [65534, 65535] and list(got.lo) == [0, 0] and list(got.hi) == [2, 1]


@pytest.mark.parametrize("metric,which", METRICS)
def test_cut_equals_the_clusters_at_every_height(pa, metric, which):
    """cut / clusters_at against the existing ps_clusters_from_counts over the same list: at every merge height (equality is
    an edge), just below it, and past the last one"""
    rng = np.random.default_rng(11)
    N, L, cg = 40, 300, 5
    r1, r2 = ref.all_pairs(N)
    h, i, u = numerators(rng, r1.size, 3000, 60000)             # (a wide range: few ties, many heights)
    got = pa.tree_from_counts(r1, r2, h, i, u, N, L, cg, metric=metric)
    assert got.distinct_heights > 5
    cuts = {(int(n), int(d)) for n, d in zip(got.num, got.den)}
    cuts |= {(0, L if which == ref.CORE else 1), (int(got.num[-1]) + 1, int(got.den[-1]))}
    if which == ref.CORE:
        cuts |= {(n - 1, d) for n, d in cuts if n > 0}
    else:
        cuts |= {(n * 100 - 1, d * 100) for n, d in cuts if n > 0}          # just below the height
    seen = set()
    for n, d in sorted(cuts):
        if which == ref.CORE:
            assert d == L
            want = pa.clusters_from_counts(r1, r2, h, i, u, N, L, cg, core_max_d=n)
        else:
            assert n <= d <= 2**24
            want = pa.clusters_from_counts(r1, r2, h, i, u, N, L, cg, acc_ratio=(n, d))
        assert np.array_equal(got.cut(n, d), want.labels), (n, d)
        assert got.clusters_at(n, d) == want.clusters
        seen.add(want.clusters)
    assert 1 in seen and len(seen - {N}) == got.distinct_heights           # (one more cluster count per height)


def test_every_new_symbol_is_exported_and_declared(pa):
    lib = C.CDLL(pa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pansim_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in pa._lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
    assert lib.ps_abi_version() == 3
    fields = re.search(r"typedef struct \{([^}]*)\} ps_tree_t;", hdr).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields)) == [n for n, _ in pa._lib.Tree._fields_]


def test_the_device_entries_need_a_device(pa):
    """without a device the three device entries fail with PS_ERR_NO_DEVICE before they look at their arguments; with one,
    the same calls refuse their null arguments"""
    lib = pa.load()
    out, prm = pa._lib.Tree(), pa._lib.TreeParams(0)
    lo, num = np.zeros(16, np.uint32), np.zeros(16, np.uint64)
    tail = (C.byref(prm), C.byref(out), lo.ctypes.data, lo.ctypes.data, num.ctypes.data, num.ctypes.data)
    want = PS_ERR_NO_DEVICE if lib.ps_device_count() <= 0 else PS_ERR_INVALID
    assert lib.ps_linkage_tree(None, None, *tail) == want
    assert lib.ps_sim_linkage_tree(None, *tail) == want
    assert lib.ps_multi_linkage_tree(None, *tail) == want
    if want == PS_ERR_NO_DEVICE:
        assert "no HIP device" in lib.ps_last_error().decode()
        bad = pa._lib.TreeParams(9)                              # ... and before the parameters
        assert lib.ps_linkage_tree(None, None, C.byref(bad), *tail[1:]) == PS_ERR_NO_DEVICE
    assert lib.ps_linkage_tree_timing(None, None, None, None) == PS_ERR_INVALID


def test_timing_before_any_call(pa):
    """a fresh handle has nothing to report (a handle needs a device: without one its creation is what fails)"""
    lib = pa.load()
    if lib.ps_device_count() <= 0:
        with pytest.raises(pa.PansimError) as e:
            pa.Population(4, 16, 4, True, 0.0, 0, 0)
        assert e.value.code == PS_ERR_NO_DEVICE
        return
    core = pa.Population(4, 16, 4, True, 0.0, 0, 0)
    with pytest.raises(pa.PansimError) as e:
        core.linkage_tree_timing()
    assert e.value.code == PS_ERR_STATE and "no linkage tree" in str(e.value)
    core.close()


def cli(*args):
    return subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=60)


def test_cli_rejects_a_bad_metric(pa):
    """checked before any device work, whether or not --print_tree is given"""
    for extra in ((), ("--print_tree",)):
        r = cli("--tree_metric", "bogus", "--pan_genes", 3000, *extra)
        assert r.returncode == 101 and r.stdout == "" and "--tree_metric" in r.stderr and "core or acc" in r.stderr, (r.returncode, r.stderr)


def test_cli_flag_shapes(pa):
    r = cli("--print_tree=1")
    assert r.returncode == 2 and "takes no value" in r.stderr
    r = cli("--tree_metric")
    assert r.returncode == 2 and "requires a value" in r.stderr


def test_help_extensions_lists_the_tree_flags(pa):
    r = cli("--help-extensions")
    assert r.returncode == 0
    assert "--print_tree\n" in r.stdout and "_tree.tsv" in r.stdout and "_tree_summary.tsv" in r.stdout
    assert "--tree_metric <tree_metric>\n" in r.stdout and "[default: core]" in r.stdout
    r = cli("--help")
    assert r.returncode == 0 and "tree" not in r.stdout
    assert r.stdout[r.stdout.index("USAGE:"):] == open(os.path.join(ROOT, "tests", "golden", "help_usage.txt")).read()
