"""The average-linkage (UPGMA) tree without a device (docs/UPGMA_TREE.md): ps_upgma_from_counts against the plain-integer
sequential algorithm (tests/upgma_tree_ref.py), ties, equal ratios, cross products beyond 64 bits, its error paths, the rounds
argument restated, cut / clusters_at / cophenetic against brute force, the Newick text, the no-device errors of the device
entries and the CLI's flag checks and help texts.  The device half is tests/test_gpu_upgma_tree.py.  Every comparison of trees
is an equality of integer arrays and integer fields."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import upgma_tree_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_NO_DEVICE, PS_ERR_STATE = -1, -2, -6
NEW_SYMBOLS = ("ps_upgma_tree", "ps_sim_upgma_tree", "ps_multi_upgma_tree", "ps_upgma_from_counts", "ps_upgma_newick", "ps_upgma_tree_timing")
METRICS = (("core", ref.CORE), ("acc", ref.ACC))


def numerators(rng, P, hmax, G):
    """h of either parity below hmax, intersections at most unions, unions at most G"""
    h = rng.integers(0, hmax, P, dtype=np.uint32)
    u = rng.integers(0, G + 1, P, dtype=np.uint32)
    i = np.minimum((rng.random(P) * (u + 1)).astype(np.uint32), u)
    return h, i, u


def shuffled_pairs(rng, N):
    """the complete list in a shuffled order, either orientation"""
    r1, r2 = ref.all_pairs(N)
    order, swap = rng.permutation(r1.size), rng.random(r1.size) < 0.5
    return np.where(swap, r2, r1)[order].astype(np.uint32), np.where(swap, r1, r2)[order].astype(np.uint32)


def check(pa, r1, r2, h, i, u, N, L, cg):
    """both metrics against the reference -> the two results"""
    out = []
    for name, metric in METRICS:
        got = pa.upgma_from_counts(r1, r2, h, i, u, N, L, cg, metric=name)
        ref.assert_equal(got, ref.tree(metric, r1, r2, h, i, u, N, L, cg), N)
        ref.assert_monotone(got)
        assert got.rounds == 0 and got.metric == metric and got.pairs == N * (N - 1) // 2
        out.append(got)
    return out


@pytest.mark.parametrize("N", [2, 3, 5, 40])
def test_complete_lists_equal_the_sequential_algorithm(pa, N):
    """random numerators over the complete list (shuffled, either orientation), few distinct values: many ties"""
    rng = np.random.default_rng(N)
    a, b = shuffled_pairs(rng, N)
    for hmax, G in ((8, 3), (600, 70)):
        h, i, u = numerators(rng, a.size, hmax, G)
        for cg in (1, 5):
            check(pa, a, b, h, i, u, N, 300, cg)
    # the numerators of the other metric may be left out
    h, i, u = numerators(rng, a.size, 8, 3)
    got = pa.upgma_from_counts(a, b, h, None, None, N, 300, 5, metric="core")
    ref.assert_equal(got, ref.tree(ref.CORE, a, b, h, i, u, N, 300, 5), N)
    got = pa.upgma_from_counts(a, b, None, i, u, N, 300, 5, metric="acc")
    ref.assert_equal(got, ref.tree(ref.ACC, a, b, h, i, u, N, 300, 5), N)


def test_all_ties_give_the_caterpillar(pa):
    """every pair at one distance: row 0's cluster takes leaf 1, 2, ... in turn"""
    N = 9
    a, b = shuffled_pairs(np.random.default_rng(3), N)
    c = np.full(a.size, 6, np.uint32)
    for got in check(pa, a, b, c, c // 2, c, N, 10, 4):
        assert list(got.left) == [0] + [N + k for k in range(N - 2)] and list(got.right) == list(range(1, N))
        assert list(got.size) == list(range(2, N + 1)) and got.distinct_heights == 1
    core, acc = check(pa, a, b, c, c // 2, c, N, 10, 4)
    assert list(core.num) == [3 * k for k in range(1, N)] and list(core.den) == [10 * k for k in range(1, N)]
    assert list(acc.num) == [3 * k for k in range(1, N)] and list(acc.den) == [10 * k for k in range(1, N)]
    assert (core.root_num, core.root_den) == (24, 80)


def test_equal_ratios_tie_and_the_ids_decide(pa):
    """1 / 2 and 2 / 4 are one height: whichever pair carries which fraction, the smaller ids merge first"""
    arr = lambda *v: np.array(v, np.uint32)
    r1, r2 = arr(0, 0, 1), arr(1, 2, 2)
    # with one core gene: (U, I) = (1, 0) -> 1 / 2, (3, 1) -> 2 / 4, (4, 1) -> 3 / 5
    cases = ((arr(1, 3, 4), arr(0, 1, 1), (0, 1), (5, 9)), (arr(3, 1, 4), arr(1, 0, 1), (0, 1), (4, 7)), (arr(4, 3, 1), arr(1, 1, 0), (0, 2), (4, 7)))
    for u, i, first, rest in cases:
        got = pa.upgma_from_counts(r1, r2, None, i, u, 3, 10, 1, metric="acc")
        ref.assert_equal(got, ref.tree(ref.ACC, r1, r2, u, i, u, 3, 10, 1), 3)
        assert (got.left[0], got.right[0]) == first and got.num[0] * 2 == got.den[0]
        assert (got.left[1], got.right[1]) == ((3, 2) if first == (0, 1) else (3, 1)) and got.distinct_heights == 2
        assert (got.num[1], got.den[1]) == rest              # the pooled distance of the other two pairs: sum of a / sum of b
    # a strictly smaller ratio with larger numbers comes first: 3 / 7 < 1 / 2
    got = pa.upgma_from_counts(r1, r2, None, arr(0, 3, 1), arr(1, 6, 4), 3, 10, 1, metric="acc")
    assert (got.left[0], got.right[0], got.num[0], got.den[0]) == (0, 2, 3, 7)


def test_cross_products_beyond_64_bits_still_order(pa):
    """three groups of 1024, 1000 and 1048 individuals far apart under the core metric (L = 2^31): the last two merges compare
    sums near 2^50 over sizes near 2^20, cross products near 2^70.  The values are chosen so that the products cut to 64 bits
    would pick another pair, which the test asserts of its own construction.  The groups' insides (random small distances) are
    not looked at here; the expected top of the tree follows from the sums."""
    rng = np.random.default_rng(50)
    sizes, L = (1024, 1000, 1048), 2**31
    N = sum(sizes)
    group = np.repeat(np.arange(3), sizes).astype(np.uint32)
    r1, r2 = ref.all_pairs(N)
    g1, g2 = group[r1], group[r2]
    h = (2 * rng.integers(1, 1000, r1.size)).astype(np.uint32)
    d = {(0, 1): 2**30 + 1060921, (0, 2): 2**30 - 3308692, (1, 2): 2**30 + 2**26}
    for (x, y), v in d.items():
        h[(g1 == x) & (g2 == y)] = 2 * v
    T = {k: sizes[k[0]] * sizes[k[1]] * v for k, v in d.items()}
    D = {k: sizes[k[0]] * sizes[k[1]] for k in d}
    assert min(T.values()) > 2**49 and min(D.values()) > 2**19 and T[0, 2] * D[0, 1] > 2**64
    true_first = min(d, key=lambda k: d[k])
    assert true_first == (0, 2)
    cut = lambda x: x % 2**64
    assert cut(T[0, 1] * D[0, 2]) < cut(T[0, 2] * D[0, 1])          # (in 64 bits (0, 1) would have looked closer)
    got = pa.upgma_from_counts(r1, r2, h, None, None, N, L, 1)
    assert (int(got.num[-2]), int(got.den[-2]), int(got.size[-2])) == (T[0, 2], D[0, 2] * L, sizes[0] + sizes[2])
    assert (int(got.num[-1]), int(got.den[-1]), int(got.size[-1])) == (T[0, 1] + T[1, 2], (sizes[0] + sizes[2]) * sizes[1] * L, N)
    assert (got.root_num, got.root_den) == (int(got.num[-1]), int(got.den[-1]))
    sets = ref.members(got)
    assert sets[int(got.left[-2])] == list(range(1024)) and sets[int(got.right[-2])] == list(range(2024, N))
    assert sets[int(got.right[-1])] == list(range(1024, 2024)) and int(got.left[-1]) == 2 * N - 3
    num, den = [int(x) for x in got.num], [int(x) for x in got.den]
    assert all(num[k] * den[k + 1] <= num[k + 1] * den[k] for k in range(N - 2))


@pytest.mark.parametrize("name,metric", METRICS)
def test_heights_are_monotone(pa, name, metric):
    """both linkages are reducible: no merge below the one before it, no node below a child (a wide range: few ties)"""
    rng = np.random.default_rng(17)
    N = 60
    a, b = shuffled_pairs(rng, N)
    h, i, u = numerators(rng, a.size, 6000, 60000)
    got = pa.upgma_from_counts(a, b, h, i, u, N, 3000, 5, metric=name)
    ref.assert_monotone(got)
    assert got.distinct_heights > N // 2
    height = [(0, 1)] * N + [(int(n), int(d)) for n, d in zip(got.num, got.den)]
    for k in range(N - 1):
        for c in (int(got.left[k]), int(got.right[k])):
            assert height[c][0] * height[N + k][1] <= height[N + k][0] * height[c][1]


def test_error_paths(pa):
    lib = pa.load()
    P, T = pa._lib.TreeParams, pa._lib.Upgma
    arr = lambda *v: np.array(v, np.uint32)
    base = dict(r1=arr(0, 1, 0), r2=arr(1, 2, 2), h=arr(4, 6, 2), i=arr(1, 2, 0), u=arr(3, 2, 5), left=np.zeros(3, np.uint32),
                right=np.zeros(3, np.uint32), size=np.zeros(3, np.uint32), num=np.zeros(3, np.uint64), den=np.zeros(3, np.uint64))
    out = T()

    def call(prm, n=3, N=3, o=out, cg=1, L=10, **kw):
        a = dict(base, **kw)
        ptr = lambda x: None if x is None else x.ctypes.data
        return lib.ps_upgma_from_counts(ptr(a["r1"]), ptr(a["r2"]), ptr(a["h"]), ptr(a["i"]), ptr(a["u"]), n, N, L, cg,
                                        C.byref(prm) if prm is not None else None, C.byref(o) if o is not None else None, ptr(a["left"]),
                                        ptr(a["right"]), ptr(a["size"]), ptr(a["num"]), ptr(a["den"]))

    def fails(text, *args, **kw):
        assert call(*args, **kw) == PS_ERR_INVALID
        assert text in lib.ps_last_error().decode(), lib.ps_last_error().decode()

    core, acc = P(0), P(1)
    assert call(core) == 0 and call(acc) == 0
    for metric in (2, -1, 7):
        fails("PS_TREE_CORE (0) or PS_TREE_ACC (1)", P(metric))
    for prm in (core, acc):
        fails("complete list of all 3 pairs", prm, n=2)                              # incomplete
        fails("the pair (0, 1) is listed twice", prm, r1=arr(0, 1, 1), r2=arr(1, 2, 0))  # duplicate (and so one missing)
        fails("pair 1: index 3 is not below pop_size 3", prm, r2=arr(1, 3, 2))
        fails("pair 0: index 7 is not below pop_size 3", prm, r1=arr(7, 1, 0))
        fails("pair 1: both indices are 1", prm, r2=arr(1, 1, 2))
        fails("pop_size <= 16384", prm, N=16385)
        fails("pop_size", prm, N=1, n=0)
        for kw in (dict(r1=None), dict(r2=None), dict(left=None), dict(right=None), dict(size=None), dict(num=None), dict(den=None),
                   dict(o=None)):
            fails("null", prm, **kw)
    fails("pair 1: intersection 3 above union 2", acc, i=arr(1, 3, 0))
    assert call(core, i=arr(1, 3, 0)) == 0                      # (the accessory numerators are not looked at)
    fails("65535 accessory genes", acc, u=arr(3, 65536, 5))
    assert call(acc, u=arr(3, 65535, 5)) == 0
    fails("core_genes >= 1", acc, cg=0)
    assert call(core, cg=0) == 0
    fails("core_genes + 65535 < 2^32", acc, cg=2**32 - 65535)
    assert call(acc, cg=2**32 - 65536) == 0
    fails("null", core, h=None)
    fails("null", acc, i=None)
    fails("null", acc, u=None)
    fails("null", None)
    with pytest.raises(ValueError):
        pa.upgma_from_counts(base["r1"], base["r2"], base["h"], base["i"], base["u"], 3, 10, 1, metric="joint")
    with pytest.raises(ValueError):
        pa.upgma_from_counts(base["r1"], base["r2"][:-1], base["h"], base["i"], base["u"], 3, 10, 1)
    with pytest.raises(pa.PansimError) as e:
        pa.upgma_from_counts(base["r1"][:2], base["r2"][:2], base["h"][:2], None, None, 3, 10, 1)
    assert e.value.code == PS_ERR_INVALID and "average linkage is undefined on a partial list" in str(e.value)


def test_the_rounds_give_the_sequential_list():
    """the argument the device rests on, restated in Python: rounds of mutual nearest neighbours, then the ordering step, give
    the list of the sequential algorithm -- on matrices of 2 .. 11 individuals with values in 0 .. 3 (heavy ties), plain and
    pooled"""
    rng = np.random.default_rng(2024)
    fewer = 0
    for trial in range(300):
        N = int(rng.integers(2, 12))
        r1, r2 = ref.all_pairs(N)
        h = (2 * rng.integers(0, 4, r1.size)).astype(np.uint32)
        u = rng.integers(0, 4, r1.size).astype(np.uint32)
        i = np.minimum(rng.integers(0, 4, r1.size), u).astype(np.uint32)
        for metric in (ref.CORE, ref.ACC):
            want = ref.tree(metric, r1, r2, h, i, u, N, 7, 1)
            got, taken = ref.tree_by_rounds(metric, r1, r2, h, i, u, N, 7, 1)
            assert 1 <= taken <= N - 1
            fewer += taken < N - 1
            for name in want:
                assert np.array_equal(want[name], got[name]), (trial, metric, name)
    assert fewer > 100                                          # (the rounds do merge several pairs at a time)


@pytest.mark.parametrize("name,metric", METRICS)
def test_cut_clusters_at_and_cophenetic_against_the_member_sets(pa, name, metric):
    """at every merge height, just below it and below all: the labels are the smallest row of the largest node at or below the
    threshold that holds the row; the cophenetic distance of a pair is that of the smallest node that holds both"""
    rng = np.random.default_rng(23)
    N = 30
    a, b = shuffled_pairs(rng, N)
    h, i, u = numerators(rng, a.size, 40, 12)                   # (some ties among the heights)
    got = pa.upgma_from_counts(a, b, h, i, u, N, 50, 2, metric=name)
    sets = ref.members(got)
    heights = [(int(n), int(d)) for n, d in zip(got.num, got.den)]
    cuts = set(heights) | {(n * 1000 - 1, d * 1000) for n, d in heights if n > 0} | {(0, 1), (heights[-1][0] + 1, heights[-1][1])}
    seen = set()
    for tn, td in sorted(cuts):
        kept = [k for k, (n, d) in enumerate(heights) if n * td <= tn * d]
        assert kept == list(range(len(kept)))                   # (a prefix: the heights are monotone)
        want = np.arange(N, dtype=np.uint32)
        for k in kept:                                          # (ascending: a later node overwrites the ones below it)
            want[sets[N + k]] = sets[N + k][0]
        assert np.array_equal(got.cut(tn, td), want), (tn, td)
        assert got.clusters_at(tn, td) == N - len(kept) == len(set(want.tolist()))
        seen.add(len(kept))
    assert N - 1 in seen and len(seen) >= got.distinct_heights      # (one more merge count per height; 0 kept unless a height is 0)
    r1, r2 = ref.all_pairs(N)
    num, den = got.cophenetic(r2, r1)
    for x, y, n, d in zip(r1.tolist(), r2.tolist(), num.tolist(), den.tolist()):
        first = min(k for k in range(N - 1) if x in sets[N + k] and y in sets[N + k])
        assert (n, d) == heights[first]
    assert num.dtype == den.dtype == np.uint64
    with pytest.raises(ValueError):
        got.cophenetic([0], [0])
    with pytest.raises(ValueError):
        got.cut(1, 0)


def test_newick_of_four_leaves_by_hand(pa):
    """(0, 1) at 2, (2, 3) at 4, both at 10: every branch is half the difference of the two heights"""
    lib = pa.load()
    left, right = np.array([0, 2, 4], np.uint32), np.array([1, 3, 5], np.uint32)
    num, den = np.array([2, 4, 10], np.uint64), np.ones(3, np.uint64)
    want = "((0:1,1:1):4,(2:2,3:2):3);"
    assert pa.upgma_newick(left, right, num, den, 4) == want
    need = C.c_uint64()
    args = (left.ctypes.data, right.ctypes.data, num.ctypes.data, den.ctypes.data, 4)
    assert lib.ps_upgma_newick(*args, None, 0, C.byref(need)) == 0 and need.value == len(want) + 1
    buf = C.create_string_buffer(need.value)
    assert lib.ps_upgma_newick(*args, buf, need.value - 1, C.byref(need)) == PS_ERR_INVALID and "terminating zero" in lib.ps_last_error().decode()
    assert lib.ps_upgma_newick(*args, buf, need.value, C.byref(need)) == 0 and buf.value.decode() == want
    # fractions and a right child that is a leaf: 1 / 2, 3 / 4, 5 / 4
    assert pa.upgma_newick([0, 4, 5], [1, 2, 3], [1, 3, 5], [2, 4, 4], 4) == "(((0:0.25,1:0.25):0.125,2:0.375):0.25,3:0.625);"
    # children that are no earlier free node, null pointers
    bad = np.array([0, 2, 5], np.uint32)
    assert lib.ps_upgma_newick(bad.ctypes.data, *args[1:], None, 0, C.byref(need)) == PS_ERR_INVALID
    twice = np.array([0, 0, 4], np.uint32)
    assert lib.ps_upgma_newick(twice.ctypes.data, *args[1:], None, 0, C.byref(need)) == PS_ERR_INVALID
    assert lib.ps_upgma_newick(None, *args[1:], None, 0, C.byref(need)) == PS_ERR_INVALID
    assert lib.ps_upgma_newick(*args, None, 0, None) == PS_ERR_INVALID


def test_newick_of_a_caterpillar_of_3000_leaves(pa):
    """as deep as the population: the walk keeps its own stack"""
    N = 3000
    left = np.array([0] + list(range(N, 2 * N - 2)), np.uint32)
    right = np.arange(1, N, dtype=np.uint32)
    num, den = np.ones(N - 1, np.uint64), np.full(N - 1, 4, np.uint64)         # (every merge at 1 / 4, as all ties give)
    text = pa.upgma_newick(left, right, num, den, N)
    assert text.startswith("(" * (N - 1) + "0:0.125,1:0.125):0,2:0.125):0,") and text.endswith(",%d:0.125);" % (N - 1))
    assert text.count("(") == text.count(")") == N - 1 and text.count(",") == N - 1


def test_every_new_symbol_is_exported_and_declared(pa):
    lib = C.CDLL(pa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pansim_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in pa._lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
        assert "fn %s(" % name in integration, name
        comment = hdr[:hdr.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert "reference has no such function" in comment and "population.rs:787-837" in comment, name
    assert lib.ps_abi_version() == 3
    fields = re.search(r"typedef struct \{([^}]*)\} ps_upgma_t;", hdr).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields)) == [n for n, _ in pa._lib.Upgma._fields_]
    assert pa.UpgmaTree.FIELDS == tuple(n for n, _ in pa._lib.Upgma._fields_)


def test_the_device_entries_need_a_device(pa):
    """without a device the three device entries fail with PS_ERR_NO_DEVICE before they look at their arguments; with one,
    the same calls refuse their null arguments"""
    lib = pa.load()
    out, prm = pa._lib.Upgma(), pa._lib.TreeParams(0)
    lo, num = np.zeros(16, np.uint32), np.zeros(16, np.uint64)
    tail = (C.byref(prm), C.byref(out), lo.ctypes.data, lo.ctypes.data, lo.ctypes.data, num.ctypes.data, num.ctypes.data)
    want = PS_ERR_NO_DEVICE if lib.ps_device_count() <= 0 else PS_ERR_INVALID
    assert lib.ps_upgma_tree(None, None, *tail) == want
    assert lib.ps_sim_upgma_tree(None, *tail) == want
    assert lib.ps_multi_upgma_tree(None, *tail) == want
    if want == PS_ERR_NO_DEVICE:
        assert "no HIP device" in lib.ps_last_error().decode()
        bad = pa._lib.TreeParams(9)                              # ... and before the parameters
        assert lib.ps_upgma_tree(None, None, C.byref(bad), *tail[1:]) == PS_ERR_NO_DEVICE
    assert lib.ps_upgma_tree_timing(None, None, None, None) == PS_ERR_INVALID


def cli(*args):
    return subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=60)


def test_cli_rejects_a_bad_metric(pa):
    """checked before any device work, whether or not --print_upgma is given"""
    for extra in ((), ("--print_upgma",)):
        r = cli("--upgma_metric", "bogus", "--pan_genes", 3000, *extra)
        assert r.returncode == 101 and r.stdout == "" and "--upgma_metric" in r.stderr and "core or acc" in r.stderr, (r.returncode, r.stderr)


def test_cli_checks_the_limits_before_the_run(pa):
    """what the flags already decide -- pop_size above 16384, the accessory metric without core genes -- ends the run before any
    device work, and only when --print_upgma is given"""
    r = cli("--print_upgma", "--pop_size", 16385)
    assert r.returncode == 101 and r.stdout == "" and "--print_upgma needs 2 <= pop_size <= 16384" in r.stderr, (r.returncode, r.stderr)
    r = cli("--print_upgma", "--upgma_metric", "acc", "--core_genes", 0, "--pan_genes", 100)
    assert r.returncode == 101 and r.stdout == "" and "--upgma_metric acc needs core_genes >= 1" in r.stderr, (r.returncode, r.stderr)


def test_cli_flag_shapes(pa):
    r = cli("--print_upgma=1")
    assert r.returncode == 2 and "takes no value" in r.stderr
    r = cli("--upgma_metric")
    assert r.returncode == 2 and "requires a value" in r.stderr


def test_help_extensions_lists_the_upgma_flags(pa):
    r = cli("--help-extensions")
    assert r.returncode == 0
    assert "--print_upgma\n" in r.stdout and "--upgma_metric <upgma_metric>\n" in r.stdout
    flat = " ".join(r.stdout.split())
    for name in ("<outpref>_upgma.tsv", "<outpref>_upgma.nwk", "<outpref>_upgma_summary.tsv"):
        assert name in flat, name
    r = cli("--help")
    assert r.returncode == 0 and "upgma" not in r.stdout
    assert r.stdout[r.stdout.index("USAGE:"):] == open(os.path.join(ROOT, "tests", "golden", "help_usage.txt")).read()


def test_the_restatement_agrees_with_scipy():
    """tie-free random matrices: the reference restatement's topology and heights against scipy's average linkage, to 1e-9
    relative.  This pins the restatement (tests/upgma_tree_ref.py), not the library."""
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    rng = np.random.default_rng(77)
    for N in (2, 7, 25):
        r1, r2 = ref.all_pairs(N)
        d = rng.choice(np.arange(1, 10**6), r1.size, replace=False)          # distinct: no ties between pairs
        want = hierarchy.linkage(d.astype(np.float64), "average")            # (the condensed form is the row-major i < j list)
        got = ref.tree(ref.CORE, r1, r2, (2 * d).astype(np.uint32), d, d, N, 1, 1)
        assert np.array_equal(np.minimum(got["left"], got["right"]), np.minimum(want[:, 0], want[:, 1]).astype(np.uint32))
        assert np.array_equal(np.maximum(got["left"], got["right"]), np.maximum(want[:, 0], want[:, 1]).astype(np.uint32))
        assert np.array_equal(got["size"], want[:, 3].astype(np.uint32))
        assert np.allclose(got["num"].astype(np.float64) / got["den"].astype(np.float64), want[:, 2], rtol=1e-9, atol=0.0)
