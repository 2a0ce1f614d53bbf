"""Tree comparison without a device (docs/TREE_COMPARISON.md): the host form ps_tree_compare_from_merges against the numpy
restatement (tests/tree_compare_ref.py), the triplet sums against a literal enumeration of all triples, the identities of a
tree against itself and of swapped arguments, the marginals against the O(M) closed forms, ps_levels_from_heights, every error
with its message, the no-device errors of the device entries and the CLI's flag checks and help text.  The device half is
tests/test_gpu_tree_compare.py.  Integers and arrays are compared by equality; the doubles within 1e-12 of the same
expression over Python integers: the conversions, one sqrt and one divide each round at 2^-53 relative and |r| <= 1, which puts
1e-12 three orders above the error."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import tree_compare_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_NO_DEVICE = -1, -2
NEW_SYMBOLS = ("ps_tree_compare", "ps_sim_tree_compare", "ps_multi_tree_compare", "ps_tree_compare_from_merges", "ps_levels_from_heights",
               "ps_tree_compare_timing")
SIZES = (2, 3, 5, 12, 64, 300)
VALUES = ("absent", "ties", "genealogy")


def valued(rng, N, t, how, step=3):
    """the tree (left, right) with values: absent, runs of equal values, or replaced by a genealogy with its heights"""
    if how == "absent":
        return t
    if how == "ties":
        return (*t, ref.tied_values(len(t[0]), step))
    return ref.genealogy_tree(rng, N, beyond=0.1 if N >= 4 else 0.0)


@pytest.mark.parametrize("how", VALUES)
@pytest.mark.parametrize("N", SIZES)
def test_from_merges_equals_the_restatement(pa, N, how):
    """the five tree shapes in pairs; N <= 12 also against the enumeration of all triples"""
    rng = np.random.default_rng(N * 7 + len(how))
    ts = ref.trees(rng, N)
    pairs = list(itertools.product(ts, ts)) if N <= 64 else list(itertools.combinations_with_replacement(ts, 2))
    for x, y in pairs:
        a, b = valued(rng, N, ts[x], how), valued(rng, N, ts[y], "ties" if how == "genealogy" else how, 2)
        want = ref.compare(N, a, b, bins=(7, 5))
        ref.assert_equal(pa.tree_compare_from_merges(N, a, b, bins=(7, 5)), want)
        if N <= 12:
            assert ref.triples_brute_force(N, a, b) == (want["resolved_a"], want["resolved_b"], want["shared_triplets"]), (x, y)
        bare = pa.tree_compare_from_merges(N, a, b, bins=(7, 5), triplets=False)
        ref.assert_equal(bare, ref.compare(N, a, b, bins=(7, 5), triplets=False))
        assert bare.triples == bare.resolved_a == bare.shared_triplets == 0 and bare.triplet_recall == 0.0


@pytest.mark.parametrize("bins,spans", [((1, 1), (0, 0)), ((127, 127), (0, 0)), ((32, 32), (10, 1000)), ((1023, 15), (299, 7))])
def test_bins_and_spans(pa, bins, spans):
    rng = np.random.default_rng(3)
    N = 300
    a, b = ref.random_joining(rng, N), (*ref.random_joining(rng, N, 200), ref.tied_values(200, 5))
    got = pa.tree_compare_from_merges(N, a, b, bins=bins, spans=spans)
    ref.assert_equal(got, ref.compare(N, a, b, bins=bins, spans=spans))
    assert got.joint.shape == (bins[0] + 1, bins[1] + 1) and int(got.joint.sum()) == got.pairs
    assert (got.span_a, got.span_b) == (spans[0] or 299, spans[1] or 40)


@pytest.mark.parametrize("how", VALUES)
def test_a_tree_against_itself(pa, how):
    rng = np.random.default_rng(11)
    N = 64
    for name, t in ref.trees(rng, N).items():
        a = valued(rng, N, t, how)
        got = pa.tree_compare_from_merges(N, a, a, bins=(16, 16))
        assert got.shared_triplets == got.resolved_a == got.resolved_b, name
        assert got.rf_distance == 0 and got.shared_clades == got.clades_a == got.clades_b, name
        assert got.joined_a_only == got.joined_b_only == 0
        assert got.cophenetic_r == (1.0 if got.joined_both * got.sum_aa != got.sum_a ** 2 else 0.0), name
        assert not (got.joint - np.diag(np.diag(got.joint))).any(), name
        assert got.clade_recall == got.clade_precision == 1.0 and (got.in_b == got.in_a).all()
        if got.resolved_a:
            assert got.triplet_recall == got.triplet_precision == 1.0


def test_swapped_arguments(pa):
    rng = np.random.default_rng(12)
    N = 65
    ts = ref.trees(rng, N)
    a, b = (*ts["forest"], ref.tied_values(len(ts["forest"][0]))), ref.genealogy_tree(rng, N, beyond=0.05)
    x, y = pa.tree_compare_from_merges(N, a, b, bins=(9, 4), spans=(50, 0)), pa.tree_compare_from_merges(N, b, a, bins=(4, 9), spans=(0, 50))
    np.testing.assert_array_equal(x.joint, y.joint.T)
    np.testing.assert_array_equal(x.in_b, y.in_a)
    np.testing.assert_array_equal(x.in_a, y.in_b)
    swap = dict(merges_a="merges_b", joined_a_only="joined_b_only", sum_a="sum_b", sum_aa="sum_bb", resolved_a="resolved_b", clades_a="clades_b",
                bins_a="bins_b", span_a="span_b", triplet_recall="triplet_precision", clade_recall="clade_precision")
    swap.update({v: k for k, v in swap.items()})
    for name in ref.INT_FIELDS + ref.DOUBLES:
        assert getattr(x, name) == getattr(y, swap.get(name, name)), name
    assert x.joined_a_only != x.joined_b_only                                      # (the swap is visible)


@pytest.mark.parametrize("N", (5, 64, 300))
def test_marginals_against_the_closed_forms(pa, N):
    """resolved_a, sum_a, sum_aa over the pairs from sum_k |left_k| |right_k| {N - |top_k|, val_k, val_k^2}: against a spanning
    tree B every pair A joins is joined in both"""
    rng = np.random.default_rng(N)
    ts = ref.trees(rng, N)
    b = ts["balanced"]
    for name, t in ts.items():
        a = (*t, ref.tied_values(len(t[0])))
        got = pa.tree_compare_from_merges(N, a, b)
        joined, resolved, s1, s2 = ref.closed_forms(N, a)
        assert (got.joined_both, got.joined_a_only, got.resolved_a, got.sum_a, got.sum_aa) == (joined, 0, resolved, s1, s2), name
        assert got.joined_both + got.joined_b_only == N * (N - 1) // 2 and got.triples == N * (N - 1) * (N - 2) // 6


def test_levels_from_heights(pa):
    # equal fractions with different denominators, a strict increase, 0 / 0 above everything and equal to itself
    num = np.array([1, 2, 3, 1, 2 ** 63, 0, 0], np.uint64)
    den = np.array([2, 4, 6, 1, 2 ** 62, 0, 0], np.uint64)
    np.testing.assert_array_equal(pa.levels_from_heights(num, den), [1, 1, 1, 2, 3, 4, 4])
    # products beyond 64 bits are compared exactly
    big = np.array([2 ** 63 - 1, 2 ** 63], np.uint64), np.array([2 ** 63, 2 ** 63 + 1], np.uint64)
    np.testing.assert_array_equal(pa.levels_from_heights(*big), [1, 2])
    assert pa.levels_from_heights([], []).size == 0
    for bad in (([2, 1], [1, 1]), ([0, 5], [0, 1]), ([1, 1], [2, 3])):
        with pytest.raises(pa.PansimError) as e:
            pa.levels_from_heights(*bad)
        assert e.value.code == PS_ERR_INVALID and "must not decrease" in str(e.value)
    distinct = C.c_uint64()
    assert pa.load().ps_levels_from_heights(num.ctypes.data, den.ctypes.data, 7, np.zeros(7, np.uint32).ctypes.data, C.byref(distinct)) == 0
    assert distinct.value == 4
    assert pa.load().ps_levels_from_heights(None, None, 3, None, None) == PS_ERR_INVALID


CAT = ([0, 5, 6], [1, 2, 3])                     # five leaves, three merges, leaf 4 uncovered


@pytest.mark.parametrize("kw,text", [
    (dict(a=([0, 0], [1, 2])), "is a child of merge"),
    (dict(a=([3], [3])), "with itself"),
    (dict(a=([0, 9], [1, 2])), "not a node below"),
    (dict(a=([], [])), "1 .. 4 merges"),
    (dict(N=1, a=([0], [0])), "2 <= pop_size <= 16384"),
    (dict(N=16385), "2 <= pop_size <= 16384"),
    (dict(b=(*CAT, [1, 0, 3])), "outside 1 .. 262143"),
    (dict(b=(*CAT, [1, 2, 262144])), "outside 1 .. 262143"),
    (dict(a=(*CAT, [2, 1, 3])), "must not descend towards the root (1 .. 262143)"),
    (dict(bins=(0, 4)), "must be >= 1"),
    (dict(bins=(4, 1025)), "limit of 1024 bins per tree"),
    (dict(bins=(127, 128)), "exceeds the limit of 16384 bins"),
    (dict(spans=(0, 2 ** 32)), "limit of 2^32 - 1")])
def test_errors(pa, kw, text):
    args = dict(N=5, a=CAT, b=CAT, bins=(4, 4), spans=(0, 0))
    args.update(kw)
    with pytest.raises(pa.PansimError) as e:
        pa.tree_compare_from_merges(args["N"], args["a"], args["b"], bins=args["bins"], spans=args["spans"])
    assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)


def test_null_arguments_and_the_tied_message_names_the_tree(pa):
    lib = pa.load()
    l, r = (np.array(x, np.uint32) for x in CAT)
    prm, out, joint = pa._lib.TreeCompareParams(4, 4, 0, 0, 1), pa._lib.TreeCompare(), np.zeros(25, np.uint64)
    trees = [l.ctypes.data, r.ctypes.data, None, 3, l.ctypes.data, r.ctypes.data, None, 3]
    assert lib.ps_tree_compare_from_merges(5, *trees, C.byref(prm), C.byref(out), joint.ctypes.data, None, None) == 0
    assert out.joined_both == 6 and out.joined_neither == 4
    for bad in ((None, C.byref(out), joint.ctypes.data), (C.byref(prm), None, joint.ctypes.data), (C.byref(prm), C.byref(out), None)):
        assert lib.ps_tree_compare_from_merges(5, *trees, *bad, None, None) == PS_ERR_INVALID
        assert "null argument" in lib.ps_last_error().decode()
    trees[0] = None
    assert lib.ps_tree_compare_from_merges(5, *trees, C.byref(prm), C.byref(out), joint.ctypes.data, None, None) == PS_ERR_INVALID
    with pytest.raises(pa.PansimError) as e:
        pa.tree_compare_from_merges(5, CAT, (*CAT, [1, 0, 3]))
    assert "tree b" in str(e.value)


def test_symbols_and_struct(pa):
    lib = pa.load()
    for name in NEW_SYMBOLS:
        assert name in pa._lib.SIGNATURES and hasattr(lib, name), name
    assert lib.ps_abi_version() == 3
    assert C.sizeof(pa._lib.TreeCompare) == 30 * 8 and C.sizeof(pa._lib.TreeCompareParams) == 32


def test_the_device_entries_need_a_device(pa):
    """without a device the three device entries fail with PS_ERR_NO_DEVICE before they look at their arguments; with one,
    the same calls refuse their null arguments"""
    lib = pa.load()
    want = PS_ERR_NO_DEVICE if lib.ps_device_count() <= 0 else PS_ERR_INVALID
    rest = [None] * 3 + [0] + [None] * 3 + [0] + [None] * 5
    for fn in (lib.ps_tree_compare, lib.ps_sim_tree_compare, lib.ps_multi_tree_compare):
        assert fn(None, *rest) == want
        if want == PS_ERR_NO_DEVICE:
            assert "no HIP device" in lib.ps_last_error().decode()
    assert lib.ps_tree_compare_timing(None, None, None) == PS_ERR_INVALID


def test_result_classes_give_their_values(pa):
    """levels() of the two inferred trees: the dense ranks of their heights"""
    t = pa._lib.Upgma()
    t.pop_size, t.merges = 4, 3
    up = pa.UpgmaTree(t, np.array([0, 2, 4], np.uint32), np.array([1, 3, 5], np.uint32), np.array([2, 2, 4], np.uint32),
                      np.array([1, 2, 3], np.uint64), np.array([2, 4, 1], np.uint64))
    np.testing.assert_array_equal(up.levels(), [1, 1, 2])
    got = pa.tree_compare_from_merges(4, up, ([0, 2, 4], [1, 3, 5]))
    assert (got.clades_a, got.clades_b, got.shared_clades) == (3, 3, 3) and got.span_a == 2


def cli(*args):
    return subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args,text", [
    (("--print_tree_compare", "upgma"), "each of upgma, tree or genealogy"),
    (("--print_tree_compare", "upgma,nj"), "each of upgma, tree or genealogy"),
    (("--print_tree_compare", "tree,tree"), "two different trees"),
    (("--print_tree_compare", "genealogy,upgma"), "needs --print_genealogy"),
    (("--print_tree_compare", "upgma,genealogy", "--print_genealogy", 262144), "--print_genealogy <= 262143"),
    (("--print_tree_compare", "upgma,tree", "--pop_size", 16385), "2 <= pop_size <= 16384"),
    (("--print_tree_compare", "upgma,tree", "--pop_size", 1), "2 <= pop_size <= 16384"),
    (("--print_tree_compare", "upgma,tree", "--tree_compare_bins", "32"), "--tree_compare_bins must be <Ba>,<Bb>"),
    (("--print_tree_compare", "upgma,tree", "--tree_compare_bins", "0,4"), "at least 1 on both axes"),
    (("--print_tree_compare", "upgma,tree", "--tree_compare_bins", "127,128"), "at most 16384"),
    (("--print_tree_compare", "tree,upgma", "--upgma_metric", "acc", "--core_genes", 0), "core_genes >= 1")])
def test_cli_checks_come_before_device_work(pa, args, text):
    r = cli(*args, "--pan_genes", 3000)
    assert r.returncode == 101 and r.stdout == "" and text in r.stderr, (r.returncode, r.stderr)


def test_help_extensions_lists_the_flags(pa):
    r = cli("--help-extensions")
    assert r.returncode == 0 and "--print_tree_compare <print_tree_compare>\n" in r.stdout and "--tree_compare_bins <tree_compare_bins>\n" in r.stdout
    text = " ".join(r.stdout.split())
    for suffix in ("_tree_compare.tsv", "_tree_compare_clades.tsv", "_tree_compare_summary.tsv"):
        assert suffix in text, suffix
    assert "tree_compare" not in cli("--help").stdout
