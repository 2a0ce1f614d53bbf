"""Group differentiation without a device (docs/GROUP_DIFFERENTIATION.md): the group rules of ps_groups_from_labels and the host
restatement ps_differentiation_from_counts against the numpy restatement (tests/group_differentiation_ref.py), their error
paths, the no-device errors of the device entries and the CLI's flag checks and help texts.  The device half is
tests/test_gpu_group_differentiation.py.  Every comparison of integers is an equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import group_differentiation_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_NO_DEVICE = -1, -2
NEW_SYMBOLS = ("ps_group_differentiation", "ps_sim_group_differentiation", "ps_multi_group_differentiation", "ps_groups_from_labels",
               "ps_differentiation_from_counts", "ps_group_differentiation_timing")


def check_groups(pa, labels, **kw):
    got = pa.groups_from_labels(labels, **kw)
    want = ref.groups(labels, **kw)
    for g, w in zip(got, want):
        assert g.dtype == np.uint32 and np.array_equal(g, w), (got, want)
    return got


def test_ranking_ties_go_to_the_smaller_label(pa):
    labels = [7, 3, 7, 3, 9, 9, 1, 9]
    group_of, label, size = check_groups(pa, labels)
    assert list(label) == [9, 3, 7, 1] and list(size) == [3, 2, 2, 1]
    assert list(group_of) == [2, 1, 2, 1, 0, 0, 3, 0]


def test_min_size_leaves_the_small_labels_unassigned(pa):
    labels = [5, 5, 5, 2, 2, 8, 0]
    group_of, label, size = check_groups(pa, labels, min_size=2)
    assert list(label) == [5, 2] and list(size) == [3, 2] and list(group_of) == [0, 0, 0, 1, 1, ref.UNASSIGNED, ref.UNASSIGNED]
    group_of, label, size = check_groups(pa, labels, min_size=3)
    assert list(label) == [5] and (group_of[3:] == ref.UNASSIGNED).all()


def test_truncation_at_max_groups(pa):
    """20 distinct labels of sizes 1 .. 20: the 16 largest are the groups, the 4 smallest unassigned; and fewer on request"""
    labels = np.repeat(np.arange(100, 120, dtype=np.uint32), np.arange(1, 21))
    labels = labels[np.random.default_rng(1).permutation(labels.size)]
    group_of, label, size = check_groups(pa, labels)
    assert list(label) == list(range(119, 103, -1)) and list(size) == list(range(20, 4, -1))
    assert (group_of == ref.UNASSIGNED).sum() == 1 + 2 + 3 + 4
    group_of, label, size = check_groups(pa, labels, max_groups=3)
    assert list(label) == [119, 118, 117]


def test_large_unsorted_label_values(pa):
    labels = np.array([4_000_000_000, 5, 4_000_000_000, 2**32 - 1, 5, 4_000_000_000, 0], np.uint32)
    group_of, label, size = check_groups(pa, labels)
    assert list(label) == [4_000_000_000, 5, 0, 2**32 - 1] and list(size) == [3, 2, 1, 1]
    assert list(group_of) == [0, 1, 0, 3, 1, 0, 2]


def test_no_group_is_an_error(pa):
    for labels, kw in (([1, 2, 3], dict(min_size=2)), ([], dict())):
        with pytest.raises(pa.PansimError) as e:
            pa.groups_from_labels(labels, **kw)
        assert e.value.code == PS_ERR_INVALID and "no groups" in str(e.value)
    lib = pa.load()
    lab, out = np.arange(4, dtype=np.uint32), np.zeros(32, np.uint32)
    K = C.c_uint32()
    for max_groups, min_size, text in ((0, 1, "max_groups"), (17, 1, "max_groups"), (4, 0, "min_size")):
        assert lib.ps_groups_from_labels(lab.ctypes.data, 4, max_groups, min_size, out.ctypes.data, out.ctypes.data, out.ctypes.data,
                                         C.byref(K)) == PS_ERR_INVALID
        assert text in lib.ps_last_error().decode()
    assert lib.ps_groups_from_labels(lab.ctypes.data, 4, 4, 1, None, out.ctypes.data, out.ctypes.data, C.byref(K)) == PS_ERR_INVALID
    for bad in (dict(max_groups=0), dict(max_groups=17), dict(min_size=0)):
        with pytest.raises(ValueError):
            pa.groups_from_labels(lab, **bad)


def random_counts(rng, L, sizes, other=0.1):
    """(L, K, 5) class counts that add up to the sizes: a multinomial per (site, group), `other` the last class"""
    c = np.zeros((L, len(sizes), 5), np.int64)
    for g, n in enumerate(sizes):
        p = rng.dirichlet(np.full(4, 0.3), L) * (1.0 - other)
        c[:, g, :] = rng.multinomial(n, np.concatenate([p, np.full((L, 1), other)], 1))
    return c


@pytest.mark.parametrize("sizes", [(37,), (1, 40), (50, 7, 1), tuple(range(16, 0, -1)), (65536,), (32768, 32767, 1)])
def test_from_counts_equals_the_restatement(pa, sizes):
    """K = 1, a group of one, K = 16, `other` cells, and the largest population (n^2 = 2^32)"""
    rng = np.random.default_rng(len(sizes) + sizes[0])
    c = random_counts(rng, 211, sizes)
    c[0], c[1] = 0, 0
    c[0, :, 0] = sizes                       # a monomorphic site
    c[1, :, 4] = sizes                       # a site of `other` only
    c[2] = 0
    c[2, np.arange(len(sizes)), 1 + (np.arange(len(sizes)) & 1)] = sizes     # a fixed difference between the even and the odd groups
    want = ref.from_class_counts(c, sizes)
    got = pa.differentiation_from_counts(c[:, :, :4], sizes)
    ref.assert_equal(got, want)
    assert got.pop_size == got.assigned == sum(sizes) and got.unassigned == 0 and got.genes == 0
    assert got.other_cells > 0 and np.array_equal(got.between, got.between.T) and np.array_equal(got.fixed, got.fixed.T)
    assert (np.diag(got.fixed) >= 3).all()
    if len(sizes) > 1:
        assert got.fixed[0, 1] >= 1 and got.fixed[0, 0] >= 3
    # the pooled identity: the differences over all pairs are those of the pooled counts
    pooled = pa.diversity_from_counts(c[:, :, :4].sum(1), sum(sizes))
    assert int(np.triu(got.between).sum()) == pooled["pair_differences"] == int(got.site_total.sum(dtype=np.uint64))
    assert got.within_differences == int(got.site_within.sum(dtype=np.uint64))
    # the ratios of the wrapper
    n = np.array(sizes, np.float64)
    if len(sizes) > 1:
        assert got.dxy()[0, 1] == float(got.between[0, 1]) / (n[0] * n[1] * 211)
    assert np.array_equal(np.diag(got.dxy()), got.pi()) and got.site_fst().shape == (211,)
    d = got.as_dict()
    assert d["between"] is got.between and d["groups"] == len(sizes) and d["fst"] == got.fst


def test_no_sites_and_no_pairs(pa):
    got = pa.differentiation_from_counts(np.zeros((0, 2, 4), np.uint32), [3, 1])
    assert got.sites == 0 and got.pi_within == got.pi_between == got.fst == 0.0 and not got.between.any()
    got = pa.differentiation_from_counts(np.array([[[1, 0, 0, 0]]], np.uint32), [1])
    assert got.within_pairs == got.between_pairs == 0 and got.pi_within == got.fst == 0.0 and got.fixed[0, 0] == 1


def test_overfull_counts_and_bad_shapes_are_refused(pa):
    c = np.zeros((3, 2, 4), np.uint32)
    c[:, 0, 0], c[:, 1, 1] = 5, 4
    assert pa.differentiation_from_counts(c, [5, 4]).fixed[0, 1] == 3
    c[2, 1, 3] = 1
    with pytest.raises(pa.PansimError) as e:
        pa.differentiation_from_counts(c, [5, 4])
    assert e.value.code == PS_ERR_INVALID and "site 2 in group 1" in str(e.value)
    with pytest.raises(pa.PansimError) as e:
        pa.differentiation_from_counts(np.zeros((1, 2, 4), np.uint32), [65536, 1])
    assert e.value.code == PS_ERR_INVALID and "65536" in str(e.value)
    for counts, sizes in ((np.zeros((3, 2, 3)), [1, 1]), (np.zeros((3, 2, 4)), [1, 1, 1]), (np.zeros((3, 17, 4)), [1] * 17), (np.zeros((3, 4)), [1])):
        with pytest.raises(ValueError):
            pa.differentiation_from_counts(counts, sizes)
    lib = pa.load()
    out, n, m = pa._lib.Diff(), np.ones(2, np.uint32), np.zeros(4, np.uint64)
    assert lib.ps_differentiation_from_counts(None, 1, 2, n.ctypes.data, C.byref(out), m.ctypes.data, m.ctypes.data, None, None) == PS_ERR_INVALID
    assert lib.ps_differentiation_from_counts(None, 0, 0, n.ctypes.data, C.byref(out), m.ctypes.data, m.ctypes.data, None, None) == PS_ERR_INVALID
    assert lib.ps_differentiation_from_counts(None, 0, 2, n.ctypes.data, C.byref(out), m.ctypes.data, m.ctypes.data, None, None) == 0


def test_every_new_symbol_is_exported_and_declared(pa):
    lib = C.CDLL(pa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pansim_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in pa._lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
    assert lib.ps_abi_version() == 3
    assert "#define PS_GROUPS_MAX 16" in hdr and pa._lib.PS_GROUPS_MAX == 16


def test_the_device_entries_need_a_device(pa):
    """without a device the three device entries fail with PS_ERR_NO_DEVICE before they look at their arguments; with one,
    the same calls refuse their null arguments"""
    lib = pa.load()
    out, prm = pa._lib.Diff(), pa._lib.DiffParams(16, 1)
    a = np.zeros(256, np.uint64)
    rest = [a.ctypes.data] * 5 + [None] * 7
    want = PS_ERR_NO_DEVICE if lib.ps_device_count() <= 0 else PS_ERR_INVALID
    assert lib.ps_group_differentiation(None, None, a.ctypes.data, C.byref(prm), C.byref(out), *rest) == want
    assert lib.ps_sim_group_differentiation(None, a.ctypes.data, C.byref(prm), C.byref(out), *rest) == want
    assert lib.ps_multi_group_differentiation(None, a.ctypes.data, C.byref(prm), C.byref(out), *rest) == want
    if want == PS_ERR_NO_DEVICE:
        assert "no HIP device" in lib.ps_last_error().decode()
        bad = pa._lib.DiffParams(0, 0)                           # ... and before the parameters
        assert lib.ps_group_differentiation(None, None, a.ctypes.data, C.byref(bad), C.byref(out), *rest) == PS_ERR_NO_DEVICE
    assert lib.ps_group_differentiation_timing(None, None, None, None) == PS_ERR_INVALID


def cli(*args):
    return subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=60)


def test_cli_needs_a_threshold(pa):
    r = cli("--print_differentiation", "--pan_genes", 3000)
    assert r.returncode == 101 and r.stdout == "" and "--cluster_core_max" in r.stderr and "--cluster_acc_max" in r.stderr, r.stderr
    r = cli("--print_differentiation", "--cluster_core_max", 0.1, "--pop_size", 65537, "--pan_genes", 3000)
    assert r.returncode == 101 and r.stdout == "" and "pop_size <= 65536" in r.stderr, r.stderr


@pytest.mark.parametrize("flag,value,text", [
    ("diff_max_groups", "0", "1 <= X <= 16"), ("diff_max_groups", "17", "1 <= X <= 16"), ("diff_max_groups", "x", "1 <= X <= 16"),
    ("diff_max_groups", "-1", "1 <= X <= 16"), ("diff_max_groups", "2.5", "1 <= X <= 16"), ("diff_min_size", "0", "a whole number >= 1"),
    ("diff_min_size", "-3", "a whole number >= 1"), ("diff_min_size", "two", "a whole number >= 1")])
def test_cli_rejects_bad_values(pa, flag, value, text):
    """checked before any device work, whether or not --print_differentiation is given"""
    for extra in ((), ("--print_differentiation", "--cluster_core_max", "0.1")):
        r = cli("--%s=%s" % (flag, value), "--pan_genes", 3000, *extra)
        assert r.returncode == 101 and r.stdout == "" and "--" + flag in r.stderr and text in r.stderr, (r.returncode, r.stderr)


def test_cli_flag_shapes(pa):
    r = cli("--print_differentiation=1")
    assert r.returncode == 2 and "takes no value" in r.stderr
    r = cli("--diff_min_size")
    assert r.returncode == 2 and "requires a value" in r.stderr


def test_help_extensions_lists_the_differentiation_flags(pa):
    r = cli("--help-extensions")
    assert r.returncode == 0
    assert "--print_differentiation\n" in r.stdout and "--diff_max_groups <diff_max_groups>\n" in r.stdout
    assert "--diff_min_size <diff_min_size>\n" in r.stdout
    for suffix in ("_diff_groups.tsv", "_diff_between.tsv", "_diff_sites.tsv", "_diff_genes.tsv", "_diff_summary.tsv"):
        assert suffix in r.stdout, suffix
    r = cli("--help")
    assert r.returncode == 0 and "print_differentiation" not in r.stdout and "diff_m" not in r.stdout
    assert r.stdout[r.stdout.index("USAGE:"):] == open(os.path.join(ROOT, "tests", "golden", "help_usage.txt")).read()
