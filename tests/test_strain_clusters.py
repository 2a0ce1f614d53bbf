"""Strain clusters without a device (docs/STRAIN_CLUSTERS.md): ps_clusters_from_counts against the plain-integer union-find
(tests/strain_clusters_ref.py), the boundary equalities of both criteria, its error paths, the no-device errors of the device
entries and the CLI's flag checks and help texts.  The device half is tests/test_gpu_strain_clusters.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import strain_clusters_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_NO_DEVICE = -1, -2
NEW_SYMBOLS = ("ps_strain_clusters", "ps_sim_strain_clusters", "ps_multi_strain_clusters", "ps_clusters_from_counts",
               "ps_strain_clusters_timing")


def random_pairs(rng, N, P, L, G):
    """P distinct pairs of N individuals with numerators: h of either parity, intersections at most unions"""
    r1, r2 = ref.all_pairs(N)
    pick = rng.permutation(r1.size)[:P]
    swap = rng.random(P) < 0.5                                   # (the list need not be i < j)
    a, b = np.where(swap, r2[pick], r1[pick]), np.where(swap, r1[pick], r2[pick])
    h = rng.integers(0, 2 * L + 2, P, dtype=np.uint32)
    u = rng.integers(0, 2 * G + 1, P, dtype=np.uint32)
    i = np.minimum((rng.random(P) * (u + 1)).astype(np.uint32), u)
    return a.astype(np.uint32), b.astype(np.uint32), h, i, u


def check(pa, r1, r2, h, i, u, N, L, cg, d=ref.NO_CORE, num=0, den=0):
    got = pa.clusters_from_counts(r1, r2, h, i, u, N, L, cg, core_max_d=d if d != ref.NO_CORE else None,
                                  acc_ratio=(num, den) if den else None)
    ref.assert_equal(got, ref.clusters(r1, r2, h, i, u, N, L, cg, d, num, den), N)
    assert got.rounds == 0
    return got


@pytest.mark.parametrize("seed,N,P", [(1, 60, 400), (2, 200, 500), (3, 200, 3000), (4, 2, 1)])
def test_from_counts_equals_the_union_find(pa, seed, N, P):
    """sparse lists (many clusters), dense ones (few), one pair; each criterion disabled in turn and both together"""
    rng = np.random.default_rng(seed)
    r1, r2, h, i, u = random_pairs(rng, N, P, 300, 70)
    u[: P // 10] = 0
    i[: P // 10] = 0                         # empty unions: undefined without core genes
    for cg in (0, 5):
        core = check(pa, r1, r2, h, i, u, N, 300, cg, d=40)
        acc = check(pa, r1, r2, h, i, u, N, 300, cg, num=1, den=3)
        both = check(pa, r1, r2, h, i, u, N, 300, cg, d=40, num=1, den=3)
        assert core.undefined_pairs == 0 and acc.undefined_pairs == both.undefined_pairs == (int((u == 0).sum()) if cg == 0 else 0)
        assert both.edges <= min(core.edges, acc.edges) and both.clusters >= max(core.clusters, acc.clusters)
    # the numerators of a criterion that is not applied may be left out
    got = pa.clusters_from_counts(r1, r2, h, None, None, N, 300, 5, core_max_d=40)
    assert np.array_equal(got.labels, check(pa, r1, r2, h, i, u, N, 300, 5, d=40).labels)
    got = pa.clusters_from_counts(r1, r2, None, i, u, N, 300, 5, acc_ratio=(1, 3))
    assert np.array_equal(got.labels, check(pa, r1, r2, h, i, u, N, 300, 5, num=1, den=3).labels)


def one_pair(pa, h, i, u, cg, **kw):
    z = np.zeros(1, np.uint32)
    got = pa.clusters_from_counts(z, z + 1, z + h, z + i, z + u, 2, 1000, cg, **kw)
    assert got.edges == 2 - got.clusters and list(got.labels) == ([0, 0] if got.edges else [0, 1])
    return got


def test_the_core_boundary(pa):
    """d == core_max_d is an edge (either parity of h), d == core_max_d + 1 is not"""
    for D in (0, 1, 37, 2**31 - 2):
        assert one_pair(pa, 2 * D, 0, 0, 1, core_max_d=D).edges == 1
        assert one_pair(pa, 2 * D + 1, 0, 0, 1, core_max_d=D).edges == 1
        assert one_pair(pa, 2 * D + 2, 0, 0, 1, core_max_d=D).edges == 0
        if D:
            assert one_pair(pa, 2 * D, 0, 0, 1, core_max_d=D - 1).edges == 0
    # thresholds past every possible d, the largest value that still is a criterion included
    for D in (2**31 - 1, 2**32, 2**64 - 2):
        assert one_pair(pa, 2**32 - 1, 0, 0, 1, core_max_d=D).edges == 1


@pytest.mark.parametrize("a,b,cg,num,den", [(1, 3, 0, 1, 3), (2, 6, 0, 1, 3), (5, 20, 5, 2**18, 2**20), (0, 7, 0, 0, 1), (12, 12, 0, 1, 1),
                                            (3, 12, 2, 2**22, 2**24), (2**16, 2**17, 0, 2**23, 2**24), (2**16, 2**40, 2**40 - 2**17, 1, 2**24)])
def test_the_accessory_boundary(pa, a, b, cg, num, den):
    """a den == num b is an edge; one more differing gene over the same b, or the next smaller numerator, is not"""
    assert a * den == num * b
    u = b - cg
    i = u - a
    assert one_pair(pa, 0, i, u, cg, acc_ratio=(num, den)).edges == 1
    if i > 0:
        assert one_pair(pa, 0, i - 1, u, cg, acc_ratio=(num, den)).edges == 0
    if num > 0:
        assert one_pair(pa, 0, i, u, cg, acc_ratio=(num - 1, den)).edges == 0


def test_core_genes_of_any_size(pa):
    """acc_num b passes 64 bits (2^24 2^41: a product cut to 64 bits would be 0): the comparison is made in 128"""
    for a in (0, 5, 8):
        assert one_pair(pa, 0, 8 - a, 8, 2**41 - 8, acc_ratio=(2**24, 2**24)).edges == 1
    # a den == num b == 2^41, and one core gene fewer
    assert one_pair(pa, 0, 0, 2**17, 2**41 - 2**17, acc_ratio=(1, 2**24)).edges == 1
    assert one_pair(pa, 0, 0, 2**17, 2**41 - 2**17 - 1, acc_ratio=(1, 2**24)).edges == 0


def test_undefined_pairs(pa):
    """b == 0 is never an edge while the accessory criterion is active -- not even at acc_num == acc_den -- and is counted;
    without the criterion it is neither"""
    for ratio in ((1, 1), (0, 1), (2**24, 2**24)):
        got = one_pair(pa, 0, 0, 0, 0, acc_ratio=ratio)
        assert got.edges == 0 and got.undefined_pairs == 1
        got = one_pair(pa, 0, 0, 0, 0, acc_ratio=ratio, core_max_d=5)
        assert got.edges == 0 and got.undefined_pairs == 1
    got = one_pair(pa, 0, 0, 0, 0, core_max_d=5)
    assert got.edges == 1 and got.undefined_pairs == 0
    assert one_pair(pa, 0, 0, 0, 1, acc_ratio=(0, 1)).edges == 1           # one core gene: distance 0 / 1


def test_an_incomplete_pair_list(pa):
    """a path given as N - 1 pairs in a shuffled order is one cluster; without its middle pair, two"""
    rng = np.random.default_rng(7)
    N = 50
    order = rng.permutation(N).astype(np.uint32)
    r1, r2 = order[:-1], order[1:]
    z = np.zeros(N - 1, np.uint32)
    got = check(pa, r1, r2, z, z, z, N, 10, 1, d=0)
    assert got.clusters == 1 and got.edges == N - 1 and got.within_pairs == N * (N - 1) // 2 and not got.labels.any()
    h = z.copy()
    h[24] = 2
    got = check(pa, r1, r2, h, z, z, N, 10, 1, d=0)
    assert got.clusters == 2 and got.largest_cluster == 25 and got.singletons == 0
    # no pair at all: every individual on its own
    e = np.zeros(0, np.uint32)
    got = pa.clusters_from_counts(e, e, e, e, e, 5, 10, 1, core_max_d=0)
    assert got.clusters == got.singletons == 5 and list(got.labels) == [0, 1, 2, 3, 4] and list(got.sizes()) == [1] * 5


def test_wrapper_thresholds_and_result(pa):
    rng = np.random.default_rng(8)
    r1, r2, h, i, u = random_pairs(rng, 40, 300, 300, 70)
    got = pa.clusters_from_counts(r1, r2, h, i, u, 40, 300, 5, core_max=0.2501, acc_max=0.4)
    want = ref.clusters(r1, r2, h, i, u, 40, 300, 5, *ref.thresholds(300, 0.2501, 0.4))
    assert ref.thresholds(300, 0.2501, 0.4) == (75, 419430, 2**20)
    ref.assert_equal(got, want, 40)
    d = got.as_dict()
    assert d["labels"] is got.labels and d["clusters"] == got.clusters and "rounds" in d
    assert list(got.sizes()) == sorted(np.bincount(got.labels)[np.bincount(got.labels) > 0], reverse=True)
    with pytest.raises(ValueError):
        pa.clusters_from_counts(r1, r2[:-1], h, i, u, 40, 300, 5, core_max=0.1)
    with pytest.raises(ValueError):
        pa.clusters_from_counts(r1, r2, h, i, u, 40, 300, 5, core_max=-0.1)
    with pytest.raises(ValueError):
        pa.clusters_from_counts(r1, r2, h, i, u, 40, 300, 5, acc_max=1.5)


def test_error_paths(pa):
    lib = pa.load()
    P, T = pa._lib.ClusterParams, pa._lib.Clusters
    arr = lambda *v: np.array(v, np.uint32)
    base = dict(r1=arr(0, 1), r2=arr(1, 2), h=arr(4, 6), i=arr(1, 2), u=arr(3, 2), lab=np.zeros(3, np.uint32))
    out = T()

    def call(prm, n=2, N=3, o=out, **kw):
        a = dict(base, **kw)
        ptr = lambda x: None if x is None else x.ctypes.data
        return lib.ps_clusters_from_counts(ptr(a["r1"]), ptr(a["r2"]), ptr(a["h"]), ptr(a["i"]), ptr(a["u"]), n, N, 10, 1,
                                           C.byref(prm) if prm is not None else None, C.byref(o) if o is not None else None, ptr(a["lab"]))

    def fails(text, *args, **kw):
        assert call(*args, **kw) == PS_ERR_INVALID
        assert text in lib.ps_last_error().decode(), lib.ps_last_error().decode()

    ok = P(3, 1, 2)
    assert call(ok) == 0
    fails("at least one criterion", P(ref.NO_CORE, 0, 0))
    fails("at least one criterion", P(ref.NO_CORE, 5, 0))
    fails("acc_num <= acc_den <= 2^24", P(3, 3, 2))
    fails("acc_num <= acc_den <= 2^24", P(ref.NO_CORE, 1, 2**24 + 1))
    assert call(P(ref.NO_CORE, 2**24, 2**24)) == 0
    fails("pair 1: intersection 3 above union 2", ok, i=arr(1, 3))
    assert call(P(3, 0, 0), i=arr(1, 3)) == 0                   # (the accessory numerators are not looked at)
    fails("pair 1: index 3 is not below pop_size 3", ok, r2=arr(1, 3))
    fails("pair 0: index 7 is not below pop_size 3", ok, r1=arr(7, 1))
    fails("pair 1: both indices are 1", ok, r2=arr(1, 1))
    fails("pop_size", ok, N=1)
    for kw in (dict(r1=None), dict(r2=None), dict(h=None), dict(i=None), dict(u=None), dict(lab=None), dict(o=None)):
        fails("null", ok, **kw)
    fails("null", None)
    with pytest.raises(pa.PansimError) as e:
        pa.clusters_from_counts(base["r1"], base["r2"], base["h"], base["i"], base["u"], 3, 10, 1)
    assert e.value.code == PS_ERR_INVALID and "at least one criterion" in str(e.value)
    with pytest.raises(pa.PansimError) as e:
        pa.clusters_from_counts(base["r1"], base["r2"], base["h"], base["i"], base["u"], 3, 10, 1, acc_ratio=(3, 2))
    assert e.value.code == PS_ERR_INVALID and "acc_num <= acc_den" in str(e.value)


def test_every_new_symbol_is_exported_and_declared(pa):
    lib = C.CDLL(pa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pansim_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in pa._lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
    assert lib.ps_abi_version() == 3


def test_the_device_entries_need_a_device(pa):
    """without a device the three device entries fail with PS_ERR_NO_DEVICE before they look at their arguments; with one,
    the same calls refuse their null arguments"""
    lib = pa.load()
    out, prm = pa._lib.Clusters(), pa._lib.ClusterParams(3, 1, 2)
    labels = np.zeros(16, np.uint32)
    want = PS_ERR_NO_DEVICE if lib.ps_device_count() <= 0 else PS_ERR_INVALID
    assert lib.ps_strain_clusters(None, None, C.byref(prm), C.byref(out), labels.ctypes.data) == want
    assert lib.ps_sim_strain_clusters(None, C.byref(prm), C.byref(out), labels.ctypes.data) == want
    assert lib.ps_multi_strain_clusters(None, C.byref(prm), C.byref(out), labels.ctypes.data) == want
    if want == PS_ERR_NO_DEVICE:
        assert "no HIP device" in lib.ps_last_error().decode()
        bad = pa._lib.ClusterParams(ref.NO_CORE, 0, 0)           # ... and before the parameters
        assert lib.ps_strain_clusters(None, None, C.byref(bad), C.byref(out), labels.ctypes.data) == PS_ERR_NO_DEVICE
    assert lib.ps_strain_clusters_timing(None, None, None, None) == PS_ERR_INVALID


def cli(*args):
    return subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=60)


def test_cli_needs_a_threshold(pa):
    r = cli("--print_clusters", "--pan_genes", 3000)
    assert r.returncode == 101 and r.stdout == "" and "--cluster_core_max" in r.stderr and "--cluster_acc_max" in r.stderr, r.stderr


@pytest.mark.parametrize("flag,value,text", [
    ("cluster_core_max", "-0.5", "must be >= 0.0"), ("cluster_core_max", "nan", "must be >= 0.0"), ("cluster_core_max", "inf", "must be >= 0.0"),
    ("cluster_core_max", "x", "invalid float literal"), ("cluster_acc_max", "-0.1", "0.0 <= X <= 1.0"), ("cluster_acc_max", "1.5", "0.0 <= X <= 1.0"),
    ("cluster_acc_max", "nan", "0.0 <= X <= 1.0"), ("cluster_acc_max", "1,0", "invalid float literal")])
def test_cli_rejects_bad_thresholds(pa, flag, value, text):
    """checked before any device work, whether or not --print_clusters is given"""
    for extra in ((), ("--print_clusters",)):
        r = cli("--%s=%s" % (flag, value), "--pan_genes", 3000, *extra)
        assert r.returncode == 101 and r.stdout == "" and "--" + flag in r.stderr and text in r.stderr, (r.returncode, r.stderr)


def test_cli_flag_shapes(pa):
    r = cli("--print_clusters=1")
    assert r.returncode == 2 and "takes no value" in r.stderr
    r = cli("--cluster_acc_max")
    assert r.returncode == 2 and "requires a value" in r.stderr


def test_help_extensions_lists_the_cluster_flags(pa):
    r = cli("--help-extensions")
    assert r.returncode == 0
    assert "--print_clusters\n" in r.stdout and "_clusters.tsv" in r.stdout and "_clusters_summary.tsv" in r.stdout
    assert "--cluster_core_max <cluster_core_max>\n" in r.stdout and "--cluster_acc_max <cluster_acc_max>\n" in r.stdout
    r = cli("--help")
    assert r.returncode == 0 and "cluster" not in r.stdout
    assert r.stdout[r.stdout.index("USAGE:"):] == open(os.path.join(ROOT, "tests", "golden", "help_usage.txt")).read()
