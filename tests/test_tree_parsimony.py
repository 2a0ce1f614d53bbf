"""Tree parsimony without a device (docs/TREE_PARSIMONY.md): the restatement (tests/tree_parsimony_ref.py) against brute force,
the host form ps_parsimony_from_rows, the level schedule and the two merge-list builders against it, the error paths of the
merge list, the no-device errors of the device entries and the CLI's flag checks and help text.  The device half is
tests/test_gpu_tree_parsimony.py.  Every comparison is an equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tree_parsimony_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_NO_DEVICE = -1, -2
NEW_SYMBOLS = ("ps_tree_parsimony", "ps_sim_tree_parsimony", "ps_multi_tree_parsimony", "ps_tree_parsimony_timing", "ps_merges_from_tree",
               "ps_merges_from_genealogy", "ps_parsimony_schedule", "ps_parsimony_from_rows")
SHAPES = [(2, 5), (7, 203), (64, 16), (65, 17), (300, 130)]


def junk_matrix(rng, N, L):
    m = ref.onehot(rng, (N, L))
    bad = rng.random((N, L)) < 0.15
    m[bad] = rng.integers(0, 256, int(bad.sum()), dtype=np.uint8)
    return m


def test_the_restatement_is_the_true_minimum():
    """Fitch's score against the minimum over all 5^M internal assignments, and the down pass's branches add up to it, on
    random trees and forests of up to six leaves with arbitrary bytes"""
    rng = np.random.default_rng(1)
    for trial in range(40):
        N = int(rng.integers(2, 7))
        M = int(rng.integers(1, N))
        left, right = ref.random_joining(rng, N, M)
        st = ref.class_bits(junk_matrix(rng, N, 12))
        st[:, 0] = st[0, 0]                                              # one column without a change
        changes, moved, X = ref.fitch(st, left, right)
        assert np.array_equal(changes, ref.brute_force(st, left, right)), (N, M)
        assert np.array_equal(moved.sum(axis=0), changes) and changes[0] == 0
        par = ref.parents(left, right, N)
        assert not moved[par < 0].any()
        covered = np.flatnonzero(par[:N] >= 0)
        assert np.array_equal(X[covered], st[covered])                   # a leaf's pick is its own state


def check_host(pa, m, left, right):
    want = ref.parsimony(m, left, right)
    full = pa.parsimony_from_rows(m, left, right)
    ref.assert_equal(full, want)
    bare = pa.parsimony_from_rows(m, left, right, per_site=False, branches=False)
    ref.assert_equal(bare, want, skip=("site_changes", "branch_changes"))
    assert bare.site_changes is None and bare.branch_changes is None
    return full


@pytest.mark.parametrize("N,L", SHAPES)
def test_from_rows_equals_the_restatement(pa, N, L):
    rng = np.random.default_rng(N * 131 + L)
    seen = 0
    for name, (left, right) in ref.trees(rng, N).items():
        m = ref.evolved(rng, N, L, left, right)
        got = check_host(pa, m, left, right)
        assert got.spanning == (name != "forest") and got.trees >= 1
        if name == "forest":
            assert got.covered_leaves < N and got.min_changes == got.homoplasic_sites == 0 and got.ci == 0.0
        seen += got.homoplasic_sites
        assert np.array_equal(got.parent, ref.parents(left, right, N))
    assert N < 7 or seen > 0


def test_from_rows_genes(pa):
    rng = np.random.default_rng(5)
    N, G = 65, 131
    for name, (left, right) in ref.trees(rng, N).items():
        a = ref.evolved_genes(rng, N, G, left, right)
        want = ref.parsimony(np.ones((N, 1), np.uint8), left, right, a)
        got = pa.parsimony_from_rows(a, left, right, genes=True)
        for k in ("gene_changes", "gene_gains", "gene_losses", "branch_gains", "branch_losses"):
            assert np.array_equal(getattr(got, k), want[k]), (name, k)
        for k in ("genes", "gene_total_changes", "gene_total_gains", "gene_total_losses", "merges", "trees", "covered_leaves"):
            assert getattr(got, k) == want[k], (name, k)
        assert got.sites == 0 and got.site_hist is None and got.gene_total_gains > 0 and got.gene_total_losses > 0
        bare = pa.parsimony_from_rows(a, left, right, genes=True, branches=False)
        assert np.array_equal(bare.gene_changes, want["gene_changes"]) and bare.gene_gains is None
        assert bare.gene_total_changes == want["gene_total_changes"] and bare.gene_total_gains == bare.gene_total_losses == 0
    lib = pa.load()
    out, buf = pa._lib.Parsimony(), np.zeros(4 * N, np.uint64)
    left, right = ref.caterpillar(N)
    args = (a.ctypes.data, N, G, 1, left.ctypes.data, right.ctypes.data, N - 1, C.byref(out))
    assert lib.ps_parsimony_from_rows(*args, buf.ctypes.data, *[None] * 7) == PS_ERR_INVALID          # a core output of a gene matrix
    assert lib.ps_parsimony_from_rows(*args[:3], 0, *args[4:], None, None, None, buf.ctypes.data, *[None] * 4) == PS_ERR_INVALID
    assert lib.ps_parsimony_from_rows(*args[:3], 2, *args[4:], *[None] * 8) == PS_ERR_INVALID


@pytest.mark.parametrize("N", [2, 7, 64, 1000])
def test_schedule_levels(pa, N):
    rng = np.random.default_rng(N)
    for name, (left, right) in ref.trees(rng, N).items():
        level_of, levels = pa.parsimony_schedule(left, right, N)
        want, top = ref.levels(left, right, N)
        assert np.array_equal(level_of, want) and levels == top, name
        for k in range(len(left)):
            for c in (int(left[k]), int(right[k])):
                assert (level_of[c - N] if c >= N else 0) < level_of[k]
        if name == "caterpillar":
            assert levels == N - 1
        if name == "balanced":
            assert levels == int(np.ceil(np.log2(N))) and (level_of == 1).sum() == N // 2
        if name == "random" and N == 1000:
            assert 10 <= levels <= 40                                    # (the depth the device tests rely on: about 20)


def test_merges_from_tree(pa):
    left, right = pa.merges_from_tree([2, 0, 1], [3, 1, 3], 4)
    assert list(left) == [2, 0, 5] and list(right) == [3, 1, 4]
    left, right = pa.merges_from_tree([3, 1, 3], [2, 0, 1], 4)            # the orientation of an edge does not matter
    assert list(left) == [2, 0, 5] and list(right) == [3, 1, 4]
    rng = np.random.default_rng(3)
    for N, E in ((2, 1), (50, 49), (50, 20), (333, 332)):
        # a random forest: row k > 0 hangs under a random earlier row; the edges shuffled, a part of them kept
        lo = np.array([rng.integers(0, k) for k in range(1, N)], np.uint32)
        hi = np.arange(1, N, dtype=np.uint32)
        keep = rng.permutation(N - 1)[:E]
        flip = rng.random(E) < 0.5
        a, b = np.where(flip, hi[keep], lo[keep]), np.where(flip, lo[keep], hi[keep])
        got, want = pa.merges_from_tree(a, b, N), ref.merges_from_tree(a, b, N)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].size == E
        assert pa.parsimony_schedule(*got, N)[1] >= 1                    # ... and a valid merge list
    with pytest.raises(pa.PansimError) as e:
        pa.merges_from_tree([0, 1, 0], [1, 2, 2], 4)
    assert e.value.code == PS_ERR_INVALID and "inside one cluster" in str(e.value)
    with pytest.raises(pa.PansimError) as e:
        pa.merges_from_tree([0], [4], 4)
    assert e.value.code == PS_ERR_INVALID
    with pytest.raises(pa.PansimError) as e:
        pa.merges_from_tree([0, 1, 2, 0], [1, 2, 3, 3], 4)
    assert e.value.code == PS_ERR_INVALID and "more than" in str(e.value)


def test_merges_from_genealogy(pa):
    B = ref.BEYOND
    left, right, height = pa.merges_from_genealogy([2, 0, 3, 1], [3, 1, 3])
    assert list(left) == [0, 2, 5] and list(right) == [3, 4, 1] and list(height) == [1, 3, 3]         # equal times: left to right
    left, right, height = pa.merges_from_genealogy([2, 0, 3, 1], [1, B, 2])
    assert list(left) == [2, 3] and list(right) == [0, 1] and list(height) == [1, 2]                  # two trees
    left, right, height = pa.merges_from_genealogy([1, 0], [B])
    assert left.size == right.size == height.size == 0
    rng = np.random.default_rng(8)
    for N in (2, 3, 40, 500):
        order = rng.permutation(N).astype(np.uint32)
        coal = rng.integers(1, 6, N - 1).astype(np.uint32)               # many equal times
        coal[rng.random(N - 1) < 0.1] = B
        got, want = pa.merges_from_genealogy(order, coal), ref.merges_from_genealogy(order, coal)
        for g, w in zip(got, want):
            assert g.dtype == np.uint32 and np.array_equal(g, w)
        assert got[0].size == int((coal != B).sum()) and (np.diff(got[2].astype(np.int64)) >= 0).all()
        if got[0].size:
            level_of, _ = pa.parsimony_schedule(got[0], got[1], N)
            assert level_of.size == got[0].size
    with pytest.raises(pa.PansimError) as e:
        pa.merges_from_genealogy([0, 0, 1], [1, 1])
    assert e.value.code == PS_ERR_INVALID and "permutation" in str(e.value)


@pytest.mark.parametrize("left,right,N,text", [
    ([0, 5], [1, 2], 4, "not a node below"),             # child >= N + k (its own node)
    ([0, 9], [1, 2], 4, "not a node below"),
    ([0, 0], [1, 2], 4, "a child of merge"),             # a node used twice
    ([0, 4], [1, 4], 4, "with itself"),                  # left == right
    ([], [], 4, "merges"),                               # M = 0
    ([0, 2, 4, 6], [1, 3, 5, 0], 4, "merges"),           # M > N - 1
    ([0], [1], 1, "pop_size"), ([0], [1], 16385, "pop_size")])
def test_bad_merge_lists(pa, left, right, N, text):
    for call in (lambda: pa.parsimony_schedule(left, right, N),
                 lambda: pa.parsimony_from_rows(np.ones((N, 3), np.uint8), left, right)):
        with pytest.raises(pa.PansimError) as e:
            call()
        assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)


def test_every_new_symbol_is_exported_and_declared(pa):
    lib = C.CDLL(pa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pansim_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in pa._lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
    assert lib.ps_abi_version() == 3
    assert "#define PS_PARS_BINS 64" in hdr and pa.PS_PARS_BINS == 64 and "#define PS_PARS_MAX_POP 16384u" in hdr and pa.PS_PARS_MAX_POP == 16384
    assert C.sizeof(pa._lib.Parsimony) == 17 * 8


def test_the_device_entries_need_a_device(pa):
    """without a device the three device entries fail with PS_ERR_NO_DEVICE before they look at their arguments; with one,
    the same calls refuse their null arguments"""
    lib = pa.load()
    out = pa._lib.Parsimony()
    bad = np.zeros(4, np.uint32)                             # (not a merge list either)
    rest = [None] * 8
    want = PS_ERR_NO_DEVICE if lib.ps_device_count() <= 0 else PS_ERR_INVALID
    assert lib.ps_tree_parsimony(None, None, bad.ctypes.data, bad.ctypes.data, 4, C.byref(out), *rest) == want
    assert lib.ps_sim_tree_parsimony(None, bad.ctypes.data, bad.ctypes.data, 4, C.byref(out), *rest) == want
    assert lib.ps_multi_tree_parsimony(None, bad.ctypes.data, bad.ctypes.data, 4, C.byref(out), *rest) == want
    if want == PS_ERR_NO_DEVICE:
        assert "no HIP device" in lib.ps_last_error().decode()
    assert lib.ps_tree_parsimony_timing(None, None, None, None) == PS_ERR_INVALID


def cli(*args):
    return subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args,text", [
    (("--print_parsimony", "nj"), "must be upgma, tree or genealogy"),
    (("--print_parsimony", "genealogy"), "needs --print_genealogy"),
    (("--print_parsimony", "upgma", "--pop_size", 16385), "2 <= pop_size <= 16384"),
    (("--print_parsimony", "tree", "--pop_size", 1), "2 <= pop_size <= 16384"),
    (("--print_parsimony", "upgma", "--upgma_metric", "acc", "--core_genes", 0), "core_genes >= 1")])
def test_cli_checks_come_before_device_work(pa, args, text):
    r = cli(*args, "--pan_genes", 3000)
    assert r.returncode == 101 and r.stdout == "" and text in r.stderr, (r.returncode, r.stderr)
    assert "--print_parsimony" in r.stderr or "--upgma_metric" in r.stderr


def test_cli_flag_needs_a_value(pa):
    r = cli("--print_parsimony")
    assert r.returncode == 2 and "requires a value" in r.stderr


def test_help_extensions_lists_the_flag(pa):
    r = cli("--help-extensions")
    assert r.returncode == 0 and "--print_parsimony <print_parsimony>\n" in r.stdout
    text = " ".join(r.stdout.split())
    for suffix in ("_parsimony_sites.tsv", "_parsimony_genes.tsv", "_parsimony_branches.tsv", "_parsimony.nwk", "_parsimony_summary.tsv"):
        assert suffix in text, suffix
    r = cli("--help")
    assert r.returncode == 0 and "print_parsimony" not in r.stdout
    assert r.stdout[r.stdout.index("USAGE:"):] == open(os.path.join(ROOT, "tests", "golden", "help_usage.txt")).read()
