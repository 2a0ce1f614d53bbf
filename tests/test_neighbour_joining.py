"""The neighbour-joining tree without a device (docs/NEIGHBOUR_JOINING.md): the symbols are declared, exported, bound and
documented, `neighbour_joining` is written once beside _Readouts and asks for the entry of its class, nothing falls back without a
device, the host form ps_nj_from_counts equals the NumPy restatement of the rule (tests/neighbour_joining_ref.py) bit for bit
and recovers planted additive trees exactly, its errors, the Newick text by hand, and the rule's header in a host program of its
own under the address and undefined-behaviour sanitizers.  The device half is tests/test_gpu_neighbour_joining.py.  Every
comparison is an equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import neighbour_joining_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS_ERR_INVALID, PS_ERR_NO_DEVICE = -1, -2
NEW_SYMBOLS = ("ps_neighbour_joining", "ps_sim_neighbour_joining", "ps_multi_neighbour_joining", "ps_nj_from_counts", "ps_nj_newick",
               "ps_neighbour_joining_timing")
METRICS = (("core", ref.CORE), ("acc", ref.ACC))
# the five-taxon example of the Wikipedia article on neighbour joining: taxa a .. e are rows 0 .. 4
FIVE = {(0, 1): 5, (0, 2): 9, (0, 3): 9, (0, 4): 8, (1, 2): 10, (1, 3): 10, (1, 4): 9, (2, 3): 8, (2, 4): 7, (3, 4): 3}


def test_abi_header_and_bindings_agree(pa):
    lib = pa.load()
    hdr = open(os.path.join(ROOT, "include", "pansim_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in pa._lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
        assert "fn %s(" % name in integration, name
        comment = hdr[:hdr.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert "reference has no such function" in comment and "population.rs:787-837" in comment, name
    assert lib.ps_abi_version() == 3
    fields = re.search(r"typedef struct \{([^}]*)\} ps_nj_t;", hdr).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    declared = [f.strip() for line in re.findall(r"uint64_t ([^;]*);", fields) for f in line.split(",")]
    assert declared == [name for name, _ in pa._lib.Nj._fields_] == list(ref.INT_FIELDS)
    assert all(t is C.c_uint64 for _, t in pa._lib.Nj._fields_) and pa.NeighbourJoiningTree.FIELDS == ref.INT_FIELDS
    assert os.path.exists(os.path.join(ROOT, "docs", "NEIGHBOUR_JOINING.md"))
    assert "NEIGHBOUR_JOINING.md" in open(os.path.join(ROOT, "docs", "UPGMA_TREE.md")).read()
    assert "ps_neighbour_joining" in open(os.path.join(ROOT, "README.md")).read()
    assert pa.nj_from_counts is pa.joining.nj_from_counts and pa.nj_newick is pa.joining.nj_newick
    assert pa.NeighbourJoiningTree is pa.joining.NeighbourJoiningTree
    for method in ("neighbour_joining", "neighbour_joining_timing"):
        assert callable(getattr(pa.Population, method))


def test_both_run_classes_ask_for_their_own_entry(pa):
    """written once in _Joining, not in _Readouts, the other mixins or the two classes; no device: the library is an object that
    notes the first symbol asked for"""
    from pansim_amd import _lib, simulation

    class Asked(Exception):
        pass

    class Library:
        def __getattr__(self, name):
            raise Asked(name)

    assert "neighbour_joining" in vars(simulation._Joining)
    for other in (simulation._Readouts, simulation._Associations, simulation._Profiles, simulation._Samples):
        assert "neighbour_joining" not in vars(other)
    for cls, symbol in ((pa.Simulation, "ps_sim_neighbour_joining"), (pa.MultiSimulation, "ps_multi_neighbour_joining")):
        assert hasattr(cls, "neighbour_joining") and "neighbour_joining" not in vars(cls)
        run = object.__new__(cls)
        run._lib, run._h, run.generation = Library(), None, 0
        run.params = _lib.SimParams(pop_size=8, core_size=100, pan_genes=60, core_genes=20, max_distances=10)
        for metric in ("core", "acc"):
            with pytest.raises(Asked) as e:
                run.neighbour_joining(metric)
            assert str(e.value) == symbol and symbol in _lib.SIGNATURES


def test_the_device_entries_need_a_device(pa):
    """a non-null handle, no device: the entries fail with PS_ERR_NO_DEVICE before they look at the handle (with a device the
    handle would have to be real: tests/test_gpu_neighbour_joining.py); null arguments behind it"""
    lib = pa.load()
    if lib.ps_device_count() > 0:
        pytest.skip("a GPU is present")
    block = np.zeros(4096, np.uint8)                     # (never read: the device check comes first)
    handle = C.c_void_p(block.ctypes.data)
    prm, out = pa._lib.TreeParams(0), pa._lib.Nj()
    a, b, x, y = np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4), np.zeros(4)
    tail = (C.byref(prm), C.byref(out), a.ctypes.data, b.ctypes.data, x.ctypes.data, y.ctypes.data)
    assert lib.ps_neighbour_joining(handle, handle, *tail) == PS_ERR_NO_DEVICE and "no HIP device" in lib.ps_last_error().decode()
    assert lib.ps_neighbour_joining(None, None, *tail) == PS_ERR_NO_DEVICE
    for fn in (lib.ps_sim_neighbour_joining, lib.ps_multi_neighbour_joining):
        assert fn(handle, *tail) == PS_ERR_NO_DEVICE
        assert fn(None, *tail) == PS_ERR_NO_DEVICE
    assert lib.ps_neighbour_joining_timing(None, None, None, None) == PS_ERR_INVALID


# -- ps_nj_from_counts against the restatement -----------------------------------------------------------------------------------

def _random_list(rng, N):
    """a complete list with arbitrary numerators: h odd and even, I <= U <= 65535"""
    r1, r2 = ref.all_pairs(N)
    h = rng.integers(0, 5000, r1.size).astype(np.uint32)
    u = rng.integers(0, 65536, r1.size).astype(np.uint32)
    i = (u * rng.random(r1.size)).astype(np.uint32)
    return r1, r2, h, i, u


@pytest.mark.parametrize("N", [2, 3, 7, 40])
def test_from_counts_equals_the_restatement(pa, N):
    rng = np.random.default_rng(N)
    nums = _random_list(rng, N)
    for name, metric in METRICS:
        want = ref.tree(metric, *nums, N, 777, 3)
        got = pa.nj_from_counts(*nums, N, 777, 3, metric=name)
        ref.assert_equal(got, want)
        assert got.joins == N - 1 and got.left.size == N - 1
        # the other metric's numerators may be left out
        part = nums[:2] + ((nums[2], None, None) if metric == ref.CORE else (None, nums[3], nums[4]))
        ref.assert_equal(pa.nj_from_counts(*part, N, 777, 3, metric=name), want)
        # any order and orientation of the list
        order = rng.permutation(nums[0].size)
        flip = rng.random(order.size) < 0.5
        a, b = nums[0][order], nums[1][order]
        shuffled = (np.where(flip, b, a), np.where(flip, a, b)) + tuple(x[order] for x in nums[2:])
        ref.assert_equal(pa.nj_from_counts(*shuffled, N, 777, 3, metric=name), want)
        d = got.as_dict()
        assert set(d) == set(ref.INT_FIELDS) | {"left", "right", "len_left", "len_right", "tree_length"}
        total = np.float64(0.0)
        for x, y in zip(got.len_left, got.len_right):
            total = (total + x) + y
        assert got.tree_length == float(total) and got.merges()[0] is got.left and got.merges()[1] is got.right
        if N > 3 and metric == ref.CORE:
            assert got.negative_branches == int((got.len_left < 0).sum() + (got.len_right < 0).sum())


@pytest.mark.parametrize("N", [2, 9, 40])
def test_all_ties_give_the_caterpillar(pa, N):
    """every pair at the same distance, 6 sites or 8 / 16 (dyadic, so every operation of the rule is exact): every q of a step is
    equal and the ids alone decide -- (0, 1), then (0, 2), ..."""
    r1, r2 = ref.all_pairs(N)
    h = np.full(r1.size, 12, np.uint32)
    i, u = np.full(r1.size, 4, np.uint32), np.full(r1.size, 12, np.uint32)
    for name, metric in METRICS:
        got = pa.nj_from_counts(r1, r2, h, i, u, N, 100, 4, metric=name)
        ref.assert_equal(got, ref.tree(metric, r1, r2, h, i, u, N, 100, 4))
        assert list(got.left) == [0] + list(range(N, 2 * N - 2)) and list(got.right) == list(range(1, N))
    star = pa.nj_from_counts(r1, r2, h, None, None, N, 100, 4)           # d = 6 everywhere: a star with branches of 3
    if N > 2:
        assert list(star.len_right[:-1]) == [3.0] * (N - 2) and star.len_left[0] == 3.0 and not star.len_left[1:-1].any()
    assert star.len_left[-1] == (6.0 if N == 2 else 3.0) and star.len_right[-1] == 0.0 and star.negative_branches == 0


def _five(pa):
    r1, r2 = ref.all_pairs(5)
    h = np.array([2 * FIVE[(int(a), int(b))] for a, b in zip(r1, r2)], np.uint32)
    return pa.nj_from_counts(r1, r2, h, None, None, 5, 100, 0), (r1, r2, h)


def test_the_five_taxon_example(pa):
    """branches a 2, b 3, c 4, d 2, e 1, inner edges 3 and 2; the ties fall to (u, c) and then (v, d) under the id order"""
    got, (r1, r2, h) = _five(pa)
    assert list(got.left) == [0, 5, 6, 7] and list(got.right) == [1, 2, 3, 4]
    assert list(got.len_left) == [2.0, 3.0, 2.0, 1.0] and list(got.len_right) == [3.0, 4.0, 2.0, 0.0]
    assert got.tree_length == 17.0 and got.negative_branches == 0 and got.metric == 0 and got.pairs == 10
    assert list(got.patristic(r1, r2)) == [float(x >> 1) for x in h]
    z = np.zeros(10, np.uint32)
    ref.assert_equal(got, ref.tree(ref.CORE, r1, r2, h, z, z, 5, 100, 0))
    assert got.newick() == "(((0:0.02,1:0.03):0.03,2:0.04):0.02,3:0.02,4:0.01);"
    assert pa.nj_newick(got.left, got.right, got.len_left, got.len_right, 5) == "(((0:2,1:3):3,2:4):2,3:2,4:1);"


@pytest.mark.parametrize("N", [4, 9, 33, 70])
def test_additive_trees_are_recovered_exactly(pa, N):
    """a random tree with integer branches: its path metric comes back split for split and length for length"""
    rng = np.random.default_rng(100 + N)
    planted = ref.random_tree(rng, N)
    D = ref.path_lengths(planted, N)
    r1, r2 = ref.all_pairs(N)
    h = (2 * D[r1, r2]).astype(np.uint32) + rng.integers(0, 2, r1.size).astype(np.uint32)      # (an odd h is halved downwards)
    got = pa.nj_from_counts(r1, r2, h, None, None, N, 10**6, 0)
    assert ref.splits(got.left, got.right, got.len_left, got.len_right, N) == ref.splits(*planted, N)
    assert np.array_equal(got.patristic(r1, r2), D[r1, r2]) and np.array_equal(got.patristic(r2, r1), D[r1, r2])
    assert got.negative_branches == 0 and got.tree_length == float(planted[2].sum() + planted[3].sum())
    # the builders agree with each other: the infinite-sites population realises the metric
    sites = ref.infinite_sites(planted, N)
    assert np.array_equal((sites[r1] != sites[r2]).sum(axis=1), D[r1, r2])
    with pytest.raises(ValueError):
        got.patristic([0], [0])
    with pytest.raises(ValueError):
        got.patristic([0], [N])


def _call(pa, *args):
    rc = pa.load().ps_nj_from_counts(*args)
    return rc, pa.load().ps_last_error().decode()


def test_from_counts_refuses_bad_lists(pa):
    N = 6
    r1, r2, h, i, u = _random_list(np.random.default_rng(1), N)
    P = r1.size
    o, prm = pa._lib.Nj(), pa._lib.TreeParams(ref.ACC)
    left, right, ll, lr = np.zeros(N, np.uint32), np.zeros(N, np.uint32), np.zeros(N), np.zeros(N)
    p = lambda a: None if a is None else a.ctypes.data                                                 # noqa: E731
    tail = lambda: (C.byref(prm), C.byref(o), p(left), p(right), p(ll), p(lr))                        # noqa: E731
    rc, msg = _call(pa, p(r1), p(r2), p(h), p(i), p(u), P - 1, N, 100, 3, *tail())
    assert rc == PS_ERR_INVALID and "complete list of all 15 pairs" in msg and "not 14" in msg
    dup = r2.copy()
    dup[1], bad = dup[0], r1.copy()
    rc, msg = _call(pa, p(r1), p(dup), p(h), p(i), p(u), P, N, 100, 3, *tail())
    assert rc == PS_ERR_INVALID and "listed twice" in msg
    flipped1, flipped2 = r1.copy(), r2.copy()
    flipped1[1], flipped2[1] = r2[0], r1[0]                         # the first pair again, the other way round
    rc, msg = _call(pa, p(flipped1), p(flipped2), p(h), p(i), p(u), P, N, 100, 3, *tail())
    assert rc == PS_ERR_INVALID and "listed twice" in msg
    bad[3] = N
    rc, msg = _call(pa, p(bad), p(r2), p(h), p(i), p(u), P, N, 100, 3, *tail())
    assert rc == PS_ERR_INVALID and "pair 3: index 6" in msg
    same = r1.copy()
    same[2] = r2[2]
    rc, msg = _call(pa, p(same), p(r2), p(h), p(i), p(u), P, N, 100, 3, *tail())
    assert rc == PS_ERR_INVALID and "both indices" in msg
    above = i.copy()
    above[4] = u[4] + 1
    rc, msg = _call(pa, p(r1), p(r2), p(h), p(above), p(u), P, N, 100, 3, *tail())
    assert rc == PS_ERR_INVALID and "pair 4: intersection" in msg
    wide = u.copy()
    wide[5] = 65536
    rc, msg = _call(pa, p(r1), p(r2), p(h), p(i), p(wide), P, N, 100, 3, *tail())
    assert rc == PS_ERR_INVALID and "65535 accessory genes" in msg
    # the metric and its limits
    rc, msg = _call(pa, p(r1), p(r2), p(h), p(i), p(u), P, N, 100, 0, *tail())
    assert rc == PS_ERR_INVALID and "core_genes >= 1" in msg
    rc, msg = _call(pa, p(r1), p(r2), p(h), p(i), p(u), P, N, 100, 2**32 - 65535, *tail())
    assert rc == PS_ERR_INVALID and "core_genes + 65535 < 2^32" in msg
    rc, msg = _call(pa, p(r1), p(r2), p(h), p(i), p(u), P, N, 2**32, 3, *tail())
    assert rc == PS_ERR_INVALID and "fewer than 2^32 core sites" in msg
    for size in (1, 16385):
        rc, msg = _call(pa, p(r1), p(r2), p(h), p(i), p(u), P, size, 100, 3, *tail())
        assert rc == PS_ERR_INVALID and "pop_size <= 16384" in msg and "not %d" % size in msg
    prm.metric = 2
    rc, msg = _call(pa, p(r1), p(r2), p(h), p(i), p(u), P, N, 100, 3, *tail())
    assert rc == PS_ERR_INVALID and "PS_TREE_CORE (0) or PS_TREE_ACC (1), not 2" in msg
    # nulls: the metric's own numerators, the indices, any output
    prm.metric = ref.ACC
    rc, msg = _call(pa, p(r1), p(r2), p(h), None, p(u), P, N, 100, 3, *tail())
    assert rc == PS_ERR_INVALID and "needs its numerators" in msg
    prm.metric = ref.CORE
    rc, msg = _call(pa, p(r1), p(r2), None, p(i), p(u), P, N, 100, 3, *tail())
    assert rc == PS_ERR_INVALID and "needs its numerators" in msg
    assert _call(pa, p(r1), p(r2), p(h), None, None, P, N, 100, 0, *tail())[0] == 0      # (the core metric: no genes needed)
    rc, msg = _call(pa, None, p(r2), p(h), p(i), p(u), P, N, 100, 3, *tail())
    assert rc == PS_ERR_INVALID and "null" in msg
    for k in range(6):
        args = list(tail())
        args[k] = None
        rc, msg = _call(pa, p(r1), p(r2), p(h), p(i), p(u), P, N, 100, 3, *args)
        assert rc == PS_ERR_INVALID and "null" in msg
    with pytest.raises(ValueError):
        pa.nj_from_counts(r1, r2, h, i, u, N, 100, 3, metric="joint")
    with pytest.raises(ValueError):
        pa.nj_from_counts(r1, r2[:-1], h, i, u, N, 100, 3)


# -- ps_nj_newick ------------------------------------------------------------------------------------------------------------------

def _u32(*v):
    return np.array(v, np.uint32)


def test_newick_by_hand(pa):
    f = pa.fmt_f64
    # two leaves: the one edge whole above the left one
    assert pa.nj_newick(_u32(0), _u32(1), [7.0], [0.0], 2) == "(0:7,1:0);"
    assert pa.nj_newick(_u32(0), _u32(1), [7.0], [0.0], 2, scale=4) == "(0:1.75,1:0);"
    # three leaves: the inner child of the last join is opened, whichever side it is on; the leaf takes the whole last edge
    assert pa.nj_newick(_u32(0, 3), _u32(1, 2), [1.5, 0.25], [2.5, 0.0], 3) == "(0:1.5,1:2.5,2:0.25);"
    assert pa.nj_newick(_u32(1, 0), _u32(2, 3), [1.0, 3.0], [-2.0, 0.5], 3) == "(1:1,2:-2,0:3.5);"
    # five leaves, both children of the last join inner nodes: the right one is opened, the left one stands behind its children
    left, right = _u32(0, 2, 4, 5), _u32(1, 3, 6, 7)
    ll, lr = np.array([1.0, 3.0, 5.0, 0.125]), np.array([2.0, 4.0, 6.0, 0.0])
    assert pa.nj_newick(left, right, ll, lr, 5) == "(4:5,(2:3,3:4):6,(0:1,1:2):0.125);"
    third = pa.nj_newick(left, right, ll, lr, 5, scale=3)
    assert third == "(4:%s,(2:1,3:%s):2,(0:%s,1:%s):%s);" % (f(5 / 3), f(4 / 3), f(1 / 3), f(2 / 3), f(0.125 / 3))
    # the size protocol
    lib, need = pa.load(), C.c_uint64()
    p = lambda a: a.ctypes.data                                                                        # noqa: E731
    assert lib.ps_nj_newick(p(left), p(right), p(ll), p(lr), 5, 1.0, None, 0, C.byref(need)) == 0 and need.value == 35
    buf = C.create_string_buffer(35)
    assert lib.ps_nj_newick(p(left), p(right), p(ll), p(lr), 5, 1.0, buf, 34, C.byref(need)) == PS_ERR_INVALID
    assert "needs 35 bytes" in lib.ps_last_error().decode() and "holds 34" in lib.ps_last_error().decode()
    assert lib.ps_nj_newick(p(left), p(right), p(ll), p(lr), 5, 1.0, buf, 35, C.byref(need)) == 0 and len(buf.value) == 34
    # what is refused
    assert lib.ps_nj_newick(p(left), p(right), p(ll), p(lr), 5, 1.0, None, 0, None) == PS_ERR_INVALID
    assert lib.ps_nj_newick(None, p(right), p(ll), p(lr), 5, 1.0, None, 0, C.byref(need)) == PS_ERR_INVALID
    assert lib.ps_nj_newick(p(left), p(right), p(ll), p(lr), 1, 1.0, None, 0, C.byref(need)) == PS_ERR_INVALID
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.ps_nj_newick(p(left), p(right), p(ll), p(lr), 5, scale, None, 0, C.byref(need)) == PS_ERR_INVALID
        assert "scale" in lib.ps_last_error().decode()
    for bad_left, bad_right in ((_u32(0, 2, 4, 5), _u32(1, 3, 6, 8)), (_u32(0, 0, 4, 5), _u32(1, 3, 6, 7)), (_u32(0, 6, 4, 5), _u32(1, 3, 6, 7))):
        assert lib.ps_nj_newick(p(bad_left), p(bad_right), p(ll), p(lr), 5, 1.0, None, 0, C.byref(need)) == PS_ERR_INVALID
        assert "not an earlier node that is still free" in lib.ps_last_error().decode()
    with pytest.raises(ValueError):
        pa.nj_newick(left, right, ll, lr, 6)


def test_newick_of_a_deep_caterpillar(pa):
    """3000 leaves in one chain: the walk keeps its own stack"""
    N = 3000
    left, right = _u32(0, *range(N, 2 * N - 2)), _u32(*range(1, N))
    text = pa.nj_newick(left, right, np.ones(N - 1), np.full(N - 1, 2.0), N)
    # N - 1 joins, the last one dissolved: N - 2 pairs of parentheses, one of them the outermost; N leaves and N - 3 closed groups
    assert text.count("(") == text.count(")") == N - 2 and text.count(",") == N - 1 and text.endswith(",2999:3);")
    assert text.startswith("(" * (N - 2) + "0:1,1:2):1,2:2):1,")
    assert sorted(int(x) for x in re.findall(r"[(,](\d+):", text)) == list(range(N))


def test_the_rule_header_alone(tmp_path):
    """tests/nj_rule_check.cpp: nj_rule.h is plain C++ under g++; the five-taxon example and planted additive trees through its
    functions, built with the sanitizers, nothing loaded into Python"""
    exe = str(tmp_path / "nj_rule_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "nj_rule_check.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "the rule holds" and len(lines) == 7 and not any("BAD" in line for line in lines)
