"""Bootstrap support without a device (docs/BOOTSTRAP_SUPPORT.md): the symbols are declared, exported, bound and documented,
`bootstrap_support` is written once in _Bootstrap and asks for the entry of its class, nothing falls back without a device, the
draw rule ps_bootstrap_sites equals its NumPy restatement on site_weights_ref.philox, the counting ps_bootstrap_from_merges
equals the set restatement (tests/bootstrap_ref.py), and the counting's host code runs in a program of its own under the address
and undefined-behaviour sanitizers.  The device half is tests/test_gpu_bootstrap_support.py.  Every comparison is an equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bootstrap_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS_ERR_INVALID, PS_ERR_NO_DEVICE = -1, -2
NEW_SYMBOLS = ("ps_bootstrap_support", "ps_sim_bootstrap_support", "ps_multi_bootstrap_support", "ps_bootstrap_sites",
               "ps_bootstrap_from_merges", "ps_bootstrap_timing")


def test_abi_header_and_bindings_agree(pa):
    lib = pa.load()
    hdr = open(os.path.join(ROOT, "include", "pansim_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in pa._lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
        comment = hdr[:hdr.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert "reference has no such function" in comment and "population.rs:787-837" in comment, name
    assert lib.ps_abi_version() == 3
    fields = re.search(r"typedef struct \{([^}]*)\} ps_bootstrap_t;", hdr).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    declared = [f.strip() for line in re.findall(r"uint64_t ([^;]*);", fields) for f in line.split(",")]
    assert declared == [name for name, _ in pa._lib.Bootstrap._fields_] == list(ref.INT_FIELDS)
    assert all(t is C.c_uint64 for _, t in pa._lib.Bootstrap._fields_) and pa.BootstrapSupport.FIELDS == ref.INT_FIELDS
    assert [(n, t) for n, t in pa._lib.BootstrapParams._fields_] == [("method", C.c_int32), ("replicates", C.c_uint32), ("draws", C.c_uint64),
                                                                     ("seed", C.c_uint64)]
    assert (pa._lib.PS_BOOT_LINKAGE, pa._lib.PS_BOOT_UPGMA, pa._lib.PS_BOOT_NJ) == (0, 1, 2)
    for k, name in enumerate(("PS_BOOT_LINKAGE", "PS_BOOT_UPGMA", "PS_BOOT_NJ")):
        assert re.search(r"#define %s %d\b" % (name, k), hdr)
    assert re.search(r"PS_STREAM_BOOTSTRAP = 22\b", open(os.path.join(ROOT, "pansim_amd", "csrc", "ps_common.h")).read())
    assert os.path.exists(os.path.join(ROOT, "docs", "BOOTSTRAP_SUPPORT.md"))
    assert "ps_bootstrap_support" in open(os.path.join(ROOT, "README.md")).read()
    assert pa.bootstrap_sites is pa.bootstrap.bootstrap_sites and pa.bootstrap_from_merges is pa.bootstrap.bootstrap_from_merges
    assert pa.BootstrapSupport is pa.bootstrap.BootstrapSupport
    for method in ("bootstrap_support", "bootstrap_support_timing"):
        assert callable(getattr(pa.Population, method))


def test_both_run_classes_ask_for_their_own_entry(pa):
    """written once in _Bootstrap, not in _Readouts, the other mixins or the two classes; no device: the library is an object
    that notes the first symbol asked for"""
    from pansim_amd import _lib, simulation

    class Asked(Exception):
        pass

    class Library:
        def __getattr__(self, name):
            raise Asked(name)

    for method in ("bootstrap_support", "bootstrap_support_timing"):
        assert method in vars(simulation._Bootstrap)
        for other in (simulation._Readouts, simulation._Associations, simulation._Profiles, simulation._Samples, simulation._Joining):
            assert method not in vars(other)
    for cls, symbol in ((pa.Simulation, "ps_sim_bootstrap_support"), (pa.MultiSimulation, "ps_multi_bootstrap_support")):
        assert hasattr(cls, "bootstrap_support") and "bootstrap_support" not in vars(cls) and "bootstrap_support_timing" not in vars(cls)
        run = object.__new__(cls)
        run._lib, run._h, run.generation = Library(), None, 0
        run.params = _lib.SimParams(pop_size=8, core_size=100, pan_genes=60, core_genes=20, max_distances=10)
        for method in ref.METHODS:
            with pytest.raises(Asked) as e:
                run.bootstrap_support(method=method, replicates=3)
            assert str(e.value) == symbol and symbol in _lib.SIGNATURES
        with pytest.raises(ValueError):
            run.bootstrap_support(method="parsimony")


def test_the_device_entries_need_a_device(pa):
    """a non-null handle, no device: the entries fail with PS_ERR_NO_DEVICE before they look at the handle (with a device the
    handle would have to be real: tests/test_gpu_bootstrap_support.py)"""
    lib = pa.load()
    if lib.ps_device_count() > 0:
        pytest.skip("a GPU is present")
    prm, out = pa._lib.BootstrapParams(2, 3, 0, 0), pa._lib.Bootstrap()
    buf = np.zeros(8, np.uint32)
    p, fake = buf.ctypes.data_as(C.c_void_p), C.c_void_p(buf.ctypes.data)
    tail = (C.byref(prm), None, C.byref(out), p, p, p, p)
    assert lib.ps_bootstrap_support(fake, fake, *tail) == PS_ERR_NO_DEVICE
    assert lib.ps_sim_bootstrap_support(fake, *tail) == PS_ERR_NO_DEVICE
    assert lib.ps_multi_bootstrap_support(fake, *tail) == PS_ERR_NO_DEVICE
    assert "no HIP device" in lib.ps_last_error().decode()


@pytest.mark.parametrize("L", [1, 2, 130, 1_200_000, 2**32 - 1])
def test_the_draw_rule(pa, L):
    """odd and even numbers of draws, whole replicates and windows that start on an odd draw, two seeds, two replicates"""
    for seed in (0, 0x9E3779B97F4A7C15):
        for rep in (0, 41):
            for draws in (1, 2, 37, 200):
                got = pa.bootstrap_sites(seed, rep, L, draws)
                want = ref.draw_sites(seed, rep, L, draws)
                assert got.dtype == np.uint32 and np.array_equal(got, want)
                assert (got.astype(np.uint64) < L).all()
            for first, count in ((1, 36), (3, 5), (7, 0), (199, 1), (101, 99)):
                assert np.array_equal(pa.bootstrap_sites(seed, rep, L, 200, first, count), ref.draw_sites(seed, rep, L, 200, first, count))
    if L >= 130:       # (the draws are no constant and differ between replicates and seeds)
        a, b, c = pa.bootstrap_sites(1, 0, L, 64), pa.bootstrap_sites(1, 1, L, 64), pa.bootstrap_sites(2, 0, L, 64)
        assert len(set(a.tolist())) > 32 and not np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(pa.bootstrap_sites(5, 2, L), ref.draw_sites(5, 2, L, L)) if L <= 130 else True


def test_the_draw_rule_refuses(pa):
    for args in ((0, 0, 0, 10), (0, 0, 2**32, 10), (0, 0, 100, 0), (0, 0, 100, 2**31), (0, 0, 100, 10, 11, 0), (0, 0, 100, 10, 5, 6)):
        with pytest.raises(pa.PansimError) as e:
            pa.bootstrap_sites(*args)
        assert e.value.code == PS_ERR_INVALID


def _both(pa, ref_tree, reps, n):
    """the library's counting == the set restatement, rooted and unrooted -> the two (support, shared)"""
    out = []
    rl, rr = np.array([r[0] for r in reps], np.uint32).reshape(len(reps), n - 1), np.array([r[1] for r in reps], np.uint32).reshape(len(reps), n - 1)
    for unrooted in (False, True):
        got = pa.bootstrap_from_merges(ref_tree[0], ref_tree[1], rl, rr, n, unrooted=unrooted)
        want = ref.support_from_merges(ref_tree[0], ref_tree[1], rl, rr, n, unrooted)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, unrooted)
        assert got[0][-1] == len(reps) and (got[1] >= 1).all()          # the last merge is always found
        out.append(got)
    return out


@pytest.mark.parametrize("n", [2, 3, 4, 65, 300])
def test_counting_of_random_trees(pa, n):
    """random merge lists, replicates that share much with the reference (a few of its leaves swapped) and nothing planned"""
    rng = np.random.default_rng(n)
    tree = ref.random_merges(rng, n)
    reps = [ref.random_merges(rng, n) for _ in range(3)]
    for _ in range(4):                  # the reference with two leaves exchanged: most clades survive
        perm = np.arange(2 * n - 1)
        i, j = rng.choice(n, 2, replace=False)
        perm[i], perm[j] = j, i
        reps.append((perm[tree[0]].astype(np.uint32), perm[tree[1]].astype(np.uint32)))
    reps.append(tree)
    (rooted, shared), (unrooted, _) = _both(pa, tree, reps, n)
    assert shared[-1] == n - 1 and (unrooted >= rooted).all()           # a clade that comes back is a split that comes back


@pytest.mark.parametrize("n", [2, 5, 64, 129])
def test_identical_trees_have_full_support(pa, n):
    tree = ref.random_merges(np.random.default_rng(100 + n), n)
    for support, shared in _both(pa, tree, [tree] * 4, n):
        assert (support == 4).all() and (shared == n - 1).all()


def test_a_caterpillar_against_a_balanced_tree(pa):
    n = 64
    cat, bal = ref.caterpillar(n), ref.balanced(n)
    (rooted, shared), (unrooted, ushared) = _both(pa, cat, [bal, cat], n)
    # rooted: {0, 1}, {0 .. 3}, {0 .. 7}, ... are clades of both; the caterpillar's other clades are not the balanced tree's
    both = {2 ** k - 2 for k in range(1, 7)}
    assert [int(s) for s in rooted] == [2 if k in both else 1 for k in range(n - 1)] and list(shared) == [len(both), n - 1]
    # unrooted: these again; {0 .. 47} | {48 .. 63}, {0 .. 55} | {56 .. 63}, {0 .. 59} | {60 .. 63} and {0 .. 61} | {62, 63}, whose
    # far sides are clades of the balanced tree; and {0 .. 62} | {63}, which is in every tree
    more = both | {46, 54, 58, 60, 61}
    assert [int(s) for s in unrooted] == [2 if k in more else 1 for k in range(n - 1)] and list(ushared) == [len(more), n - 1]
    _both(pa, bal, [cat, bal], n)


def test_one_unrooted_tree_written_with_two_last_joins(pa):
    """((0, 1), (2, 3), (4, 5)) unrooted: closed as ((01, 23), 45) and as (01, (23, 45))"""
    n = 6
    one = (np.array([0, 2, 4, 6, 9], np.uint32), np.array([1, 3, 5, 7, 8], np.uint32))
    two = (np.array([0, 2, 4, 7, 6], np.uint32), np.array([1, 3, 5, 8, 9], np.uint32))
    for a, b in ((one, two), (two, one)):
        (rooted, shared), (unrooted, ushared) = _both(pa, a, [b], n)
        assert list(unrooted) == [1] * 5 and list(ushared) == [5]
        assert list(rooted) == [1, 1, 1, 0, 1] and list(shared) == [4]
    # the same with a leaf at the last join: the split {5} | rest is no merge of the other writing
    three = (np.array([0, 2, 6, 8, 9], np.uint32), np.array([1, 3, 7, 4, 5], np.uint32))     # ((((01, 23), 4), 5)
    for a, b in ((three, one), (one, three)):
        _, (unrooted, ushared) = _both(pa, a, [b], n)
        assert list(unrooted) == [1] * 5 and list(ushared) == [5]


def test_malformed_lists_are_refused(pa):
    n = 5
    good = ref.caterpillar(n)
    bad_lists = [(np.array([0, 5, 6, 7], np.uint32), np.array([1, 2, 3, 3], np.uint32)),        # leaf 3 twice, leaf 4 never
                 (np.array([0, 6, 6, 7], np.uint32), np.array([1, 2, 3, 4], np.uint32)),        # a node that does not exist yet
                 (np.array([0, 5, 5, 7], np.uint32), np.array([1, 2, 3, 4], np.uint32)),        # node 5 is a child twice
                 (np.array([0, 5, 6, 99], np.uint32), np.array([1, 2, 3, 4], np.uint32))]
    for bad in bad_lists:
        for ref_tree, rep in ((bad, good), (good, bad)):
            with pytest.raises(pa.PansimError) as e:
                pa.bootstrap_from_merges(ref_tree[0], ref_tree[1], rep[0].reshape(1, -1), rep[1].reshape(1, -1), n)
            assert e.value.code == PS_ERR_INVALID and "not an earlier node that is still free" in str(e.value)
    with pytest.raises(pa.PansimError) as e:
        pa.bootstrap_from_merges(good[0], good[1], np.stack([good[0], bad_lists[0][0]]), np.stack([good[1], bad_lists[0][1]]), n)
    assert "replicate 1" in str(e.value)
    with pytest.raises(ValueError):
        pa.bootstrap_from_merges(good[0], good[1], good[0].reshape(1, -1)[:, :3], good[1].reshape(1, -1)[:, :3], n)
    lib = pa.load()
    z = np.zeros(4, np.uint32)
    p = z.ctypes.data_as(C.c_void_p)
    assert lib.ps_bootstrap_from_merges(p, p, p, p, 1, 1, 0, p, p) == PS_ERR_INVALID                 # pop_size below 2
    assert lib.ps_bootstrap_from_merges(None, p, p, p, 1, 5, 0, p, p) == PS_ERR_INVALID


def test_result_object(pa):
    o = pa._lib.Bootstrap(6, 15, 100, 2, 2, 4, 100, 5, 14, 3, 2, 1)
    left, right = np.array([0, 2, 4, 6, 9, 0], np.uint32), np.array([1, 3, 5, 7, 8, 0], np.uint32)
    r = pa.BootstrapSupport(o, left, right, np.array([4, 3, 2, 1, 4, 0], np.uint32), np.array([5, 3, 2, 4], np.uint32))
    assert r.merges == 5 and r.replicates == 4 and r.supported_95 == 1
    assert [a.tolist() for a in r.merges()] == [[0, 2, 4, 6, 9], [1, 3, 5, 7, 8]]
    assert r.fraction.tolist() == [1.0, 0.75, 0.5, 0.25, 1.0] and r.shared.tolist() == [5, 3, 2, 4]
    d = r.as_dict()
    assert set(ref.INT_FIELDS) | {"left", "right", "support", "shared", "fraction"} == set(d) and d["support_sum"] == 14


def test_the_counting_under_the_sanitizers(tmp_path):
    """tests/bootstrap_count_check.cpp, a program of its own around boot_counter: built with -fsanitize=address,undefined and run"""
    exe = str(tmp_path / "bootstrap_count_check")
    src = os.path.join(ROOT, "tests", "bootstrap_count_check.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    # (leak checking needs ptrace, which a container may refuse; the program keeps nothing it allocates)
    out = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "bootstrap counting ok" in out.stdout
