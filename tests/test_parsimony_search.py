"""Parsimony tree search without a device (docs/PARSIMONY_SEARCH.md): the host entries ps_nni_deltas_from_rows, ps_nni_from_rows,
ps_merges_canonical and ps_nni_apply against the restatement (tests/parsimony_search_ref.py), which gets every delta by scoring
the neighbour tree from scratch; the rollback path; data without homoplasy; the error paths and the plumbing.  The device half
is tests/test_gpu_parsimony_search.py.  Every comparison is an equality."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import parsimony_search_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS_ERR_INVALID, PS_ERR_NO_DEVICE = -1, -2
NEW_SYMBOLS = ("ps_tree_nni_deltas", "ps_tree_nni", "ps_sim_tree_nni", "ps_multi_tree_nni", "ps_tree_nni_timing", "ps_nni_deltas_from_rows",
               "ps_nni_from_rows", "ps_merges_canonical", "ps_nni_apply")


def junk_matrix(rng, N, L, states=4):
    """one-hot cells with some arbitrary bytes, 0, 3 and 255 among them"""
    m = ref.onehot(rng, (N, L), states)
    bad = rng.random((N, L)) < 0.15
    m[bad] = rng.choice(np.array([0, 3, 255, 16, 7], np.uint8), int(bad.sum()))
    return m


def trees(rng, N):
    return [ref.balanced(N), ref.caterpillar(N, rng.permutation(N)), ref.random_tree(rng, N), ref.random_tree(rng, N)]


@pytest.mark.parametrize("N", [4, 5, 6, 7, 9, 13, 16, 24])
def test_deltas_equal_the_rescored_neighbours(pa, N):
    rng = np.random.default_rng(100 + N)
    for left, right in trees(rng, N):
        L = int(rng.integers(1, 61))
        m = junk_matrix(rng, N, L)
        m[0, 0], m[1, 0], m[2, 0] = 0, 3, 255
        T, d = pa.nni_deltas_from_rows(m, left, right)
        wT, wd = ref.deltas(ref.class_bits(m), left, right)
        assert T == wT and d.dtype == np.int64 and np.array_equal(d, wd), (N, L)
        # 2 (N - 3) neighbours: every internal edge of the unrooted tree has two
        root_kids_internal = left[-1] >= N and right[-1] >= N
        inner = sum(1 for k in range(N - 2) if N + k not in (left[-1], right[-1]))
        assert int((d != ref.NONE).sum()) == 2 * (inner + (1 if root_kids_internal else 0)) == 2 * (N - 3)
        assert T == pa.parsimony_from_rows(m, left, right).total_changes


def test_two_and_three_leaves_have_no_candidates(pa):
    T, d = pa.nni_deltas_from_rows(np.array([[1, 2], [2, 2]], np.uint8), [0], [1])
    assert T == 1 and d.tolist() == [[ref.NONE, ref.NONE]] and pa.PS_NNI_NONE == ref.NONE
    T, d = pa.nni_deltas_from_rows(np.array([[1], [2], [2]], np.uint8), [0, 3], [1, 2])
    assert T == 1 and (d == ref.NONE).all()
    got = pa.nni_from_rows(np.array([[1], [2], [2]], np.uint8), [0, 3], [1, 2])
    assert got.rounds == 0 and got.passes == 1 and got.local_optimum and got.total_changes == 1 and got.moves.size == 0
    assert got.left.tolist() == [0, 3] and got.right.tolist() == [1, 2]


@pytest.mark.parametrize("N", [4, 7, 12, 33])
def test_canonical_form(pa, N):
    """idempotent, invariant under renumbering the internal nodes and swapping children, the clades unchanged, the rules of the
    document hold on the result"""
    rng = np.random.default_rng(200 + N)
    for left, right in trees(rng, N):
        cl, cr = pa.merges_canonical(left, right, N)
        wl, wr = ref.canonical(*ref.tree_of(left, right, N), N)
        assert np.array_equal(cl, wl) and np.array_equal(cr, wr)
        again = pa.merges_canonical(cl, cr, N)
        assert np.array_equal(again[0], cl) and np.array_equal(again[1], cr)
        assert ref.clades(cl, cr, N) == ref.clades(left, right, N)
        assert ref.root_split(cl, cr, N) in (ref.root_split(left, right, N), ref.root_split(left, right, N)[::-1])
        # another valid numbering of the same rooted tree: a random order that keeps children before parents, children swapped
        kids, root = ref.tree_of(left, right, N)
        order, ready = [], [x for x in kids if all(c < N for c in kids[x])]
        placed = set(range(N))
        while ready:
            x = ready.pop(int(rng.integers(len(ready))))
            order.append(x)
            placed.add(x)
            ready += [y for y in kids if y not in placed and y not in ready and all(c in placed for c in kids[y])]
        ident = {x: N + k for k, x in enumerate(order)}
        l2, r2 = [], []
        for x in order:
            a, b = (ident.get(c, c) for c in kids[x])
            if rng.random() < 0.5:
                a, b = b, a
            l2.append(a)
            r2.append(b)
        other = pa.merges_canonical(l2, r2, N)
        assert np.array_equal(other[0], cl) and np.array_equal(other[1], cr)
        level_of, _ = pa.parsimony_schedule(cl, cr, N)
        low = list(range(N))
        for a, b in zip(cl, cr):
            assert low[a] < low[b]
            low.append(low[a])
        keys = list(zip(level_of.tolist(), low[N:]))
        assert keys == sorted(keys) and len(set(keys)) == N - 1


def test_apply_equals_the_restatement(pa):
    rng = np.random.default_rng(3)
    for N in (4, 5, 8, 15):
        for left, right in trees(rng, N):
            kids, root = ref.tree_of(left, right, N)
            for k in range(N - 1):
                for kind in (0, 1):
                    nb = ref.neighbour(kids, root, N + k, kind)
                    if nb is None:
                        with pytest.raises(pa.PansimError) as e:
                            pa.nni_apply(left, right, N, N + k, kind)
                        assert e.value.code == PS_ERR_INVALID and "no interchange" in str(e.value)
                        continue
                    got = pa.nni_apply(left, right, N, N + k, kind)
                    want = ref.canonical(nb[0], root, N)
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def check_search(pa, m, left, right, **kw):
    got = pa.nni_from_rows(m, left, right, **kw)
    want = ref.search(m, left, right, **kw)
    ref.assert_search_equal(got, want)
    N = m.shape[0]
    assert got.passes == got.rounds + got.rollbacks + 1 and got.round_changes.size == got.rounds + 1
    assert (np.diff(got.round_changes.astype(np.int64)) < 0).all()
    assert got.round_changes[0] == got.start_changes and got.round_changes[-1] == got.total_changes
    end = pa.parsimony_from_rows(m, got.left, got.right)
    assert end.total_changes == got.total_changes and end.min_changes == got.min_changes and end.spanning == 1
    again = pa.merges_canonical(got.left, got.right, N)
    assert np.array_equal(again[0], got.left) and np.array_equal(again[1], got.right)
    if got.local_optimum:
        _, d = ref.deltas(ref.class_bits(m), got.left, got.right)
        assert (d >= 0).all() and got.candidates_last == 0
    else:
        assert got.rounds == kw.get("max_rounds", 1000) and got.candidates_last > 0
    return got


@pytest.mark.parametrize("moves_per_round", [1, 3, 0])
def test_search_equals_the_restatement_move_for_move(pa, moves_per_round):
    rng = np.random.default_rng(40 + moves_per_round)
    improved = 0
    for N in (4, 6, 9, 14, 20):
        for left, right in trees(rng, N)[1:]:
            m = junk_matrix(rng, N, int(rng.integers(5, 40)), states=3)
            got = check_search(pa, m, left, right, moves_per_round=moves_per_round)
            improved += got.rounds > 0
            if moves_per_round:
                assert np.bincount(got.moves["round"], minlength=2).max() <= moves_per_round
    assert improved >= 5


def test_max_rounds_stops_the_search(pa):
    rng = np.random.default_rng(5)
    N = 16
    left, right = ref.caterpillar(N, rng.permutation(N))
    m = ref.onehot(rng, (N, 30), 3)
    full = check_search(pa, m, left, right, moves_per_round=1)
    assert full.rounds >= 3 and full.local_optimum
    cut = check_search(pa, m, left, right, moves_per_round=1, max_rounds=2)
    assert cut.rounds == 2 and not cut.local_optimum and cut.round_changes.tolist() == full.round_changes[:3].tolist()


def test_the_rollback_path(pa):
    """moves of one batch touch disjoint nodes but their deltas need not add: the seeded cases must contain batches that end
    above T + the best delta, and the search must answer them as the restatement does"""
    rollbacks = 0
    for seed in range(300):
        rng = np.random.default_rng(7000 + seed)
        N, L = int(rng.integers(8, 15)), int(rng.integers(3, 13))
        left, right = ref.random_tree(rng, N)
        m = ref.onehot(rng, (N, L), 3)
        got = pa.nni_from_rows(m, left, right)
        if got.rollbacks:
            rollbacks += 1
            check_search(pa, m, left, right)
    assert rollbacks >= 3, rollbacks


def supported_tree_data(rng, left, right, N):
    """one site per inner edge of the tree (state 2 below it, 1 elsewhere) and per leaf, in random order: no homoplasy"""
    below = {i: [i] for i in range(N)}
    cols = []
    for k, (a, b) in enumerate(zip(left, right)):
        below[N + k] = below[int(a)] + below[int(b)]
        if k < N - 2:
            col = np.ones(N, np.uint8)
            col[below[N + k]] = 2
            cols.append(col)
    for i in range(N):
        col = np.full(N, 4, np.uint8)
        col[i] = 8
        cols.append(col)
    return np.stack([cols[i] for i in rng.permutation(len(cols))], axis=1)


@pytest.mark.parametrize("N", [5, 8, 13])
def test_data_without_homoplasy(pa, N):
    rng = np.random.default_rng(60 + N)
    left, right = pa.merges_canonical(*ref.random_tree(rng, N), N)
    m = supported_tree_data(rng, left, right, N)
    got = pa.nni_from_rows(m, left, right)
    assert got.rounds == 0 and got.passes == 1 and got.local_optimum and got.total_changes == got.min_changes == got.start_changes
    assert np.array_equal(got.left, left) and np.array_equal(got.right, right)
    T, d = pa.nni_deltas_from_rows(m, left, right)
    assert (d > 0).all()
    tried = 0
    for k in range(N - 1):
        for kind in (0, 1):
            if d[k, kind] == ref.NONE:
                continue
            nl, nr = pa.nni_apply(left, right, N, N + k, kind)
            back = pa.nni_from_rows(m, nl, nr)
            assert back.rounds == 1 and back.local_optimum and back.total_changes == back.min_changes
            assert back.start_changes == T + d[k, kind] and back.moves.size == 1 and back.moves["delta"][0] == -d[k, kind]
            assert np.array_equal(back.left, left) and np.array_equal(back.right, right)
            tried += 1
    assert tried == 2 * (N - 3)


@pytest.mark.parametrize("call,left,right,N,kw,text", [
    ("search", [0] * 8192, [1] * 8192, 8193, {}, "pop_size <= 8192"),
    ("search", [0], [1], 1, {}, "pop_size <= 8192"),
    ("search", [0, 2], [1, 3], 5, {}, "spanning tree: 4 merges over 5 leaves, not 2"),
    ("search", [0, 4, 5], [1, 2, 3], 4, {"max_rounds": 0}, "max_rounds must be at least 1"),
    ("search", [0, 0, 5], [1, 2, 3], 4, {}, "a child of merge"),
    ("search", [0, 6, 5], [1, 2, 3], 4, {}, "not a node below"),
    ("deltas", [0, 2], [1, 3], 5, {}, "spanning tree"),
    ("deltas", [0, 4, 4], [1, 2, 3], 4, {}, "a child of merge"),
    ("canonical", [0, 2], [1, 3], 5, {}, "spanning tree"),
    ("canonical", [0, 4, 5], [1, 2, 6], 4, {}, "not a node below")])
def test_bad_arguments(pa, call, left, right, N, kw, text):
    m = np.ones((N, 3), np.uint8)
    with pytest.raises(pa.PansimError) as e:
        if call == "search":
            pa.nni_from_rows(m, left, right, **kw)
        elif call == "deltas":
            pa.nni_deltas_from_rows(m, left, right)
        else:
            pa.merges_canonical(left, right, N)
    assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)


def test_bad_candidates_of_apply(pa):
    for node, kind, text in ((2, 0, "no interchange"), (7, 0, "no interchange"), (4, 2, "kind must be 0 or 1")):
        with pytest.raises(pa.PansimError) as e:
            pa.nni_apply([0, 4, 5], [1, 2, 3], 4, node, kind)
        assert e.value.code == PS_ERR_INVALID and text in str(e.value)
    with pytest.raises(ValueError):
        pa.nni_from_rows(np.ones(4, np.uint8), [0], [1])


def test_plumbing(pa):
    from pansim_amd import simulation
    lib = C.CDLL(pa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pansim_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in pa._lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
    assert lib.ps_abi_version() == 3
    assert "#define PS_NNI_MAX_POP 8192u" in hdr and pa.PS_NNI_MAX_POP == 8192 and "#define PS_NNI_NONE INT64_MAX" in hdr
    assert C.sizeof(pa._lib.Nni) == 12 * 8 and C.sizeof(pa._lib.NniParams) == 8
    assert "tree_nni" in vars(simulation._Search) and "tree_nni" not in vars(simulation._Readouts)
    for cls in (pa.Simulation, pa.MultiSimulation):
        assert simulation._Search in cls.__mro__ and "tree_nni" not in vars(cls)


def test_run_methods_ask_for_the_entry_of_their_class(pa):
    """written once in _Search; no device: the library is an object that notes the first symbol asked for"""
    from pansim_amd import _lib

    class Asked(Exception):
        pass

    class Library:
        def __getattr__(self, name):
            raise Asked(name)

    for cls, symbol in ((pa.Simulation, "ps_sim_tree_nni"), (pa.MultiSimulation, "ps_multi_tree_nni")):
        run = object.__new__(cls)
        run._lib, run._h = Library(), None
        run.params = _lib.SimParams(pop_size=4, core_size=100, pan_genes=60, core_genes=20, max_distances=10)
        with pytest.raises(Asked) as e:
            run.tree_nni([0, 4, 5], [1, 2, 3])
        assert str(e.value) == symbol and symbol in _lib.SIGNATURES


def test_the_device_entries_need_a_device(pa):
    """without a device the device entries fail with PS_ERR_NO_DEVICE before they look at their arguments; with one, the same
    calls refuse their null arguments; the timing entry refuses a null handle either way"""
    lib = pa.load()
    out, prm = pa._lib.Nni(), pa._lib.NniParams(1, 0)
    bad = np.zeros(4, np.uint32)
    rest = [None] * 7 + [0]
    want = PS_ERR_NO_DEVICE if lib.ps_device_count() <= 0 else PS_ERR_INVALID
    total = C.c_uint64()
    assert lib.ps_tree_nni_deltas(None, bad.ctypes.data, bad.ctypes.data, 4, C.byref(total), None) == want
    for fn in (lib.ps_tree_nni, lib.ps_sim_tree_nni, lib.ps_multi_tree_nni):
        assert fn(None, bad.ctypes.data, bad.ctypes.data, 4, C.byref(prm), C.byref(out), *rest) == want
    if want == PS_ERR_NO_DEVICE:
        assert "no HIP device" in lib.ps_last_error().decode()
    assert lib.ps_tree_nni_timing(None, None, None) == PS_ERR_INVALID
