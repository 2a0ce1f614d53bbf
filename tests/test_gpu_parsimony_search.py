"""Parsimony tree search on the device (ps_tree_nni_deltas, ps_tree_nni and its ps_sim / ps_multi forms, docs/PARSIMONY_SEARCH.md)
against the host entries bit for bit -- ps_nni_deltas_from_rows and ps_nni_from_rows, which tests/test_parsimony_search.py holds
against rescored neighbour trees -- and, at the small shapes, against the rescoring restatement itself.  The shapes are the
smallest at which each thing can still go wrong: the smallest tree with a candidate, the lane boundary, the single-wave team
against the shared tile (1024 / 1025), the LDS copy of the schedule (PS_NNI_LDS_SCHED: 2320 leaves have it, 2352 do not), LDS
counters against global atomics (PS_NNI_LDS_COUNTERS: 4096 / 4097), the largest tree (8192)."""
import numpy as np
import pytest

import parsimony_search_ref as ref
import tree_parsimony_ref as pref

pytestmark = pytest.mark.gpu

PS_ERR_INVALID, PS_ERR_STATE = -1, -6
SHAPES = [(4, 1, "random"), (5, 7, "caterpillar"), (64, 16, "balanced"), (65, 17, "caterpillar"), (1000, 203, "random"), (1024, 64, "balanced"),
          (1025, 64, "caterpillar"), (2320, 24, "random"), (2352, 24, "random"), (4096, 40, "random"), (4097, 24, "balanced"),
          (8192, 12, "random")]


def core_handle(pa, m, **kw):
    p = pa.Population(m.shape[0], m.shape[1], 4, True, 0.0, 0, 0, **kw)
    p.load_matrix(m)
    return p


def start_tree(rng, N, kind):
    if kind == "caterpillar":
        return pref.caterpillar(N, rng.permutation(N))
    if kind == "balanced":
        return pref.balanced(N, rng.permutation(N))
    return pref.random_joining(rng, N)


def assert_same_search(got, want):
    for name in got.FIELDS + ("n_moves",):
        assert getattr(got, name) == getattr(want, name), (name, getattr(got, name), getattr(want, name))
    assert np.array_equal(got.left, want.left) and np.array_equal(got.right, want.right)
    assert np.array_equal(got.round_changes, want.round_changes) and np.array_equal(got.moves, want.moves)


@pytest.mark.parametrize("N,L,kind", SHAPES)
def test_device_equals_host(pa, N, L, kind):
    """data evolved on one tree, the search started from another; arbitrary bytes on every second shape"""
    rng = np.random.default_rng(N * 31 + L)
    truth = pref.random_joining(rng, N)
    m = pref.evolved(rng, N, L, *truth, junk=L % 2 == 0)
    if L >= 16:
        m[:, 8:12] = 4                                              # a fully monomorphic tile: the skip path
    left, right = start_tree(rng, N, kind)
    if N == 2320:
        assert pa.parsimony_schedule(left, right, N)[1] <= 148       # (the schedule's LDS copy fits)
    core = core_handle(pa, m)
    T, d = core.nni_deltas(left, right)
    hT, hd = pa.nni_deltas_from_rows(m, left, right)
    assert T == hT and np.array_equal(d, hd)
    assert T == core.tree_parsimony(left, right).total_changes and int((d != ref.NONE).sum()) == 2 * max(0, N - 3)
    if N >= 64:
        assert (d[d != ref.NONE] < 0).any() and (d > 0).any()
    if N <= 65:
        wT, wd = ref.deltas(ref.class_bits(m), left, right)
        assert T == wT and np.array_equal(d, wd)
    for kw in (dict(max_rounds=4 if N >= 4096 else 40), dict(max_rounds=3, moves_per_round=2)):
        got, want = core.tree_nni(left, right, **kw), pa.nni_from_rows(m, left, right, **kw)
        assert_same_search(got, want)
        assert got.passes == got.rounds + got.rollbacks + 1 and (np.diff(got.round_changes.astype(np.int64)) < 0).all()
        assert core.tree_parsimony(got.left, got.right).total_changes == got.total_changes
        if N >= 64:
            assert got.rounds >= 1 and got.total_changes < got.start_changes
    core.close()


SIM = dict(pop_size=100, core_size=2001, pan_genes=300, core_genes=20, HR_rate=0.5, HGT_rate=0.5, seed=11, n_gen=8, max_distances=100)


def test_a_simulation_and_no_change_of_state(pa):
    """the UPGMA tree of a short run refined: leaves are rows of the reference's row order while the matrix is stored in
    another; the run continues as if it had not been asked"""
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(6)
    left, right = sim.upgma_tree().merges()
    parents = sim.last_parents()
    assert (np.diff(parents.astype(np.int64)) < 0).any()                             # the internal order is not the output order
    m = sim.core_genome.read_matrix()
    before = sim.tree_parsimony(left, right, per_site=True, branches=True)
    got, want = sim.tree_nni(left, right), pa.nni_from_rows(m, left, right)
    assert_same_search(got, want)
    assert got.rounds >= 1 and got.local_optimum and got.sites == 2001 and got.start_changes == before.total_changes
    T, d = sim.core_genome.nni_deltas(left, right)
    hT, hd = pa.nni_deltas_from_rows(m, left, right)
    assert T == hT and np.array_equal(d, hd)
    ms = sim.tree_nni_timing()
    assert len(ms) == 2 and ms[0] >= 0.0 and ms[1] > 0.0
    # the matrix and a following tree_parsimony are as before, and the run goes on bit for bit
    assert np.array_equal(sim.core_genome.read_matrix(), m)
    after = sim.tree_parsimony(left, right, per_site=True, branches=True)
    assert np.array_equal(after.site_changes, before.site_changes) and np.array_equal(after.branch_changes, before.branch_changes)
    compare = sim.tree_compare((left, right), got.merges())
    assert compare.pop_size == 100 and compare.merges_b == 99
    sim.run(2)
    plain = pa.Simulation(pa.make_params(**SIM))
    plain.run(8)
    assert np.array_equal(plain.core_genome.read_matrix(), sim.core_genome.read_matrix())
    assert np.array_equal(plain.pan_genome.read_matrix(), sim.pan_genome.read_matrix())
    plain.close()
    sim.close()


@pytest.mark.parametrize("shards", [2, 3])
def test_multi_simulation_equals_the_unsharded_run(pa, shards):
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(5)
    left, right = sim.upgma_tree().merges()
    want, m = sim.tree_nni(left, right), sim.core_genome.read_matrix()
    assert want.rounds >= 1
    sim.close()
    multi = pa.MultiSimulation(pa.make_params(**SIM), shards, devices=[0] * shards)
    multi.run(5)
    assert_same_search(multi.tree_nni(left, right), want)
    assert_same_search(multi.tree_nni(left, right, max_rounds=2, moves_per_round=1),
                       pa.nni_from_rows(m, left, right, max_rounds=2, moves_per_round=1))
    ms = multi.tree_nni_timing()
    assert len(ms) == 2 and ms[1] > 0.0
    multi.close()


def test_three_site_shards_add_to_the_whole(pa):
    rng = np.random.default_rng(4)
    N, L = 130, 1000
    m = pref.evolved(rng, N, L, *pref.random_joining(rng, N))
    left, right = pref.random_joining(rng, N)
    wT, wd = pa.nni_deltas_from_rows(m, left, right)
    cuts = [0, 333, 701, L]
    T, d = 0, np.zeros_like(wd)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        shard = core_handle(pa, np.ascontiguousarray(m[:, lo:hi]), col_offset=lo, global_cols=L)
        pT, pd = shard.nni_deltas(left, right)
        hT, hd = pa.nni_deltas_from_rows(m[:, lo:hi], left, right)
        assert pT == hT and np.array_equal(pd, hd)
        assert shard.tree_nni(left, right, max_rounds=2).sites == hi - lo
        shard.close()
        T += pT
        d = np.where(pd == ref.NONE, ref.NONE, d + np.where(pd == ref.NONE, 0, pd))
    assert T == wT and np.array_equal(d, wd)


def test_the_scratch_grows_and_timing(pa):
    rng = np.random.default_rng(8)
    N, L = 500, 300
    shallow, deep = pref.balanced(N, rng.permutation(N)), pref.caterpillar(N, rng.permutation(N))
    m = pref.evolved(rng, N, L, *pref.random_joining(rng, N))
    core = core_handle(pa, m)
    with pytest.raises(pa.PansimError) as e:
        core.tree_nni_timing()                                      # nothing to report yet
    assert e.value.code == PS_ERR_STATE
    # (the level offsets of the caterpillar need more scratch than those of the balanced tree)
    for left, right in (shallow, deep, shallow):
        T, d = core.nni_deltas(left, right)
        hT, hd = pa.nni_deltas_from_rows(m, left, right)
        assert T == hT and np.array_equal(d, hd)
        ms = core.tree_nni_timing()
        assert len(ms) == 2 and ms[0] >= 0.0 and ms[1] > 0.0
    one = core.tree_nni_timing()[1]
    got = core.tree_nni(*shallow, max_rounds=3)
    assert got.passes >= 3 and core.tree_nni_timing()[1] > one      # the sum over the passes of the call
    core.close()


def test_handle_checks(pa):
    rng = np.random.default_rng(6)
    core = core_handle(pa, pref.onehot(rng, (20, 64)))
    acc = pa.Population(20, 10, 2, False, 0.5, 0, 3)
    left, right = pref.caterpillar(20)
    for call in (lambda: acc.tree_nni(left, right), lambda: acc.nni_deltas(left, right)):
        with pytest.raises(pa.PansimError) as e:
            call()
        assert e.value.code == PS_ERR_INVALID and "core handle" in str(e.value)
    for bad_left, bad_right, kw, text in ((left[:-1], right[:-1], {}, "spanning tree: 19 merges over 20 leaves, not 18"),
                                          (left, right, dict(max_rounds=0), "max_rounds must be at least 1"),
                                          ([0] * 19, list(range(1, 20)), {}, "a child of merge")):
        with pytest.raises(pa.PansimError) as e:
            core.tree_nni(bad_left, bad_right, **kw)
        assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)
    with pytest.raises(pa.PansimError) as e:
        core.nni_deltas(left[:-1], right[:-1])
    assert e.value.code == PS_ERR_INVALID and "spanning tree" in str(e.value)
    big = pa.Population(8193, 16, 4, True, 0.0, 0, 0)
    with pytest.raises(pa.PansimError) as e:
        big.tree_nni(*pref.caterpillar(8193))
    assert e.value.code == PS_ERR_INVALID and "pop_size <= 8192" in str(e.value)
    for p in (core, acc, big):
        p.close()
