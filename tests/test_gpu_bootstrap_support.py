"""Bootstrap support on the device (ps_bootstrap_support and its ps_sim / ps_multi forms, docs/BOOTSTRAP_SUPPORT.md) against a
path that shares none of the new kernels (tests/bootstrap_ref.py): per replicate the matrix M[:, sites_b] is built in NumPy --
from the restated draw rule, or from the test's own lists --, loaded into a fresh Population of `draws` sites, the existing
tree method is called on it, and the supports are counted on frozensets.  Every comparison is an equality."""
import numpy as np
import pytest

import bootstrap_ref as ref

pytestmark = pytest.mark.gpu

PS_ERR_INVALID, PS_ERR_STATE = -1, -6
BASES = np.array([1, 2, 4, 8], np.uint8)


def _onehot(rng, N, L):
    return BASES[rng.integers(0, 4, (N, L))]


def _structured(rng, N, L, levels=5):
    """one-hot rows with some tree signal: the population halves `levels` times, every half mutating a tenth of the sites"""
    m = np.tile(_onehot(rng, 1, L), (N, 1))
    for lev in range(levels):
        for part in np.array_split(rng.permutation(N), 2 ** (lev + 1)):
            cols = rng.choice(L, max(1, L // 10), replace=False)
            m[np.ix_(part, cols)] = _onehot(rng, 1, cols.size)
    return m


def _handles(pa, core_matrix, acc_matrix, cg):
    N, L = core_matrix.shape
    core = pa.Population(N, L, 4, True, 0.0, 0, cg)
    core.load_matrix(core_matrix)
    acc = pa.Population(N, acc_matrix.shape[1], 2, False, 0.5, 0, cg)
    acc.load_matrix(acc_matrix)
    return core, acc


def _lists(seed, replicates, L, draws, sites):
    return [np.asarray(s) for s in sites] if sites is not None else [ref.draw_sites(seed, b, L, draws) for b in range(replicates)]


def _assert_equal(got, want, n, L, cg, method, replicates, draws):
    left, right, support, shared = want
    assert np.array_equal(got.left, left) and np.array_equal(got.right, right)
    assert np.array_equal(got.support, support), (method, draws, got.support, support)
    assert np.array_equal(got.shared, shared)
    assert {k: getattr(got, k) for k in ref.INT_FIELDS} == ref.summary(n, L, cg, method, replicates, draws, support)
    assert got.support[-1] == replicates and np.array_equal(got.fraction, support / np.float64(replicates))


def _check(pa, core, acc, matrix, acc_matrix, cg, method, replicates=3, seed=0, draws=None, sites=None):
    """the device == the independent path; the reference tree == the method's own entry on the same handles -> the device's"""
    n, L = matrix.shape
    got = core.bootstrap_support(acc, method=method, replicates=replicates, seed=seed, draws=draws, sites=sites)
    d = L if draws is None else draws
    if sites is not None:
        d = np.asarray(sites).shape[1]
    want = ref.independent(pa, matrix, acc_matrix, cg, method, _lists(seed, replicates, L, d, sites))
    _assert_equal(got, want, n, L, cg, method, replicates, d)
    own = ref.tree_merges(pa, core, acc, method)
    assert np.array_equal(got.left, own[0]) and np.array_equal(got.right, own[1])
    return got


@pytest.mark.parametrize("N", [2, 3, 65, 257])
def test_sizes_methods_and_draws(pa, N):
    """L = 130: draws = L, 17 (a string shorter than two dwords) and 3 L (strings longer than the matrix's, ending inside a
    dword); N below, at and past a tile of individuals"""
    rng = np.random.default_rng(N)
    m, a = _structured(rng, N, 130), (rng.random((N, 40)) < 0.3).astype(np.uint8)
    core, acc = _handles(pa, m, a, 3)
    for k, method in enumerate(ref.METHODS):
        for draws in (None, 17, 390):
            _check(pa, core, acc, m, a, 3, method, replicates=3 + k % 3, seed=N + k, draws=draws)
    core.close()
    acc.close()


@pytest.mark.parametrize("band", [0, 256])
def test_two_bands(pa, band):
    """N = 300 = 256 + 44, L = 320; band 256: the counts of a replicate arrive in two pieces"""
    rng = np.random.default_rng(5)
    m, a = _structured(rng, 300, 320), (rng.random((300, 130)) < 0.3).astype(np.uint8)
    core, acc = _handles(pa, m, a, 7)
    core.set_tuning("core_davg_band", band)
    for method in ref.METHODS:
        _check(pa, core, acc, m, a, 7, method, replicates=3, seed=band + 1)
    core.close()
    acc.close()


def test_the_callers_lists(pa):
    N, L = 65, 130
    rng = np.random.default_rng(9)
    m = _structured(rng, N, L)
    mono = np.array([3, 64, 65, 129])
    m[:, mono] = 4                                         # four sites at which everyone carries the same base
    a = (rng.random((N, 40)) < 0.3).astype(np.uint8)
    core, acc = _handles(pa, m, a, 3)
    for method in ref.METHODS:
        # a permutation of all sites is the matrix again: the known answer
        got = _check(pa, core, acc, m, a, 3, method, sites=np.stack([rng.permutation(L) for _ in range(3)]))
        assert (got.support == 3).all() and (got.shared == N - 1).all() and got.support_sum == 3 * (N - 1)
        assert got.supported_50 == got.supported_70 == got.supported_95 == N - 2
        # one site, drawn 40 times (a wave fills its run) and 7 times (its thread does)
        _check(pa, core, acc, m, a, 3, method, sites=np.array([[17] * 40, [129] * 40, [0] * 40]))
        _check(pa, core, acc, m, a, 3, method, sites=np.array([[17] * 7, [128] * 7, [1] * 7]))
        # a jackknife: half the sites without repeats, in descending order
        _check(pa, core, acc, m, a, 3, method, sites=np.stack([np.sort(rng.choice(L, 65, replace=False))[::-1] for _ in range(3)]))
    # only monomorphic sites: all distances are 0 and the tree is the tie rule's, under neighbour joining the caterpillar
    got = _check(pa, core, acc, m, a, 3, "nj", sites=mono[rng.integers(0, 4, (3, 50))])
    rl, rr = ref.caterpillar(N)
    want = ref.support_from_merges(got.left, got.right, [rl] * 3, [rr] * 3, N, True)
    assert np.array_equal(got.support, want[0]) and np.array_equal(got.shared, want[1])
    # an index that is no site
    bad = rng.integers(0, L, (3, 20))
    bad[2, 11] = L
    fresh, fresh_acc = _handles(pa, m, a, 3)               # (refused before any device work: nothing computed on it afterwards)
    with pytest.raises(pa.PansimError) as e:
        fresh.bootstrap_support(fresh_acc, replicates=3, sites=bad)
    assert e.value.code == PS_ERR_INVALID and "replicate 2, position 11" in str(e.value)
    with pytest.raises(pa.PansimError) as e:
        fresh.bootstrap_support_timing()
    assert e.value.code == PS_ERR_STATE
    for p in (core, acc, fresh, fresh_acc):
        p.close()


def test_mostly_monomorphic_sites(pa):
    """N = 70, L = 600 of which 40 vary: most of a replicate's list adds nothing to any pair"""
    rng = np.random.default_rng(13)
    N, L = 70, 600
    m = np.full((N, L), 2, np.uint8)
    cols = rng.choice(L, 40, replace=False)
    m[:, cols] = _structured(rng, N, 40)
    a = (rng.random((N, 30)) < 0.3).astype(np.uint8)
    core, acc = _handles(pa, m, a, 2)
    for method in ref.METHODS:
        _check(pa, core, acc, m, a, 2, method, replicates=4, seed=21)
    core.close()
    acc.close()


def test_arbitrary_bytes_are_refused(pa):
    rng = np.random.default_rng(3)
    core, acc = _handles(pa, rng.integers(0, 256, (70, 130), dtype=np.uint8), (rng.random((70, 40)) < 0.2).astype(np.uint8), 3)
    onehot, acc2 = _handles(pa, _onehot(rng, 70, 130), (rng.random((70, 40)) < 0.2).astype(np.uint8), 3)
    onehot.set_tuning("core_davg_form", 3)                 # the generic form forced on a one-hot matrix
    for c, a in ((core, acc), (onehot, acc2)):
        for method in ref.METHODS:
            with pytest.raises(pa.PansimError) as e:
                c.bootstrap_support(a, method=method, replicates=3)
            assert e.value.code == PS_ERR_INVALID and "one-hot matrices only" in str(e.value)
        with pytest.raises(pa.PansimError) as e:
            c.bootstrap_support_timing()
        assert e.value.code == PS_ERR_STATE
    onehot.set_tuning("core_davg_form", 0)
    assert onehot.bootstrap_support(acc2, replicates=2).replicates == 2
    for p in (core, acc, onehot, acc2):
        p.close()


def test_limits_and_timing(pa):
    """refused before any device work: nothing has been computed on the handle afterwards"""
    rng = np.random.default_rng(6)
    core, acc = _handles(pa, _onehot(rng, 20, 64), (rng.random((20, 10)) < 0.5).astype(np.uint8), 2)
    for kw, text in ((dict(replicates=0), "1 <= replicates <= 65535"), (dict(replicates=65536), "1 <= replicates <= 65535"),
                     (dict(draws=2**31), "1 <= draws < 2^31")):
        with pytest.raises(pa.PansimError) as e:
            core.bootstrap_support(acc, **kw)
        assert e.value.code == PS_ERR_INVALID and text in str(e.value)
    with pytest.raises(ValueError):
        core.bootstrap_support(acc, method="parsimony")
    with pytest.raises(ValueError):
        core.bootstrap_support(acc, replicates=3, sites=np.zeros((2, 5), np.uint32))
    big_core, big_acc = pa.Population(16385, 8, 4, True, 0.0, 0, 0), pa.Population(16385, 4, 2, False, 0.5, 0, 2)
    for method in ("upgma", "nj"):
        with pytest.raises(pa.PansimError) as e:
            big_core.bootstrap_support(big_acc, method=method, replicates=2)
        assert e.value.code == PS_ERR_INVALID and "pop_size <= 16384" in str(e.value)
    wide = pa.Population(20, 65536, 2, False, 0.5, 0, 2)
    with pytest.raises(pa.PansimError) as e:
        core.bootstrap_support(wide)
    assert e.value.code == PS_ERR_INVALID and "65535 accessory genes" in str(e.value)
    for a, b in ((core, core), (acc, acc), (acc, core)):
        with pytest.raises(pa.PansimError) as e:
            a.bootstrap_support(b)
        assert e.value.code == PS_ERR_INVALID and "core handle first" in str(e.value)
    shard = pa.Population(20, 32, 4, True, 0.0, 0, 0, col_offset=32, global_cols=64)      # a site shard on its own
    with pytest.raises(pa.PansimError) as e:
        shard.bootstrap_support(acc)
    assert e.value.code == PS_ERR_INVALID and "ps_multi_bootstrap_support" in str(e.value)
    for p in (core, big_core, shard):
        with pytest.raises(pa.PansimError) as e:
            p.bootstrap_support_timing()
        assert e.value.code == PS_ERR_STATE and "no bootstrap support" in str(e.value)
    for method in ref.METHODS:
        own = {"linkage": core.linkage_tree, "upgma": core.upgma_tree, "nj": core.neighbour_joining}[method]
        own_timing = {"linkage": core.linkage_tree_timing, "upgma": core.upgma_tree_timing, "nj": core.neighbour_joining_timing}[method]
        own(acc)
        assert core.bootstrap_support(acc, method=method, replicates=5, seed=3).merges == 19
        lists_ms, operands_ms, trees_ms = core.bootstrap_support_timing()
        assert lists_ms > 0.0 and operands_ms > 0.0 and trees_ms > 0.0
        assert all(t > 0.0 for t in own_timing())          # (the method's own times: those of the reference tree)
    for p in (core, acc, big_core, big_acc, wide, shard):
        p.close()


SIM = dict(pop_size=200, core_size=2048, pan_genes=300, core_genes=20, HR_rate=0.5, HGT_rate=0.5, seed=11, n_gen=9, max_distances=100)
SAMPLE = np.random.default_rng(12).choice(200, 60, replace=False)
ONE_SHARD = np.random.default_rng(14).integers(0, 600, (2, 50))       # sites that all lie in shard 0 of two and of three


@pytest.fixture(scope="module")
def sim_after_six(pa):
    """the unsharded run after 6 generations: its supports (drawn, and from a list whose sites lie in one shard), the independent
    path's on read_matrix() of its handles (output rows), the supports of a sample of its rows, its state after 3 more"""
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(6)
    got = {method: sim.bootstrap_support(method=method, replicates=3, seed=5) for method in ref.METHODS}     # no sync: behind the run
    listed = sim.bootstrap_support(method="upgma", replicates=2, sites=ONE_SHARD)
    timing = sim.bootstrap_support_timing()
    m, a = sim.core_genome.read_matrix(), sim.pan_genome.read_matrix()
    want = {method: ref.independent(pa, m, a, 20, method, _lists(5, 3, 2048, 2048, None)) for method in ref.METHODS}
    want_listed = ref.independent(pa, m, a, 20, "upgma", list(ONE_SHARD))
    sc, sa = sim.subset(SAMPLE)
    sample = sc.bootstrap_support(sa, method="nj", replicates=3, seed=8), sc.read_matrix(), sa.read_matrix()
    sc.close()
    sa.close()
    sim.run(3)
    state = (sim.core_genome.read_matrix(), sim.pan_genome.read_matrix(), sim.last_parents())
    sim.close()
    return got, want, listed, want_listed, state, sample, timing


def test_row_order_in_a_simulation(pa, sim_after_six):
    got, want, listed, want_listed, state, _, timing = sim_after_six
    for method in ref.METHODS:
        _assert_equal(got[method], want[method], 200, 2048, 20, method, 3, 2048)
    _assert_equal(listed, want_listed, 200, 2048, 20, "upgma", 2, 50)
    assert len(timing) == 3 and all(t > 0.0 for t in timing)
    # the call changes no state: the run that asked continues bit for bit with one that never did
    plain = pa.Simulation(pa.make_params(**SIM))
    plain.run(9)
    assert np.array_equal(plain.core_genome.read_matrix(), state[0]) and np.array_equal(plain.pan_genome.read_matrix(), state[1])
    assert np.array_equal(plain.last_parents(), state[2])
    plain.close()


def test_a_sample_of_the_run(pa, sim_after_six):
    """a `subset` handle against the independent path on that sample's own matrices"""
    got, m, a = sim_after_six[5]
    want = ref.independent(pa, m, a, 20, "nj", _lists(8, 3, 2048, 2048, None))
    _assert_equal(got, want, SAMPLE.size, 2048, 20, "nj", 3, 2048)


@pytest.mark.parametrize("shards", [2, 3])
def test_multi_simulation_equals_the_unsharded_run(pa, sim_after_six, shards):
    """the sites of a replicate fall unevenly over the shards; one list leaves every shard but the first empty"""
    got, _, listed, _, _, _, _ = sim_after_six
    multi = pa.MultiSimulation(pa.make_params(**SIM), shards, devices=[0] * shards)
    multi.run(6)
    for method in ref.METHODS:
        mine, theirs = multi.bootstrap_support(method=method, replicates=3, seed=5), got[method]
        for name in ("left", "right", "support", "shared"):
            assert np.array_equal(getattr(mine, name), getattr(theirs, name)), (method, name)
        assert mine.as_dict().keys() == theirs.as_dict().keys() and all(getattr(mine, k) == getattr(theirs, k) for k in ref.INT_FIELDS)
    mine = multi.bootstrap_support(method="upgma", replicates=2, sites=ONE_SHARD)
    assert np.array_equal(mine.support, listed.support) and np.array_equal(mine.shared, listed.shared) and np.array_equal(mine.left, listed.left)
    assert all(t > 0.0 for t in multi.bootstrap_support_timing())
    with pytest.raises(pa.PansimError) as e:             # a site shard on its own
        multi.shards[1].bootstrap_support()
    assert e.value.code == PS_ERR_INVALID and "ps_multi_bootstrap_support" in str(e.value)
    multi.close()
