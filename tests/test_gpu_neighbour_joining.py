"""The neighbour-joining tree on the device (ps_neighbour_joining and its ps_sim / ps_multi forms, docs/NEIGHBOUR_JOINING.md)
against the library's host form (ps_nj_from_counts) and the NumPy restatement of the rule (tests/neighbour_joining_ref.py) over
the numerators that the existing ps_pairwise_counts returns for the full i < j list -- a path that shares nothing with the new
kernels.  Every comparison is an equality; the lengths are compared bit for bit."""
import numpy as np
import pytest

import neighbour_joining_ref as ref

pytestmark = pytest.mark.gpu

PS_ERR_INVALID, PS_ERR_STATE = -1, -6
BASES = np.array([1, 2, 4, 8], np.uint8)
METRICS = (("core", ref.CORE), ("acc", ref.ACC))


def _onehot(rng, N, L):
    return BASES[rng.integers(0, 4, (N, L))]


def _handles(pa, core_matrix, acc_matrix, cg):
    N, L = core_matrix.shape
    core = pa.Population(N, L, 4, True, 0.0, 0, 0)
    core.load_matrix(core_matrix)
    acc = pa.Population(N, acc_matrix.shape[1], 2, False, 0.5, 0, cg)
    acc.load_matrix(acc_matrix)
    return core, acc


def _numerators(core, acc):
    """(r1, r2, h, I, U) of every pair i < j from the existing sampled-pair path"""
    r1, r2 = ref.all_pairs(core.size)
    (h,) = core.pairwise_counts(r1, r2)
    i, u = acc.pairwise_counts(r1, r2)
    return r1, r2, h, i, u


def _check(pa, core, acc, nums, cg, want=None):
    """both metrics: the device == the host form == the restatement (`want`: its two results, computed before) -> the device's"""
    out = []
    N, L = core.size, core.global_cols
    for k, (name, metric) in enumerate(METRICS):
        got = core.neighbour_joining(acc, metric=name)
        ref.assert_equal(got, want[k] if want else ref.tree(metric, *nums, N, L, cg))
        ref.assert_equal(pa.nj_from_counts(*nums, N, L, cg, metric=name), got.as_dict())
        assert got.pairs == N * (N - 1) // 2 and got.joins == N - 1
        out.append(got)
    return out


@pytest.mark.parametrize("N", [2, 3, 63, 64, 65, 257])
def test_wave_and_chunk_edges(pa, N):
    """L = 130, G = 40, cg = 3, random: the last join alone, one join before it, a first chunk of 64 columns less one / exactly /
    plus one, and several chunks of the scan's one trip (512 columns); every loop of the two join kernels takes one trip here --
    test_past_both_strides takes the second"""
    rng = np.random.default_rng(N)
    core, acc = _handles(pa, _onehot(rng, N, 130), (rng.random((N, 40)) < 0.3).astype(np.uint8), 3)
    _check(pa, core, acc, _numerators(core, acc), 3)
    core.close()
    acc.close()


def test_past_both_strides(pa):
    """N = 1100, L = 130, G = 40, cg = 3, random: the scan of a row takes up to three trips of 512 columns and starts them at
    every offset, the join workgroup's candidate loop and its update loop take a second trip of 1024 rows (until fewer are
    active), and rows retire all over the matrix.  The device against the library's host form, which runs the same rule in a
    plain loop (about 2.2e8 steps per metric) and is itself held to the restatement at the smaller sizes."""
    N = 1100
    rng = np.random.default_rng(1100)
    core, acc = _handles(pa, _onehot(rng, N, 130), (rng.random((N, 40)) < 0.3).astype(np.uint8), 3)
    nums = _numerators(core, acc)
    for name, _ in METRICS:
        got = core.neighbour_joining(acc, metric=name)
        ref.assert_equal(pa.nj_from_counts(*nums, N, 130, 3, metric=name), got.as_dict())
        assert got.joins == N - 1 and got.pairs == N * (N - 1) // 2
        sets = ref.below(got.left, got.right, N)
        assert sets[-1] == list(range(N))                # every row is joined once
        assert all(sets[int(a)][0] < sets[int(b)][0] for a, b in zip(got.left, got.right))      # left is the smaller id
    core.close()
    acc.close()


@pytest.fixture(scope="module")
def two_bands(pa):
    """N = 300 = 256 + 44, L = 320, G = 130: the matrices and, computed once, the restatement's two trees"""
    rng = np.random.default_rng(5)
    core, acc = _handles(pa, _onehot(rng, 300, 320), (rng.random((300, 130)) < 0.3).astype(np.uint8), 7)
    nums = _numerators(core, acc)
    want = [ref.tree(metric, *nums, 300, 320, 7) for _, metric in METRICS]
    yield core, acc, nums, want
    core.close()
    acc.close()


@pytest.mark.parametrize("band", [0, 256])
def test_two_bands(pa, two_bands, band):
    """band 256: the store kernels fill the matrix in two pieces"""
    core, acc, nums, want = two_bands
    core.set_tuning("core_davg_band", band)
    try:
        _check(pa, core, acc, nums, 7, want)
    finally:
        core.set_tuning("core_davg_band", 0)


def test_arbitrary_bytes(pa):
    """N = 70, L = 130 of arbitrary bytes: the generic count form, with odd h that the store halves downwards"""
    rng = np.random.default_rng(3)
    core, acc = _handles(pa, rng.integers(0, 256, (70, 130), dtype=np.uint8), (rng.random((70, 40)) < 0.2).astype(np.uint8), 3)
    nums = _numerators(core, acc)
    assert (nums[2] & 1).any()
    _check(pa, core, acc, nums, 3)
    core.close()
    acc.close()


def test_clonal_population_is_the_caterpillar(pa):
    """N = 100, every pair d = 0 and a = 0: every q is 0, so every join is decided by the ids alone -- row 0's node takes the
    rows in ascending order, and every length is 0"""
    N = 100
    core, acc = _handles(pa, np.full((N, 200), 4, np.uint8), np.tile((np.arange(50) % 3 == 0).astype(np.uint8), (N, 1)), 2)
    for got in _check(pa, core, acc, _numerators(core, acc), 2):
        assert list(got.left) == [0] + list(range(N, 2 * N - 2)) and list(got.right) == list(range(1, N))
        assert not got.len_left.view(np.uint64).any() and not got.len_right.view(np.uint64).any()      # +0.0, every one
        assert got.negative_branches == 0 and got.tree_length == 0.0
    core.close()
    acc.close()


def test_planted_infinite_sites_tree(pa):
    """N = 128 leaves of a random tree with integer branches 1 .. 9, every branch with as many private sites: the core metric is
    the tree's path metric, which neighbour joining recovers exactly -- every split with its length, no negative branch -- and on
    the recovered tree no site changes more than once"""
    N = 128
    rng = np.random.default_rng(77)
    planted = ref.random_tree(rng, N)
    sites = ref.infinite_sites(planted, N)
    L = sites.shape[1]
    assert L == int(planted[2].sum() + planted[3].sum())
    core, acc = _handles(pa, sites, (rng.random((N, 40)) < 0.3).astype(np.uint8), 3)
    nums = _numerators(core, acc)
    assert np.array_equal(nums[2], (2 * ref.path_lengths(planted, N)[nums[0], nums[1]]).astype(np.uint32))
    got = core.neighbour_joining(acc, metric="core")
    ref.assert_equal(got, ref.tree(ref.CORE, *nums, N, L, 3))
    assert ref.splits(got.left, got.right, got.len_left, got.len_right, N) == ref.splits(*planted, N)
    assert got.negative_branches == 0 and got.tree_length == float(L)
    assert np.array_equal(got.patristic(nums[0], nums[1]), ref.path_lengths(planted, N)[nums[0], nums[1]])
    pars = core.tree_parsimony(*got.merges())
    assert pars.homoplasic_sites == 0
    core.close()
    acc.close()


def test_timing(pa):
    rng = np.random.default_rng(8)
    core, acc = _handles(pa, _onehot(rng, 90, 200), (rng.random((90, 30)) < 0.4).astype(np.uint8), 5)
    with pytest.raises(pa.PansimError) as e:
        core.neighbour_joining_timing()
    assert e.value.code == PS_ERR_STATE and "no neighbour-joining tree" in str(e.value)
    for name, _ in METRICS:
        core.neighbour_joining(acc, metric=name)
        counts_ms, store_ms, joins_ms = core.neighbour_joining_timing()
        assert counts_ms > 0.0 and store_ms > 0.0 and joins_ms > 0.0
    core.close()
    acc.close()


def test_limits(pa):
    """refused before any device work: nothing has been computed on the handle afterwards"""
    rng = np.random.default_rng(6)
    core, acc = _handles(pa, _onehot(rng, 20, 64), (rng.random((20, 10)) < 0.5).astype(np.uint8), 2)
    wide = pa.Population(20, 65536, 2, False, 0.5, 0, 2)
    for name, _ in METRICS:
        with pytest.raises(pa.PansimError) as e:
            core.neighbour_joining(wide, metric=name)
        assert e.value.code == PS_ERR_INVALID and "65535 accessory genes" in str(e.value)
    none = pa.Population(20, 10, 2, False, 0.5, 0, 0)
    with pytest.raises(pa.PansimError) as e:
        core.neighbour_joining(none, metric="acc")
    assert e.value.code == PS_ERR_INVALID and "core_genes >= 1" in str(e.value)
    huge = pa.Population(20, 10, 2, False, 0.5, 0, 2**32 - 65535)
    with pytest.raises(pa.PansimError) as e:
        core.neighbour_joining(huge, metric="acc")
    assert e.value.code == PS_ERR_INVALID and "core_genes + 65535 < 2^32" in str(e.value)
    big_core, big_acc = pa.Population(16385, 8, 4, True, 0.0, 0, 0), pa.Population(16385, 4, 2, False, 0.5, 0, 2)
    for name, _ in METRICS:
        with pytest.raises(pa.PansimError) as e:
            big_core.neighbour_joining(big_acc, metric=name)
        assert e.value.code == PS_ERR_INVALID and "pop_size <= 16384" in str(e.value)
    for a, b in ((core, core), (acc, acc), (acc, core)):
        with pytest.raises(pa.PansimError) as e:
            a.neighbour_joining(b)
        assert e.value.code == PS_ERR_INVALID and "core handle first" in str(e.value)
    with pytest.raises(ValueError):
        core.neighbour_joining(acc, metric="joint")
    shard = pa.Population(20, 32, 4, True, 0.0, 0, 0, col_offset=32, global_cols=64)      # a site shard on its own
    with pytest.raises(pa.PansimError) as e:
        shard.neighbour_joining(acc)
    assert e.value.code == PS_ERR_INVALID and "ps_multi_neighbour_joining" in str(e.value)
    for p in (core, big_core, shard):
        with pytest.raises(pa.PansimError) as e:
            p.neighbour_joining_timing()
        assert e.value.code == PS_ERR_STATE
    assert core.neighbour_joining(none, metric="core").joins == 19      # (the core metric does not look at the core genes)
    for p in (core, acc, wide, none, huge, big_core, big_acc, shard):
        p.close()


SIM = dict(pop_size=200, core_size=2048, pan_genes=300, core_genes=20, HR_rate=0.5, HGT_rate=0.5, seed=11, n_gen=9, max_distances=100)
SAMPLE = np.random.default_rng(12).choice(200, 60, replace=False)


@pytest.fixture(scope="module")
def sim_after_six(pa):
    """the unsharded run after 6 generations: its trees, the restatement's over pairwise_counts on its handles (output rows),
    the trees of a sample of its rows with that sample's numerators, and its state after 3 more generations"""
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(6)
    got = [sim.neighbour_joining(metric=name) for name, _ in METRICS]     # no sync: ordered behind the run
    timing = sim.neighbour_joining_timing()
    nums = _numerators(sim.core_genome, sim.pan_genome)
    want = [ref.tree(metric, *nums, 200, 2048, 20) for _, metric in METRICS]
    sc, sa = sim.subset(SAMPLE)
    sample = [sc.neighbour_joining(sa, metric=name) for name, _ in METRICS], _numerators(sc, sa)
    sc.close()
    sa.close()
    sim.run(3)
    state = (sim.core_genome.read_matrix(), sim.pan_genome.read_matrix(), sim.last_parents())
    sim.close()
    return got, want, state, sample, timing


def test_row_order_in_a_simulation(pa, sim_after_six):
    got, want, state, _, timing = sim_after_six
    for g, w in zip(got, want):
        ref.assert_equal(g, w)
    assert len(timing) == 3 and all(t > 0.0 for t in timing)
    sets = ref.below(got[0].left, got[0].right, 200)
    assert all(sets[int(a)][0] < sets[int(b)][0] for a, b in zip(got[0].left, got[0].right))      # left is the smaller id
    # the call changes no state: the run that asked continues bit for bit with one that never did
    plain = pa.Simulation(pa.make_params(**SIM))
    plain.run(9)
    assert np.array_equal(plain.core_genome.read_matrix(), state[0]) and np.array_equal(plain.pan_genome.read_matrix(), state[1])
    assert np.array_equal(plain.last_parents(), state[2])
    plain.close()


def test_a_sample_of_the_run(pa, sim_after_six):
    """a `subset` handle: the tree of the host form on that sample's own pairs, and of the whole run's numerators at its rows"""
    _, _, _, (trees, nums), _ = sim_after_six
    n = SAMPLE.size
    for (name, metric), got in zip(METRICS, trees):
        ref.assert_equal(pa.nj_from_counts(*nums, n, 2048, 20, metric=name), got.as_dict())
        ref.assert_equal(got, ref.tree(metric, *nums, n, 2048, 20))


@pytest.mark.parametrize("shards", [2, 3])
def test_multi_simulation_equals_the_unsharded_run(pa, sim_after_six, shards):
    _, want, _, _, _ = sim_after_six
    multi = pa.MultiSimulation(pa.make_params(**SIM), shards, devices=[0] * shards)
    multi.run(6)
    for (name, _), w in zip(METRICS, want):
        ref.assert_equal(multi.neighbour_joining(metric=name), w)
    assert all(t > 0.0 for t in multi.neighbour_joining_timing())
    with pytest.raises(pa.PansimError) as e:             # a site shard on its own
        multi.shards[1].neighbour_joining()
    assert e.value.code == PS_ERR_INVALID and "ps_multi_neighbour_joining" in str(e.value)
    multi.close()
