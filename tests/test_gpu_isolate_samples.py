"""Isolate samples on the device (ps_population_pool / ps_population_subset / ps_sim_subset / ps_multi_subset,
docs/ISOLATE_SAMPLES.md): the gathered matrices against numpy indexing of the matrices that were loaded or that read_matrix()
returns, the read-outs of a sample against their existing restatements on m[rows], pools against numpy.vstack, every refusal, runs
that are sampled without a sync and continue bit for bit, shards, and the use case end to end.  Every comparison is an equality
of integers or bytes (tree_compare's doubles as tests/tree_compare_ref.py compares them)."""
import ctypes as C

import numpy as np
import pytest

import allele_profiles_ref
import core_diversity_ref
import distance_histogram_ref
import group_differentiation_ref
import tree_compare_ref
import upgma_tree_ref

pytestmark = pytest.mark.gpu

PS_ERR_INVALID, PS_ERR_STATE = -1, -6
BASES = np.array([1, 2, 4, 8], np.uint8)
POPS = [2, 7, 64, 65, 300, 1030, 2049]


def _onehot(rng, N, L):
    return BASES[rng.integers(0, 4, (N, L))]


def related(rng, N, L, founders=5, moves=3):
    """as related() of tests/test_gpu_allele_profiles.py: founders, copies that move away by a few sites, shuffled"""
    core = _onehot(rng, N, L)
    for k in range(min(founders, N), N):
        core[k] = core[rng.integers(k)]
        sites = rng.choice(L, rng.integers(0, moves), replace=False)
        core[k, sites] = BASES[(np.log2(core[k, sites]).astype(int) + 1 + rng.integers(0, 3, sites.size)) % 4]
    return np.ascontiguousarray(core[rng.permutation(N)])


def _core(pa, m, cg=0):
    h = pa.Population(m.shape[0], m.shape[1], 4, True, 0.0, 0, cg)
    h.load_matrix(m)
    return h


def _acc(pa, a, cg=0):
    h = pa.Population(a.shape[0], a.shape[1], 2, False, 0.5, 0, cg)
    h.load_matrix(a)
    return h


def _row_lists(rng, N):
    """one row, all rows reversed, random lists with repeats of length 3, 64, 129 and N + 5, and None"""
    yield [int(rng.integers(N))]
    yield np.arange(N)[::-1]
    for n in (3, 64, 129, N + 5):
        yield rng.integers(0, N, n)
    yield None


def _take(m, rows):
    return m if rows is None else m[np.asarray(rows, np.int64)]


def _check_subset(src, m, rows):
    s = src.subset(rows)
    want = _take(m, rows)
    assert s.size == want.shape[0] and s.ncols == m.shape[1] and s.core == src.core and s.core_genes == src.core_genes
    assert np.array_equal(s.read_matrix(), want)
    assert s.subset_timing() >= 0.0
    s.close()


# -- 1. loaded matrices ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 130, 1001])
@pytest.mark.parametrize("N", POPS)
def test_core_subsets_of_loaded_matrices(pa, N, L):
    """source rows and output rows below, at and above the 4-, 16-, 64-, 128- and 1024-byte boundaries; the list of one row
    takes the direct form (48 n < pitch), the list of 3 from N = 300 on, the others the LDS form; a list of 70 goes through both"""
    rng = np.random.default_rng(100 * N + L)
    m = _onehot(rng, N, L)
    src = _core(pa, m)
    for rows in _row_lists(rng, N):
        _check_subset(src, m, rows)
    rows = rng.integers(0, N, 70)
    for form in (1, 2, 0):
        src.set_tuning("gather_form", form)
        _check_subset(src, m, rows)
    assert np.array_equal(src.read_matrix(), m)                 # the source is read, not written
    src.close()


@pytest.mark.parametrize("G", [1, 64, 65, 200])
@pytest.mark.parametrize("N", POPS)
def test_accessory_subsets_of_loaded_matrices(pa, N, G):
    rng = np.random.default_rng(100 * N + G)
    a = (rng.random((N, G)) < 0.4).astype(np.uint8)
    src = _acc(pa, a, cg=1)
    for rows in _row_lists(rng, N):
        _check_subset(src, a, rows)
    assert np.array_equal(src.read_matrix(), a)
    src.close()


@pytest.mark.parametrize("high", [16, 256])
def test_the_safety_flags_travel(pa, orc, high):
    """bytes outside 1 / 2 / 4 / 8 (and, with high = 256, above 15): the pair counts of the sample take the kernels the flags
    allow, and equal the host count of m[rows]"""
    rng = np.random.default_rng(high)
    N, L, n = 90, 257, 37
    m = rng.integers(0, high, (N, L)).astype(np.uint8)
    src = _core(pa, m)
    rows = rng.integers(0, N, n)
    s = src.subset(rows)
    r1, r2 = np.triu_indices(n, 1)
    (got,) = s.pairwise_counts(r1, r2)
    assert np.array_equal(got, orc.pairwise_hamming_counts(m[rows], 0, L, r1, r2))
    # ... and a pool of it with a one-hot part is as unsafe as its worst part
    clean = _core(pa, _onehot(rng, 5, L))
    both = pa.pool([clean, s])
    r1, r2 = np.triu_indices(n + 5, 1)
    (got,) = both.pairwise_counts(r1, r2)
    assert np.array_equal(got, orc.pairwise_hamming_counts(both.read_matrix(), 0, L, r1, r2))
    for h in (both, clean, s, src):
        h.close()


# -- 2. the read-outs see a clean handle -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [61, 131])
def test_readouts_of_a_sample_equal_their_restatements(pa, n):
    """sample sizes that are no multiple of 4: a pad byte or a pad bit that is not zero would show in the read-outs that load
    whole dwords"""
    rng = np.random.default_rng(n)
    N, L, G, cg = 300, 1001, 70, 5
    m = related(rng, N, L)
    a = (rng.random((N, G)) < 0.4).astype(np.uint8)
    a[:, :cg] = 1
    core, acc = _core(pa, m, cg), _acc(pa, a, cg)
    rows = rng.integers(0, N, n)
    sc, sa = core.subset(rows), acc.subset(rows)
    mr, ar = m[rows], a[rows]
    assert core_diversity_ref.same(sc.core_diversity(spectrum=True), core_diversity_ref.of_matrix(mr)) is None
    allele_profiles_ref.assert_equal(sc.allele_profiles(7, complex_max=1), allele_profiles_ref.from_matrix(mr, 7, complex_max=1))
    # the numerators of every pair from handles that were LOADED with m[rows], as the tests of these read-outs take them
    r1, r2 = distance_histogram_ref.all_pairs(n)
    lc, la = _core(pa, mr, cg), _acc(pa, ar, cg)
    (h,), (i, u) = lc.pairwise_counts(r1, r2), la.pairwise_counts(r1, r2)
    lc.close()
    la.close()
    distance_histogram_ref.assert_equal(sc.distance_histogram(sa, 16, 8, core_span=L), distance_histogram_ref.histogram(h, i, u, L, cg, 16, 8, L),
                                        pop_size=n)
    for name, metric in (("core", upgma_tree_ref.CORE), ("acc", upgma_tree_ref.ACC)):
        upgma_tree_ref.assert_equal(sc.upgma_tree(sa, metric=name), upgma_tree_ref.tree(metric, r1, r2, h, i, u, n, L, cg), n)
    for x in (sc, sa, core, acc):
        x.close()


# -- 3. pools ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [(3, 5, 1), (64, 1, 63), (130, 129)])
def test_pools_equal_vstack(pa, sizes):
    """parts that begin at offsets that are no multiple of 4 or 16; the same handle twice; a part with all its rows"""
    rng = np.random.default_rng(sum(sizes))
    L, G = 203, 70
    mats = [_onehot(rng, 70, L), _onehot(rng, sizes[1], L)]
    accs = [(rng.random((m.shape[0], G)) < 0.5).astype(np.uint8) for m in mats]
    for make, ms in ((_core, mats), (_acc, accs)):
        hs = [make(pa, m) for m in ms]
        parts = [hs[0], hs[1]] + [hs[0]] * (len(sizes) - 2)                 # (the third part is the first handle again)
        which = [0, 1] + [0] * (len(sizes) - 2)
        rows = [rng.integers(0, 70, sizes[0]), None] + [rng.integers(0, 70, k) for k in sizes[2:]]
        want = np.vstack([_take(ms[w], r) for w, r in zip(which, rows)])
        pooled = pa.pool(parts, rows)
        assert pooled.size == sum(sizes) == want.shape[0] and np.array_equal(pooled.read_matrix(), want)
        assert pooled.subset_timing() >= 0.0
        again = pa.pool([pooled, pooled])                                   # all rows of every part
        assert np.array_equal(again.read_matrix(), np.vstack([want, want]))
        for k, h in enumerate(hs):
            assert np.array_equal(h.read_matrix(), ms[k])
        for h in [again, pooled] + hs:
            h.close()


def test_refusals_name_their_field(pa):
    rng = np.random.default_rng(2)
    core = _core(pa, _onehot(rng, 10, 40))
    acc = _acc(pa, (rng.random((10, 40)) < 0.5).astype(np.uint8))
    lib = pa.load()

    def refused(word, fn, *args):
        with pytest.raises(pa.PansimError) as e:
            fn(*args)
        assert e.value.code == PS_ERR_INVALID and word in str(e.value), (word, str(e.value))

    refused("rows[0][2] = 10", core.subset, [0, 9, 10])
    refused("rows[1][0] = 77", pa.pool, [core, core], [None, [77]])
    refused("n_rows", core.subset, [])
    refused("n_rows", pa.pool, [core, core], [[], []])
    refused("all core or all accessory", pa.pool, [core, acc])
    other = pa.Population(4, 41, 4, True, 0.0, 0, 0)
    refused("ncols", pa.pool, [core, other])
    other.close()
    other = pa.Population(4, 40, 4, True, 0.0, 0, 3)
    refused("core_genes", pa.pool, [core, other])
    other.close()
    shards = [pa.Population(4, 40, 4, True, 0.0, 0, 0, col_offset=off, global_cols=gc) for off, gc in ((0, 100), (40, 100), (0, 120))]
    refused("col_offset", pa.pool, [shards[0], shards[1]])
    refused("global_cols", pa.pool, [shards[0], shards[2]])
    for s in shards:
        s.close()
    if lib.ps_device_count() > 1:
        far = pa.Population(4, 40, 4, True, 0.0, 0, 0, device=1)
        refused("device", pa.pool, [core, far])
        far.close()
    # beyond what ps_population_create accepts: the sum is refused before a list is read
    parts = (C.c_void_p * 2)(core._h.value, core._h.value)
    few = np.zeros(4, np.uint32)
    lists = (C.c_void_p * 2)(few.ctypes.data, few.ctypes.data)
    out = C.c_void_p(1)
    assert lib.ps_population_pool(parts, lists, np.array([0xFFFFFFFF, 0xFFFFFFFF], np.uint64).ctypes.data, 2, C.byref(out)) == PS_ERR_INVALID
    assert "sum of n_rows" in lib.ps_last_error().decode() and not out.value
    assert lib.ps_population_pool(parts, lists, np.array([1 << 32, 1], np.uint64).ctypes.data, 2, C.byref(out)) == PS_ERR_INVALID
    assert "n_rows[0]" in lib.ps_last_error().decode()
    # all rows are pop_size rows
    assert lib.ps_population_subset(core._h, None, 9, C.byref(out)) == PS_ERR_INVALID and "n_rows[0] = 9" in lib.ps_last_error().decode()
    with pytest.raises(pa.PansimError) as e:
        core.subset_timing()
    assert e.value.code == PS_ERR_STATE
    core.close()
    acc.close()


# -- 4. runs -------------------------------------------------------------------------------------------------------------------

RUN = dict(pop_size=70, core_size=300, pan_genes=128, core_genes=20, HR_rate=0.5, HGT_rate=0.5, seed=5, n_gen=20, max_distances=100)


@pytest.mark.parametrize("generations", [1, 2, 5])
def test_a_run_is_sampled_without_a_sync_and_continues_bit_for_bit(pa, generations):
    """with the two-generation sweep an odd count ends on a one-generation launch"""
    rng = np.random.default_rng(generations)
    rows = rng.integers(0, 70, 33)
    sim = pa.Simulation(pa.make_params(**RUN))
    sim.run(generations)
    core, acc = sim.subset(rows)                     # no sync: ordered behind the run on the handles' streams
    whole = sim.subset()
    cm, am = sim.core_genome.read_matrix(), sim.pan_genome.read_matrix()
    assert core.size == acc.size == 33 and core.ncols == 300 and acc.ncols == am.shape[1]
    assert np.array_equal(core.read_matrix(), cm[rows]) and np.array_equal(acc.read_matrix(), am[rows])
    assert np.array_equal(whole[0].read_matrix(), cm) and np.array_equal(whole[1].read_matrix(), am)
    sim.run(4)
    assert np.array_equal(core.read_matrix(), cm[rows]) and np.array_equal(acc.read_matrix(), am[rows])
    twin = pa.Simulation(pa.make_params(**RUN))
    twin.run(generations)
    twin.run(4)
    assert np.array_equal(sim.core_genome.read_matrix(), twin.core_genome.read_matrix())
    assert np.array_equal(sim.pan_genome.read_matrix(), twin.pan_genome.read_matrix())
    for x, y in zip(sim.final_distances(), twin.final_distances()):
        assert x.tobytes() == y.tobytes()
    twin.close()
    sim.close()                                       # (the samples outlive their source)
    assert np.array_equal(core.read_matrix(), cm[rows])
    for h in (core, acc) + whole:
        h.close()


# -- 5. shards -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def run_of_five(pa):
    rows = np.random.default_rng(9).integers(0, 70, 41)
    sim = pa.Simulation(pa.make_params(**RUN))
    sim.run(5)
    core, acc = sim.subset(rows)
    out = rows, core.read_matrix(), acc.read_matrix()
    for h in (core, acc):
        h.close()
    sim.close()
    return out


@pytest.mark.parametrize("shards", [2, 3])
def test_shards_equal_the_unsharded_run(pa, run_of_five, shards):
    rows, want_core, want_acc = run_of_five
    multi = pa.MultiSimulation(pa.make_params(**RUN), shards, devices=[0] * shards)
    multi.run(5)
    core, acc = multi.subset(rows)
    assert core.ncols == core.global_cols == 300 and core.size == 41
    assert np.array_equal(core.read_matrix(), want_core) and np.array_equal(acc.read_matrix(), want_acc)
    assert core_diversity_ref.same(core.core_diversity(spectrum=True), core_diversity_ref.of_matrix(want_core)) is None      # a whole handle
    assert core.subset_timing() >= 0.0
    multi.run(1)
    multi.close()
    assert np.array_equal(core.read_matrix(), want_core)
    core.close()
    acc.close()


# -- 6. the use case, end to end -------------------------------------------------------------------------------------------------

def test_serial_samples_pooled_and_the_true_tree_of_a_sample(pa):
    rng = np.random.default_rng(6)
    sim = pa.Simulation(pa.make_params(**RUN))
    sim.record_ancestry(16)
    sim.run(4)
    rows_a = rng.choice(70, 20, replace=False)
    ca, aa = sim.subset(rows_a)
    ma, xa = sim.core_genome.read_matrix()[rows_a], sim.pan_genome.read_matrix()[rows_a]
    sim.run(5)
    rows_b = rng.choice(70, 25, replace=False)
    cb, ab = sim.subset(rows_b)
    mb, xb = sim.core_genome.read_matrix()[rows_b], sim.pan_genome.read_matrix()[rows_b]
    # temporal F_ST: the time point as the label
    core, acc = pa.pool([ca, cb]), pa.pool([aa, ab])
    labels = [4] * 20 + [9] * 25
    got = core.group_differentiation(labels, acc, per_site=True, counts=True)
    group_differentiation_ref.assert_equal(got, group_differentiation_ref.differentiation(np.vstack([ma, mb]), labels, np.vstack([xa, xb])))
    # the UPGMA tree of the sample against the TRUE genealogy of the sample
    g = sim.genealogy()
    sample_g = g.restrict(rows_b)
    r1, r2 = np.triu_indices(25, 1)
    assert np.array_equal(sample_g.pairs(r1, r2), g.pairs(rows_b[r1], rows_b[r2]))
    u = cb.upgma_tree(ab)
    got = cb.tree_compare(sample_g, u)
    tree_compare_ref.assert_equal(got, tree_compare_ref.compare(25, sample_g.merges(), (*u.merges(), u.levels())))
    for h in (core, acc, ca, aa, cb, ab):
        h.close()
    sim.close()
