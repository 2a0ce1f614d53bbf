"""Population::average_distance of the CORE matrix (population.rs:753-784 with the core branch of get_distance, :132-137):
d(i, j) = (h_ij / 2) / L with h the byte popcount of x ^ y over all sites, a left-to-right f64 fold over j != i, / (N - 1),
0.0 -> f64::MIN_POSITIVE.  Every form of DESIGN.md 4.4 against the oracle, bit for bit: the whole-matrix form (FP4 all-pairs
triangle + core_average_from_h_kernel), the banded form (FP4 rectangles + core_average_from_counts_kernel), the generic form,
row shards, a simulation's handle (output order), and ps_multi's site shards."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DBL_MIN = 2.2250738585072014e-308


def one_hot(rng, N, L):
    return (1 << rng.integers(0, 4, (N, L))).astype(np.uint8)


def core_pop(pa, m, cg=0):
    N, L = m.shape
    pop = pa.Population(N, L, 4, True, 0.0, 0, cg)
    pop.load_matrix(m)
    return pop


def check_rows(pop, want):
    N = want.size
    K = min(3, N)
    got = np.concatenate([pop.average_distance_rows(N * r // K, N * (r + 1) // K - N * r // K) for r in range(K)])
    assert np.array_equal(got, want)
    assert np.array_equal(pop.average_distance_rows(1, N - 1), want[1:])
    if N > 300:
        assert np.array_equal(pop.average_distance_rows(257, N - 300), want[257:N - 43])


@pytest.mark.parametrize("N,L", [(2, 9), (33, 129), (300, 5000), (1000, 2000), (1030, 700), (2100, 300)])
def test_core_average_distance_one_hot_every_form(pa, orc, N, L):
    rng = np.random.default_rng(N * 31 + L)
    m = one_hot(rng, N, L)
    if N > 6:
        m[5] = m[6]                                   # a zero term inside the fold
    want = orc.average_distance(m, True, 0)
    pop = core_pop(pa, m)
    # form 1: whole matrix; 2: banded (several bands of 256 rows where N > 512: bands that do not divide N); 0: the choice
    for form, band in ((1, 0), (2, 256), (2, 512), (2, 0), (0, 0)):
        pop.set_tuning("core_davg_form", form)
        pop.set_tuning("core_davg_band", band)
        assert np.array_equal(pop.average_distance(), want), (form, band)
        check_rows(pop, want)
    pop.set_tuning("core_davg_form", 3)               # the generic form on a one-hot matrix agrees too
    assert np.array_equal(pop.average_distance(), want)
    for first, count in ((N, 1), (0, N + 1), (N - 1, 2), (0, 0)):
        with pytest.raises(pa.PansimError) as e:
            pop.average_distance_rows(first, count)
        assert e.value.code == -1
    pop.close()


def test_core_average_distance_clonal_and_tiny(pa, orc):
    m = np.tile(one_hot(np.random.default_rng(3), 1, 777), (600, 1))
    pop = core_pop(pa, m)
    for form in (1, 2, 3):
        pop.set_tuning("core_davg_form", form)
        pop.set_tuning("core_davg_band", 256)
        got = pop.average_distance()
        assert (got == DBL_MIN).all(), form
        assert np.array_equal(got, orc.average_distance(m, True, 0))
    pop.close()
    lone = core_pop(pa, one_hot(np.random.default_rng(4), 1, 50))
    with pytest.raises(pa.PansimError) as e:
        lone.average_distance()
    assert e.value.code == -1
    with pytest.raises(pa.PansimError) as e:
        lone.average_distance_rows(0, 1)
    assert e.value.code == -1
    lone.close()


@pytest.mark.parametrize("N,L,hi", [(300, 5000, 16), (1030, 700, 16), (33, 129, 256), (130, 70, 256), (600, 90, 256)])
def test_core_average_distance_other_bytes(pa, orc, N, L, hi):
    # nibbles 0..15 (xor + popcount all-pairs tiles) and bytes up to 255 (the generic band kernel): odd h before the / 2
    rng = np.random.default_rng(N + L + hi)
    m = rng.integers(0, hi, (N, L)).astype(np.uint8)
    m[3] = m[4]
    want = orc.average_distance(m, True, 0)
    pop = core_pop(pa, m)
    for form, band in ((0, 0), (3, 0), (1, 0), (2, 256)):
        pop.set_tuning("core_davg_form", form)
        pop.set_tuning("core_davg_band", band)
        assert np.array_equal(pop.average_distance(), want), (form, band)
        check_rows(pop, want)
    pop.close()


def test_core_average_distance_chunk_ranges(pa, orc):
    # 70 000 sites = 547 chunks of 128: both matrix-core forms split them into ranges whose slices are summed afterwards
    rng = np.random.default_rng(70000)
    m = one_hot(rng, 300, 70000)
    m[10] = m[200]
    want = orc.average_distance(m, True, 0)
    pop = core_pop(pa, m)
    for form in (1, 2, 0):
        pop.set_tuning("core_davg_form", form)
        assert np.array_equal(pop.average_distance(), want), form
        check_rows(pop, want)
    pop.close()


def test_core_average_distance_of_a_simulation(pa, orc):
    # a simulation's handle: rows in output (draw) order, not in the internal ascending-parent order, and so is every fold
    kw = dict(pop_size=600, core_size=2000, pan_genes=300, core_genes=50, HR_rate=0.2)
    sim = pa.Simulation(pa.make_params(seed=7, n_gen=3, max_distances=100, device=0, **kw))
    sim.run(3)
    sim.sync()
    parents = sim.last_parents()
    assert not np.array_equal(parents, np.sort(parents))          # the two row orders differ
    pop = sim.core_genome
    m = pop.read_matrix()
    want = orc.average_distance(m, True, 50)
    for form, band in ((0, 0), (1, 0), (2, 256), (3, 0)):
        pop.set_tuning("core_davg_form", form)
        pop.set_tuning("core_davg_band", band)
        assert np.array_equal(pop.average_distance(), want), (form, band)
        check_rows(pop, want)
    # after ps_load_matrix the loaded order is the output order
    m2 = m[np.random.default_rng(1).permutation(600)]
    pop.load_matrix(m2)
    want2 = orc.average_distance(m2, True, 50)
    for form in (0, 2, 3):
        pop.set_tuning("core_davg_form", form)
        assert np.array_equal(pop.average_distance(), want2), form
    sim.close()


@pytest.mark.parametrize("n_shards", [2, 3])
def test_multi_average_distance(pa, orc, n_shards):
    kw = dict(pop_size=600, core_size=3001, pan_genes=400, core_genes=100, HR_rate=0.3)
    params = dict(seed=4, n_gen=3, max_distances=100, **kw)
    multi = pa.MultiSimulation(pa.make_params(**params), n_shards, devices=[0] * n_shards)
    multi.run(3)
    multi.sync()
    m = np.concatenate([s.core_genome.read_matrix() for s in multi.shards], axis=1)
    want = orc.average_distance(m, True, 100)
    assert np.array_equal(multi.average_distance(True), want)
    multi.shards[0].core_genome.set_tuning("core_davg_band", 256)   # three bands
    assert np.array_equal(multi.average_distance(True), want)
    with pytest.raises(pa.PansimError) as e:                        # one shard cannot finish the sum
        multi.shards[1].core_genome.average_distance()
    assert e.value.code == -1
    with pytest.raises(pa.PansimError) as e:
        multi.shards[0].core_genome.average_distance_rows(0, 10)
    assert e.value.code == -1
    sim = pa.Simulation(pa.make_params(device=0, **params))
    sim.run(3)
    sim.sync()
    assert np.array_equal(sim.core_genome.average_distance(), want)
    assert np.array_equal(multi.average_distance(False), sim.pan_genome.average_distance())
    sim.close()
    multi.close()


def test_core_average_distance_wide_population(pa):
    # N = 65536 from 7 haplotypes: the banded form at full width (the N x N counts exceed the whole-matrix cap).  Rows of one
    # haplotype share their terms (the skipped self term is +0.0), so each haplotype's value is one sequential fold of N terms.
    N, L, H = 65536, 3000, 7
    rng = np.random.default_rng(65536)
    hap = one_hot(rng, H, L)
    a = rng.integers(0, H, N)
    m = hap[a]
    mism = (hap[:, None, :] != hap[None, :, :]).sum(axis=2)          # h / 2 of one-hot rows
    term = mism.astype(np.float64) / float(L)
    want_h = np.array([np.add.accumulate(term[u][a])[-1] / (N - 1) for u in range(H)])
    want_h[want_h == 0.0] = DBL_MIN
    want = want_h[a]
    pop = core_pop(pa, m)
    assert np.array_equal(pop.average_distance(), want)
    assert np.array_equal(pop.average_distance_rows(40000, 300), want[40000:40300])
    pop.close()
