"""Core allele profiles on the device (ps_allele_profiles and its ps_sim / ps_multi forms, docs/ALLELE_PROFILES.md) against the
plain restatement (tests/allele_profiles_ref.py) over the matrices that were loaded or that read_matrix() returns -- a path that
shares nothing with the new code.  Every comparison is an equality of integers; the one double is compared bit for bit."""
import numpy as np
import pytest

import allele_profiles_ref as ref

pytestmark = pytest.mark.gpu

PS_ERR_INVALID, PS_ERR_STATE = -1, -6
BASES = np.array([1, 2, 4, 8], np.uint8)


def _onehot(rng, N, L):
    return BASES[rng.integers(0, 4, (N, L))]


def related(rng, N, L, founders=5, moves=3):
    """`founders` unrelated individuals; every other one copies an earlier one and moves away by a few core sites (as related()
    of tests/test_gpu_gene_site_ld.py): alleles are shared, sequence types and complexes are not trivial"""
    core = _onehot(rng, N, L)
    for k in range(min(founders, N), N):
        core[k] = core[rng.integers(k)]
        sites = rng.choice(L, rng.integers(0, moves), replace=False)
        core[k, sites] = BASES[(np.log2(core[k, sites]).astype(int) + 1 + rng.integers(0, 3, sites.size)) % 4]
    return np.ascontiguousarray(core[rng.permutation(N)])


def _handle(pa, m):
    core = pa.Population(m.shape[0], m.shape[1], 4, True, 0.0, 0, 0)
    core.load_matrix(m)
    return core


def _same(a, b):
    """two results field for field (but the informational `rounds`: the label rounds depend on the order of the atomics)"""
    a, b = a.as_dict(), b.as_dict()
    return all(np.array_equal(a[k], b[k]) for k in a if k != "rounds")


def _check(core, m, n_loci, **kw):
    """the device against the restatement of the matrix -> the result"""
    got = core.allele_profiles(n_loci, **kw)
    rkw = {k: v for k, v in kw.items() if k in ("bounds", "dist_bins", "complex_max")}
    ref.assert_equal(got, ref.from_matrix(m, n_loci, **rkw))
    timing = core.allele_profiles_timing()
    assert len(timing) == 5 and all(ms >= 0.0 for ms in timing)
    assert int(got.hist.sum()) == got.pairs and got.sum_d == sum(got.pairs - int(s) for s in got.locus_same_pairs)
    sizes = np.bincount(got.st)
    assert got.identical_pairs == int((sizes * (sizes - 1) // 2).sum())
    assert (got.rounds == 0) == (got.complex_max == 0)
    return got


@pytest.mark.parametrize("N,L,n_loci", [(2, 8, 3), (7, 203, 203), (64, 130, 7), (65, 130, 64), (300, 1001, 70), (1030, 300, 33), (2049, 70, 70)])
def test_loaded_matrices(pa, N, L, n_loci):
    """N below, at and above the 4-, 64-, 128- and 1024-cell boundaries of the kernels and of a 64 x 64 tile of the pairs; loci
    of one site, L no multiple of n_loci, n_loci odd, below and above the 32 loci of a staged chunk"""
    rng = np.random.default_rng(N)
    m = related(rng, N, L)
    core = _handle(pa, m)
    got = _check(core, m, n_loci)
    if N >= 64:
        assert 1 < got.sequence_types < N and got.identical_pairs > 0
    one = _check(core, m, n_loci, complex_max=1, dist_bins=5)
    assert one.complexes <= got.complexes and one.edges >= got.edges
    _check(core, m, n_loci, complex_max=n_loci, dist_bins=1, want_profiles=False)
    core.close()


def test_explicit_bounds_leave_sites_uncovered(pa):
    rng = np.random.default_rng(3)
    N, L = 130, 400
    m = related(rng, N, L, moves=6)
    bounds = [5, 6, 40, 41, 200, 333, 390]                     # head [0, 5) and tail [390, 400) outside; loci of one site
    core = _handle(pa, m)
    got = _check(core, m, 6, bounds=bounds, complex_max=2)
    assert got.sites_covered == 385 < L == got.core_sites
    planted = m.copy()
    planted[3, 2], planted[9, 395] = planted[3, 2] ^ 3, planted[9, 395] ^ 12          # changes outside every locus
    core.load_matrix(planted)
    again = core.allele_profiles(6, bounds=bounds, complex_max=2)
    assert _same(got, again)
    planted[3, 5] ^= 3                                          # ... and one inside locus 0
    core.load_matrix(planted)
    ref.assert_equal(core.allele_profiles(6, bounds=bounds, complex_max=2), ref.from_matrix(planted, 6, bounds=bounds, complex_max=2))
    for bad in ([5, 6, 40, 40, 200, 333, 390], [5, 6, 40, 41, 200, 333, 401], [6, 5, 40, 41, 200, 333, 390]):
        with pytest.raises(pa.PansimError) as e:
            core.allele_profiles(6, bounds=bad)
        assert e.value.code == PS_ERR_INVALID and "bounds" in str(e.value)
    core.close()


def test_bytes_that_are_no_base_are_other_values(pa):
    rng = np.random.default_rng(4)
    m = related(rng, 70, 96)
    m[:, 10] = rng.choice(np.array([0, 3, 255, 1], np.uint8), 70)
    m[:35, 50], m[35:, 50] = 0, 255
    core = _handle(pa, m)
    got = _check(core, m, 96)                                   # one site per locus: the alleles are the bytes
    assert got.locus_alleles[10] == 4 and got.locus_alleles[50] == 2
    _check(core, m, 5, complex_max=1)
    core.close()


def test_one_locus_over_everything(pa):
    rng = np.random.default_rng(8)
    m = related(rng, 200, 333, founders=3, moves=2)
    core = _handle(pa, m)
    got = _check(core, m, 1)
    _, inverse = np.unique(m, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    assert np.array_equal(got.st[:, None] == got.st[None, :], inverse[:, None] == inverse[None, :])
    assert got.sequence_types == got.locus_alleles[0] == inverse.max() + 1 and np.array_equal(got.profiles[:, 0], ref.renumber(m))
    core.close()


def test_three_bands_equal_one(pa):
    rng = np.random.default_rng(9)
    m = related(rng, 150, 700, founders=9, moves=8)
    core = _handle(pa, m)
    whole = _check(core, m, 70, complex_max=3)
    core.set_tuning("mlst_band", 30)                            # 30 + 30 + 10
    banded = _check(core, m, 70, complex_max=3)
    core.set_tuning("mlst_band", 0)
    assert _same(whole, banded)
    core.close()


def test_the_seed_changes_nothing(pa):
    rng = np.random.default_rng(10)
    m = related(rng, 260, 300)
    core = _handle(pa, m)
    a = _check(core, m, 40, complex_max=1)
    assert _same(a, _check(core, m, 40, complex_max=1, key_seed=0x9E3779B97F4A7C15))
    assert _same(a, _check(core, m, 40, complex_max=1, key_bits=20))
    core.close()


def test_a_collision_of_one_bit_keys_is_caught(pa):
    rng = np.random.default_rng(11)
    m = related(rng, 66, 64)
    m[0, 8:10], m[65, 8:10] = (1, 2), (2, 1)                    # with every key 1 the two runs of locus 4 add up alike
    m[1:65, 8:10] = 4
    core = _handle(pa, m)
    with pytest.raises(pa.PansimError) as e:
        core.allele_profiles(32, key_bits=1)
    assert e.value.code == PS_ERR_STATE and "key_seed" in str(e.value)
    count = int(str(e.value).split("(locus, individual)")[0].split()[-1])
    assert count >= 1
    got = _check(core, m, 32)
    assert got.locus_alleles[4] == 3
    core.close()


SIM = dict(core_size=1001, pan_genes=400, core_genes=20, HR_rate=0.5, HGT_rate=0.5, prop_positive=0.5, seed=11, n_gen=25, max_distances=100)
KW = dict(n_loci=7, complex_max=1)


@pytest.fixture(scope="module")
def sim_300_after_twenty(pa):
    sim = pa.Simulation(pa.make_params(pop_size=300, **SIM))
    sim.run(20)
    got = sim.allele_profiles(**KW)             # no sync: ordered behind the run, a two-generation sweep launch included
    timing = sim.allele_profiles_timing()
    m = sim.core_genome.read_matrix()
    fine = sim.allele_profiles(n_loci=143)
    sim.run(5)
    state = (sim.core_genome.read_matrix(), sim.pan_genome.read_matrix(), sim.last_parents())
    sim.close()
    return got, fine, m, timing, state


def test_a_simulation_after_twenty_generations(pa, sim_300_after_twenty):
    got, fine, m, timing, state = sim_300_after_twenty
    ref.assert_equal(got, ref.from_matrix(m, **KW))
    ref.assert_equal(fine, ref.from_matrix(m, 143))
    assert len(timing) == 5 and all(ms >= 0.0 for ms in timing)
    assert fine.sum_d > got.sum_d > 0 and got.alleles_total > got.loci
    # the call changed no state: the run that asked continues bit for bit with one that never did
    plain = pa.Simulation(pa.make_params(pop_size=300, **SIM))
    plain.run(25)
    assert np.array_equal(plain.core_genome.read_matrix(), state[0]) and np.array_equal(plain.pan_genome.read_matrix(), state[1])
    assert np.array_equal(plain.last_parents(), state[2])
    plain.close()


@pytest.mark.parametrize("shards", [2, 3])
def test_shards_equal_the_unsharded_run(pa, sim_300_after_twenty, shards):
    """L = 1001 and seven loci of 143 sites: the shard boundaries (500; 333 and 667) fall inside loci"""
    want, fine, m, _, _ = sim_300_after_twenty
    multi = pa.MultiSimulation(pa.make_params(pop_size=300, **SIM), shards, devices=[0] * shards)
    multi.run(20)
    for got, w in ((multi.allele_profiles(**KW), want), (multi.allele_profiles(n_loci=143), fine)):
        assert _same(got, w)
    assert np.float64(got.mean_distance).tobytes() == np.float64(fine.mean_distance).tobytes()
    assert all(ms >= 0.0 for ms in multi.allele_profiles_timing())
    ref.assert_equal(multi.allele_profiles(4, bounds=[3, 400, 600, 700, 990], complex_max=2),
                     ref.from_matrix(m, 4, bounds=[3, 400, 600, 700, 990], complex_max=2))
    with pytest.raises(pa.PansimError) as e:             # a site shard on its own
        multi.shards[1].core_genome.allele_profiles(3)
    assert e.value.code == PS_ERR_INVALID and "ps_multi_allele_profiles" in str(e.value)
    multi.close()


def test_limits_and_handles(pa):
    rng = np.random.default_rng(6)
    core = _handle(pa, _onehot(rng, 20, 64))
    with pytest.raises(pa.PansimError) as e:
        core.allele_profiles_timing()
    assert e.value.code == PS_ERR_STATE and "no allele profiles" in str(e.value)
    for kw, word in ((dict(n_loci=0), "n_loci"), (dict(n_loci=65), "n_loci"), (dict(n_loci=4, dist_bins=0), "dist_bins"),
                     (dict(n_loci=4, dist_bins=16385), "dist_bins"), (dict(n_loci=4, complex_max=5), "complex_max"),
                     (dict(n_loci=4, key_bits=0), "key_bits"), (dict(n_loci=4, key_bits=65), "key_bits")):
        with pytest.raises(pa.PansimError) as e:
            core.allele_profiles(**kw)
        assert e.value.code == PS_ERR_INVALID and word in str(e.value), kw
    acc = pa.Population(20, 10, 2, False, 0.5, 0, 0)
    with pytest.raises(pa.PansimError) as e:
        acc.allele_profiles(2)
    assert e.value.code == PS_ERR_INVALID and "core handle" in str(e.value)
    assert core.allele_profiles(64).loci == 64
    core.close()
    acc.close()
