"""Gene-site association on the device (ps_gene_site_ld and its ps_sim / ps_multi forms, docs/GENE_SITE_ASSOCIATION.md) against
the plain restatement (tests/gene_site_ref.py) over the matrices that were loaded or that read_matrix() returns -- a path that
shares nothing with the new code.  Every comparison is an equality of integers; the one double is compared bit for bit."""
import numpy as np
import pytest

import gene_site_ref as ref

pytestmark = pytest.mark.gpu

PS_ERR_INVALID, PS_ERR_STATE = -1, -6
BASES = np.array([1, 2, 4, 8], np.uint8)


def _onehot(rng, N, L):
    return BASES[rng.integers(0, 4, (N, L))]


def related(rng, N, L, G, founders=5, moves=3):
    """`founders` unrelated individuals; every other one copies an earlier one and moves away by a few core sites and gene
    flips (as related() of tests/test_gpu_locus_ld.py): loci carry the founders' structure, r^2 is not all near 0"""
    core, acc = _onehot(rng, N, L), (rng.random((N, G)) < 0.4).astype(np.uint8)
    for k in range(min(founders, N), N):
        src = rng.integers(k)
        core[k], acc[k] = core[src], acc[src]
        sites = rng.choice(L, rng.integers(0, moves), replace=False)
        core[k, sites] = BASES[(np.log2(core[k, sites]).astype(int) + 1 + rng.integers(0, 3, sites.size)) % 4]
        if G:
            acc[k, rng.choice(G, rng.integers(0, moves), replace=False)] ^= 1
    order = rng.permutation(N)
    return np.ascontiguousarray(core[order]), np.ascontiguousarray(acc[order])


def _handles(pa, core_m, acc_m):
    N, L = core_m.shape
    core = pa.Population(N, L, 4, True, 0.0, 0, 0)
    core.load_matrix(core_m)
    acc = pa.Population(N, acc_m.shape[1], 2, False, 0.5, 0, 0)
    acc.load_matrix(acc_m)
    return core, acc


def _check(core, acc, core_m, acc_m, **kw):
    """the device against the restatement of the two matrices -> the result"""
    got = core.gene_site_ld(acc, **kw)
    ref.assert_equal(got, ref.gene_site(ref.core_indicators(core_m), ref.acc_indicators(acc_m), **kw))
    assert got.pairs == got.defined_pairs + got.undefined_pairs == got.sites * got.genes
    assert all(ms >= 0.0 for ms in core.gene_site_ld_timing())
    return got


@pytest.mark.parametrize("N,L,G", [(2, 8, 5), (7, 203, 40), (64, 130, 64), (65, 130, 65), (300, 1001, 500), (1030, 300, 100), (2049, 70, 70)])
def test_loaded_matrices(pa, N, L, G):
    """N below, at and just above a 32-, 64-, 128- and 1024-cell boundary of the pack kernels and of WP; Mg + Ms below and above
    128 and no multiple of it, Mg a multiple of 4 and not (the aligned start of the site columns); automatic selection on both
    sides"""
    rng = np.random.default_rng(N)
    core_m, acc_m = related(rng, N, L, G)
    core, acc = _handles(pa, core_m, acc_m)
    got = _check(core, acc, core_m, acc_m, r2_bins=64, freq_bins=4)
    if N >= 64:
        assert got.sites > 1 and got.genes > 1 and got.defined_pairs > 0
        assert 0.0 < got.mean_r2 < 1.0 and np.count_nonzero(got.hist) > 4
    core.close()
    acc.close()


def test_three_bands_equal_one(pa):
    """Mg = 150 with ld_band = 64: three bands of gene rows (64 + 64 + 22) equal the unforced call and the restatement -- a
    per-site maximum or site_strong that forgets the earlier bands would not"""
    rng = np.random.default_rng(7)
    core_m, acc_m = related(rng, 150, 400, 330, founders=9, moves=30)
    core, acc = _handles(pa, core_m, acc_m)
    kw = dict(r2_bins=32, freq_bins=8, max_sites=200, max_genes=150, strong_q=20000)
    whole = _check(core, acc, core_m, acc_m, **kw)
    assert whole.genes == 150 and whole.sites == 200 and whole.strong_pairs > 0
    best_band = np.searchsorted(whole.gene_index, whole.site_best_gene[whole.site_best_gene != ref.NONE]) // 64
    assert len(set(best_band.tolist())) == 3            # (the best genes of the sites lie in all three bands)
    core.set_tuning("ld_band", 64)
    banded = _check(core, acc, core_m, acc_m, **kw)
    core.set_tuning("ld_band", 0)
    d, w = banded.as_dict(), whole.as_dict()
    assert all(np.array_equal(d[k], w[k]) for k in w)
    core.close()
    acc.close()


def test_planted_associations(pa):
    rng = np.random.default_rng(200)
    N, L, G = 200, 120, 60
    core_m, acc_m = related(rng, N, L, G)
    core_m[:, 17] = np.where(rng.random(N) < 0.35, 2, 8)            # a site of its own, so that nothing else equals it
    core_m[:, 90] = core_m[:, 17]                                   # ... but site 90, on purpose: the tie goes to 17
    x17 = ref.core_indicators(core_m)[17]
    acc_m[:, 5] = x17                                               # a copy
    acc_m[:, 6] = 1 - x17                                           # the complement
    acc_m[:, 40] = acc_m[:, 5]                                      # two identical genes: a site reports the lower one
    core, acc = _handles(pa, core_m, acc_m)
    got = _check(core, acc, core_m, acc_m, r2_bins=64, freq_bins=5)
    g = {int(c): k for k, c in enumerate(got.gene_index)}
    s = {int(c): k for k, c in enumerate(got.site_index)}
    for gene, sign in ((5, 1), (6, -1), (40, 1)):
        assert (got.gene_best_site[g[gene]], got.gene_best_q[g[gene]], got.gene_best_sign[g[gene]]) == (17, 65536, sign)
    for site in (17, 90):
        assert (got.site_best_gene[s[site]], got.site_best_q[s[site]], got.site_best_sign[s[site]]) == (5, 65536, 1)
    Xs, Xg = ref.core_indicators(core_m), ref.acc_indicators(acc_m)
    strong = lambda x, Y: sum(ref.pair_q(N, int(x.sum()), int(y.sum()), int((x & y).sum()))[1] >= 32768      # noqa: E731
                              for y in Y if 0 < y.sum() < N)
    assert got.gene_strong[g[5]] == got.gene_strong[g[6]] == got.gene_strong[g[40]] == strong(x17, Xs[got.site_index]) >= 2
    assert got.site_strong[s[17]] == got.site_strong[s[90]] == strong(x17, Xg[got.gene_index]) >= 3
    assert got.complete_pairs >= 6 and got.genes_tagged >= 3 and got.sites_tagging >= 2
    core.close()
    acc.close()


def test_caps_minors_and_bins(pa):
    """more candidates than the caps on both sides (the stride rule); minors above 1; freq_bins 1, 5, 32; r2_bins 1"""
    rng = np.random.default_rng(5)
    core_m, acc_m = related(rng, 90, 1001, 300, founders=8, moves=40)
    core, acc = _handles(pa, core_m, acc_m)
    for max_sites in (100, 128):
        for freq_bins in (1, 5, 32):
            got = _check(core, acc, core_m, acc_m, r2_bins=16, freq_bins=freq_bins, max_sites=max_sites, max_genes=50)
            assert got.site_candidates > max_sites == got.sites and got.gene_candidates > 50 == got.genes
    _check(core, acc, core_m, acc_m, r2_bins=16, freq_bins=3, site_min_minor=30, gene_min_minor=9, max_sites=300, max_genes=100)
    _check(core, acc, core_m, acc_m, r2_bins=1, freq_bins=1, site_min_minor=45, gene_min_minor=40, max_sites=7, max_genes=9, strong_q=1)
    core.close()
    acc.close()


def test_explicit_lists_with_monomorphic_entries(pa):
    rng = np.random.default_rng(8)
    N, L, G = 200, 150, 90
    core_m, acc_m = related(rng, N, L, G)
    core_m[:, [3, 77]] = 4
    acc_m[:, 10], acc_m[:, 50] = 0, 1
    core, acc = _handles(pa, core_m, acc_m)
    sites = sorted(set(rng.choice(L, 60, replace=False).tolist()) | {3, 77})
    genes = sorted(set(rng.choice(G, 30, replace=False).tolist()) | {10, 50})
    got = _check(core, acc, core_m, acc_m, r2_bins=32, freq_bins=6, sites=sites, genes=genes)
    poly_s = int(((got.site_count > 0) & (got.site_count < N)).sum())
    poly_g = int(((got.gene_count > 0) & (got.gene_count < N)).sum())
    assert poly_s <= len(sites) - 2 and poly_g <= len(genes) - 2 and (got.site_candidates, got.gene_candidates) == (poly_s, poly_g)
    assert got.undefined_pairs == len(sites) * len(genes) - poly_s * poly_g
    for gene in (10, 50):
        k = genes.index(gene)
        assert (got.gene_best_site[k], got.gene_best_q[k], got.gene_best_sign[k], got.gene_strong[k]) == (ref.NONE, 0, 0, 0)
    assert got.site_best_gene[sites.index(3)] == ref.NONE
    # one side explicit, the other automatic
    _check(core, acc, core_m, acc_m, sites=sites, max_genes=40)
    _check(core, acc, core_m, acc_m, genes=genes, max_sites=70)
    # an empty list: no pairs, the other side is still listed
    got = _check(core, acc, core_m, acc_m, sites=[], max_genes=40)
    assert got.pairs == 0 and got.genes == 40 and got.mean_r2 == 0.0 and (got.gene_best_site == ref.NONE).all()
    for kw in (dict(sites=[5, 5]), dict(sites=[9, 4]), dict(sites=[0, L]), dict(genes=[5, 5]), dict(genes=[9, 4]), dict(genes=[0, G])):
        with pytest.raises(pa.PansimError) as e:
            core.gene_site_ld(acc, **kw)
        assert e.value.code == PS_ERR_INVALID, kw
    core.close()
    acc.close()


def test_not_one_hot(pa):
    """arbitrary bytes in about 5 % of the cells: they are in no class, neither for the major base nor for the indicator"""
    rng = np.random.default_rng(31)
    N, L, G = 130, 300, 40
    core_m, acc_m = related(rng, N, L, G)
    cells = rng.random((N, L)) < 0.05
    core_m[cells] = rng.integers(0, 256, int(cells.sum()), dtype=np.uint8)
    core_m[:, 7] = 3                      # a site without a single base: monomorphic at c = 0
    core_m[: N // 2, 8], core_m[N // 2:, 8] = 1, 2        # a tie: the lowest byte is the major base
    core, acc = _handles(pa, core_m, acc_m)
    _check(core, acc, core_m, acc_m, r2_bins=64, freq_bins=3)
    got = _check(core, acc, core_m, acc_m, sites=[6, 7, 8, 9])
    assert got.site_count[1] == 0 and got.site_count[2] == int((core_m[:, 8] == 1).sum()) and got.site_best_gene[1] == ref.NONE
    core.close()
    acc.close()


SIM = dict(core_size=2048, pan_genes=400, core_genes=20, HR_rate=0.5, HGT_rate=0.5, prop_positive=0.5, seed=11, n_gen=25, max_distances=100)
KW = dict(r2_bins=32, freq_bins=5, max_sites=200, max_genes=120)


def _restated(sim, **kw):
    core_m, acc_m = sim.core_genome.read_matrix(), sim.pan_genome.read_matrix()
    return ref.gene_site(ref.core_indicators(core_m), ref.acc_indicators(acc_m), **kw)


@pytest.fixture(scope="module")
def sim_300_after_twenty(pa):
    sim = pa.Simulation(pa.make_params(pop_size=300, **SIM))
    sim.run(20)
    got = sim.gene_site_ld(**KW)            # no sync: ordered behind the run, a two-generation sweep launch included
    timing = sim.gene_site_ld_timing()
    want = _restated(sim, **KW)
    sim.run(5)
    state = (sim.core_genome.read_matrix(), sim.pan_genome.read_matrix(), sim.last_parents())
    sim.close()
    return got, want, timing, state


def test_a_simulation_after_twenty_generations(pa, sim_300_after_twenty):
    got, want, timing, state = sim_300_after_twenty
    ref.assert_equal(got, want)
    assert got.sites > 1 and got.genes > 1 and got.defined_pairs > 0 and len(timing) == 4 and all(ms >= 0.0 for ms in timing)
    # the call changed no state: the run that asked continues bit for bit with one that never did
    plain = pa.Simulation(pa.make_params(pop_size=300, **SIM))
    plain.run(25)
    assert np.array_equal(plain.core_genome.read_matrix(), state[0]) and np.array_equal(plain.pan_genome.read_matrix(), state[1])
    assert np.array_equal(plain.last_parents(), state[2])
    plain.close()


@pytest.mark.parametrize("shards", [2, 3])
def test_shards_equal_the_unsharded_run(pa, sim_300_after_twenty, shards):
    _, want, _, _ = sim_300_after_twenty
    multi = pa.MultiSimulation(pa.make_params(pop_size=300, **SIM), shards, devices=[0] * shards)
    multi.run(20)
    ref.assert_equal(multi.gene_site_ld(**KW), want)
    assert all(ms >= 0.0 for ms in multi.gene_site_ld_timing())
    # fewer sites than candidates, and an explicit list across the shards: global columns
    core_m = np.concatenate([s.core_genome.read_matrix() for s in multi.shards], axis=1)
    Xs, Xg = ref.core_indicators(core_m), ref.acc_indicators(multi.shards[0].pan_genome.read_matrix())
    for kw in (dict(max_sites=37, max_genes=50), dict(sites=list(range(0, 2048, 29)), max_genes=60, freq_bins=7)):
        ref.assert_equal(multi.gene_site_ld(**kw), ref.gene_site(Xs, Xg, **kw))
    with pytest.raises(pa.PansimError) as e:             # a site shard on its own
        multi.shards[1].core_genome.gene_site_ld(multi.shards[1].pan_genome)
    assert e.value.code == PS_ERR_INVALID and "ps_multi_gene_site_ld" in str(e.value)
    multi.close()


def test_limits_and_handles(pa):
    rng = np.random.default_rng(6)
    core, acc = _handles(pa, _onehot(rng, 20, 64), (rng.random((20, 10)) < 0.5).astype(np.uint8))
    with pytest.raises(pa.PansimError) as e:
        core.gene_site_ld_timing()
    assert e.value.code == PS_ERR_STATE and "no gene-site association" in str(e.value)
    for kw in (dict(r2_bins=0), dict(freq_bins=0), dict(r2_bins=16385), dict(r2_bins=1024, freq_bins=32), dict(site_min_minor=0),
               dict(gene_min_minor=0), dict(max_sites=0), dict(max_genes=0), dict(max_sites=65536, max_genes=1), dict(strong_q=0),
               dict(strong_q=65537), dict(sites=[1, 2], max_genes=65535)):
        with pytest.raises(pa.PansimError) as e:
            core.gene_site_ld(acc, **kw)
        assert e.value.code == PS_ERR_INVALID, kw
    other = pa.Population(21, 10, 2, False, 0.5, 0, 0)
    for first, second, word in ((acc, acc, "core handle first"), (core, core, "accessory handle second"), (core, other, "individuals")):
        with pytest.raises(pa.PansimError) as e:
            first.gene_site_ld(second)
        assert e.value.code == PS_ERR_INVALID and word in str(e.value)
    assert core.gene_site_ld(acc, max_sites=65535, max_genes=1).genes <= 1
    for p in (core, acc, other):
        p.close()
