"""The gene gain / loss model on the device (ps_tree_gene_likelihood, ps_tree_gene_ancestral, ps_tree_gene_fit and their ps_sim /
ps_multi forms, docs/GENE_MODEL.md) against the host entries, which tests/test_gene_model.py holds against the sum over all
assignments.

Every gene's (mantissa, exponent), class posteriors, mean rate and every cell's state are the same bits on host and device (one
header, gene_rule.h): the matrix read back from the new handle equals the host's byte for byte, the fit takes the same decisions
and returns the same bits, and only the sums over the genes, and log, differ.  The bounds:
  lnL          2^-53 (G + 8) sum_g (|ln l_g| + 2), the bound of tests/test_gpu_tree_model.py;
  every sum    2 G K 2^-53 of its own value: G K non-negative terms at the most, added in another order.
The shapes are the smallest at which each thing can go wrong: the smallest trees, a single gene, M = 63, 64, 65 inner nodes (a word
of the new gene-major rows), G = 63, 64, 65, 129 genes (a word of the new individual-major rows), the single-wave team against the
shared one (256 / 257; 1024 / 1025 on deep and wide trees), the largest tree of each form (the LDS at its limit), one leaf more
(refused), and 20 000 genes of a small tree (the grid-stride loop and one row of sums per workgroup)."""
import numpy as np
import pytest

import gene_model_ref as gref
import tree_likelihood_ref as ref

pytestmark = pytest.mark.gpu

PS_ERR_INVALID, PS_ERR_STATE = -1, -6
EPS = 2.0 ** -53
MAXP, MAXM = 2304, 1792
SHAPES = [(2, 1, "caterpillar"), (3, 5, "caterpillar"), (4, 6, "balanced"), (17, 7, "random"), (64, 9, "random"), (65, 63, "caterpillar"),
          (66, 64, "random"), (256, 65, "balanced"), (257, 129, "random"), (1024, 5, "caterpillar"), (1025, 6, "random"),
          (MAXM, 4, "random"), (MAXM + 1, 4, "random"), (MAXP, 3, "random"), (MAXP + 1, 3, "caterpillar"), (64, 20000, "random")]
COUNTERS = ("pop_size", "genes", "merges", "categories", "classed", "zero_genes", "clamped_lengths")


def acc_handle(pa, rows):
    p = pa.Population(rows.shape[0], rows.shape[1], 2, False, 0.5, 0, 3)
    p.load_matrix(rows)
    return p


def tree_of(rng, N, kind):
    if kind == "caterpillar":
        return ref.caterpillar(N, rng.permutation(N))
    if kind == "balanced":
        return ref.balanced(N)
    return ref.random_tree(N, rng)


def case(N, G, kind):
    rng = np.random.default_rng(N * 37 + G)
    left, right = tree_of(rng, N, kind)
    t = rng.uniform(0.005, 0.3, 2 * N - 1)
    idx = rng.choice(2 * N - 2, min(3, 2 * N - 2), replace=False)     # (never the root's entry, which is not read)
    t[idx] = [0.0, -0.5, 4000.0][:idx.size]                            # two clamped entries and a branch in generations
    rows = gref.evolve(rng, left, right, np.maximum(t, 1e-8), 0.8, 1.1, 0.5, G)[0]
    if G >= 3:
        rows[:, 1] = 0                                                  # absent everywhere
        rows[:, 2] = 1                                                  # present everywhere
    return rows, left, right, t


def models(pa, G):
    """K = 1; three assigned classes; a four-class mixture with a rate of 0; the simulator's shape: pi = (1/2, 1/2), two assigned
    compartments"""
    rng = np.random.default_rng(G)
    comp = np.zeros(G, np.uint8)
    comp[G - G // 10:] = 1
    return [pa.GeneModel((0.7, 0.3), root=(0.4, 0.6), rates=(0.8,)),
            pa.GeneModel((0.6, 0.4), root=(0.5, 0.5), rates=(0.2, 1.0, 30.0), gene_class=rng.integers(0, 3, G)),
            pa.GeneModel((0.8, 0.2), root=(0.45, 0.55), rates=(0.0, 0.4, 1.0, 2.6), weights=(0.1, 0.4, 0.3, 0.2)),
            pa.GeneModel((0.5, 0.5), root=(0.55, 0.45), rates=(0.0002, 0.4), weights=(0.9, 0.1), gene_class=comp)]


def lnl_close(got, want, gene_lnl, factor=1.0):
    if not np.isfinite(want):
        return got == want
    bound = factor * EPS * (gene_lnl.size + 8) * (np.abs(gene_lnl[np.isfinite(gene_lnl)]) + 2.0).sum()
    print("lnl", got, want, abs(got - want), bound)
    return abs(got - want) <= bound


def sums_close(got, want, G, K, factor=1.0):
    f = factor * 2 * G * K * EPS
    for name in ("node_conf", "node_genes", "branch_gains", "branch_losses", "gene_gains", "gene_losses"):
        a, b = getattr(got, name), getattr(want, name)
        err = np.abs(a - b)
        print(name, float((err / np.maximum(b, 1e-300)).max()) if b.size else 0.0, f)
        if not np.all(err <= f * b):
            return False
    for name in ("total_gains", "total_losses", "mean_conf", "total_genes"):
        if not abs(getattr(got, name) - getattr(want, name)) <= f * getattr(want, name):
            return False
    return got.branch_gains[-1] == 0.0 and got.branch_losses[-1] == 0.0


def same_bits(a, b):
    for name in COUNTERS + ("lnl", "total_gains", "total_losses", "mean_conf", "total_genes"):
        assert getattr(a, name) == getattr(b, name), name
    for name in ("node_conf", "node_genes", "branch_gains", "branch_losses", "gene_gains", "gene_losses"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize("N,G,kind", SHAPES)
def test_device_equals_host(pa, N, G, kind):
    rows, left, right, t = case(N, G, kind)
    acc = acc_handle(pa, rows)
    for model in models(pa, G):
        mixture = model.gene_class is None and model.categories > 1
        cap, name = (MAXM, "PS_GENE_MAX_POP_MIX = 1792") if mixture else (MAXP, "PS_GENE_MAX_POP = 2304")
        if N > cap:
            for call in (acc.tree_gene_likelihood, acc.tree_gene_ancestral, acc.tree_gene_fit):
                with pytest.raises(pa.PansimError) as e:
                    call(left, right, t, model)
                assert e.value.code == PS_ERR_INVALID and "pop_size <= " + name in str(e.value), str(e.value)
            continue
        K = model.categories
        want = pa.gene_likelihood_from_rows(rows, left, right, t, model)
        got = acc.tree_gene_likelihood(left, right, t, model, per_gene=True)
        for name in COUNTERS:
            assert getattr(got, name) == getattr(want, name), name
        assert np.array_equal(got.gene_mant, want.gene_mant) and np.array_equal(got.gene_exp, want.gene_exp)
        assert np.array_equal(got.gene_post, want.gene_post) and np.array_equal(got.gene_rate, want.gene_rate)
        assert lnl_close(got.lnl, want.lnl, want.gene_lnl())
        assert got.clamped_lengths >= 1
        bare = acc.tree_gene_likelihood(left, right, t, model)
        assert bare.gene_mant is None and bare.lnl == got.lnl
        # the reconstruction
        hw = pa.gene_ancestral_from_rows(rows, left, right, t, model)
        dev = acc.tree_gene_ancestral(left, right, t, model)
        made = dev.population
        assert made.size == N - 1 and made.ncols == G and not made.core
        assert np.array_equal(made.read_matrix(), hw.rows)
        # (the gene counts read every word of the gene-major rows: the pad bits)
        assert np.array_equal(made.gene_frequencies()[:G], hw.rows.sum(axis=0) / (N - 1))
        for name in COUNTERS:
            assert getattr(dev, name) == getattr(hw, name), name
        assert lnl_close(dev.lnl, hw.lnl, want.gene_lnl()) and dev.lnl == got.lnl
        assert sums_close(dev, hw, G, K)
        again = acc.tree_gene_ancestral(left, right, t, model)
        same_bits(dev, again)
        assert np.array_equal(again.population.read_matrix(), hw.rows)
        again.close()
        dev.close()
    acc.close()


@pytest.mark.parametrize("N,G,kind", [(17, 7, "random"), (66, 64, "random"), (65, 129, "caterpillar")])
def test_the_device_fit_is_the_host_fit_bit_for_bit(pa, N, G, kind):
    rows, left, right, t = case(N, G, kind)
    t = np.minimum(t, 0.5)
    acc = acc_handle(pa, rows)
    for model in models(pa, G)[1:]:
        want = pa.gene_fit_from_rows(rows, left, right, t, model, max_rounds=3, eps_lnl=1e-3)
        got = acc.tree_gene_fit(left, right, t, model, max_rounds=3, eps_lnl=1e-3)
        for name in COUNTERS + ("rounds", "passes", "converged", "lnl", "start_lnl", "beta", "mean_rate"):
            assert getattr(got, name) == getattr(want, name), name
        assert np.array_equal(got.round_lnl, want.round_lnl) and got.rounds >= 1 and got.passes > 10
        for name in ("rates", "weights", "freq", "root"):
            assert np.array_equal(getattr(got.model, name), getattr(want.model, name)), name
        assert np.all(np.diff(got.round_lnl) >= 0.0)
        ms = acc.tree_gene_timing()
        assert len(ms) == 3 and ms[1] > 0.0
    acc.close()


def test_both_teams_give_the_same_bits_per_gene(pa):
    """the tuning key "gene_team": one wave against 256 threads on the same tree"""
    rows, left, right, t = case(300, 40, "random")
    acc = acc_handle(pa, rows)
    model = models(pa, 40)[2]
    out = []
    for team in (64, 256, 0):
        acc.set_tuning("gene_team", team)
        lik, dev = acc.tree_gene_likelihood(left, right, t, model, per_gene=True), acc.tree_gene_ancestral(left, right, t, model)
        out.append((lik.gene_mant, lik.gene_exp, lik.gene_post, dev.population.read_matrix(), dev))
    hw = pa.gene_ancestral_from_rows(rows, left, right, t, model)
    for o in out:
        assert all(np.array_equal(a, b) for a, b in zip(o[:4], out[0][:4])) and np.array_equal(o[3], hw.rows)
        assert sums_close(o[4], hw, 40, 4)
        o[4].close()
    with pytest.raises(pa.PansimError) as e:
        acc.set_tuning("gene_team", 128)
    assert e.value.code == PS_ERR_INVALID and "gene_team" in str(e.value)
    acc.close()


SIM = dict(pop_size=100, core_size=2001, pan_genes=300, core_genes=20, HR_rate=0.5, HGT_rate=0.5, seed=11, n_gen=8, max_distances=100)


def run_tree(sim):
    left, right = sim.upgma_tree().merges()
    rng = np.random.default_rng(4)
    return left, right, rng.uniform(0.5, 6.0, 2 * SIM["pop_size"] - 1)


def test_a_simulation_and_no_change_of_state(pa):
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(6)
    left, right, t = run_tree(sim)
    rows = sim.pan_genome.read_matrix()
    G = rows.shape[1]
    model = pa.GeneModel.simulator(sim)
    assert model.gene_class.size == G
    for mod in (model, model.mixture()):
        K = mod.categories
        want, hw = pa.gene_likelihood_from_rows(rows, left, right, t, mod), pa.gene_ancestral_from_rows(rows, left, right, t, mod)
        own = sim.pan_genome.tree_gene_likelihood(left, right, t, mod, per_gene=True)
        got = sim.tree_gene_likelihood(left, right, t, mod, per_gene=True)
        assert got.lnl == own.lnl and np.array_equal(got.gene_mant, own.gene_mant) and np.array_equal(got.gene_mant, want.gene_mant)
        assert np.array_equal(got.gene_post, want.gene_post) and lnl_close(got.lnl, want.lnl, want.gene_lnl())
        dev = sim.tree_gene_ancestral(left, right, t, mod)
        assert dev.population.size == 99 and dev.population.ncols == G and np.array_equal(dev.population.read_matrix(), hw.rows)
        assert sums_close(dev, hw, G, K)
        fit_h = pa.gene_fit_from_rows(rows, left, right, t, mod, max_rounds=2)
        fit_d = sim.tree_gene_fit(left, right, t, mod, max_rounds=2)
        assert np.array_equal(fit_d.round_lnl, fit_h.round_lnl) and np.array_equal(fit_d.model.rates, fit_h.model.rates)
        assert np.array_equal(fit_d.model.freq, fit_h.model.freq) and np.array_equal(fit_d.model.weights, fit_h.model.weights)
        dev.close()
    ms = sim.tree_gene_timing()
    assert len(ms) == 3 and ms[0] >= 0.0 and ms[1] > 0.0 and ms[2] >= 0.0
    assert np.array_equal(sim.pan_genome.read_matrix(), rows)
    sim.run(2)
    plain = pa.Simulation(pa.make_params(**SIM))
    plain.run(8)
    assert np.array_equal(plain.core_genome.read_matrix(), sim.core_genome.read_matrix())
    assert np.array_equal(plain.pan_genome.read_matrix(), sim.pan_genome.read_matrix())
    plain.close()
    sim.close()


def test_multi_simulation_against_the_unsharded_run(pa):
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(5)
    left, right, t = run_tree(sim)
    model = pa.GeneModel.simulator(sim)
    lik, anc, fit = (sim.tree_gene_likelihood(left, right, t, model, per_gene=True), sim.tree_gene_ancestral(left, right, t, model),
                     sim.tree_gene_fit(left, right, t, model, max_rounds=2))
    rows = anc.population.read_matrix()
    sim.close()
    multi = pa.MultiSimulation(pa.make_params(**SIM), 2, devices=[0, 0])
    multi.run(5)
    got = multi.tree_gene_likelihood(left, right, t, model, per_gene=True)
    assert got.lnl == lik.lnl and np.array_equal(got.gene_mant, lik.gene_mant) and np.array_equal(got.gene_exp, lik.gene_exp)
    dev = multi.tree_gene_ancestral(left, right, t, model)
    assert np.array_equal(dev.population.read_matrix(), rows)
    same_bits(dev, anc)
    mfit = multi.tree_gene_fit(left, right, t, model, max_rounds=2)
    assert np.array_equal(mfit.round_lnl, fit.round_lnl) and np.array_equal(mfit.model.rates, fit.model.rates)
    assert len(multi.tree_gene_timing()) == 3
    dev.close()
    anc.close()
    multi.close()


def test_the_made_handle_is_a_working_population(pa):
    N, G = 131, 200
    rows, left, right, t = case(N, G, "random")
    model = models(pa, G)[0]
    acc = acc_handle(pa, rows)
    rng = np.random.default_rng(5)
    core = pa.Population(N - 1, 64, 4, True, 0.0, 0, 0)
    core.load_matrix(np.array(ref.BASES, np.uint8)[rng.integers(0, 4, (N - 1, 64))])
    got = acc.tree_gene_ancestral(left, right, t, model)
    anc = got.population
    inner = anc.read_matrix()
    both = pa.pool([acc, anc])
    assert both.size == 2 * N - 1 and np.array_equal(both.read_matrix(), np.vstack([(rows != 0).astype(np.uint8), inner]))
    cat = ref.caterpillar(N - 1)
    dev, host = core.tree_parsimony(*cat, acc=anc, genes=True), pa.parsimony_from_rows(inner, *cat, genes=True)
    assert dev.gene_total_changes == host.gene_total_changes and np.array_equal(dev.gene_changes, host.gene_changes)
    # the reconstruction's own gains and losses beside the model's expected ones: the same order of magnitude
    child, parent = np.concatenate([left, right]), np.concatenate([np.arange(N, 2 * N - 1)] * 2)
    st = both.read_matrix().astype(int)
    gains, losses = ((st[child] - st[parent]) == 1).sum(), ((st[child] - st[parent]) == -1).sum()
    assert 0.2 * got.total_gains < gains < 5.0 * got.total_gains and 0.2 * got.total_losses < losses < 5.0 * got.total_losses
    # either order of destruction
    acc.close()
    assert np.array_equal(anc.read_matrix(), inner)
    both.close()
    got.close()
    other = acc_handle(pa, rows)
    late = other.tree_gene_ancestral(left, right, t, model)
    other_rows = late.population.read_matrix()
    late.close()
    assert np.array_equal(other_rows, inner)
    assert other.tree_gene_ancestral(left, right, t, model, states=False).population is None
    other.close()
    core.close()


def test_without_states_nothing_is_allocated(pa):
    """a new matrix of 2 x 64 MB: with states=False the device's free memory stays, with states=True it drops"""
    import torch
    N, G = 2049, 65536
    rng = np.random.default_rng(8)
    rows = (rng.random((N, 1)) < 0.5).astype(np.uint8) ^ (rng.random((N, G)) < 0.01).astype(np.uint8)
    left, right = ref.balanced(N)
    t = np.full(2 * N - 1, 0.1)
    model = pa.GeneModel((0.5, 0.5), rates=(0.5,))
    acc = acc_handle(pa, rows)
    first = acc.tree_gene_ancestral(left, right, t, model, states=False)       # (the scratch of the handle is grown here)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    none = acc.tree_gene_ancestral(left, right, t, model, states=False)
    free1 = torch.cuda.mem_get_info()[0]
    assert none.population is None and abs(free1 - free0) < 16 << 20
    same_bits(first, none)
    some = acc.tree_gene_ancestral(left, right, t, model)
    free2 = torch.cuda.mem_get_info()[0]
    assert free0 - free2 >= 3 * (N - 1) * G // 8 - (16 << 20)                   # (the two row buffers and the gene-major view)
    same_bits(first, some)
    some.close()
    acc.close()


def test_timing_before_a_call_and_handle_checks(pa):
    rows, left, right, t = case(20, 10, "random")
    acc = acc_handle(pa, rows)
    with pytest.raises(pa.PansimError) as e:
        acc.tree_gene_timing()
    assert e.value.code == PS_ERR_STATE
    model = models(pa, 10)[0]
    core = pa.Population(20, 64, 4, True, 0.0, 0, 0)
    core.load_matrix(np.full((20, 64), 2, np.uint8))
    for call in (core.tree_gene_likelihood, core.tree_gene_ancestral, core.tree_gene_fit):
        with pytest.raises(pa.PansimError) as e:
            call(left, right, t, model)
        assert e.value.code == PS_ERR_INVALID and "accessory handle" in str(e.value), str(e.value)
    bad = t.copy()
    bad[4] = np.inf
    for l, r, tt, mod, text in ((left[:-1], right[:-1], t[:-1], model, "spanning tree: 19 merges over 20 leaves, not 18"),
                                (left, right, bad, model, "length of node 4 is not a finite number"),
                                (left, right, t, pa.GeneModel((1.0, 0.0)), "freq[1] must be a number > 0"),
                                (left, right, t, pa.GeneModel((0.5, 0.5), rates=(1.0, 2.0), gene_class=np.zeros(9, np.uint8)),
                                 "gene_classes = 10, not 9")):
        with pytest.raises(pa.PansimError) as e:
            acc.tree_gene_ancestral(l, r, tt, mod)
        assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)
    acc.tree_gene_likelihood(left, right, t, model)
    ms = acc.tree_gene_timing()
    assert len(ms) == 3 and ms[0] >= 0.0 and ms[1] > 0.0 and ms[2] > 0.0
    for p in (acc, core):
        p.close()
