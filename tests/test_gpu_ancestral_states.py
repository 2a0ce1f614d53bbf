"""The marginal ancestral states on the device (ps_tree_ancestral_states and its ps_sim / ps_multi forms,
docs/ANCESTRAL_STATES.md) against the host entry, which tests/test_ancestral_states.py holds against the sum over all assignments.

Every cell's posterior, arg max and pdiff are the same bits on host and device (one header, subst_rule.h): the matrix read back from
the new handle equals the host's byte for byte, and only the sums over the sites, and log, differ.  The bounds:
  lnL                     2^-53 (L + 8) sum_s (|ln l_s| + 2), the bound of tests/test_gpu_tree_model.py;
  node_conf, branch_diff  2 L K 2^-53 of their own values: L K non-negative terms at the most, added in another order.
The shapes are the smallest at which each thing can go wrong: the smallest trees, a single site, the lane boundary (64 / 65), tiles
that are not full (L = 5, 6, 7, 9), the single-wave team against the shared one (1024 / 1025), the largest tree of each form (the LDS
at its limit), one leaf more (refused), and 20 000 sites of a small tree (the grid-stride loop and one row of sums per workgroup).
Each runs on one-hot bytes and with arbitrary bytes among them, under the four models of tests/test_gpu_tree_model.py."""
import numpy as np
import pytest

import tree_likelihood_ref as ref

pytestmark = pytest.mark.gpu

PS_ERR_INVALID, PS_ERR_STATE = -1, -6
EPS = 2.0 ** -53
MAXP, MAXM = 2304, 1536
SHAPES = [(2, 1, "caterpillar"), (3, 5, "caterpillar"), (4, 1, "balanced"), (17, 6, "random"), (64, 9, "random"), (65, 5, "caterpillar"),
          (256, 7, "balanced"), (1024, 5, "caterpillar"), (1025, 5, "random"), (MAXM, 4, "random"), (MAXM + 1, 4, "random"),
          (MAXP, 4, "random"), (MAXP + 1, 4, "caterpillar"), (64, 20000, "random")]
ROOT = (0.4, 0.3, 0.2, 0.1)


def core_handle(pa, m, **kw):
    p = pa.Population(m.shape[0], m.shape[1], 4, True, 0.0, 0, 0, **kw)
    p.load_matrix(m)
    return p


def tree_of(rng, N, kind):
    if kind == "caterpillar":
        return ref.caterpillar(N, rng.permutation(N))
    if kind == "balanced":
        return ref.balanced(N)
    return ref.random_tree(N, rng)


def case(N, L, kind, junk):
    rng = np.random.default_rng(N * 31 + L)
    left, right = tree_of(rng, N, kind)
    t = rng.uniform(0.005, 0.3, 2 * N - 1)
    t[rng.integers(0, 2 * N - 1, 3)] = [0.0, -0.5, 40.0]              # clamped entries
    m = ref.evolve(left, right, t, N, L, rng)
    if junk:
        m[rng.random(m.shape) < 0.03] = rng.integers(0, 256, 1, dtype=np.uint8)[0]
        m[0, 0] = 0
    if L >= 16:
        m[:, 8:12] = 4                                                  # a fully monomorphic tile
    return m, left, right, t


def models(pa, L):
    """the three of tests/test_gpu_tree_model.py::models and its JC69 anchor"""
    rng = np.random.default_rng(L)
    return [pa.SubstModel.simulator(),
            pa.SubstModel((0.1, 0.2, 0.3, 0.4), root=ROOT, rates=(0.0, 0.4, 1.0, 2.6), weights=(0.1, 0.4, 0.3, 0.2)),
            pa.SubstModel.simulator(rates=(0.1, 0.3, 0.6, 1.0, 1.5, 2.0, 3.0, 5.0), site_class=rng.integers(0, 8, L)),
            pa.SubstModel.jc69()]


COUNTERS = ("pop_size", "sites", "merges", "categories", "classed", "masked_cells", "zero_sites", "missing_cells", "clamped_lengths")


def lnl_bound(pa, m, left, right, t, model):
    """the bound of tests/test_gpu_tree_model.py from every site's ln l: of the likelihood entry where it takes the tree, else (above
    PS_LIK_MAX_POP; few sites there) of the host entry one column at a time"""
    if m.shape[0] <= pa.PS_LIK_MAX_POP:
        site = pa.model_likelihood_from_rows(m, left, right, t, model, derivatives=False).site_lnl
    else:
        site = np.array([pa.ancestral_from_rows(np.ascontiguousarray(m[:, s:s + 1]), left, right, t, model.sliced(s, s + 1), states=False).lnl
                         for s in range(m.shape[1])])
    return EPS * (m.shape[1] + 8) * (np.abs(site[np.isfinite(site)]) + 2.0).sum()


def assert_close(pa, got, want, m, left, right, t, model, factor=1.0):
    """a device result against the host's (factor 2: against another device sum that is within the bound of the host's)"""
    L, K = m.shape[1], model.categories
    for name in COUNTERS:
        assert getattr(got, name) == getattr(want, name), name
    bound = factor * lnl_bound(pa, m, left, right, t, model)
    print("lnl", got.lnl, want.lnl, abs(got.lnl - want.lnl), bound)
    assert got.lnl == want.lnl or abs(got.lnl - want.lnl) <= bound
    f = factor * 2 * L * K * EPS
    for name in ("node_conf", "branch_diff"):
        a, b = getattr(got, name), getattr(want, name)
        err = np.abs(a - b)
        print(name, float((err / np.maximum(b, 1e-300)).max()), f)
        assert np.all(err <= f * b), name
    assert abs(got.mean_conf - want.mean_conf) <= f * want.mean_conf and abs(got.total_diff - want.total_diff) <= f * want.total_diff
    assert got.branch_diff[-1] == 0.0


def same_bits(a, b):
    for name in COUNTERS + ("lnl", "mean_conf", "total_diff"):
        assert getattr(a, name) == getattr(b, name), name
    assert np.array_equal(a.node_conf, b.node_conf) and np.array_equal(a.branch_diff, b.branch_diff)


def bits(x):
    """the set bits of every row of a uint8 matrix"""
    return np.unpackbits(x, axis=1).sum(axis=1).astype(np.uint32)


def host_counts(rows):
    """(cols, 4) counts of the bytes 1, 2, 4, 8 of an individual-major matrix"""
    return np.stack([(rows == b).sum(axis=0) for b in ref.BASES], axis=1).astype(np.uint32)


@pytest.mark.parametrize("junk", [False, True], ids=["clean", "dirty"])
@pytest.mark.parametrize("N,L,kind", SHAPES)
def test_device_equals_host(pa, N, L, kind, junk):
    m, left, right, t = case(N, L, kind, junk)
    core = core_handle(pa, m)
    for model in models(pa, L):
        mixture = model.site_class is None and model.categories > 1
        cap, name = (MAXM, "PS_ANC_MAX_POP_MIX = 1536") if mixture else (MAXP, "PS_ANC_MAX_POP = 2304")
        if N > cap:
            with pytest.raises(pa.PansimError) as e:
                core.ancestral_states(left, right, t, model)
            assert e.value.code == PS_ERR_INVALID and "pop_size <= " + name in str(e.value), str(e.value)
            continue
        want = pa.ancestral_from_rows(m, left, right, t, model, min_posterior=0.3)
        got = core.ancestral_states(left, right, t, model, min_posterior=0.3)
        made = got.population
        assert made.size == N - 1 and made.ncols == L and made.core
        assert np.array_equal(made.read_matrix(), want.rows)
        # the pad of the device rows: the counts kernel loads whole rows of the pitch
        assert np.array_equal(made.site_allele_counts(), host_counts(want.rows))
        assert_close(pa, got, want, m, left, right, t, model)
        assert got.clamped_lengths >= 1 and got.missing_cells == int((~np.isin(m, ref.BASES)).sum())
        again = core.ancestral_states(left, right, t, model, min_posterior=0.3)
        same_bits(got, again)
        assert np.array_equal(again.population.read_matrix(), want.rows)
        again.close()
        got.close()
    core.close()


def test_an_assigned_invariant_class_and_every_cell_masked(pa):
    """a site of likelihood 0 on the device: byte 0 at every node, nothing added, counted; and min_posterior = 1"""
    m, left, right, t = case(70, 11, "random", junk=False)
    cls = np.zeros(11, np.uint8)
    cls[[2, 3, 9]] = 1
    model = pa.SubstModel.simulator(rates=(0.0, 1.0), site_class=cls)
    core = core_handle(pa, m)
    for cut in (0.0, 1.0):
        want = pa.ancestral_from_rows(m, left, right, t, model, min_posterior=cut)
        got = core.ancestral_states(left, right, t, model, min_posterior=cut)
        assert want.zero_sites >= 6 and got.zero_sites == want.zero_sites and got.masked_cells == want.masked_cells and got.lnl == want.lnl == -np.inf
        assert np.array_equal(got.population.read_matrix(), want.rows)
        variable = np.ptp(m, axis=0) > 0
        assert np.all(want.rows[:, variable & (cls == 0)] == 0) and want.zero_sites == int((variable & (cls == 0)).sum())
        f = 2 * 11 * 2 * EPS
        assert np.all(np.abs(got.node_conf - want.node_conf) <= f * want.node_conf) and np.all(np.abs(got.branch_diff - want.branch_diff) <= f * want.branch_diff)
        got.close()
    assert want.masked_cells > 0
    core.close()


SIM = dict(pop_size=100, core_size=2001, pan_genes=300, core_genes=20, HR_rate=0.5, HGT_rate=0.5, seed=11, n_gen=8, max_distances=100)


def test_a_simulation_and_no_change_of_state(pa):
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(6)
    left, right = sim.neighbour_joining().merges()[:2]
    m = sim.core_genome.read_matrix()
    rng = np.random.default_rng(3)
    t = rng.uniform(0.001, 0.05, 199)
    model = pa.SubstModel.simulator(rates=(0.3, 1.0, 2.5), site_class=rng.integers(0, 3, 2001))
    got = sim.ancestral_states(left, right, t, model)
    want = pa.ancestral_from_rows(m, left, right, t, model)
    assert got.pop_size == 100 and got.sites == 2001 and got.population.size == 99 and got.population.ncols == 2001
    assert np.array_equal(got.population.read_matrix(), want.rows)
    assert_close(pa, got, want, m, left, right, t, model)
    ms = sim.ancestral_states_timing()
    assert len(ms) == 3 and ms[0] >= 0.0 and ms[1] > 0.0 and ms[2] > 0.0
    assert np.array_equal(sim.core_genome.read_matrix(), m)
    sim.run(2)
    plain = pa.Simulation(pa.make_params(**SIM))
    plain.run(8)
    assert np.array_equal(plain.core_genome.read_matrix(), sim.core_genome.read_matrix())
    assert np.array_equal(plain.pan_genome.read_matrix(), sim.pan_genome.read_matrix())
    assert np.array_equal(got.population.read_matrix(), want.rows)         # the made handle is its own
    plain.close()
    sim.close()
    got.close()


@pytest.mark.parametrize("shards", [2, 3])
def test_multi_simulation_against_the_unsharded_run(pa, shards):
    """site_class is indexed by the global site: every shard takes its own slice and writes its own block of the one handle"""
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(5)
    left, right = sim.upgma_tree().merges()
    m = sim.core_genome.read_matrix()
    rng = np.random.default_rng(shards)
    t = rng.uniform(0.001, 0.05, 199)
    models_ = [pa.SubstModel.simulator(rates=(0.3, 1.0, 2.5), site_class=rng.integers(0, 3, 2001)),
               pa.SubstModel.simulator(rates=(0.3, 1.0, 2.5), weights=(0.3, 0.4, 0.3))]
    wants = [sim.ancestral_states(left, right, t, model, min_posterior=0.5) for model in models_]
    unsharded = [w.population.read_matrix() for w in wants]
    sim.close()
    multi = pa.MultiSimulation(pa.make_params(**SIM), shards, devices=[0] * shards)
    multi.run(5)
    for model, want, rows in zip(models_, wants, unsharded):
        host = pa.ancestral_from_rows(m, left, right, t, model, min_posterior=0.5)
        got = multi.ancestral_states(left, right, t, model, min_posterior=0.5)
        assert got.population.size == 99 and got.population.ncols == 2001 and got.sites == 2001
        assert np.array_equal(got.population.read_matrix(), rows) and np.array_equal(rows, host.rows)
        assert np.array_equal(got.population.site_allele_counts(), host_counts(rows))
        assert_close(pa, got, host, m, left, right, t, model)
        assert_close(pa, got, want, m, left, right, t, model, factor=2.0)
        got.close()
        want.close()
    ms = multi.ancestral_states_timing()
    assert len(ms) == 3 and ms[1] > 0.0
    with pytest.raises(pa.PansimError) as e:
        multi.ancestral_states(left, right, t, models_[0].sliced(0, 1000))
    assert e.value.code == PS_ERR_INVALID and "site_classes = 2001, not 1000" in str(e.value)
    multi.close()


def test_site_shards_answer_for_their_own_sites(pa):
    m, left, right, t = case(130, 1000, "random", junk=True)
    model = pa.SubstModel.simulator(rates=(0.3, 1.0, 2.5), site_class=np.random.default_rng(9).integers(0, 3, 1000))
    whole = pa.ancestral_from_rows(m, left, right, t, model)
    cuts = [0, 333, 701, 1000]
    conf = np.zeros(129)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        shard = core_handle(pa, np.ascontiguousarray(m[:, lo:hi]), col_offset=lo, global_cols=1000)
        got = shard.ancestral_states(left, right, t, model.sliced(lo, hi))
        assert got.sites == hi - lo and got.population.ncols == hi - lo and got.population.global_cols == 1000
        assert np.array_equal(got.population.read_matrix(), whole.rows[:, lo:hi])
        conf += got.node_conf
        # the made handle carries the shard's col_offset in the library: a pool refuses parts whose offsets differ
        both = pa.pool([shard, got.population])
        assert np.array_equal(both.read_matrix(), np.vstack([m[:, lo:hi], whole.rows[:, lo:hi]])) and both.global_cols == 1000
        both.close()
        got.close()
        shard.close()
    assert np.all(np.abs(conf - whole.node_conf) <= 4 * 1000 * EPS * whole.node_conf)


def test_the_made_handle_is_a_working_population(pa):
    """core_diversity and tree_parsimony run on it, and a pool of leaves and ancestors gives the parent-child Hamming counts that
    the host counts from the same bytes"""
    import core_diversity_ref
    N, L = 131, 1001
    m, left, right, t = case(N, L, "random", junk=False)
    model = pa.SubstModel.simulator()
    core = core_handle(pa, m)
    got = core.ancestral_states(left, right, t, model, min_posterior=0.4)
    anc = got.population
    rows = anc.read_matrix()
    assert got.masked_cells == int((rows == 0).sum()) and got.masked_cells > 0
    assert core_diversity_ref.same(anc.core_diversity(spectrum=True), core_diversity_ref.of_matrix(rows)) is None
    cat = ref.caterpillar(N - 1)
    dev, host = anc.tree_parsimony(*cat, branches=True), pa.parsimony_from_rows(rows, *cat, branches=True)
    assert dev.total_changes == host.total_changes and np.array_equal(dev.branch_changes, host.branch_changes)
    both = pa.pool([core, anc])
    stacked = both.read_matrix()
    assert both.size == 2 * N - 1 and np.array_equal(stacked, np.vstack([m, rows]))
    child = np.concatenate([left, right]).astype(np.uint32)
    parent = np.concatenate([np.arange(N, 2 * N - 1)] * 2).astype(np.uint32)
    (ham,) = both.pairwise_counts(child, parent)
    # (the core Hamming count of this library is bitwise: the set bits of the XOR, two per pair of unlike bases, one beside a 0)
    assert np.array_equal(ham, bits(stacked[child] ^ stacked[parent]))
    # a one-hot source and nothing masked: the parsimony of the pool takes the one-hot kernels and still equals the host's
    full = core.ancestral_states(left, right, t, model)
    pooled = pa.pool([core, full.population])
    assert np.all(full.population.read_matrix() != 0) and full.masked_cells == 0
    (h2,) = pooled.pairwise_counts(child, parent)
    st = pooled.read_matrix()
    differ = (st[child] != st[parent]).sum(axis=1)
    assert np.array_equal(h2, bits(st[child] ^ st[parent])) and np.array_equal(h2, 2 * differ)
    # the model's expected count of differing branch ends beside the reconstruction's own: the same order of magnitude
    assert 0.2 * full.total_diff < differ.sum() < 5.0 * full.total_diff
    # either order of destruction
    core.close()
    assert np.array_equal(anc.read_matrix(), rows)
    for h in (both, pooled):
        h.close()
    got.close()
    other = core_handle(pa, m)
    late = other.ancestral_states(left, right, t, model)
    late.close()
    assert other.ancestral_states(left, right, t, model, states=False).population is None
    other.close()
    full.close()


def test_without_states_nothing_is_allocated(pa):
    """a matrix of 256 MB: with states=False the device's free memory stays, with states=True it drops by the matrix"""
    import torch
    N, L = 4, 2000000
    rng = np.random.default_rng(8)
    m = np.array(ref.BASES, np.uint8)[rng.integers(0, 4, (N, L))]
    left, right = ref.balanced(N)
    t = np.full(2 * N - 1, 0.1)
    model = pa.SubstModel.simulator()
    core = core_handle(pa, m)
    first = core.ancestral_states(left, right, t, model, states=False)         # (the scratch of the handle is grown here)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    none = core.ancestral_states(left, right, t, model, states=False)
    free1 = torch.cuda.mem_get_info()[0]
    assert none.population is None and abs(free1 - free0) < 16 << 20
    same_bits(first, none)
    some = core.ancestral_states(left, right, t, model)
    free2 = torch.cuda.mem_get_info()[0]
    assert free0 - free2 >= (L * 128) - (16 << 20)
    same_bits(first, some)
    assert np.array_equal(some.population.site_allele_counts().sum(axis=1), np.full(L, 3, np.uint32))
    some.close()
    core.close()


def test_the_scratch_grows_and_timing(pa):
    m, left, right, t = case(500, 300, "balanced", junk=False)
    deep = ref.caterpillar(500, np.random.default_rng(1).permutation(500))
    core = core_handle(pa, m)
    with pytest.raises(pa.PansimError) as e:
        core.ancestral_states_timing()                              # nothing to report yet
    assert e.value.code == PS_ERR_STATE
    one_k, four = pa.SubstModel.simulator(), pa.SubstModel.gamma(0.5, 4, freq=(0.1, 0.2, 0.3, 0.4))
    # (one row of x, then four and the level offsets of the caterpillar, then the small layout again in the grown scratch)
    for (l, r), model in (((left, right), one_k), (deep, four), ((left, right), one_k)):
        got, want = core.ancestral_states(l, r, t, model), pa.ancestral_from_rows(m, l, r, t, model)
        assert np.array_equal(got.population.read_matrix(), want.rows)
        assert_close(pa, got, want, m, l, r, t, model)
        ms = core.ancestral_states_timing()
        assert len(ms) == 3 and ms[0] >= 0.0 and ms[1] > 0.0 and ms[2] > 0.0
        got.close()
    with pytest.raises(pa.PansimError) as e:
        core.tree_model_timing()                                    # the likelihood entry's slots are its own
    assert e.value.code == PS_ERR_STATE
    core.close()


def test_handle_checks(pa):
    rng = np.random.default_rng(6)
    core = core_handle(pa, np.array(ref.BASES, np.uint8)[rng.integers(0, 4, (20, 64))])
    acc = pa.Population(20, 10, 2, False, 0.5, 0, 3)
    left, right = ref.caterpillar(20)
    t = np.full(39, 0.1)
    model = pa.SubstModel.simulator()
    with pytest.raises(pa.PansimError) as e:
        acc.ancestral_states(left, right, t, model)
    assert e.value.code == PS_ERR_INVALID and "core handle" in str(e.value)
    bad = t.copy()
    bad[4] = np.inf
    for l, r, tt, mod, kw, text in ((left[:-1], right[:-1], t[:-1], model, {}, "spanning tree: 19 merges over 20 leaves, not 18"),
                                    (left, right, t, model, dict(min_posterior=1.5), "min_posterior must be a number in [0, 1]"),
                                    (left, right, t, model, dict(min_posterior=np.nan), "min_posterior must be a number in [0, 1]"),
                                    (left, right, bad, model, {}, "length of node 4 is not a finite number"),
                                    ([0] * 19, list(range(1, 20)), t, model, {}, "a child of merge"),
                                    (left, right, t, pa.SubstModel((0.5, 0.5, 0.0, 0.0), root=ROOT), {}, "freq may have at most one zero"),
                                    (left, right, t, pa.SubstModel.simulator(rates=(1.0, 2.0), site_class=np.zeros(63, np.uint8)), {},
                                     "site_classes = 64, not 63")):
        with pytest.raises(pa.PansimError) as e:
            core.ancestral_states(l, r, tt, mod, **kw)
        assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)
    for p in (core, acc):
        p.close()
