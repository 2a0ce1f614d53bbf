"""The likelihood of a tree under F81 with a root distribution and rate categories on the device (ps_tree_model_likelihood,
ps_tree_model_ml_lengths and their ps_sim / ps_multi forms, docs/TREE_MODEL.md) against the host entries, which
tests/test_tree_model.py holds against the sum over all assignments.

Every site's (mantissa, exponent), posterior mean rate and derivative terms are the same bits on host and device (one header,
subst_rule.h): only the sums over the sites, and log, differ.  The bounds:
  lnL      2^-53 (L + 8) sum_s (|ln l_s| + 2): L roundings of a sum in any order, log within 1 ulp and two operations per site;
  g, h, q  2 L K 2^-53 times the sum of the absolute values of their terms (D_sc, D_sc^2, and post_sk r_k (r_k x_ck ratio_sck)
           per site AND category: q is added per category): the same L K terms at the most in another order.  The terms come
           from the host entry one column at a time, q's per category from the host entry with that category assigned and the
           posterior formed here from the categories' (mantissa, exponent).
The shapes are the smallest at which each thing can go wrong: the smallest trees, the lane boundary (64 / 65), a tile that is not
full (L = 17), the single-wave team against the shared one (1024 / 1025), the largest tree with derivatives
(PS_MODEL_MAX_POP_DERIV, random: 159 712 bytes of LDS; a caterpillar: the deepest schedule) and the largest tree at all (2048, the
up pass only).  Each runs with K = 1, a K = 4 mixture and K = 8 assigned classes; every second shape holds arbitrary bytes."""
import numpy as np
import pytest

import tree_likelihood_ref as ref

pytestmark = pytest.mark.gpu

PS_ERR_INVALID, PS_ERR_STATE = -1, -6
EPS = 2.0 ** -53
MAXD = 1536
SHAPES = [(2, 1, "caterpillar"), (5, 7, "caterpillar"), (64, 16, "balanced"), (65, 17, "caterpillar"), (1000, 12, "random"),
          (1024, 8, "balanced"), (1025, 8, "random"), (MAXD, 8, "random"), (MAXD, 5, "caterpillar"), (2048, 8, "random")]
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
    rng = np.random.default_rng(L)
    return [pa.SubstModel.simulator(),
            pa.SubstModel((0.1, 0.2, 0.3, 0.4), root=ROOT, rates=(0.0, 0.4, 1.0, 2.6), weights=(0.1, 0.4, 0.3, 0.2)),
            pa.SubstModel.simulator(rates=(0.1, 0.3, 0.6, 1.0, 1.5, 2.0, 3.0, 5.0), site_class=rng.integers(0, 8, L))]


def host_terms(pa, m, left, right, t, model, want):
    """((L, nodes) D_sc, (L, nodes) sum_k |q_sck|) from the host entry one column at a time; `want`: the host's result over m"""
    L, K = m.shape[1], model.categories
    cols = [np.ascontiguousarray(m[:, s:s + 1]) for s in range(L)]
    one = [pa.model_likelihood_from_rows(cols[s], left, right, t, model.sliced(s, s + 1), per_site=False) for s in range(L)]
    D = np.stack([r.branch_g for r in one])
    if model.site_class is not None or K == 1:
        return D, np.abs(np.stack([r.branch_q for r in one]))
    qabs = np.zeros_like(D)
    for k in range(K):
        alone = pa.SubstModel(model.freq, model.root, model.rates, model.weights, np.full(L, k, np.uint8))
        cat = pa.model_likelihood_from_rows(m, left, right, t, alone, derivatives=False)
        shift = np.where(cat.site_mant > 0, cat.site_exp - want.site_exp, 0)
        post = model.weights[k] * np.ldexp(cat.site_mant, shift) / want.site_mant
        for s in range(L):
            q = pa.model_likelihood_from_rows(cols[s], left, right, t, alone.sliced(s, s + 1), per_site=False).branch_q
            qabs[s] += post[s] * np.abs(q)
    return D, qabs


def assert_close(got, want, D, qabs, L, K):
    """a device result against the host's"""
    for name in ("site_mant", "site_exp", "site_rate"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    bound = EPS * (L + 8) * (np.abs(want.site_lnl) + 2.0).sum()
    print("lnl", got.lnl, want.lnl, abs(got.lnl - want.lnl), bound)
    assert abs(got.lnl - want.lnl) <= bound
    for name in ("pop_size", "sites", "merges", "clamped_lengths", "missing_cells", "rounds", "passes", "rollbacks", "categories", "classed"):
        assert getattr(got, name) == getattr(want, name), name
    assert got.tree_length == want.tree_length and got.start_lnl == got.lnl and got.beta == want.beta and got.mean_rate == want.mean_rate
    f = 2 * L * K * EPS
    for name, terms in (("branch_g", np.abs(D)), ("branch_h", D * D), ("branch_q", qabs)):
        err, bd = np.abs(getattr(got, name) - getattr(want, name)), f * terms.sum(axis=0)
        print(name, err.max(), bd.max())
        assert np.all(err <= bd), name


@pytest.mark.parametrize("k,N,L,kind", [(k,) + s for k, s in enumerate(SHAPES)])
def test_device_equals_host(pa, k, N, L, kind):
    """arbitrary bytes on every second shape; the up pass alone and with the down pass; a second call gives the same bits"""
    m, left, right, t = case(N, L, kind, junk=k % 2 == 1)
    core = core_handle(pa, m)
    for model in models(pa, L):
        K = model.categories
        if N > MAXD:
            with pytest.raises(pa.PansimError) as e:
                core.tree_model_likelihood(left, right, t, model, derivatives=True)
            assert e.value.code == PS_ERR_INVALID and "PS_MODEL_MAX_POP_DERIV = 1536" in str(e.value)
            want = pa.model_likelihood_from_rows(m, left, right, t, model, derivatives=False)
        else:
            want = pa.model_likelihood_from_rows(m, left, right, t, model)
            got = core.tree_model_likelihood(left, right, t, model, per_site=True, derivatives=True)
            assert_close(got, want, *host_terms(pa, m, left, right, t, model, want), L, K)
            assert got.clamped_lengths >= 1
            again = core.tree_model_likelihood(left, right, t, model, per_site=True, derivatives=True)
            for name in ("site_mant", "site_exp", "site_rate", "branch_g", "branch_h", "branch_q"):
                assert np.array_equal(getattr(got, name), getattr(again, name)), name
            assert again.lnl == got.lnl
        up = core.tree_model_likelihood(left, right, t, model, per_site=True)
        assert up.branch_g is None and up.branch_q is None
        for name in ("site_mant", "site_exp", "site_rate"):
            assert np.array_equal(getattr(up, name), getattr(want, name)), name
        assert abs(up.lnl - want.lnl) <= EPS * (L + 8) * (np.abs(want.site_lnl) + 2.0).sum()
        assert core.tree_model_likelihood(left, right, t, model).lnl == up.lnl and up.missing_cells == want.missing_cells
    core.close()


@pytest.mark.parametrize("N,L,kind,junk", [(65, 17, "caterpillar", True), (1025, 8, "random", False)])
def test_the_jc69_anchor_on_the_device(pa, N, L, kind, junk):
    m, left, right, t = case(N, L, kind, junk)
    core = core_handle(pa, m)
    jc = core.tree_likelihood(left, right, t, per_site=True, derivatives=True)
    got = core.tree_model_likelihood(left, right, t, pa.SubstModel.jc69(), per_site=True, derivatives=True)
    assert np.array_equal(got.site_mant, jc.site_mant) and np.array_equal(got.site_exp, jc.site_exp) and got.lnl == jc.lnl
    assert got.missing_cells == jc.missing_cells and np.all(got.site_rate == 1.0)
    # the same derivatives, x inside the sum instead of outside: each within the rounding bound of its L terms
    r = np.stack([pa.likelihood_from_rows(np.ascontiguousarray(m[:, s:s + 1]), left, right, t, per_site=False).branch_g for s in range(L)])
    x = np.exp(-4.0 * jc.used_lengths() / 3.0)
    assert np.all(np.abs(got.gradient() - jc.gradient()) <= 4 * L * EPS * (4 * x / 3) * np.abs(r).sum(axis=0))
    assert np.all(np.abs(got.curvature() - jc.curvature()) <= 4 * L * EPS * ((16 * x * x / 9) * (r * r).sum(axis=0) + (16 * x / 9) * np.abs(r).sum(axis=0)))
    core.close()


def test_ml_lengths_on_the_device(pa):
    rng = np.random.default_rng(21)
    N, L = 130, 1001
    left, right = ref.random_tree(N, rng)
    truth = rng.uniform(0.01, 0.3, 2 * N - 1)
    m = ref.evolve(left, right, truth, N, L, rng)
    model = pa.SubstModel.simulator(rates=(0.5, 2.0), site_class=rng.integers(0, 2, L))
    core = core_handle(pa, m)
    got = core.tree_model_ml_lengths(left, right, model, np.full(2 * N - 1, 0.1), max_rounds=12)
    assert got.rounds >= 2 and got.passes >= got.rounds + got.rollbacks + 1 and got.round_lnl.size == got.rounds + 1
    assert np.all(np.diff(got.round_lnl) > 0) and got.lnl >= got.start_lnl and got.lnl == got.round_lnl[-1]
    # rho != pi: both root branches are estimated
    assert got.lengths[int(right[-1])] != 1e-8 and got.lengths[-1] == 0.0 and got.sites == L and got.classed and got.categories == 2
    host = pa.model_likelihood_from_rows(m, left, right, got.lengths, model)
    bound = EPS * (L + 8) * (np.abs(host.site_lnl) + 2.0).sum()
    print("ml lnl", got.lnl, host.lnl, abs(got.lnl - host.lnl), bound)
    assert abs(got.lnl - host.lnl) <= bound
    rev = core.tree_model_ml_lengths(left, right, pa.SubstModel.gamma(0.7, 4), np.full(2 * N - 1, 0.1), max_rounds=2)
    assert rev.lengths[int(right[-1])] == 1e-8 and rev.rounds >= 1 and np.all(np.diff(rev.round_lnl) > 0)
    # default start lengths: the F81 correction of the parsimony changes
    auto = core.tree_model_ml_lengths(left, right, model, max_rounds=3)
    p = core.tree_parsimony(left, right, branches=True)
    start = pa.f81_lengths_from_changes(p.branch_changes, L, model.freq)
    assert auto.start_lnl == core.tree_model_ml_lengths(left, right, model, start, max_rounds=3).start_lnl and auto.lnl >= auto.start_lnl
    core.close()


SIM = dict(pop_size=100, core_size=2001, pan_genes=300, core_genes=20, HR_rate=0.5, HGT_rate=0.5, seed=11, n_gen=8, max_distances=100)


def test_a_simulation_and_no_change_of_state(pa):
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(6)
    left, right = sim.neighbour_joining().merges()[:2]
    m = sim.core_genome.read_matrix()
    model = pa.SubstModel.simulator()
    got = sim.tree_model_ml_lengths(left, right, model)
    assert got.pop_size == 100 and got.sites == 2001 and got.rounds >= 1 and got.lnl >= got.start_lnl and np.all(np.diff(got.round_lnl) > 0)
    host = pa.model_likelihood_from_rows(m, left, right, got.lengths, model)
    assert abs(got.lnl - host.lnl) <= EPS * (2001 + 8) * (np.abs(host.site_lnl) + 2.0).sum()
    one = sim.tree_model_likelihood(left, right, got.lengths, model, per_site=True, derivatives=True)
    assert_close(one, host, *host_terms(pa, m, left, right, got.lengths, model, host), 2001, 1)
    ms = sim.tree_model_timing()
    assert len(ms) == 3 and ms[0] >= 0.0 and ms[1] > 0.0 and ms[2] > 0.0
    assert got.newick().count(":") == 198 and np.allclose(got.events(), got.lengths * 1.5)
    assert np.array_equal(sim.core_genome.read_matrix(), m)
    sim.run(2)
    plain = pa.Simulation(pa.make_params(**SIM))
    plain.run(8)
    assert np.array_equal(plain.core_genome.read_matrix(), sim.core_genome.read_matrix())
    assert np.array_equal(plain.pan_genome.read_matrix(), sim.pan_genome.read_matrix())
    plain.close()
    sim.close()


@pytest.mark.parametrize("shards", [2, 3])
def test_multi_simulation_against_the_unsharded_run(pa, shards):
    """site_class is indexed by the global site: every shard takes its own slice"""
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(5)
    left, right = sim.upgma_tree().merges()
    m = sim.core_genome.read_matrix()
    rng = np.random.default_rng(shards)
    t = rng.uniform(0.001, 0.05, 199)
    model = pa.SubstModel.simulator(rates=(0.3, 1.0, 2.5), site_class=rng.integers(0, 3, 2001))
    mixture = pa.SubstModel.simulator(rates=(0.3, 1.0, 2.5), weights=(0.3, 0.4, 0.3))
    want = sim.tree_model_likelihood(left, right, t, model, per_site=True, derivatives=True)
    want_ml = sim.tree_model_ml_lengths(left, right, model, t, max_rounds=2)
    sim.close()
    multi = pa.MultiSimulation(pa.make_params(**SIM), shards, devices=[0] * shards)
    multi.run(5)
    host = pa.model_likelihood_from_rows(m, left, right, t, model)
    D, qabs = host_terms(pa, m, left, right, t, model, host)
    got = multi.tree_model_likelihood(left, right, t, model, per_site=True, derivatives=True)
    assert_close(got, host, D, qabs, 2001, 3)
    for name in ("site_mant", "site_exp", "site_rate"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    # against the unsharded handle: two sums of the same terms, each within its bound of the host's
    assert abs(got.lnl - want.lnl) <= 2 * EPS * (2001 + 8) * (np.abs(want.site_lnl) + 2.0).sum()
    assert np.all(np.abs(got.branch_g - want.branch_g) <= 4 * 2001 * 3 * EPS * np.abs(D).sum(axis=0))
    mix = multi.tree_model_likelihood(left, right, t, mixture, per_site=True)
    mix_host = pa.model_likelihood_from_rows(m, left, right, t, mixture, derivatives=False)
    assert np.array_equal(mix.site_mant, mix_host.site_mant) and np.array_equal(mix.site_rate, mix_host.site_rate) and not mix.classed
    got_ml = multi.tree_model_ml_lengths(left, right, model, t, max_rounds=2)
    assert got_ml.sites == 2001 and got_ml.rounds == want_ml.rounds and np.allclose(got_ml.lengths, want_ml.lengths, rtol=1e-9, atol=0)
    assert np.allclose(got_ml.round_lnl, want_ml.round_lnl, rtol=1e-12, atol=0)
    ms = multi.tree_model_timing()
    assert len(ms) == 3 and ms[1] > 0.0
    with pytest.raises(pa.PansimError) as e:
        multi.tree_model_likelihood(left, right, t, model.sliced(0, 1000))
    assert e.value.code == PS_ERR_INVALID and "site_classes = 2001, not 1000" in str(e.value)
    multi.close()


def test_site_shards_answer_for_their_own_sites(pa):
    m, left, right, t = case(130, 1000, "random", junk=True)
    model = pa.SubstModel.simulator(rates=(0.3, 1.0, 2.5), site_class=np.random.default_rng(9).integers(0, 3, 1000))
    whole = pa.model_likelihood_from_rows(m, left, right, t, model, derivatives=False)
    cuts = [0, 333, 701, 1000]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        shard = core_handle(pa, np.ascontiguousarray(m[:, lo:hi]), col_offset=lo, global_cols=1000)
        got = shard.tree_model_likelihood(left, right, t, model.sliced(lo, hi), per_site=True)
        assert got.sites == hi - lo
        for name in ("site_mant", "site_exp", "site_rate"):
            assert np.array_equal(getattr(got, name), getattr(whole, name)[lo:hi]), name
        shard.close()


def test_the_scratch_grows_and_timing(pa):
    m, left, right, t = case(500, 300, "balanced", junk=False)
    deep = ref.caterpillar(500, np.random.default_rng(1).permutation(500))
    core = core_handle(pa, m)
    with pytest.raises(pa.PansimError) as e:
        core.tree_model_timing()                                    # nothing to report yet
    assert e.value.code == PS_ERR_STATE
    one_k, four = pa.SubstModel.simulator(), pa.SubstModel.gamma(0.5, 4, freq=(0.1, 0.2, 0.3, 0.4))
    # (up alone, then the sums of every workgroup, then four rows of x and the level offsets of the caterpillar: each needs more)
    for (l, r), model, kw in (((left, right), one_k, {}), ((left, right), one_k, dict(derivatives=True)),
                              (deep, four, dict(derivatives=True, per_site=True)), ((left, right), one_k, {})):
        got, want = core.tree_model_likelihood(l, r, t, model, **kw), pa.model_likelihood_from_rows(m, l, r, t, model, derivatives=False)
        assert abs(got.lnl - want.lnl) <= EPS * (300 + 8) * (np.abs(want.site_lnl) + 2.0).sum()
        ms = core.tree_model_timing()
        assert len(ms) == 3 and ms[0] >= 0.0 and ms[1] > 0.0 and ms[2] > 0.0
    with pytest.raises(pa.PansimError) as e:
        core.tree_likelihood_timing()                               # the JC69 entry's slots are its own
    assert e.value.code == PS_ERR_STATE
    one = core.tree_model_timing()[1]
    got = core.tree_model_ml_lengths(left, right, one_k, t, max_rounds=3)
    assert got.passes >= 3 and core.tree_model_timing()[1] > one    # the sum over the passes of the call
    core.close()


def test_handle_checks(pa):
    rng = np.random.default_rng(6)
    core = core_handle(pa, np.array(ref.BASES, np.uint8)[rng.integers(0, 4, (20, 64))])
    acc = pa.Population(20, 10, 2, False, 0.5, 0, 3)
    left, right = ref.caterpillar(20)
    t = np.full(39, 0.1)
    model = pa.SubstModel.simulator()
    for call in (lambda: acc.tree_model_likelihood(left, right, t, model), lambda: acc.tree_model_ml_lengths(left, right, model, t)):
        with pytest.raises(pa.PansimError) as e:
            call()
        assert e.value.code == PS_ERR_INVALID and "core handle" in str(e.value)
    bad = t.copy()
    bad[4] = np.inf
    for l, r, tt, mod, kw, text in ((left[:-1], right[:-1], t[:-1], model, {}, "spanning tree: 19 merges over 20 leaves, not 18"),
                                    (left, right, t, model, dict(max_rounds=0), "max_rounds must be at least 1"),
                                    (left, right, t, model, dict(eps_lnl=-1.0), "eps_lnl must be a positive number"),
                                    (left, right, bad, model, {}, "length of node 4 is not a finite number"),
                                    ([0] * 19, list(range(1, 20)), t, model, {}, "a child of merge"),
                                    (left, right, t, pa.SubstModel((0.5, 0.5, 0.0, 0.0), root=ROOT), {}, "freq may have at most one zero"),
                                    (left, right, t, pa.SubstModel.simulator(rates=(1.0, 2.0), site_class=np.zeros(63, np.uint8)), {},
                                     "site_classes = 64, not 63"),
                                    (left, right, t, pa.SubstModel.simulator(rates=(1.0, 2.0), site_class=np.full(64, 2, np.uint8)), {},
                                     "site_class[0] = 2 is not below categories = 2")):
        with pytest.raises(pa.PansimError) as e:
            core.tree_model_ml_lengths(l, r, mod, tt, **kw)
        assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)
    with pytest.raises(pa.PansimError) as e:
        core.tree_model_likelihood(left, right, bad, model)
    assert e.value.code == PS_ERR_INVALID and "not a finite number" in str(e.value)
    big = pa.Population(2049, 16, 4, True, 0.0, 0, 0)
    with pytest.raises(pa.PansimError) as e:
        big.tree_model_likelihood(*ref.caterpillar(2049), np.full(4097, 0.1), model)
    assert e.value.code == PS_ERR_INVALID and "pop_size <= 2048" in str(e.value)
    mid = pa.Population(MAXD + 1, 16, 4, True, 0.0, 0, 0)
    with pytest.raises(pa.PansimError) as e:
        mid.tree_model_ml_lengths(*ref.caterpillar(MAXD + 1), model, np.full(2 * MAXD + 1, 0.1))
    assert e.value.code == PS_ERR_INVALID and "PS_MODEL_MAX_POP_DERIV = 1536" in str(e.value)
    for p in (core, acc, big, mid):
        p.close()
