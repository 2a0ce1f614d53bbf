"""The Jukes-Cantor likelihood of a tree on the device (ps_tree_likelihood, ps_tree_ml_lengths and their ps_sim / ps_multi forms,
docs/TREE_LIKELIHOOD.md) against the host entries, which tests/test_tree_likelihood.py holds against the sum over all assignments.

Every site's (mantissa, exponent) is the same bits on host and device, and so is every site's r (one header, jc_rule.h): only
the sums over the sites, and log, differ.  The bounds:
  lnL   2^-53 (L + 8) sum_s (|ln l_s| + 2): L roundings of a sum in any order, log within 1 ulp and two operations per site;
  g, h  2 L 2^-53 sum_s |r_s| (resp. r_s^2): the same terms in another order.  The r_s come from the host entry one column at a time.
The shapes are the smallest at which each thing can go wrong: the smallest trees, the lane boundary (64 / 65), a tile that is not
full, the single-wave team against the shared one (1024 / 1025), the largest tree (PS_LIK_MAX_POP) on both sides of the LDS copy of
the schedule (PS_LIK_LDS_SCHED, 156 KiB: with derivatives 2048 leaves have it up to 1028 levels, so a random tree has it and a
caterpillar does not; every shape runs with and without derivatives)."""
import numpy as np
import pytest

import tree_likelihood_ref as ref

pytestmark = pytest.mark.gpu

PS_ERR_INVALID, PS_ERR_STATE = -1, -6
EPS = 2.0 ** -53
SHAPES = [(2, 1, "caterpillar"), (4, 1, "random"), (5, 7, "caterpillar"), (64, 16, "balanced"), (65, 17, "caterpillar"), (1000, 203, "random"),
          (1024, 32, "balanced"), (1025, 32, "random"), (1500, 8, "balanced"), (2048, 8, "random"), (2048, 5, "caterpillar")]


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


def site_ratios(pa, m, left, right, t):
    """(L, nodes): r of every site and branch, from the host entry one column at a time (each g of one site is its r)"""
    return np.stack([pa.likelihood_from_rows(np.ascontiguousarray(m[:, s:s + 1]), left, right, t, per_site=False).branch_g
                     for s in range(m.shape[1])])


def assert_close(got, want, r, L):
    """a device result against the host's, `r` the (L, nodes) ratios of the same sites"""
    assert np.array_equal(got.site_mant, want.site_mant) and np.array_equal(got.site_exp, want.site_exp)
    bound = EPS * (L + 8) * (np.abs(want.site_lnl) + 2.0).sum()
    print("lnl", got.lnl, want.lnl, abs(got.lnl - want.lnl), bound)
    assert abs(got.lnl - want.lnl) <= bound
    for name in ("pop_size", "sites", "merges", "clamped_lengths", "missing_cells", "rounds", "passes", "rollbacks"):
        assert getattr(got, name) == getattr(want, name), name
    assert got.tree_length == want.tree_length and got.start_lnl == got.lnl
    bg, bh = 2 * L * EPS * np.abs(r).sum(axis=0), 2 * L * EPS * (r * r).sum(axis=0)
    print("g", np.abs(got.branch_g - want.branch_g).max(), bg.max(), "h", np.abs(got.branch_h - want.branch_h).max(), bh.max())
    assert np.all(np.abs(got.branch_g - want.branch_g) <= bg) and np.all(np.abs(got.branch_h - want.branch_h) <= bh)


@pytest.mark.parametrize("k,N,L,kind", [(k,) + s for k, s in enumerate(SHAPES)])
def test_device_equals_host(pa, k, N, L, kind):
    """arbitrary bytes on every second shape; the up pass alone and with the down pass; a second call gives the same bits"""
    m, left, right, t = case(N, L, kind, junk=k % 2 == 1)
    core = core_handle(pa, m)
    want = pa.likelihood_from_rows(m, left, right, t)
    got = core.tree_likelihood(left, right, t, per_site=True, derivatives=True)
    assert_close(got, want, site_ratios(pa, m, left, right, t), L)
    assert got.clamped_lengths >= 1
    again = core.tree_likelihood(left, right, t, per_site=True, derivatives=True)
    for name in ("site_mant", "site_exp", "branch_g", "branch_h"):
        assert np.array_equal(getattr(got, name), getattr(again, name)), name
    assert again.lnl == got.lnl
    up = core.tree_likelihood(left, right, t, per_site=True)
    assert up.branch_g is None and np.array_equal(up.site_mant, want.site_mant) and np.array_equal(up.site_exp, want.site_exp)
    assert abs(up.lnl - want.lnl) <= EPS * (L + 8) * (np.abs(want.site_lnl) + 2.0).sum()
    assert core.tree_likelihood(left, right, t).lnl == up.lnl and up.missing_cells == want.missing_cells
    core.close()


def test_ml_lengths_on_the_device(pa):
    rng = np.random.default_rng(21)
    N, L = 130, 1001
    left, right = ref.random_tree(N, rng)
    truth = rng.uniform(0.01, 0.3, 2 * N - 1)
    m = ref.evolve(left, right, truth, N, L, rng)
    core = core_handle(pa, m)
    got = core.tree_ml_lengths(left, right, np.full(2 * N - 1, 0.1), max_rounds=12)
    assert got.rounds >= 2 and got.passes >= got.rounds + got.rollbacks + 1 and got.round_lnl.size == got.rounds + 1
    assert np.all(np.diff(got.round_lnl) > 0) and got.lnl >= got.start_lnl and got.lnl == got.round_lnl[-1]
    assert got.lengths[int(right[-1])] == 1e-8 and got.lengths[-1] == 0.0 and got.sites == L
    host = pa.likelihood_from_rows(m, left, right, got.lengths)
    bound = EPS * (L + 8) * (np.abs(host.site_lnl) + 2.0).sum()
    print("ml lnl", got.lnl, host.lnl, abs(got.lnl - host.lnl), bound)
    assert abs(got.lnl - host.lnl) <= bound
    # default start lengths: the Jukes-Cantor correction of the parsimony changes
    auto = core.tree_ml_lengths(left, right, max_rounds=3)
    p = core.tree_parsimony(left, right, branches=True)
    start = pa.jc_lengths_from_changes(p.branch_changes, L)
    assert auto.start_lnl == core.tree_ml_lengths(left, right, start, max_rounds=3).start_lnl and auto.lnl >= auto.start_lnl
    core.close()


SIM = dict(pop_size=100, core_size=2001, pan_genes=300, core_genes=20, HR_rate=0.5, HGT_rate=0.5, seed=11, n_gen=8, max_distances=100)


def test_a_simulation_and_no_change_of_state(pa):
    """the neighbour-joining tree of a short run with default start lengths: leaves are rows of the reference's row order while the
    matrix is stored in another; the run continues as if it had not been asked"""
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(6)
    left, right = sim.neighbour_joining().merges()[:2]
    assert (np.diff(sim.last_parents().astype(np.int64)) < 0).any()                    # the internal order is not the output order
    m = sim.core_genome.read_matrix()
    got = sim.tree_ml_lengths(left, right)
    assert got.pop_size == 100 and got.sites == 2001 and got.rounds >= 1 and got.lnl >= got.start_lnl and np.all(np.diff(got.round_lnl) > 0)
    host = pa.likelihood_from_rows(m, left, right, got.lengths)
    assert abs(got.lnl - host.lnl) <= EPS * (2001 + 8) * (np.abs(host.site_lnl) + 2.0).sum()
    one = sim.tree_likelihood(left, right, got.lengths, per_site=True, derivatives=True)
    assert_close(one, host, site_ratios(pa, m, left, right, got.lengths), 2001)
    ms = sim.tree_likelihood_timing()
    assert len(ms) == 3 and ms[0] >= 0.0 and ms[1] > 0.0 and ms[2] > 0.0
    assert got.newick().count(":") == 198
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
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(5)
    left, right = sim.upgma_tree().merges()
    m = sim.core_genome.read_matrix()
    t = np.random.default_rng(shards).uniform(0.001, 0.05, 199)
    want = sim.tree_likelihood(left, right, t, per_site=True, derivatives=True)
    want_ml = sim.tree_ml_lengths(left, right, t, max_rounds=2)
    sim.close()
    multi = pa.MultiSimulation(pa.make_params(**SIM), shards, devices=[0] * shards)
    multi.run(5)
    got = multi.tree_likelihood(left, right, t, per_site=True, derivatives=True)
    r = site_ratios(pa, m, left, right, t)
    assert_close(got, pa.likelihood_from_rows(m, left, right, t), r, 2001)
    assert np.array_equal(got.site_mant, want.site_mant) and np.array_equal(got.site_exp, want.site_exp)
    # against the unsharded handle: two sums of the same terms, each within its bound of the host's
    assert abs(got.lnl - want.lnl) <= 2 * EPS * (2001 + 8) * (np.abs(want.site_lnl) + 2.0).sum()
    assert np.all(np.abs(got.branch_g - want.branch_g) <= 4 * 2001 * EPS * np.abs(r).sum(axis=0))
    got_ml = multi.tree_ml_lengths(left, right, t, max_rounds=2)
    assert got_ml.sites == 2001 and got_ml.rounds == want_ml.rounds and np.allclose(got_ml.lengths, want_ml.lengths, rtol=1e-9, atol=0)
    assert np.allclose(got_ml.round_lnl, want_ml.round_lnl, rtol=1e-12, atol=0)
    ms = multi.tree_likelihood_timing()
    assert len(ms) == 3 and ms[1] > 0.0
    multi.close()


def test_site_shards_answer_for_their_own_sites(pa):
    m, left, right, t = case(130, 1000, "random", junk=True)
    whole = pa.likelihood_from_rows(m, left, right, t)
    cuts = [0, 333, 701, 1000]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        shard = core_handle(pa, np.ascontiguousarray(m[:, lo:hi]), col_offset=lo, global_cols=1000)
        got = shard.tree_likelihood(left, right, t, per_site=True)
        assert got.sites == hi - lo and np.array_equal(got.site_mant, whole.site_mant[lo:hi]) and np.array_equal(got.site_exp, whole.site_exp[lo:hi])
        shard.close()


def test_the_scratch_grows_and_timing(pa):
    m, left, right, t = case(500, 300, "balanced", junk=False)
    deep = ref.caterpillar(500, np.random.default_rng(1).permutation(500))
    core = core_handle(pa, m)
    with pytest.raises(pa.PansimError) as e:
        core.tree_likelihood_timing()                               # nothing to report yet
    assert e.value.code == PS_ERR_STATE
    # (up alone, then with the sums of every workgroup, then the level offsets of the caterpillar: each needs more scratch)
    for (l, r), kw in (((left, right), {}), ((left, right), dict(derivatives=True)), (deep, dict(derivatives=True, per_site=True)),
                       ((left, right), {})):
        got, want = core.tree_likelihood(l, r, t, **kw), pa.likelihood_from_rows(m, l, r, t)
        assert abs(got.lnl - want.lnl) <= EPS * (300 + 8) * (np.abs(want.site_lnl) + 2.0).sum()
        ms = core.tree_likelihood_timing()
        assert len(ms) == 3 and ms[0] >= 0.0 and ms[1] > 0.0 and ms[2] > 0.0
    one = core.tree_likelihood_timing()[1]
    got = core.tree_ml_lengths(left, right, t, max_rounds=3)
    assert got.passes >= 3 and core.tree_likelihood_timing()[1] > one       # the sum over the passes of the call
    core.close()


def test_handle_checks(pa):
    rng = np.random.default_rng(6)
    core = core_handle(pa, np.array(ref.BASES, np.uint8)[rng.integers(0, 4, (20, 64))])
    acc = pa.Population(20, 10, 2, False, 0.5, 0, 3)
    left, right = ref.caterpillar(20)
    t = np.full(39, 0.1)
    for call in (lambda: acc.tree_likelihood(left, right, t), lambda: acc.tree_ml_lengths(left, right, t)):
        with pytest.raises(pa.PansimError) as e:
            call()
        assert e.value.code == PS_ERR_INVALID and "core handle" in str(e.value)
    bad = t.copy()
    bad[4] = np.inf
    for l, r, tt, kw, text in ((left[:-1], right[:-1], t[:-1], {}, "spanning tree: 19 merges over 20 leaves, not 18"),
                               (left, right, t, dict(max_rounds=0), "max_rounds must be at least 1"),
                               (left, right, t, dict(eps_lnl=-1.0), "eps_lnl must be a positive number"),
                               (left, right, bad, {}, "length of node 4 is not a finite number"),
                               ([0] * 19, list(range(1, 20)), t, {}, "a child of merge")):
        with pytest.raises(pa.PansimError) as e:
            core.tree_ml_lengths(l, r, tt, **kw)
        assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)
    with pytest.raises(pa.PansimError) as e:
        core.tree_likelihood(left, right, bad)
    assert e.value.code == PS_ERR_INVALID and "not a finite number" in str(e.value)
    big = pa.Population(2049, 16, 4, True, 0.0, 0, 0)
    with pytest.raises(pa.PansimError) as e:
        big.tree_likelihood(*ref.caterpillar(2049), np.full(4097, 0.1))
    assert e.value.code == PS_ERR_INVALID and "pop_size <= 2048" in str(e.value)
    for p in (core, acc, big):
        p.close()
