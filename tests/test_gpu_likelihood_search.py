"""The likelihood tree search on the device (ps_tree_model_nni_deltas, ps_tree_model_nni and their ps_sim / ps_multi forms,
docs/LIKELIHOOD_SEARCH.md) against the host entries, which tests/test_likelihood_search.py holds against rescoring every
neighbour tree from scratch.

Every site ratio is the same bits on host and device (one header, subst_rule.h): only the grouping of at most L + workgroups +
shards rounded multiplications, the log and the exponent term differ.  The bounds:
  lnL    2^-53 (L + 8) sum_s (|ln l_s| + 2), as tests/test_gpu_tree_model.py;
  gain   2^-52 (2 L + 16) + 2^-50 |gain of the host|.
The shapes: the smallest trees (4: the root's edge alone; 5), a tile that is not full, the lane boundary (64 / 65), levels wider
than the wave (256 balanced), the deepest and the widest schedule at the limit (1024 caterpillar / balanced), the limit itself with
a random tree, one leaf more (refused), and more tiles than workgroups (64 x 20 000).  The kernel has no other switch: at every
N <= PS_MODEL_NNI_MAX_POP the schedule's copy fits the LDS (155 644 bytes at the most, 159 744 allowed) and the team is one wave.
Each runs with JC69, the simulator's law, K = 3 assigned classes and a K = 4 mixture with an invariant category; every second
shape holds arbitrary bytes."""
import numpy as np
import pytest

import tree_likelihood_ref as ref

pytestmark = pytest.mark.gpu

PS_ERR_INVALID, PS_ERR_STATE = -1, -6
EPS = 2.0 ** -53
MAXN = 1024
SHAPES = [(4, 1, "balanced"), (5, 3, "caterpillar"), (17, 6, "random"), (64, 9, "random"), (65, 5, "caterpillar"), (256, 7, "balanced"),
          (1024, 5, "caterpillar"), (1024, 8, "balanced"), (MAXN, 5, "random"), (64, 20000, "random")]
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
    rng = np.random.default_rng(N * 37 + L)
    left, right = tree_of(rng, N, kind)
    t = rng.uniform(0.005, 0.3, 2 * N - 1)
    t[rng.integers(0, 2 * N - 1, 3)] = [0.0, -0.5, 40.0]              # entries across both clamp bounds
    m = ref.evolve(left, right, t, N, L, rng)
    if junk:
        m[rng.random(m.shape) < 0.03] = rng.integers(0, 256, 1, dtype=np.uint8)[0]
        m[0, 0], m[1 % N, L - 1] = 0, 255
    if L >= 16:
        m[:, 8:12] = 4                                                  # a fully monomorphic tile
    return m, left, right, t


def models(pa, L):
    rng = np.random.default_rng(L)
    return [pa.SubstModel.jc69(), pa.SubstModel.simulator(),
            pa.SubstModel((0.1, 0.2, 0.3, 0.4), root=ROOT, rates=(0.3, 1.0, 2.5), site_class=rng.integers(0, 3, L)),
            pa.SubstModel.simulator(rates=(0.0, 0.4, 1.0, 2.6), weights=(0.1, 0.4, 0.3, 0.2))]


def assert_deltas(got, want, site_lnl, L, what=""):
    """a device pass against the host's"""
    bound = EPS * (L + 8) * (np.abs(site_lnl) + 2.0).sum()
    print(what, "lnl", got.lnl, want.lnl, abs(got.lnl - want.lnl), bound)
    assert abs(got.lnl - want.lnl) <= bound
    assert got.zero_sites == want.zero_sites == 0
    assert np.array_equal(np.isnan(got.delta), np.isnan(want.delta)) and np.array_equal(got.delta_mant == 0.0, np.isnan(want.delta))
    assert np.all((got.delta_mant == 0.0) | ((got.delta_mant >= 0.5) & (got.delta_mant < 1.0)))
    some = ~np.isnan(want.delta)
    err, bd = np.abs(got.delta - want.delta)[some], (2 * EPS * (2 * L + 16) + 8 * EPS * np.abs(want.delta))[some]
    if err.size:
        print(what, "gains", err.max(), bd.min(), float(np.abs(want.delta[some]).max()))
    assert np.all(err <= bd)


@pytest.mark.parametrize("k,N,L,kind", [(k,) + s for k, s in enumerate(SHAPES)])
def test_device_pass_equals_host(pa, k, N, L, kind):
    """clean data on every even shape, arbitrary bytes on every odd one; a second call returns the first call's bits"""
    m, left, right, t = case(N, L, kind, junk=k % 2 == 1)
    core = core_handle(pa, m)
    for i, model in enumerate(models(pa, L)):
        want = pa.model_nni_deltas_from_rows(m, left, right, t, model)
        site = pa.model_likelihood_from_rows(m, left, right, t, model, derivatives=False).site_lnl
        got = core.model_nni_deltas(left, right, t, model)
        assert_deltas(got, want, site, L, "model %d" % i)
        assert (~np.isnan(got.delta)).sum() == 2 * (N - 3)
        again = core.model_nni_deltas(left, right, t, model)
        assert again.lnl == got.lnl and np.array_equal(again.delta_mant, got.delta_mant) and np.array_equal(again.delta_exp, got.delta_exp)
    core.close()


def test_one_leaf_above_the_limit_is_refused(pa):
    N = pa.PS_MODEL_NNI_MAX_POP + 1
    assert pa.PS_MODEL_NNI_MAX_POP == MAXN
    big = pa.Population(N, 16, 4, True, 0.0, 0, 0)
    left, right = ref.caterpillar(N)
    for call in (lambda: big.model_nni_deltas(left, right, np.full(2 * N - 1, 0.1), pa.SubstModel.simulator()),
                 lambda: big.tree_model_nni(left, right, pa.SubstModel.simulator(), np.full(2 * N - 1, 0.1))):
        with pytest.raises(pa.PansimError) as e:
            call()
        assert e.value.code == PS_ERR_INVALID and "PS_MODEL_NNI_MAX_POP = 1024" in str(e.value)
    big.close()


def search_case(pa, seed, N=40, L=900, swaps=4):
    """data evolved on a random tree; the start: that tree after a few random interchanges, its lengths carried along"""
    rng = np.random.default_rng(seed)
    left, right = ref.random_tree(N, rng)
    t = rng.uniform(0.03, 0.25, 2 * N - 1)
    m = ref.evolve(left, right, t, N, L, rng)
    l, r, tt = pa.merges_canonical_lengths(left, right, t, N)
    for _ in range(swaps):
        d = pa.model_nni_deltas_from_rows(m, l, r, tt, pa.SubstModel.jc69()).delta
        ks = np.argwhere(~np.isnan(d))
        k, kind = ks[rng.integers(0, len(ks))]
        l, r, tt = pa.nni_apply_lengths(l, r, tt, N, N + int(k), int(kind))
    return m, l, r, tt


@pytest.mark.parametrize("moves_per_round,length_rounds", [(1, 0), (0, 0), (3, 2)])
def test_the_search_matches_the_host_search_move_for_move(pa, moves_per_round, length_rounds):
    N, L = 40, 900
    m, left, right, t = search_case(pa, 5)
    model = pa.SubstModel.simulator(rates=(0.5, 2.0), weights=(0.5, 0.5))
    core = core_handle(pa, m)
    kw = dict(max_rounds=30, moves_per_round=moves_per_round, length_rounds=length_rounds)
    want = pa.model_nni_from_rows(m, left, right, t, model, **kw)
    got = core.tree_model_nni(left, right, model, t, **kw)
    assert want.rounds >= 2 and want.n_moves >= 3 and want.local_optimum
    if (moves_per_round, length_rounds) == (1, 0):
        # no two candidates of a round may tie within the gain tolerance: the tree of every round replayed on the host
        l, r, tt = pa.merges_canonical_lengths(left, right, t, N)
        for mv in want.moves:
            g = np.sort(pa.model_nni_deltas_from_rows(m, l, r, tt, model).delta.reshape(-1))
            g = g[g > 1e-3 - 1e-9]
            tol = 4 * EPS * (2 * L + 16) + 16 * EPS * np.abs(g[-1])
            assert g.size and (g.size == 1 or np.diff(g).min() > tol), "two candidates tie within the tolerance: choose other inputs"
            l, r, tt = pa.nni_apply_lengths(l, r, tt, N, int(mv["node"]), int(mv["kind"]))
        assert np.array_equal(l, want.left) and np.array_equal(r, want.right) and np.array_equal(tt[:-1], want.lengths[:-1])
    for name in ("rounds", "passes", "length_passes", "rollbacks", "n_moves", "local_optimum", "candidates_last", "zero_sites", "clamped_lengths",
                 "missing_cells", "pop_size", "sites"):
        assert getattr(got, name) == getattr(want, name), name
    assert got.passes == got.rounds + got.rollbacks + 1
    for name in ("round", "node", "kind"):
        assert np.array_equal(got.moves[name], want.moves[name]), name
    assert np.allclose(got.moves["gain"], want.moves["gain"], rtol=8 * EPS, atol=2 * EPS * (2 * L + 16))
    assert np.array_equal(got.left, want.left) and np.array_equal(got.right, want.right)
    assert np.allclose(got.lengths, want.lengths, rtol=1e-9 if length_rounds else 0, atol=0)
    assert np.all(np.diff(got.round_lnl) > 0) and got.round_lnl.size == got.rounds + 1 and got.lnl == got.round_lnl[-1]
    host = pa.model_likelihood_from_rows(m, got.left, got.right, got.lengths, model, derivatives=False)
    assert abs(got.lnl - host.lnl) <= EPS * (L + 8) * (np.abs(host.site_lnl) + 2.0).sum()
    assert got.newick().count(":") == 2 * N - 2 and got.merges()[0] is got.left and got.merges == N - 1
    core.close()


SIM = dict(pop_size=100, core_size=2001, pan_genes=300, core_genes=20, HR_rate=0.5, HGT_rate=0.5, seed=11, n_gen=8, max_distances=100)


def test_a_simulation_and_no_change_of_state(pa):
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(6)
    left, right = sim.neighbour_joining().merges()[:2]
    m = sim.core_genome.read_matrix()
    model = pa.SubstModel.simulator()
    t = pa.f81_lengths_from_changes(sim.tree_parsimony(left, right, branches=True).branch_changes, 2001, model.freq)
    got = sim.model_nni_deltas(left, right, t, model)
    want = pa.model_nni_deltas_from_rows(m, left, right, t, model)
    assert_deltas(got, want, pa.model_likelihood_from_rows(m, left, right, t, model, derivatives=False).site_lnl, 2001)
    s = sim.tree_model_nni(left, right, model, max_rounds=3)           # default start lengths: the same t
    assert s.pop_size == 100 and s.sites == 2001 and s.lnl >= s.start_lnl and np.all(np.diff(s.round_lnl) > 0)
    assert s.start_lnl == sim.tree_model_likelihood(left, right, t, model).lnl
    ms = sim.tree_model_nni_timing()
    assert len(ms) == 3 and ms[0] >= 0.0 and ms[1] > 0.0 and ms[2] > 0.0
    assert np.array_equal(sim.core_genome.read_matrix(), m)
    sim.run(2)
    plain = pa.Simulation(pa.make_params(**SIM))
    plain.run(8)
    assert np.array_equal(plain.core_genome.read_matrix(), sim.core_genome.read_matrix())
    assert np.array_equal(plain.pan_genome.read_matrix(), sim.pan_genome.read_matrix())
    plain.close()
    sim.close()


@pytest.mark.parametrize("shards", [2, 3])
def test_multi_simulation_against_the_host(pa, shards):
    """site_class is indexed by the global site; the shards' products multiply in shard order, one selection"""
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(5)
    left, right = sim.upgma_tree().merges()
    m = sim.core_genome.read_matrix()
    sim.close()
    rng = np.random.default_rng(shards)
    t = rng.uniform(0.001, 0.05, 199)
    model = pa.SubstModel.simulator(rates=(0.3, 1.0, 2.5), site_class=rng.integers(0, 3, 2001))
    multi = pa.MultiSimulation(pa.make_params(**SIM), shards, devices=[0] * shards)
    multi.run(5)
    want = pa.model_nni_deltas_from_rows(m, left, right, t, model)
    got = multi.model_nni_deltas(left, right, t, model)
    assert_deltas(got, want, pa.model_likelihood_from_rows(m, left, right, t, model, derivatives=False).site_lnl, 2001)
    kw = dict(max_rounds=2, moves_per_round=1, length_rounds=0)
    s, h = multi.tree_model_nni(left, right, model, t, **kw), pa.model_nni_from_rows(m, left, right, t, model, **kw)
    assert s.sites == 2001 and s.rounds == h.rounds and np.array_equal(s.left, h.left) and np.array_equal(s.right, h.right)
    assert np.array_equal(s.moves["node"], h.moves["node"]) and np.array_equal(s.lengths, h.lengths)
    ms = multi.tree_model_nni_timing()
    assert len(ms) == 3 and ms[1] > 0.0
    with pytest.raises(pa.PansimError) as e:
        multi.model_nni_deltas(left, right, t, model.sliced(0, 1000))
    assert e.value.code == PS_ERR_INVALID and "site_classes = 2001, not 1000" in str(e.value)
    multi.close()


def test_site_shards_answer_for_their_own_sites(pa):
    m, left, right, t = case(130, 1000, "random", junk=True)
    model = pa.SubstModel.simulator(rates=(0.3, 1.0, 2.5), site_class=np.random.default_rng(9).integers(0, 3, 1000))
    cuts = [0, 333, 701, 1000]
    total, lnl = np.zeros((129, 2)), 0.0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        piece = np.ascontiguousarray(m[:, lo:hi])
        shard = core_handle(pa, piece, col_offset=lo, global_cols=1000)
        got = shard.model_nni_deltas(left, right, t, model.sliced(lo, hi))
        want = pa.model_nni_deltas_from_rows(piece, left, right, t, model.sliced(lo, hi))
        assert_deltas(got, want, pa.model_likelihood_from_rows(piece, left, right, t, model.sliced(lo, hi), derivatives=False).site_lnl, hi - lo)
        total, lnl = total + got.delta, lnl + got.lnl
        shard.close()
    whole = pa.model_nni_deltas_from_rows(m, left, right, t, model)
    some = ~np.isnan(whole.delta)
    assert np.all(np.abs(total - whole.delta)[some] <= (2 * EPS * (2 * 1000 + 16) + 8 * EPS * np.abs(whole.delta))[some])
    assert abs(lnl - whole.lnl) <= 1e-9 * abs(whole.lnl)


def test_the_scratch_grows_and_timing(pa):
    m, left, right, t = case(500, 300, "balanced", junk=False)
    deep = ref.caterpillar(500, np.random.default_rng(1).permutation(500))
    core = core_handle(pa, m)
    with pytest.raises(pa.PansimError) as e:
        core.tree_model_nni_timing()                                # nothing to report yet
    assert e.value.code == PS_ERR_STATE
    one_k, four = pa.SubstModel.simulator(), pa.SubstModel.gamma(0.5, 4, freq=(0.1, 0.2, 0.3, 0.4))
    # (one row of x, then four rows and the level offsets of the caterpillar: each needs more; then less again)
    for (l, r), model in (((left, right), one_k), (deep, four), ((left, right), one_k)):
        got, want = core.model_nni_deltas(l, r, t, model), pa.model_nni_deltas_from_rows(m, l, r, t, model)
        assert_deltas(got, want, pa.model_likelihood_from_rows(m, l, r, t, model, derivatives=False).site_lnl, 300)
        ms = core.tree_model_nni_timing()
        assert len(ms) == 3 and ms[0] >= 0.0 and ms[1] > 0.0 and ms[2] > 0.0
    with pytest.raises(pa.PansimError) as e:
        core.tree_model_timing()                                    # the likelihood entry's slot is its own
    assert e.value.code == PS_ERR_STATE
    one = core.tree_model_nni_timing()[1]
    s = core.tree_model_nni(left, right, one_k, t, max_rounds=2, length_rounds=0)
    assert s.passes >= 2 and core.tree_model_nni_timing()[1] > one  # the sum over the passes of the call
    core.close()


def test_handle_checks(pa):
    rng = np.random.default_rng(6)
    core = core_handle(pa, np.array(ref.BASES, np.uint8)[rng.integers(0, 4, (20, 64))])
    acc = pa.Population(20, 10, 2, False, 0.5, 0, 3)
    left, right = ref.caterpillar(20)
    t = np.full(39, 0.1)
    model = pa.SubstModel.simulator()
    for call in (lambda: acc.model_nni_deltas(left, right, t, model), lambda: acc.tree_model_nni(left, right, model, t)):
        with pytest.raises(pa.PansimError) as e:
            call()
        assert e.value.code == PS_ERR_INVALID and "core handle" in str(e.value)
    bad = t.copy()
    bad[4] = np.inf
    for l, r, tt, mod, kw, text in ((left[:-1], right[:-1], t[:-1], model, {}, "spanning tree: 19 merges over 20 leaves, not 18"),
                                    (left, right, t, model, dict(max_rounds=0), "max_rounds must be at least 1"),
                                    (left, right, t, model, dict(eps_gain=0.0), "eps_gain must be a positive number"),
                                    (left, right, bad, model, {}, "length of node 4 is not a finite number"),
                                    (left, right, t, pa.SubstModel.simulator(rates=(1.0, 2.0), site_class=np.zeros(63, np.uint8)), {},
                                     "site_classes = 64, not 63"),
                                    (left, right, t, pa.SubstModel.simulator(rates=(0.0, 1.0), site_class=np.zeros(64, np.uint8)), {},
                                     "nothing to climb from")):
        with pytest.raises(pa.PansimError) as e:
            core.tree_model_nni(l, r, mod, tt, **kw)
        assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)
    # an invariant class assigned to variable sites: the pass counts them and leaves them out, every gain stays finite
    d = core.model_nni_deltas(left, right, t, pa.SubstModel.simulator(rates=(0.0, 1.0), site_class=(np.arange(64) % 2 == 0).astype(np.uint8)))
    h = pa.model_nni_deltas_from_rows(core.read_matrix(), left, right, t,
                                      pa.SubstModel.simulator(rates=(0.0, 1.0), site_class=(np.arange(64) % 2 == 0).astype(np.uint8)))
    assert d.zero_sites == h.zero_sites > 0 and d.lnl == -np.inf and np.all(np.isfinite(d.delta[~np.isnan(h.delta)]))
    assert np.allclose(d.delta[~np.isnan(h.delta)], h.delta[~np.isnan(h.delta)], rtol=1e-12, atol=1e-12)
    for p in (core, acc):
        p.close()
