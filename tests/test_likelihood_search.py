"""The host entries of the likelihood tree search (ps_model_nni_deltas_from_rows, ps_model_nni_from_rows, ps_nni_apply_lengths,
ps_merges_canonical_lengths; docs/LIKELIHOOD_SEARCH.md) against tests/likelihood_search_ref.py; no device.

A gain comes from the four pieces around an edge; the references never form them: every neighbour tree is RESCORED FROM SCRATCH --
the move applied with its lengths, the whole tree evaluated again -- by the library's own ps_model_likelihood_from_rows, by NumPy
pruning without rescaling, and at 4 to 6 leaves by the sum over all assignments.  The tolerance of a gain is
1e-10 sum_s (|ln l_s| + |ln l'_s| + 1): both log-likelihoods are sums over the sites of logs of sums of non-negative products."""
import re

import numpy as np
import pytest

import likelihood_search_ref as ls
import subst_model_ref as mref
import tree_likelihood_ref as ref

PS_ERR_INVALID = -1
NAMES = ["ps_tree_model_nni_deltas", "ps_sim_tree_model_nni_deltas", "ps_multi_tree_model_nni_deltas", "ps_tree_model_nni", "ps_sim_tree_model_nni",
         "ps_multi_tree_model_nni", "ps_tree_model_nni_timing", "ps_model_nni_deltas_from_rows", "ps_model_nni_from_rows", "ps_nni_apply_lengths",
         "ps_merges_canonical_lengths"]
UNEVEN = (0.1, 0.2, 0.3, 0.4)
ROOT = (0.4, 0.3, 0.2, 0.1)
QUARTER = (0.25, 0.25, 0.25, 0.25)


def test_every_new_symbol_is_exported_and_declared(pa):
    import ctypes
    import os
    from pansim_amd import _lib
    lib = ctypes.CDLL(pa.LIB_PATH)
    hdr = open(os.path.join(os.path.dirname(pa.LIB_PATH), "..", "include", "pansim_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
        comment = " ".join(hdr[:re.search(r"\bint %s\s*\(" % name, hdr).start()].rsplit("/*", 1)[1].replace("\n *", " ").split())
        assert "the reference has no such function" in comment and "population.rs:443" in comment, name
    assert pa.PS_MODEL_NNI_MAX_POP == 1024 and "#define PS_MODEL_NNI_MAX_POP 1024u" in hdr and lib.ps_abi_version() == 3
    # 4 n_pad + 140 Mp bytes of LDS and the schedule's copy: the largest multiple of 256 under the CU's 160 KiB
    lds = lambda n: 4 * n + 140 * n                              # noqa: E731  (n a multiple of 16: n_pad = Mp = n)
    assert lds(1024) == 147456 and lds(1024) + 4 * (1023 + 1023 + 1) == 155644 <= 156 * 1024 and lds(1280) > 160 * 1024
    assert ctypes.sizeof(_lib.MlNni) == 15 * 8 and ctypes.sizeof(_lib.MlNniParams) == 24
    for cls in (pa.Population, pa.Simulation, pa.MultiSimulation):
        for method in ("model_nni_deltas", "tree_model_nni", "tree_model_nni_timing"):
            assert callable(getattr(cls, method))
    for fn in ("model_nni_deltas_from_rows", "model_nni_from_rows", "nni_apply_lengths", "merges_canonical_lengths", "LikelihoodSearch"):
        assert callable(getattr(pa, fn))


def trees():
    """every tree shape of 4 to 6 leaves with permuted leaves; balanced, caterpillar and random trees of 8 to 24 leaves"""
    rng = np.random.default_rng(2)
    for n in range(4, 7):
        for shape in ref.shapes(n):
            yield n, ref.merges_of_shape(shape, rng.permutation(n))
    for n in (8, 13, 24):
        yield n, ref.balanced(n)
        yield n, ref.caterpillar(n, rng.permutation(n))
        yield n, ref.random_tree(n, rng)


def lengths_for(rng, nodes):
    """lengths from below the lower bound to above the upper one, both bounds among them"""
    t = 10.0 ** rng.uniform(-9, 1.2, nodes)
    t[rng.integers(0, nodes)] = 1e-8
    t[rng.integers(0, nodes)] = 10.0
    return t


def data_for(rng, left, right, n, L):
    """evolved columns with the bytes 0 / 3 / 255 among them and one column of base 1"""
    m = ref.evolve(left, right, rng.uniform(0.05, 0.6, 2 * n - 1), n, L, rng)
    m[rng.integers(0, n), 1], m[rng.integers(0, n), 2], m[rng.integers(0, n), 3] = 0, 3, 255
    m[:, 0] = 1
    return m


def models_for(pa, rng, L):
    """(name, SubstModel, the reference's dict): K = 1, 3 assigned, a 4-mixture with one zero rate, the simulator's law, JC69"""
    cls = rng.integers(0, 3, L)
    return [("jc", pa.SubstModel.jc69(), ls.model_of(QUARTER)),
            ("sim", pa.SubstModel.simulator(), ls.model_of(mref.SIM, QUARTER)),
            ("k1 uneven", pa.SubstModel(UNEVEN, root=ROOT, rates=(1.7,)), ls.model_of(UNEVEN, ROOT, (1.7,))),
            ("k3 assigned", pa.SubstModel.simulator(root=ROOT, rates=(0.5, 1.0, 2.0), site_class=cls), ls.model_of(mref.SIM, ROOT, (0.5, 1.0, 2.0), cls=cls)),
            ("k4 mixture zero rate", pa.SubstModel.simulator(rates=(0.0, 0.4, 1.0, 2.6), weights=(0.1, 0.4, 0.3, 0.2)),
             ls.model_of(mref.SIM, QUARTER, (0.0, 0.4, 1.0, 2.6), (0.1, 0.4, 0.3, 0.2)))]


@pytest.mark.parametrize("k,n,tree", [(k,) + c for k, c in enumerate(trees())])
def test_every_gain_against_rescoring_the_neighbour_tree_from_scratch(pa, k, n, tree):
    rng = np.random.default_rng(100 + k)
    left, right = tree
    L = 7
    m, t = data_for(rng, left, right, n, L), lengths_for(rng, 2 * n - 1)
    for name, model, rmodel in models_for(pa, rng, L):
        got = pa.model_nni_deltas_from_rows(m, left, right, t, model)
        base = pa.model_likelihood_from_rows(m, left, right, t, model, derivatives=False)
        assert got.lnl == base.lnl and got.zero_sites == 0, name
        cands = ls.candidates(left, right, n)
        assert len(cands) == 2 * (n - 3) and sorted(cands) == [(n + int(i), int(j)) for i, j in np.argwhere(~np.isnan(got.delta))], name
        assert np.array_equal(got.delta_mant == 0.0, np.isnan(got.delta))
        assert np.all((got.delta_mant == 0.0) | ((got.delta_mant >= 0.5) & (got.delta_mant < 1.0)))
        scratch = ls.gains(m, left, right, t, rmodel)
        for node, kind in cands:
            l2, r2, t2 = pa.nni_apply_lengths(left, right, t, n, node, kind)
            rl, rr, rt = ls.neighbour(left, right, t, n, node, kind)
            assert np.array_equal(l2, rl) and np.array_equal(r2, rr) and np.array_equal(t2, rt), (name, node, kind)
            after = pa.model_likelihood_from_rows(m, l2, r2, t2, model, derivatives=False)
            tol = 1e-10 * (np.abs(base.site_lnl) + np.abs(after.site_lnl) + 1.0).sum()
            g = got.delta[node - n, kind]
            assert abs(g - (after.lnl - base.lnl)) <= tol, (name, node, kind, g, after.lnl - base.lnl)
            assert abs(g - scratch[(node, kind)]) <= tol, (name, node, kind, g, scratch[(node, kind)])
            if n <= 6 and name in ("sim", "k4 mixture zero rate"):
                brute = sum(np.log(mref.site(m[:, s], tr[0], tr[1], tr[2], model.freq, model.root, model.rates, model.weights)["lik"]) * sign
                            for s in range(L) for tr, sign in (((l2, r2, t2), 1.0), ((left, right, t), -1.0)))
                assert abs(g - brute) <= tol, (name, node, kind, g, brute)
        some = ~np.isnan(got.delta[:, 0])
        assert np.array_equal(got.edge_margin()[some], -got.delta[some].max(axis=1)) and np.all(np.isnan(got.edge_margin()[~some]))


def test_an_invariant_class_at_a_variable_site(pa):
    rng = np.random.default_rng(3)
    n, L = 9, 12
    left, right = ref.random_tree(n, rng)
    t = rng.uniform(0.05, 0.3, 2 * n - 1)
    m = ref.evolve(left, right, np.full(2 * n - 1, 0.5), n, L, rng)
    m[:, 5] = 4
    variable = np.array([len(set(m[:, s])) > 1 for s in range(L)])
    cls = np.zeros(L, np.uint8)
    cls[[2, 5, 7]] = 1                                           # rate 0 at the sites 2, 5, 7; site 5 is constant
    assert variable[2] and variable[7]
    model = pa.SubstModel.simulator(rates=(1.0, 0.0), site_class=cls)
    got = pa.model_nni_deltas_from_rows(m, left, right, t, model)
    assert got.zero_sites == 2 and got.lnl == -np.inf
    some = ~np.isnan(got.delta)
    assert some.sum() == 2 * (n - 3) and np.all(np.isfinite(got.delta[some]))
    # the gains: those of the other sites alone
    keep = np.array([s not in (2, 7) for s in range(L)])
    rest = pa.model_nni_deltas_from_rows(np.ascontiguousarray(m[:, keep]), left, right, t, pa.SubstModel.simulator(rates=(1.0, 0.0), site_class=cls[keep]))
    assert rest.zero_sites == 0 and np.array_equal(rest.delta_mant, got.delta_mant) and np.array_equal(rest.delta_exp, got.delta_exp)
    scratch = ls.gains(m, left, right, t, ls.model_of(mref.SIM, QUARTER, (1.0, 0.0), cls=cls))
    for (node, kind), g in scratch.items():
        assert abs(got.delta[node - n, kind] - g) <= 1e-10 * L * 40
    with pytest.raises(pa.PansimError) as e:
        pa.model_nni_from_rows(m, left, right, t, model)
    assert e.value.code == PS_ERR_INVALID and "lnL = -inf" in str(e.value) and "nothing to climb from" in str(e.value)


def test_lengths_through_moves_and_the_canonical_form(pa):
    rng = np.random.default_rng(4)
    for n in (4, 5, 9, 30):
        left, right = ref.random_tree(n, rng)
        t = rng.uniform(0.01, 1.0, 2 * n - 1)
        l, r, tt = pa.merges_canonical_lengths(left, right, t, n)
        assert ls.clade_lengths(l, r, tt, n) == ls.clade_lengths(left, right, t, n) and tt[-1] == t[-1]
        again = pa.merges_canonical_lengths(l, r, tt, n)
        assert all(np.array_equal(a, b) for a, b in zip(again, (l, r, tt)))                        # idempotent
        assert all(np.array_equal(a, b) for a, b in zip((l, r), pa.merges_canonical(left, right, n)))
        for _ in range(12):
            cands = ls.candidates(l, r, n)
            node, kind = cands[rng.integers(0, len(cands))]
            before, sets = ls.clade_lengths(l, r, tt, n), ls.clades(l, r, n)
            par = ls.parents(l, r, n)
            moved = {sets[node]} | ({sets[int(r[-1])]} if par[node] == 2 * n - 2 else set())       # the root's edge regroups both sides
            l2, r2, t2 = pa.nni_apply_lengths(l, r, tt, n, node, kind)
            assert all(np.array_equal(a, b) for a, b in zip((l2, r2), pa.nni_apply(l, r, n, node, kind)))
            after = ls.clade_lengths(l2, r2, t2, n)
            # every clade but the regrouped ones keeps the length of the branch above it; the regrouped nodes keep theirs
            assert {c: v for c, v in before.items() if c not in moved} == {c: v for c, v in after.items() if c in before and c not in moved}
            assert sorted(before.values()) == sorted(after.values()) and len(set(after) - set(before)) == len(moved)
            assert sorted(after[c] for c in set(after) - set(before)) == sorted(before[c] for c in moved)
            l, r, tt = l2, r2, t2


def roll_case(seed, n=14, L=120):
    """data evolved on one random tree, the start another: many improving moves per round, some batches overshoot"""
    rng = np.random.default_rng(seed)
    left, right = ref.random_tree(n, rng)
    t = rng.uniform(0.02, 0.3, 2 * n - 1)
    m = mref.evolve(left, right, t, n, L, rng, mref.SIM, QUARTER, 1.0)
    sl, sr = ref.random_tree(n, rng)
    return m, sl, sr, rng.uniform(0.02, 0.3, 2 * n - 1)


@pytest.mark.parametrize("seed", [0, 1, 6, 8, 23])
@pytest.mark.parametrize("moves_per_round,length_rounds", [(1, 0), (3, 0), (0, 0), (0, 2)])
def test_the_search_move_for_move_against_the_reference_loop(pa, seed, moves_per_round, length_rounds):
    m, left, right, t = roll_case(seed)
    n, L = m.shape
    model, rmodel = pa.SubstModel.simulator(), ls.model_of(mref.SIM, QUARTER)
    tune = None
    if length_rounds:
        tune = lambda l, r, tt: pa.model_ml_lengths_from_rows(m, l, r, tt, model, max_rounds=length_rounds, eps_lnl=1e-3).lengths   # noqa: E731
    want = ls.search(m, left, right, t, rmodel, moves_per_round=moves_per_round, optimise=tune)
    got = pa.model_nni_from_rows(m, left, right, t, model, moves_per_round=moves_per_round, length_rounds=length_rounds)
    assert [(int(a), int(b), int(c)) for a, b, c in zip(got.moves["round"], got.moves["node"], got.moves["kind"])] == want["moves"]
    assert np.array_equal(got.left, want["left"]) and np.array_equal(got.right, want["right"])
    assert np.allclose(got.lengths, want["lengths"], rtol=1e-12, atol=0)
    assert got.rollbacks == want["rollbacks"] and got.local_optimum == want["local_optimum"] and got.local_optimum
    assert got.rounds == len(want["round_lnl"]) - 1 and got.passes == got.rounds + got.rollbacks + 1 and got.n_moves == len(want["moves"])
    assert np.allclose(got.round_lnl, want["round_lnl"], rtol=1e-12, atol=0) and np.all(np.diff(got.round_lnl) > 0)
    assert got.lnl == got.round_lnl[-1] and got.candidates_last == 0 and got.zero_sites == 0 and got.sites == L and got.pop_size == n
    assert (got.length_passes > 1) == bool(length_rounds) and got.clamped_lengths == 0
    start = pa.model_likelihood_from_rows(m, left, right, t, model, derivatives=False).lnl
    assert got.start_lnl == start and (length_rounds or got.round_lnl[0] == start)
    if moves_per_round == 1:
        assert got.rollbacks == 0 and np.all(got.moves["round"] == np.arange(1, got.n_moves + 1))
    d = pa.model_nni_deltas_from_rows(m, got.left, got.right, got.lengths, model)
    assert np.nanmax(d.delta) <= 1e-3 and np.all(d.edge_margin()[~np.isnan(d.delta[:, 0])] >= -1e-3)


def test_the_seeded_set_takes_the_rollback_path():
    """the reference loop itself rolls back in at least three of the cases above (the seeds were picked for that)"""
    rolled = [ls.search(*roll_case(seed), ls.model_of(mref.SIM, QUARTER))["rollbacks"] for seed in (0, 6, 8, 23)]
    assert sum(v > 0 for v in rolled) >= 3, rolled


def test_a_round_cap_and_the_move_cap(pa):
    m, left, right, t = roll_case(6)
    model = pa.SubstModel.simulator()
    full = pa.model_nni_from_rows(m, left, right, t, model, moves_per_round=1, length_rounds=0)
    cut = pa.model_nni_from_rows(m, left, right, t, model, max_rounds=3, moves_per_round=1, length_rounds=0)
    assert full.rounds > 3 and cut.rounds == 3 and not cut.local_optimum and cut.candidates_last > 0 and cut.passes == 4
    assert np.array_equal(cut.moves, full.moves[:3]) and np.array_equal(cut.round_lnl, full.round_lnl[:4])
    assert cut.newick().count(":") == 2 * 14 - 2 and cut.merges == 13 and cut.merges()[0] is cut.left


def test_errors(pa):
    rng = np.random.default_rng(6)
    m = np.array(ref.BASES, np.uint8)[rng.integers(0, 4, (20, 64))]
    left, right = ref.caterpillar(20)
    t, model = np.full(39, 0.1), pa.SubstModel.simulator()
    bad = t.copy()
    bad[4] = np.nan
    for l, r, tt, mod, kw, text in ((left[:-1], right[:-1], t[:-1], model, {}, "spanning tree: 19 merges over 20 leaves, not 18"),
                                    (left, right, t, model, dict(max_rounds=0), "max_rounds must be at least 1"),
                                    (left, right, t, model, dict(eps_gain=0.0), "eps_gain must be a positive number"),
                                    (left, right, t, model, dict(eps_gain=np.inf), "eps_gain must be a positive number"),
                                    (left, right, bad, model, {}, "length of node 4 is not a finite number"),
                                    ([0] * 19, list(range(1, 20)), t, model, {}, "a child of merge"),
                                    (left, right, t, pa.SubstModel((0.5, 0.5, 0.0, 0.0), root=ROOT), {}, "freq may have at most one zero"),
                                    (left, right, t, pa.SubstModel.simulator(rates=(1.0, 2.0), site_class=np.zeros(63, np.uint8)), {},
                                     "site_classes = 64, not 63")):
        with pytest.raises(pa.PansimError) as e:
            pa.model_nni_from_rows(m, l, r, tt, mod, **kw)
        assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)
        if not kw:
            with pytest.raises(pa.PansimError) as e:
                pa.model_nni_deltas_from_rows(m, l, r, tt, mod)
            assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)
    big = np.full((1025, 2), 2, np.uint8)
    for call in (lambda: pa.model_nni_deltas_from_rows(big, *ref.caterpillar(1025), np.full(2049, 0.1), model),
                 lambda: pa.model_nni_from_rows(big, *ref.caterpillar(1025), np.full(2049, 0.1), model),
                 lambda: pa.merges_canonical_lengths(*ref.caterpillar(1025), np.full(2049, 0.1), 1025)):
        with pytest.raises(pa.PansimError) as e:
            call()
        assert e.value.code == PS_ERR_INVALID and "PS_MODEL_NNI_MAX_POP = 1024" in str(e.value)
    for node, kind, text in ((38, 0, "node 38 has no interchange"), (3, 0, "node 3 has no interchange"), (25, 2, "kind must be 0 or 1")):
        with pytest.raises(pa.PansimError) as e:
            pa.nni_apply_lengths(left, right, t, 20, node, kind)
        assert e.value.code == PS_ERR_INVALID and text in str(e.value)
    with pytest.raises(ValueError):
        pa.nni_apply_lengths(left, right, t[:-1], 20, 25, 0)
    # the smallest trees: two and three leaves have no candidate, a search ends where it starts
    for n in (2, 3):
        l, r = ref.caterpillar(n)
        d = pa.model_nni_deltas_from_rows(m[:n], l, r, np.full(2 * n - 1, 0.1), model)
        assert np.all(np.isnan(d.delta)) and np.isfinite(d.lnl)
        s = pa.model_nni_from_rows(m[:n], l, r, np.full(2 * n - 1, 0.1), model)
        assert s.rounds == 0 and s.local_optimum and s.n_moves == 0 and s.passes == 1


RECOVERY_SITES = 300


def recovery_case(seed):
    """a random 16-leaf tree with 0.05 .. 0.2 events per site on every branch, data under the simulator's law, and the start: the
    generating tree after three random interchanges"""
    rng = np.random.default_rng(1000 + seed)
    n = 16
    left, right = ref.random_tree(n, rng)
    t = rng.uniform(0.05, 0.2, 2 * n - 1) * mref.beta_of(mref.SIM)
    m = mref.evolve(left, right, t, n, RECOVERY_SITES, rng, mref.SIM, QUARTER, 1.0)
    gen = ls.canonical(left, right, t, n)
    l, r, tt = gen
    for _ in range(3):
        c = ls.candidates(l, r, n)
        node, kind = c[rng.integers(0, len(c))]
        l, r, tt = ls.neighbour(l, r, tt, n, node, kind)
    return m, gen, l, r, tt


def test_the_search_recovers_the_generating_tree(pa):
    """Robinson-Foulds distance 0 in at least 8 of 10 seeds at RECOVERY_SITES sites; the reference loop (with the host's length
    rounds) meets the same bar: 10 of 10, docs/LIKELIHOOD_SEARCH.md"""
    model = pa.SubstModel.simulator()
    hits = []
    for seed in range(10):
        m, gen, l, r, tt = recovery_case(seed)
        assert ls.rf_distance(gen[:2], (l, r), 16) > 0
        s = pa.model_nni_from_rows(m, l, r, tt, model)
        hits.append(ls.rf_distance(gen[:2], (s.left, s.right), 16) == 0)
        assert s.lnl > s.start_lnl and s.local_optimum
    print("recovered", sum(hits), "of 10")
    assert sum(hits) >= 8


@pytest.mark.parametrize("seed", [0, 5])
def test_the_reference_loop_recovers_it_too(pa, seed):
    m, gen, l, r, tt = recovery_case(seed)
    model = pa.SubstModel.simulator()
    tune = lambda a, b, c: pa.model_ml_lengths_from_rows(m, a, b, c, model, max_rounds=5, eps_lnl=1e-3).lengths   # noqa: E731
    want = ls.search(m, l, r, tt, ls.model_of(mref.SIM, QUARTER), optimise=tune)
    assert ls.rf_distance(gen[:2], (want["left"], want["right"]), 16) == 0
    got = pa.model_nni_from_rows(m, l, r, tt, model)
    assert np.array_equal(got.left, want["left"]) and np.array_equal(got.right, want["right"]) and np.allclose(got.lengths, want["lengths"], rtol=1e-12)
