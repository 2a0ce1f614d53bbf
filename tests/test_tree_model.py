"""The host entries of the likelihood of a tree under F81 with a root distribution and rate categories
(ps_model_likelihood_from_rows, ps_model_ml_lengths_from_rows, ps_f81_lengths_from_changes; docs/TREE_MODEL.md) against
tests/subst_model_ref.py, and `gamma_rates`; no device.

Tolerances carry over from tests/test_tree_likelihood.py, because nothing new cancels.  A site likelihood is a sum of products of
non-negative terms (pi >= 0, rho > 0, weights > 0): a few dozen roundings, held to 1e-12 relative, and so is the posterior mean
rate, a ratio of such sums.  The derivative terms hold the one difference D - A, so their bound is absolute:
  dlnL/dt_c      1e-10 sum_s sum_k post_sk (r_k / beta) (|A| + |A + B|) / l_sk
  d2lnL/dt_c2    1e-10 sum_s [sum_k post_sk (r_k / beta)^2 (|A| + |A + B|) / l_sk + (sum_k post_sk (r_k / beta) (|A| + |A + B|) / l_sk)^2]
with A and A + B category k's likelihood at x_c = 0 and at x_c = 1 from the brute-force reference: the first term bounds q, the
second h, as the JC69 test bounds g and h."""
import math
import re
from fractions import Fraction

import numpy as np
import pytest

import subst_model_ref as mref
import tree_likelihood_ref as ref

PS_ERR_INVALID = -1
NAMES = ["ps_tree_model_likelihood", "ps_sim_tree_model_likelihood", "ps_multi_tree_model_likelihood", "ps_tree_model_ml_lengths",
         "ps_sim_tree_model_ml_lengths", "ps_multi_tree_model_ml_lengths", "ps_tree_model_timing", "ps_model_likelihood_from_rows",
         "ps_model_ml_lengths_from_rows", "ps_f81_lengths_from_changes"]
UNEVEN = (0.1, 0.2, 0.3, 0.4)
ROOT = (0.4, 0.3, 0.2, 0.1)


def test_every_new_symbol_is_exported_and_declared(pa):
    import ctypes
    import os
    from pansim_amd import _lib
    lib = ctypes.CDLL(pa.LIB_PATH)
    hdr = open(os.path.join(os.path.dirname(pa.LIB_PATH), "..", "include", "pansim_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
        comment = " ".join(hdr[:re.search(r"\bint %s\s*\(" % name, hdr).start()].rsplit("/*", 1)[1].replace("\n *", " ").split())
        assert "the reference has no such function" in comment and "population.rs:531" in comment, name
    assert "population.rs:201-203" in hdr
    assert pa.PS_MODEL_MAX_POP_DERIV == 1536 and "#define PS_MODEL_MAX_POP_DERIV 1536u" in hdr and pa.PS_MODEL_MAX_CATEGORIES == 8
    assert pa.PS_MODEL_MAX_POP_DERIV % 256 == 0 and lib.ps_abi_version() == 3
    # 4 (n_pad + Mp 9) + 32 slots bytes of LDS: the largest multiple of 256 under the CU's 160 KiB
    lds = lambda n: 4 * n + 36 * n + 32 * (2 * n - 1)          # noqa: E731  (n a multiple of 16: n_pad = Mp = n)
    assert lds(1024) == 106464 and lds(1536) == 159712 and lds(1536) <= 160 * 1024 < lds(1792)
    assert ctypes.sizeof(_lib.ModelLikelihood) == 16 * 8 and ctypes.sizeof(_lib.SubstModelC) == 8 * 8 + 8 + 16 * 8 + 16
    for cls in (pa.Population, pa.Simulation, pa.MultiSimulation):
        for method in ("tree_model_likelihood", "tree_model_ml_lengths", "tree_model_timing"):
            assert callable(getattr(cls, method))
    for fn in ("model_likelihood_from_rows", "model_ml_lengths_from_rows", "f81_lengths_from_changes", "gamma_rates", "SubstModel"):
        assert callable(getattr(pa, fn))
    sim = pa.SubstModel.simulator()
    assert list(sim.freq) == [0.0, 1 / 3, 1 / 3, 1 / 3] and list(sim.root) == [0.25] * 4 and sim.categories == 1
    assert pa.SubstModel.jc69().beta == 0.75 and abs(sim.beta - 2 / 3) < 1e-15


def small_cases():
    """every tree shape of 2 to 6 leaves with permuted leaves, and random joinings"""
    rng = np.random.default_rng(1)
    for n in range(2, 7):
        for shape in ref.shapes(n):
            yield n, ref.merges_of_shape(shape, rng.permutation(n))
        for _ in range(3):
            yield n, ref.random_tree(n, rng)


def lengths_for(rng, nodes):
    """lengths from below the lower bound to above the upper one, both bounds among them"""
    t = 10.0 ** rng.uniform(-9, 1.2, nodes)
    t[rng.integers(0, nodes)] = 1e-8
    t[rng.integers(0, nodes)] = 10.0
    return t


def models_for(pa, rng, L):
    """K in {1, 3, 8}, assigned and mixture, pi with and without a zero entry, rho != pi, a zero rate"""
    r8 = [0.0, 0.1, 0.3, 0.6, 1.0, 1.5, 2.5, 4.0]
    w8 = np.array([1, 2, 3, 4, 4, 3, 2, 1]) / 20.0
    return [("jc", pa.SubstModel.jc69()),
            ("sim", pa.SubstModel.simulator()),
            ("k1 uneven", pa.SubstModel(UNEVEN, root=ROOT, rates=(1.7,))),
            ("k3 mixture", pa.SubstModel(UNEVEN, root=ROOT, rates=(0.2, 1.0, 3.0), weights=(0.5, 0.3, 0.2))),
            ("k3 mixture zero rate", pa.SubstModel.simulator(rates=(0.0, 1.0, 2.5), weights=(0.2, 0.5, 0.3))),
            ("k3 assigned", pa.SubstModel.simulator(root=ROOT, rates=(0.5, 1.0, 2.0), site_class=rng.integers(0, 3, L))),
            ("k8 mixture", pa.SubstModel(UNEVEN, rates=r8, weights=w8)),
            ("k8 assigned", pa.SubstModel.simulator(rates=r8[1:] + [6.0], site_class=rng.integers(0, 8, L)))]


def check_against_brute(pa, rows, left, right, t, model, tag):
    n, L = rows.shape
    nodes = 2 * n - 1
    got = pa.model_likelihood_from_rows(rows, left, right, t, model)
    sites = [mref.site(rows[:, s], left, right, t, model.freq, model.root, model.rates, model.weights,
                       None if model.site_class is None else model.site_class[s], derivatives=True) for s in range(L)]
    lik = np.array([v["lik"] for v in sites])
    mine = got.site_mant * 2.0 ** got.site_exp.astype(np.float64)
    assert np.all(np.abs(mine - lik) <= 1e-12 * lik), tag
    assert abs(got.lnl - np.log(lik).sum()) <= 1e-12 * np.abs(np.log(lik)).sum() + 1e-13, tag
    rate = np.array([v["rate"] for v in sites])
    assert np.all(np.abs(got.site_rate - rate) <= 1e-12 * rate), tag
    assert got.missing_cells == int((~np.isin(rows, ref.BASES)).sum()) and got.sites == L and got.pop_size == n
    used = ref.clamp(t)
    assert got.clamped_lengths == int((used[:-1] != t[:-1]).sum()) and got.passes == 1 and got.rounds == 0
    assert got.categories == model.categories and got.classed == (model.site_class is not None)
    assert got.beta == pytest.approx(mref.beta_of(model.freq), rel=1e-15) and got.mean_rate == pytest.approx(float(model.weights @ model.rates))
    assert np.allclose(got.events()[:-1], used[:-1] / got.beta, rtol=1e-15)
    grad, curv = got.gradient(), got.curvature()
    assert got.branch_g[-1] == 0.0 and got.branch_h[-1] == 0.0 and got.branch_q[-1] == 0.0
    d1, d2 = sum(v["d1"] for v in sites), sum(v["d2"] for v in sites)
    s1, s2 = sum(v["scale1"] for v in sites), sum(v["scale2"] for v in sites)
    assert np.all(np.abs(grad[:-1] - d1) <= 1e-10 * s1), (tag, np.abs(grad[:-1] - d1).max())
    assert np.all(np.abs(curv[:-1] - d2) <= 1e-10 * s2), (tag, np.abs(curv[:-1] - d2).max())
    return got


def test_against_the_sum_over_all_assignments(pa):
    rng = np.random.default_rng(2)
    L = 4
    models = models_for(pa, rng, L)
    seen = 0
    for n, (left, right) in small_cases():
        rows = np.array(ref.BASES, np.uint8)[rng.integers(0, 4, (n, L))]
        rows[rng.random((n, L)) < 0.15] = rng.integers(0, 256, 1, dtype=np.uint8)[0]        # junk bytes: missing data
        rows[:, 0] = 1                                                                      # all base 1: the lost base
        t = lengths_for(rng, 2 * n - 1)
        # (every model on the small trees, two of them in turn on the 6-leaf ones, whose sums have 4^5 terms per branch)
        for tag, model in (models if n <= 4 else [models[seen % len(models)], models[(seen + 3) % len(models)]]):
            got = check_against_brute(pa, rows, left, right, t, model, (n, tag))
            if tag == "sim":
                # a column of base 1 everywhere: no event can have hit any branch
                x = mref.x_of(ref.clamp(t)[:-1], 1.0, got.beta)
                if not np.isin(rows[:, 0], ref.BASES).all():
                    continue
                assert got.site_mant[0] * 2.0 ** int(got.site_exp[0]) == pytest.approx(0.25 * np.prod(x), rel=1e-12)
        seen += 1
    assert seen == sum(len(ref.shapes(n)) + 3 for n in range(2, 7))


def test_a_column_of_the_lost_base_under_the_simulator_model(pa):
    """base 1 has frequency 0: it can only be inherited, so the likelihood of a column of base 1 is rho_1 times the probability
    that no branch was hit; one leaf of another base above it makes the column as likely as an event on that leaf's branch"""
    n = 5
    left, right = ref.caterpillar(n)
    t = np.array([0.1, 0.2, 0.3, 0.05, 0.4, 0.15, 0.25, 0.35, 0.0])
    rows = np.ones((n, 2), np.uint8)
    rows[2, 1] = 4
    got = pa.model_likelihood_from_rows(rows, left, right, t, pa.SubstModel.simulator())
    x = mref.x_of(t[:-1], 1.0, 2.0 / 3.0)
    lik = got.site_mant * 2.0 ** got.site_exp.astype(np.float64)
    assert lik[0] == pytest.approx(0.25 * np.prod(x), rel=1e-13)
    assert lik[1] == pytest.approx(0.25 * np.prod(x) / x[2] * (1 - x[2]) / 3, rel=1e-13)
    assert np.all(np.isfinite(got.branch_g)) and got.missing_cells == 0


def junk_cases(rng):
    for n, L in ((7, 40), (12, 33)):
        left, right = ref.random_tree(n, rng)
        t = lengths_for(rng, 2 * n - 1)
        rows = ref.evolve(left, right, np.full(2 * n - 1, 0.3), n, L, rng)
        yield rows, left, right, t
        junk = rows.copy()
        junk[rng.random(junk.shape) < 0.1] = rng.integers(0, 256, 1, dtype=np.uint8)[0]
        junk[0, 0], junk[:, 1] = 0, 0
        yield junk, left, right, t


def test_the_jc69_anchor_returns_the_bits_of_the_jc_entries(pa):
    """with pi = rho = 1/4 and one category of rate 1 every scaling is a power of two.  The gradient and curvature are the same
    sums with x inside instead of outside (sum_s x r_s against x sum_s r_s): each within 2 L 2^-53 of the sum of the absolute
    values of its terms, the JC entry's own rounding bound."""
    rng = np.random.default_rng(4)
    for rows, left, right, t in junk_cases(rng):
        L = rows.shape[1]
        jc = pa.likelihood_from_rows(rows, left, right, t)
        got = pa.model_likelihood_from_rows(rows, left, right, t, pa.SubstModel.jc69())
        assert np.array_equal(got.site_mant, jc.site_mant) and np.array_equal(got.site_exp, jc.site_exp)
        assert got.lnl == jc.lnl and got.missing_cells == jc.missing_cells and np.all(got.site_rate == 1.0)
        r = np.stack([pa.likelihood_from_rows(np.ascontiguousarray(rows[:, s:s + 1]), left, right, t, per_site=False).branch_g for s in range(L)])
        x = np.exp(-4.0 * jc.used_lengths() / 3.0)
        eps = 2.0 ** -53
        bound1 = 2 * L * eps * (4 * x / 3) * np.abs(r).sum(axis=0)
        bound2 = 2 * L * eps * ((16 * x * x / 9) * (r * r).sum(axis=0) + (16 * x / 9) * np.abs(r).sum(axis=0))
        assert np.all(np.abs(got.gradient() - jc.gradient()) <= bound1 + 1e-300)
        assert np.all(np.abs(got.curvature() - jc.curvature()) <= bound2 + 1e-300)


def test_24_leaves_against_the_unscaled_pruning(pa):
    rng = np.random.default_rng(3)
    n, L = 24, 48
    model = pa.SubstModel(UNEVEN, root=ROOT, rates=(0.3, 1.0, 2.2), weights=(0.3, 0.4, 0.3))
    for left, right in (ref.balanced(n), ref.caterpillar(n, rng.permutation(n)), ref.random_tree(n, rng)):
        t = lengths_for(rng, 2 * n - 1)
        rows = mref.evolve(left, right, np.full(2 * n - 1, 0.3), n, L, rng, UNEVEN, ROOT, 1.0)
        rows[rng.random((n, L)) < 0.05] = 0
        got = pa.model_likelihood_from_rows(rows, left, right, t, model)
        xs = mref.x_table(ref.clamp(t), model.rates, got.beta)
        cat = np.stack([mref.pruning(rows, left, right, xs[k], UNEVEN, ROOT) for k in range(3)])
        lik = model.weights @ cat
        for s in range(L):
            m, e = math.frexp(lik[s])
            assert abs(math.ldexp(got.site_mant[s], int(got.site_exp[s]) - e) - m) <= 1e-12 * m
        post = model.weights[:, None] * cat / lik
        assert np.allclose(got.site_rate, model.rates @ post, rtol=1e-12, atol=0)
        cls = rng.integers(0, 3, L).astype(np.uint8)
        one = pa.model_likelihood_from_rows(rows, left, right, t, pa.SubstModel(UNEVEN, ROOT, model.rates, model.weights, cls))
        mine = one.site_mant * 2.0 ** one.site_exp.astype(np.float64)
        assert np.allclose(mine, cat[cls, np.arange(L)], rtol=1e-12, atol=0) and np.array_equal(one.site_rate, model.rates[cls])


def test_a_640_leaf_caterpillar_against_exact_rationals(pa):
    n, L = 640, 3
    rng = np.random.default_rng(n)
    left, right = ref.caterpillar(n, rng.permutation(n))
    t = np.full(2 * n - 1, 10.0)
    t[rng.integers(0, 2 * n - 1, 40)] = 0.01
    rows = np.array(ref.BASES, np.uint8)[rng.integers(0, 4, (n, L))]
    model = pa.SubstModel.simulator()
    got = pa.model_likelihood_from_rows(rows, left, right, t, model, derivatives=False)
    x = mref.x_of(ref.clamp(t), 1.0, got.beta)
    assert np.all(mref.pruning(rows, left, right, x, model.freq, model.root) == 0.0)       # unscaled binary64 has underflowed
    for s in range(L):
        exact = mref.pruning_exact(rows[:, s].tolist(), left, right, x, model.freq, model.root)
        mine = Fraction(float(got.site_mant[s])) * Fraction(2) ** int(got.site_exp[s])
        assert abs(mine - exact) <= Fraction(1, 10 ** 12) * exact
        assert int(got.site_exp[s]) < -700
    assert np.isfinite(got.lnl) and got.lnl < -1000.0


def two_class_data(rng, n, L):
    left, right = ref.random_tree(n, rng)
    truth = rng.uniform(0.02, 0.4, 2 * n - 1)
    cls = (rng.random(L) < 0.5).astype(np.uint8)
    model = pa_model(cls)
    rows = mref.evolve(left, right, truth, n, L, rng, model.freq, model.root, model.rates[cls])
    return left, right, truth, model, rows


def pa_model(cls, **kw):
    import pansim_amd as pa
    return pa.SubstModel.simulator(rates=(0.5, 2.0), site_class=cls, **kw)


def test_the_optimiser_on_data_of_the_simulator_model_with_two_classes(pa):
    """a maximum lies at least as high as the generating lengths; rho != pi: both root branches are estimated.  The JC69 entry on
    the same data ends lower: the reference alone shows it (lnL of the model at the generating lengths, by unscaled pruning, is
    already above JC69's maximum as the existing reference optimiser finds it)."""
    rng = np.random.default_rng(31)
    n, L = 12, 4000
    left, right, truth, model, rows = two_class_data(rng, n, L)
    start = np.full(2 * n - 1, 0.1)
    got = pa.model_ml_lengths_from_rows(rows, left, right, start, model)
    at_truth = pa.model_likelihood_from_rows(rows, left, right, truth, model, per_site=False, derivatives=False).lnl
    assert got.lnl >= at_truth and got.converged and got.rounds >= 2
    assert np.all(np.diff(got.round_lnl) > 0) and got.round_lnl.size == got.rounds + 1 and got.lnl == got.round_lnl[-1]
    assert got.start_lnl == got.round_lnl[0] and got.passes >= got.rounds + got.rollbacks + 1
    rl, rr = int(left[-1]), int(right[-1])
    assert got.lengths[rr] != 1e-8 and got.lengths[rr] != start[rr] and got.lengths[rl] != start[rl] and got.lengths[-1] == 0.0
    # both root branches near the truth (4000 sites: a few per cent), which a folded root could not give
    assert abs(got.lengths[rr] - truth[rr]) < 0.25 * truth[rr] + 0.01 and abs(got.lengths[rl] - truth[rl]) < 0.25 * truth[rl] + 0.01
    again = pa.model_likelihood_from_rows(rows, left, right, got.lengths, model)
    assert again.lnl == got.lnl and np.all(again.curvature()[:-1] < 0.0)
    assert np.allclose(got.events(), got.lengths / (2.0 / 3.0), rtol=1e-15)
    text = got.newick()
    assert text.endswith(";\n") and text.count(",") == n - 1 and text.count(":") == 2 * n - 2
    # the reference computation alone: the model at the truth against the JC69 optimum
    beta = mref.beta_of(model.freq)
    cat = np.stack([mref.pruning(rows, left, right, mref.x_of(ref.clamp(truth), r, beta), model.freq, model.root) for r in model.rates])
    ref_truth = float(np.log(cat[model.site_class, np.arange(L)]).sum())
    ref_jc = ref.ml_lengths(rows, left, right, start)["lnl"]
    assert ref_truth > ref_jc + 10.0
    jc = pa.ml_lengths_from_rows(rows, left, right, start)
    assert got.lnl > jc.lnl + 10.0 and abs(at_truth - ref_truth) <= 1e-11 * abs(ref_truth)


def test_a_reversible_model_holds_the_right_root_branch(pa):
    rng = np.random.default_rng(32)
    n, L = 10, 600
    left, right = ref.random_tree(n, rng)
    rows = mref.evolve(left, right, rng.uniform(0.02, 0.4, 2 * n - 1), n, L, rng, UNEVEN, UNEVEN, 1.0)
    start = np.full(2 * n - 1, 0.1)
    rev = pa.model_ml_lengths_from_rows(rows, left, right, start, pa.SubstModel(UNEVEN, rates=(0.5, 2.0)))
    assert rev.lengths[int(right[-1])] == 1e-8 and rev.lengths[-1] == 0.0 and rev.converged and np.all(np.diff(rev.round_lnl) > 0)
    free = pa.model_ml_lengths_from_rows(rows, left, right, start, pa.SubstModel(UNEVEN, root=ROOT, rates=(0.5, 2.0)))
    assert free.lengths[int(right[-1])] != 1e-8 and free.lengths[int(left[-1])] != 1e-8


ROLLBACK_SEED, ROLLBACK_START = 0, 5.0


def test_the_optimiser_takes_the_rollback_path(pa):
    """the input of the JC69 rollback test -- the same tree, few sites, a start far off -- with the data drawn under the model"""
    rng = np.random.default_rng(ROLLBACK_SEED)
    n, L = 8, 60
    left, right = ref.random_tree(n, rng)
    cls = (np.arange(L) % 2).astype(np.uint8)
    model = pa_model(cls)
    rows = mref.evolve(left, right, rng.uniform(0.05, 1.5, 2 * n - 1), n, L, rng, model.freq, model.root, model.rates[cls])
    start = np.full(2 * n - 1, ROLLBACK_START)
    got = pa.model_ml_lengths_from_rows(rows, left, right, start, model, max_rounds=30, eps_lnl=1e-6)
    assert got.rollbacks >= 1 and got.passes == got.rounds + got.rollbacks + 1 and np.all(np.diff(got.round_lnl) > 0)
    assert got.lnl >= got.start_lnl and got.lnl == got.round_lnl[-1]
    capped = pa.model_ml_lengths_from_rows(rows, left, right, start, model, max_rounds=2, eps_lnl=1e-6)
    assert capped.rounds == 2 and not capped.converged and np.array_equal(capped.round_lnl, got.round_lnl[:3])


def test_start_lengths_from_changes(pa):
    for freq in (mref.JC, mref.SIM, UNEVEN):
        beta = mref.beta_of(freq)
        sites = 1000
        edge = int(math.ceil(0.98 * beta * sites))
        ch = [0, 100, 400, edge - 1, edge, 1000]
        got = pa.f81_lengths_from_changes(ch, sites, freq)
        want = [-beta * math.log(1 - (c / sites) / beta) if c < edge else 10.0 for c in ch]
        assert np.allclose(got, want, rtol=1e-14, atol=0) and got[0] == 0.0 and got[-2] == 10.0 and got[-3] < 10.0
    assert np.all(pa.f81_lengths_from_changes([0, 3], 0, mref.SIM) == 1e-8)
    assert np.allclose(pa.f81_lengths_from_changes([10, 50], 100, mref.JC), pa.jc_lengths_from_changes([10, 50], 100), rtol=1e-15)


@pytest.mark.parametrize("alpha", [0.1, 0.5, 1.0, 5.0])
@pytest.mark.parametrize("K", [2, 4, 8])
def test_gamma_rates(pa, alpha, K):
    rates = pa.gamma_rates(alpha, K)
    assert rates.size == K and np.all(np.diff(rates) > 0) and np.all(rates >= 0) and abs(rates.mean() - 1.0) <= 1e-12
    bounds = pa.gamma_bounds(alpha, K)
    assert bounds.size == K - 1 and np.all(np.diff(bounds) > 0)
    for i, b in enumerate(bounds, 1):
        assert abs(mref.gamma_p(alpha, alpha * b) - i / K) <= 1e-9, (alpha, K, i)
    # a category's rate lies between its bounds
    edges = np.concatenate([[0.0], bounds, [np.inf]])
    assert np.all(rates >= edges[:-1] * (1 - 1e-9)) and np.all(rates <= edges[1:] * (1 + 1e-9))
    try:
        from scipy import special
    except ImportError:
        special = None
    if special is not None:
        assert np.allclose(special.gammainc(alpha, alpha * bounds), np.arange(1, K) / K, rtol=0, atol=1e-9)
    model = pa.SubstModel.gamma(alpha, K)
    assert model.categories == K and np.allclose(model.weights, 1.0 / K) and model.site_class is None


def test_errors(pa):
    n = 5
    left, right = ref.caterpillar(n)
    rows = np.ones((n, 4), np.uint8)
    t = np.full(2 * n - 1, 0.1)
    ok = dict(freq=UNEVEN, root=ROOT, rates=(0.5, 2.0), weights=(0.5, 0.5))
    bad_models = [(dict(freq=(0.5, 0.5, 0.0, 0.0)), "freq may have at most one zero"),
                  (dict(freq=(-0.1, 0.4, 0.4, 0.3)), "freq[0]"),
                  (dict(freq=(0.1, 0.2, 0.3, 0.5)), "freq must sum to 1"),
                  (dict(freq=(np.nan, 0.2, 0.3, 0.5)), "freq[0]"),
                  (dict(root=(0.0, 0.5, 0.25, 0.25)), "root[0]"),
                  (dict(root=(0.3, 0.3, 0.3, 0.3)), "root must sum to 1"),
                  (dict(rates=(), weights=()), "categories must be 1 .. 8"),
                  (dict(rates=(-1.0, 1.0)), "rate[0]"),
                  (dict(rates=(1.0, np.inf)), "rate[1]"),
                  (dict(weights=(0.0, 1.0)), "weight[0]"),
                  (dict(weights=(0.6, 0.5)), "weight must sum to 1"),
                  (dict(site_class=[0, 1, 2, 0]), "site_class[2] = 2 is not below categories = 2"),
                  (dict(site_class=[0, 1, 0]), "site_class needs one entry per core site, site_classes = 4, not 3")]
    for change, text in bad_models:
        model = pa.SubstModel(**{**ok, **change})
        for call in (lambda: pa.model_likelihood_from_rows(rows, left, right, t, model),
                     lambda: pa.model_ml_lengths_from_rows(rows, left, right, t, model)):
            with pytest.raises(pa.PansimError) as e:
                call()
            assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        pa.SubstModel(UNEVEN, rates=np.ones(9))._c()
    with pytest.raises(ValueError):
        pa.SubstModel((0.5, 0.5))
    with pytest.raises(pa.PansimError) as e:
        pa.f81_lengths_from_changes([1], 10, (0.5, 0.5, 0.0, 0.0))
    assert e.value.code == PS_ERR_INVALID and "freq" in str(e.value)
    model = pa.SubstModel(**ok)
    for bad, text in ((np.nan, "length of node 2 is not a finite number"), (np.inf, "not a finite number")):
        tt = t.copy()
        tt[2] = bad
        for call in (lambda: pa.model_likelihood_from_rows(rows, left, right, tt, model),
                     lambda: pa.model_ml_lengths_from_rows(rows, left, right, tt, model)):
            with pytest.raises(pa.PansimError) as e:
                call()
            assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)
    with pytest.raises(pa.PansimError) as e:                 # a forest
        pa.model_likelihood_from_rows(rows, left[:-1], right[:-1], t[:-1], model)
    assert e.value.code == PS_ERR_INVALID and "spanning tree: 4 merges over 5 leaves, not 3" in str(e.value)
    for kw, text in ((dict(max_rounds=0), "max_rounds must be at least 1"), (dict(eps_lnl=0.0), "eps_lnl must be a positive number")):
        with pytest.raises(pa.PansimError) as e:
            pa.model_ml_lengths_from_rows(rows, left, right, t, model, **kw)
        assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)
    # N above either limit: the up pass to PS_LIK_MAX_POP, anything with derivatives to PS_MODEL_MAX_POP_DERIV
    big = pa.PS_LIK_MAX_POP + 1
    with pytest.raises(pa.PansimError) as e:
        pa.model_likelihood_from_rows(np.ones((big, 1), np.uint8), *ref.caterpillar(big), np.full(2 * big - 1, 0.1), model, derivatives=False)
    assert e.value.code == PS_ERR_INVALID and "pop_size <= 2048" in str(e.value)
    mid = pa.PS_MODEL_MAX_POP_DERIV + 1
    tree, tm, ones = ref.caterpillar(mid), np.full(2 * mid - 1, 0.1), np.ones((mid, 1), np.uint8)
    assert np.isfinite(pa.model_likelihood_from_rows(ones, *tree, tm, model, derivatives=False).lnl)
    for call in (lambda: pa.model_likelihood_from_rows(ones, *tree, tm, model), lambda: pa.model_ml_lengths_from_rows(ones, *tree, tm, model)):
        with pytest.raises(pa.PansimError) as e:
            call()
        assert e.value.code == PS_ERR_INVALID and "PS_MODEL_MAX_POP_DERIV = 1536" in str(e.value)
