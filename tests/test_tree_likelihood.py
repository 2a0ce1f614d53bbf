"""The host entries of the Jukes-Cantor likelihood of a tree (ps_likelihood_from_rows, ps_ml_lengths_from_rows,
ps_jc_lengths_from_changes; docs/TREE_LIKELIHOOD.md) against tests/tree_likelihood_ref.py; no device.

Tolerances.  A site likelihood is a sum of products of non-negative terms, so nothing cancels: a few dozen roundings of 1.1e-16
each, held to 1e-12 relative.  The derivative terms hold a difference (B = D - A), so their bound is absolute:
1e-10 sum_s (|A_s| + |A_s + B_s|) / l_s, A and A + B formed by the brute-force reference (the likelihood at x_c = 0 and at
x_c = 1); roundoff is about 100 * 2^-53 = 1e-14 of that scale and a wrong formula is off by the order of the scale itself.  For
h = sum r^2 the same per site, squared: |r| <= (|A| + |A + B|) / l."""
import math
import re
from fractions import Fraction

import numpy as np
import pytest

import tree_likelihood_ref as ref

PS_ERR_INVALID = -1
NAMES = ["ps_tree_likelihood", "ps_sim_tree_likelihood", "ps_multi_tree_likelihood", "ps_tree_ml_lengths", "ps_sim_tree_ml_lengths",
         "ps_multi_tree_ml_lengths", "ps_tree_likelihood_timing", "ps_likelihood_from_rows", "ps_ml_lengths_from_rows",
         "ps_jc_lengths_from_changes"]


def test_every_new_symbol_is_exported_and_declared(pa):
    import ctypes
    import os
    from pansim_amd import _lib
    lib = ctypes.CDLL(pa.LIB_PATH)
    hdr = open(os.path.join(os.path.dirname(pa.LIB_PATH), "..", "include", "pansim_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
    assert pa.PS_LIK_MAX_POP == 2048 and "#define PS_LIK_MAX_POP 2048u" in hdr
    assert ctypes.sizeof(_lib.Likelihood) == 12 * 8 and ctypes.sizeof(_lib.MlParams) == 16
    for cls in (pa.Population, pa.Simulation, pa.MultiSimulation):
        for method in ("tree_likelihood", "tree_ml_lengths", "tree_likelihood_timing"):
            assert callable(getattr(cls, method))


def small_cases():
    """every tree shape of 2 to 6 leaves (caterpillar and balanced among them) with permuted leaves, and random joinings"""
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


def test_site_likelihoods_and_derivatives_against_the_sum_over_all_assignments(pa):
    rng = np.random.default_rng(2)
    shapes_seen = 0
    for n, (left, right) in small_cases():
        shapes_seen += 1
        L, nodes = 6, 2 * n - 1
        rows = np.array(ref.BASES, np.uint8)[rng.integers(0, 4, (n, L))]
        rows[rng.random((n, L)) < 0.15] = rng.integers(0, 256, 1, dtype=np.uint8)[0]        # junk bytes: missing data
        rows[:, 0] = 4                                                                      # a monomorphic column
        t = lengths_for(rng, nodes)
        got = pa.likelihood_from_rows(rows, left, right, t)
        used = ref.clamp(t)
        x = ref.x_of(used)
        lik = np.array([ref.brute(rows[:, s], left, right, x) for s in range(L)])
        mine = got.site_mant * 2.0 ** got.site_exp.astype(np.float64)
        assert np.all(np.abs(mine - lik) <= 1e-12 * lik), (n, left, right)
        assert np.all((got.site_mant >= 0.125) & (got.site_mant < 1.0))
        assert abs(got.lnl - np.log(lik).sum()) <= 1e-12 * np.abs(np.log(lik)).sum() + 1e-13
        assert np.allclose(got.site_lnl, np.log(lik), rtol=1e-12, atol=1e-13)
        assert got.missing_cells == int((~np.isin(rows, ref.BASES)).sum()) and got.sites == L and got.pop_size == n
        assert got.clamped_lengths == int((used[:-1] != t[:-1]).sum()) and got.passes == 1 and got.rounds == 0
        assert got.tree_length == pytest.approx(used[:-1].sum(), rel=1e-14)
        grad, curv = got.gradient(), got.curvature()
        assert got.branch_g[-1] == 0.0 and got.branch_h[-1] == 0.0
        for c in range(nodes - 1):
            A = np.array([ref.brute(rows[:, s], left, right, x, branch=c, x_branch=0.0) for s in range(L)])
            AB = np.array([ref.brute(rows[:, s], left, right, x, branch=c, x_branch=1.0) for s in range(L)])
            d1 = np.array([ref.brute(rows[:, s], left, right, x, branch=c, order=1) for s in range(L)])
            d2 = np.array([ref.brute(rows[:, s], left, right, x, branch=c, order=2) for s in range(L)])
            scale_g = ((np.abs(A) + np.abs(AB)) / lik).sum()
            scale_h = (((np.abs(A) + np.abs(AB)) / lik) ** 2).sum()
            r = (AB - A) / lik
            assert abs(got.branch_g[c] - r.sum()) <= 1e-10 * scale_g, (n, c)
            assert abs(got.branch_h[c] - (r * r).sum()) <= 1e-10 * scale_h, (n, c)
            xc = x[c]
            assert abs(grad[c] - (d1 / lik).sum()) <= 1e-10 * (4 * xc / 3) * scale_g, (n, c)
            want2 = (d2 / lik - (d1 / lik) ** 2).sum()
            assert abs(curv[c] - want2) <= 1e-10 * ((16 * xc * xc / 9) * scale_h + (16 * xc / 9) * scale_g), (n, c)
    assert shapes_seen == sum(len(ref.shapes(n)) + 3 for n in range(2, 7)) and len(ref.shapes(6)) == 6


def test_24_leaves_against_the_unscaled_pruning(pa):
    rng = np.random.default_rng(3)
    n, L = 24, 64
    for left, right in (ref.balanced(n), ref.caterpillar(n, rng.permutation(n)), ref.random_tree(n, rng)):
        t = lengths_for(rng, 2 * n - 1)
        rows = ref.evolve(left, right, np.full(2 * n - 1, 0.3), n, L, rng)
        rows[rng.random((n, L)) < 0.05] = 0
        got = pa.likelihood_from_rows(rows, left, right, t)
        lik, r = ref.pruning(rows, left, right, ref.x_of(ref.clamp(t)), derivatives=True)
        for s in range(L):
            m, e = math.frexp(lik[s])
            # (mant, exp) of the entry against frexp of the reference: the same number up to 1e-12
            assert abs(math.ldexp(got.site_mant[s], int(got.site_exp[s]) - e) - m) <= 1e-12 * m
        assert np.allclose(got.branch_g[:-1], r.sum(axis=0)[:-1], rtol=0, atol=1e-10 * np.abs(r).sum(axis=0)[:-1].max() + 1e-300)
        assert np.allclose(got.branch_h[:-1], (r * r).sum(axis=0)[:-1], rtol=1e-9)


@pytest.mark.parametrize("n", [400, 640])
def test_a_long_caterpillar_whose_likelihood_the_exponents_carry(pa, n):
    rng = np.random.default_rng(n)
    L = 3
    left, right = ref.caterpillar(n, rng.permutation(n))
    t = np.full(2 * n - 1, 10.0)
    t[rng.integers(0, 2 * n - 1, 40)] = 0.01
    rows = np.array(ref.BASES, np.uint8)[rng.integers(0, 4, (n, L))]
    x = ref.x_of(ref.clamp(t))
    got = pa.likelihood_from_rows(rows, left, right, t)
    plain = ref.pruning(rows, left, right, x)
    if n == 640:
        assert np.all(plain == 0.0)                       # unscaled binary64 has underflowed: 4^-640 < 2^-1074
    for s in range(L):
        exact = ref.pruning_exact(rows[:, s].tolist(), left, right, x)
        mine = Fraction(float(got.site_mant[s])) * Fraction(2) ** int(got.site_exp[s])
        assert abs(mine - exact) <= Fraction(1, 10 ** 12) * exact
        assert int(got.site_exp[s]) < -700
    assert np.isfinite(got.lnl) and got.lnl < -1000.0 and np.all(np.isfinite(got.branch_g)) and np.all(np.isfinite(got.branch_h))


def test_plumbing_clamp_root_rule_and_special_columns(pa):
    rng = np.random.default_rng(5)
    n, L = 9, 40
    left, right = ref.random_tree(n, rng)
    nodes = 2 * n - 1
    rows = ref.evolve(left, right, np.full(nodes, 0.2), n, L, rng)
    t = rng.uniform(0.01, 0.5, nodes)
    base = pa.likelihood_from_rows(rows, left, right, t)
    assert base.clamped_lengths == 0 and base.missing_cells == 0
    # the clamp and its count: zero, negative and huge lengths go in as they are and are used at the bounds
    odd = t.copy()
    odd[0], odd[3], odd[n + 1] = 0.0, -0.25, 1e6
    bound = odd.copy()
    bound[0], bound[3], bound[n + 1] = 1e-8, 1e-8, 10.0
    a, b = pa.likelihood_from_rows(rows, left, right, odd), pa.likelihood_from_rows(rows, left, right, bound)
    assert a.clamped_lengths == 3 and b.clamped_lengths == 0 and a.lnl == b.lnl and np.array_equal(a.site_mant, b.site_mant)
    assert a.tree_length == b.tree_length
    # the root's entry is ignored, whatever it holds
    junk_root = t.copy()
    junk_root[-1] = np.nan
    assert pa.likelihood_from_rows(rows, left, right, junk_root).lnl == base.lnl
    # the root rule: only the sum of the two root branches is identified
    moved = t.copy()
    rl, rr = int(left[-1]), int(right[-1])
    moved[rl], moved[rr] = t[rl] + t[rr] - 0.004, 0.004
    assert abs(pa.likelihood_from_rows(rows, left, right, moved).lnl - base.lnl) <= 1e-12 * abs(base.lnl)
    # a monomorphic column, and an all-missing column whose likelihood is 1 exactly
    special = rows.copy()
    special[:, 0], special[:, 1] = 2, 0
    got = pa.likelihood_from_rows(special, left, right, t)
    assert got.site_mant[1] == 0.5 and got.site_exp[1] == 1 and got.site_lnl[1] == 0.0 and got.missing_cells == n
    mono = ref.brute(special[:, 0], left, right, ref.x_of(t)) if n <= 6 else ref.pruning(special[:, :1], left, right, ref.x_of(t))[0]
    assert abs(got.site_mant[0] * 2.0 ** int(got.site_exp[0]) - mono) <= 1e-12 * mono
    # without the optional outputs
    bare = pa.likelihood_from_rows(rows, left, right, t, per_site=False, derivatives=False)
    assert bare.lnl == base.lnl and bare.site_mant is None and bare.branch_g is None
    with pytest.raises(ValueError):
        bare.gradient()
    # start lengths from parsimony changes
    got = pa.jc_lengths_from_changes([0, 10, 50, 73, 74, 100], 100)
    want = [0.0, -0.75 * math.log(1 - 4 * 0.1 / 3), -0.75 * math.log(1 - 4 * 0.5 / 3), -0.75 * math.log(1 - 4 * 0.73 / 3), 10.0, 10.0]
    assert np.allclose(got, want, rtol=1e-15, atol=0)


def test_errors(pa):
    n = 5
    left, right = ref.caterpillar(n)
    rows = np.ones((n, 4), np.uint8)
    t = np.full(2 * n - 1, 0.1)
    for bad, text in ((np.nan, "length of node 2 is not a finite number"), (np.inf, "not a finite number")):
        tt = t.copy()
        tt[2] = bad
        for call in (lambda: pa.likelihood_from_rows(rows, left, right, tt), lambda: pa.ml_lengths_from_rows(rows, left, right, tt)):
            with pytest.raises(pa.PansimError) as e:
                call()
            assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)
    with pytest.raises(pa.PansimError) as e:                 # a forest
        pa.likelihood_from_rows(rows, left[:-1], right[:-1], t[:-1])
    assert e.value.code == PS_ERR_INVALID and "spanning tree: 4 merges over 5 leaves, not 3" in str(e.value)
    with pytest.raises(pa.PansimError) as e:
        pa.likelihood_from_rows(rows, [0] * 4, [1, 2, 3, 4], t)
    assert e.value.code == PS_ERR_INVALID and "a child of merge" in str(e.value)
    with pytest.raises(ValueError):
        pa.likelihood_from_rows(rows, left, right, t[:-1])
    for kw, text in ((dict(max_rounds=0), "max_rounds must be at least 1"), (dict(eps_lnl=0.0), "eps_lnl must be a positive number"),
                     (dict(eps_lnl=float("nan")), "eps_lnl must be a positive number")):
        with pytest.raises(pa.PansimError) as e:
            pa.ml_lengths_from_rows(rows, left, right, t, **kw)
        assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)
    big = pa.PS_LIK_MAX_POP + 1
    with pytest.raises(pa.PansimError) as e:
        pa.likelihood_from_rows(np.ones((big, 1), np.uint8), *ref.caterpillar(big), np.full(2 * big - 1, 0.1))
    assert e.value.code == PS_ERR_INVALID and "pop_size <= 2048" in str(e.value)


def same_path(got, want):
    assert (got.rounds, got.passes, got.rollbacks, got.converged) == (want["rounds"], want["passes"], want["rollbacks"], want["converged"])
    assert np.all(np.diff(got.round_lnl) > 0) and np.all(np.diff(want["round_lnl"]) > 0) and got.round_lnl.size == got.rounds + 1
    # the two pruning passes differ by roundoff only (1e-13 of lnL); a Newton step divides two sums of that accuracy
    assert np.allclose(got.round_lnl, want["round_lnl"], rtol=1e-11, atol=0)
    assert np.allclose(got.lengths, want["lengths"], rtol=1e-6, atol=1e-12)
    assert got.lnl == got.round_lnl[-1] and got.start_lnl == got.round_lnl[0] and got.lnl >= got.start_lnl


@pytest.mark.parametrize("seed", [11, 12])
def test_the_optimiser_reaches_above_the_generating_lengths(pa, seed):
    """a property of a maximum: lnL at the returned lengths is at least lnL at the lengths that generated the data"""
    rng = np.random.default_rng(seed)
    n, L = 16, 20000
    left, right = ref.random_tree(n, rng)
    truth = rng.uniform(0.02, 0.4, 2 * n - 1)
    rows = ref.evolve(left, right, truth, n, L, rng)
    start = np.full(2 * n - 1, 0.1)
    want = ref.ml_lengths(rows, left, right, start)
    got = pa.ml_lengths_from_rows(rows, left, right, start)
    same_path(got, want)
    at_truth = pa.likelihood_from_rows(rows, left, right, truth, per_site=False, derivatives=False).lnl
    ref_truth = float(np.log(ref.pruning(rows, left, right, ref.x_of(ref.clamp(truth)))).sum())
    assert want["lnl"] >= ref_truth and got.lnl >= at_truth and got.converged
    assert got.lengths[int(right[-1])] == 1e-8 and got.lengths[-1] == 0.0
    again = pa.likelihood_from_rows(rows, left, right, got.lengths, derivatives=True)
    assert again.lnl == got.lnl
    text = got.newick()
    assert text.endswith(";\n") and text.count(",") == n - 1 and text.count(":") == 2 * n - 2


def test_the_optimiser_takes_the_rollback_path(pa):
    """few sites, a start far off: a full Newton step on all branches at once overshoots and is halved"""
    rng = np.random.default_rng(ROLLBACK_SEED)
    n, L = 8, 60
    left, right = ref.random_tree(n, rng)
    rows = ref.evolve(left, right, rng.uniform(0.05, 1.5, 2 * n - 1), n, L, rng)
    start = np.full(2 * n - 1, ROLLBACK_START)
    want = ref.ml_lengths(rows, left, right, start, max_rounds=30, eps_lnl=1e-6)
    got = pa.ml_lengths_from_rows(rows, left, right, start, max_rounds=30, eps_lnl=1e-6)
    assert want["rollbacks"] >= 1 and got.rollbacks == want["rollbacks"]
    same_path(got, want)
    capped = pa.ml_lengths_from_rows(rows, left, right, start, max_rounds=2, eps_lnl=1e-6)
    assert capped.rounds == 2 and not capped.converged and np.array_equal(capped.round_lnl, got.round_lnl[:3])


ROLLBACK_SEED, ROLLBACK_START = 0, 5.0
