"""The host entry of the marginal ancestral states (ps_ancestral_from_rows; docs/ANCESTRAL_STATES.md) against
tests/ancestral_ref.py, the sum over all assignments of the internal nodes; no device.

Tolerances.  A node's posterior is a ratio of sums of products of non-negative terms: a few dozen roundings.  pdiff holds the one
difference A - S, whose absolute error is a few roundings of A <= the denominator / (1 - x): a few 1e-16 per site, absolute.  Both
sums over the sites are held to 1e-12 of the reference's own sum: node_conf is at least L / 4, and a branch_diff entry is carried
by the sites at which the branch's ends are likely to differ, where A - S does not cancel.  States are compared wherever the
reference's two largest posteriors differ by more than 1e-9 -- seven orders above the rounding of a posterior -- and the cells it
calls nearer than that are at most 1 % of every case: the committed seed was picked so that the reference alone says so (of the
seeds 0 .. 39, nine do; CASE_SEED is the first; `cases` asserts it again)."""
import re

import numpy as np
import pytest

import ancestral_ref as aref
import subst_model_ref as mref
import tree_likelihood_ref as ref

PS_ERR_INVALID = -1
NAMES = ["ps_tree_ancestral_states", "ps_sim_tree_ancestral_states", "ps_multi_tree_ancestral_states", "ps_ancestral_states_timing",
         "ps_ancestral_from_rows"]
UNEVEN = (0.1, 0.2, 0.3, 0.4)
ROOT = (0.4, 0.3, 0.2, 0.1)
CASE_SEED = 3
SITES = 8
GAP = 1e-9


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
    assert lib.ps_abi_version() == 3
    assert pa.PS_ANC_MAX_POP == 2304 and "#define PS_ANC_MAX_POP 2304u" in hdr
    assert pa.PS_ANC_MAX_POP_MIX == 1536 and "#define PS_ANC_MAX_POP_MIX 1536u" in hdr
    # 12 bytes per leaf, 36 per node (Mp = n) and 20 per merge of LDS, a mixture 32 more per merge, beside 336 static bytes: the
    # largest multiples of 256 under the CU's 160 KiB
    lds = lambda n, mix: 12 * n + 36 * n + (20 + 32 * mix) * (n - 1) + 336      # noqa: E731  (n a multiple of 16: n_pad = Mp = n)
    assert lds(2304, 0) == 156988 and lds(2304, 0) <= 160 * 1024 < lds(2560, 0)
    assert lds(1536, 1) == 153884 and lds(1536, 1) <= 160 * 1024 < lds(1792, 1)
    assert 12 * 1008 + 36 * 1000 + 20 * 999 == 68076             # (N = 1000: n_pad = 1008, Mp = 1000; two of them share a CU)
    assert ctypes.sizeof(_lib.Ancestral) == 12 * 8
    for cls in (pa.Population, pa.Simulation, pa.MultiSimulation):
        for method in ("ancestral_states", "ancestral_states_timing"):
            assert callable(getattr(cls, method))
    assert callable(pa.ancestral_from_rows) and callable(pa.AncestralStates.node_accuracy)


# --------------------------------------------------------------------------------------------------------- brute force
def models_for(pa, rng, L):
    """K in {1, 3 assigned, 4 mixture with a zero rate} under JC69, the simulator's law and pi without a zero"""
    r4, w4 = (0.0, 0.4, 1.0, 2.6), (0.1, 0.4, 0.3, 0.2)
    out = []
    for tag, freq, root in (("jc", mref.JC, mref.JC), ("sim", mref.SIM, mref.JC), ("uneven", UNEVEN, ROOT)):
        out.append((tag + " k1", pa.SubstModel(freq, root=root)))
        out.append((tag + " k3 assigned", pa.SubstModel(freq, root=root, rates=(0.5, 1.0, 2.0), site_class=rng.integers(0, 3, L))))
        out.append((tag + " k4 mixture", pa.SubstModel(freq, root=root, rates=r4, weights=w4)))
    return out


def lengths_for(rng, nodes):
    """lengths from below the lower bound to above the upper one, both bounds among them"""
    t = 10.0 ** rng.uniform(-9, 1.2, nodes)
    t[rng.integers(0, nodes)] = 1e-8
    t[rng.integers(0, nodes)] = 10.0
    return t


def cases(pa):
    """(tag, rows, left, right, t, model, reference): every tree shape of 2 to 6 leaves under every model; the bytes 0, 3 and
    255 among the bases and a column of base 1.  Asserted here, from the reference alone: at most 1 % of the cells of every case
    have their two largest posteriors within GAP."""
    rng = np.random.default_rng(CASE_SEED)
    models = models_for(pa, rng, SITES)
    out = []
    for n in range(2, 7):
        for shape in ref.shapes(n):
            left, right = ref.merges_of_shape(shape, rng.permutation(n))
            rows = np.array(ref.BASES, np.uint8)[rng.integers(0, 4, (n, SITES))]
            junk = rng.random((n, SITES)) < 0.12
            rows[junk] = np.array([0, 3, 255], np.uint8)[rng.integers(0, 3, int(junk.sum()))]
            rows[:, 0] = 1                                                                  # all base 1: the lost base
            t = lengths_for(rng, 2 * n - 1)
            for tag, model in models:
                want = aref.reconstruct(rows, left, right, t, model.freq, model.root, model.rates, model.weights, model.site_class)
                top = np.sort(want["node"], axis=-1)
                near = (top[..., 3] - top[..., 2] <= GAP) & (want["lik"] > 0)[:, None]
                assert near.sum() <= 0.01 * near.size, (n, tag, int(near.sum()))
                out.append(((n, tag), rows, left, right, t, model, want, near))
    return out


def close(got, want_terms, tag):
    """a sum over the sites against the reference's terms (L, entries): within 1e-12 of the reference's own sum"""
    want = want_terms.sum(axis=0)
    err = np.abs(got - want)
    assert np.all(err <= 1e-12 * want), (tag, float(err.max()), np.argwhere(err > 1e-12 * want)[:3], want)


def test_against_the_sum_over_all_assignments(pa):
    seen = 0
    for tag, rows, left, right, t, model, want, near in cases(pa):
        n, L = rows.shape
        got = pa.ancestral_from_rows(rows, left, right, t, model)
        assert got.rows.shape == (n - 1, L) and got.node_conf.shape == (n - 1,) and got.branch_diff.shape == (2 * n - 1,)
        assert got.sites == L and got.pop_size == n and got.merges == n - 1 and got.zero_sites == int((want["lik"] == 0).sum())
        assert got.missing_cells == int((~np.isin(rows, ref.BASES)).sum()) and got.masked_cells == 0
        used = ref.clamp(t)
        assert got.clamped_lengths == int((used[:-1] != t[:-1]).sum())
        assert got.categories == model.categories and got.classed == (model.site_class is not None)
        pmax = want["node"].max(axis=-1)                                      # (L, M)
        close(got.node_conf, pmax, tag)
        close(got.branch_diff, want["pdiff"], tag)
        assert got.branch_diff[-1] == 0.0
        assert got.total_diff == pytest.approx(got.branch_diff.sum(), rel=1e-15)
        counted = L - got.zero_sites
        assert got.mean_conf == pytest.approx(got.node_conf.sum() / ((n - 1) * counted), rel=1e-15)
        assert np.allclose(got.node_accuracy(), got.node_conf / counted, rtol=1e-15)
        best = np.array(ref.BASES, np.uint8)[want["node"].argmax(axis=-1)]    # (L, M)
        best[want["lik"] == 0] = 0
        agree = got.rows.T == best
        assert np.all(agree | near), (tag, np.argwhere(~(agree | near))[:4])
        assert np.all(np.isin(got.rows, (0,) + ref.BASES))
        lik = want["lik"]
        assert np.all(lik > 0) and abs(got.lnl - np.log(lik).sum()) <= 1e-12 * np.abs(np.log(lik)).sum() + 1e-13, tag
        seen += 1
    assert seen == sum(len(ref.shapes(n)) for n in range(2, 7)) * 9


def test_a_column_of_the_lost_base(pa):
    """base 1 has frequency 0 under the simulator's law: a column of base 1 can only be inherited, so every inner node is base 1
    for certain and no branch differs"""
    n = 5
    left, right = ref.caterpillar(n)
    t = np.array([0.1, 0.2, 0.3, 0.05, 0.4, 0.15, 0.25, 0.35, 0.0])
    got = pa.ancestral_from_rows(np.ones((n, 3), np.uint8), left, right, t, pa.SubstModel.simulator())
    assert np.all(got.rows == 1) and np.all(got.node_conf == 3.0) and np.all(got.branch_diff == 0.0) and got.mean_conf == 1.0


# --------------------------------------------------------------------------------------------------- other host checks
def test_the_site_likelihoods_are_the_model_entrys(pa):
    """each site's (mantissa, exponent) behind lnl: the entry called one column at a time returns ps_jc_site_ln of the site, the
    same function of the same pair as ps_model_likelihood_from_rows of that column, so the two are equal bit for bit; and the sum
    over all columns is the same sum in the same order"""
    rng = np.random.default_rng(11)
    n, L = 9, 24
    left, right = ref.random_tree(n, rng)
    t = lengths_for(rng, 2 * n - 1)
    rows = ref.evolve(left, right, np.full(2 * n - 1, 0.3), n, L, rng)
    rows[rng.random(rows.shape) < 0.05] = 255
    for tag, model in models_for(pa, rng, L):
        whole = pa.model_likelihood_from_rows(rows, left, right, t, model, derivatives=False)
        got = pa.ancestral_from_rows(rows, left, right, t, model)
        assert got.lnl == whole.lnl and got.missing_cells == whole.missing_cells and got.clamped_lengths == whole.clamped_lengths, tag
        for s in range(L):
            col, one = np.ascontiguousarray(rows[:, s:s + 1]), model.sliced(s, s + 1)
            mine = pa.ancestral_from_rows(col, left, right, t, one, states=False)
            theirs = pa.model_likelihood_from_rows(col, left, right, t, one, derivatives=False)
            # ln of (mant, exp) is injective enough: a different pair gives a different double except across an exact power of two
            assert mine.lnl == theirs.lnl == float(theirs.site_lnl[0]), (tag, s)
            assert mine.rows is None and mine.population is None


def test_an_exact_tie_goes_to_the_lowest_index(pa):
    """a cherry of two different bases with equal lengths under JC69: the root's posterior is the same binary64 number for both
    bases (the products commute), and the lower base wins"""
    left, right = np.array([0], np.uint32), np.array([1], np.uint32)
    t = np.array([0.2, 0.2, 0.0])
    for a, b in ((2, 8), (8, 2), (4, 1), (8, 4)):
        rows = np.array([[a], [b]], np.uint8)
        got = pa.ancestral_from_rows(rows, left, right, t, pa.SubstModel.jc69())
        want = aref.site(rows[:, 0], left, right, t, mref.JC, mref.JC, (1.0,), (1.0,))
        top = np.sort(want["node"][0])
        assert top[3] == top[2] and top[3] > top[1]                  # the reference ties too
        assert int(got.rows[0, 0]) == min(a, b)
        assert got.node_conf[0] == pytest.approx(top[3], rel=1e-14) and 0.25 < got.node_conf[0] < 0.5
    # four missing leaves' worth of nothing: the root's posterior is rho, all four equal, base 1 wins
    got = pa.ancestral_from_rows(np.zeros((2, 1), np.uint8), left, right, t, pa.SubstModel.jc69())
    assert int(got.rows[0, 0]) == 1 and got.node_conf[0] == 0.25 and got.missing_cells == 2


def test_min_posterior_masks_exactly_the_cells_below_it(pa):
    rng = np.random.default_rng(12)
    n, L = 7, 40
    left, right = ref.random_tree(n, rng)
    t = rng.uniform(0.2, 1.5, 2 * n - 1)
    model = pa.SubstModel.simulator(rates=(0.3, 1.0, 2.5), weights=(0.3, 0.4, 0.3))
    rows = mref.evolve(left, right, t, n, L, rng, model.freq, model.root, 1.0)
    plain = pa.ancestral_from_rows(rows, left, right, t, model)
    # pmax of every cell: node_conf of the one-column calls
    pmax = np.stack([pa.ancestral_from_rows(np.ascontiguousarray(rows[:, s:s + 1]), left, right, t, model).node_conf for s in range(L)])
    assert plain.masked_cells == 0 and np.all(plain.rows != 0) and 0.3 < pmax.min() < 0.9 < pmax.max()
    for cut in (0.0, 0.5, float(np.sort(pmax.reshape(-1))[17]), 0.9, 1.0):
        got = pa.ancestral_from_rows(rows, left, right, t, model, min_posterior=cut)
        below = (pmax < cut).T
        assert np.array_equal(got.rows == 0, below) and got.masked_cells == int(below.sum())
        assert np.array_equal(got.rows[~below], plain.rows[~below])
        assert np.array_equal(got.node_conf, plain.node_conf) and np.array_equal(got.branch_diff, plain.branch_diff)
        assert got.mean_conf == plain.mean_conf and got.lnl == plain.lnl
    # the threshold itself is not below it
    edge = float(pmax.reshape(-1)[5])
    assert pa.ancestral_from_rows(rows, left, right, t, model, min_posterior=edge).rows.T.reshape(-1)[5] != 0


def test_an_assigned_invariant_class_at_a_variable_site(pa):
    """rate 0 means x = 1 on every branch: a site whose leaves differ has likelihood 0 in that class -- byte 0 at every node,
    nothing added to any sum, counted in zero_sites; the same class at a constant site is certain of it"""
    n = 4
    left, right = ref.balanced(n)
    t = np.full(2 * n - 1, 0.3)
    rows = np.array([[2, 2, 4], [2, 4, 4], [2, 2, 4], [2, 8, 4]], np.uint8)
    cls = np.array([0, 0, 1], np.uint8)
    model = pa.SubstModel.simulator(rates=(0.0, 1.0), site_class=cls)
    got = pa.ancestral_from_rows(rows, left, right, t, model)
    assert got.zero_sites == 1 and got.masked_cells == 0 and got.lnl == -np.inf
    assert np.all(got.rows[:, 1] == 0) and np.all(got.rows[:, 0] == 2) and np.all(got.rows[:, 2] == 4)
    alone = pa.ancestral_from_rows(np.ascontiguousarray(rows[:, [0, 2]]), left, right, t, pa.SubstModel.simulator(rates=(0.0, 1.0), site_class=cls[[0, 2]]))
    assert np.array_equal(got.node_conf, alone.node_conf) and np.array_equal(got.branch_diff, alone.branch_diff)
    assert got.mean_conf == alone.mean_conf and np.array_equal(got.node_accuracy(), alone.node_accuracy()) and got.counted_sites() == 2
    assert np.all(alone.branch_diff[:n] >= 0.0) and alone.node_conf[0] > 1.9
    # as a mixture the invariant category only adds nothing at the variable site
    mix = pa.ancestral_from_rows(rows, left, right, t, pa.SubstModel.simulator(rates=(0.0, 1.0), weights=(0.4, 0.6)))
    assert mix.zero_sites == 0 and np.all(mix.rows != 0) and np.isfinite(mix.lnl)
    only = pa.ancestral_from_rows(np.ascontiguousarray(rows[:, 1:2]), left, right, t, pa.SubstModel.simulator())
    assert np.array_equal(mix.rows[:, 1], only.rows[:, 0])


def test_errors(pa):
    n = 5
    left, right = ref.caterpillar(n)
    rows = np.ones((n, 4), np.uint8)
    t = np.full(2 * n - 1, 0.1)
    model = pa.SubstModel(UNEVEN, root=ROOT, rates=(0.5, 2.0), weights=(0.5, 0.5))

    def fails(text, *args, **kw):
        with pytest.raises(pa.PansimError) as e:
            pa.ancestral_from_rows(*args, **kw)
        assert e.value.code == PS_ERR_INVALID and text in str(e.value), str(e.value)

    fails("spanning tree: 4 merges over 5 leaves, not 3", rows, left[:-1], right[:-1], t[:-1], model)
    for bad in (-0.1, 1.5, np.nan, np.inf):
        fails("min_posterior must be a number in [0, 1]", rows, left, right, t, model, min_posterior=bad)
    for bad in (np.nan, np.inf):
        tt = t.copy()
        tt[2] = bad
        fails("length of node 2 is not a finite number", rows, left, right, tt, model)
    fails("a child of merge", rows, [0] * 4, [1, 2, 3, 4], t, model)
    for change, text in ((dict(freq=(0.5, 0.5, 0.0, 0.0)), "freq may have at most one zero"), (dict(root=(0.0, 0.5, 0.25, 0.25)), "root[0]"),
                         (dict(rates=(-1.0, 1.0)), "rate[0]"), (dict(weights=(0.6, 0.5)), "weight must sum to 1"),
                         (dict(site_class=[0, 1, 2, 0]), "site_class[2] = 2 is not below categories = 2"),
                         (dict(site_class=[0, 1, 0]), "site_classes = 4, not 3")):
        fails(text, rows, left, right, t, pa.SubstModel(**{**dict(freq=UNEVEN, root=ROOT, rates=(0.5, 2.0), weights=(0.5, 0.5)), **change}))
    # N above the limit of the form in use: the message names the limit
    big = pa.PS_ANC_MAX_POP + 1
    one = pa.SubstModel.simulator()
    fails("pop_size <= PS_ANC_MAX_POP = 2304", np.ones((big, 1), np.uint8), *ref.caterpillar(big), np.full(2 * big - 1, 0.1), one)
    mid = pa.PS_ANC_MAX_POP_MIX + 1
    tree, tm, ones = ref.caterpillar(mid), np.full(2 * mid - 1, 0.1), np.ones((mid, 1), np.uint8)
    fails("pop_size <= PS_ANC_MAX_POP_MIX = 1536", ones, *tree, tm, model)
    ok = pa.ancestral_from_rows(ones, *tree, tm, one)                          # (one category: the assigned form's limit)
    assert ok.merges == mid - 1 and np.all(ok.rows == 1)
    assigned = pa.SubstModel(UNEVEN, root=ROOT, rates=(0.5, 2.0), site_class=[1])
    assert pa.ancestral_from_rows(ones, *tree, tm, assigned).classed


# --------------------------------------------------------------------------------------------------------- calibration
def test_the_confidences_are_calibrated(pa):
    """a random 16-leaf tree with 0.05 to 0.3 events per site per branch, 2000 sites evolved under the simulator's law: the share
    of the 15 x 2000 inner cells reconstructed correctly lies within 4 sigma of mean_conf, and the true number of branch-end
    differences within 4 sigma of total_diff; sigma from the posteriors themselves, sqrt(sum p (1 - p)), a Bernoulli sum (the
    cells of a site are correlated, but a site's cells share their 2000th of the sum)"""
    rng = np.random.default_rng(2024)
    n, L = 16, 2000
    left, right = ref.random_tree(n, rng)
    model = pa.SubstModel.simulator()
    t = rng.uniform(0.05, 0.3, 2 * n - 1) * model.beta                        # events per site -> substitutions per site
    leaves, inner = aref.evolve(left, right, t, n, L, rng, model.freq, model.root, 1.0)
    got = pa.ancestral_from_rows(leaves, left, right, t, model)
    assert got.zero_sites == 0 and got.masked_cells == 0 and got.sites == L
    cols = [pa.ancestral_from_rows(np.ascontiguousarray(leaves[:, s:s + 1]), left, right, t, model, states=False) for s in range(L)]
    pmax = np.stack([c.node_conf for c in cols])                              # (L, M)
    pdiff = np.stack([c.branch_diff for c in cols])[:, :-1]                   # (L, nodes - 1)
    correct = int((got.rows == inner).sum())
    sigma = np.sqrt((pmax * (1.0 - pmax)).sum())
    print("correct", correct, "expected", got.mean_conf * 15 * L, "sigma", sigma)
    assert abs(correct - got.mean_conf * 15 * L) <= 4.0 * sigma and 0.5 < got.mean_conf < 0.999
    states = np.concatenate([leaves, inner])
    parent = np.zeros(2 * n - 1, np.int64)
    parent[left], parent[right] = np.arange(n, 2 * n - 1), np.arange(n, 2 * n - 1)
    differ = int((states[:-1] != states[parent[:-1]]).sum())
    sigma_d = np.sqrt((pdiff * (1.0 - pdiff)).sum())
    print("differences", differ, "expected", got.total_diff, "sigma", sigma_d)
    assert abs(differ - got.total_diff) <= 4.0 * sigma_d and got.total_diff > 0.0
