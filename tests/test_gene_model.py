"""The host entries of the gene gain / loss model (ps_gene_likelihood_from_rows, ps_gene_ancestral_from_rows,
ps_gene_fit_from_rows; docs/GENE_MODEL.md) against tests/gene_model_ref.py -- the sum over all assignments of the inner nodes with
explicit 2 x 2 matrices in the gain / loss parametrisation -- and the fit and the calibration on data the reference evolved; no
device.

Tolerances.  A gene's likelihood, its class posteriors, a node's posterior and a branch's two joints are sums, products and ratios
of non-negative terms on both sides (the library carries 1 - x as -expm1, the reference its off-diagonal entries likewise): a few
dozen roundings each, so 1e-12 relative holds with three orders to spare.  States are compared wherever the reference's
|p_1 - 1/2| > 1e-9; CASE_SEED is the first seed for which the reference alone finds no nearer cell in any case (`cases` asserts it
again)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import gene_model_ref as gref

PS_ERR_INVALID = -1
NAMES = ["ps_tree_gene_likelihood", "ps_sim_tree_gene_likelihood", "ps_multi_tree_gene_likelihood", "ps_tree_gene_ancestral",
         "ps_sim_tree_gene_ancestral", "ps_multi_tree_gene_ancestral", "ps_tree_gene_fit", "ps_sim_tree_gene_fit", "ps_multi_tree_gene_fit",
         "ps_tree_gene_timing", "ps_gene_likelihood_from_rows", "ps_gene_ancestral_from_rows", "ps_gene_fit_from_rows"]
CASE_SEED = 0
GENES = 12
GAP = 1e-9
RTOL = 1e-12


def test_every_new_symbol_is_exported_and_declared(pa):
    from pansim_amd import _lib
    lib = ctypes.CDLL(pa.LIB_PATH)
    hdr = open(os.path.join(os.path.dirname(pa.LIB_PATH), "..", "include", "pansim_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
        comment = " ".join(hdr[:re.search(r"\bint %s\s*\(" % name, hdr).start()].rsplit("/*", 1)[1].replace("\n *", " ").split())
        assert "the reference has no such function" in comment and "population.rs:505" in comment, name
    assert lib.ps_abi_version() == 3
    assert pa.PS_GENE_MAX_POP == 2304 and "#define PS_GENE_MAX_POP 2304u" in hdr
    assert pa.PS_GENE_MAX_POP_MIX == 1792 and "#define PS_GENE_MAX_POP_MIX 1792u" in hdr
    # (n a multiple of 256: n_pad = Mp = n, W = Wm = n / 64) two f64 and one i32 per node, two f64 per slot, two per merge (a
    # mixture: two more), the leaf and the state words; 512 bytes kept for static LDS: the largest multiples of 256 under 160 KiB
    lds = lambda n, mix: 20 * n + 16 * (2 * n - 1) + (16 + 16 * mix) * (n - 1) + 2 * 8 * (n // 64)      # noqa: E731
    assert lds(2304, 0) == 157216 and lds(2304, 0) + 512 <= 160 * 1024 < lds(2560, 0)
    assert lds(1792, 1) == 150928 and lds(1792, 1) + 512 <= 160 * 1024 < lds(2048, 1)
    assert ctypes.sizeof(_lib.GeneSummary) == 18 * 8 and ctypes.sizeof(_lib.GeneFitParams) == 24
    for cls in (pa.Population, pa.Simulation, pa.MultiSimulation):
        for method in ("tree_gene_likelihood", "tree_gene_ancestral", "tree_gene_fit", "tree_gene_timing"):
            assert callable(getattr(cls, method))
    assert b"gene_team" in [pa.load().ps_tuning_key(k) for k in range(64)] and '"gene_team"' in hdr


# --------------------------------------------------------------------------------------------------------- brute force
def gain_loss(freq, rates):
    """the model's classes in the reference's parametrisation, from the definitions alone"""
    beta = 1.0 - freq[0] ** 2 - freq[1] ** 2
    return [r * freq[1] / beta for r in rates], [r * freq[0] / beta for r in rates]


def models_for(pa, rng, G):
    """K in {1, 3 assigned, 4 mixture with a zero rate} under pi = (1/2, 1/2) and (0.8, 0.2), rho != pi"""
    out = []
    for tag, freq, root in (("half", (0.5, 0.5), (0.3, 0.7)), ("uneven", (0.8, 0.2), (0.45, 0.55))):
        out.append((tag + " k1", pa.GeneModel(freq, root=root, rates=(0.7,))))
        out.append((tag + " k3 assigned", pa.GeneModel(freq, root=root, rates=(0.2, 1.0, 30.0), gene_class=rng.integers(0, 3, G))))
        out.append((tag + " k4 mixture", pa.GeneModel(freq, root=root, rates=(0.0, 0.4, 1.0, 2.6), weights=(0.1, 0.4, 0.3, 0.2))))
    return out


def lengths_for(rng, nodes):
    """lengths from below the lower clamp to 1e4, the clamp itself among them"""
    t = 10.0 ** rng.uniform(-10, 4, nodes)
    t[rng.integers(0, nodes)] = 1e-8
    t[-1] = 0.0
    return t


def rows_for(rng, n, G):
    rows = (rng.random((n, G)) < 0.5).astype(np.uint8)
    rows[:, 0] = 0                       # absent everywhere
    rows[:, 1] = 1                       # present everywhere
    rows[:, 2] = rng.integers(2, 256, n)  # any byte but 0 is present
    return rows


def ref_of(rows, left, right, lengths, model, method=gref.brute):
    g, l = gain_loss(model.freq, model.rates)
    used = np.maximum(lengths, 1e-8)
    return gref.reference(rows, left, right, used, g, l, model.root, model.weights, model.gene_class, method)


@pytest.fixture(scope="module")
def cases(pa):
    """every tree shape of 2 to 6 leaves x the six models: (tag, rows, left, right, lengths, model, reference)"""
    rng = np.random.default_rng(CASE_SEED)
    out = []
    for n in range(2, 7):
        for s, (left, right) in enumerate(gref.tree_shapes(n)):
            rows, lengths = rows_for(rng, n, GENES), lengths_for(rng, 2 * n - 1)
            for tag, model in models_for(pa, rng, GENES):
                out.append(("n%d shape%d %s" % (n, s, tag), rows, left, right, lengths, model, ref_of(rows, left, right, lengths, model)))
    assert [len(gref.tree_shapes(n)) for n in range(2, 7)] == [1, 1, 2, 3, 6]
    near = [np.sum((np.abs(c[6]["p1"] - 0.5) <= GAP) & np.isfinite(c[6]["lnl_g"])) for c in out]
    assert sum(near) == 0, "CASE_SEED leaves cells within %g of a tie" % GAP
    return out


def close(a, b, rtol=RTOL):
    return np.all(np.abs(a - b) <= rtol * np.abs(b))


def test_the_host_likelihood_matches_the_sum_over_all_assignments(pa, cases):
    for tag, rows, left, right, lengths, model, ref in cases:
        r = pa.gene_likelihood_from_rows(rows, left, right, lengths, model)
        lnl = r.gene_lnl()
        zero = ~np.isfinite(ref["lnl_g"])
        assert np.array_equal(zero, ~np.isfinite(lnl)) and r.zero_genes == zero.sum(), tag
        assert np.all(np.abs(lnl[~zero] - ref["lnl_g"][~zero]) <= RTOL), tag            # (ln: relative in the likelihood)
        assert close(r.gene_post[~zero], ref["post"][~zero]), tag
        assert close(r.gene_rate[~zero], ref["post"][~zero] @ model.rates, 1e-12), tag
        if zero.any():
            assert r.lnl == -np.inf, tag
        else:
            assert abs(r.lnl - ref["lnl_g"].sum()) <= 1e-12 * np.abs(ref["lnl_g"]).sum(), tag
        assert r.clamped_lengths == np.sum(lengths[:-1] < 1e-8) and r.categories == model.categories, tag
        assert r.classed == (model.gene_class is not None), tag


def test_the_host_reconstruction_matches_the_sum_over_all_assignments(pa, cases):
    for tag, rows, left, right, lengths, model, ref in cases:
        a = pa.gene_ancestral_from_rows(rows, left, right, lengths, model)
        p1, has = ref["p1"], np.isfinite(ref["lnl_g"])
        conf = np.where(has, np.maximum(p1, 1.0 - p1), 0.0)
        assert close(a.node_conf, conf.sum(1)) and close(a.node_genes, p1.sum(1)), tag
        assert close(a.branch_gains, ref["gains"].sum(1)) and close(a.branch_losses, ref["losses"].sum(1)), tag
        assert close(a.gene_gains, ref["gains"].sum(0)) and close(a.gene_losses, ref["losses"].sum(0)), tag
        assert np.array_equal(a.rows, (p1 > 0.5).astype(np.uint8)), tag                  # (no cell is within GAP of a tie: `cases`)
        assert abs(a.total_gains - ref["gains"].sum()) <= 1e-12 * ref["gains"].sum() + 1e-300, tag
        assert a.zero_genes == (~has).sum(), tag
        lik = pa.gene_likelihood_from_rows(rows, left, right, lengths, model)
        assert a.lnl == lik.lnl or (np.isinf(a.lnl) and np.isinf(lik.lnl)), tag
        none = pa.gene_ancestral_from_rows(rows, left, right, lengths, model, states=False)
        assert none.rows is None and np.array_equal(none.node_conf, a.node_conf), tag


def test_the_pruning_reference_is_the_brute_force_reference(pa, cases):
    """the large-tree form of the reference, used below, against the sum over all assignments"""
    for tag, rows, left, right, lengths, model, ref in cases[::7]:
        fast = ref_of(rows, left, right, lengths, model, gref.pruning)
        has = np.isfinite(ref["lnl_g"])
        assert np.allclose(fast["lnl_g"][has], ref["lnl_g"][has], rtol=0, atol=1e-10) and np.array_equal(has, np.isfinite(fast["lnl_g"])), tag
        for key in ("post", "p1", "gains", "losses"):
            assert np.allclose(fast[key], ref[key], rtol=1e-9, atol=1e-13), (tag, key)


# -------------------------------------------------------------------------------------------------------- single cases
def test_an_exact_tie_is_absent(pa):
    """a 0 / 1 cherry with equal lengths under pi = (1/2, 1/2) and rho = pi: p_0 == p_1 bit for bit at the root"""
    m = pa.GeneModel((0.5, 0.5))
    for t in (1e-8, 0.1, 0.37, 5.0):
        a = pa.gene_ancestral_from_rows(np.array([[0], [1]], np.uint8), [0], [1], [t, t, 0.0], m)
        assert a.rows[0, 0] == 0 and a.node_conf[0] == 0.5 and a.node_genes[0] == 0.5
        b = pa.gene_ancestral_from_rows(np.array([[1], [0]], np.uint8), [0], [1], [t, t, 0.0], m)
        assert b.rows[0, 0] == 0 and b.node_conf[0] == 0.5
        assert abs(a.branch_gains.sum() - 0.5) < 1e-15 and abs(a.branch_losses.sum() - 0.5) < 1e-15


def test_an_assigned_zero_rate_class_at_a_variable_gene_is_ln_zero_and_counted(pa):
    rows = np.array([[0, 1, 1], [1, 1, 0], [1, 1, 0]], np.uint8)
    m = pa.GeneModel((0.5, 0.5), rates=(0.0, 1.0), gene_class=(0, 0, 1))
    r = pa.gene_likelihood_from_rows(rows, [0, 3], [1, 2], [0.1, 0.2, 0.3, 0.1, 0.0], m)
    assert r.lnl == -np.inf and r.zero_genes == 1 and r.gene_mant[0] == 0.0 and abs(r.gene_lnl()[1] - math.log(0.5)) < 1e-15
    a = pa.gene_ancestral_from_rows(rows, [0, 3], [1, 2], [0.1, 0.2, 0.3, 0.1, 0.0], m)
    assert a.zero_genes == 1 and np.array_equal(a.rows[:, 0], [0, 0]) and a.gene_gains[0] == 0.0 and a.gene_losses[0] == 0.0
    assert np.array_equal(a.rows[:, 1], [1, 1]) and a.gene_gains[1] == 0.0          # (the invariant class never changes)
    assert abs(a.mean_conf - (a.node_conf.sum() / (2 * 2))) < 1e-15


def test_all_absent_and_all_present_genes(pa):
    left, right, t = [0, 3], [1, 2], [0.3, 0.2, 0.5, 0.1, 0.0]
    m = pa.GeneModel((0.6, 0.4), root=(0.5, 0.5), rates=(0.8,))
    a = pa.gene_ancestral_from_rows(np.array([[0, 1]] * 3, np.uint8), left, right, t, m)
    assert np.array_equal(a.rows, [[0, 1], [0, 1]]) and a.node_genes.sum() > 0.0
    ref = ref_of(np.array([[0, 1]] * 3, np.uint8), np.array(left), np.array(right), np.array(t), m)
    assert close(a.node_genes, ref["p1"].sum(1)) and close(a.gene_gains, ref["gains"].sum(0))


def test_the_gain_loss_round_trip(pa):
    m = pa.GeneModel.from_gain_loss((0.02, 0.5), (0.06, 1.5), weights=(0.7, 0.3))
    assert abs(m.freq[1] - 0.25) < 1e-15 and abs(m.freq.sum() - 1.0) < 1e-15
    gain, loss = m.gain_loss()
    assert np.allclose(gain, (0.02, 0.5), rtol=1e-14) and np.allclose(loss, (0.06, 1.5), rtol=1e-14)
    assert np.allclose(m.rates, 2.0 * gain * loss / (gain + loss), rtol=1e-14)
    with pytest.raises(ValueError):
        pa.GeneModel.from_gain_loss((0.02, 0.5), (0.06, 0.5))
    mix = pa.GeneModel((0.5, 0.5), rates=(1.0, 2.0), gene_class=(0, 0, 0, 1)).mixture()
    assert mix.gene_class is None and np.allclose(mix.weights, (0.75, 0.25))


def test_the_simulator_model(pa):
    prm = pa.make_params(pop_size=32, core_size=1000, pan_genes=600, core_genes=200, seed=5)
    m = pa.GeneModel.simulator(prm)
    d = pa.derive(prm)
    assert m.gene_class.size == d.pan_size and tuple(m.freq) == (0.5, 0.5) and m.categories == d.n_comp
    for c in range(d.n_comp):
        size = d.comp_end[c] - d.comp_begin[c]
        assert m.rates[c] == d.n_pan_mutations[c] / size and np.all(m.gene_class[d.comp_begin[c]:d.comp_end[c]] == c)
        # the simulator's flip probability is this model's off-diagonal entry over one generation
        P = gref.transition(*[v[c] for v in m.gain_loss()], 1.0)
        assert abs(P[0, 1] - (1.0 - math.exp(-2.0 * d.n_pan_mutations[c] / size)) / 2.0) < 1e-15
    assert 0.0 < m.root[1] < 1.0 and abs(m.root.sum() - 1.0) < 1e-15


def test_every_error_names_its_field(pa):
    rows = np.zeros((3, 2), np.uint8)
    left, right, t = [0, 3], [1, 2], [0.1] * 4 + [0.0]
    ok = dict(freq=(0.5, 0.5), root=(0.5, 0.5), rates=(1.0, 2.0), weights=(0.5, 0.5))

    def fails(words, lengths=t, rows=rows, left=left, right=right, **change):
        with pytest.raises(pa.PansimError) as e:
            pa.gene_likelihood_from_rows(rows, left, right, lengths, pa.GeneModel(**{**ok, **change}))
        assert e.value.code == PS_ERR_INVALID and all(w in str(e.value) for w in words), str(e.value)

    fails(["freq[0]", "> 0"], freq=(0.0, 1.0))
    fails(["freq[1]", "> 0"], freq=(1.0, 0.0))
    fails(["freq", "sum to 1"], freq=(0.5, 0.6))
    fails(["root[1]", "> 0"], root=(1.0, 0.0))
    fails(["root", "sum to 1"], root=(0.5, 0.4))
    fails(["rate[1]", ">= 0"], rates=(1.0, -1.0))
    fails(["rate[0]", "finite"], rates=(np.inf, 1.0))
    fails(["weight[0]", "> 0"], weights=(0.0, 1.0))
    fails(["weight", "sum to 1"], weights=(0.5, 0.6))
    fails(["categories", "1 .. 8"], rates=(), weights=())
    fails(["gene_class", "gene_classes = 2"], gene_class=(0, 1, 0))
    fails(["gene_class[1] = 2", "categories = 2"], gene_class=(0, 2))
    fails(["length of node 1", "finite"], lengths=[0.1, np.nan, 0.1, 0.1, 0.0])
    fails(["spanning tree"], left=[0], right=[1], lengths=[0.1] * 4)
    big = np.zeros((pa.PS_GENE_MAX_POP_MIX + 1, 1), np.uint8)
    chain = (np.r_[0, np.arange(big.shape[0], 2 * big.shape[0] - 2)], np.arange(1, big.shape[0]))
    fails(["PS_GENE_MAX_POP_MIX = 1792"], rows=big, left=chain[0], right=chain[1], lengths=np.full(2 * big.shape[0] - 1, 0.1))
    with pytest.raises(pa.PansimError) as e:
        pa.gene_fit_from_rows(rows, left, right, t, pa.GeneModel(**ok), eps_lnl=0.0)
    assert "eps_lnl" in str(e.value)
    with pytest.raises(pa.PansimError) as e:
        pa.gene_fit_from_rows(rows, left, right, t, pa.GeneModel(**ok), max_rounds=0)
    assert "max_rounds" in str(e.value)


# -------------------------------------------------------------------------------------------------------------- the fit
FIT_SEED = 11
FIT_RATES, FIT_WEIGHTS, FIT_PI1, FIT_RHO1 = (0.3, 3.0), (0.8, 0.2), 0.3, 0.4
EPS = 1e-3


def chi2_quantile(df, p):
    """x with P(df / 2, x / 2) = p, from the incomplete gamma function of pansim_amd/models.py"""
    from pansim_amd.models import _gamma_p
    lo, hi = 0.0, 1.0
    while _gamma_p(df / 2.0, hi / 2.0) < p:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _gamma_p(df / 2.0, mid / 2.0) < p else (lo, mid)
    return hi


@pytest.fixture(scope="module")
def fit_data():
    """a random 64-leaf tree and 4000 genes the reference evolved under two classes"""
    rng = np.random.default_rng(FIT_SEED)
    left, right = gref.random_tree(rng, 64)
    lengths = np.r_[rng.uniform(0.02, 0.4, 126), 0.0]
    cls = (rng.random(4000) < FIT_WEIGHTS[1]).astype(np.uint8)
    g, l = gain_loss((1.0 - FIT_PI1, FIT_PI1), FIT_RATES)
    rows = np.zeros((64, 4000), np.uint8)
    for k in (0, 1):
        rows[:, cls == k] = gref.evolve(rng, left, right, lengths, g[k], l[k], FIT_RHO1, int((cls == k).sum()))[0]
    return left, right, lengths, cls, rows


def truth_of(pa, cls):
    return pa.GeneModel((1.0 - FIT_PI1, FIT_PI1), root=(1.0 - FIT_RHO1, FIT_RHO1), rates=FIT_RATES, weights=FIT_WEIGHTS, gene_class=cls)


@pytest.mark.parametrize("mixture", [False, True])
def test_the_fit_reaches_the_truth(pa, fit_data, mixture):
    left, right, lengths, cls, rows = fit_data
    truth = truth_of(pa, None if mixture else cls)
    ref = ref_of(rows, left, right, lengths, truth, gref.pruning)
    lnl_truth = ref["lnl_g"].sum()
    start = pa.GeneModel((0.5, 0.5), root=truth.root, rates=(0.5, 2.0) if mixture else (1.0, 1.0), weights=(0.5, 0.5), gene_class=truth.gene_class)
    f = pa.gene_fit_from_rows(rows, left, right, lengths, start, max_rounds=60, eps_lnl=EPS)
    print("fit", "mixture" if mixture else "assigned", f.model.rates, f.model.weights, f.model.freq, f.lnl, lnl_truth, f.rounds, f.passes)
    assert f.converged and f.round_lnl.size == f.rounds + 1 and f.round_lnl[0] == f.start_lnl and f.round_lnl[-1] == f.lnl
    assert np.all(np.diff(f.round_lnl) >= 0.0)
    assert f.lnl >= lnl_truth - EPS
    params = 4 if mixture else 3
    assert 2.0 * (f.lnl - lnl_truth) < chi2_quantile(params, 1.0 - 1e-6)
    assert abs(f.model.freq.sum() - 1.0) <= 1e-12 and abs(f.model.weights.sum() - 1.0) <= 1e-12
    assert np.array_equal(f.model.root, truth.root)
    # the returned lnL is the returned model's
    again = pa.gene_likelihood_from_rows(rows, left, right, lengths, f.model)
    assert abs(again.lnl - f.lnl) <= 1e-9 * abs(f.lnl)
    # a fit started from the fit stays
    g = pa.gene_fit_from_rows(rows, left, right, lengths, f.model, max_rounds=60, eps_lnl=EPS)
    assert 0.0 <= g.lnl - f.lnl < EPS
    if mixture:
        # the genes' largest posterior class against their true class: no worse than the reference's own posteriors under the
        # true parameters, less four sigma of that binomial
        share_ref = np.mean(np.argmax(ref["post"], axis=1) == cls)
        got = np.mean(again.gene_best_class() == cls)
        sigma = math.sqrt(share_ref * (1.0 - share_ref) / cls.size)
        print("classified", got, share_ref, sigma)
        assert got >= share_ref - 4.0 * sigma
    else:
        unfitted = pa.gene_fit_from_rows(rows, left, right, lengths, start, fit_rates=False, fit_freq=False, max_rounds=3, eps_lnl=EPS)
        assert unfitted.lnl == unfitted.start_lnl and np.array_equal(unfitted.model.rates, start.rates)


# ------------------------------------------------------------------------------------------------------ calibration
CAL_SEED = 2


def test_the_posteriors_are_calibrated(pa):
    """16 leaves, 3000 genes evolved by the reference: the cells reconstructed correctly against the summed confidence, the true
    gains and losses against the expected ones"""
    rng = np.random.default_rng(CAL_SEED)
    left, right = gref.random_tree(rng, 16)
    lengths = np.r_[rng.uniform(0.05, 0.6, 30), 0.0]
    pi1, rho1, rate = 0.35, 0.5, 1.2
    g, l = gain_loss((1.0 - pi1, pi1), (rate,))
    rows, inner, tg, tl = gref.evolve(rng, left, right, lengths, g[0], l[0], rho1, 3000)
    model = pa.GeneModel((1.0 - pi1, pi1), root=(1.0 - rho1, rho1), rates=(rate,))
    ref = ref_of(rows, left, right, lengths, model, gref.pruning)
    pmax = np.maximum(ref["p1"], 1.0 - ref["p1"])
    sigma = math.sqrt((pmax * (1.0 - pmax)).sum())

    def calibrated(states, conf, gg, gl):
        ok = abs(float((states == inner).sum()) - conf) <= 4.0 * sigma
        for true, got in ((tg, gg), (tl, gl)):
            d = true - got
            ok = ok and abs(d.sum()) <= 4.0 * math.sqrt(((d - d.mean()) ** 2).sum())
        return ok

    assert calibrated((ref["p1"] > 0.5).astype(np.uint8), pmax.sum(), ref["gains"].sum(0), ref["losses"].sum(0)), "CAL_SEED: the reference itself"
    a = pa.gene_ancestral_from_rows(rows, left, right, lengths, model)
    assert calibrated(a.rows, a.node_conf.sum(), a.gene_gains, a.gene_losses)
