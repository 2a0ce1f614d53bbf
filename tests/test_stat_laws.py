"""The closed forms of tests/stat_laws.py on the CPU: the integer tables of the oracle and of the library's host side lie within
the bounds DESIGN.md states of them (3.2, 3.3, 3.6) at every plan the GPU conformance test covers, the statistics of that test
see a wrong level-2 table at the size a CPU run affords, and every statistic function is right on a hand-countable case."""
import math
from fractions import Fraction

import numpy as np
import pytest

import stat_laws as sl

L_TEST = 100000            # the global number of sites of tests/test_gpu_stat_conformance.py


def _plan_rates(pa, name):
    flags, levels, shape = sl.WORKLOAD_PLANS[name]
    p = pa.make_params(**flags)
    d = pa.derive(p)
    lm, lh = sl.scaled_rates(p.core_size, d.n_core_mutations, d.n_recombinations_core, L_TEST)
    return lm, lh, levels, shape


def _assert_classes(impl, p, q, R, what):
    """every implemented class mass, and every cumulative one, within 2^-32 R / 64 of the closed form (f64 rounding of the
    closed form itself: 2^-50)"""
    want = [Fraction(x) for x in sl.core_classes(p, q)]
    bound = sl.plan_bound(R) + Fraction(1, 1 << 50)
    for j in range(7):
        assert abs(impl[j] - want[j]) <= bound, (what, j, float(impl[j]), float(want[j]))
        assert abs(sum(impl[:j + 1]) - sum(want[:j + 1])) <= bound, (what, "cumulative", j)


# ----------------------------------------------------------------------------- integers against the closed form
@pytest.mark.parametrize("name", [n for n, v in sl.WORKLOAD_PLANS.items() if v[1] is None])
def test_uniform_plans_lie_within_the_stated_bound(pa, orc, name):
    lm, lh, _, shape = _plan_rates(pa, name)
    p, q = sl.core_pq(lm, lh, L_TEST)
    assert sl.core_plan_shape(p, q) == shape
    plan = orc.core_plan(lm, lh, L_TEST)
    assert (plan.k, plan.R, plan.cshift) == shape
    _assert_classes(sl.plan_classes(plan.k, plan.R, list(plan.T)), p, q, plan.R, "oracle " + name)
    t = pa.site_tables(True, L_TEST, [lm], [lh], np.ones(L_TEST, np.float32))
    assert t["ranges"] and (t["k"], t["R"], t["cshift"]) == shape
    assert (t["thresholds"] == t["thresholds"][0]).all()
    _assert_classes(sl.plan_classes(t["k"], t["R"], t["thresholds"][0]), p, q, t["R"], "library " + name)
    # what the GPU test's power assertion rests on: the share of the mutation mass that only level 2 decides
    if name == "cfg2":
        share = sl.level2_mutation_share(plan.k, p, q)
        assert abs(share - 0.00177) < 5e-6 and abs(share / p - 0.036) < 5e-4


def test_weighted_plan_lies_within_the_stated_bound(pa):
    lm, lh, levels, shape = _plan_rates(pa, "weighted")
    w, idx = sl.level_weights(levels, L_TEST)
    p_s, q = sl.weighted_core_pq([lm], [lh], w)
    assert sl.weighted_plan_shape(p_s, q) == shape and shape[0] == 0 and shape[1] >= 5
    t = pa.site_tables(True, L_TEST, [lm], [lh], w)
    assert not t["ranges"] and (t["k"], t["R"], t["cshift"]) == shape
    for lv in range(len(levels)):
        sites = np.nonzero(idx == lv)[0]
        T = t["thresholds"][sites]
        assert (T == T[0]).all()
        _assert_classes(sl.plan_classes(0, t["R"], T[0]), float(p_s[sites[0]]), q, t["R"], "level %d" % lv)
        if levels[lv] == 0.0:
            assert (T[:, :6] == 0).all()              # a site of weight 0 never mutates, and still receives
            assert T[0, 6] > 0


def test_flip_thresholds_and_weight_quantisation_lie_within_their_bounds(pa, orc):
    G = 6000
    cb, ce, lam = [0, 5400], [5400, 6000], [5400.0, 600000.0]          # cfg2's per-gene rates 1 and 1000 at G = 6000
    mask = np.zeros((2, G), np.float32)
    mask[0, :5400] = 1
    mask[1, 5400:] = 1
    t = pa.site_tables(False, G, lam, [0.0, 0.0], mask, mask)
    for c in range(2):
        want = sl.p_flip(lam[c], ce[c] - cb[c])
        thr = t["thresholds"][cb[c]:ce[c]]
        assert (thr == thr[0]).all() and int(thr[0]) == orc.lib().orc_acc_flip_threshold(lam[c], ce[c] - cb[c])
        assert 0 <= Fraction(want) - Fraction(int(thr[0]), sl.TWO32) <= Fraction(1, sl.TWO32)
    # weighted flips: every gene's own threshold
    rng = np.random.default_rng(3)
    wm = rng.random((1, G)).astype(np.float32)
    wm[0, ::7] = 0.0
    wr = np.asarray([1.0, 10.0, 100.0, 1000.0], np.float32)[np.arange(G) % 4].reshape(1, G)
    wr[0, ::9] = 0.0
    t = pa.site_tables(False, G, [5400.0], [27000.0], wm, wr)
    pf = -np.expm1(-2.0 * sl.site_rates([5400.0], wm)) / 2.0
    err = pf - t["thresholds"].astype(np.float64) / sl.TWO32
    assert (err >= -2.0 ** -50).all() and (err <= 2.0 ** -32 + 2.0 ** -50).all()
    assert (t["thresholds"][::7] == 0).all()
    # HGT weights (3.6): half a step of the u16 scale, a positive weight at least 1, a zero weight 0
    wq = t["hgt_weights"][0].astype(np.float64)
    assert np.array_equal(wq, sl.hgt_quantise(wr[0]))
    x = wr[0].astype(np.float64) / float(wr[0].max())
    assert (np.abs(wq / 65535.0 - x) <= sl.HGT_QUANT_STEP * (1.0 + 1e-12)).all()
    assert ((wq == 0) == (wr[0] == 0)).all()
    present = np.arange(G) % 3 == 0
    rel = sl.hgt_quant_bound(wr[0], present)
    P = present & (wr[0] > 0)
    law = np.where(P, wr[0], 0.0) / wr[0][P].sum()
    got = np.where(P, wq, 0.0) / wq[P].sum()
    assert (np.abs(got - law)[P] <= (rel * law)[P]).all() and (rel[~P] == 0).all()
    assert rel[P].max() < 0.02


# ----------------------------------------------------------------------------- the detector detects
def _report(what, n, prob, count, z, z_pred=None):
    print("%-40s n %.4g expected %.6g observed %d z %+.2f%s" % (what, n, n * prob, count, z, "" if z_pred is None else "  predicted %+.2f" % z_pred))


def test_a_wrong_level2_mutation_table_is_detected(orc):
    """The marginal statistics of the GPU test on the oracle's mutate_core at 200 x 20000 cells: the true cfg2 plan passes; a
    copy with T[0..2] zeroed moves the level-2 mutate-only mass (0.00177) to the class above it, 'mutate to C and receive' --
    which mutate_alleles shows as C.  So the hit rate does not move and the alleles do: C gains 2/3 of that mass, G and T lose
    1/3 each (z about +19, -9, -9); the observed z follow the prediction from the edited integers."""
    N, L, lam = 200, 20000, 1000.0
    n = N * L
    plan = orc.core_plan(lam, 0.0, L)
    assert (plan.k, plan.R) == (1, 1)
    p, q = sl.core_pq(lam, 0.0, L)
    law = sl.mutate_law(sl.core_classes(p, q))
    bad = type(plan).from_buffer_copy(plan)
    for j in range(3):
        bad.T[j] = 0
    assert list(plan.T)[:3] != [0, 0, 0] and list(bad.T)[3:] == list(plan.T)[3:]
    shifted = [float(x) for x in sl.mutate_law(sl.plan_classes(bad.k, bad.R, list(bad.T)))]
    share = sl.level2_mutation_share(plan.k, p, q)
    assert abs(shifted[0] - law[0] - 2.0 * share / 3.0) < 1e-9 and abs(shifted[1] - law[1] + share / 3.0) < 1e-9
    fails = 0
    for gen, pl, true_plan in ((0, plan, True), (1, bad, False)):
        m = orc.mutate_core(np.ones((N, L), np.uint8), 0, 123, gen, pl)
        for j, v in enumerate((2, 4, 8)):
            count = int((m == v).sum())
            z = sl.z_binomial(count, n, law[j])
            z_pred = n * (shifted[j] - law[j]) / math.sqrt(n * law[j] * (1.0 - law[j]))
            _report("mutate %s allele %d" % ("true" if true_plan else "edited", v), n, law[j], count, z, None if true_plan else z_pred)
            if true_plan:
                assert abs(z) <= 5.0
            else:
                assert abs(z_pred) > 9.0 and abs(z - z_pred) <= 5.0
                fails += abs(z) > 5.0
        if true_plan:
            assert abs(sl.z_binomial(int((m != 1).sum()), n, p)) <= 5.0
    assert fails == 3


def test_a_halved_receive_threshold_is_detected(orc):
    """recombine_core with T[6] halved: half of the receive mass is gone.  The rate is the smallest (by doubling) at which the
    per-block tallies of this size resolve a relative error of one half at |z| = 15."""
    N, L, n_own = 200, 20000, (150, 50)
    rate = 1.0e-6
    while max(sl.resolution(n_own[b] * L, sl.event_prob(rate) * n_own[1 - b] / (N - 1), 15.0) for b in (0, 1)) > 0.5:
        rate *= 2.0
    plan = orc.core_plan(0.0, rate * L, L)
    q = sl.event_prob(rate)
    assert (plan.k, plan.R) == (0, 1) and list(plan.T)[:6] == [0] * 6
    bad = type(plan).from_buffer_copy(plan)
    bad.T[6] = plan.T[6] // 2
    q_bad = float(sl.receive_prob(sl.plan_classes(bad.k, bad.R, list(bad.T))))
    assert abs(q_bad / q - 0.5) < 1e-6
    m0 = np.ones((N, L), np.uint8)
    m0[n_own[0]:] = 2
    for gen, pl, true_plan in ((0, plan, True), (1, bad, False)):
        m = orc.recombine_core(m0.copy(), 0, 77, gen, pl)
        for b, rows in enumerate((slice(0, n_own[0]), slice(n_own[0], N))):
            n = n_own[b] * L
            prob = q * n_own[1 - b] / (N - 1)
            count = int((m[rows] != m0[rows]).sum())
            z = sl.z_binomial(count, n, prob)
            z_pred = n * (q_bad - q) * n_own[1 - b] / (N - 1) / math.sqrt(n * prob * (1.0 - prob))
            _report("recombine %s block %d" % ("true" if true_plan else "edited", b), n, prob, count, z, None if true_plan else z_pred)
            if true_plan:
                assert abs(z) <= 5.0
            else:
                assert z_pred <= -7.5 and abs(z - z_pred) <= 5.0 and abs(z) > 5.0


# ----------------------------------------------------------------------------- the statistics on hand-countable cases
def test_statistics_on_hand_countable_cases():
    assert sl.z_binomial(60, 100, 0.5) == pytest.approx(2.0)                    # (60 - 50) / sqrt(25)
    assert sl.z_joint(30, 400, 0.5, 0.1) == pytest.approx(10.0 / math.sqrt(400 * 0.05 * 0.95))
    assert sl.resolution(10000, 0.5, 5.0) == pytest.approx(0.05)                # 5 sqrt(0.5 / 5000)
    # z_lag: X = 1 1 0 1 1 1, lag 1: products 1 0 0 1 1 -> 3 of n = 5 pairs, 4 couples of pairs share a cell
    x = np.array([1, 1, 0, 1, 1, 1])
    both = int((x[:-1] & x[1:]).sum())
    assert both == 3
    var = 5 * 0.25 * 0.75 + 2 * 4 * (0.125 - 0.0625)
    assert sl.z_lag(both, 5, 4, 0.5) == pytest.approx((3 - 1.25) / math.sqrt(var))
    # ... and that variance is the exact one: all 2^6 arrays, equally likely
    tot = [sum(((a >> i) & 1) * ((a >> (i + 1)) & 1) for i in range(5)) for a in range(64)]
    assert np.var(tot) == pytest.approx(var)
    # z_dispersion: totals 0 and 2 of Binomial(2, 1/2): sum of squares 2 against 2 * 1/2, variance 2 (mu4 - mu2^2) = 2 * 1/4
    assert sl.z_dispersion([0, 2], 2, 0.5) == pytest.approx((2.0 - 1.0) / math.sqrt(0.5))
    sq = [(bin(a).count("1") - 1.0) ** 2 for a in range(4)]
    assert np.mean(sq) == pytest.approx(0.5) and np.var(sq) == pytest.approx(0.25)
    # chi-square: (12 - 10)^2 / 10 + (8 - 10)^2 / 10; with an allowance of 1 per cell the deviations shrink to 1
    assert sl.chi2_statistic([12, 8, 5], [10, 10, 0]) == (pytest.approx(0.8), 2)
    assert sl.chi2_statistic([12, 8], [10, 10], systematic=[1, 1])[0] == pytest.approx(0.2)
    assert sl.chi2_statistic([12, 8], [10, 10], var=[5, 5])[0] == pytest.approx(1.6)
    assert sl.chi2_tail(2.0, 2) == pytest.approx(math.exp(-1.0), rel=1e-9 if _has_scipy() else 0.05)     # df 2: exp(-x / 2)
    for x, df in ((2.0, 2), (30.0, 10), (1200.0, 999), (1300.0, 999)):
        exact = _chi2_sf_even(x, df) if df % 2 == 0 else None
        wh = sl.chi2_tail_wilson_hilferty(x, df)
        if exact is not None:
            assert wh == pytest.approx(exact, rel=0.12)
        assert abs(math.log(wh / sl.chi2_tail(x, df))) < 0.15
    # with_systematic: 3 sigma of 10 counts = 30, less an allowance of 100 * 0.1 = 10 -> 2 sigma; never below 0
    assert sl.with_systematic(-3.0, 100, 10.0, 0.1) == pytest.approx(-2.0)
    assert sl.with_systematic(0.5, 100, 10.0, 0.1) == 0.0


def _has_scipy():
    try:
        import scipy.stats  # noqa: F401
        return True
    except ImportError:
        return False


def _chi2_sf_even(x, df):
    """exact tail for even df: exp(-x / 2) sum_{i < df / 2} (x / 2)^i / i!"""
    return math.exp(-x / 2.0) * sum((x / 2.0) ** i / math.factorial(i) for i in range(df // 2))


def test_laws_on_hand_countable_cases():
    # p = q = 1/2: a = 1/12, b = 1/12, c = 1/4
    cl = sl.core_classes(0.5, 0.5)
    assert cl == pytest.approx([1 / 12] * 6 + [0.25])
    assert sl.mutate_law(cl) == pytest.approx([1 / 6] * 3) and sl.receive_prob(cl) == pytest.approx(0.5)
    # a plan of k = 1, R = 2 with the word cut at 1/4, 1/2, 3/4 and nothing else: 1/64 + 2/64 * 1/4 per allele
    T = [sl.TWO32 // 4, sl.TWO32 // 2, 3 * sl.TWO32 // 4] + [3 * sl.TWO32 // 4] * 4
    assert sl.plan_classes(1, 2, T) == [Fraction(3, 128)] * 3 + [0] * 4
    assert sl.plan_bound(2) == Fraction(1, 32 * sl.TWO32)
    # two blocks of 3 A and 2 C, HR only with q = 1/2: an A cell turns C with 1/2 * 2/4, a C cell turns A with 1/2 * 3/4
    only_hr = sl.core_classes(0.0, 0.5)
    assert sl.block_law(only_hr, 1, 2, 3, 2, mutate=False)[2] == pytest.approx(0.25)
    assert sl.block_law(only_hr, 2, 1, 2, 3, mutate=False)[1] == pytest.approx(0.375)
    # fused, p = q = 1/2: an A cell ends as A iff nothing happens to it (1/4) or it receives -- mutated or not -- the allele of
    # an unmutated A donor (1/2 * 2/4 * 1/2)
    law = sl.block_law(cl, 1, 2, 3, 2)
    assert law[1] == pytest.approx(0.25 + 0.5 * 0.5 * 0.5) and sum(law.values()) == pytest.approx(1.0)
    assert law[4] == pytest.approx(1 / 6) and law[8] == pytest.approx(1 / 6)        # G and T only ever come from a mutation: p / 3
    # site rates: weights 1, 3 with lam 2 -> 1/2, 3/2
    assert sl.site_rates([2.0], [1.0, 3.0]) == pytest.approx([0.5, 1.5])
    assert sl.p_flip(1.0, 2) == pytest.approx((1 - math.exp(-1.0)) / 2)
    # HGT: donor 0 carries genes 0, 1 of 3; N = 3, lam = 2: each of its genes at rate 2 / 2 / 2 per recipient
    rate, prob = sl.hgt_gain_law([[1, 1, 0], [0, 0, 0], [0, 0, 0]], 2.0)
    assert rate == pytest.approx([0.5, 0.5, 0.0]) and prob[0] == pytest.approx(1 - math.exp(-0.5))
    mean, var = sl.hgt_expected_gains([[1, 1, 0], [0, 0, 0], [0, 0, 0]], prob)
    assert mean == pytest.approx(4 * prob[0]) and var == pytest.approx(4 * prob[0] * (1 - prob[0]))
    rate, _ = sl.hgt_gain_law([[1, 1, 0], [0, 0, 0], [0, 0, 0]], 2.0, weights=[1.0, 3.0, 5.0])
    assert rate == pytest.approx([0.25, 0.75, 0.0])
    assert list(sl.hgt_quantise([0.0, 1e-9, 0.5, 1.0])) == [0.0, 1.0, 32768.0, 65535.0]
