"""Per-site rate weights, CPU side: the new entries are declared, bound and wrapped; the host-only tables equal the
independent restatement's exactly; contiguous 0/1 masks are the ps_set_rates path; validation; and the restated dense form
conforms to the law and to the reference's event-driven algorithm.  Bounds are binomial / chi-square ones: 5 sigma per cell of
a count table, chi-square below its mean + 5 standard deviations (df + 5 sqrt(2 df))."""
import math
import os
import re

import numpy as np
import pytest

import site_weights_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _weight_cases(cols, rng):
    smooth = (1.0 + 0.8 * np.sin(np.arange(cols) / 7.0)).astype(np.float32)
    spiky = np.full(cols, 0.01, np.float32)
    spiky[rng.integers(0, cols, max(1, cols // 20))] = 50.0
    zeros = rng.random(cols).astype(np.float32)
    zeros[rng.random(cols) < 0.4] = 0.0
    return {"smooth": smooth, "spiky": spiky, "zeros": zeros}


# ----------------------------------------------------------------------------- surface
def test_entries_are_declared_bound_and_wrapped(pa):
    from pansim_amd import _lib
    header = open(os.path.join(ROOT, "include", "pansim_hip.h")).read()
    lib = pa.load()
    for name in ("ps_set_site_rates", "ps_site_tables", "ps_sim_set_site_weights", "ps_multi_set_site_weights"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert callable(pa.Population.set_site_rates) and callable(pa.Simulation.set_site_weights) and callable(pa.site_tables)
    assert int(re.search(r"#define PS_MAX_SITE_COMP (\d+)", header).group(1)) >= 8
    assert lib.ps_abi_version() == 3


# ----------------------------------------------------------------------------- tables
@pytest.mark.parametrize("L,lam_mut,lam_rec", [(257, [3.0], [1.0]), (1000, [40.0], [0.0]), (64, [30.0], [20.0]), (500, [0.0], [5.0])])
def test_core_tables_equal_the_restatement(pa, L, lam_mut, lam_rec):
    rng = np.random.default_rng(L)
    for name, w in _weight_cases(L, rng).items():
        t = pa.site_tables(True, L, lam_mut, lam_rec, w)
        R, cshift, T = ref.core_tables(lam_mut, lam_rec, w)
        assert not t["ranges"] and t["k"] == 0, name
        assert (t["R"], t["cshift"]) == (R, cshift), name
        assert t["has_events"] == (1 if R else 0)
        assert np.array_equal(t["thresholds"], T), name
        assert (np.diff(T.astype(np.int64), axis=1) >= 0).all()
        if lam_mut[0] > 0:
            assert (T[w == 0, 2] == 0).all()          # a site of weight 0 never mutates


def test_core_tables_with_several_compartments(pa):
    L = 300
    rng = np.random.default_rng(5)
    w = np.stack(list(_weight_cases(L, rng).values()))
    lam_mut, lam_rec = [2.0, 0.0, 7.5], [0.5, 0.25, 0.0]
    t = pa.site_tables(True, L, lam_mut, lam_rec, w)
    R, cshift, T = ref.core_tables(lam_mut, lam_rec, w)
    assert (t["k"], t["R"], t["cshift"]) == (0, R, cshift)
    assert np.array_equal(t["thresholds"], T)


@pytest.mark.parametrize("G,lam_mut", [(130, [1.0]), (700, [2.0, 0.3, 5.0]), (64, [0.0, 1.0])])
def test_accessory_tables_equal_the_restatement(pa, G, lam_mut):
    rng = np.random.default_rng(G)
    cases = list(_weight_cases(G, rng).values())
    n = len(lam_mut)
    wm = np.stack([cases[c % 3] for c in range(n)])
    wr = np.stack([cases[(c + 1) % 3] for c in range(n)])
    t = pa.site_tables(False, G, lam_mut, [1.0] * n, wm, wr)
    flip, wq = ref.acc_tables(lam_mut, wm, wr)
    assert not t["ranges"]
    assert np.array_equal(t["thresholds"], flip)
    assert np.array_equal(t["hgt_weights"], wq)
    assert ((wq == 0) == (wr == 0)).all() and int(wq.max()) == 65535
    # the quantisation bound DESIGN.md states: within half a step of 65535 w / wmax, a positive weight at least 1
    for c in range(n):
        x = 65535.0 * wr[c].astype(np.float64) / float(wr[c].max())
        assert (np.abs(wq[c] - x)[wr[c] > 0] <= np.maximum(0.5, 1.0 - x[wr[c] > 0])).all()


def test_contiguous_masks_are_the_ranges_path(pa, orc):
    L = 12000
    t = pa.site_tables(True, L, [600.0], [30.0], np.ones(L, np.float32))
    plan = orc.core_plan(600.0, 30.0, L)
    assert t["ranges"] and (t["k"], t["R"], t["cshift"]) == (plan.k, plan.R, plan.cshift)
    assert np.array_equal(t["thresholds"], np.tile(np.array(list(plan.T), np.uint32), (L, 1)))
    # a partial range on the core matrix is NOT ps_set_rates (which mutates every site): it stays weighted
    part = np.zeros(L, np.float32)
    part[100:200] = 1
    assert not pa.site_tables(True, L, [600.0], [30.0], part)["ranges"]
    G = 300
    m = np.zeros((2, G), np.float32)
    m[0, :100] = 1
    m[1, 100:] = 1
    t = pa.site_tables(False, G, [1.0, 2.0], [5.0, 6.0], m, m)
    assert t["ranges"]
    lib = orc.lib()
    lib.orc_acc_flip_threshold.restype = np.ctypeslib.ctypes.c_uint32
    lib.orc_acc_flip_threshold.argtypes = [np.ctypeslib.ctypes.c_double, np.ctypeslib.ctypes.c_uint64]
    assert (t["thresholds"][:100] == lib.orc_acc_flip_threshold(1.0, 100)).all()
    assert (t["thresholds"][100:] == lib.orc_acc_flip_threshold(2.0, 200)).all()
    assert np.array_equal(t["hgt_weights"], m.astype(np.uint16))
    # ... and the weighted arithmetic agrees with the ranges' on such masks (2 lam / n either way)
    flip, _ = ref.acc_tables([1.0, 2.0], m, m)
    assert np.array_equal(flip, t["thresholds"])
    # overlapping masks, or different masks for the two operators, are weighted
    m2 = m.copy()
    m2[1, 50:] = 1
    assert not pa.site_tables(False, G, [1.0, 2.0], [5.0, 6.0], m2, m2)["ranges"]
    assert not pa.site_tables(False, G, [1.0, 2.0], [5.0, 6.0], m, m2)["ranges"]


def test_validation_messages(pa):
    L = 50
    w = np.ones(L, np.float32)
    for bad, msg in ((-1.0, "negative or not finite"), (np.nan, "negative or not finite"), (np.inf, "negative or not finite")):
        v = w.copy()
        v[7] = bad
        with pytest.raises(pa.PansimError, match=msg):
            pa.site_tables(True, L, [1.0], [0.0], v)
    with pytest.raises(pa.PansimError, match="all zero"):
        pa.site_tables(True, L, [1.0], [0.0], np.zeros(L, np.float32))
    with pytest.raises(pa.PansimError, match="recombination weights of compartment 1 are all zero"):
        pa.site_tables(False, L, [1.0, 1.0], [1.0, 1.0], np.ones((2, L), np.float32), np.stack([w, 0 * w]))
    pa.site_tables(False, L, [0.0], [0.0], np.zeros((1, L), np.float32), np.zeros((1, L), np.float32))   # rate 0: nothing is drawn
    with pytest.raises(pa.PansimError, match="n_comp must be 1..8"):
        pa.site_tables(True, L, [1.0] * 9, [0.0] * 9, np.ones((9, L), np.float32))
    with pytest.raises(pa.PansimError, match="needs recombination weights"):
        pa.site_tables(False, L, [1.0], [1.0], w)
    with pytest.raises(pa.PansimError, match="finite and >= 0"):
        pa.site_tables(True, L, [-1.0], [0.0], w)


def test_restated_philox_is_the_oracles(orc):
    for ctr, seed in (((0, 0, 0, 0), 0), ((1, 2, 3, 4), 0x123456789ABCDEF), ((0xFFFFFFFF, 7, 21, 5), 42)):
        want = orc.philox(ctr, (seed & 0xFFFFFFFF, seed >> 32))
        assert [int(x) for x in ref.philox(*ctr, seed)] == [int(x) for x in want]


# ----------------------------------------------------------------------------- the dense form against the law
def _chi2_ok(obs, exp):
    keep = exp > 0
    df = int(keep.sum()) - 1
    chi2 = float((((obs - exp) ** 2)[keep] / exp[keep]).sum())
    return chi2 <= df + 5.0 * math.sqrt(2.0 * df), chi2, df


def test_core_mutation_counts_follow_the_per_site_law():
    L, N, gens, lam = 16, 1024, 20, [3.0, 1.0]
    w = np.stack([np.arange(1, L + 1), (np.arange(L) % 4 == 0) * 1.0]).astype(np.float32)
    w[0, 5] = 0.0
    w[1, 5] = 0.0
    R, _, T = ref.core_tables(lam, [0.0, 0.0], w)
    p = -np.expm1(-ref.site_rates(lam, w))
    counts = np.zeros(L)
    alleles = np.zeros(3)
    for g in range(gens):
        pop = ref.core_mutate(np.ones((N, L), np.uint8), 0, 99, g, R, T)
        counts += (pop != 1).sum(0)
        alleles += [(pop == v).sum() for v in (2, 4, 8)]
    trials = N * gens
    sigma = np.sqrt(trials * p * (1 - p))
    assert (trials * p)[p > 0].min() >= 20
    assert (np.abs(counts - trials * p) <= 5 * sigma).all(), (counts, trials * p)
    assert counts[5] == 0
    assert _chi2_ok(alleles, np.full(3, alleles.sum() / 3))[0]          # uniform over {2, 4, 8}


def test_core_recombination_stays_uniform_over_sites():
    L, N, gens = 12, 1024, 20
    w = np.arange(1, L + 1).astype(np.float32)
    R, _, T = ref.core_tables([2.0], [3.0], w)
    q = -math.expm1(-3.0 / L)
    pop0 = np.ones((N, L), np.uint8)
    pop0[::2] = 2                        # a donor differs from the recipient with probability 512 / 1023
    counts = np.zeros(L)
    for g in range(gens):
        counts += (ref.core_recombine(pop0.copy(), 0, 7, g, R, T) != pop0).sum(0)
    trials, pr = N * gens, q * 512.0 / 1023.0
    assert (np.abs(counts - trials * pr) <= 5 * math.sqrt(trials * pr * (1 - pr))).all(), counts


def test_accessory_flip_counts_follow_the_per_gene_law():
    G, N, gens, lam = 24, 1000, 20, [2.0, 1.5, 0.5]
    rng = np.random.default_rng(3)
    w = rng.random((3, G)).astype(np.float32)
    w[:, 4] = 0.0
    w[1, :12] = 0.0
    flip, _ = ref.acc_tables(lam, w, w)
    p = -np.expm1(-2.0 * ref.site_rates(lam, w)) / 2.0
    counts = np.zeros(G)
    for g in range(gens):
        counts += ref.acc_mutate(np.zeros((N, G), np.uint8), 11, g, flip).sum(0)
    trials = N * gens
    assert (trials * p)[p > 0].min() >= 20
    assert (np.abs(counts - trials * p) <= 5 * np.sqrt(trials * p * (1 - p))).all()
    assert counts[4] == 0


def _hgt_gene_counts(orc, N, G, lam, w, seed):
    """gene frequencies of the dense form's HGT events: every donor carries the same genes, the recipients start empty of
    them, so a gained bit names its gene (idempotent ORs lose a few events: the expected table accounts for that)"""
    _, wq = ref.acc_tables([0.0] * len(lam), w, w)
    present = np.zeros(G, bool)
    present[: G - 3] = True
    pop = np.zeros((N, G), np.uint8)
    pop[0, present] = 1                   # one donor with genes: its events go to the N - 1 empty rows
    out = pop.copy()
    events = ref.acc_hgt(out, seed, 0, lam, wq, orc.poisson_table)
    return out[1:].sum(0).astype(np.float64), present, events, wq


def test_hgt_gene_frequencies_follow_the_weights(orc):
    N, G, lam = 4000, 20, [1500.0]
    rng = np.random.default_rng(8)
    w = (rng.random((1, G)) + 0.2).astype(np.float32)
    w[0, 3] = 0.0
    got, present, events, wq = _hgt_gene_counts(orc, N, G, lam, w, 5)
    pr = np.where(present, w[0].astype(np.float64), 0.0)
    pr /= pr.sum()
    # k events of gene g over N - 1 recipients fill (N - 1)(1 - (1 - 1 / (N - 1))^k) distinct cells
    exp = (N - 1) * (1.0 - (1.0 - 1.0 / (N - 1)) ** (events * pr))
    assert exp[exp > 0].min() >= 20
    ok, chi2, df = _chi2_ok(got, exp)
    assert ok, (chi2, df)
    assert got[3] == 0 and got[~present].sum() == 0
    # the quantised weights are within 2^-16 of the law's
    assert np.abs(wq[0] / 65535.0 - w[0] / w[0].max()).max() <= 1.0 / 65535.0


def test_dense_form_against_the_event_driven_algorithm(orc):
    """two-sample comparison: per-site counts of the dense form and of the reference's sequential algorithm differ by no more
    than 5 sigma of the difference of two binomials with the pooled rate"""
    L, N, gens, lam = 12, 600, 12, [2.5]
    w = (1.0 + np.arange(L) % 5).astype(np.float32)
    w[2] = 0.0
    R, _, T = ref.core_tables(lam, [0.0], w)
    rng = np.random.default_rng(17)
    a, b = np.zeros(L), np.zeros(L)
    for g in range(gens):
        a += (ref.core_mutate(np.ones((N, L), np.uint8), 0, 3, g, R, T) != 1).sum(0)
        b += (ref.event_mutate_core(np.ones((N, L), np.uint8), rng, lam, w) != 1).sum(0)
    n = N * gens
    pooled = (a + b) / (2 * n)
    assert (np.abs(a - b) <= 5 * np.sqrt(2 * n * pooled * (1 - pooled)) + 1e-9).all(), (a, b)
    # accessory gain/loss
    G, lam2 = 10, [1.0, 2.0]
    w2 = np.stack([np.arange(1, G + 1), np.arange(G, 0, -1) ** 2]).astype(np.float32)
    flip, _ = ref.acc_tables(lam2, w2, w2)
    a, b = np.zeros(G), np.zeros(G)
    for g in range(gens):
        a += ref.acc_mutate(np.zeros((N, G), np.uint8), 3, g, flip).sum(0)
        b += ref.event_mutate_acc(np.zeros((N, G), np.uint8), rng, lam2, w2).sum(0)
    pooled = (a + b) / (2 * n)
    assert (np.abs(a - b) <= 5 * np.sqrt(2 * n * pooled * (1 - pooled)) + 1e-9).all(), (a, b)
    # HGT: gene counts of one donor's events, both ways (same total rate; chi-square of the 2 x G table)
    G, Nh = 15, 3000
    w3 = (np.arange(G) % 4 + 0.5).astype(np.float32).reshape(1, G)
    w3[0, 1] = 0.0
    got, present, _, _ = _hgt_gene_counts(orc, Nh, G, [1500.0], w3, 23)
    pop = np.zeros((Nh, G), np.uint8)
    pop[0, present] = 1
    lam_one = np.zeros(1) + 1500.0
    # only donor 0 has genes: the other donors' events find no qualifying gene (population.rs:672)
    out, _ = ref.event_hgt(pop.copy(), rng, lam_one, w3)
    other = out[1:].sum(0).astype(np.float64)
    tot = got + other
    keep = tot > 0
    e1, e2 = tot * got.sum() / tot.sum(), tot * other.sum() / tot.sum()
    chi2 = float(((got - e1)[keep] ** 2 / e1[keep] + (other - e2)[keep] ** 2 / e2[keep]).sum())
    df = int(keep.sum()) - 1
    assert tot[keep].min() >= 40 and chi2 <= df + 5.0 * math.sqrt(2.0 * df), (chi2, df)
    assert got[1] == 0 and other[1] == 0
