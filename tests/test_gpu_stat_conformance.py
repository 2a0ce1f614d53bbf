"""The device operators against their closed-form laws (tests/stat_laws.py), at the plans the benchmark's
workloads use and at 10^9 cells per plan.  The reference here is mathematics, not the oracle: every other GPU test compares
the kernels with the oracle bit for bit, which cannot see an error both share.

Every statistic prints its n, the expected and the observed count, z and the relative error it resolves at |z| = 5; a single
count must lie within 5 sigma of its law, a chi-square tail must be >= 1e-6.  Seeds and generation numbers are fixed: a run is
deterministic.  Known systematic terms come from stat_laws, each with the section of DESIGN.md that states it: the integer
thresholds of 3.2 (2^-32 R / 64 per class), of 3.3 (2^-32) and the weight quantisation of 3.6."""
import math
import time

import numpy as np
import pytest

import stat_laws as sl

pytestmark = pytest.mark.gpu

WAVE, WINDOW, BLOCK, INLINE = 1, 3, 4, 5
SEED = 20260101
N_POP, L_CORE = 1000, 100000
N_ODD, L_ODD = 1030, 99999            # neither a multiple of 16 or 4; N > 1024 takes the block and window sweeps
CELLS = 10 ** 9                       # cells per plan and operator
SLAB_L, SLAB_OFF, SLAB_GENS = 4096, 50002, 26       # the read-back slab: sites [50002, 54098) of the L_CORE global ones
SMALL_BLOCK = 100                     # the two blocks of individuals: N - 100 of allele A, 100 of allele C
ZMAX, TAIL_MIN = 5.0, 1.0e-6
PAIRS_MIN = 10 ** 8                   # cell pairs per lag of the independence statistics

RECORDS = []                          # (name, |z| or the z equivalent of a chi-square tail) of every statistic of the run
T0 = time.time()


# ----------------------------------------------------------------------------- reporting
def _record(what, n, expected, observed, z, res):
    RECORDS.append((what, abs(z)))
    print("%-58s n %.4g expected %.8g observed %.8g z %+.2f resolves %.3g" % (what, n, expected, observed, z, res))


def _check_count(what, count, trials, probs, systematic=0.0):
    """a count pooled over `trials` cells at each of `probs`; `systematic`: how far the implemented probability may lie from
    the closed form for a stated reason"""
    t, p = np.broadcast_arrays(np.asarray(trials, np.float64), np.asarray(probs, np.float64))
    n, mean, var = float(t.sum()), float((t * p).sum()), float((t * p * (1.0 - p)).sum())
    z = sl.z_pooled(count, t, p)
    if p.size == 1:
        assert z == pytest.approx(sl.z_binomial(count, n, float(p.reshape(-1)[0])), abs=1e-6)
    z = sl.with_systematic(z, n, math.sqrt(var), systematic)
    _record(what, n, mean, count, z, ZMAX * math.sqrt(var) / mean)
    assert abs(z) <= ZMAX, (what, count, mean, z)
    return z


def _check_z(what, z, n, expected, observed, sigma):
    """a z computed by the caller; sigma: the standard deviation of `observed` under the law"""
    _record(what, n, expected, observed, z, ZMAX * sigma / expected)
    assert abs(z) <= ZMAX, (what, observed, expected, z)


def _check_chi2(what, obs, exp, var=None, systematic=None):
    chi2, cells = sl.chi2_statistic(obs, exp, var, systematic)
    tail = sl.chi2_tail(chi2, cells)
    RECORDS.append((what, 0.0 if tail >= 0.5 else math.sqrt(-2.0 * math.log(2.0 * tail))))
    print("%-58s cells %d chi2 %.1f tail %.3g (expected per cell %.4g .. %.4g)" % (what, cells, chi2, tail, float(np.min(np.asarray(exp)[np.asarray(exp) > 0])), float(np.max(exp))))
    assert tail >= TAIL_MIN, (what, chi2, cells, tail)


def _assert_power(what, n, prob, bound, scale=1.0):
    """resolution(n, prob, 5), as a relative error of the part `prob / scale` of prob, must be <= bound"""
    res = sl.resolution(n, prob, ZMAX) * scale
    print("%-58s power: n %.4g resolves %.3g (<= %.3g)" % (what, n, res, bound))
    assert res <= bound, (what, n, res, bound)


# ----------------------------------------------------------------------------- plans
class _Plan:
    pass


def _plan(pa, name, L):
    """the core plan `name` of stat_laws.WORKLOAD_PLANS at L global sites: rates, per-site laws, and the (k, R, cshift) the
    library's own host tables give -- asserted, so that a case cannot silently test another regime"""
    flags, levels, shape = sl.WORKLOAD_PLANS[name]
    prm = pa.make_params(**flags)
    d = pa.derive(prm)
    pl = _Plan()
    pl.name, pl.L, pl.shape = name, L, shape
    pl.lm, pl.lh = sl.scaled_rates(prm.core_size, d.n_core_mutations, d.n_recombinations_core, L)
    assert pl.lm / L == pytest.approx(d.n_core_mutations / prm.core_size, rel=1e-12)
    if levels is None:
        pl.w, pl.level = None, np.zeros(L, np.int64)
        p, pl.q = sl.core_pq(pl.lm, pl.lh, L)
        pl.p_level = np.array([p])
        assert sl.core_plan_shape(p, pl.q) == shape
        t = pa.site_tables(True, L, [pl.lm], [pl.lh], np.ones(L, np.float32))
    else:
        pl.w, pl.level = sl.level_weights(levels, L)
        p_s, pl.q = sl.weighted_core_pq([pl.lm], [pl.lh], pl.w)
        pl.p_level = np.array([p_s[np.argmax(pl.level == lv)] for lv in range(len(levels))])
        assert sl.weighted_plan_shape(p_s, pl.q) == shape
        t = pa.site_tables(True, L, [pl.lm], [pl.lh], pl.w)
    assert (t["k"], t["R"], t["cshift"]) == shape, (name, t["k"], t["R"], t["cshift"])
    pl.k, pl.R, pl.cshift = shape
    pl.p_site = pl.p_level[pl.level]
    pl.classes = [sl.core_classes(float(p), pl.q) for p in pl.p_level]
    pl.systematic = 7.0 * float(sl.plan_bound(pl.R))           # 2^-32 R / 64 per class, seven classes at most
    return pl


def _core_pop(pa, pl, N, L, off=0, init=1):
    pop = pa.Population(N, L, 4, True, 0.0, SEED, 0, col_offset=off, global_cols=pl.L, init_vec=np.full(L, init, np.uint8))
    if pl.w is None:
        pop.set_rates([pl.lm], [pl.lh])
    else:
        pop.set_site_rates([pl.lm], [pl.lh], pl.w)
    return pop


def _expected_form(pl, N, fused):
    if pl.cshift > 1:
        return INLINE
    if N <= 1024:
        return WAVE
    return WINDOW if fused else BLOCK


def _blocks(N, L):
    m = np.ones((N, L), np.uint8)
    m[N - SMALL_BLOCK:] = 2
    labels = np.zeros(N, np.uint32)
    labels[N - SMALL_BLOCK:] = 1
    return m, labels


def _block_counts(pop, labels, N):
    """(L, 2, 4) per-block A, C, G, T counts of every site, tallied on the device; padding cells enter no tally"""
    gd = pop.group_differentiation(labels, max_groups=2, counts=True)
    assert list(gd.group_label) == [0, 1] and list(gd.group_size) == [N - SMALL_BLOCK, SMALL_BLOCK]
    c = gd.counts.astype(np.int64)
    assert (c[:, 0].sum(1) == N - SMALL_BLOCK).all() and (c[:, 1].sum(1) == SMALL_BLOCK).all()
    return c


def _generations(base, n_cells_per_generation, more=1):
    return [base + t for t in range(max(more, -(-CELLS // n_cells_per_generation)))]


CORE_CASES = [("cfg2", N_POP, L_CORE, 1000), ("cfg3", N_POP, L_CORE, 2000), ("authors", N_POP, L_CORE, 3000),
              ("hr_heavy", N_POP, L_CORE, 4000), ("weighted", N_POP, L_CORE, 5000), ("cfg2", N_ODD, L_ODD, 6000)]
CORE_IDS = ["%s-%dx%d" % c[:3] for c in CORE_CASES]


# ----------------------------------------------------------------------------- A. marginal laws of the core operators
@pytest.mark.parametrize("name,N,L,base", CORE_CASES, ids=CORE_IDS)
def test_mutate_alleles_follows_the_mutation_law(pa, name, N, L, base):
    pl = _plan(pa, name, L)
    gens = _generations(base, N * L)
    n = N * L * len(gens)
    what = "mutate %s %dx%d" % (name, N, L)
    if name == "cfg2":            # the level-2 share of the mutation mass (0.00177 of 0.0488) to 2 %
        p = float(pl.p_level[0])
        _assert_power(what + " level-2 share", n, p, 0.02, scale=p / sl.level2_mutation_share(pl.k, p, pl.q))
    pop = _core_pop(pa, pl, N, L)
    ones = np.ones((N, L), np.uint8)
    tally = np.zeros((2, L, 4), np.int64)
    for t, g in enumerate(gens):
        if t:
            pop.load_matrix(ones)
        pop.mutate_alleles(g)
        assert pop.last_sweep_form() == _expected_form(pl, N, False)
        c = pop.site_allele_counts().astype(np.int64)
        assert (c.sum(1) == N).all()                        # every cell once, no padding cell
        tally[g & 1] += c
    pop.close()
    per_gen = np.array([sum(1 for g in gens if (g & 1) == e) for e in (0, 1)])
    both = tally.sum(0)
    _check_count(what + " all hits", both[:, 1:].sum(), N * len(gens), pl.p_site, pl.systematic)      # (the statistic of the power above)
    for j, base_name in enumerate("CGT"):                   # mutate_alleles shows outcomes j and 3 + j alike: p_s / 3
        _check_count("%s allele %s" % (what, base_name), both[:, 1 + j].sum(), N * len(gens), pl.p_site / 3.0, pl.systematic)
    hits = tally[:, :, 1:].sum(2)
    for r in range(4):                                      # the positions inside the level-1 blocks of 3.2
        _check_count("%s site mod 4 = %d" % (what, r), hits[:, r::4].sum(), N * len(gens), pl.p_site[r::4], pl.systematic)
    for e in (0, 1):
        _check_count("%s generation parity %d" % (what, e), hits[e].sum(), N * per_gen[e], pl.p_site, pl.systematic)
    if pl.w is not None:
        for lv, p in enumerate(pl.p_level):
            got = hits[:, pl.level == lv].sum()
            if p == 0.0:
                assert got == 0                             # a site of weight 0 never mutates
            else:
                _check_count("%s weight level %d" % (what, lv), got, N * len(gens) * int((pl.level == lv).sum()), p, pl.systematic)
    # 'A' is never written: from an all-C matrix no A appears, at any plan, and two thirds of the hits show as G or T
    pop = _core_pop(pa, pl, N, L, init=2)
    twos = np.full((N, L), 2, np.uint8)
    moved = 0
    for t, g in enumerate(gens):
        if t:
            pop.load_matrix(twos)
        pop.mutate_alleles(g + 500)
        c = pop.site_allele_counts().astype(np.int64)
        assert (c.sum(1) == N).all() and c[:, 0].sum() == 0
        moved += int(c[:, 2:].sum())
    pop.close()
    _check_count(what + " from C: G or T", moved, N * len(gens), 2.0 * pl.p_site / 3.0, pl.systematic)


HR_CASES = [c for c in CORE_CASES if c[0] != "authors"]
HR_IDS = ["%s-%dx%d" % c[:3] for c in HR_CASES]


@pytest.mark.parametrize("name,N,L,base", HR_CASES, ids=HR_IDS)
def test_recombine_follows_the_transfer_law(pa, name, N, L, base):
    pl = _plan(pa, name, L)
    n_own = (N - SMALL_BLOCK, SMALL_BLOCK)
    # a cell of block b takes the other block's allele with q n_other / (N - 1): the total allele count is neutral under
    # copying, so the tallies are per block
    prob = [pl.q * n_own[1 - b] / (N - 1) for b in (0, 1)]
    pooled = (n_own[0] * prob[0] + n_own[1] * prob[1]) / N
    more = 1
    while sl.resolution(N * L * more, pooled, ZMAX) > 0.005:       # generations until q is resolved to 0.5 %
        more += 1
    gens = _generations(base + 100, N * L, more)
    what = "recombine %s %dx%d" % (name, N, L)
    _assert_power(what + " q", N * L * len(gens), pooled, 0.005)
    pop = _core_pop(pa, pl, N, L)
    m0, labels = _blocks(N, L)
    moved = np.zeros((L, 2), np.int64)
    for g in gens:
        pop.load_matrix(m0)
        pop.recombine(g)
        assert pop.last_sweep_form() == _expected_form(pl, N, False)
        c = _block_counts(pop, labels, N)
        assert (c[:, :, 2:] == 0).all()                      # copying creates no allele
        moved[:, 0] += c[:, 0, 1]
        moved[:, 1] += c[:, 1, 0]
    pop.close()
    sys_q = 4.0 * float(sl.plan_bound(pl.R))                # outcomes 3 .. 6
    for b in (0, 1):
        _check_count("%s block %d" % (what, b), moved[:, b].sum(), n_own[b] * L * len(gens), prob[b], sys_q)
    _check_count("%s both blocks" % what, moved.sum(), [n_own[0] * L * len(gens), n_own[1] * L * len(gens)], prob, sys_q)
    if pl.w is not None:                                    # HR stays uniform over the sites whatever their weights
        for lv in range(len(pl.p_level)):
            sites = int((pl.level == lv).sum())
            _check_count("%s weight level %d" % (what, lv), moved[pl.level == lv].sum(),
                         [n_own[0] * sites * len(gens), n_own[1] * sites * len(gens)], prob, sys_q)


@pytest.mark.parametrize("name,N,L,base", CORE_CASES, ids=CORE_IDS)
def test_fused_step_follows_both_laws(pa, name, N, L, base):
    pl = _plan(pa, name, L)
    what = "step %s %dx%d" % (name, N, L)
    n_own = (N - SMALL_BLOCK, SMALL_BLOCK)
    # per weight level the law of a cell of each block: block 0 holds A beside C, block 1 C beside A
    laws = [[sl.block_law(cl, own, other, n_own[b], n_own[1 - b]) for cl in pl.classes] for b, (own, other) in enumerate(((1, 2), (2, 1)))]
    law_site = [{v: np.array([laws[b][lv][v] for lv in range(len(pl.classes))])[pl.level] for v in sl.ALLELES} for b in (0, 1)]
    # q shows in one tally only: a cell of the C block ends as A iff it received the allele of an unmutated donor of the A
    # block, q (1 - p) n_other / (N - 1) -- a relative error of q is the same relative error of that count.  The mutation law
    # shows in the cells that end as G or T (2 p / 3 in both blocks, whatever was received).  Generations until the first
    # resolves q to 0.5 % and, at cfg2, the second the level-2 share of the mutation mass to 2 %.
    prob_a = float(law_site[1][1].mean())
    prob_gt = float((law_site[0][4] + law_site[0][8]).mean())
    share_scale = prob_gt / (2.0 / 3.0 * sl.level2_mutation_share(pl.k, float(pl.p_level[0]), pl.q)) if name == "cfg2" else None
    more = 1
    while (pl.q > 0.0 and sl.resolution(n_own[1] * L * more, prob_a, ZMAX) > 0.005) or \
            (share_scale is not None and sl.resolution(N * L * more, prob_gt, ZMAX) * share_scale > 0.02):
        more += 1
    gens = _generations(base + 200, N * L, more)
    if pl.q > 0.0:
        _assert_power(what + " q", n_own[1] * L * len(gens), prob_a, 0.005)
    if share_scale is not None:
        _assert_power(what + " level-2 share", N * L * len(gens), prob_gt, 0.02, scale=share_scale)
    pop = _core_pop(pa, pl, N, L)
    m0, labels = _blocks(N, L)
    identity = np.arange(N, dtype=np.uint32)
    tally = np.zeros((L, 2, 4), np.int64)
    for g in gens:
        pop.load_matrix(m0)
        pop.step(g, identity, True)
        assert pop.last_sweep_form() == _expected_form(pl, N, True)
        tally += _block_counts(pop, labels, N)
    pop.close()
    for b in (0, 1):
        trials = n_own[b] * len(gens)
        if b == 0 or pl.q > 0.0:       # (block 1 shows A only by a transfer from an unmutated donor of block 0)
            _check_count("%s block %d ends A" % (what, b), tally[:, b, 0].sum(), trials, law_site[b][1], pl.systematic)
        else:
            assert tally[:, b, 0].sum() == 0
        _check_count("%s block %d ends G or T" % (what, b), tally[:, b, 2:].sum(), trials, law_site[b][4] + law_site[b][8], pl.systematic)
    gt = [law_site[b][4] + law_site[b][8] for b in (0, 1)]
    _check_count("%s both blocks end G or T" % what, tally[:, :, 2:].sum(), [[n_own[0] * len(gens)], [n_own[1] * len(gens)]], gt, pl.systematic)


# ----------------------------------------------------------------------------- B. independence where the layout shares blocks
def _lag_count(h, axis, lag):
    a = [slice(None)] * h.ndim
    b = [slice(None)] * h.ndim
    a[axis], b[axis] = slice(0, h.shape[axis] - lag), slice(lag, None)
    return int((h[tuple(a)] & h[tuple(b)]).sum())


def test_mutation_hits_are_independent_across_cells_and_generations(pa):
    """hits of mutate_alleles on a read-back slab: cells that share a plane word (individuals 1 and 4 apart), a Philox block
    (sites 1 and 2 apart) or nothing (16 individuals, 4 sites apart: the controls), and the same cell one generation on"""
    pl = _plan(pa, "cfg2", L_CORE)
    p = float(pl.p_level[0])
    N, Ls, G = N_POP, SLAB_L, SLAB_GENS
    pop = _core_pop(pa, pl, N, Ls, SLAB_OFF)
    ones = np.ones((N, Ls), np.uint8)
    h = np.zeros((G, N, Ls), bool)
    for t in range(G):
        if t:
            pop.load_matrix(ones)
        pop.mutate_alleles(7000 + t)
        h[t] = pop.read_matrix() != 1
    pop.close()
    _check_count("slab hits", int(h.sum()), h.size, p, pl.systematic)
    shape = {0: G, 1: N, 2: Ls}
    for axis, lags, unit in ((1, (1, 4, 16), "individuals"), (2, (1, 2, 4), "sites"), (0, (1,), "generations")):
        for lag in lags:
            other = h.size // shape[axis]
            n, n_adj = (shape[axis] - lag) * other, max(shape[axis] - 2 * lag, 0) * other
            assert n >= PAIRS_MIN
            got = _lag_count(h, axis, lag)
            _check_z("joint hits %d %s apart" % (lag, unit), sl.z_lag(got, n, n_adj, p), n, n * p * p, got, sl.sigma_lag(n, n_adj, p))
    # dispersion of the totals about their known means, against the statistic's own variance
    for axis, trials, unit in ((2, Ls, "individual"), (1, N, "site")):
        totals = h.sum(axis)
        z = sl.z_dispersion(totals, trials, p)
        _check_z("dispersion of per-%s totals" % unit, z, totals.size, totals.size * trials * p * (1 - p), float(((totals - trials * p) ** 2).sum()),
                 sl.sigma_dispersion(totals.size, trials, p))


def test_mutation_and_recombination_of_a_cell_follow_the_joint_law(pa):
    """cfg3's joint plan on a read-back slab: the mutation hit and the HR hit of one cell from the two separate calls of a
    generation (joint mass 3 b = p q), and the same outcome inside the fused step: a cell of the C block that mutate_alleles
    hits and that the step leaves as A was mutated AND received the allele of an unmutated donor of the A block"""
    pl = _plan(pa, "cfg3", L_CORE)
    p, q = float(pl.p_level[0]), pl.q
    N, Ls, G = N_POP, SLAB_L, SLAB_GENS
    n_own = (N - SMALL_BLOCK, SMALL_BLOCK)
    rows = (slice(0, n_own[0]), slice(n_own[0], N))
    pop = _core_pop(pa, pl, N, Ls, SLAB_OFF)
    ones = np.ones((N, Ls), np.uint8)
    m0, _ = _blocks(N, Ls)
    identity = np.arange(N, dtype=np.uint32)
    both = [0, 0]
    fused = 0
    for t in range(G):
        g = 8000 + t
        pop.load_matrix(ones)
        pop.mutate_alleles(g)
        mut = pop.read_matrix() != 1
        pop.load_matrix(m0)
        pop.recombine(g)
        hr = pop.read_matrix() != m0
        pop.load_matrix(m0)
        pop.step(g, identity, True)
        assert pop.last_sweep_form() == WAVE
        end = pop.read_matrix()
        for b in (0, 1):
            both[b] += int((mut[rows[b]] & hr[rows[b]]).sum())
        fused += int((mut[rows[1]] & (end[rows[1]] == 1)).sum())
    pop.close()
    sys_b = 3.0 * float(sl.plan_bound(pl.R))
    for b in (0, 1):
        n = n_own[b] * Ls * G
        vis = q * n_own[1 - b] / (N - 1)
        z = sl.with_systematic(sl.z_joint(both[b], n, p, vis), n, math.sqrt(n * p * vis * (1.0 - p * vis)), sys_b)
        _check_z("mutation hit x HR hit, block %d" % b, z, n, n * p * vis, both[b], math.sqrt(n * p * vis * (1.0 - p * vis)))
    b3 = 3.0 * sl.core_classes(p, q)[3]
    _check_count("step: mutated and received (3 b)", fused, n_own[1] * Ls * G, b3 * n_own[0] / (N - 1) * (1.0 - p), sys_b)


# ----------------------------------------------------------------------------- C. accessory flips
def test_accessory_flips_follow_p_flip(pa):
    N, G = N_POP, 6000
    prm = pa.make_params()
    d = pa.derive(prm)
    assert d.n_comp == 2
    size = [int(d.comp_end[c] - d.comp_begin[c]) for c in (0, 1)]
    cut = G * size[0] // int(d.pan_size)
    cb, ce = [0, cut], [cut, G]
    lam = [d.n_pan_mutations[c] / size[c] * (ce[c] - cb[c]) for c in (0, 1)]       # cfg2's per-gene rates at this G
    pf = [sl.p_flip(lam[c], ce[c] - cb[c]) for c in (0, 1)]
    assert pf[0] == pytest.approx((1.0 - math.exp(-2.0)) / 2.0) and pf[1] == pytest.approx(0.5)
    gens = -(-5 * 10 ** 8 // (2 * N * G))
    flips = np.zeros((2, G), np.int64)
    for start in (0, 1):
        pop = pa.Population(N, G, 2, False, 0.0, SEED, 0, init_vec=np.full(G, start, np.uint8))
        pop.set_rates(lam, [0.0, 0.0], cb, ce)
        m0 = np.full((N, G), start, np.uint8)
        for t in range(gens):
            if t:
                pop.load_matrix(m0)
            pop.mutate_alleles(9000 + 1000 * start + t)
            carried = np.rint(pop.gene_frequencies()[:G] * N).astype(np.int64)
            flips[start] += N - carried if start else carried
        if start == 0:       # joint flips of neighbouring genes from one read-back: four genes share a Philox block
            joint = [0, 0]
            for t in range(4):
                pop.load_matrix(m0)
                pop.mutate_alleles(9500 + t)
                x = pop.read_matrix()[:, :cut - cut % 4].astype(bool)
                joint[0] += int((x[:, 0::2] & x[:, 1::2]).sum())                      # genes 2j, 2j + 1: one block
                joint[1] += int((x[:, 1:-1:2] & x[:, 2::2]).sum())                    # genes 2j + 1, 2j + 2: every other pair crosses
            pairs = [4 * N * (x.shape[1] // 2), 4 * N * (x.shape[1] // 2 - 1)]
        pop.close()
    assert 2 * N * G * gens >= 5 * 10 ** 8
    for c in (0, 1):
        for start in (0, 1):
            _check_count("flips compartment %d from all-%d" % (c, start), flips[start, cb[c]:ce[c]].sum(), N * gens * (ce[c] - cb[c]), pf[c], 2.0 ** -32)
    for r in range(4):
        _check_count("flips compartment 0, gene mod 4 = %d" % r, flips[:, r:cut:4].sum(), 2 * N * gens * len(range(r, cut, 4)), pf[0], 2.0 ** -32)
    for k in (0, 1):
        _check_z("joint flips of genes g, g + 1 (%s)" % ("one block", "across blocks")[k], sl.z_joint(joint[k], pairs[k], pf[0], pf[0]), pairs[k],
                 pairs[k] * pf[0] ** 2, joint[k], math.sqrt(pairs[k] * pf[0] ** 2 * (1.0 - pf[0] ** 2)))
    # a compartment of rate 0 has exactly zero flips
    pop = pa.Population(N, G, 2, False, 0.0, SEED, 0, init_vec=np.zeros(G, np.uint8))
    pop.set_rates([lam[0], 0.0], [0.0, 0.0], cb, ce)
    for t in range(3):
        pop.mutate_alleles(9900 + t)
    f = pop.gene_frequencies()[:G]
    pop.close()
    assert (f[cut:] == 0.0).all() and (f[:cut] > 0.0).all()


# ----------------------------------------------------------------------------- D. HGT at cfg3's rates, both kernel forms
def _hgt_setup(pa):
    prm = pa.make_params(HR_rate=0.5, HGT_rate=0.5)
    d = pa.derive(prm)
    G = int(d.pan_size)
    cb, ce = [int(d.comp_begin[c]) for c in (0, 1)], [int(d.comp_end[c]) for c in (0, 1)]
    lam = [float(d.n_recombinations_pan[c]) for c in (0, 1)]
    assert lam[0] == pytest.approx(27000.0) and lam[1] == pytest.approx(3000.0)
    return int(prm.pop_size), G, cb, ce, lam


def _acc_pop(pa, N, G):
    return pa.Population(N, G, 2, False, 0.0, SEED, 0, init_vec=np.zeros(G, np.uint8))


@pytest.mark.parametrize("mode", [1, 2], ids=["light", "binned"])
def test_hgt_total_events_follow_the_gain_law(pa, monkeypatch, mode):
    monkeypatch.setenv("PANSIM_HGT_MODE", str(mode))
    N, G, cb, ce, lam = _hgt_setup(pa)
    rng = np.random.default_rng(11)
    m0 = np.zeros((N, G), np.uint8)
    m0[::10] = rng.random((N // 10, G)) < 0.5                # a tenth of the individuals carry genes: rate 0.75 per lacking cell
    m0[:, 17::40] = 0                                        # genes nobody carries can never be gained
    pop = _acc_pop(pa, N, G)
    pop.set_rates([0.0, 0.0], lam, cb, ce)
    gained = np.zeros(2, np.int64)
    gens = 3
    for t in range(gens):
        pop.load_matrix(m0)
        pop.recombine(10000 + 100 * mode + t)
        m = pop.read_matrix()
        assert (m >= m0).all() and m[:, 17::40].sum() == 0  # gain only, and only genes a donor carries
        for c in (0, 1):
            gained[c] += int((m > m0)[:, cb[c]:ce[c]].sum())
    pop.close()
    for c in (0, 1):
        # Poisson(lam) events per donor, uniform recipient and gene: a lacking cell gains with 1 - exp(-sum_d lam / ((N - 1) n_d))
        sub = m0[:, cb[c]:ce[c]]
        _, prob = sl.hgt_gain_law(sub, lam[c])
        mean, var = sl.hgt_expected_gains(sub, prob)
        z = (gained[c] - gens * mean) / math.sqrt(gens * var)
        _check_z("HGT form %d gains of compartment %d" % (mode, c), z, gens * (1 - sub).sum(), gens * mean, gained[c], math.sqrt(gens * var))


@pytest.mark.parametrize("mode", [1, 2], ids=["light", "binned"])
def test_hgt_recipients_and_genes_are_uniform(pa, monkeypatch, mode):
    monkeypatch.setenv("PANSIM_HGT_MODE", str(mode))
    N, G, cb, ce, lam = _hgt_setup(pa)
    donor = 7
    m0 = np.zeros((N, G), np.uint8)
    m0[donor, ::2] = 1                                       # one donor carries every other gene, everyone else is empty
    pop = _acc_pop(pa, N, G)
    pop.set_rates([0.0, 0.0], lam, cb, ce)
    gens = 10
    got = np.zeros((N, G), np.int64)
    for t in range(gens):
        pop.load_matrix(m0)
        pop.recombine(11000 + 100 * mode + t)
        m = pop.read_matrix()
        assert np.array_equal(m[donor], m0[donor])           # the donor itself is unchanged
        got += m > m0
    pop.close()
    prob = np.zeros(G)
    for c in (0, 1):
        prob[cb[c]:ce[c]] = sl.hgt_gain_law(m0[:, cb[c]:ce[c]], lam[c])[1]
    assert got[:, 1::2].sum() == 0                           # a gene nobody carries is never gained
    others = np.arange(N) != donor
    mean, var = gens * prob.sum(), gens * (prob * (1.0 - prob)).sum()
    _check_chi2("HGT form %d gains per recipient" % mode, got[others].sum(1), np.full(N - 1, mean), np.full(N - 1, var))
    trials = gens * (N - 1)
    _check_chi2("HGT form %d gains per gene" % mode, got[others].sum(0), trials * prob, trials * prob * (1.0 - prob))


def _pool(level, *arrays, min_exp=20.0):
    """greedy pooling of neighbouring genes of one weight level until a pool's expectation (arrays[1]) reaches min_exp; what
    is left over at the end of a level joins the level's last pool, so that every gene is in one"""
    out = [[] for _ in arrays]
    for lv in np.unique(level):
        idx = np.nonzero(level == lv)[0]
        acc = [0.0] * len(arrays)
        filled = False
        for i in idx:
            acc = [a + float(x[i]) for a, x in zip(acc, arrays)]
            if acc[1] >= min_exp:
                for o, a in zip(out, acc):
                    o.append(a)
                acc = [0.0] * len(arrays)
                filled = True
        if acc[1] > 0.0:
            for o, a in zip(out, acc):
                if filled:
                    o[-1] += a
                else:
                    o.append(a)
    return [np.array(o) for o in out]


@pytest.mark.parametrize("mode", [1, 2], ids=["light", "binned"])
def test_hgt_gene_pick_follows_the_weights(pa, monkeypatch, mode):
    monkeypatch.setenv("PANSIM_HGT_MODE", str(mode))
    N, G, _, _, lam2 = _hgt_setup(pa)
    lam = lam2[0]
    level = np.arange(G) % 4
    w = np.asarray([1.0, 10.0, 100.0, 1000.0], np.float32)[level]
    w[::9] = 0.0                                             # genes of weight 0 are never picked
    present = np.arange(G) % 5 == 0
    assert (present & (w == 0)).sum() > 10 and all(((level == lv) & present & (w > 0)).sum() > 100 for lv in range(4))
    donor = 3
    m0 = np.zeros((N, G), np.uint8)
    m0[donor, present] = 1
    pop = _acc_pop(pa, N, G)
    pop.set_site_rates([0.0], [lam], np.ones(G, np.float32), w)
    gens = 40
    got = np.zeros(G, np.int64)
    for t in range(gens):
        pop.load_matrix(m0)
        pop.recombine(12000 + 100 * mode + t)
        m = pop.read_matrix()
        assert np.array_equal(m[donor], m0[donor])
        got += (m > m0).sum(0)
    pop.close()
    assert got[~present].sum() == 0 and got[w == 0].sum() == 0
    _, prob = sl.hgt_gain_law(m0, lam, weights=w)
    trials = gens * (N - 1)
    exp, var = trials * prob, trials * prob * (1.0 - prob)
    # the u16 weights move a gene's pick probability by at most this relative amount
    systematic = exp * sl.hgt_quant_bound(w, present)
    keep = present & (w > 0)
    o, e, v, s = _pool(level[keep], got[keep], exp[keep], var[keep], systematic[keep])
    _check_chi2("HGT form %d weighted gains per gene" % mode, o, e, v, s)
    for lv in range(4):                                      # ... and the levels as wholes: the ratio 1 : 1000
        sel = keep & (level == lv)
        z = (got[sel].sum() - exp[sel].sum()) / math.sqrt(var[sel].sum())
        z = sl.with_systematic(z, 1.0, math.sqrt(var[sel].sum()), systematic[sel].sum())
        _check_z("HGT form %d gains of weight %g" % (mode, [1, 10, 100, 1000][lv]), z, trials * sel.sum(), exp[sel].sum(), got[sel].sum(),
                 math.sqrt(var[sel].sum()))


# ----------------------------------------------------------------------------- the run as a whole
def test_the_run_stays_within_its_budget_of_statistics(request):
    """at most about 200 statistics: the chance that a correct engine fails somewhere stays below 2e-4.  It counts what the
    tests of this file recorded before it IN THIS PROCESS: selected with any of them it must have seen statistics, selected
    alone it has nothing to count."""
    mine = [i for i in request.session.items if i.fspath == request.node.fspath]
    if len(mine) > 1:
        assert RECORDS
    worst = max(RECORDS, key=lambda r: r[1]) if RECORDS else ("none", 0.0)
    print("%d statistics, largest |z| %.2f (%s), %.1f s since the module was imported" % (len(RECORDS), worst[1], worst[0], time.time() - T0))
    assert len(RECORDS) <= 200
