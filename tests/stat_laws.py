"""The closed-form laws of the stochastic operators and the plain statistics that hold an implementation
to them.  A helper, not a test: plain Python and numpy, f64 and `fractions` where exactness is cheap, nothing of the product
or the oracle.  tests/test_stat_laws.py checks the integer tables against these forms on the CPU,
tests/test_gpu_stat_conformance.py the kernels' tallies on the device.

Alleles are the one-hot bytes A, C, G, T = 1, 2, 4, 8; the seven outcomes of a core cell (3.2) are numbered
0, 1, 2 = mutate to C, G, T only; 3, 4, 5 = the same and receive a donor allele; 6 = donor allele only."""
import math
from fractions import Fraction

import numpy as np

TWO32 = 1 << 32
ALLELES = (1, 2, 4, 8)


# ----------------------------------------------------------------------------- core cell law (3.2)
def event_prob(rate):
    """1 - exp(-rate): a Poisson(rate) count is not zero"""
    return -math.expm1(-rate) if rate > 0.0 else 0.0


def core_pq(lam_mut, lam_hr, L):
    """(p, q) of a cell from the per-individual rates and the GLOBAL number of sites"""
    return event_prob(lam_mut / L), event_prob(lam_hr / L)


def core_classes(p, q):
    """the seven outcome masses [a, a, a, b, b, b, c]"""
    a, b, c = p * (1.0 - q) / 3.0, p * q / 3.0, (1.0 - p) * q
    return [a, a, a, b, b, b, c]


def core_plan_shape(p, q):
    """(k, R, cshift) of the cell plan of 3.2 for a uniform law: k decided symbols per allele, R residual symbols, and the
    smallest shift with 3k + R <= 4 * 2^cshift"""
    a, b, c = core_classes(p, q)[0], core_classes(p, q)[3], core_classes(p, q)[6]
    k = int(math.floor(64.0 * a))
    R = int(math.ceil(64.0 * (3.0 * (a - k / 64.0) + 3.0 * b + c)))
    return (k, R) + (_cshift(3 * k + R),)


def _cshift(symbols):
    cs = 0
    while cs < 4 and symbols > (4 << cs):
        cs += 1
    return cs


def plan_classes(k, R, T):
    """The IMPLEMENTED seven masses of a plan's integers, exact (Fractions): a symbol is uniform on 0 .. 63, k of them decide
    each allele, and inside the R residual ones the word is cut by the cumulative thresholds T[0 .. 6] -- the residual class
    scaled by R / 64"""
    T = [int(t) for t in T]
    out = []
    for j in range(7):
        width = Fraction(T[j] - (T[j - 1] if j else 0), TWO32) * Fraction(int(R), 64)
        out.append(width + (Fraction(int(k), 64) if j < 3 else 0))
    return out


def plan_bound(R):
    """what 3.2 states for the distance of a class of plan_classes from the closed form: 2^-32 R / 64"""
    return Fraction(int(R), 64 * TWO32)


def level2_mutation_share(k, p, q):
    """the mutate-only mass 3 a = p (1 - q) less what the 3 k decided symbols hold: the part of the mutation law that only the
    residual word decides (the mutate-and-receive mass 3 b lies there as well, whatever k is)"""
    return p * (1.0 - q) - 3.0 * k / 64.0


def mutate_law(classes):
    """`mutate_alleles` alone: the probability that a cell is written C, G, T (outcomes 0-2 and 3-5 show alike)"""
    return [classes[j] + classes[3 + j] for j in range(3)]


def receive_prob(classes):
    """`recombine` alone: the probability that a cell takes its donor's allele (outcomes 3-6)"""
    return classes[3] + classes[4] + classes[5] + classes[6]


def block_law(classes, own, other, n_own, n_other, mutate=True, recombine=True):
    """The law of a cell's value after one generation in a population of two blocks: the cell's block holds n_own individuals
    of allele `own`, the other block n_other of allele `other`.  -> {allele: probability}.  The donor is uniform over the
    N - 1 others and hands over its post-mutation allele; a cell's own outcome and its donor's mutation are independent.
    `mutate` / `recombine` False: the entry point that applies only the other operator (fused step: both)."""
    N = n_own + n_other
    mut = mutate_law(classes) if mutate else [0, 0, 0]
    stay = 1 - sum(mut)

    def post(x):          # the post-mutation value of a cell that held x
        d = {v: mut[j] for j, v in enumerate((2, 4, 8))}
        d[1] = 0
        d[x] = d[x] + stay
        return d

    recv = receive_prob(classes) if recombine else 0
    if not mutate:
        own_only = {v: 0 for v in ALLELES}
    elif recombine:
        own_only = {1: 0, 2: classes[0], 4: classes[1], 8: classes[2]}
    else:
        own_only = {1: 0, 2: mut[0], 4: mut[1], 8: mut[2]}
    nothing = 1 - recv - sum(own_only.values())
    f_own = (n_own - 1) / (N - 1) if not isinstance(recv, Fraction) else Fraction(n_own - 1, N - 1)
    f_other = n_other / (N - 1) if not isinstance(recv, Fraction) else Fraction(n_other, N - 1)
    po, pt = post(own), post(other)
    out = {}
    for v in ALLELES:
        out[v] = own_only[v] + (nothing if v == own else 0) + recv * (f_own * po[v] + f_other * pt[v])
    return out


# ----------------------------------------------------------------------------- per-site weights (3.6)
def site_rates(lams, weights):
    """r[s] = sum_c lam_c w_c[s] / W_c: W_c the f64 sum left to right, compartments in order, a rate of 0 skipped"""
    w = np.asarray(weights, np.float64)
    if w.ndim == 1:
        w = w.reshape(1, -1)
    r = np.zeros(w.shape[1])
    for c, lam in enumerate(lams):
        if lam > 0.0:
            r = r + lam * w[c] / np.cumsum(w[c])[-1]
    return r


def weighted_core_pq(lam_mut, lam_hr, weights):
    """(p_s per site, q): mutation follows the weights, HR stays uniform over the sites and the compartments' rates add"""
    r = site_rates(lam_mut, weights)
    return -np.expm1(-r), event_prob(float(sum(lam_hr)) / r.size)


def weighted_plan_shape(p_s, q):
    """(k, R, cshift) of a weighted plan: k = 0 always, R from the largest event mass of a site"""
    m = max(sum(core_classes(float(p), q)) for p in np.unique(p_s))
    R = min(64, int(math.ceil(64.0 * m)))
    return 0, R, _cshift(R)


# ----------------------------------------------------------------------------- accessory (3.3, 3.4, 3.6)
def p_flip(lam, n_genes):
    """3.3: a gene of a compartment of n_genes genes with rate lam per individual flips iff its Poisson count is odd"""
    return -math.expm1(-2.0 * lam / n_genes) / 2.0 if lam > 0.0 and n_genes else 0.0


def hgt_gain_law(present, lam, weights=None):
    """The gain law of one compartment's HGT: `present` (N, G) 0/1 the pre-HGT snapshot, lam events per donor, recipient
    uniform over the N - 1 others, gene uniform -- or with `weights` in proportion to w[g] -- over the donor's present genes.
    -> (rate, prob): rate[g] = sum_d lam / (N - 1) pick_d(g), prob[g] = 1 - exp(-rate[g]) that an individual LACKING gene g
    gains it (one that carries g is no recipient of it, and a donor never sends to itself)."""
    x = np.asarray(present, np.float64)
    N = x.shape[0]
    w = np.ones(x.shape[1]) if weights is None else np.asarray(weights, np.float64)
    tot = (x * w).sum(1)
    pick = np.divide(x * w, tot[:, None], out=np.zeros_like(x), where=tot[:, None] > 0)
    rate = lam / (N - 1) * pick.sum(0)
    return rate, -np.expm1(-rate)


def hgt_expected_gains(present, prob):
    """(mean, variance) of the number of gained cells: independent Bernoulli(prob[g]) over the cells that lack their gene"""
    lack = 1.0 - np.asarray(present, np.float64)
    return float((lack * prob).sum()), float((lack * prob * (1.0 - prob)).sum())


HGT_QUANT_STEP = 1.0 / (2.0 * 65535.0)        # half a step of the u16 scale: what 3.6 rounds to 2^-17


def hgt_quantise(w):
    """3.6: w_hat = max(1, floor(65535 w / w_max + 1/2)) for w > 0, else 0"""
    w = np.asarray(w, np.float64)
    x = np.floor(65535.0 * w / w.max() + 0.5)
    return np.where(w > 0, np.maximum(x, 1.0), 0.0)


def hgt_quant_bound(w, present_set):
    """3.6's error bound as numbers: by what RELATIVE amount the pick probability of each gene of `present_set` (a boolean
    mask) may differ from w[g] / sum_P w -- (1 + e w_max / w[g]) / (1 - e |P| w_max / sum_P w) - 1 with e half a step of the u16
    scale (a whole step for weights that round up to 1), plus the term of `mulhi32`.  A gene owns a CONTIGUOUS stretch of the
    values x = mulhi32(word, total), so the words that pick it number w_hat 2^32 / total give or take one: 2^-32 absolute,
    total 2^-32 / w_hat[g] relative -- the `total 2^-32 per gene` of 3.6 is this at w_hat = 1.  0 where the gene is not in the set."""
    w = np.asarray(w, np.float64)
    P = np.asarray(present_set, bool) & (w > 0)
    wmax = w.max()
    e = np.where(w < wmax / 131070.0, 2.0 * HGT_QUANT_STEP, HGT_QUANT_STEP)
    with np.errstate(divide="ignore"):
        up = 1.0 + e * wmax / w
    down = 1.0 - float((e * P).sum()) * wmax / float(w[P].sum())
    wq = hgt_quantise(w)
    total = float(wq[P].sum())
    return np.where(P, up / down - 1.0 + total / TWO32 / np.maximum(wq, 1.0), 0.0)


# ----------------------------------------------------------------------------- statistics
def z_binomial(count, n, prob):
    """(count - n prob) / sqrt(n prob (1 - prob))"""
    prob = float(prob)
    return (float(count) - n * prob) / math.sqrt(n * prob * (1.0 - prob))


def z_pooled(count, trials, probs):
    """a count pooled over cells of different laws: `trials` independent cells at each of `probs` (arrays broadcast against
    each other) -- mean sum t p, variance sum t p (1 - p)"""
    t, p = np.broadcast_arrays(np.asarray(trials, np.float64), np.asarray(probs, np.float64))
    return (float(count) - float((t * p).sum())) / math.sqrt(float((t * p * (1.0 - p)).sum()))


def z_joint(count_both, n, px, py):
    """independence of two events over n disjoint trials: the joint count against n px py"""
    return z_binomial(count_both, n, float(px) * float(py))


def z_lag(count_both, n, n_adjacent, prob):
    """The joint count of X[i] X[i + d] over n pairs of ONE array of independent Bernoulli(prob) cells, n_adjacent couples of
    which share a cell ((i, i + d) and (i + d, i + 2 d)): variance n p^2 (1 - p^2) + 2 n_adjacent (p^3 - p^4)"""
    p = float(prob)
    return (float(count_both) - n * p * p) / sigma_lag(n, n_adjacent, p)


def sigma_lag(n, n_adjacent, prob):
    """the standard deviation of z_lag's count"""
    p = float(prob)
    return math.sqrt(n * p * p * (1.0 - p * p) + 2.0 * n_adjacent * (p ** 3 - p ** 4))


def z_dispersion(totals, trials, prob):
    """Dispersion of many Binomial(trials, prob) totals about their KNOWN mean: sum (S - trials prob)^2 against its own
    closed-form mean m mu2 and variance m (mu4 - mu2^2), mu2 = n p (1 - p), mu4 = mu2 (1 + 3 (n - 2) p (1 - p))"""
    s = np.asarray(totals, np.float64).reshape(-1)
    p = float(prob)
    mu2 = trials * p * (1.0 - p)
    stat = float(((s - trials * p) ** 2).sum())
    return (stat - s.size * mu2) / sigma_dispersion(s.size, trials, p)


def sigma_dispersion(m, trials, prob):
    """the standard deviation of z_dispersion's sum of squares over m totals"""
    p = float(prob)
    mu2 = trials * p * (1.0 - p)
    mu4 = mu2 * (1.0 + 3.0 * (trials - 2) * p * (1.0 - p))
    return math.sqrt(m * (mu4 - mu2 * mu2))


def with_systematic(z, n, sigma_unit, systematic):
    """a z whose count may be off by n * systematic (a probability) for a KNOWN reason: the deviation less that allowance,
    never below 0; sigma_unit = the standard deviation of the count"""
    d = abs(z) * sigma_unit - n * float(systematic)
    return math.copysign(max(d, 0.0) / sigma_unit, z)


def chi2_statistic(obs, exp, var=None, systematic=None):
    """sum (|obs - exp| - systematic)_+^2 / var over the cells with exp > 0 -> (chi2, cells); var defaults to exp"""
    obs, exp = np.asarray(obs, np.float64), np.asarray(exp, np.float64)
    var = exp if var is None else np.asarray(var, np.float64)
    d = np.abs(obs - exp)
    if systematic is not None:
        d = np.maximum(d - np.asarray(systematic, np.float64), 0.0)
    keep = exp > 0
    return float((d[keep] ** 2 / var[keep]).sum()), int(keep.sum())


def chi2_tail(chi2, df):
    """P(chi-square with df degrees of freedom >= chi2): scipy's where it imports, else the Wilson-Hilferty cube root"""
    try:
        from scipy.stats import chi2 as dist
        return float(dist.sf(chi2, df))
    except ImportError:
        return chi2_tail_wilson_hilferty(chi2, df)


def chi2_tail_wilson_hilferty(chi2, df):
    z = ((chi2 / df) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * df))) / math.sqrt(2.0 / (9.0 * df))
    return 0.5 * math.erfc(z / math.sqrt(2.0))


def resolution(n, prob, zmax):
    """the relative error of `prob` at which |z_binomial| reaches zmax over n trials"""
    prob = float(prob)
    return zmax * math.sqrt((1.0 - prob) / (n * prob))


# ----------------------------------------------------------------------------- the plans the benchmark's workloads use
# name -> (flags of make_params, per-site weight levels or None, (k, R, cshift) the plan must have).  The plan depends on the
# rates through lam / L only: `scaled_rates` keeps that ratio at the test's L.
WORKLOAD_PLANS = {
    "cfg2": (dict(), None, (1, 1, 0)),
    "cfg3": (dict(HR_rate=0.5), None, (1, 2, 1)),
    "authors": (dict(core_mu=0.019, HR_rate=0.0), None, (0, 2, 0)),
    "hr_heavy": (dict(HR_rate=4.0), None, (0, 15, 2)),                 # cshift > 1: only the inline sweep takes it
    "weighted": (dict(), (0.0, 1.0, 2.0, 4.0), (0, 8, 1)),
}


def scaled_rates(core_size, n_core_mutations, n_recombinations_core, L):
    """the workload's per-individual core rates at L global sites instead of core_size"""
    return n_core_mutations * L / core_size, n_recombinations_core * L / core_size


def level_weights(levels, L):
    """(weights, level index per site): runs of five sites per level, so that a level is no residue class of the site number"""
    idx = (np.arange(L) // 5) % len(levels)
    return np.asarray(levels, np.float32)[idx], idx
