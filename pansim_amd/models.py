"""Likelihood of a tree under the simulator's own substitution process over the C ABI (docs/TREE_MODEL.md): F81 with base
frequencies, a root distribution and up to 8 rate categories per site -- `SubstModel`, the results of `tree_model_likelihood()`
and `tree_model_ml_lengths()`, the host restatements of both, the start lengths from parsimony changes and the discrete-gamma
rates.

All likelihood computation happens in the HIP library; this module marshals buffers.  `gamma_rates` is host arithmetic on K
numbers (NumPy and `math` only).
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import (PS_MODEL_MAX_CATEGORIES, PS_MODEL_MAX_POP_DERIV, MlParams, ModelLikelihood as _CSummary,
                   SubstModelC, check)
from .likelihood import MlLengths, TreeLikelihood, _lengths, _LikSummary, _rows
from .parsimony import _merge_list
from .population import _ptr

SIMULATOR_FREQ = (0.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0)


# ------------------------------------------------------------------------------------------------------ discrete gamma
def _gamma_p(a, x):
    """the regularised incomplete gamma function P(a, x): its series below x = a + 1, else one minus Lentz's continued
    fraction of Q(a, x); both scaled by exp(a ln x - x - lgamma(a))"""
    if x <= 0.0:
        return 0.0
    front = math.exp(a * math.log(x) - x - math.lgamma(a))
    if x < a + 1.0:
        term = total = 1.0 / a
        n = a
        for _ in range(10000):
            n += 1.0
            term *= x / n
            total += term
            if abs(term) < abs(total) * 1e-17:
                break
        return min(1.0, front * total)
    tiny = 1e-300
    b = x + 1.0 - a
    c, d = 1.0 / tiny, 1.0 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return max(0.0, 1.0 - front * h)


def _gamma_quantile(a, p):
    """x with P(a, x) = p by bisection (in ln x below 1: the small quantiles of a small shape span many decades)"""
    lo, hi = 0.0, max(1.0, a)
    while _gamma_p(a, hi) < p:
        hi *= 2.0
    for _ in range(400):
        mid = math.sqrt(lo * hi) if lo > 0.0 and hi / lo > 4.0 else 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if _gamma_p(a, mid) < p:
            lo = mid
        else:
            hi = mid
        if lo == 0.0 and hi < 1e-300:
            break
    return 0.5 * (lo + hi)


def gamma_bounds(alpha, categories):
    """the K - 1 inner category bounds b_i of the rate distribution Gamma(alpha, alpha): P(alpha, alpha b_i) = i / K"""
    alpha, K = float(alpha), int(categories)
    if not (alpha > 0.0 and math.isfinite(alpha)) or not 1 <= K <= PS_MODEL_MAX_CATEGORIES:
        raise ValueError("alpha must be a positive number and 1 <= categories <= %d" % PS_MODEL_MAX_CATEGORIES)
    return np.array([_gamma_quantile(alpha, i / K) / alpha for i in range(1, K)], np.float64)


def gamma_rates(alpha, categories=4):
    """K equal-weight rates: the means of the K equal-probability categories of Gamma(alpha, alpha), rescaled to mean 1.  The mean
    of the category between the bounds b_lo, b_hi is K (P(alpha + 1, alpha b_hi) - P(alpha + 1, alpha b_lo))."""
    K = int(categories)
    b = gamma_bounds(alpha, K)
    alpha = float(alpha)
    cum = np.array([0.0] + [_gamma_p(alpha + 1.0, alpha * v) for v in b] + [1.0])
    rates = np.diff(cum) * K
    return rates / rates.mean()


# --------------------------------------------------------------------------------------------------------------- model
class SubstModel:
    """ps_subst_model: `freq` pi (4 values >= 0, at most one 0), `root` rho (4 values > 0; None: pi, which makes the model
    reversible), `rates` r_k >= 0 and `weights` w_k > 0 of 1 .. 8 categories (None: equal), `site_class` (None: every site a mixture
    of the categories; else one uint8 < K per core site -- of the handle for a Population and the host entries, of the whole run
    for a Simulation or MultiSimulation).  The library validates; this class only holds the values."""

    def __init__(self, freq, root=None, rates=(1.0,), weights=None, site_class=None):
        self.freq = np.ascontiguousarray(freq, np.float64).reshape(-1)
        self.root = self.freq.copy() if root is None else np.ascontiguousarray(root, np.float64).reshape(-1)
        self.rates = np.ascontiguousarray(rates, np.float64).reshape(-1)
        K = self.rates.size
        self.weights = np.full(K, 1.0 / K if K else 0.0) if weights is None else np.ascontiguousarray(weights, np.float64).reshape(-1)
        if self.freq.size != 4 or self.root.size != 4:
            raise ValueError("freq and root have four entries: the bases 1, 2, 4, 8")
        if self.weights.size != K:
            raise ValueError("one weight per rate")
        self.site_class = None if site_class is None else np.ascontiguousarray(site_class, np.uint8).reshape(-1)

    @classmethod
    def jc69(cls):
        """Jukes-Cantor: pi = rho = 1/4, one category of rate 1 -- the same site likelihoods, bit for bit, as tree_likelihood"""
        return cls((0.25, 0.25, 0.25, 0.25))

    @classmethod
    def simulator(cls, root=(0.25, 0.25, 0.25, 0.25), **rates):
        """the simulator's core mutation: a hit cell is redrawn from {2, 4, 8} (pi = (0, 1/3, 1/3, 1/3)), the founding genome is
        uniform over the four bases (rho = 1/4).  `rates`, `weights`, `site_class` as the constructor takes them."""
        return cls(SIMULATOR_FREQ, root=root, **rates)

    @classmethod
    def gamma(cls, alpha, categories=4, freq=(0.25, 0.25, 0.25, 0.25), root=None):
        """discrete-gamma rate heterogeneity: a mixture of `categories` equal-weight categories with gamma_rates(alpha)"""
        return cls(freq, root=root, rates=gamma_rates(alpha, categories))

    @property
    def categories(self):
        return self.rates.size

    @property
    def beta(self):
        """1 - sum pi_a^2: substitutions per event"""
        f = self.freq
        return 1.0 - ((f[0] * f[0] + f[1] * f[1]) + (f[2] * f[2] + f[3] * f[3]))

    def sliced(self, lo, hi):
        """the model of the sites [lo, hi): site_class cut, everything else shared"""
        return SubstModel(self.freq, self.root, self.rates, self.weights, None if self.site_class is None else self.site_class[lo:hi])

    def _c(self):
        """(the C struct, what must stay alive while it is used)"""
        K = self.rates.size
        if K > PS_MODEL_MAX_CATEGORIES:
            raise ValueError("at most %d categories" % PS_MODEL_MAX_CATEGORIES)
        m = SubstModelC()
        m.freq[:] = list(self.freq)
        m.root[:] = list(self.root)
        m.categories = K
        m.rate[:K] = list(self.rates)
        m.weight[:K] = list(self.weights)
        if self.site_class is not None:
            m.site_class = self.site_class.ctypes.data_as(C.c_void_p)
            m.site_classes = self.site_class.size
        return m, self.site_class


class _ModelSummary(_LikSummary):
    FIELDS = tuple(name for name, kind in _CSummary._fields_ if kind is C.c_uint64)
    REALS = tuple(name for name, kind in _CSummary._fields_ if kind is C.c_double)

    def _take(self, summary):
        super()._take(summary)
        self.classed = bool(self.classed)


class ModelLikelihood(_ModelSummary, TreeLikelihood):
    """The result of `tree_model_likelihood` (ps_model_likelihood_t + the arrays): the summary fields as attributes (`lnl`,
    `tree_length`, `categories`, `classed`, `beta`, `mean_rate`, ...), `model`, the merge list and the `lengths` given, and, when
    asked for, `site_mant`, `site_exp` (with `site_lnl`), `site_rate` (sites float64: the posterior mean rate) and `branch_g`,
    `branch_h`, `branch_q` (pop_size + merges float64, the root's 0).  What was not asked for is None."""

    def __init__(self, s, model, left, right, lengths, site_mant, site_exp, site_rate, branch_g, branch_h, branch_q):
        TreeLikelihood.__init__(self, s, left, right, lengths, site_mant, site_exp, branch_g, branch_h)
        self.model, self.site_rate, self.branch_q = model, site_rate, branch_q

    def events(self):
        """pop_size + merges float64: the used lengths in events per site, t / beta"""
        return self.used_lengths() / self.beta

    def gradient(self):
        """pop_size + merges float64 (needs derivatives): dlnL/dt of the branch above every node, -g / beta; the root's 0"""
        if self.branch_g is None:
            raise ValueError("gradient needs derivatives=True")
        return -self.branch_g / self.beta

    def curvature(self):
        """pop_size + merges float64 (needs derivatives): d2lnL/dt2 of the branch above every node, (q - h) / beta^2"""
        if self.branch_g is None:
            raise ValueError("curvature needs derivatives=True")
        return (self.branch_q - self.branch_h) / (self.beta * self.beta)

    def as_dict(self):
        out = TreeLikelihood.as_dict(self)
        out.update(site_rate=self.site_rate, branch_q=self.branch_q)
        return out


class ModelMlLengths(_ModelSummary, MlLengths):
    """The result of `tree_model_ml_lengths` (ps_model_likelihood_t + the arrays): as MlLengths, the lengths in substitutions per
    site at rate 1 under pi (`events()`: in events per site); with a reversible model the right root child's length is at the
    lower bound, otherwise both root branches are estimated."""

    def __init__(self, s, model, left, right, lengths, round_lnl):
        MlLengths.__init__(self, s, left, right, lengths, round_lnl)
        self.model = model

    def events(self):
        """pop_size + merges float64: the lengths in events per site, t / beta"""
        return self.lengths / self.beta


def _model_call(fn, left, right, lengths, model, pop_size, sites, per_site, derivatives, *head):
    """fn(*head, left, right, length, merges, &model, &summary, site_mant, site_exp, site_rate, g, h, q) -> ModelLikelihood"""
    left, right = _merge_list(left, right)
    N, M, L = int(pop_size), left.size, int(sites)
    lengths = _lengths(lengths, N + M)
    mant, rate = (np.zeros(max(1, L), np.float64) for _ in range(2)) if per_site else (None, None)
    exp = np.zeros(max(1, L), np.int32) if per_site else None
    g, h, q = (np.zeros(N + M, np.float64) for _ in range(3)) if derivatives else (None, None, None)
    s = _CSummary()
    cm, keep = model._c()
    check(fn(*head, _ptr(left), _ptr(right), _ptr(lengths), M, C.byref(cm), C.byref(s), _ptr(mant), _ptr(exp), _ptr(rate), _ptr(g), _ptr(h), _ptr(q)))
    del keep
    cut = (lambda a: a[:L]) if per_site else (lambda a: None)
    return ModelLikelihood(s, model, left, right, lengths, cut(mant), cut(exp), cut(rate), g, h, q)


def _model_ml_call(fn, left, right, lengths, model, pop_size, max_rounds, eps_lnl, *head):
    """fn(*head, left, right, length_in, merges, &model, &params, &summary, length_out, round_lnl, round_cap) -> ModelMlLengths"""
    left, right = _merge_list(left, right)
    N, M, R = int(pop_size), left.size, max(0, int(max_rounds))
    lengths = _lengths(lengths, N + M)
    out, rl = np.zeros(N + M, np.float64), np.zeros(R + 1, np.float64)
    prm, s = MlParams(R, float(eps_lnl)), _CSummary()
    cm, keep = model._c()
    check(fn(*head, _ptr(left), _ptr(right), _ptr(lengths), M, C.byref(cm), C.byref(prm), C.byref(s), _ptr(out), _ptr(rl), R + 1))
    del keep
    return ModelMlLengths(s, model, left, right, out, rl[:int(s.rounds) + 1])


def _model_start_lengths(handle, left, right, model):
    """the default start lengths of `tree_model_ml_lengths`: the F81 correction of the parsimony changes of every branch"""
    p = handle.tree_parsimony(left, right, branches=True)
    return f81_lengths_from_changes(p.branch_changes, p.sites, model.freq)


def model_likelihood_from_rows(rows, left, right, lengths, model, per_site=True, derivatives=True):
    """`Population.tree_model_likelihood` of an individual-major (pop_size, cols) uint8 matrix on the host alone
    (ps_model_likelihood_from_rows; no device): the same arithmetic, sites summed in ascending order -> a ModelLikelihood"""
    rows = _rows(rows)
    return _model_call(_lib.load().ps_model_likelihood_from_rows, left, right, lengths, model, rows.shape[0], rows.shape[1], per_site, derivatives,
                       _ptr(rows), rows.shape[0], rows.shape[1])


def model_ml_lengths_from_rows(rows, left, right, lengths, model, max_rounds=50, eps_lnl=1e-3):
    """`Population.tree_model_ml_lengths` of an individual-major (pop_size, cols) uint8 matrix on the host alone
    (ps_model_ml_lengths_from_rows; no device) -> a ModelMlLengths"""
    rows = _rows(rows)
    return _model_ml_call(_lib.load().ps_model_ml_lengths_from_rows, left, right, lengths, model, rows.shape[0], max_rounds, eps_lnl, _ptr(rows),
                          rows.shape[0], rows.shape[1])


def f81_lengths_from_changes(branch_changes, sites, freq):
    """start lengths from the `branch_changes` of a TreeParsimony over `sites` sites under base frequencies `freq`
    (ps_f81_lengths_from_changes; host only): with p = changes / sites, -beta ln(1 - p / beta); PS_LIK_MAX_LENGTH from
    p = 0.98 beta on"""
    ch = np.ascontiguousarray(branch_changes, np.uint64).reshape(-1)
    f = np.ascontiguousarray(freq, np.float64).reshape(-1)
    if f.size != 4:
        raise ValueError("freq has four entries")
    out = np.zeros(max(1, ch.size), np.float64)
    check(_lib.load().ps_f81_lengths_from_changes(_ptr(ch), ch.size, int(sites), _ptr(f), _ptr(out)))
    return out[:ch.size]


__all__ = ["PS_MODEL_MAX_CATEGORIES", "PS_MODEL_MAX_POP_DERIV", "ModelLikelihood", "ModelMlLengths", "SubstModel", "f81_lengths_from_changes",
           "gamma_bounds", "gamma_rates", "model_likelihood_from_rows", "model_ml_lengths_from_rows"]
