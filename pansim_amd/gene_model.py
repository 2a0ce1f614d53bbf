"""Gene gain and loss on a tree over the C ABI (docs/GENE_MODEL.md): the two-state likelihood of the accessory matrix under a
`GeneModel`, its rate fit, and the gene content of the inner nodes as a new Population on the device -- the results of
`tree_gene_likelihood()`, `tree_gene_ancestral()` and `tree_gene_fit()`, and the host restatements of the three.

All computation happens in the HIP library; this module marshals buffers.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (PS_GENE_MAX_POP, PS_GENE_MAX_POP_MIX, PS_MODEL_MAX_CATEGORIES, GeneFitParams, GeneModelC, GeneSummary as _CSummary,
                   check)
from .likelihood import _lengths, _rows
from .parsimony import _merge_list
from .population import _ptr


class GeneModel:
    """ps_gene_model: `freq` pi = (pi_0, pi_1) of absent and present (both > 0), `root` rho (None: pi), `rates` r_k >= 0 and
    `weights` w_k > 0 of 1 .. 8 classes (None: equal), `gene_class` (None: every gene a mixture of the classes; else one uint8 < K
    per gene).  P(t) = x I + (1 - x) 1 pi^T with x = exp(-r t / beta), beta = 1 - pi_0^2 - pi_1^2: a gene is gained at rate
    r pi_1 / beta and lost at rate r pi_0 / beta.  The library validates; this class only holds the values."""

    def __init__(self, freq, root=None, rates=(1.0,), weights=None, gene_class=None):
        self.freq = np.ascontiguousarray(freq, np.float64).reshape(-1)
        self.root = self.freq.copy() if root is None else np.ascontiguousarray(root, np.float64).reshape(-1)
        self.rates = np.ascontiguousarray(rates, np.float64).reshape(-1)
        K = self.rates.size
        self.weights = np.full(K, 1.0 / K if K else 0.0) if weights is None else np.ascontiguousarray(weights, np.float64).reshape(-1)
        if self.freq.size != 2 or self.root.size != 2:
            raise ValueError("freq and root have two entries: absent, present")
        if self.weights.size != K:
            raise ValueError("one weight per rate")
        self.gene_class = None if gene_class is None else np.ascontiguousarray(gene_class, np.uint8).reshape(-1)

    @classmethod
    def from_gain_loss(cls, gain, loss, root=None, weights=None, gene_class=None):
        """the model of per-class gain and loss rates (scalars or one value per class; one pi for all classes, so gain / loss is
        the same in every class): pi_1 = gain / (gain + loss), r = 2 gain loss / (gain + loss)"""
        gain, loss = np.atleast_1d(np.asarray(gain, np.float64)), np.atleast_1d(np.asarray(loss, np.float64))
        gain, loss = np.broadcast_arrays(gain, loss)
        pi1 = gain[0] / (gain[0] + loss[0])
        if not np.allclose(gain / (gain + loss), pi1, rtol=1e-12, atol=0.0):
            raise ValueError("every class has the same gain / (gain + loss): the model has one pi")
        return cls((1.0 - pi1, pi1), root=root, rates=2.0 * gain * loss / (gain + loss), weights=weights, gene_class=gene_class)

    @classmethod
    def simulator(cls, sim_or_params):
        """the simulator's own gain / loss law for lengths in generations: pi = (1/2, 1/2), the classes are the
        run's compartments with r_c = lambda_c / |c|, every gene assigned to its compartment, rho_1 the share of the accessory
        genes the founder carries.  `sim_or_params`: a Simulation, a MultiSimulation or a SimParams."""
        from .population import init_vector
        from .simulation import derive
        params = getattr(sim_or_params, "params", sim_or_params)
        d = derive(params)
        G, n = int(d.pan_size), int(d.n_comp)
        size = [int(d.comp_end[c]) - int(d.comp_begin[c]) for c in range(n)]
        rates = [float(d.n_pan_mutations[c]) / size[c] if size[c] else 0.0 for c in range(n)]
        cls_of = np.zeros(G, np.uint8)
        for c in range(n):
            cls_of[int(d.comp_begin[c]):int(d.comp_end[c])] = c
        rho1 = float(init_vector(params.seed, False, G, d.avg_gene_freq_adj).mean()) if G else 0.5
        rho1 = min(max(rho1, 1e-9), 1.0 - 1e-9)
        share = np.array([s / max(1, G) for s in size], np.float64)
        return cls((0.5, 0.5), root=(1.0 - rho1, rho1), rates=rates, weights=share / share.sum() if G else None, gene_class=cls_of)

    def mixture(self):
        """the same model without `gene_class`: every gene a mixture of the classes, the weights the class shares (the weights as
        they are when there are no gene classes)"""
        w = self.weights
        if self.gene_class is not None and self.gene_class.size:
            w = np.bincount(self.gene_class, minlength=self.categories).astype(np.float64) / self.gene_class.size
        return GeneModel(self.freq, self.root, self.rates, w)

    @property
    def categories(self):
        return self.rates.size

    @property
    def beta(self):
        """1 - pi_0^2 - pi_1^2"""
        f = self.freq
        return 1.0 - (f[0] * f[0] + f[1] * f[1])

    def gain_loss(self):
        """(gain, loss): K float64 each, r_k pi_1 / beta and r_k pi_0 / beta"""
        return self.rates * self.freq[1] / self.beta, self.rates * self.freq[0] / self.beta

    def _c(self):
        """(the C struct, what must stay alive while it is used)"""
        K = self.rates.size
        if K > PS_MODEL_MAX_CATEGORIES:
            raise ValueError("at most %d classes" % PS_MODEL_MAX_CATEGORIES)
        m = GeneModelC()
        m.freq[:] = list(self.freq)
        m.root[:] = list(self.root)
        m.categories = K
        m.rate[:K] = list(self.rates)
        m.weight[:K] = list(self.weights)
        if self.gene_class is not None:
            m.gene_class = self.gene_class.ctypes.data_as(C.c_void_p)
            m.gene_classes = self.gene_class.size
        return m, self.gene_class


class _GeneSummary:
    FIELDS = tuple(name for name, kind in _CSummary._fields_ if kind is C.c_uint64)
    REALS = tuple(name for name, kind in _CSummary._fields_ if kind is C.c_double)

    def _take(self, s, model, left, right, lengths):
        for name in self.FIELDS:
            setattr(self, name, int(getattr(s, name)))
        for name in self.REALS:
            setattr(self, name, float(getattr(s, name)))
        self.classed, self.converged = bool(self.classed), bool(self.converged)
        self.model, self.left, self.right, self.lengths = model, left, right, lengths

    def as_dict(self):
        return {name: getattr(self, name) for name in self.FIELDS + self.REALS}


class GeneLikelihood(_GeneSummary):
    """The result of `tree_gene_likelihood` (ps_gene_t + the arrays): the summary fields as attributes (`lnl`, `genes`,
    `categories`, `classed`, `zero_genes`, `clamped_lengths`, `beta`, `mean_rate`, ...) and, with per_gene, `gene_mant`, `gene_exp`
    (with `gene_lnl()`), `gene_post` (genes x K) and `gene_rate`; None otherwise."""

    def __init__(self, s, model, left, right, lengths, mant, exp, post, rate):
        self._take(s, model, left, right, lengths)
        self.gene_mant, self.gene_exp, self.gene_post, self.gene_rate = mant, exp, post, rate

    def gene_lnl(self):
        """genes float64: ln of every gene's likelihood (-inf for a gene of likelihood 0)"""
        with np.errstate(divide="ignore"):
            return np.log(self.gene_mant) + self.gene_exp * np.log(2.0)

    def gene_best_class(self):
        """genes int: the class of the largest posterior, ties to the lowest"""
        return np.argmax(self.gene_post, axis=1)


class GeneAncestral(_GeneSummary):
    """The result of `tree_gene_ancestral`: the summary fields (`lnl`, `total_gains`, `total_losses`, `mean_conf`, `total_genes`,
    ...), `node_conf` and `node_genes` (merges float64: the summed confidence and the expected accessory genome size of every inner
    node), `branch_gains`, `branch_losses` (pop_size + merges float64, the root's 0), `gene_gains`, `gene_losses` (genes float64)
    and `population`: the reconstructed gene content, row k = node pop_size + k, as an accessory Population that owns its handle
    (None when the states were not asked for; `rows` instead for the host restatement)."""

    def __init__(self, s, model, left, right, lengths, arrays, population=None, rows=None):
        self._take(s, model, left, right, lengths)
        (self.node_conf, self.node_genes, self.branch_gains, self.branch_losses, self.gene_gains, self.gene_losses) = arrays
        self.population, self.rows = population, rows

    def close(self):
        if self.population is not None:
            self.population.close()
            self.population = None


class GeneFit(_GeneSummary):
    """The result of `tree_gene_fit`: the summary fields (`lnl`, `start_lnl`, `rounds`, `passes`, `converged`, ...), `model` -- the
    fitted GeneModel (the start's rho and gene classes) -- and `round_lnl` (rounds + 1 float64: [0] the start's lnL)."""

    def __init__(self, s, start, left, right, lengths, rates, weights, freq, round_lnl):
        fitted = GeneModel(freq, start.root, rates, weights, start.gene_class)
        self._take(s, fitted, left, right, lengths)
        self.start_model, self.round_lnl = start, round_lnl


def _head(left, right, lengths, pop_size):
    left, right = _merge_list(left, right)
    N, M = int(pop_size), left.size
    return left, right, _lengths(lengths, N + M), N, M


def _lik_call(fn, left, right, lengths, model, pop_size, genes, per_gene, *head):
    """fn(*head, left, right, length, merges, &model, &summary, gene_mant, gene_exp, gene_post, gene_rate) -> GeneLikelihood"""
    left, right, lengths, N, M = _head(left, right, lengths, pop_size)
    G, K = int(genes), model.categories
    mant, rate = (np.zeros(max(1, G), np.float64) for _ in range(2)) if per_gene else (None, None)
    exp = np.zeros(max(1, G), np.int32) if per_gene else None
    post = np.zeros((max(1, G), max(1, K)), np.float64) if per_gene else None
    s = _CSummary()
    cm, keep = model._c()
    check(fn(*head, _ptr(left), _ptr(right), _ptr(lengths), M, C.byref(cm), C.byref(s), _ptr(mant), _ptr(exp), _ptr(post), _ptr(rate)))
    del keep
    cut = (lambda a: a[:G]) if per_gene else (lambda a: None)
    return GeneLikelihood(s, model, left, right, lengths, cut(mant), cut(exp), cut(post), cut(rate))


def _anc_call(fn, left, right, lengths, model, pop_size, genes, out_arg, *head):
    """fn(*head, left, right, length, merges, &model, &summary, out_arg, the six arrays) -> (summary, ..., the six arrays)"""
    left, right, lengths, N, M = _head(left, right, lengths, pop_size)
    G = int(genes)
    conf, ngenes = np.zeros(max(1, M), np.float64), np.zeros(max(1, M), np.float64)
    bg, bl = np.zeros(N + M, np.float64), np.zeros(N + M, np.float64)
    gg, gl = np.zeros(max(1, G), np.float64), np.zeros(max(1, G), np.float64)
    s = _CSummary()
    cm, keep = model._c()
    check(fn(*head, _ptr(left), _ptr(right), _ptr(lengths), M, C.byref(cm), C.byref(s), out_arg, _ptr(conf), _ptr(ngenes), _ptr(bg), _ptr(bl),
             _ptr(gg), _ptr(gl)))
    del keep
    return s, left, right, lengths, (conf[:M], ngenes[:M], bg, bl, gg[:G], gl[:G])


def _anc_device_call(fn, like, left, right, lengths, model, pop_size, states, *head):
    """a device entry -> GeneAncestral; `like`: the accessory Population the new handle is shaped like"""
    from .samples import _wrap
    h = C.c_void_p()
    s, left, right, lengths, arrays = _anc_call(fn, left, right, lengths, model, pop_size, like.ncols, C.byref(h) if states else None, *head)
    made = _wrap(like, h, int(s.merges)) if states else None
    return GeneAncestral(s, model, left, right, lengths, arrays, population=made)


def _fit_call(fn, left, right, lengths, model, pop_size, fit_rates, fit_freq, fit_weights, max_rounds, eps_lnl, *head):
    """fn(*head, left, right, length, merges, &model, &params, &summary, rate_out, weight_out, freq_out, round_lnl, round_cap)"""
    left, right, lengths, N, M = _head(left, right, lengths, pop_size)
    K, R = model.categories, max(0, int(max_rounds))
    rates, weights, freq, rl = np.zeros(max(1, K)), np.zeros(max(1, K)), np.zeros(2), np.zeros(R + 1)
    prm, s = GeneFitParams(int(bool(fit_rates)), int(bool(fit_freq)), int(bool(fit_weights)), R, float(eps_lnl)), _CSummary()
    cm, keep = model._c()
    check(fn(*head, _ptr(left), _ptr(right), _ptr(lengths), M, C.byref(cm), C.byref(prm), C.byref(s), _ptr(rates), _ptr(weights), _ptr(freq),
             _ptr(rl), R + 1))
    del keep
    return GeneFit(s, model, left, right, lengths, rates[:K], weights[:K], freq, rl[:int(s.rounds) + 1])


class _GeneReadouts:
    """`tree_gene_*` of a run (mixed into Simulation and MultiSimulation): the run's accessory matrix, shard 0's replica of a
    sharded run"""

    def tree_gene_likelihood(self, left, right, lengths, model, per_gene=False):
        """Population.tree_gene_likelihood() of the run's accessory matrix (ps_sim_tree_gene_likelihood /
        ps_multi_tree_gene_likelihood; docs/GENE_MODEL.md) -> a GeneLikelihood"""
        return _lik_call(self._entry("tree_gene_likelihood"), left, right, lengths, model, self.params.pop_size, self.pan_genome.ncols, per_gene,
                         self._h)

    def tree_gene_ancestral(self, left, right, lengths, model, states=True):
        """Population.tree_gene_ancestral() of the run's accessory matrix (ps_sim_tree_gene_ancestral /
        ps_multi_tree_gene_ancestral) -> a GeneAncestral"""
        return _anc_device_call(self._entry("tree_gene_ancestral"), self.pan_genome, left, right, lengths, model, self.params.pop_size, states,
                                self._h)

    def tree_gene_fit(self, left, right, lengths, model, fit_rates=True, fit_freq=True, fit_weights=True, max_rounds=50, eps_lnl=1e-3):
        """Population.tree_gene_fit() of the run's accessory matrix (ps_sim_tree_gene_fit / ps_multi_tree_gene_fit) -> a GeneFit"""
        return _fit_call(self._entry("tree_gene_fit"), left, right, lengths, model, self.params.pop_size, fit_rates, fit_freq, fit_weights,
                         max_rounds, eps_lnl, self._h)

    def tree_gene_timing(self):
        """device ms of (the uploads, the kernels, the sums of the rows) of the last tree_gene_*() call"""
        return self.pan_genome.tree_gene_timing()


def gene_likelihood_from_rows(rows, left, right, lengths, model, per_gene=True):
    """`Population.tree_gene_likelihood` of an individual-major (pop_size, genes) uint8 matrix on the host alone
    (ps_gene_likelihood_from_rows; no device): the same arithmetic, genes summed in ascending order -> a GeneLikelihood"""
    rows = _rows(rows)
    return _lik_call(_lib.load().ps_gene_likelihood_from_rows, left, right, lengths, model, rows.shape[0], rows.shape[1], per_gene, _ptr(rows),
                     rows.shape[0], rows.shape[1])


def gene_ancestral_from_rows(rows, left, right, lengths, model, states=True):
    """`Population.tree_gene_ancestral` on the host alone (ps_gene_ancestral_from_rows; no device) -> a GeneAncestral whose `rows`
    is the (merges, genes) uint8 matrix 0 / 1 of the inner nodes"""
    rows = _rows(rows)
    out = np.zeros((max(1, rows.shape[0] - 1), rows.shape[1]), np.uint8) if states else None
    s, left, right, lengths, arrays = _anc_call(_lib.load().ps_gene_ancestral_from_rows, left, right, lengths, model, rows.shape[0], rows.shape[1],
                                                _ptr(out), _ptr(rows), rows.shape[0], rows.shape[1])
    return GeneAncestral(s, model, left, right, lengths, arrays, rows=None if out is None else out[:int(s.merges)])


def gene_fit_from_rows(rows, left, right, lengths, model, fit_rates=True, fit_freq=True, fit_weights=True, max_rounds=50, eps_lnl=1e-3):
    """`Population.tree_gene_fit` on the host alone (ps_gene_fit_from_rows; no device): the same loop over host passes, the same
    decisions and the same bits -> a GeneFit"""
    rows = _rows(rows)
    return _fit_call(_lib.load().ps_gene_fit_from_rows, left, right, lengths, model, rows.shape[0], fit_rates, fit_freq, fit_weights, max_rounds,
                     eps_lnl, _ptr(rows), rows.shape[0], rows.shape[1])


__all__ = ["PS_GENE_MAX_POP", "PS_GENE_MAX_POP_MIX", "GeneAncestral", "GeneFit", "GeneLikelihood", "GeneModel", "gene_ancestral_from_rows",
           "gene_fit_from_rows", "gene_likelihood_from_rows"]
