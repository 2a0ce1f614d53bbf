"""Jukes-Cantor likelihood of a tree over the C ABI (docs/TREE_LIKELIHOOD.md): the results of `tree_likelihood()` and
`tree_ml_lengths()`, the host restatements of both and the start lengths from parsimony changes.

All computation happens in the HIP library; this module only marshals buffers.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import PS_LIK_MAX_LENGTH, PS_LIK_MAX_POP, PS_LIK_MIN_LENGTH, Likelihood, MlParams, check
from .parsimony import _merge_list
from .population import _ptr, _Summary, fmt_f64

_LN2 = 0.6931471805599453094


class _LikSummary(_Summary):
    FIELDS = tuple(name for name, kind in Likelihood._fields_ if kind is C.c_uint64)
    REALS = tuple(name for name, kind in Likelihood._fields_ if kind is C.c_double)

    def _take(self, summary):
        super()._take(summary)
        for name in self.REALS:
            setattr(self, name, float(getattr(summary, name)))
        self.converged = bool(self.converged)


class TreeLikelihood(_LikSummary):
    """The result of `tree_likelihood` (ps_likelihood_t + the arrays): the summary fields as attributes (`lnl`, `tree_length`,
    `clamped_lengths`, `missing_cells`, ...), the merge list `left`, `right` and the `lengths` given, and, when asked for,
    `site_mant` (sites float64) and `site_exp` (sites int32) with `site_lnl` = log(mant) + exp ln 2 formed here, `branch_g` and
    `branch_h` (pop_size + merges float64: the sums of r and of r r over the sites, the root's 0).  What was not asked for is
    None."""

    def __init__(self, s, left, right, lengths, site_mant, site_exp, branch_g, branch_h):
        self._take(s)
        self.left, self.right, self.lengths = left, right, lengths
        self.site_mant, self.site_exp, self.branch_g, self.branch_h = site_mant, site_exp, branch_g, branch_h

    @property
    def site_lnl(self):
        """sites float64 (needs per_site): the log-likelihood of every site"""
        if self.site_mant is None:
            raise ValueError("site_lnl needs per_site=True")
        return np.log(self.site_mant) + self.site_exp.astype(np.float64) * _LN2

    def used_lengths(self):
        """pop_size + merges float64: the lengths as the pass used them (clamped; the root's 0)"""
        t = np.clip(self.lengths, PS_LIK_MIN_LENGTH, PS_LIK_MAX_LENGTH)
        t[-1] = 0.0
        return t

    def gradient(self):
        """pop_size + merges float64 (needs derivatives): dlnL/dt of the branch above every node, -(4 x / 3) g with
        x = exp(-4 t / 3) of the used length; the root's 0"""
        if self.branch_g is None:
            raise ValueError("gradient needs derivatives=True")
        x = np.exp(-4.0 * self.used_lengths() / 3.0)
        out = -(4.0 * x / 3.0) * self.branch_g
        out[-1] = 0.0
        return out

    def curvature(self):
        """pop_size + merges float64 (needs derivatives): d2lnL/dt2 of the branch above every node"""
        if self.branch_g is None:
            raise ValueError("curvature needs derivatives=True")
        x = np.exp(-4.0 * self.used_lengths() / 3.0)
        out = (16.0 * x * x / 9.0) * (-self.branch_h) + (16.0 * x / 9.0) * self.branch_g
        out[-1] = 0.0
        return out

    def as_dict(self):
        out = self._head(*self.REALS)
        out.update(left=self.left, right=self.right, lengths=self.lengths, site_mant=self.site_mant, site_exp=self.site_exp,
                   branch_g=self.branch_g, branch_h=self.branch_h)
        return out


class MlLengths(_LikSummary):
    """The result of `tree_ml_lengths` (ps_likelihood_t + the arrays): the summary fields as attributes (`lnl`, `start_lnl`,
    `rounds`, `passes`, `rollbacks`, `converged`, `tree_length`, ...), the merge list `left`, `right`, `lengths` (pop_size +
    merges float64: the maximum-likelihood length of the branch above every node in substitutions per site, the right root
    child's at the lower bound, the root's 0) and `round_lnl` (rounds + 1 float64: lnL at the start lengths, then after every
    round)."""

    def __init__(self, s, left, right, lengths, round_lnl):
        self._take(s)
        self.left, self.right, self.lengths, self.round_lnl = left, right, lengths, round_lnl

    def merges_list(self):
        """(left, right): the merge list in the numbering `tree_parsimony` takes"""
        return self.left, self.right

    def newick(self, order=None):
        """the tree as one line of Newick text, children as (left:len,right:len) with branch lengths in substitutions per site;
        leaf k is written as order[k] (None: k)"""
        n = self.pop_size
        names = [str(k) for k in range(n)] if order is None else [str(x) for x in order]
        if len(names) != n:
            raise ValueError("one name per leaf")
        root, out = n + self.merges - 1, []
        stack = [(True, root)]
        while stack:
            is_node, x = stack.pop()
            if not is_node:
                out.append(x)
                continue
            tail = ":" + fmt_f64(self.lengths[x]) if x != root else ""
            if x < n:
                out.append(names[x] + tail)
            else:
                out.append("(")
                stack += [(False, ")" + tail), (True, int(self.right[x - n])), (False, ","), (True, int(self.left[x - n]))]
        out.append(";\n")
        return "".join(out)

    def as_dict(self):
        out = self._head(*self.REALS)
        out.update(left=self.left, right=self.right, lengths=self.lengths, round_lnl=self.round_lnl)
        return out


def _lengths(lengths, nodes):
    lengths = np.ascontiguousarray(lengths, np.float64).reshape(-1)
    if lengths.size != nodes:
        raise ValueError("one length per node: pop_size + merges = %d values, not %d" % (nodes, lengths.size))
    return lengths


def _lik_call(fn, left, right, lengths, pop_size, sites, per_site, derivatives, *head):
    """fn(*head, left, right, length, merges, &summary, site_mant, site_exp, branch_g, branch_h) -> TreeLikelihood"""
    left, right = _merge_list(left, right)
    N, M, L = int(pop_size), left.size, int(sites)
    lengths = _lengths(lengths, N + M)
    mant = np.zeros(max(1, L), np.float64) if per_site else None
    exp = np.zeros(max(1, L), np.int32) if per_site else None
    g = np.zeros(N + M, np.float64) if derivatives else None
    h = np.zeros(N + M, np.float64) if derivatives else None
    s = Likelihood()
    check(fn(*head, _ptr(left), _ptr(right), _ptr(lengths), M, C.byref(s), _ptr(mant), _ptr(exp), _ptr(g), _ptr(h)))
    return TreeLikelihood(s, left, right, lengths, mant[:L] if per_site else None, exp[:L] if per_site else None, g, h)


def _ml_call(fn, left, right, lengths, pop_size, max_rounds, eps_lnl, *head):
    """fn(*head, left, right, length_in, merges, &params, &summary, length_out, round_lnl, round_cap) -> MlLengths"""
    left, right = _merge_list(left, right)
    N, M, R = int(pop_size), left.size, max(0, int(max_rounds))
    lengths = _lengths(lengths, N + M)
    out, rl = np.zeros(N + M, np.float64), np.zeros(R + 1, np.float64)
    prm, s = MlParams(R, float(eps_lnl)), Likelihood()
    check(fn(*head, _ptr(left), _ptr(right), _ptr(lengths), M, C.byref(prm), C.byref(s), _ptr(out), _ptr(rl), R + 1))
    return MlLengths(s, left, right, out, rl[:int(s.rounds) + 1])


def _start_lengths(handle, left, right):
    """the default start lengths of `tree_ml_lengths`: the Jukes-Cantor correction of the parsimony changes of every branch"""
    p = handle.tree_parsimony(left, right, branches=True)
    return jc_lengths_from_changes(p.branch_changes, p.sites)


def _rows(rows):
    rows = np.ascontiguousarray(rows, np.uint8)
    if rows.ndim != 2:
        raise ValueError("rows must be (pop_size, cols)")
    return rows


def likelihood_from_rows(rows, left, right, lengths, per_site=True, derivatives=True):
    """`Population.tree_likelihood` of an individual-major (pop_size, cols) uint8 matrix on the host alone
    (ps_likelihood_from_rows; no device): the sequential restatement through the same arithmetic, sites summed in ascending order
    -> a TreeLikelihood"""
    rows = _rows(rows)
    return _lik_call(_lib.load().ps_likelihood_from_rows, left, right, lengths, rows.shape[0], rows.shape[1], per_site, derivatives,
                     _ptr(rows), rows.shape[0], rows.shape[1])


def ml_lengths_from_rows(rows, left, right, lengths, max_rounds=50, eps_lnl=1e-3):
    """`Population.tree_ml_lengths` of an individual-major (pop_size, cols) uint8 matrix on the host alone
    (ps_ml_lengths_from_rows; no device) -> an MlLengths"""
    rows = _rows(rows)
    return _ml_call(_lib.load().ps_ml_lengths_from_rows, left, right, lengths, rows.shape[0], max_rounds, eps_lnl, _ptr(rows),
                    rows.shape[0], rows.shape[1])


def jc_lengths_from_changes(branch_changes, sites):
    """start lengths from the `branch_changes` of a TreeParsimony over `sites` sites (ps_jc_lengths_from_changes; host only): with
    p = changes / sites, -3/4 ln(1 - 4 p / 3); PS_LIK_MAX_LENGTH from p = 0.74 on"""
    ch = np.ascontiguousarray(branch_changes, np.uint64).reshape(-1)
    out = np.zeros(max(1, ch.size), np.float64)
    check(_lib.load().ps_jc_lengths_from_changes(_ptr(ch), ch.size, int(sites), _ptr(out)))
    return out[:ch.size]


__all__ = ["PS_LIK_MAX_LENGTH", "PS_LIK_MAX_POP", "PS_LIK_MIN_LENGTH", "MlLengths", "TreeLikelihood", "jc_lengths_from_changes",
           "likelihood_from_rows", "ml_lengths_from_rows"]
