"""Marginal ancestral states over the C ABI (docs/ANCESTRAL_STATES.md): the sequences at the inner nodes of a tree, reconstructed
under a `SubstModel` -- the result of `ancestral_states()` with the reconstructed genomes as a new Population on the device, and
the host restatement `ancestral_from_rows`.

All computation happens in the HIP library; this module marshals buffers.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import PS_ANC_MAX_POP, PS_ANC_MAX_POP_MIX, Ancestral as _CSummary, check
from .likelihood import _lengths, _rows
from .parsimony import _merge_list
from .population import _ptr


class AncestralStates:
    """The result of `ancestral_states` (ps_ancestral_t + the arrays): the summary fields as attributes (`pop_size`, `sites`,
    `merges`, `categories`, `classed`, `lnl`, `mean_conf`, `total_diff`, `masked_cells`, `zero_sites`, `missing_cells`,
    `clamped_lengths`), `model`, the merge list and the `lengths` given, `node_conf` (merges float64: the summed confidence of every
    inner node), `branch_diff` (pop_size + merges float64: the expected number of sites at which the two ends of the branch above
    every node differ; the root's 0) and `population`: the reconstructed genomes, row k = node pop_size + k, as a Population that
    owns its handle (None when the states were not asked for; `rows` instead for the host restatement)."""

    FIELDS = tuple(name for name, kind in _CSummary._fields_ if kind is C.c_uint64)
    REALS = tuple(name for name, kind in _CSummary._fields_ if kind is C.c_double)

    def __init__(self, s, model, left, right, lengths, node_conf, branch_diff, population=None, rows=None):
        for name in self.FIELDS:
            setattr(self, name, int(getattr(s, name)))
        for name in self.REALS:
            setattr(self, name, float(getattr(s, name)))
        self.classed = bool(self.classed)
        self.model, self.left, self.right, self.lengths = model, left, right, lengths
        self.node_conf, self.branch_diff, self.population, self.rows = node_conf, branch_diff, population, rows

    def counted_sites(self):
        """the sites that have a likelihood in this tree: sites - zero_sites"""
        return self.sites - self.zero_sites

    def node_accuracy(self):
        """merges float64: the expected share of every inner node's sites that are reconstructed correctly, node_conf / counted
        sites"""
        return self.node_conf / max(1, self.counted_sites())

    def as_dict(self):
        out = {name: getattr(self, name) for name in self.FIELDS + self.REALS}
        out.update(node_conf=self.node_conf, branch_diff=self.branch_diff)
        return out

    def close(self):
        if self.population is not None:
            self.population.close()
            self.population = None


def _anc_call(fn, left, right, lengths, model, pop_size, min_posterior, *head):
    """fn(*head, left, right, length, merges, &model, min_posterior, &summary) -> (summary, the arrays); the caller appends its
    own tail through `finish`"""
    left, right = _merge_list(left, right)
    N, M = int(pop_size), left.size
    lengths = _lengths(lengths, N + M)
    conf, diff = np.zeros(max(1, M), np.float64), np.zeros(N + M, np.float64)
    s = _CSummary()
    cm, keep = model._c()

    def finish(out_arg):
        check(fn(*head, _ptr(left), _ptr(right), _ptr(lengths), M, C.byref(cm), float(min_posterior), C.byref(s), out_arg, _ptr(conf), _ptr(diff)))
        return s, left, right, lengths, conf[:M], diff

    return finish, keep


def _device_call(fn, like, ncols, left, right, lengths, model, pop_size, min_posterior, states, *head):
    """a device entry -> AncestralStates; `like`: the Population the new handle is shaped like, `ncols` its columns"""
    from .samples import _wrap
    finish, keep = _anc_call(fn, left, right, lengths, model, pop_size, min_posterior, *head)
    h = C.c_void_p()
    s, left, right, lengths, conf, diff = finish(C.byref(h) if states else None)
    del keep
    made = _wrap(like, h, int(s.merges), ncols=ncols) if states else None
    return AncestralStates(s, model, left, right, lengths, conf, diff, population=made)


def ancestral_from_rows(rows, left, right, lengths, model, min_posterior=0.0, states=True):
    """`Population.ancestral_states` of an individual-major (pop_size, cols) uint8 matrix on the host alone
    (ps_ancestral_from_rows; no device): the same arithmetic, sites summed in ascending order -> an AncestralStates whose `rows`
    is the (merges, cols) uint8 matrix of the inner nodes"""
    rows = _rows(rows)
    finish, keep = _anc_call(_lib.load().ps_ancestral_from_rows, left, right, lengths, model, rows.shape[0], min_posterior, _ptr(rows),
                             rows.shape[0], rows.shape[1])
    out = np.zeros((max(1, rows.shape[0] - 1), rows.shape[1]), np.uint8) if states else None
    s, left, right, lengths, conf, diff = finish(_ptr(out))
    del keep
    return AncestralStates(s, model, left, right, lengths, conf, diff, rows=None if out is None else out[:int(s.merges)])


__all__ = ["PS_ANC_MAX_POP", "PS_ANC_MAX_POP_MIX", "AncestralStates", "ancestral_from_rows"]
