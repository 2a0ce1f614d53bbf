"""Likelihood tree search over the C ABI (docs/LIKELIHOOD_SEARCH.md): the results of `model_nni_deltas()` and `tree_model_nni()`,
the canonical form of a merge list with its lengths, one interchange applied with its lengths, and the host restatements of a
pass and of the search.

All computation happens in the HIP library; this module marshals buffers and forms log(mantissa) + exponent ln 2 of the 2 merges
products a pass returns.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import PS_MODEL_NNI_MAX_POP, MlNni, MlNniParams, check
from .likelihood import MlLengths, _lengths, _rows
from .parsimony import _merge_list
from .population import _MergeCount, _ptr, _Summary

_LN2 = 0.6931471805599453094


class ModelNniDeltas:
    """The result of `model_nni_deltas` (one pass): `lnl` of the tree, `delta` ((merges, 2) float64: the change of lnL under
    interchange (pop_size + k, kind), exact up to the rounding of a product of site ratios; NaN where there is no candidate), the
    products themselves as `delta_mant` (0.0 where there is no candidate) and `delta_exp` (int64), and `zero_sites`, the sites
    whose likelihood is 0 in this tree (left out of every product; lnl is -inf when there is one)."""

    def __init__(self, lnl, mant, exp, zero_sites):
        self.lnl, self.delta_mant, self.delta_exp, self.zero_sites = float(lnl), mant, exp, int(zero_sites)
        with np.errstate(divide="ignore"):
            self.delta = np.where(mant > 0.0, np.log(np.where(mant > 0.0, mant, 1.0)) + exp.astype(np.float64) * _LN2, np.nan)

    def edge_margin(self):
        """merges float64: -max of the two gains of the edge above every merge -- how much lnL the better of its two interchanges
        would lose (negative: the tree is not a local optimum there); NaN where the merge has no candidate"""
        return -np.max(self.delta, axis=1)


class LikelihoodSearch(MlLengths):
    """The result of `tree_model_nni` (ps_ml_nni_t + the arrays; docs/LIKELIHOOD_SEARCH.md): the summary fields as attributes (the
    count `moves` of ps_ml_nni_t as `n_moves`; `merges`, the number of merges, called gives the merge list), `lnl`, `start_lnl`,
    the returned tree `left`, `right` in canonical form with its `lengths`, `round_lnl` (rounds + 1 float64: lnL of the first pass,
    then after every round) and `moves`, a record array of (round, node, kind, gain) -- the interchanges applied, each numbered in
    the canonical tree its round started from.  `newick()` as MlLengths."""
    FIELDS = tuple(name for name, kind in MlNni._fields_ if kind is C.c_uint64 and name != "moves")
    REALS = tuple(name for name, kind in MlNni._fields_ if kind is C.c_double)
    MOVE = np.dtype([("round", np.uint32), ("node", np.uint32), ("kind", np.uint32), ("gain", np.float64)])

    def __init__(self, summary, model, left, right, lengths, round_lnl, moves):
        _Summary._take(self, summary)
        for name in self.REALS:
            setattr(self, name, float(getattr(summary, name)))
        self.local_optimum, self.n_moves = bool(self.local_optimum), int(summary.moves)
        self.model, self.left, self.right, self.lengths, self.round_lnl, self.moves = model, left, right, lengths, round_lnl, moves
        self.merges = _MergeCount(self.merges, left, right)

    def as_dict(self):
        out = self._head("n_moves", *self.REALS)
        out.update(left=self.left, right=self.right, lengths=self.lengths, round_lnl=self.round_lnl, moves=self.moves)
        return out


def _deltas_call(fn, left, right, lengths, model, pop_size, *head):
    """fn(*head, left, right, length, merges, &model, &lnl, delta_mant, delta_exp, &zero_sites) -> ModelNniDeltas"""
    left, right = _merge_list(left, right)
    M = left.size
    lengths = _lengths(lengths, int(pop_size) + M)
    lnl, zero = C.c_double(), C.c_uint64()
    mant, exp = np.zeros(max(1, 2 * M), np.float64), np.zeros(max(1, 2 * M), np.int64)
    cm, keep = model._c()
    check(fn(*head, _ptr(left), _ptr(right), _ptr(lengths), M, C.byref(cm), C.byref(lnl), _ptr(mant), _ptr(exp), C.byref(zero)))
    del keep
    return ModelNniDeltas(lnl.value, mant[:2 * M].reshape(-1, 2), exp[:2 * M].reshape(-1, 2), zero.value)


def _search_call(fn, left, right, lengths, model, pop_size, max_rounds, moves_per_round, length_rounds, eps_gain, *head):
    """fn(*head, left, right, length_in, merges, &model, &params, &summary, the two lists, length_out, round_lnl, the four move
    arrays, move_cap) -> LikelihoodSearch"""
    left, right = _merge_list(left, right)
    N, M, R = int(pop_size), left.size, max(0, int(max_rounds))
    lengths = _lengths(lengths, N + M)
    # a batch's moves touch at least five nodes each of the 2 N - 1
    per_round = min(int(moves_per_round), N) if int(moves_per_round) > 0 else (2 * N) // 5 + 1
    cap = max(1, min(R * per_round, 1 << 22))
    out_l, out_r = np.zeros(max(1, M), np.uint32), np.zeros(max(1, M), np.uint32)
    out_t, rl = np.zeros(N + M, np.float64), np.zeros(R + 1, np.float64)
    mr, mn, mk, mg = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.float64)
    prm, s = MlNniParams(R, max(0, int(moves_per_round)), max(0, int(length_rounds)), float(eps_gain)), MlNni()
    cm, keep = model._c()
    check(fn(*head, _ptr(left), _ptr(right), _ptr(lengths), M, C.byref(cm), C.byref(prm), C.byref(s), _ptr(out_l), _ptr(out_r), _ptr(out_t),
             _ptr(rl), _ptr(mr), _ptr(mn), _ptr(mk), _ptr(mg), cap))
    del keep
    n = min(int(s.moves), cap)
    moves = np.zeros(n, LikelihoodSearch.MOVE)
    moves["round"], moves["node"], moves["kind"], moves["gain"] = mr[:n], mn[:n], mk[:n], mg[:n]
    return LikelihoodSearch(s, model, out_l[:M], out_r[:M], out_t, rl[:int(s.rounds) + 1], moves)


def model_nni_deltas_from_rows(rows, left, right, lengths, model):
    """`Population.model_nni_deltas` of an individual-major (pop_size, cols) uint8 matrix on the host alone
    (ps_model_nni_deltas_from_rows; no device): the same site ratios, multiplied in ascending order -> a ModelNniDeltas"""
    rows = _rows(rows)
    return _deltas_call(_lib.load().ps_model_nni_deltas_from_rows, left, right, lengths, model, rows.shape[0], _ptr(rows), rows.shape[0],
                        rows.shape[1])


def model_nni_from_rows(rows, left, right, lengths, model, max_rounds=1000, moves_per_round=0, length_rounds=5, eps_gain=1e-3):
    """`Population.tree_model_nni` of an individual-major (pop_size, cols) uint8 matrix on the host alone
    (ps_model_nni_from_rows; no device) -> a LikelihoodSearch"""
    rows = _rows(rows)
    return _search_call(_lib.load().ps_model_nni_from_rows, left, right, lengths, model, rows.shape[0], max_rounds, moves_per_round,
                        length_rounds, eps_gain, _ptr(rows), rows.shape[0], rows.shape[1])


def merges_canonical_lengths(left, right, lengths, pop_size):
    """the canonical form (left, right, lengths) of a spanning merge list with the length of the branch above every node
    (ps_merges_canonical_lengths; host only): every length follows its node to the node's new id"""
    left, right = _merge_list(left, right)
    lengths = _lengths(lengths, int(pop_size) + left.size)
    out_l, out_r, out_t = np.zeros(max(1, left.size), np.uint32), np.zeros(max(1, left.size), np.uint32), np.zeros(lengths.size, np.float64)
    check(_lib.load().ps_merges_canonical_lengths(_ptr(left), _ptr(right), _ptr(lengths), left.size, int(pop_size), _ptr(out_l), _ptr(out_r),
                                                  _ptr(out_t)))
    return out_l[:left.size], out_r[:left.size], out_t


def nni_apply_lengths(left, right, lengths, pop_size, node, kind):
    """candidate (node, kind) of the merge list as given applied, the neighbour tree and its lengths in canonical form
    (ps_nni_apply_lengths; host only): every subtree keeps the length of the branch above it"""
    left, right = _merge_list(left, right)
    lengths = _lengths(lengths, int(pop_size) + left.size)
    out_l, out_r, out_t = np.zeros(max(1, left.size), np.uint32), np.zeros(max(1, left.size), np.uint32), np.zeros(lengths.size, np.float64)
    check(_lib.load().ps_nni_apply_lengths(_ptr(left), _ptr(right), _ptr(lengths), left.size, int(pop_size), int(node), int(kind), _ptr(out_l),
                                           _ptr(out_r), _ptr(out_t)))
    return out_l[:left.size], out_r[:left.size], out_t


__all__ = ["PS_MODEL_NNI_MAX_POP", "LikelihoodSearch", "ModelNniDeltas", "merges_canonical_lengths", "model_nni_deltas_from_rows",
           "model_nni_from_rows", "nni_apply_lengths"]
