"""Parsimony tree search over the C ABI (docs/PARSIMONY_SEARCH.md): the result of `tree_nni()`, the canonical form of a merge
list, one interchange applied, and the host restatements of a pass and of the search.

All computation happens in the HIP library; this module only marshals buffers.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import PS_NNI_MAX_POP, PS_NNI_NONE, Nni, NniParams, check
from .parsimony import _merge_list
from .population import _MergeCount, _ptr, _Summary


class ParsimonySearch(_Summary):
    """The result of `tree_nni` (ps_nni_t + the arrays; docs/PARSIMONY_SEARCH.md): the integer summary fields as attributes (the
    count `moves` of ps_nni_t as `n_moves`; `merges`, the number of merges, called gives the merge list as `UpgmaTree.merges`
    does), the returned tree `left`, `right` in canonical form, `round_changes` (rounds + 1 uint64: the total changes of the
    start tree, then after every round) and `moves`, a record array of (round, node, kind, delta) -- the interchanges applied,
    each numbered in the canonical tree its round started from."""
    FIELDS = tuple(name for name, _ in Nni._fields_ if name != "moves")
    MOVE = np.dtype([("round", np.uint32), ("node", np.uint32), ("kind", np.uint32), ("delta", np.int64)])

    def __init__(self, summary, left, right, round_changes, moves):
        self._take(summary)
        self.local_optimum, self.n_moves = bool(self.local_optimum), int(summary.moves)
        self.left, self.right, self.round_changes, self.moves = left, right, round_changes, moves
        self.merges = _MergeCount(self.merges, left, right)

    def as_dict(self):
        out = self._head("n_moves")
        out.update(left=self.left, right=self.right, round_changes=self.round_changes, moves=self.moves)
        return out


def _nni_call(fn, left, right, pop_size, max_rounds, moves_per_round, *head):
    """fn(*head, left, right, merges, &params, &summary, the two lists, round_changes, the four move arrays, move_cap) ->
    ParsimonySearch"""
    left, right = _merge_list(left, right)
    N, M, R = int(pop_size), left.size, max(0, int(max_rounds))
    # a batch's moves touch at least five nodes each of the 2 N - 1
    per_round = min(int(moves_per_round), N) if int(moves_per_round) > 0 else (2 * N) // 5 + 1
    cap = max(1, min(R * per_round, 1 << 22))
    out_l, out_r = np.zeros(max(1, M), np.uint32), np.zeros(max(1, M), np.uint32)
    rc = np.zeros(R + 1, np.uint64)
    mr, mn, mk, md = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.int64)
    prm, s = NniParams(R, max(0, int(moves_per_round))), Nni()
    check(fn(*head, _ptr(left), _ptr(right), M, C.byref(prm), C.byref(s), _ptr(out_l), _ptr(out_r), _ptr(rc), _ptr(mr), _ptr(mn), _ptr(mk),
             _ptr(md), cap))
    n = min(int(s.moves), cap)
    moves = np.zeros(n, ParsimonySearch.MOVE)
    moves["round"], moves["node"], moves["kind"], moves["delta"] = mr[:n], mn[:n], mk[:n], md[:n]
    return ParsimonySearch(s, out_l[:M], out_r[:M], rc[:int(s.rounds) + 1], moves)


def _deltas_call(fn, left, right, *head):
    """fn(*head, left, right, merges, &total, delta) -> (total, delta as (merges, 2) int64)"""
    left, right = _merge_list(left, right)
    total, delta = C.c_uint64(), np.zeros(max(1, 2 * left.size), np.int64)
    check(fn(*head, _ptr(left), _ptr(right), left.size, C.byref(total), _ptr(delta)))
    return total.value, delta[:2 * left.size].reshape(-1, 2)


def _rows(rows):
    rows = np.ascontiguousarray(rows, np.uint8)
    if rows.ndim != 2:
        raise ValueError("rows must be (pop_size, cols)")
    return rows


def nni_deltas_from_rows(rows, left, right):
    """`Population.nni_deltas` of an individual-major (pop_size, cols) uint8 matrix on the host alone (ps_nni_deltas_from_rows;
    no device) -> (total_changes, delta): delta[k, kind] of merge k, PS_NNI_NONE where there is no candidate"""
    rows = _rows(rows)
    return _deltas_call(_lib.load().ps_nni_deltas_from_rows, left, right, _ptr(rows), rows.shape[0], rows.shape[1])


def nni_from_rows(rows, left, right, max_rounds=1000, moves_per_round=0):
    """`Population.tree_nni` of an individual-major (pop_size, cols) uint8 matrix on the host alone (ps_nni_from_rows; no
    device) -> a ParsimonySearch"""
    rows = _rows(rows)
    return _nni_call(_lib.load().ps_nni_from_rows, left, right, rows.shape[0], max_rounds, moves_per_round, _ptr(rows), rows.shape[0],
                     rows.shape[1])


def merges_canonical(left, right, pop_size):
    """the canonical form (left, right) of a spanning merge list (ps_merges_canonical; host only): internal nodes in (level,
    smallest leaf) order, left the child with the smaller smallest leaf -- one list per rooted topology"""
    left, right = _merge_list(left, right)
    out_l, out_r = np.zeros(max(1, left.size), np.uint32), np.zeros(max(1, left.size), np.uint32)
    check(_lib.load().ps_merges_canonical(_ptr(left), _ptr(right), left.size, int(pop_size), _ptr(out_l), _ptr(out_r)))
    return out_l[:left.size], out_r[:left.size]


def nni_apply(left, right, pop_size, node, kind):
    """candidate (node, kind) of the merge list as given applied, the neighbour tree in canonical form (ps_nni_apply; host only)"""
    left, right = _merge_list(left, right)
    out_l, out_r = np.zeros(max(1, left.size), np.uint32), np.zeros(max(1, left.size), np.uint32)
    check(_lib.load().ps_nni_apply(_ptr(left), _ptr(right), left.size, int(pop_size), int(node), int(kind), _ptr(out_l), _ptr(out_r)))
    return out_l[:left.size], out_r[:left.size]


__all__ = ["PS_NNI_MAX_POP", "PS_NNI_NONE", "ParsimonySearch", "merges_canonical", "nni_apply", "nni_deltas_from_rows", "nni_from_rows"]
