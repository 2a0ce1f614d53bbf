"""References for the likelihood tree search (docs/LIKELIHOOD_SEARCH.md), NumPy on top of subst_model_ref -- nothing here calls the
library unless a test hands it in:

(a) the tree rules in plain Python: the candidate table, one interchange with the lengths carried by their nodes, the canonical
    form with lengths, clade -> length maps and the Robinson-Foulds distance of two rooted trees;
(b) `site_lnl` / `lnl`: the log-likelihood of a tree under a model by pruning without rescaling (subst_model_ref.pruning), and
    `gains`: every candidate RESCORED FROM SCRATCH -- the move applied, the whole tree pruned again -- which never forms the four
    pieces around an edge;
(c) `search`: the loop of the document over (b); the length rounds are a callable the test hands in (None: none).
A model here is a dict(pi, rho, rates, weights, cls): cls None = every site a mixture.
"""
import numpy as np

import subst_model_ref as sm
from tree_likelihood_ref import clamp


def model_of(pi, rho=None, rates=(1.0,), weights=None, cls=None):
    rates = np.asarray(rates, np.float64)
    return dict(pi=np.asarray(pi, np.float64), rho=np.asarray(pi if rho is None else rho, np.float64), rates=rates,
                weights=np.full(rates.size, 1.0 / rates.size) if weights is None else np.asarray(weights, np.float64),
                cls=None if cls is None else np.asarray(cls))


# ------------------------------------------------------------------------------------------------------ (a) tree rules
def parents(left, right, n):
    par = {}
    for k in range(len(left)):
        par[int(left[k])] = par[int(right[k])] = n + k
    return par


def candidates(left, right, n):
    """[(node, kind)] in (node, kind) order: every internal node below an inner node; below the root its left child beside an
    internal right child"""
    m, par = len(left), parents(left, right, n)
    root, out = n + m - 1, []
    for k in range(m - 1):
        c = n + k
        if par[c] != root or (int(left[m - 1]) == c and int(right[m - 1]) >= n):
            out += [(c, 0), (c, 1)]
    return out


def apply_move(left, right, n, node, kind):
    """the merge list with candidate (node, kind) applied, every node keeping its id (not canonical: a parent may be below its
    child).  Below an inner node kind 0 swaps b with s, kind 1 swaps a with s; on the root's edge kind 0 swaps b with p, kind 1 b with q."""
    left, right = [int(v) for v in left], [int(v) for v in right]
    m, par = len(left), parents(left, right, n)
    v, c = par[node], node - n
    if v != n + m - 1:
        side = left if left[v - n] != node else right          # where the sibling hangs on v
        mine = right if kind == 0 else left
        mine[c], side[v - n] = side[v - n], mine[c]
    else:
        s = right[v - n] - n
        other = left if kind == 0 else right
        right[c], other[s] = other[s], right[c]
    return left, right


def canonical(left, right, lengths, n):
    """(left, right, lengths) in canonical form: internal nodes in (level, smallest leaf) order, left the child with the smaller
    smallest leaf, every length with its node.  The input may list a parent before its child."""
    m = len(left)
    par = parents(left, right, n)
    root = next(x for x in range(n, n + m) if x not in par)
    level, low = {i: 0 for i in range(n)}, {i: i for i in range(n)}

    def walk(x):
        if x in level:
            return
        l, r = int(left[x - n]), int(right[x - n])
        walk(l)
        walk(r)
        level[x], low[x] = 1 + max(level[l], level[r]), min(low[l], low[r])

    walk(root)
    order = sorted(range(n, n + m), key=lambda x: (level[x], low[x]))
    new = {i: i for i in range(n)}
    new.update({x: n + k for k, x in enumerate(order)})
    out_l, out_r, out_t = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(n + m)
    for k, x in enumerate(order):
        l, r = int(left[x - n]), int(right[x - n])
        if low[r] < low[l]:
            l, r = r, l
        out_l[k], out_r[k] = new[l], new[r]
    for x in range(n + m):
        out_t[new[x]] = lengths[x]
    return out_l, out_r, out_t


def clades(left, right, n):
    """the leaf set of every node, by node id (children first in the list)"""
    sets = {i: frozenset([i]) for i in range(n)}
    for k in range(len(left)):
        sets[n + k] = sets[int(left[k])] | sets[int(right[k])]
    return sets


def clade_lengths(left, right, lengths, n):
    """{clade: length of the branch above it}, the root's clade left out"""
    sets = clades(left, right, n)
    return {sets[x]: float(lengths[x]) for x in range(n + len(left) - 1)}


def rf_distance(a, b, n):
    """the Robinson-Foulds distance of two rooted trees: the clades of one that the other lacks, both ways"""
    ca, cb = (set(clades(l, r, n).values()) for l, r in (a, b))
    return len(ca ^ cb)


# ---------------------------------------------------------------------------------------------------- (b) likelihoods
def site_lik(rows, left, right, t, model):
    """sites float64: the likelihood of every site, pruned without rescaling"""
    pi, rho, rates, beta = model["pi"], model["rho"], model["rates"], sm.beta_of(model["pi"])
    used = clamp(t)
    cat = np.stack([sm.pruning(rows, left, right, sm.x_of(used, r, beta), pi, rho) for r in rates])
    if model["cls"] is not None:
        return cat[model["cls"], np.arange(rows.shape[1])]
    return (model["weights"][:, None] * cat).sum(axis=0)


def site_lnl(rows, left, right, t, model):
    with np.errstate(divide="ignore"):
        return np.log(site_lik(rows, left, right, t, model))


def lnl(rows, left, right, t, model):
    return float(site_lnl(rows, left, right, t, model).sum())


def neighbour(left, right, t, n, node, kind):
    l, r = apply_move(left, right, n, node, kind)
    return canonical(l, r, t, n)


def gains(rows, left, right, t, model):
    """{(node, kind): lnL of the neighbour tree - lnL of this tree}, each neighbour rescored from scratch; sites whose likelihood
    is 0 in this tree are left out of both"""
    n = rows.shape[0]
    base = site_lnl(rows, left, right, t, model)
    keep = np.isfinite(base)
    out = {}
    for node, kind in candidates(left, right, n):
        l, r, tt = neighbour(left, right, t, n, node, kind)
        out[(node, kind)] = float((site_lnl(rows, l, r, tt, model)[keep] - base[keep]).sum())
    return out


# ------------------------------------------------------------------------------------------------------------ (c) loop
def touched(left, right, n, node):
    m, par = len(left), parents(left, right, n)
    v, c = par[node], node - n
    sib = int(left[v - n]) if int(left[v - n]) != node else int(right[v - n])
    if v != n + m - 1:
        return {v, node, int(left[c]), int(right[c]), sib}
    return {v, node, sib, int(left[c]), int(right[c]), int(left[sib - n]), int(right[sib - n])}


def search(rows, left, right, t, model, max_rounds=1000, moves_per_round=0, eps_gain=1e-3, optimise=None):
    """the loop of the document -> dict(left, right, lengths, round_lnl, moves [(round, node, kind)], rollbacks, local_optimum).
    optimise(left, right, lengths) -> lengths: the length rounds before every pass (None: none)."""
    n = rows.shape[0]
    tune = (lambda l, r, tt: tt) if optimise is None else optimise
    used = clamp(t)
    used[-1] = 0.0
    left, right, t = canonical(left, right, used, n)
    t = tune(left, right, t)
    cur = lnl(rows, left, right, t, model)
    round_lnl, moves, rollbacks, optimum = [cur], [], 0, False
    while True:
        g = gains(rows, left, right, t, model)
        ranked = sorted((k for k in g if g[k] > eps_gain), key=lambda k: (-g[k], k[0], k[1]))
        batch, marked = [], set()
        for node, kind in ranked:
            if moves_per_round and len(batch) >= moves_per_round:
                break
            tch = touched(left, right, n, node)
            if tch & marked:
                continue
            marked |= tch
            batch.append((node, kind))
        if not batch:
            optimum = True
            break
        if len(round_lnl) - 1 == max_rounds:
            break
        while True:
            l, r = left, right
            for node, kind in batch:
                l, r = apply_move(l, r, n, node, kind)
            nl, nr, nt = canonical(l, r, t, n)
            nt = tune(nl, nr, nt)
            new = lnl(rows, nl, nr, nt, model)
            if len(batch) == 1 or new >= cur + g[batch[0]]:
                break
            rollbacks += 1
            batch = batch[:1]
        if not new > cur:
            break
        moves += [(len(round_lnl), node, kind) for node, kind in batch]
        left, right, t, cur = nl, nr, nt, new
        round_lnl.append(cur)
    return dict(left=left, right=right, lengths=t, round_lnl=np.array(round_lnl), moves=moves, rollbacks=rollbacks, local_optimum=optimum)
