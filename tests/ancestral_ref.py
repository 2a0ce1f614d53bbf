"""References for the marginal ancestral states of a tree under F81 with a root distribution and rate categories
(docs/ANCESTRAL_STATES.md), NumPy only -- nothing here calls the library:

(a) `joint`: the joint probability of one column and EVERY assignment of the internal nodes in one category, a tensor of 4^M
    entries built from explicit 4 x 4 matrices x I + (1 - x) 1 pi^T and the root drawn from rho; `site`: from it the marginal
    posterior of every internal node and, from the joint of the two ends of every branch, the posterior probability that they
    differ -- of the assigned class, or mixed over the categories by their posterior;
(b) `evolve`: data generated under the model down a tree, the internal nodes' true states returned with the leaves'.
The trees come from tree_likelihood_ref, the matrices from subst_model_ref.
"""
import numpy as np

from subst_model_ref import beta_of, matrix, x_table
from tree_likelihood_ref import BASES, clamp


# ------------------------------------------------------------------------------------------------------ (a) brute force
def joint(col, left, right, x, pi, rho):
    """P(column, internal nodes = (a_0 .. a_{M-1})) in one category: axis k is merge k, the root the last"""
    n, m = len(col), len(left)
    shape = [1] * m
    shape[m - 1] = 4
    total = np.ones((4,) * m) * np.asarray(rho, np.float64).reshape(shape)
    for k in range(m):
        for c in (int(left[k]), int(right[k])):
            P = matrix(float(x[c]), pi)
            shape = [1] * m
            shape[k] = 4
            if c < n:
                v = P[:, BASES.index(col[c])] if col[c] in BASES else P.sum(axis=1)
                total = total * v.reshape(shape)
            else:
                shape[c - n] = 4
                total = total * P.T.reshape(shape)          # (the parent's axis k is above the child's)
    return total


def _category(col, left, right, x, pi, rho):
    """(likelihood, (M, 4) node marginals times the likelihood, (N + M) differing mass of every branch) of one category"""
    n, m = len(col), len(left)
    J = joint(col, left, right, x, pi, rho)
    lik = float(J.sum())
    marg = np.stack([J.sum(axis=tuple(a for a in range(m) if a != k)) for k in range(m)])
    diff = np.zeros(n + m)
    for k in range(m):
        for c in (int(left[k]), int(right[k])):
            if c >= n:
                pair = J.sum(axis=tuple(a for a in range(m) if a not in (k, c - n)))       # [child, parent]: the child's axis is lower
                diff[c] = float(pair[~np.eye(4, dtype=bool)].sum())          # (the unlike pairs added up: no difference of sums)
            elif col[c] in BASES:
                diff[c] = float(np.delete(marg[k], BASES.index(col[c])).sum())
            else:
                # an unobserved leaf: its state is drawn along the branch from the parent's; the unlike entries of the parent's row
                # added up (1 - P[a, a] would cancel on a short branch)
                P = matrix(float(x[c]), pi)
                diff[c] = float((marg[k] * (P * ~np.eye(4, dtype=bool)).sum(axis=1)).sum())
    return lik, marg, diff


def site(col, left, right, t, pi, rho, rates, weights, cls=None):
    """one column -> dict(lik, post, node (M, 4), pdiff (N + M; the root's 0)): the likelihood (of class `cls`, or the mixture),
    the posterior of the categories, every internal node's marginal posterior and every branch's posterior probability of a
    difference between its ends.  lik = 0: node and pdiff are zeros."""
    beta = beta_of(pi)
    K, n, m = len(rates), len(col), len(left)
    xs = x_table(clamp(t), rates, beta)
    ks = range(K) if cls is None else [int(cls)]
    w = np.asarray(weights, np.float64) if cls is None else np.eye(K)[int(cls)]
    lk, marg, diff = np.zeros(K), np.zeros((K, m, 4)), np.zeros((K, n + m))
    for k in ks:
        lk[k], marg[k], diff[k] = _category(col, left, right, xs[k], pi, rho)
    lik = float((w * lk).sum())
    if lik == 0.0:
        return dict(lik=0.0, post=w, node=np.zeros((m, 4)), pdiff=np.zeros(n + m))
    # sum_k post_k (marg_k / l_k) = sum_k w_k marg_k / lik
    node = np.tensordot(w, marg, axes=1) / lik
    pdiff = (w @ diff) / lik
    return dict(lik=lik, post=w * lk / lik, node=node, pdiff=pdiff)


def reconstruct(rows, left, right, t, pi, rho, rates, weights, site_class=None):
    """every column of an individual-major matrix -> dict(node (L, M, 4), pdiff (L, N + M), lik (L,))"""
    sites = [site(rows[:, s], left, right, t, pi, rho, rates, weights, None if site_class is None else site_class[s]) for s in range(rows.shape[1])]
    return dict(node=np.stack([v["node"] for v in sites]), pdiff=np.stack([v["pdiff"] for v in sites]), lik=np.array([v["lik"] for v in sites]))


# ---------------------------------------------------------------------------------------------------------- (b) data
def evolve(left, right, lengths, n, sites, rng, pi, rho, site_rates):
    """((n, sites) uint8 leaves, (M, sites) uint8 internal nodes) evolved under the model down the tree: the root from rho; along
    a branch a site of rate r is hit with probability 1 - exp(-(r t) / beta) and then redrawn from pi, whatever it was"""
    m = len(left)
    beta = beta_of(pi)
    t = clamp(lengths)
    site_rates = np.broadcast_to(np.asarray(site_rates, np.float64), (sites,))
    pi, rho = np.asarray(pi, np.float64), np.asarray(rho, np.float64)
    state = [None] * (n + m)
    state[n + m - 1] = rng.choice(4, sites, p=rho)
    for k in range(m - 1, -1, -1):
        for c in (int(left[k]), int(right[k])):
            hit = rng.random(sites) >= np.exp(-(site_rates * t[c]) / beta)
            state[c] = np.where(hit, rng.choice(4, sites, p=pi), state[n + k])
    bases = np.array(BASES, np.uint8)
    return bases[np.stack(state[:n])], bases[np.stack(state[n:])]
