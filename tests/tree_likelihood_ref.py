"""References for the Jukes-Cantor likelihood of a tree (docs/TREE_LIKELIHOOD.md), NumPy and the standard library only -- nothing
here calls the library:

(a) `brute`: the site likelihood as the sum over ALL assignments of the internal nodes, and its derivatives with respect to a
    branch from the same sum with the derivative of that branch's transition probabilities;
(b) `pruning`: Felsenstein's pruning without any rescaling, all sites at once, and `pruning_exact`, the same over exact
    rationals (a binary64 number is a dyadic rational), which no number of leaves can underflow;
(c) `ml_lengths`: the branch-length optimiser as the document specifies it, over an unscaled up and down pass;
(d) `evolve`: data generated under Jukes-Cantor on a tree with given lengths;
and the trees the tests walk.
"""
import math
from fractions import Fraction

import numpy as np

MIN_LENGTH, MAX_LENGTH = 1e-8, 10.0
BASES = (1, 2, 4, 8)


def clamp(t):
    return np.minimum(np.maximum(np.asarray(t, np.float64), MIN_LENGTH), MAX_LENGTH)


def x_of(t):
    """x = exp(-4 t / 3) of used lengths, in the library's association and through the same libm"""
    return np.array([math.exp((-4.0 * float(v)) / 3.0) for v in np.asarray(t, np.float64).reshape(-1)])


# ---------------------------------------------------------------------------------------------------------------- trees
def shapes(n):
    """every rooted binary tree shape of n leaves as nested tuples (a leaf is None), one per unlabelled topology"""
    if n == 1:
        return [None]
    out = []
    for a in range(1, n // 2 + 1):
        for l in shapes(a):
            for r in shapes(n - a):
                if a * 2 == n and repr(l) > repr(r):
                    continue
                out.append((l, r))
    return out


def merges_of_shape(shape, leaves):
    """the merge list of a nested shape, its leaves numbered in the order of `leaves` from left to right"""
    leaves, left, right, n = list(leaves), [], [], len(leaves)
    it = iter(leaves)

    def walk(s):
        if s is None:
            return next(it)
        a, b = walk(s[0]), walk(s[1])
        left.append(a)
        right.append(b)
        return n + len(left) - 1

    walk(shape)
    return np.array(left, np.uint32), np.array(right, np.uint32)


def caterpillar(n, leaves=None):
    leaves = list(range(n)) if leaves is None else list(leaves)
    left = [leaves[0]] + [n + k for k in range(n - 2)]
    return np.array(left, np.uint32), np.array(leaves[1:], np.uint32)


def balanced(n):
    nodes, left, right = list(range(n)), [], []
    while len(nodes) > 1:
        nxt = []
        for i in range(0, len(nodes) - 1, 2):
            left.append(nodes[i])
            right.append(nodes[i + 1])
            nxt.append(n + len(left) - 1)
        if len(nodes) % 2:
            nxt.append(nodes[-1])
        nodes = nxt
    return np.array(left, np.uint32), np.array(right, np.uint32)


def random_tree(n, rng):
    nodes, left, right = list(range(n)), [], []
    while len(nodes) > 1:
        i, j = rng.choice(len(nodes), 2, replace=False)
        a, b = nodes[i], nodes[j]
        nodes = [v for k, v in enumerate(nodes) if k not in (i, j)] + [n + len(left)]
        left.append(a)
        right.append(b)
    return np.array(left, np.uint32), np.array(right, np.uint32)


# ------------------------------------------------------------------------------------------------------ (a) brute force
def _factor(x, order):
    """the 4 x 4 matrix of P(child | parent) of a branch with x, or of its first or second derivative with respect to t"""
    same, diff = ((1.0 + 3.0 * x) / 4.0, (1.0 - x) / 4.0) if order == 0 else (-x, x / 3.0) if order == 1 else (4.0 * x / 3.0, -4.0 * x / 9.0)
    return np.full((4, 4), diff) + np.eye(4) * (same - diff)


def brute(col, left, right, x, branch=None, order=0, x_branch=None):
    """the likelihood of one column: a quarter of the sum over all 4^M assignments of the internal nodes of the product of
    P(child | parent) over the branches.  `branch`, `order`: that branch's factor replaced by its derivative of that order;
    `x_branch`: that branch's x replaced (the likelihood is linear in it)."""
    n, m = len(col), len(left)
    total = np.ones((4,) * m)
    for k in range(m):
        for c in (int(left[k]), int(right[k])):
            xc = x_branch if (c == branch and x_branch is not None) else float(x[c])
            P = _factor(xc, order if (c == branch and x_branch is None) else 0)
            shape = [1] * m
            shape[k] = 4
            if c < n:
                v = P[:, BASES.index(col[c])] if col[c] in BASES else P.sum(axis=1)
                total = total * v.reshape(shape)
            else:
                shape[c - n] = 4
                # axis of the parent k is above the child's (k > c - n): P[parent, child] transposed into the axes' order
                total = total * P.T.reshape(shape)
    return 0.25 * float(total.sum())


# ------------------------------------------------------------------------------------------------- (b) pruning, unscaled
def leaf_partials(rows):
    """(pop, sites, 4): the indicator of the base, ones for any other byte"""
    rows = np.asarray(rows, np.uint8)
    out = np.stack([(rows == b) for b in BASES], axis=-1).astype(np.float64)
    out[~np.isin(rows, BASES)] = 1.0
    return out


def _message(x, L):
    return ((1.0 - x) / 4.0) * L.sum(axis=-1, keepdims=True) + x * L


def pruning(rows, left, right, x, derivatives=False):
    """the site likelihoods (sites float64) of an individual-major matrix by pruning without rescaling; with `derivatives` also
    B / likelihood per site and node, (sites, nodes), from the outside partials of an unscaled down pass"""
    n, m = rows.shape[0], len(left)
    L = [None] * (n + m)
    L[:n] = list(leaf_partials(rows))
    for k in range(m):
        L[n + k] = _message(x[left[k]], L[left[k]]) * _message(x[right[k]], L[right[k]])
    lik = 0.25 * L[-1].sum(axis=-1)
    if not derivatives:
        return lik
    U, r = [None] * (n + m), np.zeros((rows.shape[1], n + m))
    for k in range(m - 1, -1, -1):
        a, b, c = int(left[k]), int(right[k]), n + k
        T = np.ones_like(L[c]) if k == m - 1 else _message(x[c], U[c])
        U[a], U[b] = _message(x[b], L[b]) * T, _message(x[a], L[a]) * T
        for v in (a, b):
            A = L[v].sum(axis=-1) * U[v].sum(axis=-1) / 16.0
            D = (U[v] * L[v]).sum(axis=-1) / 4.0
            r[:, v] = (D - A) / ((1.0 - x[v]) * A + x[v] * D)       # (= B / (A + x B), the denominator without a difference)
    return lik, r


def pruning_exact(col, left, right, x):
    """the likelihood of one column as an exact rational of the binary64 values x.  A partial is four integers over one power of
    two (every binary64 number is an integer over a power of two), so nothing is ever reduced until the end."""
    n, m = len(col), len(left)
    L = [([1 if (b not in BASES or b == s) else 0 for s in BASES], 0) for b in col] + [None] * m

    def message(xc, P):
        nx, den = float(xc).as_integer_ratio()
        dx = den.bit_length() - 1                        # (den = 2^dx)
        p, d = P
        qs = (den - nx) * sum(p)
        return [qs + 4 * nx * v for v in p], d + dx + 2

    for k in range(m):
        (a, da), (b, db) = message(x[left[k]], L[left[k]]), message(x[right[k]], L[right[k]])
        L[n + k] = ([u * v for u, v in zip(a, b)], da + db)
    return Fraction(sum(L[-1][0]), 4 << L[-1][1])


# ------------------------------------------------------------------------------------------------------- (c) optimiser
def newton(t, x, g, h, lam):
    gt = -(4.0 * x / 3.0) * g
    ht = (16.0 * x * x / 9.0) * (-h) + (16.0 * x / 9.0) * g
    d = -gt / ht if ht < 0.0 else (t if gt > 0.0 else -t if gt < 0.0 else 0.0)
    d = min(max(d, -0.5 * t), max(t, 1e-3))
    return float(clamp(t + lam * d))


def ml_lengths(rows, left, right, lengths, max_rounds=50, eps_lnl=1e-3):
    """the optimiser loop of the document -> dict(lengths, round_lnl, rounds, passes, rollbacks, converged, lnl, start_lnl)"""
    n, m = rows.shape[0], len(left)
    root, rl, rr = n + m - 1, int(left[-1]), int(right[-1])
    t = clamp(lengths).copy()
    t[root] = 0.0
    t[rl] = float(clamp(t[rl] + t[rr]))
    t[rr] = MIN_LENGTH

    def run(t):
        x = x_of(t)
        lik, r = pruning(rows, left, right, x, derivatives=True)
        return float(np.log(lik).sum()), r.sum(axis=0), (r * r).sum(axis=0), x

    lnl, g, h, x = run(t)
    out = dict(start_lnl=lnl, round_lnl=[lnl], rounds=0, passes=1, rollbacks=0, converged=False)
    lam = 1.0
    while out["rounds"] < max_rounds and lam >= 2.0 ** -20:
        cand = t.copy()
        for c in range(root):
            if c != rr:
                cand[c] = newton(t[c], x[c], g[c], h[c], lam)
        lnl2, g2, h2, x2 = run(cand)
        out["passes"] += 1
        if lnl2 < lnl:
            out["rollbacks"] += 1
            lam *= 0.5
            continue
        if lnl2 == lnl:
            out["converged"] = True
            break
        gain = lnl2 - lnl
        out["rounds"] += 1
        t, lnl, g, h, x, lam = cand, lnl2, g2, h2, x2, 1.0
        out["round_lnl"].append(lnl)
        if gain < eps_lnl:
            out["converged"] = True
            break
    out.update(lengths=t, lnl=lnl, round_lnl=np.array(out["round_lnl"]))
    return out


# ------------------------------------------------------------------------------------------------------- (d) JC69 data
def evolve(left, right, lengths, n, sites, rng):
    """(n, sites) uint8 bases evolved under Jukes-Cantor down the tree: the root uniform, along a branch a site is redrawn
    uniformly from the four bases with probability 1 - x (so it stays with (1 + 3 x) / 4)"""
    m = len(left)
    x = x_of(clamp(lengths))
    state = [None] * (n + m)
    state[n + m - 1] = rng.integers(0, 4, sites)
    for k in range(m - 1, -1, -1):
        for c in (int(left[k]), int(right[k])):
            redraw = rng.random(sites) >= x[c]
            state[c] = np.where(redraw, rng.integers(0, 4, sites), state[n + k])
    return np.array(BASES, np.uint8)[np.stack(state[:n])]
