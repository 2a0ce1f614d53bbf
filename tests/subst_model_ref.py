"""References for the likelihood of a tree under F81 with a root distribution and rate categories (docs/TREE_MODEL.md), NumPy and
the standard library only -- nothing here calls the library:

(a) `brute`: a category's site likelihood as the sum over ALL 4^M assignments of the internal nodes with explicit 4 x 4 matrices
    x I + (1 - x) 1 pi^T and the root drawn from rho, and its derivatives with respect to a branch length from the matrices' own
    derivatives; `site`: the assigned or mixture likelihood, posterior, mean rate and the two derivatives of ln l per branch;
(b) `pruning`: pruning without any rescaling, and `pruning_exact` over exact rationals;
(c) `evolve`: data generated under the model with a rate per site;
(d) `gamma_p`: the regularised incomplete gamma function by numerical integration.
The trees come from tree_likelihood_ref.
"""
import math
from fractions import Fraction

import numpy as np

from tree_likelihood_ref import BASES, clamp

JC = (0.25, 0.25, 0.25, 0.25)
SIM = (0.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0)


def beta_of(pi):
    return 1.0 - float(np.sum(np.asarray(pi, np.float64) ** 2))


def x_of(t, rate, beta):
    """x = exp(-(r t) / beta) of used lengths, in the library's association and through the same libm"""
    return np.array([math.exp(-(float(rate) * float(v)) / beta) for v in np.asarray(t, np.float64).reshape(-1)])


def x_table(t, rates, beta):
    return np.stack([x_of(t, r, beta) for r in rates])


# ------------------------------------------------------------------------------------------------------ (a) brute force
def matrix(x, pi, order=0, scale=1.0):
    """P[parent, child] = x I + (1 - x) 1 pi^T of a branch, or its first or second derivative with respect to t, where
    dx/dt = -scale x (scale = r / beta)"""
    pi = np.asarray(pi, np.float64)
    away = np.eye(4) - np.outer(np.ones(4), pi)
    if order == 0:
        return x * np.eye(4) + (1.0 - x) * np.outer(np.ones(4), pi)
    return (-scale * x if order == 1 else scale * scale * x) * away


def brute(col, left, right, x, pi, rho, branch=None, order=0, x_branch=None, scale=1.0):
    """the likelihood of one column in one category: the sum over all 4^M assignments of the internal nodes of rho(root) times the
    product of P(child | parent) over the branches.  `branch`, `order`: that branch's matrix replaced by its derivative of that
    order; `x_branch`: that branch's x replaced (the likelihood is linear in it)."""
    n, m = len(col), len(left)
    shape = [1] * m
    shape[m - 1] = 4
    total = np.ones((4,) * m) * np.asarray(rho, np.float64).reshape(shape)
    for k in range(m):
        for c in (int(left[k]), int(right[k])):
            xc = x_branch if (c == branch and x_branch is not None) else float(x[c])
            P = matrix(xc, pi, order if (c == branch and x_branch is None) else 0, scale)
            shape = [1] * m
            shape[k] = 4
            if c < n:
                v = P[:, BASES.index(col[c])] if col[c] in BASES else P.sum(axis=1)
                total = total * v.reshape(shape)
            else:
                shape[c - n] = 4
                total = total * P.T.reshape(shape)          # (the parent's axis k is above the child's)
    return float(total.sum())


def site(col, left, right, t, pi, rho, rates, weights, cls=None, derivatives=False):
    """one column -> dict(lik, post, rate[, d1, d2, scale1, scale2]): the likelihood (of class `cls`, or the mixture), the
    posterior of the categories and its mean rate; with `derivatives` dlnl/dt and d2lnl/dt2 per branch (nodes - 1 values) and the
    scales of their error bounds: with s_k = (|A| + |A + B|) / l_k of category k (A, A + B: l_k at x_c = 0 and 1),
    scale1 = sum_k post_k (r_k / beta) s_k and scale2 = sum_k post_k (r_k / beta)^2 s_k + scale1^2."""
    beta = beta_of(pi)
    used = clamp(t)
    K, nodes = len(rates), len(col) + len(left)
    xs = x_table(used, rates, beta)
    ks = range(K) if cls is None else [int(cls)]
    w = np.asarray(weights, np.float64) if cls is None else np.eye(K)[int(cls)]
    lk = np.zeros(K)
    for k in ks:
        lk[k] = brute(col, left, right, xs[k], pi, rho)
    lik = float((w * lk).sum())
    post = w * lk / lik
    out = dict(lik=lik, post=post, rate=float((post * np.asarray(rates)).sum()), cat=lk)
    if not derivatives:
        return out
    d1, d2, s1, s2 = (np.zeros(nodes - 1) for _ in range(4))
    for c in range(nodes - 1):
        f1 = f2 = 0.0
        for k in ks:
            if post[k] == 0.0:
                continue
            sc = rates[k] / beta
            a1 = brute(col, left, right, xs[k], pi, rho, branch=c, order=1, scale=sc)
            a2 = brute(col, left, right, xs[k], pi, rho, branch=c, order=2, scale=sc)
            A = brute(col, left, right, xs[k], pi, rho, branch=c, x_branch=0.0)
            AB = brute(col, left, right, xs[k], pi, rho, branch=c, x_branch=1.0)
            f1 += w[k] * a1
            f2 += w[k] * a2
            s = (abs(A) + abs(AB)) / lk[k]
            s1[c] += post[k] * sc * s
            s2[c] += post[k] * sc * sc * s
        d1[c] = f1 / lik
        d2[c] = f2 / lik - (f1 / lik) ** 2
        s2[c] += s1[c] ** 2
    out.update(d1=d1, d2=d2, scale1=s1, scale2=s2)
    return out


# ------------------------------------------------------------------------------------------------- (b) pruning, unscaled
def leaf_partials(rows):
    rows = np.asarray(rows, np.uint8)
    out = np.stack([(rows == b) for b in BASES], axis=-1).astype(np.float64)
    out[~np.isin(rows, BASES)] = 1.0
    return out


def pruning(rows, left, right, x, pi, rho):
    """the site likelihoods (sites float64) of one category by pruning without rescaling, all sites at once"""
    n, m = rows.shape[0], len(left)
    pi, rho = np.asarray(pi, np.float64), np.asarray(rho, np.float64)
    L = [None] * (n + m)
    L[:n] = list(leaf_partials(rows))

    def message(xc, P):
        return (1.0 - xc) * (P * pi).sum(axis=-1, keepdims=True) + xc * P

    for k in range(m):
        L[n + k] = message(x[left[k]], L[left[k]]) * message(x[right[k]], L[right[k]])
    return (L[-1] * rho).sum(axis=-1)


def pruning_exact(col, left, right, x, pi, rho):
    """the likelihood of one column in one category as an exact rational of the binary64 values x, pi and rho"""
    n, m = len(col), len(left)
    pi, rho = [Fraction(float(v)) for v in pi], [Fraction(float(v)) for v in rho]
    L = [[Fraction(1 if (b not in BASES or b == s) else 0) for s in BASES] for b in col] + [None] * m

    def message(xc, P):
        xc = Fraction(float(xc))
        s = (1 - xc) * sum(p * v for p, v in zip(pi, P))
        return [s + xc * v for v in P]

    for k in range(m):
        a, b = message(x[left[k]], L[left[k]]), message(x[right[k]], L[right[k]])
        L[n + k] = [u * v for u, v in zip(a, b)]
    return sum(r * v for r, v in zip(rho, L[-1]))


# ---------------------------------------------------------------------------------------------------------- (c) data
def evolve(left, right, lengths, n, sites, rng, pi, rho, site_rates):
    """(n, sites) uint8 bases evolved under the model down the tree: the root from rho; along a branch a site of rate r is hit
    with probability 1 - exp(-(r t) / beta) and then redrawn from pi, whatever it was"""
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
    return np.array(BASES, np.uint8)[np.stack(state[:n])]


# ----------------------------------------------------------------------------------------- (d) incomplete gamma function
_GL = np.polynomial.legendre.leggauss(48)


def _integrate(f, lo, hi, panels):
    edges = np.linspace(lo, hi, panels + 1)
    half, mid = 0.5 * np.diff(edges)[:, None], 0.5 * (edges[1:] + edges[:-1])[:, None]
    return float((f(mid + half * _GL[0][None, :]) * _GL[1][None, :] * half).sum())


def gamma_p(a, x):
    """P(a, x) = int_0^x t^(a-1) e^-t dt / Gamma(a) by Gauss-Legendre panels.  For a < 1 the integrand is singular at 0: with
    t = u^(1/a) the integral is (1 / a) int_0^(x^a) exp(-u^(1/a)) du, whose integrand is smooth."""
    if x <= 0.0:
        return 0.0
    if a < 1.0:
        val = _integrate(lambda u: np.exp(-u ** (1.0 / a)), 0.0, x ** a, 400) / a
    else:
        val = _integrate(lambda t: t ** (a - 1.0) * np.exp(-t), 0.0, x, 400)
    return val / math.gamma(a)
