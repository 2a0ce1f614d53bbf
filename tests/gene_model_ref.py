"""The reference of the gene gain / loss model (docs/GENE_MODEL.md): NumPy only, none of the library's code and none of its
parametrisation.  Every branch carries an explicit 2 x 2 transition matrix P = expm(Q t) of the generator

    Q = [[-gain, gain], [loss, -loss]]

taken from Q's eigen-decomposition (eigenvalues 0 and -(gain + loss), right eigenvectors (1, 1) and (gain, -loss), left eigenvectors
pi = (loss, gain) / (gain + loss) and (1, -1)), so that P = 1 pi^T + e^{-(gain + loss) t} (I - 1 pi^T).  The second eigenvalue's term
is written so that no entry is a difference: off the diagonal P_ij = (1 - e^{-(gain + loss) t}) pi_j with the factor taken through
expm1, on it P_ii = pi_i + e^{-(gain + loss) t} pi_j, which keeps every entry's relative precision on the shortest branches.

`brute` sums over all 2^M assignments of the inner nodes (small trees: the yardstick); `pruning` is Felsenstein's recursion with
explicit matrices, vectorised over genes (large trees; the tests hold it to `brute` on the small ones).  Both return per class the
gene likelihoods, the inner nodes' P(present) and every branch's directed joints P(absent above, present below) and the reverse;
`combine` turns the classes into the assigned or the mixture answer.  `evolve` draws data with the inner nodes' true states.
"""
import itertools

import numpy as np


def transition(gain, loss, t):
    """P(t) = expm(Q t), rows = the state above the branch, columns = the state below"""
    s = gain + loss
    if s == 0.0:
        return np.eye(2)
    pi = np.array([loss / s, gain / s])
    x, y = np.exp(-s * t), -np.expm1(-s * t)
    # off the diagonal y pi_j; on it pi_i + x pi_j: no entry is a difference
    return np.array([[pi[0] + x * pi[1], y * pi[1]], [y * pi[0], pi[1] + x * pi[0]]])


def tree_shapes(n):
    """every unlabelled rooted binary tree shape of n leaves as (left, right) merge lists over leaves 0 .. n - 1"""
    def shapes(k):
        if k == 1:
            return ["L"]
        out = []
        for a in range(1, k // 2 + 1):
            for sa in shapes(a):
                for sb in shapes(k - a):
                    if a == k - a and repr(sa) > repr(sb):
                        continue
                    out.append((sa, sb))
        return out

    lists = []
    for sh in shapes(n):
        left, right, leaf = [], [], [0]

        def walk(node):
            if node == "L":
                leaf[0] += 1
                return leaf[0] - 1
            a, b = walk(node[0]), walk(node[1])
            left.append(a)
            right.append(b)
            return n + len(left) - 1

        walk(sh)
        lists.append((np.array(left, np.uint32), np.array(right, np.uint32)))
    return lists


def random_tree(rng, n):
    """a random merge list: two random roots of the forest join until one is left"""
    roots, left, right = list(range(n)), [], []
    while len(roots) > 1:
        i, j = rng.choice(len(roots), 2, replace=False)
        a, b = roots[i], roots[j]
        left.append(a)
        right.append(b)
        roots = [r for r in roots if r not in (a, b)] + [n + len(left) - 1]
    return np.array(left, np.uint32), np.array(right, np.uint32)


def _parents(left, right, n):
    par = np.full(n + len(left), -1)
    for k, (a, b) in enumerate(zip(left, right)):
        par[a] = par[b] = n + k
    return par


def brute(rows, left, right, lengths, gain, loss, rho):
    """one class by the sum over all 2^M inner assignments -> (lik[G], p1[M, G], gains[N + M, G], losses[N + M, G])"""
    rows = np.asarray(rows) != 0
    n, G = rows.shape
    M = len(left)
    par = _parents(left, right, n)
    P = [transition(gain, loss, lengths[c]) for c in range(n + M - 1)]
    assign = np.array(list(itertools.product((0, 1), repeat=M)))            # (2^M, M)
    lik, p1 = np.zeros(G), np.zeros((M, G))
    gains, losses = np.zeros((n + M, G)), np.zeros((n + M, G))
    for g in range(G):
        state = np.concatenate([np.tile(rows[:, g].astype(int), (len(assign), 1)), assign], axis=1)
        w = np.asarray(rho)[state[:, n + M - 1]].astype(float)
        for c in range(n + M - 1):
            w = w * P[c][state[:, par[c]], state[:, c]]
        lik[g] = w.sum()
        if lik[g] == 0.0:
            continue
        p1[:, g] = (w[:, None] * assign).sum(0) / lik[g]
        for c in range(n + M - 1):
            gains[c, g] = w[(state[:, par[c]] == 0) & (state[:, c] == 1)].sum() / lik[g]
            losses[c, g] = w[(state[:, par[c]] == 1) & (state[:, c] == 0)].sum() / lik[g]
    return lik, p1, gains, losses


def pruning(rows, left, right, lengths, gain, loss, rho):
    """one class by Felsenstein's recursion with explicit matrices, every vector normalised (the scales kept as logs) ->
    (lnlik[G], p1[M, G], gains[N + M, G], losses[N + M, G])"""
    rows = np.asarray(rows) != 0
    n, G = rows.shape
    M = len(left)
    nodes = n + M
    P = [transition(gain, loss, lengths[c]) for c in range(nodes - 1)] + [np.eye(2)]
    L = np.zeros((nodes, 2, G))
    L[:n, 1] = rows
    L[:n, 0] = ~rows
    logs = np.zeros(G)
    msg = np.zeros((nodes, 2, G))
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(M):
            a, b, v = left[k], right[k], n + k
            msg[a], msg[b] = P[a] @ L[a], P[b] @ L[b]
            L[v] = msg[a] * msg[b]
            s = L[v].sum(0)
            L[v] = np.where(s > 0, L[v] / s, 0.0)
            logs += np.log(s)
        root = np.asarray(rho)[:, None] * L[nodes - 1]
        lnlik = logs + np.log(root.sum(0))
        p1 = np.zeros((M, G))
        gains, losses = np.zeros((nodes, G)), np.zeros((nodes, G))
        T = np.zeros((nodes, 2, G))
        T[nodes - 1] = np.asarray(rho)[:, None]
        for k in range(M - 1, -1, -1):
            a, b, v = left[k], right[k], n + k
            w = T[v] * L[v]
            p1[k] = np.where(w.sum(0) > 0, w[1] / w.sum(0), 0.0)
            for c, sib in ((a, b), (b, a)):
                U = T[v] * msg[sib]
                s = U.sum(0)
                U = np.where(s > 0, U / s, 0.0)
                joint = U[:, None, :] * P[c][:, :, None] * L[c][None, :, :]       # [above, below, gene]
                tot = joint.sum((0, 1))
                gains[c] = np.where(tot > 0, joint[0, 1] / tot, 0.0)
                losses[c] = np.where(tot > 0, joint[1, 0] / tot, 0.0)
                T[c] = np.einsum("bg,ba->ag", U, P[c])
    return lnlik, p1, gains, losses


def combine(per_class, weights=None, gene_class=None, logs=False):
    """per_class[k] = (lik or lnlik, p1, gains, losses) of class k -> dict(lnl_g, post[G, K], p1, gains, losses): every gene its
    class's answer (gene_class), or the mixture over the classes with `weights`"""
    K = len(per_class)
    with np.errstate(divide="ignore"):
        ln = np.array([pc[0] if logs else np.log(pc[0]) for pc in per_class])          # (K, G)
    G = ln.shape[1]
    if gene_class is not None or K == 1:
        cls = np.zeros(G, int) if gene_class is None else np.asarray(gene_class, int)
        post = np.zeros((G, K))
        post[np.arange(G), cls] = 1.0
        lnl_g = ln[cls, np.arange(G)]
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            top = ln.max(0)
            rel = np.where(np.isfinite(top), np.asarray(weights)[:, None] * np.exp(ln - np.where(np.isfinite(top), top, 0.0)), 0.0)
            tot = rel.sum(0)
            lnl_g = np.where(tot > 0, top + np.log(tot), -np.inf)
            post = np.where(tot > 0, rel / np.where(tot > 0, tot, 1.0), np.asarray(weights)[:, None]).T
    has = np.isfinite(lnl_g)
    p1 = sum(post[:, k] * per_class[k][1] for k in range(K)) * has
    gains = sum(post[:, k] * per_class[k][2] for k in range(K)) * has
    losses = sum(post[:, k] * per_class[k][3] for k in range(K)) * has
    return dict(lnl_g=lnl_g, post=post, p1=p1, gains=gains, losses=losses)


def reference(rows, left, right, lengths, gains, losses, rho, weights=None, gene_class=None, method=brute):
    """the whole model: `gains`, `losses` one value per class"""
    per_class = [method(rows, left, right, lengths, g, l, rho) for g, l in zip(gains, losses)]
    return combine(per_class, weights, gene_class, logs=method is pruning)


def evolve(rng, left, right, lengths, gain, loss, rho1, genes):
    """`genes` independent genes down the tree -> (leaf rows[N, genes] uint8, inner states[M, genes] uint8, true gains[genes],
    true losses[genes]: the branches on which the two ends differ, by direction)"""
    n, M = len(left) + 1, len(left)
    state = np.zeros((n + M, genes), np.uint8)
    state[n + M - 1] = rng.random(genes) < rho1
    tg, tl = np.zeros(genes, int), np.zeros(genes, int)
    for k in range(M - 1, -1, -1):
        for c in (left[k], right[k]):
            P = transition(gain, loss, lengths[c])
            up = state[n + k]
            state[c] = rng.random(genes) < P[up, 1]
            tg += (up == 0) & (state[c] == 1)
            tl += (up == 1) & (state[c] == 0)
    return state[:n].copy(), state[n:].copy(), tg, tl
