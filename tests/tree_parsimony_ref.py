"""A numpy restatement of docs/TREE_PARSIMONY.md that shares nothing with the library: the sequential Fitch up and down passes
over (matrix bytes, merge list), the summary, a brute-force minimum over all internal assignments for small trees, the level
schedule, union-find forms of the two merge-list builders, and the trees and matrices the tests run on."""
import itertools

import numpy as np

BEYOND = 0xffffffff
BINS = 64
BASES = np.array([1, 2, 4, 8], np.uint8)
INTEGERS = ("pop_size", "sites", "genes", "merges", "trees", "covered_leaves", "spanning", "total_changes", "changed_sites", "max_changes",
            "gene_total_changes", "gene_total_gains", "gene_total_losses", "min_changes", "excess_changes", "homoplasic_sites")
ARRAYS = ("site_changes", "site_hist", "branch_changes", "gene_changes", "gene_gains", "gene_losses", "branch_gains", "branch_losses")


def class_bits(m):
    m = np.asarray(m, np.uint8)
    return np.where(np.isin(m, BASES), m, np.uint8(16)).astype(np.uint8)


def parents(left, right, N):
    out = np.full(N + len(left), -1, np.int64)
    for k, (a, b) in enumerate(zip(left, right)):
        out[int(a)], out[int(b)] = N + k, N + k
    return out


def lowbit(x):
    return (x & (~x + np.uint8(1))).astype(np.uint8)


def fitch(states, left, right, down=True):
    """states: (N, C) class bits -> changes[C], and with `down` the (N + M, C) boolean table of the branches that change and the
    picks X"""
    N, C = states.shape
    M = len(left)
    S = np.zeros((N + M, C), np.uint8)
    S[:N] = states
    changes = np.zeros(C, np.int64)
    for k in range(M):
        a, b = S[int(left[k])], S[int(right[k])]
        i = a & b
        e = i == 0
        S[N + k] = np.where(e, a | b, i)
        changes += e
    if not down:
        return changes, None, None
    par = parents(left, right, N)
    X = np.zeros((N + M, C), np.uint8)
    moved = np.zeros((N + M, C), bool)
    for k in range(M - 1, -1, -1):
        v = N + k
        if par[v] < 0:
            X[v] = lowbit(S[v])
        for c in (int(left[k]), int(right[k])):
            X[c] = np.where((X[v] & S[c]) != 0, X[v], lowbit(S[c]))
            moved[c] = X[c] != X[v]
    return changes, moved, X


def brute_force(states, left, right):
    """the true minimum number of changes of every column over ALL assignments of the five states to the internal nodes (M <= 5)"""
    N, C = states.shape
    M = len(left)
    assign = np.array(list(itertools.product((1, 2, 4, 8, 16), repeat=M)), np.uint8)       # (5^M, M)
    best = np.zeros(C, np.int64)
    for s in range(C):
        cost = np.zeros(len(assign), np.int64)
        for k in range(M):
            for c in (int(left[k]), int(right[k])):
                child = assign[:, c - N] if c >= N else np.full(len(assign), states[c, s], np.uint8)
                cost += child != assign[:, k]
        best[s] = cost.min()
    return best


def levels(left, right, N):
    lev = np.zeros(N + len(left), np.int64)
    for k, (a, b) in enumerate(zip(left, right)):
        lev[N + k] = 1 + max(lev[int(a)], lev[int(b)])
    return lev[N:], int(lev.max())


def parsimony(core, left, right, acc=None):
    """every output of the call as a dict: core (N, L) bytes, acc (N, G) presences or None"""
    core = np.asarray(core, np.uint8)
    N, L = core.shape
    M = len(left)
    par = parents(left, right, N)
    st = class_bits(core)
    changes, moved, _ = fitch(st, left, right)
    classes = np.array([len(np.unique(st[:, s])) for s in range(L)], np.int64)
    out = dict(pop_size=N, sites=L, genes=0, merges=M, trees=int((par[N:] < 0).sum()), covered_leaves=int((par[:N] >= 0).sum()),
               spanning=int(M == N - 1), total_changes=int(changes.sum()), changed_sites=int((changes > 0).sum()),
               max_changes=int(changes.max()) if L else 0, gene_total_changes=0, gene_total_gains=0, gene_total_losses=0, min_changes=0,
               excess_changes=0, homoplasic_sites=0, ci=0.0)
    out["site_changes"] = changes.astype(np.uint32)
    out["site_hist"] = np.bincount(np.minimum(changes, BINS - 1), minlength=BINS).astype(np.uint64)
    out["branch_changes"] = moved.sum(axis=1).astype(np.uint64)
    assert int(out["branch_changes"].sum()) == out["total_changes"] and not out["branch_changes"][par < 0].any()
    if out["spanning"]:
        out["min_changes"] = int((classes - 1).sum())
        out["excess_changes"] = out["total_changes"] - out["min_changes"]
        out["homoplasic_sites"] = int((changes > classes - 1).sum())
        out["ci"] = out["min_changes"] / out["total_changes"] if out["total_changes"] else 0.0
    for name in ARRAYS[3:]:
        out[name] = None
    if acc is not None:
        g = np.where(np.asarray(acc) != 0, 2, 1).astype(np.uint8)
        gch, gmoved, X = fitch(g, left, right)
        gain, loss = gmoved & (X == 2), gmoved & (X == 1)
        out.update(genes=g.shape[1], gene_changes=gch.astype(np.uint32), gene_gains=gain.sum(axis=0).astype(np.uint32),
                   gene_losses=loss.sum(axis=0).astype(np.uint32), branch_gains=gain.sum(axis=1).astype(np.uint64),
                   branch_losses=loss.sum(axis=1).astype(np.uint64), gene_total_changes=int(gch.sum()), gene_total_gains=int(gain.sum()),
                   gene_total_losses=int(loss.sum()))
        assert out["gene_total_gains"] + out["gene_total_losses"] == out["gene_total_changes"]
    return out


def assert_equal(got, want, skip=()):
    """a TreeParsimony against the dict of parsimony(): every integer, ci and every array that is not skipped"""
    for name in INTEGERS:
        if name not in skip:
            assert getattr(got, name) == want[name], (name, getattr(got, name), want[name])
    if "ci" not in skip:
        assert got.ci == want["ci"], (got.ci, want["ci"])
    for name in ARRAYS:
        if name in skip:
            continue
        g, w = getattr(got, name), want[name]
        assert (g is None) == (w is None), name
        if w is not None:
            assert g.dtype == w.dtype and np.array_equal(g, w), (name, np.flatnonzero(np.asarray(g) != np.asarray(w))[:8])


# -- the merge-list builders ----------------------------------------------------------------------------------------------
def merges_from_tree(lo, hi, N):
    """Kruskal over the edges in their given order with a dict per cluster: left is the cluster with the smaller smallest row"""
    cluster = {i: (i, {i}) for i in range(N)}            # row -> (node, members), shared by the members
    left, right = [], []
    for k, (a, b) in enumerate(zip(lo, hi)):
        ca, cb = cluster[int(a)], cluster[int(b)]
        assert ca is not cb
        if min(cb[1]) < min(ca[1]):
            ca, cb = cb, ca
        left.append(ca[0])
        right.append(cb[0])
        merged = (N + k, ca[1] | cb[1])
        for i in merged[1]:
            cluster[i] = merged
    return np.array(left, np.uint32), np.array(right, np.uint32)


def merges_from_genealogy(order, coal):
    N = len(order)
    pos = sorted((int(coal[r]), r) for r in range(N - 1) if int(coal[r]) != BEYOND)
    node = {r: (int(order[r]), r, r) for r in range(N)}  # internal row -> (node, first row, last row) of its interval
    left, right, height = [], [], []
    for k, (t, r) in enumerate(pos):
        a, b = node[r], node[r + 1]
        assert a[2] == r and b[1] == r + 1
        left.append(a[0])
        right.append(b[0])
        height.append(t)
        merged = (N + k, a[1], b[2])
        for i in range(a[1], b[2] + 1):
            node[i] = merged
    return np.array(left, np.uint32), np.array(right, np.uint32), np.array(height, np.uint32)


# -- trees ----------------------------------------------------------------------------------------------------------------
def random_joining(rng, N, M=None):
    """M merges of two random roots each (M < N - 1: a forest with uncovered leaves when M is well below)"""
    M = N - 1 if M is None else M
    roots = list(range(N))
    left, right = [], []
    for k in range(M):
        i, j = rng.choice(len(roots), 2, replace=False)
        left.append(roots[i])
        right.append(roots[j])
        for x in sorted((int(i), int(j)), reverse=True):
            roots.pop(x)
        roots.append(N + k)
    return np.array(left, np.uint32), np.array(right, np.uint32)


def caterpillar(N, leaves=None):
    """depth N - 1, one merge per level; `leaves`: the order the leaves join in"""
    leaves = np.arange(N) if leaves is None else np.asarray(leaves)
    left = np.concatenate(([leaves[0]], N + np.arange(N - 2))).astype(np.uint32)
    return left, leaves[1:].astype(np.uint32)


def balanced(N, leaves=None):
    """rounds of neighbouring pairs: the widest level holds N // 2 merges"""
    cur = list(range(N)) if leaves is None else [int(x) for x in leaves]
    left, right, k = [], [], 0
    while len(cur) > 1:
        nxt = []
        for i in range(0, len(cur) - 1, 2):
            left.append(cur[i])
            right.append(cur[i + 1])
            nxt.append(N + k)
            k += 1
        if len(cur) & 1:
            nxt.append(cur[-1])
        cur = nxt
    return np.array(left, np.uint32), np.array(right, np.uint32)


def trees(rng, N):
    """name -> (left, right): the trees every shape is run on"""
    perm = rng.permutation(N)
    out = {"random": random_joining(rng, N), "caterpillar": caterpillar(N), "balanced": balanced(N),
           "permuted": balanced(N, perm) if N > 2 else caterpillar(N, perm[::-1])}
    if N >= 4:
        out["forest"] = random_joining(rng, N, max(1, int(0.6 * N)))
    return out


# -- matrices -------------------------------------------------------------------------------------------------------------
def onehot(rng, shape):
    return BASES[rng.integers(0, 4, shape)]


def evolved(rng, N, L, left, right, junk=True):
    """one-hot columns that follow the tree: a site changes on a branch with its own rate (none, rare, common), 2 % of the cells
    are random bases on top (homoplasy); with `junk` 3 % arbitrary bytes, a column of zeros and a column of 0x03"""
    M = len(left)
    rate = rng.choice([0.0, 0.5 / M, 3.0 / M, 0.1], L)
    state = np.zeros((N + M, L), np.uint8)
    have = np.zeros(N + M, bool)
    for k in range(M - 1, -1, -1):
        v = N + k
        if not have[v]:
            state[v] = onehot(rng, L)
        for c in (int(left[k]), int(right[k])):
            state[c] = np.where(rng.random(L) < rate, onehot(rng, L), state[v])
            have[c] = True
    m = state[:N].copy()
    m[~have[:N]] = onehot(rng, (int((~have[:N]).sum()), L))
    noise = rng.random((N, L)) < 0.02
    m[noise] = onehot(rng, (N, L))[noise]
    if junk:
        bad = rng.random((N, L)) < 0.03
        m[bad] = rng.integers(0, 256, int(bad.sum()), dtype=np.uint8)
        if L > 3:
            m[:, 1], m[:, 3] = 0, 3
    return np.ascontiguousarray(m)


def evolved_genes(rng, N, G, left, right):
    """presences that follow the tree with gains and losses, 3 % flipped on top"""
    M = len(left)
    state = np.zeros((N + M, G), np.uint8)
    have = np.zeros(N + M, bool)
    for k in range(M - 1, -1, -1):
        v = N + k
        if not have[v]:
            state[v] = rng.random(G) < 0.4
        for c in (int(left[k]), int(right[k])):
            state[c] = state[v] ^ (rng.random(G) < 2.0 / M)
            have[c] = True
    a = state[:N].copy()
    a[~have[:N]] = rng.random((int((~have[:N]).sum()), G)) < 0.4
    return np.ascontiguousarray(a ^ (rng.random((N, G)) < 0.03).astype(np.uint8))
