"""A numpy restatement of the tree comparison (docs/TREE_COMPARISON.md) that shares nothing with the library: leaf sets by set
union, the lowest common ancestor of every pair filled in merge by merge, clades as frozensets, and for small trees a literal
enumeration of all triples.  The tree generators are those of tree_parsimony_ref."""
import itertools
import math

import numpy as np

from tree_parsimony_ref import balanced, caterpillar, merges_from_genealogy, random_joining, trees  # noqa: F401

MAX_VAL = (1 << 18) - 1
INT_FIELDS = ("pop_size", "merges_a", "merges_b", "pairs", "joined_both", "joined_a_only", "joined_b_only", "joined_neither", "sum_a",
              "sum_b", "sum_aa", "sum_bb", "sum_ab", "triples", "resolved_a", "resolved_b", "shared_triplets", "clades_a", "clades_b",
              "shared_clades", "rf_distance", "bins_a", "bins_b", "span_a", "span_b")
DOUBLES = ("cophenetic_r", "triplet_recall", "triplet_precision", "clade_recall", "clade_precision")


class Tree:
    """one tree: members[k] (bool row per merge), val[k], top[k] (the highest ancestor with the same value), lca[i, j] (the merge
    index of the pair, -1 where not joined)"""

    def __init__(self, N, left, right, val=None):
        left, right = [int(x) for x in left], [int(x) for x in right]
        M = len(left)
        self.N, self.M, self.left, self.right = N, M, left, right
        self.val = np.arange(1, M + 1, dtype=np.int64) if val is None else np.asarray(val, np.int64)
        self.members = np.zeros((M, N), bool)
        self.lca = np.full((N, N), -1, np.int32)
        parent = [-1] * M
        for k in range(M):
            side = []
            for x in (left[k], right[k]):
                if x < N:
                    s = np.zeros(N, bool)
                    s[x] = True
                else:
                    s = self.members[x - N]
                    parent[x - N] = k
                side.append(s)
            self.members[k] = side[0] | side[1]
            li, ri = np.flatnonzero(side[0]), np.flatnonzero(side[1])
            self.lca[np.ix_(li, ri)] = k
            self.lca[np.ix_(ri, li)] = k
        self.parent = parent
        self.top = list(range(M))
        for k in range(M - 1, -1, -1):
            if parent[k] >= 0 and self.val[parent[k]] == self.val[k]:
                self.top[k] = self.top[parent[k]]
        self.top = np.array(self.top, np.int64) if M else np.zeros(0, np.int64)
        self.size = self.members.sum(axis=1).astype(np.int64)
        self.is_top = self.top == np.arange(M)

    def clades(self):
        return {frozenset(np.flatnonzero(self.members[k]).tolist()): k for k in range(self.M) if self.is_top[k]}


def value_bin(v, B, S):
    return np.minimum(B - 1, (v - 1) * B // S)


def ratio(a, b):
    return a / b if b else 0.0


def cophenetic(n, sa, sb, saa, sbb, sab):
    """over Python integers"""
    n, sa, sb, saa, sbb, sab = (int(x) for x in (n, sa, sb, saa, sbb, sab))
    va, vb = n * saa - sa * sa, n * sbb - sb * sb
    if n == 0 or va == 0 or vb == 0:
        return 0.0
    return (n * sab - sa * sb) / math.sqrt(va * vb)


def compare(N, a, b, bins=(32, 32), spans=(0, 0), triplets=True):
    """a, b: (left, right) or (left, right, val) -> a dict of every field of ps_tree_compare_t, joint, in_b, in_a"""
    A, B = Tree(N, *a), Tree(N, *b)
    iu = np.triu(np.ones((N, N), bool), 1)
    ka, kb = A.lca[iu].astype(np.int64), B.lca[iu].astype(np.int64)
    ja, jb = ka >= 0, kb >= 0
    both = ja & jb
    va, vb = A.val[ka[both]], B.val[kb[both]]
    out = dict(pop_size=N, merges_a=A.M, merges_b=B.M, pairs=N * (N - 1) // 2, joined_both=int(both.sum()),
               joined_a_only=int((ja & ~jb).sum()), joined_b_only=int((~ja & jb).sum()), joined_neither=int((~ja & ~jb).sum()),
               sum_a=int(va.sum()), sum_b=int(vb.sum()), sum_aa=int((va * va).sum()), sum_bb=int((vb * vb).sum()), sum_ab=int((va * vb).sum()),
               triples=0, resolved_a=0, resolved_b=0, shared_triplets=0)
    Ba, Bb = bins
    Sa, Sb = spans[0] or int(A.val.max()), spans[1] or int(B.val.max())
    ba, bb = np.full(ka.size, Ba, np.int64), np.full(kb.size, Bb, np.int64)
    ba[ja] = value_bin(A.val[ka[ja]], Ba, Sa)
    bb[jb] = value_bin(B.val[kb[jb]], Bb, Sb)
    out["joint"] = np.bincount(ba * (Bb + 1) + bb, minlength=(Ba + 1) * (Bb + 1)).astype(np.uint64).reshape(Ba + 1, Bb + 1)
    out.update(bins_a=Ba, bins_b=Bb, span_a=Sa, span_b=Sb)
    if triplets:
        ta, tb = A.top[ka[ja]], B.top[kb[jb]]
        out["triples"] = N * (N - 1) * (N - 2) // 6
        out["resolved_a"] = int((N - A.size[ta]).sum())
        out["resolved_b"] = int((N - B.size[tb]).sum())
        # |C_A & C_B| of every pair of merges (f32 products of 0 / 1 add exactly below 2^24)
        inter = (A.members.astype(np.float32) @ B.members.astype(np.float32).T).astype(np.int64)
        ta, tb = A.top[ka[both]], B.top[kb[both]]
        out["shared_triplets"] = int((N - A.size[ta] - B.size[tb] + inter[ta, tb]).sum())
    ca, cb = A.clades(), B.clades()
    shared = set(ca) & set(cb)
    out.update(clades_a=len(ca), clades_b=len(cb), shared_clades=len(shared), rf_distance=len(ca) + len(cb) - 2 * len(shared))
    out["in_b"] = np.zeros(A.M, np.uint8)
    out["in_a"] = np.zeros(B.M, np.uint8)
    for s in shared:
        out["in_b"][ca[s]] = 1
        out["in_a"][cb[s]] = 1
    out["cophenetic_r"] = cophenetic(out["joined_both"], out["sum_a"], out["sum_b"], out["sum_aa"], out["sum_bb"], out["sum_ab"])
    out["triplet_recall"] = ratio(out["shared_triplets"], out["resolved_a"])
    out["triplet_precision"] = ratio(out["shared_triplets"], out["resolved_b"])
    out["clade_recall"] = ratio(len(shared), len(ca))
    out["clade_precision"] = ratio(len(shared), len(cb))
    return out


def _resolution(T, i, j, k):
    """the cherry of the triple in T as a frozenset, or None when it is not resolved"""
    inf = float("inf")
    v = lambda x, y: float(T.val[T.lca[x, y]]) if T.lca[x, y] >= 0 else inf
    for x, y, z in ((i, j, k), (i, k, j), (j, k, i)):
        if T.lca[x, y] >= 0 and v(x, y) < v(x, z):
            return frozenset((x, y))
    return None


def triples_brute_force(N, a, b):
    """(resolved_a, resolved_b, shared) by enumerating every triple"""
    A, B = Tree(N, *a), Tree(N, *b)
    ra = rb = sh = 0
    for i, j, k in itertools.combinations(range(N), 3):
        x, y = _resolution(A, i, j, k), _resolution(B, i, j, k)
        ra += x is not None
        rb += y is not None
        sh += x is not None and x == y
    return ra, rb, sh


def closed_forms(N, t):
    """(pairs joined, resolved, sum of val, sum of val^2) of one tree from its merges alone, O(M) in Python integers: merge k is
    the lowest common ancestor of |left_k| |right_k| pairs, and its clade is the subtree of its tie-top"""
    left, right = [int(x) for x in t[0]], [int(x) for x in t[1]]
    M = len(left)
    val = list(range(1, M + 1)) if len(t) == 2 or t[2] is None else [int(x) for x in t[2]]
    size, parent = [1] * N + [0] * M, [-1] * M
    for k in range(M):
        size[N + k] = size[left[k]] + size[right[k]]
        for x in (left[k], right[k]):
            if x >= N:
                parent[x - N] = k
    top = list(range(M))
    for k in range(M - 1, -1, -1):
        if parent[k] >= 0 and val[parent[k]] == val[k]:
            top[k] = top[parent[k]]
    w = [size[left[k]] * size[right[k]] for k in range(M)]
    return (sum(w), sum(w[k] * (N - size[N + top[k]]) for k in range(M)), sum(w[k] * val[k] for k in range(M)),
            sum(w[k] * val[k] * val[k] for k in range(M)))


def tied_values(M, step=3):
    """non-decreasing in the merge index, so never above a parent's: runs of `step` equal values"""
    return (np.arange(M) // step + 1).astype(np.uint32)


def genealogy_tree(rng, N, depth=12, beyond=0.0):
    """a random comb (order, coal) and its merge list with the coalescence times as values: many ties"""
    order = rng.permutation(N).astype(np.uint32)
    coal = rng.integers(1, depth + 1, max(N - 1, 0)).astype(np.uint32)
    coal[rng.random(coal.size) < beyond] = 0xFFFFFFFF
    if (coal == 0xFFFFFFFF).all():
        coal[0] = 1
    return merges_from_genealogy(order, coal)


def assert_equal(got, want):
    """a TreeComparison against compare(): every integer, joint, in_b, in_a by equality, the doubles within 1e-12"""
    for name in INT_FIELDS:
        assert getattr(got, name) == want[name], (name, getattr(got, name), want[name])
    for name in ("joint", "in_b", "in_a"):
        np.testing.assert_array_equal(getattr(got, name), want[name], err_msg=name)
    for name in DOUBLES:
        assert abs(getattr(got, name) - want[name]) <= 1e-12, (name, getattr(got, name), want[name])
