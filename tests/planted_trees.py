"""Populations whose all-pairs trees and clusters are known in closed form (NumPy only; no device, no library), so that the device
read-outs can be judged at sizes where the plain-Python references (tests/upgma_tree_ref.py, tests/linkage_tree_ref.py,
tests/strain_clusters_ref.py: O(N^3), O(N^2 log N)) cannot run.  tests/test_planted_trees.py holds every closed form below to
those references, field for field, at N = 8, 64 and 128.

The population.  The N = 2^K rows are the leaves of a complete binary tree, shuffled: row r is leaf `leaf[r]`, leaf p is row
`row[p]`.  The block of level l that holds leaf p is p >> l (2^l leaves, N >> l blocks; a block of level 0 is a leaf); its left
half is the block 2 (p >> l) of level l - 1.  The *level* of a pair is that of the smallest block that holds both, the bit
length of leaf[i] ^ leaf[j].  Internal node q(l, b) = first[l] + b, levels ascending, owns

* `c` core sites q c .. q c + c - 1 at which its left leaves carry base 2, its right leaves base 4 and every other leaf base 1
  (L = c (N - 1)).  A pair of level l differs at the c sites of its lowest common ancestor (2 against 4) and at the c sites of
  each of the l - 1 nodes between that ancestor and either leaf (2 or 4 against 1): d = h / 2 = c (2 l - 1).
* two accessory genes 2 q, 2 q + 1: the left leaves carry the first, the right leaves the second (G = 2 (N - 1)).  Every leaf
  has one gene per ancestor, K in all; a pair of level l shares those of the K - l ancestors above its lowest common one:
  I = K - l, U = K + l, a = U - I = 2 l, b = U + core_genes = K + l + core_genes.

Both c (2 l - 1) / L and 2 l / (K + l + core_genes) ascend strictly in l and depend on nothing else: two ultrametrics.

The closed forms.  `low[l][b]` is the smallest row of block b of level l: the id of the cluster, and the label of the component,
that the block forms.

* UPGMA (docs/UPGMA_TREE.md).  The average distance of two clusters that are blocks is the distance of the level that joins
  them; while blocks of level l - 1 remain unmerged the smallest pairs are the siblings of level l, so the sequential algorithm
  merges level by level and inside a level by (lo id, hi id) -- by low[l][b] alone, the lo ids of a level being distinct.  The
  merge of block b joins 2^(l-1) x 2^(l-1) pairs, each at (n, d) = distance(metric, l): num = 4^(l-1) n and den = 4^(l-1) d
  (the core den |A| |B| L, the accessory den the sum of b).  `left` is the half with the smaller low; a half of level 0 is its
  row, a half of level l - 1 the node N + (its place in the list).  Every cluster's nearest other cluster is its sibling, which
  chose it: the device takes one round per level.  K rounds, K distinct heights.
* The minimum spanning tree under (distance, lo, hi) (docs/LINKAGE_TREE.md).  Kruskal takes every pair of level 1, then per
  block of level 2 the first of its four pairs across the halves, and so on: per block of level l the smallest (lo, hi) with lo
  in one half and hi in the other.  The smallest lo is the block's smallest row; hi is then the smallest row of the other
  half, which is above lo.  The edge is (min, max) of the two halves' lows at (n, d) of level l, the order again by level and
  low[l][b].  N - 1 edges, none undefined, K distinct heights.
* Strain clusters (docs/STRAIN_CLUSTERS.md) when exactly the pairs of level <= l are edges (the thresholds lie between the
  distances of level l and l + 1): the components are the blocks of level l, labels low[l][leaf >> l]; N 2^-l clusters of 2^l,
  edges = within_pairs = N (2^l - 1) / 2, all singletons at l = 0, no pair undefined."""
import numpy as np

CORE, ACC = 0, 1


class Planted:
    def __init__(self, K, c=1, core_genes=3, seed=0):
        self.K, self.N, self.c, self.core_genes = int(K), 1 << int(K), int(c), int(core_genes)
        self.L, self.G = self.c * (self.N - 1), 2 * (self.N - 1)
        self.leaf = np.random.default_rng(seed).permutation(self.N).astype(np.int64)
        self.row = np.empty(self.N, np.int64)
        self.row[self.leaf] = np.arange(self.N)
        self.first = [0, 0]                                   # first[l]: the first node of level l (levels from 1)
        for l in range(1, self.K):
            self.first.append(self.first[l] + (self.N >> l))
        self.low = [self.row.reshape(self.N >> l, 1 << l).min(1) for l in range(self.K + 1)]

    def _owners(self):
        """per level l = 1 .. K: (the node above each row, whether the row is in that node's right half)"""
        for l in range(1, self.K + 1):
            yield self.first[l] + (self.leaf >> l), ((self.leaf >> (l - 1)) & 1).astype(bool)

    def core_matrix(self):
        """(N, L) one-hot bytes, rows in output order"""
        m = np.full((self.N, self.L), 1, np.uint8)
        rows, sites = np.arange(self.N)[:, None], np.arange(self.c)[None, :]
        for node, right in self._owners():
            m[rows, node[:, None] * self.c + sites] = np.where(right, 4, 2).astype(np.uint8)[:, None]
        return m

    def acc_matrix(self):
        """(N, G) 0 / 1 bytes, rows in output order"""
        a = np.zeros((self.N, self.G), np.uint8)
        for node, right in self._owners():
            a[np.arange(self.N), 2 * node + right] = 1
        return a

    def level(self, r1, r2):
        """the level of each pair of rows (0 for a row against itself): the bit length of leaf[r1] ^ leaf[r2]"""
        return np.frexp((self.leaf[np.asarray(r1, np.int64)] ^ self.leaf[np.asarray(r2, np.int64)]).astype(np.float64))[1]

    def distance(self, metric, l):
        """(num, den) of a pair of level l"""
        return (self.c * (2 * l - 1), self.L) if metric == CORE else (2 * l, self.K + l + self.core_genes)

    def _levels(self):
        """per level l: (the lows of the left halves, of the right halves, the order of the blocks by their own low)"""
        for l in range(1, self.K + 1):
            a, b = self.low[l - 1][0::2], self.low[l - 1][1::2]
            yield l, a, b, np.argsort(np.minimum(a, b), kind="stable")

    def _head(self, metric):
        return dict(pairs=self.N * (self.N - 1) // 2, core_sites=self.L, core_genes=self.core_genes, metric=metric, distinct_heights=self.K)

    def upgma(self, metric):
        """the dict of upgma_tree_ref.tree, and `rounds`"""
        left, right, size, num, den = [], [], [], [], []
        node = self.row                                        # the node of each block of the level below
        for l, a, b, order in self._levels():
            first, second = np.where(a < b, node[0::2], node[1::2]), np.where(a < b, node[1::2], node[0::2])
            left.append(first[order])
            right.append(second[order])
            n, d = self.distance(metric, l)
            pairs = 4 ** (l - 1)
            size += [2 << (l - 1)] * order.size
            num += [pairs * n] * order.size
            den += [pairs * d] * order.size
            node = np.empty(order.size, np.int64)
            node[order] = self.N + len(size) - order.size + np.arange(order.size)
        out = self._head(metric)
        out.update(merges=self.N - 1, root_num=num[-1], root_den=den[-1], rounds=self.K, left=np.concatenate(left).astype(np.uint32),
                   right=np.concatenate(right).astype(np.uint32), size=np.array(size, np.uint32), num=np.array(num, np.uint64),
                   den=np.array(den, np.uint64))
        return out

    def mst(self, metric):
        """the dict of linkage_tree_ref.tree"""
        lo, hi, num, den = [], [], [], []
        for l, a, b, order in self._levels():
            lo.append(np.minimum(a, b)[order])
            hi.append(np.maximum(a, b)[order])
            n, d = self.distance(metric, l)
            num += [n] * order.size
            den += [d] * order.size
        out = self._head(metric)
        out.update(edges=self.N - 1, undefined_edges=0, lo=np.concatenate(lo).astype(np.uint32), hi=np.concatenate(hi).astype(np.uint32),
                   num=np.array(num, np.uint64), den=np.array(den, np.uint64))
        return out

    def labels(self, l):
        """the smallest row of each row's block of level l"""
        return self.low[l][self.leaf >> l].astype(np.uint32)

    def clusters(self, l):
        """the dict of strain_clusters_ref.clusters when exactly the pairs of level <= l are edges"""
        within = self.N * ((1 << l) - 1) // 2
        return dict(pairs=self.N * (self.N - 1) // 2, core_sites=self.L, core_genes=self.core_genes, edges=within, clusters=self.N >> l,
                    singletons=self.N if l == 0 else 0, largest_cluster=1 << l, within_pairs=within, undefined_pairs=0, labels=self.labels(l))


def numerators(core_matrix, acc_matrix):
    """(r1, r2, h, I, U) of every pair i < j, row-major, from a one-hot core matrix and a 0 / 1 accessory matrix: h = 2 (L - the
    sites at which both carry the same base), I = the genes both carry, U = cnt[i] + cnt[j] - I; as matrix products, exact in
    float32 below 2^24 columns"""
    n, L = core_matrix.shape
    assert max(L, acc_matrix.shape[1]) < 2**24 and np.isin(core_matrix, (1, 2, 4, 8)).all() and acc_matrix.max() <= 1
    same = np.zeros((n, n), np.float32)
    for base in (1, 2, 4, 8):
        x = (core_matrix == base).astype(np.float32)
        same += x @ x.T
    a = acc_matrix.astype(np.float32)
    inter, cnt = (a @ a.T).astype(np.int64), acc_matrix.sum(1, dtype=np.int64)
    r1, r2 = np.triu_indices(n, 1)
    h = 2 * (L - same.astype(np.int64)[r1, r2])
    i = inter[r1, r2]
    return r1.astype(np.uint32), r2.astype(np.uint32), h.astype(np.uint32), i.astype(np.uint32), (cnt[r1] + cnt[r2] - i).astype(np.uint32)
