"""The NumPy and set restatements behind the bootstrap tests (docs/BOOTSTRAP_SUPPORT.md): the draw rule on
site_weights_ref.philox, the counting on frozensets of leaves, a few merge lists, and the independent path of the device tests
(M[:, sites_b] built on the host, loaded into a fresh handle, the existing tree called on it).  Nothing here calls the new
entries."""
import numpy as np

from site_weights_ref import philox

STREAM_BOOTSTRAP = 22
INT_FIELDS = ("pop_size", "pairs", "core_sites", "core_genes", "method", "replicates", "draws", "merges", "support_sum", "supported_50",
              "supported_70", "supported_95")
METHODS = ("linkage", "upgma", "nj")


def draw_sites(seed, replicate, core_sites, draws, first=0, count=None):
    """draw k of a replicate: the block (k >> 1, replicate, 0, 22) under the key `seed`; the words (x, y) serve an even k and
    (z, w) an odd one; site = ((x << 32 | y) * L) >> 64, in Python integers"""
    count = draws - first if count is None else count
    k = np.arange(first, first + count, dtype=np.uint64)
    x, y, z, w = philox(k >> np.uint64(1), replicate, 0, STREAM_BOOTSTRAP, seed)
    odd = (k & np.uint64(1)).astype(bool)
    hi, lo = np.where(odd, z, x), np.where(odd, w, y)
    L = int(core_sites)
    return np.array([(((int(a) << 32) | int(b)) * L) >> 64 for a, b in zip(hi.tolist(), lo.tolist())], np.uint32)


def leaf_sets(left, right, n):
    """the leaf set below every merge of a merge list"""
    below = [frozenset([i]) for i in range(n)]
    for a, b in zip(np.asarray(left).tolist(), np.asarray(right).tolist()):
        below.append(below[a] | below[b])
    return below[n:]


def _looked_for(sets, n, unrooted):
    """rooted: the sets themselves.  Unrooted: of every split the side without leaf 0 -- None where a side holds fewer than two
    leaves: such a split is in every tree"""
    if not unrooted:
        return list(sets)
    everyone, out = frozenset(range(n)), []
    for s in sets:
        side = everyone - s if 0 in s else s
        out.append(None if len(side) < 2 or len(side) > n - 2 else side)
    return out


def support_from_merges(ref_left, ref_right, rep_left, rep_right, n, unrooted):
    """support[k] = the replicates whose tree holds what merge k of the reference tree is looked for by; shared[b] = the
    reference merges found in replicate b"""
    ref = _looked_for(leaf_sets(ref_left, ref_right, n), n, unrooted)
    support, shared = np.zeros(n - 1, np.uint32), np.zeros(len(rep_left), np.uint32)
    for b, (rl, rr) in enumerate(zip(rep_left, rep_right)):
        have = set(_looked_for(leaf_sets(rl, rr, n), n, unrooted))
        for k, s in enumerate(ref):
            if s is None or s in have:
                support[k] += 1
                shared[b] += 1
    return support, shared


def random_merges(rng, n):
    """a random binary tree as a merge list: two free nodes joined at a time"""
    free, left, right = list(range(n)), [], []
    for k in range(n - 1):
        i, j = sorted(rng.choice(len(free), 2, replace=False).tolist())
        b, a = free.pop(j), free.pop(i)
        left.append(a)
        right.append(b)
        free.append(n + k)
    return np.array(left, np.uint32), np.array(right, np.uint32)


def caterpillar(n):
    """((((0, 1), 2), 3), ...)"""
    return np.array([0] + [n + k for k in range(n - 2)], np.uint32), np.arange(1, n, dtype=np.uint32)


def balanced(n):
    """neighbours joined level by level, an odd one carried up"""
    level, left, right = list(range(n)), [], []
    while len(level) > 1:
        nxt = []
        for i in range(0, len(level) - 1, 2):
            left.append(level[i])
            right.append(level[i + 1])
            nxt.append(n + len(left) - 1)
        if len(level) % 2:
            nxt.append(level[-1])
        level = nxt
    return np.array(left, np.uint32), np.array(right, np.uint32)


def summary(n, core_sites, core_genes, method, replicates, draws, support):
    s = np.asarray(support, np.uint64)
    inner = s[:-1] * np.uint64(100)
    return dict(pop_size=n, pairs=n * (n - 1) // 2, core_sites=core_sites, core_genes=core_genes, method=METHODS.index(method),
                replicates=replicates, draws=draws, merges=n - 1, support_sum=int(s.sum()),
                supported_50=int((inner >= 50 * replicates).sum()), supported_70=int((inner >= 70 * replicates).sum()),
                supported_95=int((inner >= 95 * replicates).sum()))


def tree_merges(pa, core, acc, method):
    """the merge list of the method's own call on two handles"""
    if method == "linkage":
        t = core.linkage_tree(acc)
        return pa.merges_from_tree(t.lo, t.hi, core.size)[:2]
    t = core.upgma_tree(acc) if method == "upgma" else core.neighbour_joining(acc)
    return t.left, t.right


def independent(pa, matrix, acc_matrix, core_genes, method, site_lists):
    """matrix: (N, L) one-hot bytes in output rows; site_lists: one array of global sites per replicate.  The method's tree of
    `matrix`, then of every matrix[:, sites_b] in a fresh Population, counted by the set restatement -> (left, right, support,
    shared)"""
    n = matrix.shape[0]

    def tree_of(m):
        core = pa.Population(n, m.shape[1], 4, True, 0.0, 0, core_genes)
        acc = pa.Population(n, acc_matrix.shape[1], 2, False, 0.5, 0, core_genes)
        core.load_matrix(np.ascontiguousarray(m))
        acc.load_matrix(acc_matrix)
        out = tree_merges(pa, core, acc, method)
        core.close()
        acc.close()
        return np.array(out[0], np.uint32), np.array(out[1], np.uint32)

    left, right = tree_of(matrix)
    reps = [tree_of(matrix[:, np.asarray(s, np.int64)]) for s in site_lists]
    support, shared = support_from_merges(left, right, [r[0] for r in reps], [r[1] for r in reps], n, method == "nj")
    return left, right, support, shared
