"""The neighbour-joining tree of docs/NEIGHBOUR_JOINING.md restated in NumPy float64, written from its rule: every line of the rule
is one NumPy expression in the rule's own association (separate element-wise operations, so nothing is fused), the pair is the
first minimum of the upper triangle in row-major order, which is the strict order (q, lo id, hi id) when ids are rows.  What
ps_nj_from_counts and the device entries must reproduce bit for bit.  Beside it the builders of the tests: random trees with
integer branches, their path metric, infinite-sites populations that realise it, and the splits of a join list.  Not a
transliteration of the library."""
import numpy as np

CORE, ACC = 0, 1
INT_FIELDS = ("pop_size", "pairs", "core_sites", "core_genes", "metric", "joins", "negative_branches")


def all_pairs(n):
    """the full i < j list, row-major"""
    i, j = np.triu_indices(int(n), 1)
    return i.astype(np.uint32), j.astype(np.uint32)


def distances(metric, r1, r2, core_h, acc_inter, acc_union, pop_size, core_genes):
    """the N x N float64 entry distances of a complete pair list: h >> 1 as a double, or one division a / b"""
    n = int(pop_size)
    D = np.zeros((n, n), np.float64)
    r1, r2 = np.asarray(r1, np.int64), np.asarray(r2, np.int64)
    if metric == CORE:
        d = (np.asarray(core_h, np.uint32) >> np.uint32(1)).astype(np.float64)
    else:
        i, u = np.asarray(acc_inter, np.uint64), np.asarray(acc_union, np.uint64)
        d = (u - i).astype(np.float64) / (u + np.uint64(core_genes)).astype(np.float64)
    D[r1, r2] = d
    D[r2, r1] = d
    return D


def join(D):
    """the rule on a symmetric float64 matrix with a zero diagonal (changed in place); ids are rows -> (left, right, len_left,
    len_right), N - 1 joins in the order performed"""
    N = D.shape[0]
    r = np.zeros(N, np.float64)
    for k in range(N):                  # ascending row k from +0.0; the diagonal's +0.0 leaves a sum of non-negative terms as it is
        r = r + D[:, k]
    alive = np.arange(N)
    node = list(range(N))
    left, right = np.zeros(N - 1, np.uint32), np.zeros(N - 1, np.uint32)
    ll, lr = np.zeros(N - 1, np.float64), np.zeros(N - 1, np.float64)
    for t in range(N - 1):
        n = N - t
        if n > 2:
            sub = D[np.ix_(alive, alive)]
            q = (np.float64(n - 2) * sub - r[alive][:, None]) - r[alive][None, :]      # row = lo, column = hi above the diagonal
            q[np.tril_indices(n)] = np.inf
            x, y = divmod(int(np.argmin(q)), n)                                        # the first minimum: the smallest (lo, hi)
            lo, hi = int(alive[x]), int(alive[y])
            dlh = D[lo, hi]
            b_lo = np.float64(0.5) * dlh + (r[lo] - r[hi]) / (np.float64(2.0) * np.float64(n - 2))
            b_hi = dlh - b_lo
        else:
            lo, hi = int(alive[0]), int(alive[1])
            dlh = D[lo, hi]
            b_lo, b_hi = dlh, np.float64(0.0)
        left[t], right[t], ll[t], lr[t] = node[lo], node[hi], b_lo, b_hi
        node[lo] = N + t
        ks = alive[(alive != lo) & (alive != hi)]
        dlk, dhk = D[lo, ks].copy(), D[hi, ks].copy()
        duk = np.float64(0.5) * ((dlk + dhk) - dlh)
        r[ks] = ((r[ks] - dlk) - dhk) + duk
        D[lo, ks] = duk
        D[ks, lo] = duk
        r[lo] = np.float64(0.5) * ((r[lo] + r[hi]) - np.float64(n) * dlh)
        alive = alive[alive != hi]
    return left, right, ll, lr


def tree(metric, r1, r2, core_h, acc_inter, acc_union, pop_size, core_sites, core_genes):
    """the neighbour-joining tree of the complete list -> the dict that assert_equal compares"""
    left, right, ll, lr = join(distances(metric, r1, r2, core_h, acc_inter, acc_union, pop_size, core_genes))
    return dict(pop_size=int(pop_size), pairs=len(r1), core_sites=int(core_sites), core_genes=int(core_genes), metric=metric,
                joins=int(pop_size) - 1, negative_branches=int((ll < 0.0).sum() + (lr < 0.0).sum()), left=left, right=right,
                len_left=ll, len_right=lr)


def assert_equal(got, want):
    """got: a pansim_amd.NeighbourJoiningTree; want: tree()'s dict.  Every field, the children, and the lengths bit for bit."""
    for name in INT_FIELDS:
        assert getattr(got, name) == want[name], (name, getattr(got, name), want[name])
    for name in ("left", "right"):
        a = getattr(got, name)
        assert a.dtype == np.uint32 and np.array_equal(a, want[name]), (name, a, want[name])
    for name in ("len_left", "len_right"):
        a = getattr(got, name)
        assert a.dtype == np.float64 and a.shape == want[name].shape, name
        assert np.array_equal(a.view(np.uint64), want[name].view(np.uint64)), (name, a, want[name])


# -- planted trees -------------------------------------------------------------------------------------------------------------

def random_tree(rng, n, longest=9):
    """a random binary tree over the leaves 0 .. n - 1 as a join list (left, right, len_left, len_right) with integer branches
    in 1 .. longest: n - 1 times two random nodes of those left are joined; the last join is the artificial root"""
    nodes = list(range(n))
    left, right = np.zeros(n - 1, np.uint32), np.zeros(n - 1, np.uint32)
    for k in range(n - 1):
        a, b = (nodes.pop(int(rng.integers(len(nodes)))) for _ in range(2))
        left[k], right[k] = a, b
        nodes.append(n + k)
    ll, lr = (rng.integers(1, longest + 1, n - 1).astype(np.float64) for _ in range(2))
    return left, right, ll, lr


def below(left, right, n):
    """per node (leaves first) the sorted rows below it"""
    sets = [[r] for r in range(n)]
    for a, b in zip(left, right):
        sets.append(sorted(sets[int(a)] + sets[int(b)]))
    return sets


def path_lengths(tree_, n):
    """the n x n float64 path metric of a join list: a branch separates the leaves below it from all others"""
    left, right, ll, lr = tree_
    sets = below(left, right, n)
    D = np.zeros((n, n), np.float64)
    for k in range(n - 1):
        for child, length in ((int(left[k]), ll[k]), (int(right[k]), lr[k])):
            inside = np.zeros(n, bool)
            inside[sets[child]] = True
            D[np.ix_(inside, ~inside)] += length
            D[np.ix_(~inside, inside)] += length
    return D


def infinite_sites(tree_, n):
    """(n, L) one-hot core bytes: every branch owns as many private sites as it is long, where the leaves below it carry base 2
    and all others base 1 -- a pair differs at the sites of the branches on its path, so h / 2 is the path length"""
    left, right, ll, lr = tree_
    sets = below(left, right, n)
    cols = []
    for k in range(n - 1):
        for child, length in ((int(left[k]), ll[k]), (int(right[k]), lr[k])):
            col = np.full(n, 1, np.uint8)
            col[sets[child]] = 2
            cols += [col] * int(length)
    return np.ascontiguousarray(np.stack(cols, axis=1))


def splits(left, right, len_left, len_right, n):
    """{the side of a branch that does not hold row 0, as a frozenset: its length}; the two edges at the artificial root cut the
    same way and are merged (their lengths added)"""
    sets = below(left, right, n)
    everyone = frozenset(range(n))
    out = {}
    for k in range(n - 1):
        for child, length in ((int(left[k]), len_left[k]), (int(right[k]), len_right[k])):
            side = frozenset(sets[child])
            if 0 in side:
                side = everyone - side
            out[side] = out.get(side, np.float64(0.0)) + np.float64(length)
    return out
