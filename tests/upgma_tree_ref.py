"""The average-linkage (UPGMA) tree of docs/UPGMA_TREE.md in plain Python integers, written from its definitions: the sequential
algorithm -- N - 1 times a scan of all pairs of clusters for the smallest under (distance, lo id, hi id), O(N^3) in all -- with
cross-multiplied comparisons in Python's unbounded integers; no floats, no numpy in the comparison.  Beside it the argument the
device rests on, restated: rounds of mutual nearest neighbours followed by the ordering step give the same list.  What
ps_upgma_from_counts and the device entries must reproduce merge for merge and field for field.  Not a transliteration of the
library."""
import functools
import heapq

import numpy as np

CORE, ACC = 0, 1
INT_FIELDS = ("pairs", "core_sites", "core_genes", "metric", "merges", "distinct_heights", "root_num", "root_den")
# (`rounds` is informational: the device tests assert its value where the construction fixes it)


def matrices(metric, r1, r2, core_h, acc_inter, acc_union, pop_size, core_genes):
    """-> (S, B): N lists of N ints, the per-pair num and (accessory metric) den; B is None under the core metric"""
    n = int(pop_size)
    S = [[0] * n for _ in range(n)]
    B = [[0] * n for _ in range(n)] if metric == ACC else None
    for x, y, h, i, u in zip(map(int, r1), map(int, r2), map(int, core_h), map(int, acc_inter), map(int, acc_union)):
        if metric == CORE:
            S[x][y] = S[y][x] = h // 2
        else:
            S[x][y] = S[y][x] = u - i
            B[x][y] = B[y][x] = u + int(core_genes)
    return S, B


def sequential(S, B, less=None):
    """the sequential algorithm on the pair sums (changed in place) -> the merges (num, den, id a, id b, size a, size b), a < b,
    in the order they are performed; den = |A| |B| under the core metric (B is None), else the sum of b.  `less(num1, den1, num2,
    den2)` takes the place of the exact num1 den2 < num2 den1, for a test that asks what a wrong comparator would produce"""
    n = len(S)
    alive, size, out = list(range(n)), [1] * n, []
    while len(alive) > 1:
        # the pairs in ascending order of (lo id, hi id): of equal distances the first one found is the smallest
        bn, bd, ba, bb = 0, 0, -1, -1
        for k, a in enumerate(alive):
            Sa, sa, Ba = S[a], size[a], (B[a] if B else None)
            for b in alive[k + 1:]:
                num = Sa[b]
                den = Ba[b] if B else sa * size[b]
                if ba < 0 or (num * bd < bn * den if less is None else less(num, den, bn, bd)):
                    bn, bd, ba, bb = num, den, a, b
        out.append((bn, bd, ba, bb, size[ba], size[bb]))
        for c in alive:
            if c != ba and c != bb:
                S[ba][c] = S[c][ba] = S[ba][c] + S[bb][c]
                if B:
                    B[ba][c] = B[c][ba] = B[ba][c] + B[bb][c]
        size[ba] += size[bb]
        alive.remove(bb)
    return out


def cmp_merge(x, y):
    """merges (num, den, a, b, ...) under (distance, lo id, hi id)"""
    left, right = x[0] * y[1], y[0] * x[1]
    if left != right:
        return -1 if left < right else 1
    return (x[2:4] > y[2:4]) - (x[2:4] < y[2:4])


def rounds(S, B):
    """rounds of mutual nearest neighbours on the pair sums (changed in place) -> (merges in the order found, rounds taken):
    every cluster finds its nearest other cluster under the total order, every pair that chose each other merges"""
    n = len(S)
    alive, size, out, taken = list(range(n)), [1] * n, [], 0
    while len(alive) > 1:
        taken += 1
        nn = {}
        for a in alive:
            best = None
            for b in alive:
                if b != a:
                    e = (S[a][b], B[a][b] if B else size[a] * size[b], min(a, b), max(a, b))
                    if best is None or cmp_merge(e, best) < 0:
                        best = e
            nn[a] = best
        pairs = [e for a, e in nn.items() if a == e[2] and nn[e[3]][2:4] == e[2:4]]
        assert pairs, "a round merged nothing"
        for num, den, a, b in pairs:
            out.append((num, den, a, b, size[a], size[b]))
        # rows, then columns: simultaneous merges meet in the matrix
        for _, _, a, b in pairs:
            for c in range(n):
                S[a][c] += S[b][c]
                if B:
                    B[a][c] += B[b][c]
        gone = {b for _, _, _, b in pairs}
        for r in alive:
            if r not in gone:
                for _, _, c, d in pairs:
                    S[r][c] += S[r][d]
                    if B:
                        B[r][c] += B[r][d]
        for _, _, a, b in pairs:
            size[a] += size[b]
        alive = [a for a in alive if a not in gone]
    return out, taken


def ordered(merges, pop_size):
    """the ordering step: the merges of a tree, simultaneous ones in one piece, linked into nodes and put into the order of the
    sequential algorithm -- of the nodes whose children are out, the smallest under (distance, lo id, hi id) next"""
    n = int(pop_size)
    cur, child, parent, pending = list(range(n)), [], {}, []
    for t, (_, _, a, b, _, _) in enumerate(merges):
        kids = (cur[a], cur[b])
        assert None not in kids
        child.append(kids)
        pending.append(sum(1 for c in kids if c >= n))
        for c in kids:
            if c >= n:
                parent[c - n] = t
        cur[a], cur[b] = n + t, None
    key = functools.cmp_to_key(cmp_merge)
    ready = [(key(merges[t]), t) for t in range(len(merges)) if pending[t] == 0]
    heapq.heapify(ready)
    seq, out = {}, []
    while ready:
        _, t = heapq.heappop(ready)
        seq[t] = len(out)
        num, den, _, _, sa, sb = merges[t]
        out.append(tuple(c if c < n else n + seq[c - n] for c in child[t]) + (sa + sb, num, den))
        if t in parent:
            pending[parent[t]] -= 1
            if pending[parent[t]] == 0:
                heapq.heappush(ready, (key(merges[parent[t]]), parent[t]))
    assert len(out) == len(merges)
    return out


def result(metric, nodes, n_pairs, pop_size, core_sites, core_genes):
    """(left, right, size, num, den) per merge -> the dict that assert_equal compares; the core den takes its factor L here"""
    scale = int(core_sites) if metric == CORE else 1
    num, den = [e[3] for e in nodes], [e[4] * scale for e in nodes]
    heights = sum(1 for k in range(len(nodes)) if k == 0 or num[k - 1] * den[k] != num[k] * den[k - 1])
    return dict(pairs=int(n_pairs), core_sites=int(core_sites), core_genes=int(core_genes), metric=metric, merges=len(nodes),
                distinct_heights=heights, root_num=num[-1], root_den=den[-1],
                left=np.array([e[0] for e in nodes], np.uint32), right=np.array([e[1] for e in nodes], np.uint32),
                size=np.array([e[2] for e in nodes], np.uint32), num=np.array(num, np.uint64), den=np.array(den, np.uint64))


def tree(metric, r1, r2, core_h, acc_inter, acc_union, pop_size, core_sites, core_genes, less=None):
    """the UPGMA tree of the complete list by the sequential algorithm (a merge's node is its place in the list)"""
    S, B = matrices(metric, r1, r2, core_h, acc_inter, acc_union, pop_size, core_genes)
    n, nodes, cur = int(pop_size), [], list(range(int(pop_size)))
    for k, (num, den, a, b, sa, sb) in enumerate(sequential(S, B, less)):
        nodes.append((cur[a], cur[b], sa + sb, num, den))
        cur[a] = n + k
    return result(metric, nodes, len(r1), pop_size, core_sites, core_genes)


def tree_by_rounds(metric, r1, r2, core_h, acc_inter, acc_union, pop_size, core_sites, core_genes):
    """the same tree by the rounds and the ordering step -> (dict, rounds taken)"""
    S, B = matrices(metric, r1, r2, core_h, acc_inter, acc_union, pop_size, core_genes)
    merges, taken = rounds(S, B)
    return result(metric, ordered(merges, pop_size), len(r1), pop_size, core_sites, core_genes), taken


def all_pairs(n):
    """the full i < j list, row-major"""
    i, j = np.triu_indices(int(n), 1)
    return i.astype(np.uint32), j.astype(np.uint32)


def members(got):
    """per node (leaves first) the sorted rows below it"""
    sets = [[r] for r in range(got.pop_size)]
    for a, b in zip(got.left, got.right):
        sets.append(sorted(sets[int(a)] + sets[int(b)]))
    return sets


def assert_monotone(got):
    """the heights do not descend, and `left` is the child with the smaller id (its smallest row)"""
    num, den = [int(x) for x in got.num], [int(x) for x in got.den]
    assert all(num[k] * den[k + 1] <= num[k + 1] * den[k] for k in range(len(num) - 1))
    sets = members(got)
    for k, (a, b) in enumerate(zip(got.left, got.right)):
        assert sets[int(a)][0] < sets[int(b)][0] and got.size[k] == len(sets[got.pop_size + k])


def assert_equal(got, want, pop_size):
    """got: a pansim_amd.UpgmaTree; want: tree()'s dict.  The five arrays and every integer field but `rounds`."""
    for name in INT_FIELDS:
        assert getattr(got, name) == want[name], (name, getattr(got, name), want[name])
    assert got.pop_size == pop_size and got.merges == pop_size - 1
    for name, dt in (("left", np.uint32), ("right", np.uint32), ("size", np.uint32), ("num", np.uint64), ("den", np.uint64)):
        a = getattr(got, name)
        assert a.dtype == dt and a.shape == (want["merges"],), name
        assert np.array_equal(a, want[name]), (name, a, want[name])
    assert got.distance.dtype == np.float64
    assert np.array_equal(got.distance, got.num.astype(np.float64) / got.den.astype(np.float64))
