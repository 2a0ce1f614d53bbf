"""The single-linkage tree of docs/LINKAGE_TREE.md in plain Python integers, written from its definitions: Kruskal with its own
union-find and its own cross-multiplying compare.  What ps_tree_from_counts and the device entries must reproduce edge for edge
and field for field.  Not a transliteration of the library."""
import functools

import numpy as np

CORE, ACC = 0, 1
INT_FIELDS = ("pairs", "core_sites", "core_genes", "metric", "edges", "undefined_edges", "distinct_heights")
# (`rounds` is informational: only its range is asserted, by the device tests)


def distance(metric, h, i, u, core_sites, core_genes):
    """-> (num, den) of one pair from its numerators; (0, 0) = undefined"""
    if metric == CORE:
        return int(h) // 2, int(core_sites)
    b = int(u) + int(core_genes)
    return (int(u) - int(i), b) if b else (0, 0)


def cmp_distance(x, y):
    """-1 / 0 / 1; undefined is above every defined distance and equal to undefined"""
    (n1, d1), (n2, d2) = x, y
    if d1 == 0 or d2 == 0:
        return (d1 == 0) - (d2 == 0)
    left, right = n1 * d2, n2 * d1
    return (left > right) - (left < right)


def cmp_edge(x, y):
    """edges (num, den, lo, hi) under (distance, lo, hi)"""
    c = cmp_distance(x[:2], y[:2])
    if c:
        return c
    return (x[2:] > y[2:]) - (x[2:] < y[2:])


def tree(metric, r1, r2, core_h, acc_inter, acc_union, pop_size, core_sites, core_genes):
    """-> dict of INT_FIELDS and lo, hi (uint32), num, den (uint64): the minimum spanning forest of the list, ascending"""
    edges = []
    for x, y, h, i, u in zip(r1, r2, core_h, acc_inter, acc_union):
        edges.append(distance(metric, h, i, u, core_sites, core_genes) + (min(int(x), int(y)), max(int(x), int(y))))
    edges.sort(key=functools.cmp_to_key(cmp_edge))
    parent = list(range(int(pop_size)))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    kept = []
    for e in edges:
        a, b = find(e[2]), find(e[3])
        if a != b:
            parent[max(a, b)] = min(a, b)
            kept.append(e)
    heights = sum(1 for k, e in enumerate(kept) if k == 0 or cmp_distance(kept[k - 1][:2], e[:2]) != 0)
    col = lambda k, dt: np.array([e[k] for e in kept], dt)
    return dict(pairs=len(r1), core_sites=int(core_sites), core_genes=int(core_genes), metric=metric, edges=len(kept),
                undefined_edges=sum(1 for e in kept if e[1] == 0), distinct_heights=heights,
                num=col(0, np.uint64), den=col(1, np.uint64), lo=col(2, np.uint32), hi=col(3, np.uint32))


def all_pairs(n):
    """the full i < j list, row-major"""
    i, j = np.triu_indices(int(n), 1)
    return i.astype(np.uint32), j.astype(np.uint32)


def assert_spanning(got, pop_size):
    """N - 1 edges that join everything into one component, sorted strictly ascending under the total order"""
    assert got.edges == pop_size - 1 == got.lo.size
    parent = list(range(pop_size))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for a, b in zip(got.lo, got.hi):
        assert a < b
        x, y = find(int(a)), find(int(b))
        assert x != y                                   # (no edge closes a cycle)
        parent[max(x, y)] = min(x, y)
    assert len({find(k) for k in range(pop_size)}) == 1
    assert_sorted(got)


def assert_sorted(got):
    e = [(int(n), int(d), int(a), int(b)) for n, d, a, b in zip(got.num, got.den, got.lo, got.hi)]
    assert all(cmp_edge(e[k], e[k + 1]) < 0 for k in range(len(e) - 1))


def assert_equal(got, want, pop_size):
    """got: a pansim_amd.LinkageTree; want: tree()'s dict.  The four edge arrays and every integer field but `rounds`."""
    for name in INT_FIELDS:
        assert getattr(got, name) == want[name], (name, getattr(got, name), want[name])
    assert got.pop_size == pop_size
    for name, dt in (("lo", np.uint32), ("hi", np.uint32), ("num", np.uint64), ("den", np.uint64)):
        a = getattr(got, name)
        assert a.dtype == dt and a.shape == (want["edges"],), name
        assert np.array_equal(a, want[name]), (name, a, want[name])
    assert_sorted(got)
    assert got.distance.dtype == np.float64 and np.array_equal(np.isnan(got.distance), got.den == 0)
    ok = got.den != 0
    assert np.array_equal(got.distance[ok], got.num[ok].astype(np.float64) / got.den[ok].astype(np.float64))
