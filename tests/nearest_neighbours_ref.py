"""The nearest neighbours and lineages of docs/NEAREST_NEIGHBOURS.md restated from their definitions in numpy and Python
integers: the numerators of every ordered pair from the two matrices themselves, the order of the distances by cross products
in Python integers, a stable sort on (distance, row), union-find for the lineages.  What the device entries,
ps_neighbours_from_counts and ps_lineages_from_neighbours must reproduce entry for entry and field for field.  Nothing is
imported from the library."""
import functools

import numpy as np

CORE, ACC = 0, 1
NONE = 2**32 - 1
INT_FIELDS = ("pop_size", "pairs", "core_sites", "core_genes", "metric", "k", "undefined_neighbours", "graph_edges", "mutual_edges")
LINEAGE_FIELDS = ("pop_size", "rank", "edges", "lineages", "largest_lineage", "within_pairs")


def cmp_distance(x, y):
    """-1 / 0 / 1 of (num, den) pairs; undefined (den 0) is above every defined distance and equal to undefined"""
    (n1, d1), (n2, d2) = x, y
    if d1 == 0 or d2 == 0:
        return (d1 == 0) - (d2 == 0)
    left, right = int(n1) * int(d2), int(n2) * int(d1)
    return (left > right) - (left < right)


def _common_bits(m):
    """c[i, j] = the bits set in both row i and row j, and the bits set in each row.  The rows are compared bit by bit through one
    product of 0/1 matrices; every partial sum is a whole number below 2^24, so float32 is exact."""
    bits = np.unpackbits(np.ascontiguousarray(m, np.uint8), axis=1).astype(np.float32)
    assert bits.shape[1] < 2**24
    return (bits @ bits.T).astype(np.int64), bits.sum(1).astype(np.int64)


def numerators(core, acc):
    """(h, I, U), each (N, N) int64, of all ordered pairs: h = the bits in which two core rows differ (popcount of x ^ y summed
    over the sites), I / U = the genes that both / either of two accessory rows hold"""
    N = core.shape[0]
    c, n = _common_bits(core)
    h = n[:, None] + n[None, :] - 2 * c
    if acc is None or acc.shape[1] == 0:
        return h, np.zeros((N, N), np.int64), np.zeros((N, N), np.int64)
    a = (np.asarray(acc) != 0).astype(np.uint8)
    i, g = _common_bits(a)
    return h, i, g[:, None] + g[None, :] - i


def distances(metric, h, i, u, core_sites, core_genes):
    """(num, den) arrays from the numerators; (0, 0) = undefined"""
    if metric == CORE:
        return h // 2, np.full_like(h, int(core_sites))
    den = u + int(core_genes)
    return np.where(den == 0, 0, u - i), den


def ranks(num, den):
    """a whole number per entry that orders the distances exactly: the distinct (num, den) sorted by cross products in Python
    integers, equal fractions sharing one rank, the undefined distance last"""
    assert num.max(initial=0) < 2**31 and den.max(initial=0) < 2**32
    packed = (num.astype(np.uint64) << np.uint64(32)) | den.astype(np.uint64)
    uniq, inverse = np.unique(packed, return_inverse=True)
    pairs = [(int(p) >> 32, int(p) & 0xffffffff) for p in uniq]
    order = sorted(range(len(pairs)), key=functools.cmp_to_key(lambda a, b: cmp_distance(pairs[a], pairs[b])))
    rank_of = np.zeros(len(pairs), np.int64)
    r = 0
    for pos, idx in enumerate(order):
        if pos and cmp_distance(pairs[order[pos - 1]], pairs[idx]) != 0:
            r += 1
        rank_of[idx] = r
    return rank_of[inverse.reshape(-1)].reshape(num.shape)


def graph_counts(nbr, rank=None):
    """(distinct unordered pairs, pairs listed from both ends) of the first `rank` columns of nbr; NONE entries skipped"""
    N, k = nbr.shape
    j = nbr[:, :k if rank is None else rank].astype(np.int64)
    i = np.broadcast_to(np.arange(N, dtype=np.int64)[:, None], j.shape)
    listed = (j != NONE) & (j != i)
    i, j = i[listed], j[listed]
    directed = np.unique(i * N + j)                          # i -> j as one whole number
    mutual = int(np.isin(directed % N * N + directed // N, directed).sum()) // 2
    return int(np.unique(np.minimum(i, j) * N + np.maximum(i, j)).size), mutual


def summary(metric, nbr, den, pairs, core_sites, core_genes):
    N, k = nbr.shape
    edges, mutual = graph_counts(nbr)
    return dict(pop_size=N, pairs=int(pairs), core_sites=int(core_sites), core_genes=int(core_genes), metric=metric, k=k,
                undefined_neighbours=int(((den == 0) & (nbr != NONE)).sum()), graph_edges=edges, mutual_edges=mutual)


def neighbours(metric, core, acc, core_genes, k, nums=None):
    """-> dict of INT_FIELDS and nbr (uint32), num, den (uint64), each (N, k): the k nearest others of every row of the two
    matrices (rows = output rows) under (distance, row).  nums: numerators(core, acc), where a caller has them already."""
    N, L = core.shape
    num, den = distances(metric, *(nums or numerators(core, acc)), L, core_genes)
    rk = ranks(num, den)
    np.fill_diagonal(rk, rk.max() + 1)                       # (never one's own neighbour: k <= N - 1 others come first)
    nbr = np.argsort(rk, axis=1, kind="stable")[:, :k]       # stable: equal distances stay in ascending row order
    rows = np.arange(N)[:, None]
    assert (nbr != rows).all()
    out = summary(metric, nbr.astype(np.uint32), den[rows, nbr], N * (N - 1) // 2, L, core_genes)
    out.update(nbr=nbr.astype(np.uint32), num=num[rows, nbr].astype(np.uint64), den=den[rows, nbr].astype(np.uint64))
    return out


def from_pairs(metric, r1, r2, core_h, acc_inter, acc_union, pop_size, core_sites, core_genes, k):
    """the same from any pair list: every pair is a candidate of both its ends; of several copies of a pair the first under
    (distance, position in the list) is listed; unfilled slots hold NONE, 0, 0"""
    N = int(pop_size)
    cand = [[] for _ in range(N)]
    for x, y, h, i, u in zip(r1, r2, core_h, acc_inter, acc_union):
        if metric == CORE:
            d = (int(h) // 2, int(core_sites))
        else:
            b = int(u) + int(core_genes)
            d = (int(u) - int(i), b) if b else (0, 0)
        cand[int(x)].append(d + (int(y),))
        cand[int(y)].append(d + (int(x),))

    def cmp(a, b):
        return cmp_distance(a[:2], b[:2]) or (a[2] > b[2]) - (a[2] < b[2])

    nbr, num, den = np.full((N, k), NONE, np.uint32), np.zeros((N, k), np.uint64), np.zeros((N, k), np.uint64)
    for i in range(N):
        n = 0
        for e in sorted(cand[i], key=functools.cmp_to_key(cmp)):      # (sorted() is stable)
            if n == k:
                break
            if e[2] in nbr[i, :n]:
                continue
            num[i, n], den[i, n], nbr[i, n] = e
            n += 1
    out = summary(metric, nbr, den, len(r1), core_sites, core_genes)
    out.update(nbr=nbr, num=num, den=den)
    return out


def lineages(nbr, rank):
    """-> (labels uint32, dict of LINEAGE_FIELDS): the connected components of {i, nbr[i, q]}, q < rank; labels[i] = the smallest
    row of i's component"""
    N, k = nbr.shape
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i in range(N):
        for j in nbr[i, :rank]:
            if j != NONE:
                a, b = find(i), find(int(j))
                parent[max(a, b)] = min(a, b)
    labels = np.array([find(i) for i in range(N)], np.uint32)
    sizes = np.bincount(labels, minlength=N)
    sizes = sizes[sizes > 0]
    return labels, dict(pop_size=N, rank=rank, edges=graph_counts(nbr, rank)[0], lineages=int(sizes.size), largest_lineage=int(sizes.max()),
                        within_pairs=int((sizes * (sizes - 1) // 2).sum()))


def assert_equal(got, want):
    """got: a pansim_amd.NearestNeighbours; want: neighbours()'s or from_pairs()'s dict.  The three arrays, every field, the
    doubles bit for bit, and the identity graph_edges + mutual_edges = listed entries."""
    for name in INT_FIELDS:
        assert getattr(got, name) == want[name], (name, getattr(got, name), want[name])
    shape = (want["pop_size"], want["k"])
    for name, dt in (("nbr", np.uint32), ("num", np.uint64), ("den", np.uint64)):
        a = getattr(got, name)
        assert a.dtype == dt and a.shape == shape, name
        bad = np.argwhere(a != want[name])
        assert bad.size == 0, (name, bad[:5], a[tuple(bad[0])], want[name][tuple(bad[0])])
    assert got.graph_edges + got.mutual_edges == int((got.nbr != NONE).sum())
    assert got.distance.dtype == np.float64 and got.distance.shape == shape
    assert np.array_equal(np.isnan(got.distance), got.den == 0)
    ok = got.den != 0
    want_d = got.num[ok].astype(np.float64) / got.den[ok].astype(np.float64)
    assert np.array_equal(got.distance[ok].view(np.uint64), want_d.view(np.uint64))


def assert_lineages(got, nbr, rank):
    """got: (labels, summary dict) of NearestNeighbours.lineages(rank)"""
    labels, fields = lineages(nbr, rank)
    assert got[0].dtype == np.uint32 and np.array_equal(got[0], labels)
    assert got[1] == fields, (got[1], fields)


def all_pairs(n):
    """the full i < j list, row-major"""
    i, j = np.triu_indices(int(n), 1)
    return i.astype(np.uint32), j.astype(np.uint32)


def tsv_files(want, fmt_f64):
    """the three files of --print_knn as text: _knn.tsv, _lineages.tsv, _knn_summary.tsv"""
    N, k = want["nbr"].shape
    knn = "".join("%d\t%d\t%d\t%d\t%d\t%s\n" % (i, r + 1, want["nbr"][i, r], want["num"][i, r], want["den"][i, r],
                                               fmt_f64(float(want["num"][i, r]) / float(want["den"][i, r])) if want["den"][i, r] else "NaN")
                  for i in range(N) for r in range(k))
    labels, _ = lineages(want["nbr"], k)
    lin = "".join("%d\t%d\n" % (i, labels[i]) for i in range(N))
    text = "".join("%s\t%d\n" % (f, want[f]) for f in INT_FIELDS)
    for r in range(1, k + 1):
        f = lineages(want["nbr"], r)[1]
        text += "lineages\t%d\t%d\t%d\n" % (r, f["lineages"], f["largest_lineage"])
    return knn, lin, text
