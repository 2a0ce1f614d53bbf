"""The strain clusters of docs/STRAIN_CLUSTERS.md in plain Python integers, written from its definitions: what
ps_clusters_from_counts and the device entries must reproduce label for label and field for field.  Not a transliteration of
the library."""
import numpy as np

INT_FIELDS = ("pairs", "core_sites", "core_genes", "edges", "clusters", "singletons", "largest_cluster", "within_pairs",
              "undefined_pairs")          # (`rounds` is informational: part of no comparison)
NO_CORE = 2**64 - 1


def is_edge(h, i, u, core_genes, core_max_d=NO_CORE, acc_num=0, acc_den=0):
    """-> (edge, undefined) of one pair from its numerators"""
    edge, undefined = True, False
    if core_max_d != NO_CORE:
        edge = int(h) // 2 <= core_max_d
    if acc_den:
        a, b = int(u) - int(i), int(u) + int(core_genes)
        undefined = b == 0
        edge = edge and not undefined and a * acc_den <= acc_num * b
    return edge, undefined


def clusters(r1, r2, core_h, acc_inter, acc_union, pop_size, core_sites, core_genes, core_max_d=NO_CORE, acc_num=0, acc_den=0):
    """-> dict of INT_FIELDS and labels (pop_size uint32: the smallest index of each one's cluster)"""
    assert core_max_d != NO_CORE or acc_den
    n = int(pop_size)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    edges = undefined = 0
    for x, y, h, i, u in zip(r1, r2, core_h, acc_inter, acc_union):
        e, un = is_edge(h, i, u, core_genes, core_max_d, acc_num, acc_den)
        undefined += un
        if e:
            edges += 1
            a, b = find(int(x)), find(int(y))
            parent[max(a, b)] = min(a, b)
    labels = np.array([find(k) for k in range(n)], np.uint32)          # the smaller root is kept: the smallest member
    sizes = np.bincount(labels, minlength=n)
    sizes = sizes[sizes > 0]
    return dict(pairs=len(r1), core_sites=int(core_sites), core_genes=int(core_genes), edges=edges, clusters=int(sizes.size),
                singletons=int((sizes == 1).sum()), largest_cluster=int(sizes.max()),
                within_pairs=int(sum(int(s) * (int(s) - 1) // 2 for s in sizes)), undefined_pairs=undefined, labels=labels)


def all_pairs(n):
    """the full i < j list, row-major"""
    i, j = np.triu_indices(int(n), 1)
    return i.astype(np.uint32), j.astype(np.uint32)


def thresholds(core_sites, core_max=None, acc_max=None):
    """the one conversion of real thresholds to the integers of the contract -> (core_max_d, acc_num, acc_den)"""
    d = NO_CORE if core_max is None else int(np.floor(float(core_max) * int(core_sites)))
    return (d, 0, 0) if acc_max is None else (d, int(np.floor(float(acc_max) * 2**20)), 2**20)


def assert_equal(got, want, pop_size):
    """got: a pansim_amd.StrainClusters; want: clusters()'s dict.  The labels and every integer field but `rounds`."""
    for name in INT_FIELDS:
        assert getattr(got, name) == want[name], (name, getattr(got, name), want[name])
    assert got.pop_size == pop_size
    assert got.labels.dtype == np.uint32 and got.labels.shape == (pop_size,)
    assert np.array_equal(got.labels, want["labels"])
    assert int(got.sizes().sum()) == pop_size and got.sizes().size == got.clusters and int(got.sizes()[0]) == got.largest_cluster
