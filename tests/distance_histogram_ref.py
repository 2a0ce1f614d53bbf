"""The joint distance histogram of docs/DISTANCE_HISTOGRAM.md in plain Python integers, written from its definitions: what
ps_histogram_from_counts and the device entries must reproduce field for field.  Not a transliteration of the library."""
import numpy as np

INT_FIELDS = ("pairs", "core_sites", "core_genes", "core_bins", "acc_bins", "core_span", "undefined_pairs", "core_clamped",
              "core_d_min", "core_d_max", "core_d_sum", "core_d_sqsum")


def histogram(core_h, acc_inter, acc_union, core_sites, core_genes, core_bins, acc_bins, core_span=0):
    """-> dict of INT_FIELDS, mean_core_distance and joint ((core_bins, acc_bins) uint64)"""
    d = [int(h) // 2 for h in core_h]
    span = int(core_span) if core_span else max(d) + 1
    joint = np.zeros((core_bins, acc_bins), np.uint64)
    undefined = clamped = 0
    for dk, i, u in zip(d, acc_inter, acc_union):
        i, u = int(i), int(u)
        if dk >= span:
            clamped += 1
        bc = min(core_bins - 1, dk * core_bins // span)
        a, b = u - i, u + int(core_genes)
        if b == 0:
            undefined += 1
            continue
        ba = min(acc_bins - 1, a * acc_bins // b)
        joint[bc, ba] += np.uint64(1)
    pairs = len(d)
    return dict(pairs=pairs, core_sites=int(core_sites), core_genes=int(core_genes), core_bins=core_bins, acc_bins=acc_bins,
                core_span=span, undefined_pairs=undefined, core_clamped=clamped, core_d_min=min(d), core_d_max=max(d),
                core_d_sum=sum(d), core_d_sqsum=sum(x * x for x in d),
                mean_core_distance=float(sum(d)) / float(pairs) / float(core_sites) if core_sites else 0.0, joint=joint)


def all_pairs(n):
    """the full i < j list, row-major"""
    i, j = np.triu_indices(int(n), 1)
    return i.astype(np.uint32), j.astype(np.uint32)


def assert_equal(got, want, pop_size=None):
    """got: a pansim_amd.DistanceHistogram; want: histogram()'s dict.  Every integer field, the double and every bin."""
    for name in INT_FIELDS:
        assert getattr(got, name) == want[name], (name, getattr(got, name), want[name])
    if pop_size is not None:
        assert got.pop_size == pop_size
    assert got.mean_core_distance == want["mean_core_distance"]
    assert got.joint.dtype == np.uint64 and got.joint.shape == want["joint"].shape
    assert np.array_equal(got.joint, want["joint"])
    assert int(got.joint.sum()) == got.pairs - got.undefined_pairs
    assert np.array_equal(got.core_marginal, want["joint"].sum(axis=1))
    assert np.array_equal(got.acc_marginal, want["joint"].sum(axis=0))


def core_edges(core_bins, core_span):
    """bin k of the core axis holds d in [ceil(k S / Bc), ceil((k + 1) S / Bc))"""
    return [-((-k * core_span) // core_bins) for k in range(core_bins + 1)]
