"""Plain numpy restatement of the core allele profiles (docs/ALLELE_PROFILES.md) from an N x L byte matrix in output row
order: np.unique over the byte rows of every locus, renumbered by first appearance, and the distance matrix by broadcasting.
No fingerprints, no bands, no shards: nothing here is shared with the library."""
import numpy as np


def default_bounds(L, n_loci):
    return [g * L // n_loci for g in range(n_loci + 1)]


def renumber(column):
    """dense numbers of the values of one column (any array whose rows are the individuals' alleles), by first appearance"""
    column = np.asarray(column)
    if column.ndim == 1:
        column = column.reshape(-1, 1)
    _, first, inverse = np.unique(column, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(first.size, np.int64)
    rank[np.argsort(first)] = np.arange(first.size)
    return rank[np.asarray(inverse).reshape(-1)]


def _labels(same):
    """same[i, j]: i and j are joined -> the smallest member of every connected component, per individual"""
    N = same.shape[0]
    label = np.arange(N)
    for _ in range(N):
        new = np.where(same, label[None, :], N).min(1)
        new = np.minimum(new, label)
        if np.array_equal(new, label):
            break
        label = new
    return label


def from_ids(ids, dist_bins=None, complex_max=0, core_sites=0, sites_covered=0):
    """everything from an N x n_loci table of any allele ids"""
    ids = np.asarray(ids)
    N, M = ids.shape
    dist_bins = min(M + 1, 16384) if dist_bins is None else dist_bins
    prof = np.stack([renumber(ids[:, g]) for g in range(M)], axis=1)
    d = np.zeros((N, N), np.int64)
    for g in range(M):                   # (one locus at a time: N x N, not N x N x M)
        d += prof[:, g][:, None] != prof[:, g][None, :]
    iu = np.triu_indices(N, 1)
    dp = d[iu]
    pairs = N * (N - 1) // 2
    locus_alleles = prof.max(0) + 1
    locus_same = np.array([sum(int(c) * (int(c) - 1) // 2 for c in np.bincount(prof[:, g])) for g in range(M)], np.int64)
    st = _labels(d == 0)
    cx = _labels(d <= complex_max)
    st_size, cx_size = np.bincount(st, minlength=N), np.bincount(cx, minlength=N)
    out = dict(pop_size=N, pairs=pairs, core_sites=core_sites, loci=M, sites_covered=sites_covered, alleles_total=int(locus_alleles.sum()),
               max_alleles=int(locus_alleles.max()), monomorphic_loci=int((locus_alleles == 1).sum()), sequence_types=int((st_size > 0).sum()),
               singleton_sts=int((st_size == 1).sum()), largest_st=int(st_size.max()), identical_pairs=int((dp == 0).sum()),
               complexes=int((cx_size > 0).sum()), largest_complex=int(cx_size.max()), edges=int((dp <= complex_max).sum()), sum_d=int(dp.sum()),
               min_d=int(dp.min()), max_d=int(dp.max()), dist_bins=dist_bins, complex_max=complex_max)
    out["mean_distance"] = float(out["sum_d"]) / float(pairs) / float(M)
    out["hist"] = np.bincount(dp * dist_bins // (M + 1), minlength=dist_bins)
    out.update(locus_alleles=locus_alleles, locus_same_pairs=locus_same, st=st, complex=cx, profiles=prof)
    return out


def from_matrix(m, n_loci, bounds=None, **kw):
    """everything from the N x L byte matrix"""
    m = np.asarray(m, np.uint8)
    N, L = m.shape
    b = default_bounds(L, n_loci) if bounds is None else [int(x) for x in bounds]
    ids = np.stack([renumber(m[:, b[g]:b[g + 1]]) for g in range(n_loci)], axis=1)
    return from_ids(ids, core_sites=L, sites_covered=b[-1] - b[0], **kw)


def assert_equal(got, want, rounds=None):
    """got: an AlleleProfiles; want: the dict of from_ids / from_matrix.  Integers equal, the double bit for bit."""
    for k, v in want.items():
        g = getattr(got, k)
        if isinstance(v, np.ndarray):
            if k == "profiles" and g is None:
                continue
            assert np.array_equal(np.asarray(g).astype(np.int64), v.astype(np.int64)), k
        elif k == "mean_distance":
            assert np.float64(g).tobytes() == np.float64(v).tobytes(), (k, g, v)
        else:
            assert g == v, (k, g, v)
    if rounds is not None:
        assert got.rounds == rounds
