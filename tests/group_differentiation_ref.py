"""Group differentiation restated in numpy (docs/GROUP_DIFFERENTIATION.md), by brute force over the matrix bytes and the
labels.  Shares no code with the library: the groups come from a dictionary count, the class counts from comparisons of
the bytes, every statistic from int64 arithmetic over the count tables (nothing here passes 2^63)."""
import numpy as np

UNASSIGNED = 2**32 - 1
BASES = (1, 2, 4, 8)


def groups(labels, max_groups=16, min_size=1):
    """-> (group_of[N] with UNASSIGNED, group_label[K], group_size[K]); K == 0: empty arrays"""
    sizes = {}
    for x in labels:
        sizes[int(x)] = sizes.get(int(x), 0) + 1
    cand = sorted(((n, lab) for lab, n in sizes.items() if n >= min_size), key=lambda t: (-t[0], t[1]))[:max_groups]
    index = {lab: g for g, (_, lab) in enumerate(cand)}
    group_of = np.array([index.get(int(x), UNASSIGNED) for x in labels], np.uint32)
    return group_of, np.array([lab for _, lab in cand], np.uint32), np.array([n for n, _ in cand], np.uint32)


def class_counts(core, group_of, K):
    """core: (N, L) bytes in output order -> (L, K, 5) int64: A, C, G, T, other per site and group"""
    L = core.shape[1]
    out = np.zeros((L, K, 5), np.int64)
    for g in range(K):
        rows = core[group_of == g]
        for a, b in enumerate(BASES):
            out[:, g, a] = (rows == b).sum(0)
        out[:, g, 4] = rows.shape[0] - out[:, g, :4].sum(1)
    return out


def from_class_counts(c, group_size):
    """c: (L, K, 5) int64 -> dict of every core result (Python integers and numpy arrays)"""
    L, K, _ = c.shape
    n = [int(x) for x in group_size]
    between = np.zeros((K, K), np.uint64)
    fixed = np.zeros((K, K), np.uint64)
    for g in range(K):
        for h in range(K):
            dot = (c[:, g, :] * c[:, h, :]).sum(1)                      # per site, below 2^33
            if g == h:
                between[g, g] = int(((n[g] * n[g] - dot) // 2).sum())
                fixed[g, g] = int((dot == n[g] * n[g]).sum())
            else:
                between[g, h] = int((n[g] * n[h] - dot).sum())
                fixed[g, h] = int((dot == 0).sum())
    Na = sum(n)
    sq = (c * c).sum(2)                                                  # (L, K)
    site_within = ((np.array(n, np.int64)[None, :] ** 2 - sq) // 2).sum(1).astype(np.uint32).reshape(L)
    pooled = c.sum(1)
    site_total = ((Na * Na - (pooled * pooled).sum(1)) // 2).astype(np.uint32).reshape(L)
    out = dict(sites=L, groups=K, assigned=Na, other_cells=int(c[:, :, 4].sum()),
               within_pairs=sum(x * (x - 1) // 2 for x in n), between_pairs=sum(n[g] * n[h] for g in range(K) for h in range(g + 1, K)),
               within_differences=sum(int(between[g, g]) for g in range(K)),
               between_differences=sum(int(between[g, h]) for g in range(K) for h in range(g + 1, K)),
               between=between, fixed=fixed, site_within=site_within, site_total=site_total, counts=c[:, :, :4].astype(np.uint32))

    def per(d, p):
        return d / p / L if p and L else 0.0
    out["pi_within"] = per(out["within_differences"], out["within_pairs"])
    out["pi_between"] = per(out["between_differences"], out["between_pairs"])
    out["fst"] = 1.0 - out["pi_within"] / out["pi_between"] if out["pi_between"] != 0.0 else 0.0
    return out


def genes(acc, group_of, group_size):
    """acc: (N, G) 0/1 in output order -> dict of gene_counts (G, K), acc_between, gene_fixed (K, K), gene_private (K)"""
    K, G = len(group_size), acc.shape[1]
    n = [int(x) for x in group_size]
    gc = np.zeros((G, K), np.int64)
    for g in range(K):
        gc[:, g] = (acc[group_of == g] != 0).sum(0)
    acc_between, gene_fixed = np.zeros((K, K), np.uint64), np.zeros((K, K), np.uint64)
    for g in range(K):
        for h in range(K):
            if g == h:
                acc_between[g, g] = int((gc[:, g] * (n[g] - gc[:, g])).sum())
            else:
                acc_between[g, h] = int((gc[:, g] * (n[h] - gc[:, h]) + (n[g] - gc[:, g]) * gc[:, h]).sum())
                gene_fixed[g, h] = int(((gc[:, g] == n[g]) & (gc[:, h] == 0)).sum())
    carriers = (gc > 0).sum(1)
    gene_private = np.array([int(((gc[:, g] > 0) & (carriers == 1)).sum()) for g in range(K)], np.uint64)
    return dict(genes=G, gene_counts=gc.astype(np.uint32), acc_between=acc_between, gene_fixed=gene_fixed, gene_private=gene_private)


def differentiation(core, labels, acc=None, max_groups=16, min_size=1):
    """everything `Population.group_differentiation(labels, acc, ..., per_site=True, counts=True)` returns"""
    group_of, group_label, group_size = groups(labels, max_groups, min_size)
    out = from_class_counts(class_counts(core, group_of, len(group_size)), group_size)
    out.update(pop_size=core.shape[0], unassigned=core.shape[0] - out["assigned"], group_of=group_of, group_label=group_label,
               group_size=group_size, genes=0)
    if acc is not None:
        out.update(genes(acc, group_of, group_size))
    return out


INTEGERS = ("sites", "groups", "assigned", "other_cells", "within_pairs", "between_pairs", "within_differences", "between_differences")
DOUBLES = ("pi_within", "pi_between", "fst")


def assert_equal(got, want, skip=()):
    """every field of `want` (a dict of this module) against the library's GroupDifferentiation: integers and arrays equal,
    the doubles equal as well -- both sides form them from the same integers in the same order of operations"""
    for name in INTEGERS + tuple(k for k in ("pop_size", "unassigned", "genes") if k in want):
        assert getattr(got, name) == want[name], (name, getattr(got, name), want[name])
    for name in DOUBLES:
        assert getattr(got, name) == want[name], (name, getattr(got, name), want[name])
    for name in ("group_of", "group_label", "group_size", "between", "fixed", "site_within", "site_total", "counts", "gene_counts",
                 "acc_between", "gene_fixed", "gene_private"):
        if name in want and name not in skip:
            have = getattr(got, name)
            assert have is not None and have.shape == want[name].shape and np.array_equal(have, want[name]), name
