"""A plain numpy restatement of docs/CORE_DIVERSITY.md, independent of the library: per-site base counts of an
individual-major core matrix, the five classes A, C, G, T, other, the minor-count spectrum, the integers and the double of
ps_core_diversity_t (the double by the expression in the header's struct comment).  Integers are Python ints."""
import numpy as np

BASES = (1, 2, 4, 8)
INT_FIELDS = ("pop_size", "sites", "other_cells", "segregating_sites", "pair_differences")


def site_counts(M):
    """(N, L) u8 -> (L, 4) uint32: cells of every column equal to 1, 2, 4, 8"""
    M = np.asarray(M, np.uint8)
    return np.stack([(M == b).sum(0) for b in BASES], axis=1).astype(np.uint32).reshape(M.shape[1], 4)


def summary(counts, pop_size):
    """the dict of Population.core_diversity(spectrum=True) from a (sites, 4) table"""
    counts = np.asarray(counts).reshape(-1, 4)
    N = int(pop_size)
    sites = counts.shape[0]
    spectrum = np.zeros(N + 1, np.uint64)
    pair = seg = other = 0
    for row in counts.tolist():
        o = N - sum(row)
        assert o >= 0
        classes = row + [o]
        pair += (N * N - sum(c * c for c in classes)) // 2
        seg += sum(1 for c in classes if c) >= 2
        other += o
        spectrum[N - max(classes)] += 1
    mean = 0.0
    if N >= 2 and sites:
        mean = float(pair) / float(N * (N - 1) // 2) / float(sites)
    return dict(pop_size=N, sites=sites, other_cells=other, segregating_sites=seg, pair_differences=pair,
                base_cells=[int(x) for x in counts.astype(np.uint64).sum(0)] if sites else [0, 0, 0, 0],
                mean_pairwise_distance=mean, spectrum=spectrum)


def of_matrix(M):
    M = np.asarray(M, np.uint8)
    return summary(site_counts(M), M.shape[0])


def same(got, want):
    """integers and spectrum equal, the double bit for bit; returns the name of the first field that differs, or None"""
    for k in INT_FIELDS + ("base_cells",):
        if got[k] != want[k]:
            return k
    if np.float64(got["mean_pairwise_distance"]).tobytes() != np.float64(want["mean_pairwise_distance"]).tobytes():
        return "mean_pairwise_distance"
    if "spectrum" in want and "spectrum" in got and not np.array_equal(got["spectrum"], want["spectrum"]):
        return "spectrum"
    return None


def add(parts):
    """the sum of shard summaries: every integer and the spectrum add; the double is formed once over all sites"""
    N = parts[0]["pop_size"]
    out = dict(pop_size=N, sites=0, other_cells=0, segregating_sites=0, pair_differences=0, base_cells=[0, 0, 0, 0],
               spectrum=np.zeros(N + 1, np.uint64))
    for p in parts:
        for k in INT_FIELDS[1:]:
            out[k] += p[k]
        out["base_cells"] = [a + b for a, b in zip(out["base_cells"], p["base_cells"])]
        out["spectrum"] += p["spectrum"]
    out["mean_pairwise_distance"] = 0.0
    if N >= 2 and out["sites"]:
        out["mean_pairwise_distance"] = float(out["pair_differences"]) / float(N * (N - 1) // 2) / float(out["sites"])
    return out
