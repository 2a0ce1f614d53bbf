"""Linkage disequilibrium between loci in plain Python integers: an independent restatement of docs/LINKAGE_DISEQUILIBRIUM.md,
the yardstick of tests/test_locus_ld.py and tests/test_gpu_locus_ld.py.  Nothing here is fast and nothing is shared with the
library: indicators from matrices, the selection of loci, q of a pair through (D * D << 16) // den."""
import numpy as np

BASES = (1, 2, 4, 8)
FIELDS = ("pop_size", "columns", "candidates", "loci", "pairs", "defined_pairs", "undefined_pairs", "four_gamete_pairs", "complete_pairs",
          "positive_pairs", "negative_pairs", "sum_q", "mean_r2", "r2_bins", "lag_bins", "min_minor", "max_loci")


def core_indicators(core):
    """(N, L) bytes -> (L, N) 0 / 1: the cell equals the site's major base (the largest count of 1, 2, 4, 8; ties to the lowest
    byte); any other byte is in no class"""
    core = np.asarray(core, np.uint8)
    counts = np.stack([(core == b).sum(0) for b in BASES])          # (4, L)
    major = np.array(BASES, np.uint8)[np.argmax(counts, axis=0)]    # (argmax: the first of equal maxima = the lowest byte)
    return np.ascontiguousarray((core == major[None, :]).T.astype(np.uint8))


def acc_indicators(acc):
    return np.ascontiguousarray((np.asarray(acc) != 0).T.astype(np.uint8))


def select(ones, N, min_minor, max_loci):
    """-> (list of columns, candidates)"""
    cand = [s for s, c in enumerate(ones) if min(int(c), N - int(c)) >= min_minor]
    C = len(cand)
    if C <= max_loci:
        return cand, C
    return [cand[(j * C) // max_loci] for j in range(max_loci)], C


def pair_q(N, ca, cb, n11):
    D = N * n11 - ca * cb
    den = ca * (N - ca) * cb * (N - cb)
    return D, (D * D << 16) // den


def from_counts(index, count, n11, N, r2_bins, lag_bins, columns=0, candidates=0, min_minor=1, max_loci=1):
    """index, count: M loci; n11: a callable (a, b) -> n11 of positions a < b.  -> dict of the fields, `hist` (lag_bins x
    r2_bins) and `lag_sum_q`"""
    M = len(index)
    o = dict.fromkeys(FIELDS, 0)
    o.update(pop_size=N, columns=columns, candidates=candidates, loci=M, pairs=M * (M - 1) // 2, r2_bins=r2_bins, lag_bins=lag_bins,
             min_minor=min_minor, max_loci=max_loci)
    hist = np.zeros((lag_bins, r2_bins), np.uint64)
    lag_sum = [0] * lag_bins
    for a in range(M):
        ca = int(count[a])
        for b in range(a + 1, M):
            cb = int(count[b])
            if ca in (0, N) or cb in (0, N):
                o["undefined_pairs"] += 1
                continue
            n = int(n11(a, b))
            D, q = pair_q(N, ca, cb, n)
            assert 0 <= q <= 65536
            r2 = min(r2_bins - 1, (q * r2_bins) >> 16)
            lag = min(lag_bins - 1, (int(index[b]) - int(index[a])).bit_length() - 1)
            hist[lag, r2] += 1
            lag_sum[lag] += q
            o["defined_pairs"] += 1
            o["sum_q"] += q
            o["complete_pairs"] += q == 65536
            o["positive_pairs"] += D > 0
            o["negative_pairs"] += D < 0
            o["four_gamete_pairs"] += n > 0 and ca - n > 0 and cb - n > 0 and N - ca - cb + n > 0
    o["mean_r2"] = float(np.float64(o["sum_q"]) / np.float64(65536.0) / np.float64(o["defined_pairs"])) if o["defined_pairs"] else 0.0
    o["hist"], o["lag_sum_q"] = hist, np.array(lag_sum, np.uint64)
    return o


def locus_ld(X, r2_bins=64, lag_bins=1, min_minor=1, max_loci=4096, loci=None):
    """X: (columns, N) indicators -> the result of ps_locus_ld, with `locus_index` and `locus_count`"""
    X = np.asarray(X, np.uint8)
    cols, N = X.shape
    ones = X.sum(1, dtype=np.int64)
    if loci is None:
        index, C = select(ones, N, min_minor, max_loci)
    else:
        index = [int(s) for s in loci]
        C = sum(0 < ones[s] < N for s in index)
    count = [int(ones[s]) for s in index]
    S = X[index].astype(np.int64) if index else np.zeros((0, N), np.int64)
    n11 = S @ S.T
    o = from_counts(index, count, lambda a, b: n11[a, b], N, r2_bins, lag_bins, cols, C, min_minor, max_loci)
    o["locus_index"], o["locus_count"] = np.array(index, np.uint32), np.array(count, np.uint32)
    return o


def assert_equal(got, want, arrays=True):
    """got: a pansim_amd LocusLd; every integer equal, mean_r2 bit-equal"""
    for f in FIELDS:
        g, w = getattr(got, f), want[f]
        if f == "mean_r2":
            assert np.float64(g).tobytes() == np.float64(w).tobytes(), (f, g, w)
        else:
            assert g == w, (f, g, w)
    assert np.array_equal(got.hist, want["hist"])
    assert np.array_equal(got.lag_sum_q, want["lag_sum_q"])
    if arrays:
        assert np.array_equal(got.locus_index, want["locus_index"])
        assert np.array_equal(got.locus_count, want["locus_count"])
