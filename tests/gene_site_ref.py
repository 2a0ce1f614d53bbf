"""Gene-site association in plain Python integers: an independent restatement of docs/GENE_SITE_ASSOCIATION.md, the yardstick
of tests/test_gene_site_ld.py and tests/test_gpu_gene_site_ld.py.  Nothing here is fast and nothing is shared with the library:
indicators, the selection of each side and q of a pair come from tests/ld_ref.py, n11 from a brute-force product, the best tags
from a plain scan in column order that replaces the best only on a strictly larger q."""
import numpy as np

from ld_ref import acc_indicators, core_indicators, pair_q, select  # noqa: F401

NONE = 0xFFFFFFFF
FIELDS = ("pop_size", "site_columns", "gene_columns", "site_candidates", "gene_candidates", "sites", "genes", "pairs", "defined_pairs",
          "undefined_pairs", "four_gamete_pairs", "complete_pairs", "positive_pairs", "negative_pairs", "strong_pairs", "genes_tagged",
          "sites_tagging", "sum_q", "mean_r2", "r2_bins", "freq_bins", "site_min_minor", "gene_min_minor", "max_sites", "max_genes", "strong_q")
SIDE = ("index", "count", "best", "best_q", "best_sign", "strong")


def from_counts(site_index, site_count, gene_index, gene_count, n11, N, r2_bins=64, freq_bins=1, strong_q=32768, **head):
    """n11: a callable (gene position, site position) -> n11.  -> dict of the fields, `hist` (freq_bins x r2_bins), `freq_sum_q`
    and the twelve per-side arrays; `head`: the fields a device call adds (columns, candidates, minors, caps)"""
    Ms, Mg = len(site_index), len(gene_index)
    o = dict.fromkeys(FIELDS, 0)
    o.update(pop_size=N, sites=Ms, genes=Mg, pairs=Ms * Mg, r2_bins=r2_bins, freq_bins=freq_bins, strong_q=strong_q, site_min_minor=1,
             gene_min_minor=1, max_sites=1, max_genes=1)
    o.update(head)
    hist = np.zeros((freq_bins, r2_bins), np.uint64)
    freq_sum = [0] * freq_bins
    gene = dict(best=[NONE] * Mg, best_q=[0] * Mg, best_sign=[0] * Mg, strong=[0] * Mg)
    site = dict(best=[NONE] * Ms, best_q=[0] * Ms, best_sign=[0] * Ms, strong=[0] * Ms)
    for a in range(Mg):
        cg = int(gene_count[a])
        for b in range(Ms):
            cs = int(site_count[b])
            if cg in (0, N) or cs in (0, N):
                o["undefined_pairs"] += 1
                continue
            n = int(n11(a, b))
            D, q = pair_q(N, cg, cs, n)
            assert 0 <= q <= 65536
            sign = (D > 0) - (D < 0)
            r2 = min(r2_bins - 1, (q * r2_bins) >> 16)
            fb = min(freq_bins - 1, (2 * min(cg, N - cg) * freq_bins) // N)
            hist[fb, r2] += 1
            freq_sum[fb] += q
            o["defined_pairs"] += 1
            o["sum_q"] += q
            o["complete_pairs"] += q == 65536
            o["positive_pairs"] += D > 0
            o["negative_pairs"] += D < 0
            o["four_gamete_pairs"] += n > 0 and cg - n > 0 and cs - n > 0 and N - cg - cs + n > 0
            strong = q >= strong_q
            o["strong_pairs"] += strong
            gene["strong"][a] += strong
            site["strong"][b] += strong
            # (both scans meet their partners in ascending column order: only a strictly larger q replaces the best)
            for side, me, other in ((gene, a, int(site_index[b])), (site, b, int(gene_index[a]))):
                if side["best"][me] == NONE or q > side["best_q"][me]:
                    side["best"][me], side["best_q"][me], side["best_sign"][me] = other, q, sign
    o["genes_tagged"] = sum(1 for a in range(Mg) if gene["best"][a] != NONE and gene["best_q"][a] >= strong_q)
    o["sites_tagging"] = sum(1 for b in range(Ms) if site["best"][b] != NONE and site["best_q"][b] >= strong_q)
    o["mean_r2"] = float(np.float64(o["sum_q"]) / np.float64(65536.0) / np.float64(o["defined_pairs"])) if o["defined_pairs"] else 0.0
    o["hist"], o["freq_sum_q"] = hist, np.array(freq_sum, np.uint64)
    for name, side, index, count, other in (("site", site, site_index, site_count, "gene"), ("gene", gene, gene_index, gene_count, "site")):
        o[name + "_index"], o[name + "_count"] = np.array(index, np.uint32).reshape(-1), np.array(count, np.uint32).reshape(-1)
        o["%s_best_%s" % (name, other)] = np.array(side["best"], np.uint32)
        o[name + "_best_q"], o[name + "_strong"] = np.array(side["best_q"], np.uint32), np.array(side["strong"], np.uint32)
        o[name + "_best_sign"] = np.array(side["best_sign"], np.int32)
    return o


def _side(X, min_minor, cap, explicit):
    """X: (columns, N) indicators -> (columns of the list, their ones, candidates)"""
    N = X.shape[1]
    ones = X.sum(1, dtype=np.int64)
    if explicit is None:
        index, C = select(ones, N, min_minor, cap)
    else:
        index = [int(s) for s in explicit]
        C = sum(0 < ones[s] < N for s in index)
    return index, [int(ones[s]) for s in index], C


def gene_site(Xs, Xg, r2_bins=64, freq_bins=1, site_min_minor=1, gene_min_minor=1, max_sites=4096, max_genes=4096, strong_q=32768, sites=None,
              genes=None):
    """Xs: (sites, N) and Xg: (genes, N) indicators -> the result of ps_gene_site_ld; n11 by brute force"""
    Xs, Xg = np.asarray(Xs, np.uint8), np.asarray(Xg, np.uint8)
    N = Xs.shape[1]
    si, sc, Cs = _side(Xs, site_min_minor, max_sites, sites)
    gi, gc, Cg = _side(Xg, gene_min_minor, max_genes, genes)
    S = Xs[si].astype(np.int64) if si else np.zeros((0, N), np.int64)
    G = Xg[gi].astype(np.int64) if gi else np.zeros((0, N), np.int64)
    n11 = G @ S.T
    return from_counts(si, sc, gi, gc, lambda a, b: n11[a, b], N, r2_bins, freq_bins, strong_q, site_columns=Xs.shape[0],
                       gene_columns=Xg.shape[0], site_candidates=Cs, gene_candidates=Cg, site_min_minor=site_min_minor,
                       gene_min_minor=gene_min_minor, max_sites=max_sites, max_genes=max_genes)


def assert_equal(got, want, arrays=True):
    """got: a pansim_amd GeneSiteLd; every integer equal, mean_r2 bit-equal"""
    for f in FIELDS:
        g, w = getattr(got, f), want[f]
        if f == "mean_r2":
            assert np.float64(g).tobytes() == np.float64(w).tobytes(), (f, g, w)
        else:
            assert g == w, (f, g, w)
    assert np.array_equal(got.hist, want["hist"])
    assert np.array_equal(got.freq_sum_q, want["freq_sum_q"])
    for side, other in (("site", "gene"), ("gene", "site")):
        for name in ("index", "count") if arrays else ():
            assert np.array_equal(getattr(got, "%s_%s" % (side, name)), want["%s_%s" % (side, name)]), (side, name)
        for name in ("best_" + other, "best_q", "best_sign", "strong"):
            g, w = getattr(got, "%s_%s" % (side, name)), want["%s_%s" % (side, name)]
            assert np.array_equal(g, w), (side, name, g, w)
