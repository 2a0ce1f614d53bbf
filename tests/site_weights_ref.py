"""Per-site rate weights: an independent restatement in plain Python / numpy, written from DESIGN.md section 3.6.

Two things live here (test infrastructure; nothing below imports pansim_amd):

* the KEYED DENSE FORM the device runs -- the host tables (`core_tables`, `acc_tables`) and the operators on
  individual-major u8 matrices (`core_mutate`, `core_recombine`, `acc_mutate`, `acc_hgt`), bit for bit what the kernels
  must produce;
* the EVENT-DRIVEN algorithm of the reference with a sequential generator (`event_mutate_core`, `event_mutate_acc`,
  `event_hgt`: a Poisson count per row and a weighted index per event, population.rs:476-540 and :594-680) -- the
  distributional yardstick of the dense form.

Philox4x32-10 is restated here in numpy (vectorised); tests compare it with the C oracle's (`oracle.philox`).
"""
import math

import numpy as np

STREAM_CORE_L1, STREAM_CORE_L2, STREAM_ACC_MUT, STREAM_HGT, STREAM_CORE_L1B, STREAM_HGT_COUNT = 1, 2, 3, 4, 5, 21
U32 = 4294967296.0
M32 = np.uint64(0xFFFFFFFF)


# ----------------------------------------------------------------------------- generator
def philox(c0, c1, c2, c3, seed):
    """Philox4x32-10 on arrays of counters (broadcast), key = the 64-bit seed; returns the four output words"""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, np.uint64) for c in (c0, c1, c2, c3)])
    c0, c1, c2, c3 = c0 & M32, c1 & M32, c2 & M32, c3 & M32
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def mulhi(a, b):
    return (np.asarray(a, np.uint64) * np.asarray(b, np.uint64)) >> np.uint64(32)


def prob_to_u32(p):
    x = math.floor(p * U32)
    if not x > 0.0:
        return 0
    return 0xFFFFFFFF if x >= 4294967295.0 else int(x)


def _seq_sum(w):
    """left-to-right f64 sum"""
    w = np.asarray(w, np.float64)
    return float(np.cumsum(w)[-1]) if w.size else 0.0


def site_rates(lam, w):
    """r[s] = sum_c lam_c w_c[s] / W_c in f64, compartments in order, a compartment of rate 0 skipped"""
    w = np.asarray(w, np.float32).reshape(len(lam), -1)
    r = np.zeros(w.shape[1], np.float64)
    for c, l in enumerate(lam):
        if l > 0.0:
            r = r + float(l) * w[c].astype(np.float64) / _seq_sum(w[c])
    return r


# ----------------------------------------------------------------------------- tables
def _cell_law(p, q):
    a, b, c = p * (1.0 - q) / 3.0, p * q / 3.0, (1.0 - p) * q
    return a, b, c


def core_tables(lam_mut, lam_rec, w_mut):
    """(R, cshift, T): k = 0; R from the envelope of the per-site event mass; T[s] = seven cumulative thresholds of site s"""
    w_mut = np.asarray(w_mut, np.float32).reshape(len(lam_mut), -1)
    L = w_mut.shape[1]
    lam_hr = 0.0
    for l in lam_rec:
        lam_hr += float(l)
    q = -math.expm1(-lam_hr / L) if lam_hr > 0.0 else 0.0
    r = site_rates(lam_mut, w_mut)
    ps = [(-math.expm1(-x) if x > 0.0 else 0.0) for x in r.tolist()]
    m_max = 0.0
    for p in ps:
        a, b, c = _cell_law(p, q)
        m_max = max(m_max, a + a + a + b + b + b + c)
    R = min(64, int(math.ceil(m_max * 64.0)))
    scale = 64.0 / R if R else 0.0
    T = np.zeros((L, 7), np.uint32)
    for s, p in enumerate(ps):
        a, b, c = _cell_law(p, q)
        cum = [a, a + a, a + a + a, a + a + a + b, a + a + a + b + b, a + a + a + b + b + b, a + a + a + b + b + b + c]
        prev = 0
        for j in range(7):
            prev = max(prev, prob_to_u32(cum[j] * scale))
            T[s, j] = prev
    if L == 0 or int(T[:, 6].max()) == 0:
        R = 0
    cshift = 0
    while cshift < 4 and R > (4 << cshift):
        cshift += 1
    return R, cshift, T


def acc_tables(lam_mut, w_mut, w_rec):
    """(flip thresholds per gene, quantised HGT weights per compartment and gene)"""
    r = site_rates(lam_mut, w_mut)
    flip = np.array([prob_to_u32(-math.expm1(-2.0 * x) / 2.0) if x > 0.0 else 0 for x in r.tolist()], np.uint32)
    w_rec = np.asarray(w_rec, np.float32).reshape(len(lam_mut), -1)
    wq = np.zeros(w_rec.shape, np.uint16)
    for c in range(w_rec.shape[0]):
        w = w_rec[c].astype(np.float64)
        wmax = float(w.max()) if w.size else 0.0
        if wmax > 0.0:
            x = np.floor(w / wmax * 65535.0 + 0.5)
            wq[c] = np.where(w > 0.0, np.maximum(x, 1.0), 0.0).astype(np.uint16)
    return flip, wq


# ----------------------------------------------------------------------------- core operators
def _core_events(N, sites, seed, gen, R, T_rows):
    """the residual cells of the given GLOBAL sites with an event: (row index into sites, individual, mut allele, hr, donor)"""
    sites = np.asarray(sites, np.uint64)
    i = np.arange(N, dtype=np.uint64)
    S, I = sites[:, None], i[None, :]
    A = philox(S >> np.uint64(1), I >> np.uint64(4), gen, STREAM_CORE_L1, seed)
    B = philox(S >> np.uint64(2), I >> np.uint64(4), gen, STREAM_CORE_L1B, seed)
    pos = np.uint64(8) * (I & np.uint64(3)) + ((I >> np.uint64(2)) & np.uint64(3)) + np.uint64(4) * (S & np.uint64(1))
    one = np.uint64(1)
    n = sum((((A[k] >> pos) & one) << np.uint64(k)) for k in range(4))
    hi = (S & np.uint64(2)) != 0
    p4, p5 = np.where(hi, B[1], B[0]), np.where(hi, B[3], B[2])
    sym = np.uint64(4) * n + ((p4 >> pos) & one) + (((p5 >> pos) & one) << one)
    rs, ri = np.nonzero(sym < np.uint64(R))               # k = 0: the R lowest symbols are residual
    l2 = philox(sites[rs], ri, gen, STREAM_CORE_L2, seed)
    u = l2[0]
    T = np.asarray(T_rows, np.uint64)[rs]
    mut = np.zeros(len(rs), np.uint8)
    lo = u < T[:, 2]
    mid = (~lo) & (u < T[:, 5])
    mut[lo] = np.where(u[lo] < T[lo, 0], 2, np.where(u[lo] < T[lo, 1], 4, 8))
    mut[mid] = np.where(u[mid] < T[mid, 3], 2, np.where(u[mid] < T[mid, 4], 4, 8))
    hr = (~lo) & (u < T[:, 6])
    donor = mulhi(l2[1], max(N - 1, 0))
    donor = donor + (donor >= ri.astype(np.uint64))
    return rs, ri, mut, hr, donor.astype(np.int64)


def core_mutate(pop, site_offset, seed, gen, R, T, cols=None):
    """ps_mutate_alleles on pop (N x L_local); T = the table rows of the local columns; cols = only these local columns"""
    N = pop.shape[0]
    cols = np.arange(pop.shape[1]) if cols is None else np.asarray(cols)
    rs, ri, mut, _, _ = _core_events(N, cols + site_offset, seed, gen, R, np.asarray(T)[cols])
    m = mut > 0
    pop[ri[m], cols[rs[m]]] = mut[m]
    return pop


def core_recombine(pop, site_offset, seed, gen, R, T, cols=None):
    """ps_recombine: every receiving cell takes its donor's allele at the same site from the state before the call"""
    N = pop.shape[0]
    cols = np.arange(pop.shape[1]) if cols is None else np.asarray(cols)
    rs, ri, _, hr, donor = _core_events(N, cols + site_offset, seed, gen, R, np.asarray(T)[cols])
    snap = pop.copy()
    pop[ri[hr], cols[rs[hr]]] = snap[donor[hr], cols[rs[hr]]]
    return pop


# ----------------------------------------------------------------------------- accessory operators
def acc_mutate(pop, seed, gen, flip):
    """cell (i, g) flips iff word g mod 4 of Philox(g / 4, i, gen, 3) is below the gene's threshold"""
    N, G = pop.shape
    g = np.arange(G, dtype=np.uint64)
    words = philox((g >> np.uint64(2))[None, :], np.arange(N, dtype=np.uint64)[:, None], gen, STREAM_ACC_MUT, seed)
    sel = (g & np.uint64(3))[None, :]
    w = np.where(sel == 0, words[0], np.where(sel == 1, words[1], np.where(sel == 2, words[2], words[3])))
    pop ^= (w < np.asarray(flip, np.uint64)[None, :]).astype(np.uint8)
    return pop


def acc_hgt(pop, seed, gen, lam_rec, wq, poisson_table, donors=None):
    """ps_recombine on the accessory matrix under per-gene weights; `poisson_table(lam)` -> (kmin, thresholds) is the
    oracle's integer Poisson inversion table.  donors: only these donors send (a donor shard).  Returns the event count."""
    N, G = pop.shape
    snap = pop.copy()
    donors = range(N) if donors is None else donors
    events = 0
    for c, lam in enumerate(lam_rec):
        if not lam > 0.0 or N < 2:
            continue
        kmin, thr = poisson_table(lam)
        w = np.asarray(wq[c], np.uint64)
        for dn in donors:
            u = int(philox(dn, 0, gen, STREAM_HGT_COUNT | (c << 8), seed)[0])
            k = kmin + min(int(np.searchsorted(thr, u, side="right")), len(thr) - 1)
            present = np.nonzero((snap[dn] != 0) & (w > 0))[0]
            if k == 0 or present.size == 0:
                continue
            pref = np.cumsum(w[present])
            j = np.arange(k, dtype=np.uint64)
            r = philox(j >> np.uint64(1), dn, gen, STREAM_HGT | (c << 8), seed)
            odd = (j & np.uint64(1)) != 0
            wr, wg = np.where(odd, r[2], r[0]), np.where(odd, r[3], r[1])
            rc = mulhi(wr, N - 1)
            rc = rc + (rc >= np.uint64(dn))
            gene = present[np.searchsorted(pref, mulhi(wg, pref[-1]), side="right")]
            pop[rc.astype(np.int64), gene] = 1
            events += k
    return events


# ----------------------------------------------------------------------------- the reference's event-driven algorithm
def event_mutate_core(pop, rng, lam_mut, w_mut):
    """population.rs:511-540: per compartment and row, Poisson(lam) events, site from weighted_dist[c], value from [2, 4, 8]
    (the `core_vec[1 >> value]` quirk of :531 always lands there)"""
    w_mut = np.asarray(w_mut, np.float64).reshape(len(lam_mut), -1)
    for c, lam in enumerate(lam_mut):
        if not lam > 0.0:
            continue
        pr = w_mut[c] / w_mut[c].sum()
        for i in range(pop.shape[0]):
            k = rng.poisson(lam)
            sites = rng.choice(pr.size, size=k, p=pr)
            vals = rng.choice(np.array([2, 4, 8], np.uint8), size=k)
            for s, v in zip(sites, vals):
                pop[i, s] = v
    return pop


def event_mutate_acc(pop, rng, lam_mut, w_mut):
    """population.rs:486-510: the same with a toggle of the drawn gene"""
    w_mut = np.asarray(w_mut, np.float64).reshape(len(lam_mut), -1)
    for c, lam in enumerate(lam_mut):
        if not lam > 0.0:
            continue
        pr = w_mut[c] / w_mut[c].sum()
        for i in range(pop.shape[0]):
            for g in rng.choice(pr.size, size=rng.poisson(lam), p=pr):
                pop[i, g] ^= 1
    return pop


def event_hgt(pop, rng, lam_rec, w_rec):
    """population.rs:594-680: per compartment and donor Poisson(lam) events, a recipient among the others, the gene drawn from
    locus_weights[c] over the donor's present genes (none qualifies: no event, :672); recipients gain the gene"""
    w_rec = np.asarray(w_rec, np.float64).reshape(len(lam_rec), -1)
    N = pop.shape[0]
    snap = pop.copy()
    picks = []
    for c, lam in enumerate(lam_rec):
        if not lam > 0.0:
            continue
        for dn in range(N):
            k = rng.poisson(lam)
            wt = w_rec[c] * (snap[dn] != 0)
            if k == 0 or not wt.sum() > 0.0:
                continue
            genes = rng.choice(wt.size, size=k, p=wt / wt.sum())
            rc = rng.integers(0, N - 1, size=k)
            rc = rc + (rc >= dn)
            pop[rc, genes] = 1
            picks.append((c, dn, genes))
    return pop, picks
