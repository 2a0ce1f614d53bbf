// locus_ld.h -- ps_locus_ld / ps_sim_locus_ld / ps_multi_locus_ld, the host restatements ps_ld_select_loci and ps_ld_from_counts
// and ps_locus_ld_timing (include/pansim_hip.h; the definitions: docs/LINKAGE_DISEQUILIBRIUM.md).  Included by pansim_capi.hip
// behind the all-pairs read-outs.
//
// The statistics are sums over pairs of COLUMNS and do not depend on the order of the individuals: no row map of DESIGN.md 3.5
// is involved, everything runs in internal order on the handle's own stream -- behind every queued generation, a two-generation
// sweep launch included (the sweeps swap state / state2 on the host when they are enqueued).
// One routine serves every entry: a list of `parts` (one handle; or the core handles of the shards of a run, which hold disjoint
// runs of the sites in order).  Every part counts, selects and packs its own columns into bit rows at their positions in the
// list; the parts' rows are ORed on part 0, where the contraction (acc_intersections_launch) and ld_pair_kernel run per band.
#pragma once

#include "ld_kernels.h"

#define PS_LD_MAX_BINS 16384u      // 64 KB of u32 bins in LDS per workgroup
#define PS_LD_MAX_POP 65536u       // u16 n11: N - 1 <= 65535

static int ld_check_params(const ps_ld_params *prm, bool automatic)
{
    if (prm->r2_bins < 1) return ps_fail(PS_ERR_INVALID, "r2_bins must be >= 1");
    if (prm->lag_bins < 1 || prm->lag_bins > PS_LD_MAX_LAGS)
        return ps_fail(PS_ERR_INVALID, "lag_bins must be 1 .. %u, not %u", PS_LD_MAX_LAGS, prm->lag_bins);
    if ((uint64_t)prm->r2_bins * prm->lag_bins > PS_LD_MAX_BINS)
        return ps_fail(PS_ERR_INVALID, "r2_bins x lag_bins = %llu exceeds the limit of %u bins (64 KB of LDS per workgroup)",
                       (unsigned long long)prm->r2_bins * prm->lag_bins, PS_LD_MAX_BINS);
    if (automatic) {
        if (prm->min_minor < 1) return ps_fail(PS_ERR_INVALID, "min_minor must be >= 1");
        if (prm->max_loci < 1 || prm->max_loci > PS_LD_MAX_LOCI)
            return ps_fail(PS_ERR_INVALID, "max_loci must be 1 .. %u, not %u", PS_LD_MAX_LOCI, prm->max_loci);
    }
    return PS_OK;
}

static int ld_check_pop(uint64_t N)
{
    if (N < 1 || N > PS_LD_MAX_POP)
        return ps_fail(PS_ERR_INVALID, "linkage disequilibrium needs 1 <= pop_size <= %u (u16 pair counts), not %llu", PS_LD_MAX_POP,
                       (unsigned long long)N);
    return PS_OK;
}

static int ld_check_list(const uint32_t *loci, uint64_t n, uint64_t columns)
{
    if (n > PS_LD_MAX_LOCI) return ps_fail(PS_ERR_INVALID, "a list of %llu loci exceeds the limit of %u", (unsigned long long)n, PS_LD_MAX_LOCI);
    for (uint64_t k = 0; k < n; k++) {
        if (columns && loci[k] >= columns)
            return ps_fail(PS_ERR_INVALID, "locus %llu: column %u is not below the %llu columns", (unsigned long long)k, loci[k],
                           (unsigned long long)columns);
        if (k && loci[k] <= loci[k - 1])
            return ps_fail(PS_ERR_INVALID, "locus %llu: the list must be strictly ascending (%u after %u)", (unsigned long long)k, loci[k], loci[k - 1]);
    }
    return PS_OK;
}

static void ld_fill(ps_ld_t *o, uint64_t N, uint64_t columns, uint64_t candidates, uint64_t M, const ps_ld_params *prm)
{
    memset(o, 0, sizeof *o);
    o->pop_size = N;
    o->columns = columns;
    o->candidates = candidates;
    o->loci = M;
    o->pairs = M * (M - (M ? 1 : 0)) / 2;
    o->r2_bins = prm->r2_bins;
    o->lag_bins = prm->lag_bins;
    o->min_minor = prm->min_minor;
    o->max_loci = prm->max_loci;
}

// the summary words, the bins and the lag sums in place -> the totals and the one double
static void ld_finish(ps_ld_t *o, const unsigned long long *w, const uint64_t *hist, const uint64_t *lag_sum_q)
{
    o->undefined_pairs = w[PS_LD_UNDEF];
    o->four_gamete_pairs = w[PS_LD_FOURG];
    o->complete_pairs = w[PS_LD_COMPLETE];
    o->positive_pairs = w[PS_LD_POS];
    o->negative_pairs = w[PS_LD_NEG];
    for (uint64_t b = 0; b < o->r2_bins * o->lag_bins; b++) o->defined_pairs += hist[b];
    for (uint64_t b = 0; b < o->lag_bins; b++) o->sum_q += lag_sum_q[b];
    o->mean_r2 = o->defined_pairs ? (double)o->sum_q / 65536.0 / (double)o->defined_pairs : 0.0;
}

extern "C" int ps_ld_select_loci(const uint32_t *ones, uint64_t columns, uint64_t pop_size, uint32_t min_minor, uint32_t max_loci,
                                 uint32_t *index, uint64_t *n_loci, uint64_t *candidates)
{
    if ((!ones && columns) || !index || !n_loci) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(ld_check_pop(pop_size));
    const ps_ld_params prm = { 1u, 1u, min_minor, max_loci };
    PSCHK(ld_check_params(&prm, true));
    if (columns > 0xffffffffull) return ps_fail(PS_ERR_INVALID, "at most 2^32 - 1 columns");
    uint64_t C = 0;
    for (uint64_t s = 0; s < columns; s++) {
        if (ones[s] > pop_size)
            return ps_fail(PS_ERR_INVALID, "column %llu: %u ones among %llu individuals", (unsigned long long)s, ones[s], (unsigned long long)pop_size);
        C += std::min<uint64_t>(ones[s], pop_size - ones[s]) >= min_minor ? 1 : 0;
    }
    const uint64_t M = std::min<uint64_t>(C, max_loci);
    uint64_t rank = 0, j = 0;
    for (uint64_t s = 0; s < columns && j < M; s++) {
        if (std::min<uint64_t>(ones[s], pop_size - ones[s]) < min_minor) continue;
        // (several j may not share a rank: C > max_loci makes the ranks strictly ascending)
        if (rank == (C <= max_loci ? j : j * C / max_loci)) index[j++] = (uint32_t)s;
        rank++;
    }
    *n_loci = M;
    if (candidates) *candidates = C;
    return PS_OK;
}

extern "C" int ps_ld_from_counts(const uint32_t *locus_index, const uint32_t *locus_count, const uint32_t *n11, uint64_t n_loci,
                                 uint64_t pop_size, const ps_ld_params *prm, ps_ld_t *out, uint64_t *hist, uint64_t *lag_sum_q)
{
    if (!prm || !out || !hist || !lag_sum_q || (n_loci && (!locus_index || !locus_count)) || (n_loci > 1 && !n11))
        return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(ld_check_params(prm, false));
    PSCHK(ld_check_pop(pop_size));
    PSCHK(ld_check_list(locus_index, n_loci, 0));
    const uint64_t M = n_loci;
    const uint32_t N = (uint32_t)pop_size;
    for (uint64_t a = 0; a < M; a++)
        if (locus_count[a] > N)
            return ps_fail(PS_ERR_INVALID, "locus %llu: %u ones among %u individuals", (unsigned long long)a, locus_count[a], N);
    const uint64_t nbins = (uint64_t)prm->r2_bins * prm->lag_bins;
    memset(hist, 0, nbins * sizeof(uint64_t));
    memset(lag_sum_q, 0, prm->lag_bins * sizeof(uint64_t));
    unsigned long long w[PS_LD_WORDS] = {};
    uint64_t k = 0;
    for (uint64_t a = 0; a < M; a++)
        for (uint64_t b = a + 1; b < M; b++, k++) {
            const uint32_t ca = locus_count[a], cb = locus_count[b], n = n11[k];
            if (n > std::min(ca, cb) || (uint64_t)ca + cb > (uint64_t)N + n)
                return ps_fail(PS_ERR_INVALID, "pair (%llu, %llu): n11 = %u does not fit the counts %u and %u of %u individuals",
                               (unsigned long long)a, (unsigned long long)b, n, ca, cb, N);
            if (ps_ld_monomorphic(ca, N) || ps_ld_monomorphic(cb, N)) {
                w[PS_LD_UNDEF]++;
                continue;
            }
            ps_ld_pair_t p;
            ps_ld_pair(N, ca, cb, n, locus_index[a], locus_index[b], prm->r2_bins, prm->lag_bins, &p);
            hist[(uint64_t)p.lag_bin * prm->r2_bins + p.r2_bin]++;
            lag_sum_q[p.lag_bin] += p.q;
            w[PS_LD_FOURG] += p.four;
            w[PS_LD_COMPLETE] += p.complete;
            w[PS_LD_POS] += p.sign > 0 ? 1 : 0;
            w[PS_LD_NEG] += p.sign < 0 ? 1 : 0;
        }
    ld_fill(out, pop_size, 0, 0, M, prm);
    ld_finish(out, w, hist, lag_sum_q);
    return PS_OK;
}

// The ones of every column of `p` and the inclusive prefix sums of its candidate flags, in its selection scratch on its stream; *C = its
// candidates (one u32 through the host: the stream is synchronised).  *d_incl is null for a handle without columns.
static int ld_count_candidates(ps_population *p, uint32_t min_minor, uint32_t **d_incl, uint64_t *C)
{
    const uint64_t ncols = p->cfg.ncols;
    const uint32_t N = (uint32_t)p->cfg.pop_size;
    const bool core = p->cfg.core != 0;
    *d_incl = nullptr;
    *C = 0;
    if (ncols == 0) return PS_OK;
    const uint64_t tiles = (ncols + 1023) / 1024;
    if (tiles > 256u * 64u)
        return ps_fail(PS_ERR_INVALID, "the automatic selection of loci scans at most 2^24 columns per handle, not %llu", (unsigned long long)ncols);
    const uint64_t n_cnt = (core ? 4 : 1) * ncols, n_cnt_pad = (n_cnt + 3) & ~3ull;
    readout_slot &sel = p->ro[PS_RO_LD_SEL];
    PSCHK(dev_grow(sel.d, sel.cap, (n_cnt_pad + ncols + tiles) * sizeof(uint32_t)));
    uint32_t *colcnt = (uint32_t *)sel.d, *flag = colcnt + n_cnt_pad, *tsum = flag + ncols;
    hipStream_t st = p->stream;
    if (core) {
        const uint32_t rows = (uint32_t)ncols, grid = std::max(1u, std::min((rows + 3u) / 4u, 256u * 8u));
        hipLaunchKernelGGL((core_site_counts_kernel<true, false>), dim3(grid), dim3(256), 0, st, (const uint8_t *)p->state, p->pitch, N, rows,
                           colcnt, (unsigned long long *)nullptr, (unsigned long long *)nullptr, 0u);
    } else {
        PSCHK(ensure_gene_major(p, st));
        acc_gene_counts_kernel<<<(uint32_t)((ncols + 255) / 256), 256, 0, st>>>(p->G[0], colcnt, p->d);
    }
    HIPCHK(hipGetLastError());
    ld_candidate_kernel<<<(uint32_t)((ncols + 255) / 256), 256, 0, st>>>(colcnt, core ? 1u : 0u, (uint32_t)ncols, N, min_minor, flag);
    idx_tile_sums_kernel<<<(uint32_t)tiles, 256, 0, st>>>(flag, (uint32_t)ncols, tsum);
    idx_tile_prefix_kernel<<<1, 256, 0, st>>>(tsum, (uint32_t)tiles);
    idx_scan_kernel<<<(uint32_t)tiles, 256, 0, st>>>(flag, (uint32_t)ncols, tsum);
    HIPCHK(hipGetLastError());
    uint32_t c = 0;
    HIPCHK(hipMemcpyAsync(&c, flag + ncols - 1, sizeof c, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *d_incl = flag;
    *C = c;
    return PS_OK;
}

// What the phases of ld_run share: the kind of the columns, the list (M loci of C candidates; `loci`: the caller's own list) and
// the sizes that follow from it
struct ld_geom {
    bool core = false;
    const uint32_t *loci = nullptr;         // (nullptr: the automatic selection)
    uint32_t N = 0, max_loci = 0, Mpad = 0, WP = 0, ldi = 0;
    uint64_t C = 0, M = 0, band = 0, n_words = 0, row_words = 0;
    size_t K = 1;
};

// the call's scratch on one part: sel | cnt | idx | rows; in front of them on part 0 the words, behind them the landing rows (with
// several parts) and one band of n11
struct ld_scratch {
    unsigned long long *words = nullptr;
    uint32_t *sel = nullptr, *cnt = nullptr, *idx = nullptr, *rows = nullptr, *land = nullptr;
    uint16_t *in = nullptr;
};

static int ld_scratch_get(ps_population *p, const ld_geom &g, bool first, ld_scratch *s)
{
    scratch_layout lay;
    const uint64_t o_words = lay.add(first ? g.n_words * 8 : 0, 8);
    const uint64_t o_sel = lay.add(g.Mpad * 4ull, 4), o_cnt = lay.add(g.Mpad * 4ull, 4), o_idx = lay.add(g.Mpad * 4ull, 4);
    const uint64_t o_rows = lay.add(g.row_words * 4, 4);
    const uint64_t o_land = lay.add(first && g.K > 1 ? g.row_words * 4 : 0, 4), o_in = lay.add(first ? g.band * g.ldi * 2 : 0, 2);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(p->ro[PS_RO_LD], lay.bytes, &base, nullptr));
    s->sel = (uint32_t *)(base + o_sel);
    s->cnt = (uint32_t *)(base + o_cnt);
    s->idx = (uint32_t *)(base + o_idx);
    s->rows = (uint32_t *)(base + o_rows);
    s->words = (unsigned long long *)(base + o_words);      // (the three of part 0 are empty on the others)
    s->land = (uint32_t *)(base + o_land);
    s->in = (uint16_t *)(base + o_in);
    return PS_OK;
}

// The list entries [j_lo, j_lo + rows_k) that part `p` holds: selected on its device, packed into bit rows at their positions in
// the list and counted, on its own stream (pad dwords, pad rows and monomorphic rows stay zero); their columns and counts in
// h_idx / h_cnt once the stream has been synchronised.  tm: part 0, whose select and pack are timed (groups 0 and 1).
static int ld_select_pack(ps_population *p, const ld_geom &g, const ld_scratch &s, event_timer *tm, const uint32_t *d_incl, uint64_t rank_lo,
                          uint32_t j_lo, uint32_t rows_k, uint32_t *h_idx, uint32_t *h_cnt)
{
    hipStream_t st = p->stream;
    std::vector<uint32_t> h_sel(rows_k);
    auto select = [&]() -> int {
        if (!rows_k) return PS_OK;
        if (!g.loci) {
            ld_select_kernel<<<(rows_k + 255u) / 256u, 256, 0, st>>>(d_incl, (uint32_t)p->cfg.ncols, g.C, rank_lo, j_lo, rows_k, g.max_loci, s.sel);
            HIPCHK(hipGetLastError());
        } else {
            for (uint32_t t = 0; t < rows_k; t++) h_sel[t] = (uint32_t)(g.loci[j_lo + t] - p->cfg.col_offset);
            HIPCHK(hipMemcpyAsync(s.sel, h_sel.data(), rows_k * 4ull, hipMemcpyHostToDevice, st));
        }
        return PS_OK;
    };
    auto pack = [&]() -> int {
        if (!rows_k) return PS_OK;
        if (g.core) {
            ld_pack_core_kernel<<<(rows_k + 3u) / 4u, 256, 0, st>>>((const uint8_t *)p->state, p->pitch, g.N, s.sel, rows_k, j_lo, g.WP, s.rows, s.cnt);
        } else {
            PSCHK(ensure_gene_major(p, st));
            ld_pack_acc_kernel<<<(rows_k + 3u) / 4u, 256, 0, st>>>(p->G[0], p->d, s.sel, rows_k, j_lo, g.WP, s.rows, s.cnt);
        }
        HIPCHK(hipGetLastError());
        return PS_OK;
    };
    HIPCHK(hipMemsetAsync(s.sel, 0, (3ull * g.Mpad + g.row_words) * 4, st));
    PSCHK(tm ? tm->timed(0, st, select) : select());
    PSCHK(tm ? tm->timed(1, st, pack) : pack());
    if (rows_k) {
        if (!g.loci) HIPCHK(hipMemcpyAsync(h_sel.data(), s.sel, rows_k * 4ull, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_cnt + j_lo, s.cnt + j_lo, rows_k * 4ull, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t t = 0; t < rows_k; t++) h_idx[j_lo + t] = (uint32_t)(h_sel[t] + p->cfg.col_offset);
    return PS_OK;
}

// The pair phase, queued on part 0's stream (the caller synchronises it): the other parts' rows join part 0's (their streams
// are idle), the whole list goes up, per band the contraction (group 2) and ld_pair_kernel (group 3), then the words, the lag
// sums and the bins come back.
static int ld_pair_phase(const std::vector<ps_population *> &parts, const ld_geom &g, const std::vector<ld_scratch> &S,
                         const std::vector<uint32_t> &j_cnt, event_timer &tm, const ps_ld_params *prm, const uint32_t *h_idx,
                         const uint32_t *h_cnt, unsigned long long *w, uint64_t *hist, uint64_t *lag_sum_q)
{
    ps_population *p0 = parts[0];
    hipStream_t s0 = p0->stream;
    const ld_scratch &s = S[0];
    const uint64_t nbins = (uint64_t)prm->r2_bins * prm->lag_bins;
    for (size_t k = 1; k < g.K; k++) {
        if (!j_cnt[k]) continue;
        PSCHK(tm.timed(1, s0, [&]() -> int {
            HIPCHK(hipMemcpyPeerAsync(s.land, p0->device, S[k].rows, parts[k]->device, g.row_words * 4, s0));
            ld_or_kernel<<<(uint32_t)((g.row_words + 255) / 256), 256, 0, s0>>>(s.rows, s.land, g.row_words);
            HIPCHK(hipGetLastError());
            return PS_OK;
        }));
    }
    HIPCHK(hipMemcpyAsync(s.idx, h_idx, g.M * 4, hipMemcpyHostToDevice, s0));
    if (g.K > 1) HIPCHK(hipMemcpyAsync(s.cnt, h_cnt, g.M * 4, hipMemcpyHostToDevice, s0));
    unsigned long long *d_lag = s.words + PS_LD_WORDS, *d_hist = d_lag + PS_LD_MAX_LAGS;
    const uint32_t Mu = (uint32_t)g.M, lds = (uint32_t)nbins * 4u;
    for (uint32_t lo = 0; lo + 1u < Mu; lo += (uint32_t)g.band) {
        const uint32_t nrows = std::min<uint32_t>((uint32_t)g.band, Mu - lo);
        dim3 grid;
        PSCHK(bin_grid((const void *)ld_pair_kernel, Mu, nrows, lds, 512u, &grid));
        PSCHK(tm.timed(2, s0, [&]() { return acc_intersections_launch(s.rows, g.WP, g.Mpad, g.ldi, 2u, lo, nrows, s.in, s0); }));
        PSCHK(tm.timed(3, s0, [&]() -> int {
            hipLaunchKernelGGL(ld_pair_kernel, grid, dim3(256), lds, s0, (const uint16_t *)s.in, g.ldi, (const uint32_t *)s.cnt,
                               (const uint32_t *)s.idx, g.N, Mu, lo, nrows, prm->r2_bins, prm->lag_bins, d_hist, d_lag, s.words);
            HIPCHK(hipGetLastError());
            return PS_OK;
        }));
    }
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the bins are copied as they are");
    HIPCHK(hipMemcpyAsync(w, s.words, PS_LD_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s0));
    HIPCHK(hipMemcpyAsync(lag_sum_q, d_lag, prm->lag_bins * sizeof(uint64_t), hipMemcpyDeviceToHost, s0));
    HIPCHK(hipMemcpyAsync(hist, d_hist, nbins * sizeof(uint64_t), hipMemcpyDeviceToHost, s0));
    return PS_OK;
}

// Everything queued on every part is complete or ordered on its own stream before this is called; parts[0] computes.
static int ld_run(const std::vector<ps_population *> &parts, uint64_t columns, const ps_ld_params *prm, const uint32_t *loci, uint32_t n_loci,
                  ps_ld_t *out, uint32_t *locus_index, uint32_t *locus_count, uint64_t *hist, uint64_t *lag_sum_q)
{
    ps_population *p0 = parts[0];
    const size_t K = parts.size();
    const bool automatic = loci == nullptr;
    const uint64_t N64 = p0->cfg.pop_size;
    PSCHK(ld_check_params(prm, automatic));
    PSCHK(ld_check_pop(N64));
    if (!automatic) PSCHK(ld_check_list(loci, n_loci, std::max<uint64_t>(columns, 1)));
    if (!automatic && n_loci && columns == 0) return ps_fail(PS_ERR_INVALID, "the handle has no columns to list");
    ld_geom g;
    g.core = p0->cfg.core != 0;
    g.loci = loci;
    g.N = (uint32_t)N64;
    g.max_loci = prm->max_loci;
    g.K = K;
    const uint64_t nbins = (uint64_t)prm->r2_bins * prm->lag_bins;
    // timer groups: 0 = counts and selection, 1 = packing, 2 = the contraction, 3 = the pair statistics
    event_timer tm;
    readout_slot &ro = p0->ro[PS_RO_LD];
    ro.timed = false;
    // the rows of the list every part holds: [j_lo, j_lo + j_cnt)
    std::vector<uint32_t> j_lo(K, 0), j_cnt(K, 0);
    std::vector<uint32_t *> d_incl(K, nullptr);
    std::vector<uint64_t> rank_lo(K + 1, 0);
    if (automatic) {
        for (size_t k = 0; k < K; k++) {
            PSCHK(use_device(parts[k]));
            uint64_t ck = 0;
            if (k == 0) PSCHK(tm.timed(0, p0->stream, [&]() { return ld_count_candidates(p0, prm->min_minor, &d_incl[0], &ck); }));
            else PSCHK(ld_count_candidates(parts[k], prm->min_minor, &d_incl[k], &ck));
            rank_lo[k + 1] = rank_lo[k] + ck;
        }
        const uint64_t C = g.C = rank_lo[K], M = g.M = std::min<uint64_t>(C, prm->max_loci);
        auto first_j = [&](uint64_t rank) { return C <= prm->max_loci ? rank : (rank * prm->max_loci + C - 1) / C; };
        for (size_t k = 0; k < K; k++) {
            j_lo[k] = (uint32_t)std::min(M, first_j(rank_lo[k]));
            j_cnt[k] = (uint32_t)std::min(M, first_j(rank_lo[k + 1])) - j_lo[k];
        }
    } else {
        g.M = n_loci;
        for (size_t k = 0; k < K; k++) {
            const uint64_t off = parts[k]->cfg.col_offset, end = off + parts[k]->cfg.ncols;
            j_lo[k] = (uint32_t)(std::lower_bound(loci, loci + n_loci, (uint32_t)std::min<uint64_t>(off, 0xffffffffull)) - loci);
            j_cnt[k] = (uint32_t)(std::lower_bound(loci, loci + n_loci, (uint32_t)std::min<uint64_t>(end, 0xffffffffull)) - loci) - j_lo[k];
        }
    }
    const uint64_t M = g.M;
    g.Mpad = (uint32_t)((std::max<uint64_t>(M, 1) + 127) & ~127ull);
    g.WP = ((g.N + 31u) / 32u + 7u) & ~7u;
    g.ldi = g.Mpad + 128u;
    // rows of loci per band: the u16 counts of a band stay below 128 MB unless asked otherwise; a wave of the contraction stores 64
    // whole rows, so a band is a multiple of that
    g.band = p0->ld_band ? ((uint64_t)p0->ld_band + 63) & ~63ull : std::max<uint64_t>(256, ((64ull << 20) / g.ldi) & ~255ull);
    g.band = std::min<uint64_t>(g.band, g.Mpad);
    g.n_words = (PS_LD_WORDS + PS_LD_MAX_LAGS + nbins + 1) & ~1ull;
    g.row_words = (uint64_t)g.Mpad * g.WP;
    std::vector<uint32_t> h_idx(M), h_cnt(M);
    std::vector<ld_scratch> S(K);
    for (size_t k = 0; k < K && M > 0; k++) {
        ps_population *p = parts[k];
        if (k && !j_cnt[k]) continue;
        PSCHK(use_device(p));
        PSCHK(ld_scratch_get(p, g, k == 0, &S[k]));
        if (k == 0) HIPCHK(hipMemsetAsync(S[0].words, 0, g.n_words * 8, p->stream));
        PSCHK(ld_select_pack(p, g, S[k], k == 0 ? &tm : nullptr, d_incl[k], rank_lo[k], j_lo[k], j_cnt[k], h_idx.data(), h_cnt.data()));
    }
    uint64_t poly = 0;
    for (uint64_t a = 0; a < M; a++) poly += ps_ld_monomorphic(h_cnt[a], g.N) ? 0 : 1;
    ld_fill(out, g.N, columns, automatic ? g.C : poly, M, prm);
    memset(hist, 0, nbins * sizeof(uint64_t));
    memset(lag_sum_q, 0, prm->lag_bins * sizeof(uint64_t));
    if (locus_index && M) memcpy(locus_index, h_idx.data(), M * sizeof(uint32_t));
    if (locus_count && M) memcpy(locus_count, h_cnt.data(), M * sizeof(uint32_t));
    unsigned long long w[PS_LD_WORDS] = {};
    PSCHK(use_device(p0));
    if (M >= 2) PSCHK(ld_pair_phase(parts, g, S, j_cnt, tm, prm, h_idx.data(), h_cnt.data(), w, hist, lag_sum_q));
    HIPCHK(hipStreamSynchronize(p0->stream));
    PSCHK(tm.collect(ro, 4));
    ld_finish(out, w, hist, lag_sum_q);
    return PS_OK;
}

extern "C" int ps_locus_ld(ps_population *p, const ps_ld_params *prm, const uint32_t *loci, uint32_t n_loci, ps_ld_t *out,
                           uint32_t *locus_index, uint32_t *locus_count, uint64_t *hist, uint64_t *lag_sum_q)
{
    PSCHK(ps_needs_device());
    if (!p || !prm || !out || !hist || !lag_sum_q) return ps_fail(PS_ERR_INVALID, "null argument");
    if (p->cfg.ncols != p->cfg.global_cols)
        return ps_fail(PS_ERR_INVALID, "ps_locus_ld pairs loci over all %llu core sites; this handle is one site shard ([%llu, %llu)): use "
                                       "ps_multi_locus_ld", (unsigned long long)p->cfg.global_cols, (unsigned long long)p->cfg.col_offset,
                       (unsigned long long)(p->cfg.col_offset + p->cfg.ncols));
    return ld_run({ p }, p->cfg.ncols, prm, loci, n_loci, out, locus_index, locus_count, hist, lag_sum_q);
}

static int ld_check_metric(int32_t metric)
{
    if (metric != PS_LD_CORE && metric != PS_LD_ACC)
        return ps_fail(PS_ERR_INVALID, "the metric of linkage disequilibrium is PS_LD_CORE (0) or PS_LD_ACC (1), not %d", (int)metric);
    return PS_OK;
}

extern "C" int ps_sim_locus_ld(ps_sim *s, int32_t metric, const ps_ld_params *prm, const uint32_t *loci, uint32_t n_loci, ps_ld_t *out,
                               uint32_t *locus_index, uint32_t *locus_count, uint64_t *hist, uint64_t *lag_sum_q)
{
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(ld_check_metric(metric));
    PSCHK(ps_sim_sync(s));
    return ps_locus_ld(metric == PS_LD_CORE ? s->core : s->acc, prm, loci, n_loci, out, locus_index, locus_count, hist, lag_sum_q);
}

extern "C" int ps_multi_locus_ld(ps_multi *m, int32_t metric, const ps_ld_params *prm, const uint32_t *loci, uint32_t n_loci, ps_ld_t *out,
                                 uint32_t *locus_index, uint32_t *locus_count, uint64_t *hist, uint64_t *lag_sum_q)
{
    PSCHK(ps_needs_device());
    if (!m || !prm || !out || !hist || !lag_sum_q) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(ld_check_metric(metric));
    if (m->shard.size() == 1 || metric == PS_LD_ACC)
        return ps_sim_locus_ld(m->shard[0], metric, prm, loci, n_loci, out, locus_index, locus_count, hist, lag_sum_q);
    // (the pack kernels of the shards run on their own streams behind their generations; part 0 reads the others' rows only
    // after their streams have been synchronised)
    PSCHK(ps_multi_sync(m));
    std::vector<ps_population *> parts;
    for (ps_sim *s : m->shard) parts.push_back(s->core);
    return ld_run(parts, m->prm.core_size, prm, loci, n_loci, out, locus_index, locus_count, hist, lag_sum_q);
}

extern "C" int ps_locus_ld_timing(ps_population *p, double *select_ms, double *pack_ms, double *counts_ms, double *stats_ms)
{
    if (!p) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(p->ro[PS_RO_LD], "no linkage disequilibrium has been computed on this handle", { select_ms, pack_ms, counts_ms, stats_ms });
}
