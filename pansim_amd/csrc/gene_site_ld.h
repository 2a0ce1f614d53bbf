// gene_site_ld.h -- ps_gene_site_ld / ps_sim_gene_site_ld / ps_multi_gene_site_ld, the host restatement ps_gene_site_from_counts
// and ps_gene_site_ld_timing (include/pansim_hip.h; the definitions: docs/GENE_SITE_ASSOCIATION.md).  Included by pansim_capi.hip
// behind locus_ld.h, whose selection (ld_count_candidates, ld_select_kernel) and pack kernels it runs once per side.
//
// One routine serves every entry: the accessory handle and a list of `parts` (the core handle; or the core handles of the shards
// of a run).  The genes take the list positions [0, Mg) of one blocked bit operand on part 0 and are selected and packed on the
// accessory handle's stream; the sites take [Mg, Mg + Ms) and are packed by every part on its own stream, part 0 behind an event
// of the accessory stream (which zeroed the operand first).  The other parts' rows are ORed on part 0, where the contraction
// (acc_intersections_launch over bands of GENE rows) and gene_site_pair_kernel run; the host decodes the arg-max keys.
#pragma once

#include "gene_site_kernels.h"

#define PS_GS_MAX_BINS 16384u      // 64 KB of u32 bins in LDS per workgroup
#define PS_GS_MAX_LOCI 65536u      // both lists share one operand of at most PS_LD_MAX_LOCI rows

static int gs_check_params(const ps_gs_params *prm)
{
    if (prm->r2_bins < 1) return ps_fail(PS_ERR_INVALID, "r2_bins must be >= 1");
    if (prm->freq_bins < 1) return ps_fail(PS_ERR_INVALID, "freq_bins must be >= 1");
    if ((uint64_t)prm->r2_bins * prm->freq_bins > PS_GS_MAX_BINS)
        return ps_fail(PS_ERR_INVALID, "r2_bins x freq_bins = %llu exceeds the limit of %u bins (64 KB of LDS per workgroup)",
                       (unsigned long long)prm->r2_bins * prm->freq_bins, PS_GS_MAX_BINS);
    if (prm->strong_q < 1 || prm->strong_q > 65536u) return ps_fail(PS_ERR_INVALID, "strong_q must be 1 .. 65536, not %u", prm->strong_q);
    return PS_OK;
}

// the selection of both sides: an automatic side needs its minor and its cap, the two lists fit one operand
static int gs_check_selection(const ps_gs_params *prm, bool auto_sites, uint32_t n_sites, bool auto_genes, uint32_t n_genes)
{
    if (auto_sites && prm->site_min_minor < 1) return ps_fail(PS_ERR_INVALID, "site_min_minor must be >= 1");
    if (auto_genes && prm->gene_min_minor < 1) return ps_fail(PS_ERR_INVALID, "gene_min_minor must be >= 1");
    if (auto_sites && prm->max_sites < 1) return ps_fail(PS_ERR_INVALID, "max_sites must be >= 1");
    if (auto_genes && prm->max_genes < 1) return ps_fail(PS_ERR_INVALID, "max_genes must be >= 1");
    const uint64_t room = (uint64_t)(auto_sites ? prm->max_sites : n_sites) + (auto_genes ? prm->max_genes : n_genes);
    if (room > PS_GS_MAX_LOCI)
        return ps_fail(PS_ERR_INVALID, "%s + %s = %llu exceeds the limit of %u loci in one operand", auto_sites ? "max_sites" : "n_sites",
                       auto_genes ? "max_genes" : "n_genes", (unsigned long long)room, PS_GS_MAX_LOCI);
    return PS_OK;
}

static int gs_check_list(const char *what, const uint32_t *list, uint64_t n, uint64_t columns)
{
    for (uint64_t k = 0; k < n; k++) {
        if (columns && list[k] >= columns)
            return ps_fail(PS_ERR_INVALID, "%s %llu: column %u is not below the %llu columns", what, (unsigned long long)k, list[k],
                           (unsigned long long)columns);
        if (k && list[k] <= list[k - 1])
            return ps_fail(PS_ERR_INVALID, "%s %llu: the list must be strictly ascending (%u after %u)", what, (unsigned long long)k, list[k],
                           list[k - 1]);
    }
    return PS_OK;
}

static void gs_fill(ps_gs_t *o, uint64_t N, uint64_t Ms, uint64_t Mg, const ps_gs_params *prm)
{
    memset(o, 0, sizeof *o);
    o->pop_size = N;
    o->sites = Ms;
    o->genes = Mg;
    o->pairs = Ms * Mg;
    o->r2_bins = prm->r2_bins;
    o->freq_bins = prm->freq_bins;
    o->site_min_minor = prm->site_min_minor;
    o->gene_min_minor = prm->gene_min_minor;
    o->max_sites = prm->max_sites;
    o->max_genes = prm->max_genes;
    o->strong_q = prm->strong_q;
}

// The arg-max keys of the M loci of one side -> (column of the best partner, q, sign) through the optional arrays; -> the loci
// whose best q reaches strong_q
static uint64_t gs_decode_side(const unsigned long long *key, uint64_t M, const uint32_t *partner_index, uint32_t strong_q,
                               const ps_gs_side *side)
{
    uint64_t tagged = 0;
    for (uint64_t a = 0; a < M; a++) {
        const unsigned long long k = key[a];
        const uint32_t q = k ? ps_gs_key_q(k) : 0u;
        tagged += k && q >= strong_q ? 1 : 0;
        if (!side) continue;
        if (side->best) side->best[a] = k ? partner_index[ps_gs_key_partner(k)] : PS_GS_NONE;
        if (side->best_q) side->best_q[a] = q;
        if (side->best_sign) side->best_sign[a] = k ? ps_gs_key_sign(k) : 0;
    }
    return tagged;
}

// the summary words, the bins and the frequency sums in place, the decoded keys -> the totals and the one double
static void gs_finish(ps_gs_t *o, const unsigned long long *w, const uint64_t *hist, const uint64_t *freq_sum_q, uint64_t genes_tagged,
                      uint64_t sites_tagging)
{
    o->undefined_pairs = w[PS_GS_UNDEF];
    o->four_gamete_pairs = w[PS_GS_FOURG];
    o->complete_pairs = w[PS_GS_COMPLETE];
    o->positive_pairs = w[PS_GS_POS];
    o->negative_pairs = w[PS_GS_NEG];
    o->strong_pairs = w[PS_GS_STRONG];
    o->genes_tagged = genes_tagged;
    o->sites_tagging = sites_tagging;
    for (uint64_t b = 0; b < o->r2_bins * o->freq_bins; b++) o->defined_pairs += hist[b];
    for (uint64_t b = 0; b < o->freq_bins; b++) o->sum_q += freq_sum_q[b];
    o->mean_r2 = o->defined_pairs ? (double)o->sum_q / 65536.0 / (double)o->defined_pairs : 0.0;
}

extern "C" int ps_gene_site_from_counts(const uint32_t *site_index, const uint32_t *site_count, uint64_t n_sites, const uint32_t *gene_index,
                                        const uint32_t *gene_count, uint64_t n_genes, const uint32_t *n11, uint64_t pop_size,
                                        const ps_gs_params *prm, ps_gs_t *out, const ps_gs_side *site_out, const ps_gs_side *gene_out,
                                        uint64_t *hist, uint64_t *freq_sum_q)
{
    if (!prm || !out || !hist || !freq_sum_q || (n_sites && (!site_index || !site_count)) || (n_genes && (!gene_index || !gene_count)) ||
        (n_sites && n_genes && !n11))
        return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(gs_check_params(prm));
    PSCHK(ld_check_pop(pop_size));
    if (n_sites + n_genes > PS_GS_MAX_LOCI || n_sites > PS_GS_MAX_LOCI)
        return ps_fail(PS_ERR_INVALID, "n_sites + n_genes = %llu exceeds the limit of %u loci in one operand",
                       (unsigned long long)(n_sites + n_genes), PS_GS_MAX_LOCI);
    PSCHK(gs_check_list("site", site_index, n_sites, 0));
    PSCHK(gs_check_list("gene", gene_index, n_genes, 0));
    const uint64_t Ms = n_sites, Mg = n_genes;
    const uint32_t N = (uint32_t)pop_size;
    for (uint64_t b = 0; b < Ms; b++)
        if (site_count[b] > N)
            return ps_fail(PS_ERR_INVALID, "site %llu: %u ones among %u individuals", (unsigned long long)b, site_count[b], N);
    for (uint64_t a = 0; a < Mg; a++)
        if (gene_count[a] > N)
            return ps_fail(PS_ERR_INVALID, "gene %llu: %u ones among %u individuals", (unsigned long long)a, gene_count[a], N);
    const uint64_t nbins = (uint64_t)prm->r2_bins * prm->freq_bins;
    memset(hist, 0, nbins * sizeof(uint64_t));
    memset(freq_sum_q, 0, prm->freq_bins * sizeof(uint64_t));
    unsigned long long w[PS_GS_WORDS] = {};
    std::vector<unsigned long long> gene_key(Mg, 0ull), site_key(Ms, 0ull);
    std::vector<uint32_t> gene_strong(Mg, 0u), site_strong(Ms, 0u);
    for (uint64_t a = 0; a < Mg; a++) {
        const uint32_t ca = gene_count[a];
        const bool mono_a = ps_ld_monomorphic(ca, N);
        const uint32_t fb = mono_a ? 0u : ps_gs_freq_bin(ca, N, prm->freq_bins);
        for (uint64_t b = 0; b < Ms; b++) {
            const uint32_t cb = site_count[b], n = n11[a * Ms + b];
            if (n > std::min(ca, cb) || (uint64_t)ca + cb > (uint64_t)N + n)
                return ps_fail(PS_ERR_INVALID, "pair (%llu, %llu): n11 = %u does not fit the counts %u and %u of %u individuals",
                               (unsigned long long)a, (unsigned long long)b, n, ca, cb, N);
            if (mono_a || ps_ld_monomorphic(cb, N)) {
                w[PS_GS_UNDEF]++;
                continue;
            }
            ps_ld_pair_t p;
            ps_ld_pair(N, ca, cb, n, 0u, 1u, prm->r2_bins, 1u, &p);
            hist[(uint64_t)fb * prm->r2_bins + p.r2_bin]++;
            freq_sum_q[fb] += p.q;
            const uint32_t strong = p.q >= prm->strong_q ? 1u : 0u;
            w[PS_GS_STRONG] += strong;
            gene_strong[a] += strong;
            site_strong[b] += strong;
            w[PS_GS_FOURG] += p.four;
            w[PS_GS_COMPLETE] += p.complete;
            w[PS_GS_POS] += p.sign > 0 ? 1 : 0;
            w[PS_GS_NEG] += p.sign < 0 ? 1 : 0;
            gene_key[a] = std::max<unsigned long long>(gene_key[a], ps_gs_key(p.q, (uint32_t)b, p.sign));
            site_key[b] = std::max<unsigned long long>(site_key[b], ps_gs_key(p.q, (uint32_t)a, p.sign));
        }
    }
    gs_fill(out, pop_size, Ms, Mg, prm);
    if (gene_out && gene_out->strong && Mg) memcpy(gene_out->strong, gene_strong.data(), Mg * sizeof(uint32_t));
    if (site_out && site_out->strong && Ms) memcpy(site_out->strong, site_strong.data(), Ms * sizeof(uint32_t));
    const uint64_t tagged = gs_decode_side(gene_key.data(), Mg, site_index, prm->strong_q, gene_out);
    const uint64_t tagging = gs_decode_side(site_key.data(), Ms, gene_index, prm->strong_q, site_out);
    gs_finish(out, w, hist, freq_sum_q, tagged, tagging);
    return PS_OK;
}

// What the phases of gs_run share: the two lists (nullptr: automatic) and the sizes that follow from them
struct gs_geom {
    const uint32_t *sites = nullptr, *genes = nullptr;
    uint32_t N = 0, Mg = 0, Ms = 0, Mpad = 0, WP = 0, ldi = 0, freq_bins = 0;
    uint64_t Cs = 0, Cg = 0, band = 0, nbins = 0, row_words = 0;
    size_t K = 1;
};

// the call's scratch on one part: words | freq sums | bins | gene keys | site keys | gene strong | site strong (part 0 only), then
// sel | cnt | rows on every part -- all of it zeroed per call -- and behind them on part 0 the landing rows (with several parts)
// and one band of n11
struct gs_scratch {
    unsigned long long *words = nullptr, *freq = nullptr, *hist = nullptr, *gene_key = nullptr, *site_key = nullptr;
    uint32_t *gene_strong = nullptr, *site_strong = nullptr, *sel = nullptr, *cnt = nullptr, *rows = nullptr, *land = nullptr;
    uint16_t *in = nullptr;
    uint8_t *base = nullptr;
    uint64_t zero_bytes = 0;
};

static int gs_scratch_get(ps_population *p, const gs_geom &g, bool first, gs_scratch *s)
{
    // (every region a multiple of 256 bytes: the pair kernel reads four counts per lane, the contraction whole 16-byte pieces of the rows)
    scratch_layout lay;
    const uint64_t o_words = lay.add(first ? PS_GS_WORDS * 8 : 0, 256), o_freq = lay.add(first ? g.freq_bins * 8ull : 0, 256);
    const uint64_t o_hist = lay.add(first ? g.nbins * 8 : 0, 256);
    const uint64_t o_gkey = lay.add(first ? g.Mg * 8ull : 0, 256), o_skey = lay.add(first ? g.Ms * 8ull : 0, 256);
    const uint64_t o_gstr = lay.add(first ? g.Mg * 4ull : 0, 256), o_sstr = lay.add(first ? g.Ms * 4ull : 0, 256);
    const uint64_t o_sel = lay.add(g.Mpad * 4ull, 256), o_cnt = lay.add(g.Mpad * 4ull, 256), o_rows = lay.add(g.row_words * 4, 256);
    const uint64_t zero_bytes = lay.bytes;
    const uint64_t o_land = lay.add(first && g.K > 1 ? g.row_words * 4 : 0, 256), o_in = lay.add(first ? g.band * g.ldi * 2 : 0, 256);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(p->ro[PS_RO_GS], lay.bytes, &base, "cannot allocate the %llu bytes of the bit rows of %u loci and one band of their pair counts",
                      g.Mg + g.Ms));
    s->base = base;
    s->zero_bytes = zero_bytes;
    s->words = (unsigned long long *)(base + o_words);      // (the regions of part 0 are empty on the others)
    s->freq = (unsigned long long *)(base + o_freq);
    s->hist = (unsigned long long *)(base + o_hist);
    s->gene_key = (unsigned long long *)(base + o_gkey);
    s->site_key = (unsigned long long *)(base + o_skey);
    s->gene_strong = (uint32_t *)(base + o_gstr);
    s->site_strong = (uint32_t *)(base + o_sstr);
    s->sel = (uint32_t *)(base + o_sel);
    s->cnt = (uint32_t *)(base + o_cnt);
    s->rows = (uint32_t *)(base + o_rows);
    s->land = (uint32_t *)(base + o_land);
    s->in = (uint16_t *)(base + o_in);
    return PS_OK;
}

// The list entries [pos, pos + n) that handle `p` holds, queued on its stream: selected on its device (entry t = the candidate of
// rank_lo-relative rank j_lo + t of C, or list[j_lo + t]) and packed into bit rows at their positions (the scratch is zero: pad
// dwords, pad rows and monomorphic rows stay so).  h_sel: the explicit entries' local columns, alive until the stream has run.
static int gs_select_pack(ps_population *p, const gs_geom &g, const gs_scratch &s, event_timer *tm, const uint32_t *list, const uint32_t *d_incl,
                          uint64_t C, uint32_t cap, uint64_t rank_lo, uint32_t j_lo, uint32_t pos, uint32_t n, std::vector<uint32_t> &h_sel)
{
    if (!n) return PS_OK;
    hipStream_t st = p->stream;
    auto select = [&]() -> int {
        if (!list) {
            ld_select_kernel<<<(n + 255u) / 256u, 256, 0, st>>>(d_incl, (uint32_t)p->cfg.ncols, C, rank_lo, j_lo, n, cap, s.sel + pos);
            HIPCHK(hipGetLastError());
        } else {
            h_sel.resize(n);
            for (uint32_t t = 0; t < n; t++) h_sel[t] = (uint32_t)(list[j_lo + t] - p->cfg.col_offset);
            HIPCHK(hipMemcpyAsync(s.sel + pos, h_sel.data(), n * 4ull, hipMemcpyHostToDevice, st));
        }
        return PS_OK;
    };
    auto pack = [&]() -> int {
        if (p->cfg.core) {
            ld_pack_core_kernel<<<(n + 3u) / 4u, 256, 0, st>>>((const uint8_t *)p->state, p->pitch, g.N, s.sel + pos, n, pos, g.WP, s.rows, s.cnt);
        } else {
            PSCHK(ensure_gene_major(p, st));
            ld_pack_acc_kernel<<<(n + 3u) / 4u, 256, 0, st>>>(p->G[0], p->d, s.sel + pos, n, pos, g.WP, s.rows, s.cnt);
        }
        HIPCHK(hipGetLastError());
        return PS_OK;
    };
    PSCHK(tm ? tm->timed(0, st, select) : select());
    return tm ? tm->timed(1, st, pack) : pack();
}

// The pair phase, queued on part 0's stream: per band of gene rows the contraction (group 2) and gene_site_pair_kernel (group 3)
static int gs_pair_phase(ps_population *p0, const gs_geom &g, const gs_scratch &s, event_timer &tm, const ps_gs_params *prm)
{
    hipStream_t s0 = p0->stream;
    const uint32_t lds = (uint32_t)g.nbins * 4u;
    for (uint32_t lo = 0; lo < g.Mg; lo += (uint32_t)g.band) {
        const uint32_t nrows = std::min<uint32_t>((uint32_t)g.band, g.Mg - lo);
        dim3 grid;
        PSCHK(bin_grid((const void *)gene_site_pair_kernel, g.Ms, nrows, lds, 512u, &grid));
        PSCHK(tm.timed(2, s0, [&]() { return acc_intersections_launch(s.rows, g.WP, g.Mpad, g.ldi, 2u, lo, nrows, s.in, s0); }));
        PSCHK(tm.timed(3, s0, [&]() -> int {
            hipLaunchKernelGGL(gene_site_pair_kernel, grid, dim3(256), lds, s0, (const uint16_t *)s.in, g.ldi, (const uint32_t *)s.cnt, g.N, g.Mg,
                               g.Ms, lo, nrows, prm->r2_bins, prm->freq_bins, prm->strong_q, s.hist, s.freq, s.words, s.gene_strong, s.site_strong,
                               s.gene_key, s.site_key);
            HIPCHK(hipGetLastError());
            return PS_OK;
        }));
    }
    return PS_OK;
}

static void gs_side_copy(const ps_gs_side *side, const uint32_t *index, const uint32_t *count, const uint32_t *strong, uint64_t M)
{
    if (!side || !M) return;
    if (side->index) memcpy(side->index, index, M * sizeof(uint32_t));
    if (side->count) memcpy(side->count, count, M * sizeof(uint32_t));
    if (side->strong) memcpy(side->strong, strong, M * sizeof(uint32_t));
}

// parts[0] and acc live on one device; with several parts everything queued on every handle is complete (ps_multi_sync)
static int gs_run(const std::vector<ps_population *> &parts, ps_population *acc, uint64_t site_columns, const ps_gs_params *prm,
                  const uint32_t *sites, uint32_t n_sites, const uint32_t *genes, uint32_t n_genes, ps_gs_t *out, const ps_gs_side *site_out,
                  const ps_gs_side *gene_out, uint64_t *hist, uint64_t *freq_sum_q)
{
    ps_population *p0 = parts[0];
    const size_t K = parts.size();
    const bool auto_sites = sites == nullptr, auto_genes = genes == nullptr;
    const uint64_t N64 = p0->cfg.pop_size, gene_columns = acc->cfg.ncols;
    PSCHK(gs_check_params(prm));
    PSCHK(gs_check_selection(prm, auto_sites, n_sites, auto_genes, n_genes));
    PSCHK(ld_check_pop(N64));
    if (!auto_sites) PSCHK(gs_check_list("site", sites, n_sites, std::max<uint64_t>(site_columns, 1)));
    if (!auto_genes) PSCHK(gs_check_list("gene", genes, n_genes, std::max<uint64_t>(gene_columns, 1)));
    if (!auto_sites && n_sites && site_columns == 0) return ps_fail(PS_ERR_INVALID, "the core handle has no columns to list");
    if (!auto_genes && n_genes && gene_columns == 0) return ps_fail(PS_ERR_INVALID, "the accessory handle has no columns to list");
    gs_geom g;
    g.sites = sites;
    g.genes = genes;
    g.N = (uint32_t)N64;
    g.K = K;
    g.freq_bins = prm->freq_bins;
    g.nbins = (uint64_t)prm->r2_bins * prm->freq_bins;
    // timer groups: 0 = counts and selection of both sides, 1 = packing, 2 = the contraction, 3 = the pair statistics
    event_timer tm;
    readout_slot &ro = p0->ro[PS_RO_GS];
    ro.timed = false;
    PSCHK(use_device(p0));
    hipEvent_t ev_core = nullptr, ev_acc = nullptr;
    PSCHK(tm.make(&ev_core));
    PSCHK(tm.make(&ev_acc));
    // whatever either handle has queued precedes the work of both: the accessory stream waits for the core stream here, the core
    // stream for the accessory stream once the genes are packed
    HIPCHK(hipEventRecord(ev_core, p0->stream));
    HIPCHK(hipStreamWaitEvent(acc->stream, ev_core, 0));
    // the genes: the candidates of the accessory handle
    uint32_t *d_incl_g = nullptr;
    if (auto_genes) {
        PSCHK(tm.timed(0, acc->stream, [&]() { return ld_count_candidates(acc, prm->gene_min_minor, &d_incl_g, &g.Cg); }));
        g.Mg = (uint32_t)std::min<uint64_t>(g.Cg, prm->max_genes);
    } else {
        g.Mg = n_genes;
    }
    // the sites: the rows of the list every part holds, [j_lo, j_lo + j_cnt) (as ld_run)
    std::vector<uint32_t> j_lo(K, 0), j_cnt(K, 0);
    std::vector<uint32_t *> d_incl(K, nullptr);
    std::vector<uint64_t> rank_lo(K + 1, 0);
    if (auto_sites) {
        for (size_t k = 0; k < K; k++) {
            PSCHK(use_device(parts[k]));
            uint64_t ck = 0;
            if (k == 0) PSCHK(tm.timed(0, p0->stream, [&]() { return ld_count_candidates(p0, prm->site_min_minor, &d_incl[0], &ck); }));
            else PSCHK(ld_count_candidates(parts[k], prm->site_min_minor, &d_incl[k], &ck));
            rank_lo[k + 1] = rank_lo[k] + ck;
        }
        const uint64_t C = g.Cs = rank_lo[K], M = std::min<uint64_t>(C, prm->max_sites);
        g.Ms = (uint32_t)M;
        auto first_j = [&](uint64_t rank) { return C <= prm->max_sites ? rank : (rank * prm->max_sites + C - 1) / C; };
        for (size_t k = 0; k < K; k++) {
            j_lo[k] = (uint32_t)std::min(M, first_j(rank_lo[k]));
            j_cnt[k] = (uint32_t)std::min(M, first_j(rank_lo[k + 1])) - j_lo[k];
        }
    } else {
        g.Ms = n_sites;
        for (size_t k = 0; k < K; k++) {
            const uint64_t off = parts[k]->cfg.col_offset, end = off + parts[k]->cfg.ncols;
            j_lo[k] = (uint32_t)(std::lower_bound(sites, sites + n_sites, (uint32_t)std::min<uint64_t>(off, 0xffffffffull)) - sites);
            j_cnt[k] = (uint32_t)(std::lower_bound(sites, sites + n_sites, (uint32_t)std::min<uint64_t>(end, 0xffffffffull)) - sites) - j_lo[k];
        }
    }
    const uint32_t Mg = g.Mg, Ms = g.Ms, M = Mg + Ms;
    g.Mpad = (uint32_t)((std::max<uint64_t>(M, 1) + 127) & ~127ull);
    g.WP = ((g.N + 31u) / 32u + 7u) & ~7u;
    g.ldi = g.Mpad + 128u;
    // gene rows per band, as the loci of ld_run: the u16 counts of a band stay below 128 MB unless asked otherwise ("ld_band"); a wave
    // of the contraction stores 64 whole rows, so a band is a multiple of that
    g.band = p0->ld_band ? ((uint64_t)p0->ld_band + 63) & ~63ull : std::max<uint64_t>(256, ((64ull << 20) / g.ldi) & ~255ull);
    g.band = std::min<uint64_t>(g.band, ((uint64_t)std::max(Mg, 1u) + 63) & ~63ull);
    g.row_words = (uint64_t)g.Mpad * g.WP;
    // list position -> local column (automatic sides; the explicit ones keep their upload alive), ones, keys and strong pairs
    std::vector<uint32_t> h_sel(g.Mpad), h_cnt(g.Mpad), h_idx(g.Mpad), h_strong(std::max(M, 1u)), h_sel_g;
    std::vector<std::vector<uint32_t>> h_sel_s(K);
    std::vector<unsigned long long> h_key(std::max(M, 1u));
    std::vector<gs_scratch> S(K);
    PSCHK(use_device(p0));
    PSCHK(gs_scratch_get(p0, g, true, &S[0]));
    const gs_scratch &s = S[0];
    HIPCHK(hipMemsetAsync(s.base, 0, s.zero_bytes, acc->stream));
    PSCHK(gs_select_pack(acc, g, s, &tm, genes, d_incl_g, g.Cg, prm->max_genes, 0, 0, 0, Mg, h_sel_g));
    HIPCHK(hipEventRecord(ev_acc, acc->stream));
    HIPCHK(hipStreamWaitEvent(p0->stream, ev_acc, 0));
    PSCHK(gs_select_pack(p0, g, s, &tm, sites, d_incl[0], g.Cs, prm->max_sites, rank_lo[0], j_lo[0], Mg + j_lo[0], j_cnt[0], h_sel_s[0]));
    if (K > 1) {
        // every part's columns and counts through the host, as ld_run: part 0's stream first, then the others'
        HIPCHK(hipMemcpyAsync(h_sel.data(), s.sel, std::max(M, 1u) * 4ull, hipMemcpyDeviceToHost, p0->stream));
        HIPCHK(hipMemcpyAsync(h_cnt.data(), s.cnt, std::max(M, 1u) * 4ull, hipMemcpyDeviceToHost, p0->stream));
        HIPCHK(hipStreamSynchronize(p0->stream));
        for (size_t k = 1; k < K; k++) {
            ps_population *p = parts[k];
            if (!j_cnt[k]) continue;
            const uint32_t pos = Mg + j_lo[k];
            PSCHK(use_device(p));
            PSCHK(gs_scratch_get(p, g, false, &S[k]));
            HIPCHK(hipMemsetAsync(S[k].base, 0, S[k].zero_bytes, p->stream));
            PSCHK(gs_select_pack(p, g, S[k], nullptr, sites, d_incl[k], g.Cs, prm->max_sites, rank_lo[k], j_lo[k], pos, j_cnt[k], h_sel_s[k]));
            HIPCHK(hipMemcpyAsync(h_sel.data() + pos, S[k].sel + pos, j_cnt[k] * 4ull, hipMemcpyDeviceToHost, p->stream));
            HIPCHK(hipMemcpyAsync(h_cnt.data() + pos, S[k].cnt + pos, j_cnt[k] * 4ull, hipMemcpyDeviceToHost, p->stream));
            HIPCHK(hipStreamSynchronize(p->stream));
            for (uint32_t t = 0; t < j_cnt[k]; t++) h_sel[pos + t] += (uint32_t)p->cfg.col_offset;
        }
        PSCHK(use_device(p0));
        for (size_t k = 1; k < K; k++) {
            if (!j_cnt[k]) continue;
            PSCHK(tm.timed(1, p0->stream, [&]() -> int {
                HIPCHK(hipMemcpyPeerAsync(s.land, p0->device, S[k].rows, parts[k]->device, g.row_words * 4, p0->stream));
                ld_or_kernel<<<(uint32_t)((g.row_words + 255) / 256), 256, 0, p0->stream>>>(s.rows, s.land, g.row_words);
                HIPCHK(hipGetLastError());
                return PS_OK;
            }));
        }
        if (Ms) HIPCHK(hipMemcpyAsync(s.cnt + Mg, h_cnt.data() + Mg, Ms * 4ull, hipMemcpyHostToDevice, p0->stream));
    }
    if (Mg && Ms) PSCHK(gs_pair_phase(p0, g, s, tm, prm));
    unsigned long long w[PS_GS_WORDS] = {};
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the bins are copied as they are");
    hipStream_t s0 = p0->stream;
    if (K == 1) {
        HIPCHK(hipMemcpyAsync(h_sel.data(), s.sel, std::max(M, 1u) * 4ull, hipMemcpyDeviceToHost, s0));
        HIPCHK(hipMemcpyAsync(h_cnt.data(), s.cnt, std::max(M, 1u) * 4ull, hipMemcpyDeviceToHost, s0));
    }
    HIPCHK(hipMemcpyAsync(w, s.words, sizeof w, hipMemcpyDeviceToHost, s0));
    HIPCHK(hipMemcpyAsync(freq_sum_q, s.freq, prm->freq_bins * sizeof(uint64_t), hipMemcpyDeviceToHost, s0));
    HIPCHK(hipMemcpyAsync(hist, s.hist, g.nbins * sizeof(uint64_t), hipMemcpyDeviceToHost, s0));
    if (M) {
        // (gene keys | site keys and gene strong | site strong are contiguous when Mg is even; copied per side either way)
        if (Mg) HIPCHK(hipMemcpyAsync(h_key.data(), s.gene_key, Mg * 8ull, hipMemcpyDeviceToHost, s0));
        if (Ms) HIPCHK(hipMemcpyAsync(h_key.data() + Mg, s.site_key, Ms * 8ull, hipMemcpyDeviceToHost, s0));
        if (Mg) HIPCHK(hipMemcpyAsync(h_strong.data(), s.gene_strong, Mg * 4ull, hipMemcpyDeviceToHost, s0));
        if (Ms) HIPCHK(hipMemcpyAsync(h_strong.data() + Mg, s.site_strong, Ms * 4ull, hipMemcpyDeviceToHost, s0));
    }
    HIPCHK(hipStreamSynchronize(s0));
    PSCHK(tm.collect(ro, 4));
    // list position -> global column: the explicit lists as given, the automatic ones from the selected local columns (the
    // offsets of part 0 and of the accessory handle are 0; those of the other parts have been added)
    for (uint32_t a = 0; a < Mg; a++) h_idx[a] = auto_genes ? h_sel[a] : genes[a];
    for (uint32_t b = 0; b < Ms; b++) h_idx[Mg + b] = auto_sites ? h_sel[Mg + b] : sites[b];
    uint64_t poly_g = 0, poly_s = 0;
    for (uint32_t a = 0; a < Mg; a++) poly_g += ps_ld_monomorphic(h_cnt[a], g.N) ? 0 : 1;
    for (uint32_t b = 0; b < Ms; b++) poly_s += ps_ld_monomorphic(h_cnt[Mg + b], g.N) ? 0 : 1;
    gs_fill(out, g.N, Ms, Mg, prm);
    out->site_columns = site_columns;
    out->gene_columns = gene_columns;
    out->site_candidates = auto_sites ? g.Cs : poly_s;
    out->gene_candidates = auto_genes ? g.Cg : poly_g;
    gs_side_copy(gene_out, h_idx.data(), h_cnt.data(), h_strong.data(), Mg);
    gs_side_copy(site_out, h_idx.data() + Mg, h_cnt.data() + Mg, h_strong.data() + Mg, Ms);
    const uint64_t tagged = gs_decode_side(h_key.data(), Mg, h_idx.data() + Mg, prm->strong_q, gene_out);
    const uint64_t tagging = gs_decode_side(h_key.data() + Mg, Ms, h_idx.data(), prm->strong_q, site_out);
    gs_finish(out, w, hist, freq_sum_q, tagged, tagging);
    return PS_OK;
}

static int gs_handles(const ps_population *core, const ps_population *acc, const char *call)
{
    if (!core->cfg.core) return ps_fail(PS_ERR_INVALID, "%s takes a core handle first", call);
    if (acc->cfg.core) return ps_fail(PS_ERR_INVALID, "%s takes an accessory handle second", call);
    if (core->cfg.pop_size != acc->cfg.pop_size)
        return ps_fail(PS_ERR_INVALID, "%s: the core handle holds %llu individuals, the accessory handle %llu", call,
                       (unsigned long long)core->cfg.pop_size, (unsigned long long)acc->cfg.pop_size);
    if (core->device != acc->device) return ps_fail(PS_ERR_INVALID, "%s: the two handles live on different devices", call);
    return PS_OK;
}

extern "C" int ps_gene_site_ld(ps_population *core, ps_population *acc, const ps_gs_params *prm, const uint32_t *sites, uint32_t n_sites,
                               const uint32_t *genes, uint32_t n_genes, ps_gs_t *out, const ps_gs_side *site_out, const ps_gs_side *gene_out,
                               uint64_t *hist, uint64_t *freq_sum_q)
{
    PSCHK(ps_needs_device());
    if (!core || !acc || !prm || !out || !hist || !freq_sum_q) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(gs_handles(core, acc, "ps_gene_site_ld"));
    if (core->cfg.ncols != core->cfg.global_cols)
        return ps_fail(PS_ERR_INVALID, "ps_gene_site_ld pairs genes with all %llu core sites; this handle is one site shard ([%llu, %llu)): use "
                                       "ps_multi_gene_site_ld", (unsigned long long)core->cfg.global_cols, (unsigned long long)core->cfg.col_offset,
                       (unsigned long long)(core->cfg.col_offset + core->cfg.ncols));
    return gs_run({ core }, acc, core->cfg.ncols, prm, sites, n_sites, genes, n_genes, out, site_out, gene_out, hist, freq_sum_q);
}

extern "C" int ps_sim_gene_site_ld(ps_sim *s, const ps_gs_params *prm, const uint32_t *sites, uint32_t n_sites, const uint32_t *genes,
                                   uint32_t n_genes, ps_gs_t *out, const ps_gs_side *site_out, const ps_gs_side *gene_out, uint64_t *hist,
                                   uint64_t *freq_sum_q)
{
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    // (no ps_sim_sync: the call is ordered behind the run on the two streams)
    return ps_gene_site_ld(s->core, s->acc, prm, sites, n_sites, genes, n_genes, out, site_out, gene_out, hist, freq_sum_q);
}

extern "C" int ps_multi_gene_site_ld(ps_multi *m, const ps_gs_params *prm, const uint32_t *sites, uint32_t n_sites, const uint32_t *genes,
                                     uint32_t n_genes, ps_gs_t *out, const ps_gs_side *site_out, const ps_gs_side *gene_out, uint64_t *hist,
                                     uint64_t *freq_sum_q)
{
    PSCHK(ps_needs_device());
    if (!m || !prm || !out || !hist || !freq_sum_q) return ps_fail(PS_ERR_INVALID, "null argument");
    if (m->shard.size() == 1) return ps_sim_gene_site_ld(m->shard[0], prm, sites, n_sites, genes, n_genes, out, site_out, gene_out, hist, freq_sum_q);
    // (the pack kernels of the shards run on their own streams behind their generations; part 0 reads the others' rows only
    // after their streams have been synchronised)
    PSCHK(ps_multi_sync(m));
    PSCHK(gs_handles(m->shard[0]->core, m->shard[0]->acc, "ps_multi_gene_site_ld"));
    std::vector<ps_population *> parts;
    for (ps_sim *s : m->shard) parts.push_back(s->core);
    return gs_run(parts, m->shard[0]->acc, m->prm.core_size, prm, sites, n_sites, genes, n_genes, out, site_out, gene_out, hist, freq_sum_q);
}

extern "C" int ps_gene_site_ld_timing(ps_population *core, double *select_ms, double *pack_ms, double *counts_ms, double *stats_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_GS], "no gene-site association has been computed on this handle", { select_ms, pack_ms, counts_ms, stats_ms });
}
