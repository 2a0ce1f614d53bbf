// group_differentiation.h -- ps_group_differentiation / ps_sim_group_differentiation / ps_multi_group_differentiation, the host
// rules ps_groups_from_labels and the host restatement ps_differentiation_from_counts (include/pansim_hip.h; the definitions:
// docs/GROUP_DIFFERENTIATION.md).  Included by pansim_capi.hip behind pair_readout.h.
//
// Labels arrive in the reference's row order, the matrices are in internal order: group_of is mapped through the handle's row
// slot (rows_current) before the membership tables are built (group_fragments_kernel, group_masks_kernel); the order of the
// sites is unaffected.  One pass over the core matrix on the core stream (core_group_counts_kernel), one over the gene-major
// view on the accessory stream (acc_group_gene_counts_kernel); everything else is integer arithmetic on the host.
#pragma once

#include "diff_kernels.h"

static int diff_check_params(const ps_diff_params *prm)
{
    if (prm->max_groups < 1 || prm->max_groups > PS_GROUPS_MAX)
        return ps_fail(PS_ERR_INVALID, "max_groups must be 1 .. %d, not %u", PS_GROUPS_MAX, prm->max_groups);
    if (prm->min_size < 1) return ps_fail(PS_ERR_INVALID, "min_size must be >= 1");
    return PS_OK;
}

extern "C" int ps_groups_from_labels(const uint32_t *labels, uint64_t pop_size, uint32_t max_groups, uint32_t min_size, uint32_t *group_of,
                                     uint32_t *group_label, uint32_t *group_size, uint32_t *groups)
{
    if (!group_of || !group_label || !group_size || !groups || (pop_size && !labels)) return ps_fail(PS_ERR_INVALID, "null argument");
    const ps_diff_params prm = { max_groups, min_size };
    PSCHK(diff_check_params(&prm));
    if (pop_size > 0xffffffffull) return ps_fail(PS_ERR_INVALID, "groups need pop_size < 2^32");
    // the distinct values with their sizes, then the candidates by (size descending, label ascending)
    std::vector<uint32_t> sorted(labels, labels + pop_size);
    std::sort(sorted.begin(), sorted.end());
    std::vector<std::pair<uint32_t, uint32_t>> cand;       // (size, label)
    for (uint64_t i = 0; i < pop_size;) {
        uint64_t j = i;
        while (j < pop_size && sorted[j] == sorted[i]) j++;
        if (j - i >= min_size) cand.push_back({ (uint32_t)(j - i), sorted[i] });
        i = j;
    }
    if (cand.empty())
        return ps_fail(PS_ERR_INVALID, "no label has at least %u members among %llu individuals: no groups", min_size, (unsigned long long)pop_size);
    std::sort(cand.begin(), cand.end(), [](const auto &a, const auto &b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
    const uint32_t K = (uint32_t)std::min<size_t>(cand.size(), max_groups);
    std::vector<std::pair<uint32_t, uint32_t>> by_label(K);  // (label, group)
    for (uint32_t g = 0; g < K; g++) {
        group_size[g] = cand[g].first;
        group_label[g] = cand[g].second;
        by_label[g] = { cand[g].second, g };
    }
    std::sort(by_label.begin(), by_label.end());
    for (uint64_t k = 0; k < pop_size; k++) {
        const auto it = std::lower_bound(by_label.begin(), by_label.end(), std::make_pair(labels[k], 0u));
        group_of[k] = it != by_label.end() && it->first == labels[k] ? it->second : UINT32_MAX;
    }
    *groups = K;
    return PS_OK;
}

// the fields of the summary that follow from the group sizes and the K x K differences
static void diff_summary(ps_diff_t *o, uint64_t N, uint64_t L, uint64_t G, uint32_t K, const uint32_t *group_size, const uint64_t *between,
                         uint64_t other_cells)
{
    memset(o, 0, sizeof *o);
    o->pop_size = N;
    o->sites = L;
    o->genes = G;
    o->groups = K;
    o->other_cells = other_cells;
    for (uint32_t g = 0; g < K; g++) {
        const uint64_t n = group_size[g];
        o->assigned += n;
        o->within_pairs += n * (n - (n ? 1 : 0)) / 2;
        o->within_differences += between[(uint64_t)g * K + g];
        for (uint32_t h = g + 1; h < K; h++) {
            o->between_pairs += n * group_size[h];
            o->between_differences += between[(uint64_t)g * K + h];
        }
    }
    o->unassigned = N - o->assigned;
    auto per = [&](uint64_t diffs, uint64_t pairs) { return pairs && L ? (double)diffs / (double)pairs / (double)L : 0.0; };
    o->pi_within = per(o->within_differences, o->within_pairs);
    o->pi_between = per(o->between_differences, o->between_pairs);
    o->fst = o->pi_between != 0.0 ? 1.0 - o->pi_within / o->pi_between : 0.0;
}

static int diff_check_sizes(uint32_t K, const uint32_t *group_size, uint64_t *assigned)
{
    if (K < 1 || K > PS_GROUPS_MAX) return ps_fail(PS_ERR_INVALID, "the number of groups must be 1 .. %d, not %u", PS_GROUPS_MAX, K);
    *assigned = 0;
    for (uint32_t g = 0; g < K; g++) *assigned += group_size[g];
    if (*assigned > 65536) return ps_fail(PS_ERR_INVALID, "the groups hold %llu individuals: more than 65536", (unsigned long long)*assigned);
    return PS_OK;
}

extern "C" int ps_differentiation_from_counts(const uint32_t *counts, uint64_t sites, uint32_t groups, const uint32_t *group_size, ps_diff_t *out,
                                              uint64_t *between, uint64_t *fixed, uint32_t *site_within, uint32_t *site_total)
{
    if (!out || !group_size || !between || !fixed || (!counts && sites)) return ps_fail(PS_ERR_INVALID, "null argument");
    const uint32_t K = groups;
    uint64_t Na;
    PSCHK(diff_check_sizes(K, group_size, &Na));
    memset(between, 0, (uint64_t)K * K * sizeof(uint64_t));
    memset(fixed, 0, (uint64_t)K * K * sizeof(uint64_t));
    uint64_t other_cells = 0;
    uint32_t c[PS_GROUPS_MAX][5];
    for (uint64_t s = 0; s < sites; s++) {
        uint32_t tot[5] = { 0, 0, 0, 0, 0 };
        for (uint32_t g = 0; g < K; g++) {
            const uint32_t *n = counts + (s * K + g) * 4;
            const uint64_t sum = (uint64_t)n[0] + n[1] + n[2] + n[3];
            if (sum > group_size[g])
                return ps_fail(PS_ERR_INVALID, "the counts of site %llu in group %u add up to more than its size %u", (unsigned long long)s, g,
                               group_size[g]);
            for (int a = 0; a < 4; a++) c[g][a] = n[a];
            c[g][4] = group_size[g] - (uint32_t)sum;
            other_cells += c[g][4];
            for (int a = 0; a < 5; a++) tot[a] += c[g][a];
        }
        uint64_t within = 0, df;
        uint32_t fx;
        for (uint32_t g = 0; g < K; g++)
            for (uint32_t h = g; h < K; h++) {
                ps_diff_site_terms(group_size[g], group_size[h], c[g], c[h], g == h, &df, &fx);
                between[(uint64_t)g * K + h] += df;
                fixed[(uint64_t)g * K + h] += fx;
                if (g == h) within += df;
            }
        ps_diff_site_terms(Na, Na, tot, tot, true, &df, &fx);
        if (site_within) site_within[s] = (uint32_t)within;
        if (site_total) site_total[s] = (uint32_t)df;
    }
    for (uint32_t g = 0; g < K; g++)
        for (uint32_t h = g + 1; h < K; h++) {
            between[(uint64_t)h * K + g] = between[(uint64_t)g * K + h];
            fixed[(uint64_t)h * K + g] = fixed[(uint64_t)g * K + h];
        }
    diff_summary(out, Na, sites, 0, K, group_size, between, other_cells);
    return PS_OK;
}

// what a call fills beside the summary and the groups: the required K x K matrices and the optional outputs (null: not asked for)
struct diff_outputs {
    uint64_t *between, *fixed;
    uint32_t *site_within, *site_total, *counts, *gene_counts;
    uint64_t *acc_between, *gene_fixed, *gene_private;
    bool genes() const { return gene_counts || acc_between || gene_fixed || gene_private; }
};

// the three results the host derives from the per-group gene counts
static void diff_gene_results(const uint32_t *gc, uint64_t G, uint32_t K, const uint32_t *group_size, const diff_outputs &o)
{
    if (o.acc_between) memset(o.acc_between, 0, (uint64_t)K * K * sizeof(uint64_t));
    if (o.gene_fixed) memset(o.gene_fixed, 0, (uint64_t)K * K * sizeof(uint64_t));
    if (o.gene_private) memset(o.gene_private, 0, (uint64_t)K * sizeof(uint64_t));
    for (uint64_t y = 0; y < G; y++) {
        const uint32_t *c = gc + y * K;
        uint32_t carriers = 0, last = 0;
        for (uint32_t g = 0; g < K; g++) {
            const uint64_t ng = group_size[g], cg = c[g];
            if (cg) {
                carriers++;
                last = g;
            }
            for (uint32_t h = 0; h < K; h++) {
                const uint64_t nh = group_size[h], ch = c[h];
                if (o.acc_between) o.acc_between[(uint64_t)g * K + h] += g == h ? cg * (ng - cg) : cg * (nh - ch) + (ng - cg) * ch;
                if (o.gene_fixed && g != h && cg == ng && ch == 0) o.gene_fixed[(uint64_t)g * K + h]++;
            }
        }
        if (o.gene_private && carriers == 1) o.gene_private[last]++;
    }
}

// group_int[internal row] = the group of the output row that lives there
static int diff_group_int(ps_population *p, const uint32_t *group_of, std::vector<uint32_t> *group_int)
{
    const uint32_t N = (uint32_t)p->cfg.pop_size;
    const uint32_t *slot = nullptr;
    PSCHK(rows_current(p, &slot));
    group_int->resize(N);
    for (uint32_t k = 0; k < N; k++) (*group_int)[slot ? slot[k] : k] = group_of[k];
    return PS_OK;
}

// The core pass of one handle (all sites, or one site shard: its own) on its stream, timed into groups 0 (members) and 1 (core);
// the words, and what `o` asks for of site_within / site_total / counts, land in host memory once the stream is synchronised.
static int diff_core_launch(ps_population *p, event_timer &tm, const uint32_t *group_of, uint32_t K, const uint32_t *group_size,
                            unsigned long long *words, const diff_outputs &o)
{
    const uint32_t N = (uint32_t)p->cfg.pop_size, rows = (uint32_t)p->cfg.ncols, nchunks = p->pitch / 64u;
    const bool sites = o.site_within || o.site_total, store = o.counts != nullptr;
    PSCHK(use_device(p));
    std::vector<uint32_t> group_int;
    PSCHK(diff_group_int(p, group_of, &group_int));
    uint32_t gsize[16] = {}, Na = 0;
    for (uint32_t g = 0; g < K; g++) Na += gsize[g] = group_size[g];
    scratch_layout lay;
    const uint64_t o_words = lay.add(PS_DIFF_WORDS * 8, 16), o_gsize = lay.add(sizeof gsize, 16), o_gint = lay.add((uint64_t)N * 4, 16);
    const uint64_t o_frag = lay.add((uint64_t)nchunks * 1024, 16);
    const uint64_t o_within = lay.add(sites ? (uint64_t)rows * 4 : 0, 16), o_total = lay.add(sites ? (uint64_t)rows * 4 : 0, 16);
    const uint64_t o_counts = lay.add(store ? (uint64_t)rows * K * 16 : 0, 16);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(p->ro[PS_RO_DIFF], lay.bytes, &base, "cannot allocate the %llu bytes of the membership tables and the per-group counts of %u sites in %u groups",
                      rows, K));
    hipStream_t st = p->stream;
    unsigned long long *d_words = (unsigned long long *)(base + o_words);
    uint32_t *d_gsize = (uint32_t *)(base + o_gsize), *d_gint = (uint32_t *)(base + o_gint);
    uint32_t *d_within = (uint32_t *)(base + o_within), *d_total = (uint32_t *)(base + o_total), *d_counts = (uint32_t *)(base + o_counts);
    uint4 *d_frag = (uint4 *)(base + o_frag);
    HIPCHK(hipMemsetAsync(d_words, 0, PS_DIFF_WORDS * 8, st));
    HIPCHK(hipMemcpyAsync(d_gsize, gsize, sizeof gsize, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_gint, group_int.data(), (uint64_t)N * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));        // (the two sources are this function's own)
    PSCHK(tm.timed(0, st, [&]() -> int {
        group_fragments_kernel<<<(nchunks * 64u + 255u) / 256u, 256, 0, st>>>(d_gint, N, nchunks, d_frag);
        HIPCHK(hipGetLastError());
        return PS_OK;
    }));
    if (rows) {
        // the fragments in LDS while they (beside the static words) leave a CU room for several workgroups
        const uint32_t lds = nchunks * 1024u <= 65536u ? nchunks * 1024u : 0u;
        const uint32_t threads = lds > 16384u ? 1024u : 256u, wpb = threads / 64u, ntiles = (rows + 15u) / 16u;
        const uint32_t per_cu = std::max(1u, std::min(2048u / threads, (160u * 1024u) / (lds + 4096u)));
        const uint32_t grid = std::max(1u, std::min((ntiles + wpb - 1u) / wpb, 256u * per_cu));
        auto kern = store ? (sites ? core_group_counts_kernel<true, true> : core_group_counts_kernel<true, false>)
                          : (sites ? core_group_counts_kernel<false, true> : core_group_counts_kernel<false, false>);
        if (lds > 32768u) HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        PSCHK(tm.timed(1, st, [&]() -> int {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, (const uint8_t *)p->state, p->pitch, rows, K, (const uint4 *)d_frag,
                               lds ? nchunks : 0u, (const uint32_t *)d_gsize, Na, d_words, d_within, d_total, d_counts);
            HIPCHK(hipGetLastError());
            return PS_OK;
        }));
    }
    HIPCHK(hipMemcpyAsync(words, d_words, PS_DIFF_WORDS * 8, hipMemcpyDeviceToHost, st));
    if (rows && o.site_within) HIPCHK(hipMemcpyAsync(o.site_within, d_within, (uint64_t)rows * 4, hipMemcpyDeviceToHost, st));
    if (rows && o.site_total) HIPCHK(hipMemcpyAsync(o.site_total, d_total, (uint64_t)rows * 4, hipMemcpyDeviceToHost, st));
    if (rows && store) HIPCHK(hipMemcpyAsync(o.counts, d_counts, (uint64_t)rows * K * 16, hipMemcpyDeviceToHost, st));
    return PS_OK;
}

// the gene pass on the accessory handle's stream, timed into group 2: gene_counts[G x K] on the host once it is synchronised
static int diff_gene_launch(ps_population *acc, event_timer &tm, const uint32_t *group_of, uint32_t K, uint32_t *gene_counts)
{
    const acc_dims d = acc->d;
    if (d.G == 0) return PS_OK;
    PSCHK(use_device(acc));
    std::vector<uint32_t> group_int;
    PSCHK(diff_group_int(acc, group_of, &group_int));
    scratch_layout lay;
    const uint64_t o_gint = lay.add((uint64_t)d.N * 4, 16), o_masks = lay.add((uint64_t)K * d.W * 8, 16), o_gc = lay.add((uint64_t)d.G * K * 4, 16);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(acc->ro[PS_RO_DIFF], lay.bytes, &base, "cannot allocate the %llu bytes of the group masks and the counts of %u genes in %u groups",
                      d.G, K));
    hipStream_t st = acc->stream;
    uint32_t *d_gint = (uint32_t *)(base + o_gint), *d_gc = (uint32_t *)(base + o_gc);
    unsigned long long *d_masks = (unsigned long long *)(base + o_masks);
    HIPCHK(hipMemcpyAsync(d_gint, group_int.data(), (uint64_t)d.N * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));        // (the source is this function's own)
    PSCHK(tm.timed(2, st, [&]() -> int {
        PSCHK(ensure_gene_major(acc, st));
        group_masks_kernel<<<(K * d.W + 255u) / 256u, 256, 0, st>>>(d_gint, d.N, d.W, K, d_masks);
        HIPCHK(hipGetLastError());
        acc_group_gene_counts_kernel<<<std::max(1u, std::min((d.G + 3u) / 4u, 2048u)), 256, 0, st>>>(acc->G[0], d_masks, d, K, d_gc);
        HIPCHK(hipGetLastError());
        return PS_OK;
    }));
    HIPCHK(hipMemcpyAsync(gene_counts, d_gc, (uint64_t)d.G * K * 4, hipMemcpyDeviceToHost, st));
    return PS_OK;
}

// the K x K matrices and the `other` cells of a handle's words, added to what the arrays hold
static uint64_t diff_words_add(const unsigned long long *w, uint32_t K, uint64_t *between, uint64_t *fixed)
{
    for (uint32_t d = 0; d < (uint32_t)PS_DIFF_ROT; d++)
        for (uint32_t g = 0; g < K; g++) {
            if (!ps_diff_keeps(g, d, K)) continue;
            const uint32_t h = (g + d) & 15u;
            between[(uint64_t)g * K + h] += w[PS_DIFF_W_DIFF + d * 16 + g];
            fixed[(uint64_t)g * K + h] += w[PS_DIFF_W_FIXED + d * 16 + g];
            if (g != h) {
                between[(uint64_t)h * K + g] += w[PS_DIFF_W_DIFF + d * 16 + g];
                fixed[(uint64_t)h * K + g] += w[PS_DIFF_W_FIXED + d * 16 + g];
            }
        }
    uint64_t other = 0;
    for (uint32_t g = 0; g < K; g++) other += w[PS_DIFF_W_OTHER + g];
    return other;
}

static int diff_handles(const ps_population *core, const ps_population *acc, const char *call)
{
    if (!core->cfg.core) return ps_fail(PS_ERR_INVALID, "%s takes a core handle first", call);
    if (acc && acc->cfg.core) return ps_fail(PS_ERR_INVALID, "%s takes an accessory handle (or NULL) second", call);
    if (acc && core->cfg.pop_size != acc->cfg.pop_size)
        return ps_fail(PS_ERR_INVALID, "%s: the core handle holds %llu individuals, the accessory handle %llu", call,
                       (unsigned long long)core->cfg.pop_size, (unsigned long long)acc->cfg.pop_size);
    if (acc && core->device != acc->device) return ps_fail(PS_ERR_INVALID, "%s: the two handles live on different devices", call);
    if (core->cfg.pop_size > 65536)
        return ps_fail(PS_ERR_INVALID, "%s needs pop_size <= 65536, not %llu", call, (unsigned long long)core->cfg.pop_size);
    return PS_OK;
}

// The call behind the three device entries.  m == nullptr: `core` answers for its own sites; else every shard's core handle
// does and the results add (core, acc: shard 0's handles).  Genes: from `acc` when a gene output is asked for.
static int diff_run(ps_multi *m, ps_population *core, ps_population *acc, const uint32_t *labels, const ps_diff_params *prm, ps_diff_t *out,
                    uint32_t *group_of, uint32_t *group_label, uint32_t *group_size, const diff_outputs &o)
{
    const char *call = m ? "ps_multi_group_differentiation" : "ps_group_differentiation";
    PSCHK(diff_handles(core, acc, call));
    PSCHK(diff_check_params(prm));
    if (!m && acc && core->cfg.ncols != core->cfg.global_cols)
        return ps_fail(PS_ERR_INVALID, "%s: this core handle is one site shard ([%llu, %llu) of %llu sites): with an accessory handle use "
                                       "ps_multi_group_differentiation", call, (unsigned long long)core->cfg.col_offset,
                       (unsigned long long)(core->cfg.col_offset + core->cfg.ncols), (unsigned long long)core->cfg.global_cols);
    if (o.genes() && !acc) return ps_fail(PS_ERR_INVALID, "%s: the gene outputs need the accessory handle", call);
    const uint64_t N = core->cfg.pop_size;
    uint32_t K = 0;
    PSCHK(ps_groups_from_labels(labels, N, prm->max_groups, prm->min_size, group_of, group_label, group_size, &K));
    memset(o.between, 0, (uint64_t)K * K * sizeof(uint64_t));
    memset(o.fixed, 0, (uint64_t)K * K * sizeof(uint64_t));
    // everything queued on either handle precedes the passes of both (as pair_source_open orders the all-pairs read-outs)
    if (m) {
        PSCHK(ps_multi_sync(m));
    } else {
        PSCHK(use_device(core));
        if (acc) HIPCHK(hipStreamSynchronize(acc->stream));
        HIPCHK(hipStreamSynchronize(core->stream));
    }
    const size_t S = m ? m->shard.size() : 1;
    const uint64_t G = acc ? acc->d.G : 0;
    std::vector<std::vector<unsigned long long>> words(S, std::vector<unsigned long long>(PS_DIFF_WORDS));
    std::vector<uint32_t> gc_own;
    uint32_t *gc = o.gene_counts;
    if (o.genes() && !gc) {
        gc_own.resize(std::max<uint64_t>(G * K, 1));
        gc = gc_own.data();
    }
    auto shard_pass = [&](size_t k) -> int {
        ps_population *c = m ? m->shard[k]->core : core;
        const uint64_t off = m ? c->cfg.col_offset : 0;
        diff_outputs part = o;
        if (part.site_within) part.site_within += off;
        if (part.site_total) part.site_total += off;
        if (part.counts) part.counts += off * K * 4;
        event_timer tm;
        readout_slot &ro = c->ro[PS_RO_DIFF];
        ro.timed = false;
        PSCHK(diff_core_launch(c, tm, group_of, K, group_size, words[k].data(), part));
        if (k == 0 && o.genes()) {
            PSCHK(diff_gene_launch(acc, tm, group_of, K, gc));
            PSCHK(use_device(c));
            HIPCHK(hipStreamSynchronize(acc->stream));
        }
        HIPCHK(hipStreamSynchronize(c->stream));
        return tm.collect(ro, 3);
    };
    if (m) PSCHK(multi_for_each(m, shard_pass));
    else PSCHK(shard_pass(0));
    uint64_t other = 0;
    for (size_t k = 0; k < S; k++) other += diff_words_add(words[k].data(), K, o.between, o.fixed);
    if (o.genes()) diff_gene_results(gc, G, K, group_size, o);
    diff_summary(out, N, m ? m->prm.core_size : core->cfg.ncols, G, K, group_size, o.between, other);
    return PS_OK;
}

#define PS_DIFF_OUTPUTS { between, fixed, site_within, site_total, counts, gene_counts, acc_between, gene_fixed, gene_private }

extern "C" int ps_group_differentiation(ps_population *core, ps_population *acc, const uint32_t *labels, const ps_diff_params *prm, ps_diff_t *out,
                                        uint32_t *group_of, uint32_t *group_label, uint32_t *group_size, uint64_t *between, uint64_t *fixed,
                                        uint32_t *site_within, uint32_t *site_total, uint32_t *counts, uint32_t *gene_counts,
                                        uint64_t *acc_between, uint64_t *gene_fixed, uint64_t *gene_private)
{
    PSCHK(ps_needs_device());
    if (!core || !labels || !prm || !out || !group_of || !group_label || !group_size || !between || !fixed)
        return ps_fail(PS_ERR_INVALID, "null argument");
    return diff_run(nullptr, core, acc, labels, prm, out, group_of, group_label, group_size, PS_DIFF_OUTPUTS);
}

extern "C" int ps_sim_group_differentiation(ps_sim *s, const uint32_t *labels, const ps_diff_params *prm, ps_diff_t *out, uint32_t *group_of,
                                            uint32_t *group_label, uint32_t *group_size, uint64_t *between, uint64_t *fixed,
                                            uint32_t *site_within, uint32_t *site_total, uint32_t *counts, uint32_t *gene_counts,
                                            uint64_t *acc_between, uint64_t *gene_fixed, uint64_t *gene_private)
{
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    return ps_group_differentiation(s->core, s->acc, labels, prm, out, group_of, group_label, group_size, between, fixed, site_within,
                                    site_total, counts, gene_counts, acc_between, gene_fixed, gene_private);
}

extern "C" int ps_multi_group_differentiation(ps_multi *m, const uint32_t *labels, const ps_diff_params *prm, ps_diff_t *out, uint32_t *group_of,
                                              uint32_t *group_label, uint32_t *group_size, uint64_t *between, uint64_t *fixed,
                                              uint32_t *site_within, uint32_t *site_total, uint32_t *counts, uint32_t *gene_counts,
                                              uint64_t *acc_between, uint64_t *gene_fixed, uint64_t *gene_private)
{
    PSCHK(ps_needs_device());
    if (!m || !labels || !prm || !out || !group_of || !group_label || !group_size || !between || !fixed)
        return ps_fail(PS_ERR_INVALID, "null argument");
    if (m->shard.size() == 1)
        return ps_sim_group_differentiation(m->shard[0], labels, prm, out, group_of, group_label, group_size, between, fixed, site_within,
                                            site_total, counts, gene_counts, acc_between, gene_fixed, gene_private);
    return diff_run(m, m->shard[0]->core, m->shard[0]->acc, labels, prm, out, group_of, group_label, group_size, PS_DIFF_OUTPUTS);
}

#undef PS_DIFF_OUTPUTS

extern "C" int ps_group_differentiation_timing(ps_population *core, double *members_ms, double *core_ms, double *genes_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_DIFF], "no group differentiation has been computed on this handle", { members_ms, core_ms, genes_ms });
}
