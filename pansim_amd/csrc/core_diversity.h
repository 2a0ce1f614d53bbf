// core_diversity.h -- ps_site_allele_counts / ps_core_diversity / ps_diversity_from_counts and their ps_multi forms
// (include/pansim_hip.h; the definitions: docs/CORE_DIVERSITY.md).  Included by pansim_capi.hip behind struct ps_multi.
//
// Column sums do not depend on the row order, so none of the row mapping of DESIGN.md 3.5 is needed: the kernel reads
// p->state as it is, on the handle's stream -- behind every queued generation, a two-generation sweep launch included (the
// sweeps swap state / state2 on the host when they are enqueued).
#pragma once

#include "diversity_kernels.h"

static int diversity_core_handle(const ps_population *p, const char *call)
{
    if (!p->cfg.core)
        return ps_fail(PS_ERR_INVALID, "%s runs on the core matrix; the accessory counterpart is ps_gene_frequencies", call);
    return PS_OK;
}

static void diversity_mean(ps_core_diversity_t *o)
{
    const uint64_t N = o->pop_size;
    o->mean_pairwise_distance = (N < 2 || o->sites == 0) ? 0.0
        : (double)o->pair_differences / (double)(N * (N - 1) / 2) / (double)o->sites;
}

// One pass over the handle's rows on `st`: STORE leaves the ncols x 4 counts in p->d_site_counts, SUMMARY the PS_DIV_WORDS
// summary words followed by the N + 1 spectrum bins in p->d_div.  Two events around the launch time it
// (ps_core_diversity_timing).
template <bool STORE, bool SUMMARY>
static int launch_site_counts(ps_population *p, hipStream_t st)
{
    const uint32_t N = (uint32_t)p->cfg.pop_size, rows = (uint32_t)p->cfg.ncols;
    if (STORE && !p->d_site_counts) HIPCHK(hipMalloc(&p->d_site_counts, std::max<uint64_t>(rows, 1) * 4 * sizeof(uint32_t)));
    const uint64_t div_bytes = ((uint64_t)PS_DIV_WORDS + N + 1) * sizeof(unsigned long long);
    if (SUMMARY) {
        if (!p->d_div) HIPCHK(hipMalloc(&p->d_div, div_bytes));
        HIPCHK(hipMemsetAsync(p->d_div, 0, div_bytes, st));
    }
    for (hipEvent_t &e : p->div_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    p->div_timed = false;
    if (rows == 0) return PS_OK;
    // the spectrum in an LDS histogram per workgroup while its N + 1 bins (beside the static summary words) fit
    uint32_t bins = 0;
    if (SUMMARY && ((uint64_t)N + 1) * 4 + 256 <= p->lds_limit) bins = N + 1;
    const uint32_t lds = bins * 4u;
    // (a histogram that leaves room for few workgroups per CU: wide ones, so that the CU still holds 16 waves or more)
    const uint32_t threads = lds > 16384u ? 1024u : 256u, wpb = threads / 64u;
    const uint32_t per_cu = std::max(1u, std::min(2048u / threads, (160u * 1024u) / (lds + 256u)));
    const uint32_t grid = std::max(1u, std::min((rows + wpb - 1u) / wpb, 256u * per_cu));
    auto kern = core_site_counts_kernel<STORE, SUMMARY>;
    if (lds > 32768u) HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPCHK(hipEventRecord(p->div_ev[0], st));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, (const uint8_t *)p->state, p->pitch, N, rows, p->d_site_counts,
                       p->d_div, p->d_div ? p->d_div + PS_DIV_WORDS : nullptr, bins);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->div_ev[1], st));
    p->div_timed = true;
    return PS_OK;
}

extern "C" int ps_site_allele_counts(ps_population *p, uint32_t *counts)
{
    PSCHK(ps_needs_device());
    if (!p || !counts) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(diversity_core_handle(p, "ps_site_allele_counts"));
    PSCHK(use_device(p));
    PSCHK((launch_site_counts<true, false>(p, p->stream)));
    if (p->cfg.ncols)
        HIPCHK(hipMemcpyAsync(counts, p->d_site_counts, p->cfg.ncols * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return PS_OK;
}

extern "C" int ps_core_diversity(ps_population *p, ps_core_diversity_t *out, uint64_t *spectrum)
{
    PSCHK(ps_needs_device());
    if (!p || !out) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(diversity_core_handle(p, "ps_core_diversity"));
    PSCHK(use_device(p));
    PSCHK((launch_site_counts<false, true>(p, p->stream)));
    const uint64_t N = p->cfg.pop_size;
    unsigned long long w[PS_DIV_WORDS];
    HIPCHK(hipMemcpyAsync(w, p->d_div, sizeof w, hipMemcpyDeviceToHost, p->stream));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the spectrum is copied as it is");
    if (spectrum) HIPCHK(hipMemcpyAsync(spectrum, p->d_div + PS_DIV_WORDS, (N + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    memset(out, 0, sizeof *out);
    out->pop_size = N;
    out->sites = p->cfg.ncols;
    out->pair_differences = w[PS_DIV_PAIR];
    out->segregating_sites = w[PS_DIV_SEG];
    out->other_cells = w[PS_DIV_OTHER];
    for (int a = 0; a < 4; a++) out->base_cells[a] = w[PS_DIV_BASE + a];
    diversity_mean(out);
    return PS_OK;
}

extern "C" int ps_core_diversity_timing(ps_population *p, double *kernel_ms)
{
    if (!p || !kernel_ms) return ps_fail(PS_ERR_INVALID, "null argument");
    if (!p->div_timed) return ps_fail(PS_ERR_STATE, "no counts kernel has been launched on this handle");
    PSCHK(use_device(p));
    float ms = 0.0f;
    HIPCHK(hipEventSynchronize(p->div_ev[1]));
    HIPCHK(hipEventElapsedTime(&ms, p->div_ev[0], p->div_ev[1]));
    *kernel_ms = (double)ms;
    return PS_OK;
}

extern "C" int ps_diversity_from_counts(const uint32_t *counts, uint64_t sites, uint64_t pop_size, ps_core_diversity_t *out,
                                        uint64_t *spectrum)
{
    if (!out || (!counts && sites)) return ps_fail(PS_ERR_INVALID, "null argument");
    if (pop_size < 1 || pop_size > 0xFFFFFFFFull - 128) return ps_fail(PS_ERR_INVALID, "pop_size must be 1 .. 2^32 - 129");
    memset(out, 0, sizeof *out);
    out->pop_size = pop_size;
    out->sites = sites;
    if (spectrum) memset(spectrum, 0, (pop_size + 1) * sizeof(uint64_t));
    for (uint64_t s = 0; s < sites; s++) {
        const uint32_t *n = counts + 4 * s;
        if ((uint64_t)n[0] + n[1] + n[2] + n[3] > pop_size)
            return ps_fail(PS_ERR_INVALID, "the counts of site %llu add up to more than pop_size %llu", (unsigned long long)s,
                           (unsigned long long)pop_size);
        uint64_t pair, other, minor;
        uint32_t seg;
        ps_div_site_terms(pop_size, n[0], n[1], n[2], n[3], &pair, &seg, &other, &minor);
        out->pair_differences += pair;
        out->segregating_sites += seg;
        out->other_cells += other;
        for (int a = 0; a < 4; a++) out->base_cells[a] += n[a];
        if (spectrum) spectrum[minor]++;
    }
    diversity_mean(out);
    return PS_OK;
}

// The shards hold disjoint runs of the core sites in order: their counts concatenate, their integers and spectra add, and
// the double is formed once over core_size.
extern "C" int ps_multi_site_allele_counts(ps_multi *m, uint32_t *counts)
{
    PSCHK(ps_needs_device());
    if (!m || !counts) return ps_fail(PS_ERR_INVALID, "null argument");
    return multi_for_each(m, [&](size_t k) {
        ps_population *c = m->shard[k]->core;
        return ps_site_allele_counts(c, counts + 4 * c->cfg.col_offset);
    });
}

extern "C" int ps_multi_core_diversity(ps_multi *m, ps_core_diversity_t *out, uint64_t *spectrum)
{
    PSCHK(ps_needs_device());
    if (!m || !out) return ps_fail(PS_ERR_INVALID, "null argument");
    const size_t K = m->shard.size();
    const uint64_t bins = m->prm.pop_size + 1;
    std::vector<ps_core_diversity_t> part(K);
    std::vector<uint64_t> spec(spectrum ? K * bins : 0);
    PSCHK(multi_for_each(m, [&](size_t k) {
        return ps_core_diversity(m->shard[k]->core, &part[k], spectrum ? spec.data() + k * bins : nullptr);
    }));
    memset(out, 0, sizeof *out);
    out->pop_size = m->prm.pop_size;
    if (spectrum) memset(spectrum, 0, bins * sizeof(uint64_t));
    for (size_t k = 0; k < K; k++) {
        out->sites += part[k].sites;
        out->other_cells += part[k].other_cells;
        out->segregating_sites += part[k].segregating_sites;
        out->pair_differences += part[k].pair_differences;
        for (int a = 0; a < 4; a++) out->base_cells[a] += part[k].base_cells[a];
        for (uint64_t b = 0; spectrum && b < bins; b++) spectrum[b] += spec[k * bins + b];
    }
    diversity_mean(out);
    return PS_OK;
}
