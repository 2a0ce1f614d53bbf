// clock_histogram.h -- ps_sim_clock_histogram / ps_multi_clock_histogram, the host restatement ps_clock_from_counts and
// ps_clock_histogram_timing (include/pansim_hip.h; the definitions: docs/GENEALOGY.md).  Included by pansim_capi.hip behind
// genealogy.h; the pair-list reader, the metric checks and the band pipeline (pair_source_open, pair_pipeline) are those of
// pair_readout.h, the distance bins the histogram's own.
//
// Everything on the device runs in INTERNAL row order, which is the comb's order: the divergence time of a pair of band row i
// and column j is the maximum of coal[i .. j - 1], two reads of the sparse table.  Before the bands the comb and the table are
// built on the core stream; per band the numerators of the metric asked for (the other metric's count kernels are not
// launched), then pair_clock_kernel behind them.  Every sum is an integer sum.
#pragma once

#define PS_CLOCK_MAX_BINS 16384u        // 64 KB of u32 bins in LDS per workgroup
#define PS_CLOCK_MAX_TIME_BINS 1024u    // ... beside 16 bytes of sums per time row

static const metric_names CLOCK_NAMES = { "a clock histogram", "PS_KNN_CORE", "PS_KNN_ACC" };

static int clock_check_params(const ps_clock_params *prm)
{
    PSCHK(metric_check(prm->metric, CLOCK_NAMES));
    if (prm->time_bins < 1 || prm->dist_bins < 1) return ps_fail(PS_ERR_INVALID, "time_bins and dist_bins must be >= 1");
    if (prm->time_bins > PS_CLOCK_MAX_TIME_BINS)
        return ps_fail(PS_ERR_INVALID, "time_bins = %u exceeds the limit of %u time bins", prm->time_bins, PS_CLOCK_MAX_TIME_BINS);
    if (((uint64_t)prm->time_bins + 1) * prm->dist_bins > PS_CLOCK_MAX_BINS)
        return ps_fail(PS_ERR_INVALID, "(time_bins + 1) x dist_bins = %llu exceeds the limit of %u bins (64 KB of LDS per workgroup)",
                       ((unsigned long long)prm->time_bins + 1) * prm->dist_bins, PS_CLOCK_MAX_BINS);
    if (prm->time_span > 0xffffffffull)
        return ps_fail(PS_ERR_INVALID, "time_span = %llu exceeds the limit of 2^32 - 1 generations", (unsigned long long)prm->time_span);
    return PS_OK;
}

static ps_clock_args clock_args(const ps_clock_params *prm, uint64_t St, uint64_t S, uint64_t cg)
{
    ps_clock_args a;
    const ps_pair_hist_params h = { prm->dist_bins, prm->dist_bins, S };
    a.d = pair_hist_args(&h, S, cg);
    a.Bt = prm->time_bins;
    a.St = St;
    a.t_scale = (float)((double)prm->time_bins / (double)St);
    return a;
}

// joint, and per_time with its sums of num (and of den under the accessory metric) in place -> the pairs of every time row,
// the core den sums, the totals
static void clock_finish(ps_clock_t *o, const uint64_t *joint, uint64_t *per_time)
{
    const uint64_t nt = o->time_bins + 1, Bx = o->dist_bins;
    for (uint64_t bt = 0; bt < nt; bt++) {
        uint64_t n = 0;
        for (uint64_t bx = 0; bx < Bx; bx++) n += joint[bt * Bx + bx];
        per_time[3 * bt] = n;
        if (o->metric == PS_KNN_CORE) per_time[3 * bt + 2] = n * o->core_sites;
        o->binned_pairs += n;
        o->num_sum += per_time[3 * bt + 1];
        o->den_sum += per_time[3 * bt + 2];
    }
    o->beyond_pairs = per_time[3 * (nt - 1)];
}

static void clock_fill(ps_clock_t *o, uint64_t N, uint64_t pairs, uint64_t L, uint64_t cg, const ps_clock_params *prm, uint64_t St, uint64_t S,
                       uint64_t depth)
{
    readout_head(o, N, pairs, L, cg);
    o->metric = (uint64_t)prm->metric;
    o->time_bins = prm->time_bins;
    o->dist_bins = prm->dist_bins;
    o->time_span = St;
    o->core_span = prm->metric == PS_KNN_CORE ? S : 0;
    o->depth = depth;
}

extern "C" int ps_clock_from_counts(const uint32_t *tmrca, const uint32_t *core_h, const uint32_t *acc_inter, const uint32_t *acc_union,
                                    uint64_t n_pairs, uint64_t depth, uint64_t core_sites, uint64_t core_genes, const ps_clock_params *prm,
                                    ps_clock_t *out, uint64_t *joint, uint64_t *per_time)
{
    if (!tmrca || !prm || !out || !joint || !per_time) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(clock_check_params(prm));
    const bool acc = prm->metric == PS_KNN_ACC;
    const pair_list pairs = { nullptr, nullptr, core_h, acc_inter, acc_union, n_pairs, 0 };
    if (pairs.lacks(!acc, acc)) return ps_fail(PS_ERR_INVALID, "null argument: the metric needs its numerators");
    PSCHK(metric_check_core_genes(prm->metric, core_genes, CLOCK_NAMES));
    if (n_pairs < 1) return ps_fail(PS_ERR_INVALID, "a clock histogram needs at least one pair (pop_size >= 2)");
    if (depth < 1 || depth > 0xfffffffeull) return ps_fail(PS_ERR_INVALID, "a clock histogram needs 1 <= depth < 2^32 - 1 recorded generations, not %llu", (unsigned long long)depth);
    uint64_t d_max = 0;
    for (uint64_t p = 0; p < n_pairs; p++) {
        if (tmrca[p] != PS_GEN_BEYOND && (tmrca[p] < 1 || tmrca[p] > depth))
            return ps_fail(PS_ERR_INVALID, "pair %llu: a divergence time is 1 .. depth = %llu or PS_GEN_BEYOND, not %u", (unsigned long long)p,
                           (unsigned long long)depth, tmrca[p]);
        if (acc) PSCHK(pairs.check_acc(p, true));
        if (!acc) d_max = std::max<uint64_t>(d_max, core_h[p] / 2);
    }
    const uint64_t St = prm->time_span ? prm->time_span : depth, S = acc ? 1 : prm->core_span ? prm->core_span : d_max + 1;
    const ps_clock_args a = clock_args(prm, St, S, core_genes);
    const uint64_t nt = (uint64_t)prm->time_bins + 1, Bx = prm->dist_bins;
    memset(joint, 0, nt * Bx * sizeof(uint64_t));
    memset(per_time, 0, 3 * nt * sizeof(uint64_t));
    clock_fill(out, 0, n_pairs, core_sites, core_genes, prm, St, S, depth);
    for (uint64_t p = 0; p < n_pairs; p++) {
        const uint32_t bt = tmrca[p] == PS_GEN_BEYOND ? a.Bt : ps_clock_time_bin(tmrca[p], a.Bt, a.St, a.t_scale);
        uint32_t bx;
        if (acc) {
            bool undefined;
            bx = ps_ph_acc_bin(acc_inter[p], acc_union[p], a.d, &undefined);
            if (undefined) {
                out->undefined_pairs++;
                continue;
            }
            per_time[3 * bt + 1] += acc_union[p] - acc_inter[p];
            per_time[3 * bt + 2] += (uint64_t)acc_union[p] + core_genes;
        } else {
            bool clamped;
            bx = ps_ph_core_bin(core_h[p] / 2, a.d, &clamped);
            out->core_clamped += clamped ? 1 : 0;
            per_time[3 * bt + 1] += core_h[p] / 2;
        }
        joint[(uint64_t)bt * Bx + bx]++;
    }
    clock_finish(out, joint, per_time);
    return PS_OK;
}

template <bool ACC>
static int clock_launch(const pair_pipeline &pl, uint32_t lo, uint32_t nrows, const ps_clock_args &a, const uint32_t *table,
                        unsigned long long *words, unsigned long long *sums, unsigned long long *joint)
{
    const uint32_t N = (uint32_t)pl.c0->cfg.pop_size;
    const uint32_t nt = a.Bt + 1u, lds = nt * a.d.Bc * 4u + nt * 16u;
    auto kern = pair_clock_kernel<ACC>;
    dim3 grid;
    PSCHK(bin_grid((const void *)kern, N, nrows, lds, 256u, &grid));
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, pl.sc, (const uint32_t *)pl.c0->d_cdavg, pl.src.b.ld, pl.In(), pl.A.ld,
                       (const uint32_t *)pl.A.rowcnt, table, N, lo, nrows, a, words, sums, joint);
    HIPCHK(hipGetLastError());
    return PS_OK;
}

// The call behind the device entries: src holds the bands (open in internal order with the core metric), `s` is the simulation
// whose record is read (src.c0 is its core handle), both streams are idle and every copy into the log is complete.
static int clock_device(core_band_source &src, ps_sim *s, uint64_t L, const ps_clock_params *prm, ps_clock_t *out, uint64_t *joint,
                        uint64_t *per_time)
{
    ps_population *c0 = src.c0, *acc = s->acc;
    const core_davg_bands &b = src.b;
    const uint32_t N = (uint32_t)c0->cfg.pop_size;
    const uint64_t cg = acc->cfg.core_genes, nt = (uint64_t)prm->time_bins + 1, nbins = nt * prm->dist_bins;
    const bool acc_metric = prm->metric == PS_KNN_ACC;
    const uint64_t depth = std::min<uint64_t>(s->anc_written, s->anc_capacity);
    if (depth > 0xfffffffeull) return ps_fail(PS_ERR_INVALID, "a clock histogram needs depth < 2^32 - 1 recorded generations");
    PSCHK(metric_check_core_genes(prm->metric, cg, CLOCK_NAMES));
    PSCHK(use_device(c0));
    const uint32_t levels = gen_levels(N);
    const uint64_t n_words = PS_CK_WORDS + 2 * nt + nbins;
    uint32_t *table = nullptr;
    void *tail = nullptr;
    PSCHK(gen_scratch_get(c0, N, levels, n_words * sizeof(unsigned long long), &table, &tail));
    unsigned long long *words = (unsigned long long *)tail, *sums = words + PS_CK_WORDS, *d_joint = sums + 2 * nt;
    pair_pipeline pl(src, acc);
    hipStream_t sc = pl.sc;
    readout_slot &ro = c0->ro[PS_RO_GEN];
    ro.timed = false;
    HIPCHK(hipMemsetAsync(words, 0, n_words * sizeof(unsigned long long), sc));
    // timer groups: 0 = the count phase, 1 = the comb, the table and the binning
    PSCHK(pl.timed(1, sc, [&]() -> int {
        PSCHK(gen_comb_launch(s, table, sc));
        for (uint32_t k = 1; k < levels; k++)
            ancestry_table_kernel<<<(N - 1 + 255) / 256, 256, 0, sc>>>(table + (uint64_t)(k - 1) * N, table + (uint64_t)k * N, N - 1, 1u << (k - 1));
        HIPCHK(hipGetLastError());
        return PS_OK;
    }));
    PSCHK(pl.open(acc_metric));
    const uint64_t St = prm->time_span ? prm->time_span : depth;
    uint64_t S = acc_metric ? 1 : prm->core_span;
    auto bin_band = [&](uint32_t lo, uint32_t nrows) -> int {
        const ps_clock_args a = clock_args(prm, St, S, cg);
        return pl.consume(1, [&]() {
            return acc_metric ? clock_launch<true>(pl, lo, nrows, a, table, words, sums, d_joint) : clock_launch<false>(pl, lo, nrows, a, table, words, sums, d_joint);
        });
    };
    if (acc_metric) {
        PSCHK(pl.for_bands([&](uint32_t lo, uint32_t nrows) -> int {
            PSCHK(pl.acc_counts(0, lo, nrows));
            return bin_band(lo, nrows);
        }));
    } else if (S) {
        PSCHK(pl.for_bands([&](uint32_t lo, uint32_t nrows) -> int {
            PSCHK(pl.core_counts(0, lo, nrows));
            return bin_band(lo, nrows);
        }));
    } else {
        // the automatic span, as the histogram finds it: the moments pass of pair_hist_kernel into the histogram's own words
        // first; over one band the bins come from the same counts, over several the core contraction runs twice
        readout_slot &hist = c0->ro[PS_RO_HIST];
        PSCHK(dev_grow(hist.d, hist.cap, PS_PH_WORDS * sizeof(unsigned long long)));
        unsigned long long *d_ph = (unsigned long long *)hist.d;
        HIPCHK(hipMemsetAsync(d_ph, 0, PS_PH_WORDS * sizeof(unsigned long long), sc));
        HIPCHK(hipMemsetAsync(d_ph + PS_PH_MIN, 0xff, sizeof(unsigned long long), sc));
        const bool one_band = b.c_end - b.c0 <= b.band;
        PSCHK(pl.for_bands([&](uint32_t lo, uint32_t nrows) -> int {
            PSCHK(pl.core_counts(0, lo, nrows));
            return pl.consume(1, [&]() { return pair_hist_launch<false, true>(pl, lo, nrows, ps_ph_args{}, d_ph); });
        }));
        unsigned long long mx = 0;
        HIPCHK(hipMemcpyAsync(&mx, d_ph + PS_PH_MAX, sizeof mx, hipMemcpyDeviceToHost, sc));
        HIPCHK(hipStreamSynchronize(sc));
        S = mx + 1;
        PSCHK(pl.for_bands([&](uint32_t lo, uint32_t nrows) -> int {
            if (!one_band) PSCHK(pl.core_counts(0, lo, nrows));
            return bin_band(lo, nrows);
        }));
    }
    unsigned long long w[PS_CK_WORDS];
    std::vector<unsigned long long> hs(2 * nt);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the bins are copied as they are");
    HIPCHK(hipMemcpyAsync(w, words, sizeof w, hipMemcpyDeviceToHost, sc));
    HIPCHK(hipMemcpyAsync(hs.data(), sums, 2 * nt * sizeof(unsigned long long), hipMemcpyDeviceToHost, sc));
    HIPCHK(hipMemcpyAsync(joint, d_joint, nbins * sizeof(uint64_t), hipMemcpyDeviceToHost, sc));
    PSCHK(pl.finish(ro, 2));
    clock_fill(out, N, (uint64_t)N * (N - 1) / 2, L, cg, prm, St, S, depth);
    out->undefined_pairs = w[PS_CK_UNDEF];
    out->core_clamped = w[PS_CK_CLAMP];
    for (uint64_t bt = 0; bt < nt; bt++) {
        per_time[3 * bt] = 0;
        per_time[3 * bt + 1] = hs[2 * bt];
        per_time[3 * bt + 2] = hs[2 * bt + 1];
    }
    clock_finish(out, joint, per_time);
    return PS_OK;
}

// ps_sim_clock_histogram (m == nullptr) and ps_multi_clock_histogram (s: shard 0, which holds the record; the binning on shard 0
// against its accessory replica)
static int clock_entry(ps_multi *m, ps_sim *s, const ps_clock_params *prm, ps_clock_t *out, uint64_t *joint, uint64_t *per_time)
{
    PSCHK(clock_check_params(prm));
    PSCHK(gen_recording(s, m ? "ps_multi_clock_histogram" : "ps_sim_clock_histogram", true));
    core_band_source src;
    PSCHK(pair_source_open(&src, "clock_histogram", "a clock histogram needs", "bins", m, s->core, s->acc, prm->metric == PS_KNN_CORE, nullptr));
    return clock_device(src, s, m ? m->prm.core_size : s->core->cfg.global_cols, prm, out, joint, per_time);
}

extern "C" int ps_sim_clock_histogram(ps_sim *s, const ps_clock_params *prm, ps_clock_t *out, uint64_t *joint, uint64_t *per_time)
{
    PSCHK(ps_needs_device());
    if (!s || !prm || !out || !joint || !per_time) return ps_fail(PS_ERR_INVALID, "null argument");
    return clock_entry(nullptr, s, prm, out, joint, per_time);
}

extern "C" int ps_multi_clock_histogram(ps_multi *m, const ps_clock_params *prm, ps_clock_t *out, uint64_t *joint, uint64_t *per_time)
{
    PSCHK(ps_needs_device());
    if (!m || !prm || !out || !joint || !per_time) return ps_fail(PS_ERR_INVALID, "null argument");
    if (m->shard.size() == 1) return ps_sim_clock_histogram(m->shard[0], prm, out, joint, per_time);
    return clock_entry(m, m->shard[0], prm, out, joint, per_time);
}

extern "C" int ps_clock_histogram_timing(ps_population *core, double *counts_ms, double *binning_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_GEN], "no clock histogram has been computed on this handle", { counts_ms, binning_ms });
}
