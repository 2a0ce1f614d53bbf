// pair_histogram.h -- ps_distance_histogram / ps_sim_distance_histogram / ps_multi_distance_histogram and the host
// restatement ps_histogram_from_counts (include/pansim_hip.h; the definitions: docs/DISTANCE_HISTOGRAM.md).  Included by
// pansim_capi.hip behind pair_readout.h, whose pair-list reader, band pipeline (pair_source_open, pair_pipeline) and entry
// bodies it reuses.
//
// Both count phases run in INTERNAL row order (no row slot): the set of unordered pairs does not change under one
// permutation applied to both matrices, and inside a simulation the two matrices hold the same individuals in the same
// internal order, so none of the row mapping of DESIGN.md 3.5 is needed.  Per band of rows (core_band_source; pair_pipeline
// orders the streams): the core numerators (the FP4 contraction for one-hot matrices, core_band_counts_simple otherwise;
// summed over the site shards of a run) on the core stream, the accessory intersections of the same rows
// (acc_intersections_band) on the accessory stream, then pair_hist_kernel on the core stream behind both.
#pragma once

#include "pair_hist_kernels.h"

#define PS_PH_MAX_BINS 16384u      // 64 KB of u32 bins in LDS per workgroup

static int pair_hist_check_params(const ps_pair_hist_params *prm)
{
    if (prm->core_bins < 1 || prm->acc_bins < 1) return ps_fail(PS_ERR_INVALID, "core_bins and acc_bins must be >= 1");
    if ((uint64_t)prm->core_bins * prm->acc_bins > PS_PH_MAX_BINS)
        return ps_fail(PS_ERR_INVALID, "core_bins x acc_bins = %llu exceeds the limit of %u bins (64 KB of LDS per workgroup)",
                       (unsigned long long)prm->core_bins * prm->acc_bins, PS_PH_MAX_BINS);
    return PS_OK;
}

static ps_ph_args pair_hist_args(const ps_pair_hist_params *prm, uint64_t S, uint64_t cg)
{
    ps_ph_args a;
    a.Bc = prm->core_bins;
    a.Ba = prm->acc_bins;
    a.S = S;
    a.cg = cg;
    a.c_scale = (float)((double)prm->core_bins / (double)S);
    a.cg_f = (float)cg;
    return a;
}

static void pair_hist_finish(ps_pair_hist_t *o, const unsigned long long *w)
{
    o->undefined_pairs = w[PS_PH_UNDEF];
    o->core_clamped = w[PS_PH_CLAMP];
    o->core_d_min = w[PS_PH_MIN];
    o->core_d_max = w[PS_PH_MAX];
    o->core_d_sum = w[PS_PH_SUM];
    const unsigned __int128 sq = (unsigned __int128)w[PS_PH_SQ0] + ((unsigned __int128)w[PS_PH_SQ1] << 32)
                                 + ((unsigned __int128)w[PS_PH_SQ2] << 64);
    o->core_d_sqsum_lo = (uint64_t)sq;
    o->core_d_sqsum_hi = (uint64_t)(sq >> 64);
    o->mean_core_distance = (o->pairs == 0 || o->core_sites == 0) ? 0.0
        : (double)o->core_d_sum / (double)o->pairs / (double)o->core_sites;
}

extern "C" int ps_histogram_from_counts(const uint32_t *core_h, const uint32_t *acc_inter, const uint32_t *acc_union, uint64_t n_pairs,
                                        uint64_t core_sites, uint64_t core_genes, const ps_pair_hist_params *prm, ps_pair_hist_t *out,
                                        uint64_t *joint)
{
    if (!core_h || !acc_inter || !acc_union || !prm || !out || !joint) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(pair_hist_check_params(prm));
    if (n_pairs < 1) return ps_fail(PS_ERR_INVALID, "a distance histogram needs at least one pair (pop_size >= 2)");
    const pair_list pairs = { nullptr, nullptr, core_h, acc_inter, acc_union, n_pairs, 0 };
    for (uint64_t k = 0; k < n_pairs; k++) PSCHK(pairs.check_acc(k, false));
    unsigned long long w[PS_PH_WORDS] = {};
    w[PS_PH_MIN] = ~0ull;
    unsigned __int128 sq = 0;
    for (uint64_t k = 0; k < n_pairs; k++) {
        const uint64_t d = core_h[k] / 2;
        w[PS_PH_MIN] = std::min<unsigned long long>(w[PS_PH_MIN], d);
        w[PS_PH_MAX] = std::max<unsigned long long>(w[PS_PH_MAX], d);
        w[PS_PH_SUM] += d;
        sq += (unsigned __int128)d * d;
    }
    w[PS_PH_SQ0] = (uint64_t)sq & 0xffffffffull;
    w[PS_PH_SQ1] = (uint64_t)sq >> 32;
    w[PS_PH_SQ2] = (uint64_t)(sq >> 64);
    const uint64_t S = prm->core_span ? prm->core_span : w[PS_PH_MAX] + 1;
    const ps_ph_args a = pair_hist_args(prm, S, core_genes);
    memset(joint, 0, (size_t)prm->core_bins * prm->acc_bins * sizeof(uint64_t));
    for (uint64_t k = 0; k < n_pairs; k++) {
        bool clamped, undefined;
        const uint32_t bc = ps_ph_core_bin(core_h[k] / 2, a, &clamped);
        w[PS_PH_CLAMP] += clamped ? 1 : 0;
        // (unions above 2^31 / acc_bins leave the kernel's 32-bit product: the same floor in 64 bits)
        uint32_t ba = 0;
        const uint64_t b = (uint64_t)acc_union[k] + core_genes;
        undefined = b == 0;
        if (!undefined) {
            if (acc_union[k] <= (1u << 17)) ba = ps_ph_acc_bin(acc_inter[k], acc_union[k], a, &undefined);
            else ba = (uint32_t)std::min<unsigned __int128>(a.Ba - 1u, (unsigned __int128)(acc_union[k] - acc_inter[k]) * a.Ba / b);
        }
        if (undefined) w[PS_PH_UNDEF]++;
        else joint[(size_t)bc * a.Ba + ba]++;
    }
    readout_head(out, 0, n_pairs, core_sites, core_genes);
    out->core_bins = prm->core_bins;
    out->acc_bins = prm->acc_bins;
    out->core_span = S;
    pair_hist_finish(out, w);
    return PS_OK;
}

template <bool BIN, bool MOM>
static int pair_hist_launch(const pair_pipeline &pl, uint32_t lo, uint32_t nrows, const ps_ph_args &a, unsigned long long *d_ph)
{
    const uint32_t N = (uint32_t)pl.c0->cfg.pop_size;
    const uint32_t lds = BIN ? a.Bc * a.Ba * 4u : 0u;
    // (a workgroup's u32 bins cannot overflow: a band holds fewer than 2^32 pairs)
    auto kern = pair_hist_kernel<BIN, MOM>;
    dim3 grid;
    PSCHK(bin_grid((const void *)kern, N, nrows, lds, 256u, &grid));
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, pl.sc, (const uint32_t *)pl.c0->d_cdavg, pl.src.b.ld, pl.In(), pl.A.ld,
                       (const uint32_t *)pl.A.rowcnt, N, lo, nrows, a, d_ph + PS_PH_WORDS, d_ph);
    HIPCHK(hipGetLastError());
    return PS_OK;
}

// The call behind the device entries: src is open in internal order, `acc` lives on src.c0's device, both streams are idle.
static int pair_hist_device(core_band_source &src, ps_population *acc, uint64_t L, const ps_pair_hist_params *prm, ps_pair_hist_t *out,
                            uint64_t *joint)
{
    ps_population *c0 = src.c0;
    const core_davg_bands &b = src.b;
    const uint64_t N = c0->cfg.pop_size, nbins = (uint64_t)prm->core_bins * prm->acc_bins, cg = acc->cfg.core_genes;
    PSCHK(use_device(c0));
    const uint64_t need = PS_PH_WORDS + nbins;
    readout_slot &ro = c0->ro[PS_RO_HIST];
    PSCHK(dev_grow(ro.d, ro.cap, need * sizeof(unsigned long long)));
    unsigned long long *d_ph = (unsigned long long *)ro.d;
    pair_pipeline pl(src, acc);
    hipStream_t sc = pl.sc;
    HIPCHK(hipMemsetAsync(d_ph, 0, need * sizeof(unsigned long long), sc));
    HIPCHK(hipMemsetAsync(d_ph + PS_PH_MIN, 0xff, sizeof(unsigned long long), sc));
    ro.timed = false;
    PSCHK(pl.open(true));
    const bool automatic = prm->core_span == 0;
    const bool one_band = b.c_end - b.c0 <= b.band;
    uint64_t S = prm->core_span;
    auto read_span = [&]() -> int {
        unsigned long long mx = 0;
        HIPCHK(hipMemcpyAsync(&mx, d_ph + PS_PH_MAX, sizeof mx, hipMemcpyDeviceToHost, sc));
        HIPCHK(hipStreamSynchronize(sc));
        S = mx + 1;
        return PS_OK;
    };
    // timer groups: 0 = both count phases, 1 = the moments and the binning
    auto bin_band = [&](uint32_t lo, uint32_t nrows, bool moments) -> int {
        const ps_ph_args a = pair_hist_args(prm, S, cg);
        return pl.consume(1, [&]() {
            return moments ? pair_hist_launch<true, true>(pl, lo, nrows, a, d_ph) : pair_hist_launch<true, false>(pl, lo, nrows, a, d_ph);
        });
    };
    auto moments_band = [&](uint32_t lo, uint32_t nrows) -> int {
        return pl.consume(1, [&]() { return pair_hist_launch<false, true>(pl, lo, nrows, ps_ph_args{}, d_ph); });
    };
    if (!automatic) {
        PSCHK(pl.for_bands([&](uint32_t lo, uint32_t nrows) -> int {
            PSCHK(pl.core_counts(0, lo, nrows));
            PSCHK(pl.acc_counts(0, lo, nrows));
            return bin_band(lo, nrows, true);
        }));
    } else if (one_band) {
        // the automatic span over one band: the moments first, the bins from the same counts
        PSCHK(pl.core_counts(0, b.c0, b.c_end - b.c0));
        PSCHK(pl.acc_counts(0, b.c0, b.c_end - b.c0));
        PSCHK(moments_band(b.c0, b.c_end - b.c0));
        PSCHK(read_span());
        PSCHK(bin_band(b.c0, b.c_end - b.c0, false));
    } else {
        // ... over several bands: the core contraction runs twice (docs/DISTANCE_HISTOGRAM.md)
        PSCHK(pl.for_bands([&](uint32_t lo, uint32_t nrows) -> int {
            PSCHK(pl.core_counts(0, lo, nrows));
            return moments_band(lo, nrows);
        }));
        PSCHK(read_span());
        PSCHK(pl.for_bands([&](uint32_t lo, uint32_t nrows) -> int {
            PSCHK(pl.core_counts(0, lo, nrows));
            PSCHK(pl.acc_counts(0, lo, nrows));
            return bin_band(lo, nrows, false);
        }));
    }
    unsigned long long w[PS_PH_WORDS];
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the bins are copied as they are");
    HIPCHK(hipMemcpyAsync(w, d_ph, sizeof w, hipMemcpyDeviceToHost, sc));
    HIPCHK(hipMemcpyAsync(joint, d_ph + PS_PH_WORDS, nbins * sizeof(uint64_t), hipMemcpyDeviceToHost, sc));
    PSCHK(pl.finish(ro, 2));
    readout_head(out, N, N * (N - 1) / 2, L, cg);
    out->core_bins = prm->core_bins;
    out->acc_bins = prm->acc_bins;
    out->core_span = S;
    pair_hist_finish(out, w);
    return PS_OK;
}

// behind pair_entry: ps_distance_histogram (m == nullptr) and ps_multi_distance_histogram (core, acc: shard 0's handles; the
// binning -- with the halving h / 2 behind the sum over the shards -- runs on shard 0 against its accessory replica)
static auto pair_hist_entry(const ps_pair_hist_params *prm, ps_pair_hist_t *out, uint64_t *joint)
{
    return [=](ps_multi *m, ps_population *core, ps_population *acc) -> int {
        PSCHK(pair_hist_check_params(prm));
        core_band_source src;
        PSCHK(pair_source_open(&src, "distance_histogram", "a distance histogram needs", "sums", m, core, acc, true, nullptr));
        return pair_hist_device(src, acc, m ? m->prm.core_size : core->cfg.global_cols, prm, out, joint);
    };
}

extern "C" int ps_distance_histogram(ps_population *core, ps_population *acc, const ps_pair_hist_params *prm, ps_pair_hist_t *out,
                                     uint64_t *joint)
{
    return pair_entry(core, acc, prm && out && joint, pair_hist_entry(prm, out, joint));
}

extern "C" int ps_sim_distance_histogram(ps_sim *s, const ps_pair_hist_params *prm, ps_pair_hist_t *out, uint64_t *joint)
{
    return pair_entry(s, prm && out && joint, pair_hist_entry(prm, out, joint));
}

extern "C" int ps_distance_histogram_timing(ps_population *core, double *counts_ms, double *binning_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_HIST], "no distance histogram has been computed on this handle", { counts_ms, binning_ms });
}

extern "C" int ps_multi_distance_histogram(ps_multi *m, const ps_pair_hist_params *prm, ps_pair_hist_t *out, uint64_t *joint)
{
    return pair_entry(m, prm && out && joint, pair_hist_entry(prm, out, joint));
}
