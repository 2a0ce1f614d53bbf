// pair_histogram.h -- ps_distance_histogram / ps_sim_distance_histogram / ps_multi_distance_histogram and the host
// restatement ps_histogram_from_counts (include/pansim_hip.h; the definitions: docs/DISTANCE_HISTOGRAM.md).  Included by
// pansim_capi.hip behind core_band_source.
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
    for (uint64_t k = 0; k < n_pairs; k++)
        if (acc_inter[k] > acc_union[k])
            return ps_fail(PS_ERR_INVALID, "pair %llu: intersection %u above union %u", (unsigned long long)k, acc_inter[k], acc_union[k]);
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
    memset(out, 0, sizeof *out);
    out->pairs = n_pairs;
    out->core_sites = core_sites;
    out->core_genes = core_genes;
    out->core_bins = prm->core_bins;
    out->acc_bins = prm->acc_bins;
    out->core_span = S;
    pair_hist_finish(out, w);
    return PS_OK;
}

static int pair_hist_handles(const ps_population *core, const ps_population *acc, const char *call, const char *what = "a distance histogram needs")
{
    if (!core->cfg.core || acc->cfg.core)
        return ps_fail(PS_ERR_INVALID, "%s takes a core handle first and an accessory handle second", call);
    if (core->cfg.pop_size != acc->cfg.pop_size)
        return ps_fail(PS_ERR_INVALID, "%s: the core handle holds %llu individuals, the accessory handle %llu", call,
                       (unsigned long long)core->cfg.pop_size, (unsigned long long)acc->cfg.pop_size);
    if (core->device != acc->device) return ps_fail(PS_ERR_INVALID, "%s: the two handles live on different devices", call);
    if (core->cfg.pop_size < 2) return ps_fail(PS_ERR_INVALID, "%s pop_size >= 2", what);
    if (acc->d.G > 65535) return ps_fail(PS_ERR_INVALID, "%s at most 65535 accessory genes (u16 intersection counts)", what);
    return PS_OK;
}

// The per-band pipeline of the all-pairs read-outs (histogram, clusters) over the core stream of src.c0 and the stream of the
// accessory handle on the same device; both idle on entry.  Per band: core_counts() on the core stream, acc_counts() on the
// accessory stream behind the last consumer that read the scratch, consume() on the core stream behind both.  Every piece of
// work is timed into a group (event_timer); finish() synchronises both streams and leaves the groups' totals in the read-out's slot.
struct pair_pipeline : event_timer {
    core_band_source &src;
    ps_population *c0, *acc;
    hipStream_t sc, sa;
    acc_padded A;                   // (all null without accessory counts: the kernels take I = U = 0)
    bool acc_on = false, consumed = false;
    hipEvent_t ev_acc = nullptr, ev_used = nullptr;

    pair_pipeline(core_band_source &s, ps_population *a) : src(s), c0(s.c0), acc(a), sc(s.c0->stream), sa(a->stream) {}
    // want_acc: the accessory counts are read at all; the padded rows and row counts on the accessory stream (G == 0: nothing)
    int open(bool want_acc)
    {
        acc_on = want_acc && acc->d.G > 0;
        if (acc_on) PSCHK(acc_rows_padded(acc, sa, &A));
        PSCHK(make(&ev_acc));
        return make(&ev_used);
    }
    const uint16_t *In() const { return acc_on ? (const uint16_t *)acc->d_davg_in : nullptr; }
    // body(lo, nrows) for every band of the source
    template <class B>
    int for_bands(B &&body)
    {
        const core_davg_bands &b = src.b;
        for (uint32_t lo = b.c0; lo < b.c_end; lo += b.band) PSCHK(body(lo, std::min(b.band, b.c_end - lo)));
        return PS_OK;
    }
    int core_counts(int group, uint32_t lo, uint32_t nrows)
    {
        return timed(group, sc, [&]() { return src.counts(lo, nrows); });
    }
    int acc_counts(int group, uint32_t lo, uint32_t nrows)
    {
        if (!acc_on) return PS_OK;
        if (consumed) HIPCHK(hipStreamWaitEvent(sa, ev_used, 0));
        // (a wave of the contraction stores 64 whole rows: the scratch's band is a multiple of 256)
        PSCHK(timed(group, sa, [&]() { return acc_intersections_band(acc, A, 2u, ((uint64_t)src.b.band + 255) & ~255ull, lo, nrows, sa); }));
        HIPCHK(hipEventRecord(ev_acc, sa));
        HIPCHK(hipStreamWaitEvent(sc, ev_acc, 0));
        return PS_OK;
    }
    template <class W>
    int consume(int group, W &&work)
    {
        PSCHK(timed(group, sc, work));
        HIPCHK(hipEventRecord(ev_used, sc));
        consumed = true;
        return PS_OK;
    }
    // the end of a read-out: everything queued on both streams complete, the first `groups` totals in its slot
    int finish(readout_slot &ro, int groups)
    {
        HIPCHK(hipStreamSynchronize(sa));
        HIPCHK(hipStreamSynchronize(sc));
        return collect(ro, groups);
    }
};

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
    memset(out, 0, sizeof *out);
    out->pop_size = N;
    out->pairs = N * (N - 1) / 2;
    out->core_sites = L;
    out->core_genes = cg;
    out->core_bins = prm->core_bins;
    out->acc_bins = prm->acc_bins;
    out->core_span = S;
    pair_hist_finish(out, w);
    return PS_OK;
}

// What the entries of the histogram and of the clusters share behind their own parameter checks, under the name ps_<name> (m ==
// nullptr: `core` must hold all sites, over which the read-out `verb`s) or ps_multi_<name> (core, acc: shard 0's handles).  The
// handles checked, `slot` (if asked for) the current row map of `core`, everything queued before the call complete, the band
// source open in internal order.
static int pair_source_open(core_band_source *src, const char *name, const char *what, const char *verb, ps_multi *m, ps_population *core,
                            ps_population *acc, bool core_counts, const uint32_t **slot)
{
    const std::string call = std::string(m ? "ps_multi_" : "ps_") + name;
    PSCHK(pair_hist_handles(core, acc, call.c_str(), what));
    if (!m && core->cfg.ncols != core->cfg.global_cols)
        return ps_fail(PS_ERR_INVALID, "%s %s over all %llu core sites; this handle is one site shard ([%llu, %llu)): use ps_multi_%s",
                       call.c_str(), verb, (unsigned long long)core->cfg.global_cols, (unsigned long long)core->cfg.col_offset,
                       (unsigned long long)(core->cfg.col_offset + core->cfg.ncols), name);
    PSCHK(use_device(core));
    if (slot) PSCHK(rows_current(core, slot));
    if (m) {
        PSCHK(ps_multi_sync(m));
    } else {
        // everything queued on either handle precedes the count kernels of both (as sim_pair_counts orders them)
        HIPCHK(hipStreamSynchronize(acc->stream));
        HIPCHK(hipStreamSynchronize(core->stream));
    }
    return src->open(core, m, 0, core->cfg.pop_size, false, core_counts);
}

// ps_distance_histogram (m == nullptr) and ps_multi_distance_histogram (core, acc: shard 0's handles; the binning -- with the
// halving h / 2 behind the sum over the shards -- runs on shard 0 against its accessory replica)
static int pair_hist_entry(ps_multi *m, ps_population *core, ps_population *acc, const ps_pair_hist_params *prm, ps_pair_hist_t *out,
                           uint64_t *joint)
{
    PSCHK(pair_hist_check_params(prm));
    core_band_source src;
    PSCHK(pair_source_open(&src, "distance_histogram", "a distance histogram needs", "sums", m, core, acc, true, nullptr));
    return pair_hist_device(src, acc, m ? m->prm.core_size : core->cfg.global_cols, prm, out, joint);
}

extern "C" int ps_distance_histogram(ps_population *core, ps_population *acc, const ps_pair_hist_params *prm, ps_pair_hist_t *out,
                                     uint64_t *joint)
{
    PSCHK(ps_needs_device());
    if (!core || !acc || !prm || !out || !joint) return ps_fail(PS_ERR_INVALID, "null argument");
    return pair_hist_entry(nullptr, core, acc, prm, out, joint);
}

extern "C" int ps_sim_distance_histogram(ps_sim *s, const ps_pair_hist_params *prm, ps_pair_hist_t *out, uint64_t *joint)
{
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    return ps_distance_histogram(s->core, s->acc, prm, out, joint);
}

extern "C" int ps_distance_histogram_timing(ps_population *core, double *counts_ms, double *binning_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_HIST], "no distance histogram has been computed on this handle", { counts_ms, binning_ms });
}

extern "C" int ps_multi_distance_histogram(ps_multi *m, const ps_pair_hist_params *prm, ps_pair_hist_t *out, uint64_t *joint)
{
    PSCHK(ps_needs_device());
    if (!m || !prm || !out || !joint) return ps_fail(PS_ERR_INVALID, "null argument");
    if (m->shard.size() == 1) return ps_sim_distance_histogram(m->shard[0], prm, out, joint);
    return pair_hist_entry(m, m->shard[0]->core, m->shard[0]->acc, prm, out, joint);
}
