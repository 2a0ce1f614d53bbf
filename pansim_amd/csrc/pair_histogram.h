// pair_histogram.h -- ps_distance_histogram / ps_sim_distance_histogram / ps_multi_distance_histogram and the host
// restatement ps_histogram_from_counts (include/pansim_hip.h; the definitions: docs/DISTANCE_HISTOGRAM.md).  Included by
// pansim_capi.hip behind struct ps_multi.
//
// Both count phases run in INTERNAL row order (no row slot): the set of unordered pairs does not change under one
// permutation applied to both matrices, and inside a simulation the two matrices hold the same individuals in the same
// internal order, so none of the row mapping of DESIGN.md 3.5 is needed.  Per band of rows (core_davg_plan_bands): the
// core numerators (core_davg_band_counts: the FP4 contraction for one-hot matrices, core_band_counts_simple otherwise) on
// the core stream, the accessory intersections of the same rows (acc_intersections_mfma_kernel) on the accessory stream,
// then pair_hist_kernel on the core stream behind both.
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

struct pair_hist_events {
    std::vector<hipEvent_t> ev;
    ~pair_hist_events() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    int make(hipEvent_t *out)
    {
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreate(&e));
        ev.push_back(e);
        *out = e;
        return PS_OK;
    }
};

// The padded rows and row counts of the accessory matrix (as average_distance_device prepares them) and the scratch of one
// band's u16 intersections, on `st`.  G == 0: nothing (the kernel takes I = U = 0).
struct pair_hist_acc { uint32_t *rowsP = nullptr, *rowcnt = nullptr; uint16_t *In = nullptr; uint32_t WP = 0, Npad = 0, ld = 0; };

static int pair_hist_acc_prepare(ps_population *p, uint32_t band, hipStream_t st, pair_hist_acc *o)
{
    *o = pair_hist_acc{};
    if (p->d.G == 0) return PS_OK;
    const uint64_t N = p->cfg.pop_size;
    const uint32_t WP = (2u * p->d.GW + 7u) & ~7u, Npad = (uint32_t)((N + 127) & ~127ull), ld = Npad + 128u;
    const uint64_t need = (uint64_t)Npad * WP * 4 + (uint64_t)Npad * 4 + 64;
    if (p->davg_cap < need) {
        if (p->d_davg) HIPCHK(hipFree(p->d_davg));
        p->d_davg = nullptr;
        p->davg_cap = 0;
        HIPCHK(hipMalloc(&p->d_davg, need));
        p->davg_cap = need;
    }
    // (a wave of the contraction stores 64 whole rows: the band is a multiple of 256)
    const uint64_t need_in = (((uint64_t)band + 255) & ~255ull) * ld * 2;
    if (p->davg_in_cap < need_in) {
        if (p->d_davg_in) HIPCHK(hipFree(p->d_davg_in));
        p->d_davg_in = nullptr;
        p->davg_in_cap = 0;
        HIPCHK(hipMalloc(&p->d_davg_in, need_in));
        p->davg_in_cap = need_in;
    }
    o->rowsP = (uint32_t *)p->d_davg;
    o->rowcnt = o->rowsP + (uint64_t)Npad * WP;
    o->In = (uint16_t *)p->d_davg_in;
    o->WP = WP;
    o->Npad = Npad;
    o->ld = ld;
    acc_rows_pad_kernel<<<(Npad + 3u) / 4u, 256, 0, st>>>(p->I[p->cur], o->rowsP, o->rowcnt, p->d, WP, Npad);
    HIPCHK(hipGetLastError());
    return PS_OK;
}

static int pair_hist_acc_band(const pair_hist_acc &A, uint32_t lo, uint32_t nrows, hipStream_t st)
{
    const uint32_t lds = 256u * 64u * 4u, steps = A.Npad / 128u, gx = (nrows + 255u) / 256u;
    uint32_t jsteps = 8u;
    while (jsteps > 1u && (uint64_t)gx * ((steps + jsteps - 1u) / jsteps) < 2048u) jsteps >>= 1;
    HIPCHK(hipFuncSetAttribute((const void *)acc_intersections_mfma_kernel<2u>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    acc_intersections_mfma_kernel<2u><<<dim3(gx, (steps + jsteps - 1u) / jsteps), 256, lds, st>>>(A.rowsP, A.WP, A.Npad, lo, nrows, jsteps, A.In, A.ld);
    HIPCHK(hipGetLastError());
    return PS_OK;
}

template <bool BIN, bool MOM>
static int pair_hist_launch(const ps_population *c0, const core_davg_bands &b, const pair_hist_acc &A, uint32_t lo, uint32_t nrows,
                            const ps_ph_args &a, unsigned long long *d_ph, hipStream_t st)
{
    const uint32_t N = (uint32_t)c0->cfg.pop_size;
    const uint32_t lds = BIN ? a.Bc * a.Ba * 4u : 0u;
    // four waves per workgroup over the row's chunks, the rows over y; as many workgroups as the bins' LDS lets a CU hold
    // (a workgroup's u32 bins cannot overflow: a band holds fewer than 2^32 pairs)
    const uint32_t nchunk = (N + 255u) / 256u, gx = std::max(1u, std::min((nchunk + 3u) / 4u, 8u));
    const uint32_t per_cu = std::max(1u, std::min(8u, (160u * 1024u) / (lds + 256u)));
    const uint32_t gy = std::max(1u, std::min(std::min(nrows, 65535u), 256u * per_cu / gx));
    auto kern = pair_hist_kernel<BIN, MOM>;
    if (lds > 32768u) HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(gx, gy), dim3(256), lds, st, (const uint32_t *)c0->d_cdavg, b.ld, (const uint16_t *)A.In, A.ld,
                       (const uint32_t *)A.rowcnt, N, lo, nrows, a, d_ph + PS_PH_WORDS, d_ph);
    HIPCHK(hipGetLastError());
    return PS_OK;
}

// The call behind the three device entries.  band_counts(lo, nrows) leaves h(i, j) over ALL core sites for the rows of the
// band in c0->d_cdavg, ordered on c0->stream; `acc` lives on c0's device.  Both streams are idle on entry.
template <class F>
static int pair_hist_device(ps_population *c0, ps_population *acc, const core_davg_bands &b, uint64_t L, const ps_pair_hist_params *prm,
                            F &&band_counts, ps_pair_hist_t *out, uint64_t *joint)
{
    const uint64_t N = c0->cfg.pop_size, nbins = (uint64_t)prm->core_bins * prm->acc_bins, cg = acc->cfg.core_genes;
    hipStream_t sc = c0->stream, sa = acc->stream;
    PSCHK(use_device(c0));
    const uint64_t need = PS_PH_WORDS + nbins;
    if (c0->ph_cap < need) {
        if (c0->d_ph) HIPCHK(hipFree(c0->d_ph));
        c0->d_ph = nullptr;
        c0->ph_cap = 0;
        HIPCHK(hipMalloc(&c0->d_ph, need * sizeof(unsigned long long)));
        c0->ph_cap = need;
    }
    unsigned long long *d_ph = c0->d_ph;
    HIPCHK(hipMemsetAsync(d_ph, 0, need * sizeof(unsigned long long), sc));
    HIPCHK(hipMemsetAsync(d_ph + PS_PH_MIN, 0xff, sizeof(unsigned long long), sc));
    c0->ph_timed = false;
    pair_hist_acc A;
    PSCHK(pair_hist_acc_prepare(acc, b.band, sa, &A));
    pair_hist_events evs;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> t_counts, t_bin;
    auto timed = [&](std::vector<std::pair<hipEvent_t, hipEvent_t>> &list, hipStream_t st, auto &&work) -> int {
        hipEvent_t e0, e1;
        PSCHK(evs.make(&e0));
        PSCHK(evs.make(&e1));
        HIPCHK(hipEventRecord(e0, st));
        PSCHK(work());
        HIPCHK(hipEventRecord(e1, st));
        list.push_back({ e0, e1 });
        return PS_OK;
    };
    hipEvent_t ev_acc = nullptr, ev_bin = nullptr;
    PSCHK(evs.make(&ev_acc));
    PSCHK(evs.make(&ev_bin));
    const bool automatic = prm->core_span == 0;
    const bool one_band = b.c_end - b.c0 <= b.band;
    uint64_t S = prm->core_span;
    auto for_bands = [&](auto &&body) -> int {
        for (uint32_t lo = b.c0; lo < b.c_end; lo += b.band) PSCHK(body(lo, std::min(b.band, b.c_end - lo)));
        return PS_OK;
    };
    auto read_span = [&]() -> int {
        unsigned long long mx = 0;
        HIPCHK(hipMemcpyAsync(&mx, d_ph + PS_PH_MAX, sizeof mx, hipMemcpyDeviceToHost, sc));
        HIPCHK(hipStreamSynchronize(sc));
        S = mx + 1;
        return PS_OK;
    };
    // the accessory counts of a band on their stream, behind the last binning that read the scratch; the binning behind them
    bool binned_before = false;
    auto acc_band = [&](uint32_t lo, uint32_t nrows) -> int {
        if (!A.In) return PS_OK;
        if (binned_before) HIPCHK(hipStreamWaitEvent(sa, ev_bin, 0));
        PSCHK(timed(t_counts, sa, [&]() { return pair_hist_acc_band(A, lo, nrows, sa); }));
        HIPCHK(hipEventRecord(ev_acc, sa));
        HIPCHK(hipStreamWaitEvent(sc, ev_acc, 0));
        return PS_OK;
    };
    auto bin_band = [&](uint32_t lo, uint32_t nrows, bool moments) -> int {
        const ps_ph_args a = pair_hist_args(prm, S, cg);
        PSCHK(timed(t_bin, sc, [&]() {
            return moments ? pair_hist_launch<true, true>(c0, b, A, lo, nrows, a, d_ph, sc)
                           : pair_hist_launch<true, false>(c0, b, A, lo, nrows, a, d_ph, sc);
        }));
        HIPCHK(hipEventRecord(ev_bin, sc));
        binned_before = true;
        return PS_OK;
    };
    auto moments_band = [&](uint32_t lo, uint32_t nrows) -> int {
        return timed(t_bin, sc, [&]() { return pair_hist_launch<false, true>(c0, b, A, lo, nrows, ps_ph_args{}, d_ph, sc); });
    };
    auto counts = [&](uint32_t lo, uint32_t nrows) -> int { return timed(t_counts, sc, [&]() { return band_counts(lo, nrows); }); };
    if (!automatic) {
        PSCHK(for_bands([&](uint32_t lo, uint32_t nrows) -> int {
            PSCHK(counts(lo, nrows));
            PSCHK(acc_band(lo, nrows));
            return bin_band(lo, nrows, true);
        }));
    } else if (one_band) {
        // the automatic span over one band: the moments first, the bins from the same counts
        PSCHK(counts(b.c0, b.c_end - b.c0));
        PSCHK(acc_band(b.c0, b.c_end - b.c0));
        PSCHK(moments_band(b.c0, b.c_end - b.c0));
        PSCHK(read_span());
        PSCHK(bin_band(b.c0, b.c_end - b.c0, false));
    } else {
        // ... over several bands: the core contraction runs twice (docs/DISTANCE_HISTOGRAM.md)
        PSCHK(for_bands([&](uint32_t lo, uint32_t nrows) -> int {
            PSCHK(counts(lo, nrows));
            return moments_band(lo, nrows);
        }));
        PSCHK(read_span());
        PSCHK(for_bands([&](uint32_t lo, uint32_t nrows) -> int {
            PSCHK(counts(lo, nrows));
            PSCHK(acc_band(lo, nrows));
            return bin_band(lo, nrows, false);
        }));
    }
    unsigned long long w[PS_PH_WORDS];
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the bins are copied as they are");
    HIPCHK(hipMemcpyAsync(w, d_ph, sizeof w, hipMemcpyDeviceToHost, sc));
    HIPCHK(hipMemcpyAsync(joint, d_ph + PS_PH_WORDS, nbins * sizeof(uint64_t), hipMemcpyDeviceToHost, sc));
    HIPCHK(hipStreamSynchronize(sa));
    HIPCHK(hipStreamSynchronize(sc));
    double ms_counts = 0.0, ms_bin = 0.0;
    for (int which = 0; which < 2; which++)
        for (const auto &e : which ? t_bin : t_counts) {
            float ms = 0.0f;
            HIPCHK(hipEventElapsedTime(&ms, e.first, e.second));
            (which ? ms_bin : ms_counts) += (double)ms;
        }
    c0->ph_counts_ms = ms_counts;
    c0->ph_bin_ms = ms_bin;
    c0->ph_timed = true;
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

static int pair_hist_needs_device(void)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return ps_fail(PS_ERR_NO_DEVICE, "no HIP device is visible: libpansim_hip has no CPU path");
    return PS_OK;
}

extern "C" int ps_distance_histogram(ps_population *core, ps_population *acc, const ps_pair_hist_params *prm, ps_pair_hist_t *out,
                                     uint64_t *joint)
{
    PSCHK(pair_hist_needs_device());
    if (!core || !acc || !prm || !out || !joint) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(pair_hist_check_params(prm));
    PSCHK(pair_hist_handles(core, acc, "ps_distance_histogram"));
    if (core->cfg.ncols != core->cfg.global_cols)
        return ps_fail(PS_ERR_INVALID, "ps_distance_histogram sums over all %llu core sites; this handle is one site shard "
                                       "([%llu, %llu)): use ps_multi_distance_histogram", (unsigned long long)core->cfg.global_cols,
                       (unsigned long long)core->cfg.col_offset, (unsigned long long)(core->cfg.col_offset + core->cfg.ncols));
    PSCHK(use_device(core));
    // everything queued on either handle precedes the count kernels of both (as sim_pair_counts orders them)
    HIPCHK(hipStreamSynchronize(acc->stream));
    HIPCHK(hipStreamSynchronize(core->stream));
    const uint32_t N = (uint32_t)core->cfg.pop_size;
    const core_davg_bands b = core_davg_plan_bands(core, 0, N);
    core_davg_src src;
    PSCHK(core_davg_prepare(core, b, core->onehot_safe && core->core_davg_form != 3, nullptr, core->stream, &src));
    return pair_hist_device(core, acc, b, core->cfg.global_cols, prm,
                            [&](uint32_t lo, uint32_t nrows) { return core_davg_band_counts(core, src, b, lo, nrows, core->stream); }, out, joint);
}

extern "C" int ps_sim_distance_histogram(ps_sim *s, const ps_pair_hist_params *prm, ps_pair_hist_t *out, uint64_t *joint)
{
    PSCHK(pair_hist_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    return ps_distance_histogram(s->core, s->acc, prm, out, joint);
}

extern "C" int ps_distance_histogram_timing(ps_population *core, double *counts_ms, double *binning_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    if (!core->ph_timed) return ps_fail(PS_ERR_STATE, "no distance histogram has been computed on this handle");
    if (counts_ms) *counts_ms = core->ph_counts_ms;
    if (binning_ms) *binning_ms = core->ph_bin_ms;
    return PS_OK;
}

// One band of a sharded run: every shard counts its own sites, shard 0's device adds the shards' counts into its own (where
// they are with peer access, through the landing buffer d_land without).  Ordered on shard 0's core stream.
static int multi_band_counts(ps_multi *m, const std::vector<core_davg_src> &src, const core_davg_bands &b, uint32_t *d_land, uint32_t lo,
                             uint32_t nrows)
{
    const size_t K = m->shard.size();
    ps_population *c0 = m->shard[0]->core;
    const uint64_t n = (uint64_t)nrows * b.ld;
    // (the last kernel that reads shard 0's counts has finished before any shard overwrites its own)
    PSCHK(use_device(c0));
    HIPCHK(hipStreamSynchronize(c0->stream));
    PSCHK(multi_for_each(m, [&](size_t k) {
        ps_population *c = m->shard[k]->core;
        PSCHK(use_device(c));
        PSCHK(core_davg_band_counts(c, src[k], b, lo, nrows, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return (int)PS_OK;
    }));
    PSCHK(use_device(c0));
    for (size_t k = 1; k < K; k++) {
        ps_population *c = m->shard[k]->core;
        if (m->peers_ok) {
            u32_add_kernel<<<(uint32_t)((n + 255) / 256), 256, 0, c0->stream>>>(c0->d_cdavg, c->d_cdavg, n);
        } else {
            HIPCHK(hipMemcpyPeerAsync(d_land, c0->device, c->d_cdavg, c->device, n * sizeof(uint32_t), c0->stream));
            u32_add_kernel<<<(uint32_t)((n + 255) / 256), 256, 0, c0->stream>>>(c0->d_cdavg, d_land, n);
        }
        HIPCHK(hipGetLastError());
    }
    return PS_OK;
}

// As ps_multi_average_distance: band by band every shard counts its own sites, shard 0's device adds the shards' counts
// (where they are with peer access, through a landing buffer without), and the binning -- with the halving h / 2 behind
// the sum over the shards -- runs on shard 0 against its accessory replica.
extern "C" int ps_multi_distance_histogram(ps_multi *m, const ps_pair_hist_params *prm, ps_pair_hist_t *out, uint64_t *joint)
{
    PSCHK(pair_hist_needs_device());
    if (!m || !prm || !out || !joint) return ps_fail(PS_ERR_INVALID, "null argument");
    const size_t K = m->shard.size();
    if (K == 1) return ps_sim_distance_histogram(m->shard[0], prm, out, joint);
    PSCHK(pair_hist_check_params(prm));
    ps_population *c0 = m->shard[0]->core, *acc = m->shard[0]->acc;
    PSCHK(pair_hist_handles(c0, acc, "ps_multi_distance_histogram"));
    const uint32_t N = (uint32_t)m->prm.pop_size;
    PSCHK(ps_multi_sync(m));
    const core_davg_bands b = core_davg_plan_bands(c0, 0, N);
    bool onehot = true;
    for (size_t k = 0; k < K; k++) onehot = onehot && m->shard[k]->core->onehot_safe && c0->core_davg_form != 3;
    std::vector<core_davg_src> src(K);
    PSCHK(multi_for_each(m, [&](size_t k) {
        ps_population *c = m->shard[k]->core;
        PSCHK(use_device(c));
        return core_davg_prepare(c, b, onehot, nullptr, c->stream, &src[k]);
    }));
    PSCHK(use_device(c0));
    uint32_t *d_land = nullptr;         // (without peer access: a peer's band counts copied over first)
    if (!m->peers_ok) HIPCHK(hipMalloc(&d_land, (uint64_t)b.band * b.ld * sizeof(uint32_t)));
    auto band_counts = [&](uint32_t lo, uint32_t nrows) { return multi_band_counts(m, src, b, d_land, lo, nrows); };
    const int rc = pair_hist_device(c0, acc, b, m->prm.core_size, prm, band_counts, out, joint);
    (void)hipSetDevice(c0->device);
    (void)hipStreamSynchronize(c0->stream);
    if (d_land) (void)hipFree(d_land);
    return rc;
}
