// pair_readout.h -- the host frame that the all-pairs read-outs share (pair_histogram.h, strain_clusters.h, linkage_tree.h,
// upgma_tree.h, nearest_neighbours.h, clock_histogram.h): the reader of a pair list behind the ps_*_from_counts restatements,
// the metric checks, the row-order inverse, the head of a summary, the handle checks, the per-band pipeline of the two streams
// (pair_pipeline), the opening of the band source (pair_source_open) and the bodies of the ps_X / ps_sim_X / ps_multi_X entry
// triple.  Included by pansim_capi.hip behind core_band_source and readout_common.h, ahead of the read-outs.
#pragma once

#include "linkage_kernels.h"        // (ps_tr_acc_distance: the accessory distance as every metric read-out compares it)

static_assert(PS_TREE_CORE == 0 && PS_TREE_ACC == 1 && PS_KNN_CORE == PS_TREE_CORE && PS_KNN_ACC == PS_TREE_ACC, "one metric check");

// what a read-out with a metric calls itself in its messages, and the public names of its two constants
struct metric_names {
    const char *noun, *core, *acc;
};

static int metric_check(int32_t metric, const metric_names &n)
{
    if (metric != PS_TREE_CORE && metric != PS_TREE_ACC)
        return ps_fail(PS_ERR_INVALID, "the metric of %s is %s (0) or %s (1), not %d", n.noun, n.core, n.acc, (int)metric);
    return PS_OK;
}

// the cross products of two accessory distances stay in 64 bits while a <= 65535 and b = U + core_genes < 2^32
static int metric_check_core_genes(int32_t metric, uint64_t cg, const metric_names &n)
{
    if (metric == PS_TREE_ACC && cg + 65535ull >= (1ull << 32))
        return ps_fail(PS_ERR_INVALID, "the accessory metric of %s needs core_genes + 65535 < 2^32, not %llu core genes", n.noun,
                       (unsigned long long)cg);
    return PS_OK;
}

// The pair list of a host restatement: the indices of pair k (null for a caller without any) and its three numerators (null
// where the caller does not read them).  The checks are per pair, so that a caller's own check can stand between them.
struct pair_list {
    const uint32_t *r1, *r2, *core_h, *acc_inter, *acc_union;
    uint64_t n_pairs, pop_size;

    // a numerator array that an active criterion or metric reads is missing
    bool lacks(bool core_on, bool acc_on) const { return (core_on && !core_h) || (acc_on && (!acc_inter || !acc_union)); }
    int check_indices(uint64_t k) const
    {
        if (r1[k] >= pop_size || r2[k] >= pop_size)
            return ps_fail(PS_ERR_INVALID, "pair %llu: index %u is not below pop_size %llu", (unsigned long long)k, std::max(r1[k], r2[k]),
                           (unsigned long long)pop_size);
        if (r1[k] == r2[k]) return ps_fail(PS_ERR_INVALID, "pair %llu: both indices are %u", (unsigned long long)k, r1[k]);
        return PS_OK;
    }
    // for a caller that reads the accessory numerators; u16_limit: its kernels keep the intersections as u16
    int check_acc(uint64_t k, bool u16_limit) const
    {
        if (acc_inter[k] > acc_union[k])
            return ps_fail(PS_ERR_INVALID, "pair %llu: intersection %u above union %u", (unsigned long long)k, acc_inter[k], acc_union[k]);
        if (u16_limit && acc_union[k] > 65535u)
            return ps_fail(PS_ERR_INVALID, "pair %llu: union %u above the limit of 65535 accessory genes", (unsigned long long)k, acc_union[k]);
        return PS_OK;
    }
    // both, in that order, for a read-out with a metric
    int check(uint64_t k, bool acc) const
    {
        PSCHK(check_indices(k));
        return acc ? check_acc(k, true) : PS_OK;
    }
    // the distance of pair k under a metric: h / 2 over the core sites, or the accessory a / b
    void distance(uint64_t k, bool acc, uint64_t core_sites, uint64_t core_genes, uint64_t *num, uint64_t *den) const
    {
        if (acc) ps_tr_acc_distance(acc_inter[k], acc_union[k], core_genes, num, den);
        else {
            *num = core_h[k] / 2;
            *den = core_sites;
        }
    }
};

// out_row[i] = the output row of internal row i: the inverse of the row slot (null: the identity)
static std::vector<uint32_t> row_inverse(const uint32_t *slot, uint32_t N)
{
    std::vector<uint32_t> out_row(N);
    for (uint32_t k = 0; k < N; k++) out_row[slot ? slot[k] : k] = k;
    return out_row;
}

// a summary cleared, and the fields every all-pairs summary opens with
template <class T>
static void readout_head(T *o, uint64_t N, uint64_t pairs, uint64_t L, uint64_t cg)
{
    memset(o, 0, sizeof *o);
    o->pop_size = N;
    o->pairs = pairs;
    o->core_sites = L;
    o->core_genes = cg;
}

static int pair_handles(const ps_population *core, const ps_population *acc, const char *call, const char *what)
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

// The per-band pipeline of the all-pairs read-outs over the core stream of src.c0 and the stream of the accessory handle on the
// same device; both idle on entry.  Per band: core_counts() on the core stream, acc_counts() on the accessory stream behind the
// last consumer that read the scratch, consume() on the core stream behind both.  Every piece of work is timed into a group
// (event_timer); finish() synchronises both streams and leaves the groups' totals in the read-out's slot.
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

// What the device entries share behind their own parameter checks, under the name ps_<name> (m == nullptr: `core` must hold all
// sites, over which the read-out `verb`s) or ps_multi_<name> (core, acc: shard 0's handles).  The handles checked, `slot` (if
// asked for) the current row map of `core`, everything queued before the call complete, the band source open in internal order.
static int pair_source_open(core_band_source *src, const char *name, const char *what, const char *verb, ps_multi *m, ps_population *core,
                            ps_population *acc, bool core_counts, const uint32_t **slot)
{
    const std::string call = std::string(m ? "ps_multi_" : "ps_") + name;
    PSCHK(pair_handles(core, acc, call.c_str(), what));
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

// The bodies of a read-out's entry triple.  `args`: none of its other pointers is null; run(m, core, acc) is the read-out behind
// the checks -- m == nullptr over two handles that hold all sites, otherwise over shard 0's handles of a run of several shards.
// Each: the device, then the null pointers; a run of one shard is that shard's simulation.
template <class R>
static int pair_entry(ps_population *core, ps_population *acc, bool args, R &&run)
{
    PSCHK(ps_needs_device());
    if (!core || !acc || !args) return ps_fail(PS_ERR_INVALID, "null argument");
    return run((ps_multi *)nullptr, core, acc);
}

template <class R>
static int pair_entry(ps_sim *s, bool args, R &&run)
{
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    return pair_entry(s->core, s->acc, args, run);
}

template <class R>
static int pair_entry(ps_multi *m, bool args, R &&run)
{
    PSCHK(ps_needs_device());
    if (!m || !args) return ps_fail(PS_ERR_INVALID, "null argument");
    if (m->shard.size() == 1) return pair_entry(m->shard[0], args, run);
    return run(m, m->shard[0]->core, m->shard[0]->acc);
}
