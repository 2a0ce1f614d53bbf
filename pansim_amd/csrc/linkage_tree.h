// linkage_tree.h -- ps_linkage_tree / ps_sim_linkage_tree / ps_multi_linkage_tree and the host restatement
// ps_tree_from_counts (include/pansim_hip.h; the definitions: docs/LINKAGE_TREE.md).  Included by pansim_capi.hip behind
// pair_readout.h, whose pair-list reader, metric checks, band pipeline (pair_source_open, pair_pipeline) and entry bodies it reuses.
//
// As the clusters, everything on the device runs in INTERNAL row order: per band the numerators of the metric asked for (the
// other metric's count kernels are not launched), then a store kernel on the core stream that keeps them as the band's rows of a
// full N x N matrix; after the last band the Boruvka rounds on the core stream (linkage_kernels.h) until N - 1 edges are
// listed.  The rounds compare edges by their OUTPUT rows (out_row, the inverse of the row slot), so the tree is the one of the
// reference's row order; the host maps the listed edges to output rows and sorts them (tree_finish).
#pragma once

#include "linkage_kernels.h"

static const metric_names TREE_NAMES = { "a linkage tree", "PS_TREE_CORE", "PS_TREE_ACC" };

// e[0 .. n): tree edges with lo < hi in output rows, in any order -> the four arrays in ascending order and the summary fields
// that follow from them
static void tree_finish(std::vector<ps_tr_edge> &e, ps_tree_t *o, uint32_t *lo, uint32_t *hi, uint64_t *num, uint64_t *den)
{
    std::sort(e.begin(), e.end(), [](const ps_tr_edge &a, const ps_tr_edge &b) { return ps_tr_less(a, b); });
    o->edges = e.size();
    for (size_t k = 0; k < e.size(); k++) {
        lo[k] = e[k].lo;
        hi[k] = e[k].hi;
        num[k] = e[k].num;
        den[k] = e[k].den;
        o->undefined_edges += e[k].den == 0 ? 1 : 0;
        if (k == 0 || ps_tr_dist_cmp(e[k - 1].num, e[k - 1].den, e[k].num, e[k].den) != 0) o->distinct_heights++;
    }
}

extern "C" int ps_tree_from_counts(const uint32_t *r1, const uint32_t *r2, const uint32_t *core_h, const uint32_t *acc_inter,
                                   const uint32_t *acc_union, uint64_t n_pairs, uint64_t pop_size, uint64_t core_sites, uint64_t core_genes,
                                   const ps_tree_params *prm, ps_tree_t *out, uint32_t *lo, uint32_t *hi, uint64_t *num, uint64_t *den)
{
    if (!prm || !out || !lo || !hi || !num || !den || (n_pairs && (!r1 || !r2))) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(metric_check(prm->metric, TREE_NAMES));
    const bool acc = prm->metric == PS_TREE_ACC;
    const pair_list pairs = { r1, r2, core_h, acc_inter, acc_union, n_pairs, pop_size };
    if (n_pairs && pairs.lacks(!acc, acc))
        return ps_fail(PS_ERR_INVALID, "null argument: the metric needs its numerators");
    if (pop_size < 2 || pop_size > 0xffffffffull) return ps_fail(PS_ERR_INVALID, "a linkage tree needs 2 <= pop_size < 2^32");
    PSCHK(metric_check_core_genes(prm->metric, core_genes, TREE_NAMES));
    std::vector<ps_tr_edge> all(n_pairs);
    for (uint64_t k = 0; k < n_pairs; k++) {
        PSCHK(pairs.check(k, acc));
        ps_tr_edge &e = all[k];
        e.lo = std::min(r1[k], r2[k]);
        e.hi = std::max(r1[k], r2[k]);
        pairs.distance(k, acc, core_sites, core_genes, &e.num, &e.den);
    }
    // Kruskal: the pairs in ascending order, a pair kept when it joins two sets (stable: of two copies of a pair at one distance
    // written as different fractions, the earlier one of the list is the one reported)
    std::stable_sort(all.begin(), all.end(), [](const ps_tr_edge &a, const ps_tr_edge &b) { return ps_tr_less(a, b); });
    std::vector<uint32_t> parent(pop_size);
    for (uint64_t k = 0; k < pop_size; k++) parent[k] = (uint32_t)k;
    auto root = [&](uint32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    std::vector<ps_tr_edge> kept;
    for (const ps_tr_edge &e : all) {
        const uint32_t x = root(e.lo), y = root(e.hi);
        if (x == y) continue;
        parent[std::max(x, y)] = std::min(x, y);
        kept.push_back(e);
    }
    readout_head(out, pop_size, n_pairs, core_sites, core_genes);
    out->metric = (uint64_t)prm->metric;
    tree_finish(kept, out, lo, hi, num, den);
    return PS_OK;
}

// the scratch on the core handle: the edge counter, twelve arrays of N u32, the matrix (N rows of ldm u32 or u16)
enum { PS_TR_COMP = 0, PS_TR_PARENT, PS_TR_OUT, PS_TR_BEST, PS_TR_CJ, PS_TR_CNUM, PS_TR_CDEN, PS_TR_EI, PS_TR_EJ, PS_TR_ENUM, PS_TR_EDEN,
       PS_TR_ROWCNT, PS_TR_ARRAYS };

struct tree_scratch {
    uint32_t *count = nullptr, *arr[PS_TR_ARRAYS] = {};
    void *M = nullptr;
    uint64_t ldm = 0;
};

static int tree_scratch_get(ps_population *c0, uint64_t N, bool acc, tree_scratch *s)
{
    scratch_layout lay;
    uint64_t o_arr[PS_TR_ARRAYS];
    s->ldm = (N + 63) & ~63ull;
    const uint64_t o_count = lay.add(16, 16);
    for (uint64_t &o : o_arr) o = lay.add(N * 4, 16);
    const uint64_t o_M = lay.add(N * s->ldm * (acc ? 2 : 4), 16);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(c0->ro[PS_RO_TREE], lay.bytes, &base, "cannot allocate the %llu bytes of the distance numerators of all pairs of %llu individuals",
                      (unsigned long long)N));
    s->count = (uint32_t *)(base + o_count);
    for (int k = 0; k < PS_TR_ARRAYS; k++) s->arr[k] = (uint32_t *)(base + o_arr[k]);
    s->M = base + o_M;
    return PS_OK;
}

static int tree_store_launch(const pair_pipeline &pl, bool acc, uint32_t lo, uint32_t nrows, const tree_scratch &s)
{
    const uint32_t N = (uint32_t)pl.c0->cfg.pop_size;
    const uint32_t per = acc ? 2u : 4u, gx = (uint32_t)((s.ldm / per + 255u) / 256u), gy = std::max(1u, std::min(nrows, 4096u));
    if (acc) tree_store_acc_kernel<<<dim3(gx, gy), 256, 0, pl.sc>>>(pl.In(), pl.A.ld, N, lo, nrows, (uint16_t *)s.M, s.ldm);
    else tree_store_core_kernel<<<dim3(gx, gy), 256, 0, pl.sc>>>((const uint32_t *)pl.c0->d_cdavg, pl.src.b.ld, N, lo, nrows, (uint32_t *)s.M, s.ldm);
    HIPCHK(hipGetLastError());
    return PS_OK;
}

// The call behind the device entries: src holds the bands (open in internal order with the core metric; with the accessory
// metric its counts are not asked for), `acc` lives on src.c0's device, both streams are idle; `slot` is c0's current row map.
static int tree_device(core_band_source &src, ps_population *acc, uint64_t L, const ps_tree_params *prm, const uint32_t *slot, ps_tree_t *out,
                       uint32_t *lo_out, uint32_t *hi_out, uint64_t *num_out, uint64_t *den_out)
{
    ps_population *c0 = src.c0;
    const uint32_t N = (uint32_t)c0->cfg.pop_size;
    const uint64_t cg = acc->cfg.core_genes;
    const bool acc_metric = prm->metric == PS_TREE_ACC;
    PSCHK(metric_check_core_genes(prm->metric, cg, TREE_NAMES));
    PSCHK(use_device(c0));
    tree_scratch s;
    PSCHK(tree_scratch_get(c0, N, acc_metric, &s));
    // out_row[i] = the output row of internal row i
    const std::vector<uint32_t> out_row = row_inverse(slot, N);
    readout_slot &ro = c0->ro[PS_RO_TREE];
    pair_pipeline pl(src, acc);
    hipStream_t sc = pl.sc;
    HIPCHK(hipMemsetAsync(s.count, 0, 16, sc));
    HIPCHK(hipMemcpyAsync(s.arr[PS_TR_OUT], out_row.data(), (uint64_t)N * sizeof(uint32_t), hipMemcpyHostToDevice, sc));
    tree_init_kernel<<<(N + 255u) / 256u, 256, 0, sc>>>(s.arr[PS_TR_COMP], s.arr[PS_TR_PARENT], N);
    HIPCHK(hipGetLastError());
    ro.timed = false;
    PSCHK(pl.open(acc_metric));
    const bool have_in = acc_metric && pl.acc_on;          // (no accessory genes: I = U = 0 for every pair, nothing to store)
    // timer groups: 0 = the count phase, 1 = the store kernels, 2 = the rounds
    PSCHK(pl.for_bands([&](uint32_t lo, uint32_t nrows) -> int {
        if (!acc_metric) PSCHK(pl.core_counts(0, lo, nrows));
        else PSCHK(pl.acc_counts(0, lo, nrows));
        if (acc_metric && !have_in) return PS_OK;
        return pl.consume(1, [&]() { return tree_store_launch(pl, acc_metric, lo, nrows, s); });
    }));
    // (the rows' gene counts beside the intersections: the core stream is behind the accessory stream's padding kernel here)
    if (have_in) HIPCHK(hipMemcpyAsync(s.arr[PS_TR_ROWCNT], pl.A.rowcnt, (uint64_t)N * sizeof(uint32_t), hipMemcpyDeviceToDevice, sc));
    // the rounds: every component hooks to another, so a round at least halves their number
    uint32_t max_rounds = 0;
    while ((1ull << max_rounds) < N) max_rounds++;
    uint64_t rounds = 0;
    uint32_t count = 0;
    const uint32_t gn = (N + 255u) / 256u;
    PSCHK(pl.timed(2, sc, [&]() -> int {
        while (count < N - 1u) {
            if (rounds == max_rounds)
                return ps_fail(PS_ERR_STATE, "the tree of %u individuals holds %u edges after %u rounds", N, count, max_rounds);
            rounds++;
            HIPCHK(hipMemsetAsync(s.arr[PS_TR_BEST], 0xff, (uint64_t)N * sizeof(uint32_t), sc));
            const uint32_t gw = std::min((N + 3u) / 4u, 4096u);
            if (acc_metric)
                tree_row_min_kernel<true><<<gw, 256, 0, sc>>>(nullptr, have_in ? (const uint16_t *)s.M : nullptr, s.ldm, s.arr[PS_TR_ROWCNT], cg, N,
                                                              s.arr[PS_TR_COMP], s.arr[PS_TR_OUT], s.arr[PS_TR_CJ], s.arr[PS_TR_CNUM], s.arr[PS_TR_CDEN]);
            else
                tree_row_min_kernel<false><<<gw, 256, 0, sc>>>((const uint32_t *)s.M, nullptr, s.ldm, nullptr, cg, N, s.arr[PS_TR_COMP],
                                                               s.arr[PS_TR_OUT], s.arr[PS_TR_CJ], s.arr[PS_TR_CNUM], s.arr[PS_TR_CDEN]);
            tree_comp_min_kernel<<<gn, 256, 0, sc>>>(N, s.arr[PS_TR_COMP], s.arr[PS_TR_OUT], s.arr[PS_TR_CJ], s.arr[PS_TR_CNUM], s.arr[PS_TR_CDEN],
                                                     s.arr[PS_TR_BEST]);
            tree_link_kernel<<<gn, 256, 0, sc>>>(N, s.arr[PS_TR_COMP], s.arr[PS_TR_CJ], s.arr[PS_TR_CNUM], s.arr[PS_TR_CDEN], s.arr[PS_TR_BEST],
                                                 s.arr[PS_TR_PARENT], s.count, s.arr[PS_TR_EI], s.arr[PS_TR_EJ], s.arr[PS_TR_ENUM], s.arr[PS_TR_EDEN]);
            tree_jump_kernel<<<gn, 256, 0, sc>>>(N, s.arr[PS_TR_PARENT], s.arr[PS_TR_COMP]);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&count, s.count, sizeof count, hipMemcpyDeviceToHost, sc));
            HIPCHK(hipStreamSynchronize(sc));
            if (count > N - 1u) return ps_fail(PS_ERR_STATE, "the tree of %u individuals lists %u edges", N, count);
        }
        return PS_OK;
    }));
    std::vector<uint32_t> ei(N), ej(N), en(N), ed(N);
    const uint64_t eb = (uint64_t)(N - 1u) * sizeof(uint32_t);
    HIPCHK(hipMemcpyAsync(ei.data(), s.arr[PS_TR_EI], eb, hipMemcpyDeviceToHost, sc));
    HIPCHK(hipMemcpyAsync(ej.data(), s.arr[PS_TR_EJ], eb, hipMemcpyDeviceToHost, sc));
    HIPCHK(hipMemcpyAsync(en.data(), s.arr[PS_TR_ENUM], eb, hipMemcpyDeviceToHost, sc));
    HIPCHK(hipMemcpyAsync(ed.data(), s.arr[PS_TR_EDEN], eb, hipMemcpyDeviceToHost, sc));
    PSCHK(pl.finish(ro, 3));
    std::vector<ps_tr_edge> e(N - 1u);
    for (uint32_t k = 0; k + 1u < N; k++) {
        if (ei[k] >= N || ej[k] >= N) return ps_fail(PS_ERR_STATE, "edge %u of the tree joins rows %u and %u of %u", k, ei[k], ej[k], N);
        const uint32_t a = out_row[ei[k]], c = out_row[ej[k]];
        e[k].lo = std::min(a, c);
        e[k].hi = std::max(a, c);
        e[k].num = en[k];
        e[k].den = acc_metric ? (uint64_t)ed[k] : L;
    }
    readout_head(out, N, (uint64_t)N * (N - 1) / 2, L, cg);
    out->metric = (uint64_t)prm->metric;
    out->rounds = rounds;
    tree_finish(e, out, lo_out, hi_out, num_out, den_out);
    return PS_OK;
}

// behind pair_entry: ps_linkage_tree (m == nullptr) and ps_multi_linkage_tree (core, acc: shard 0's handles; the matrix and the
// rounds on shard 0 against its accessory replica, the row map from shard 0's simulation)
static auto tree_entry(const ps_tree_params *prm, ps_tree_t *out, uint32_t *lo, uint32_t *hi, uint64_t *num, uint64_t *den)
{
    return [=](ps_multi *m, ps_population *core, ps_population *acc) -> int {
        PSCHK(metric_check(prm->metric, TREE_NAMES));
        core_band_source src;
        const uint32_t *slot = nullptr;
        PSCHK(pair_source_open(&src, "linkage_tree", "a linkage tree needs", "compares", m, core, acc, prm->metric == PS_TREE_CORE, &slot));
        return tree_device(src, acc, m ? m->prm.core_size : core->cfg.global_cols, prm, slot, out, lo, hi, num, den);
    };
}

extern "C" int ps_linkage_tree(ps_population *core, ps_population *acc, const ps_tree_params *prm, ps_tree_t *out, uint32_t *lo, uint32_t *hi,
                               uint64_t *num, uint64_t *den)
{
    return pair_entry(core, acc, prm && out && lo && hi && num && den, tree_entry(prm, out, lo, hi, num, den));
}

extern "C" int ps_sim_linkage_tree(ps_sim *s, const ps_tree_params *prm, ps_tree_t *out, uint32_t *lo, uint32_t *hi, uint64_t *num,
                                   uint64_t *den)
{
    return pair_entry(s, prm && out && lo && hi && num && den, tree_entry(prm, out, lo, hi, num, den));
}

extern "C" int ps_linkage_tree_timing(ps_population *core, double *counts_ms, double *store_ms, double *rounds_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_TREE], "no linkage tree has been computed on this handle", { counts_ms, store_ms, rounds_ms });
}

extern "C" int ps_multi_linkage_tree(ps_multi *m, const ps_tree_params *prm, ps_tree_t *out, uint32_t *lo, uint32_t *hi, uint64_t *num,
                                     uint64_t *den)
{
    return pair_entry(m, prm && out && lo && hi && num && den, tree_entry(prm, out, lo, hi, num, den));
}
