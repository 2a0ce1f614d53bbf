// strain_clusters.h -- ps_strain_clusters / ps_sim_strain_clusters / ps_multi_strain_clusters and the host restatement
// ps_clusters_from_counts (include/pansim_hip.h; the definitions: docs/STRAIN_CLUSTERS.md).  Included by pansim_capi.hip
// behind pair_readout.h, whose pair-list reader, band pipeline (pair_source_open, pair_pipeline) and entry bodies it reuses.
//
// As the histogram, everything on the device runs in INTERNAL row order: per band the core numerators on the core stream,
// the accessory intersections on the accessory stream, pair_edge_kernel on the core stream behind both; after the last band
// the label rounds (cluster_hook_kernel, cluster_jump_kernel) until a hook round moves no label.  Only the labels are mapped
// to the reference's row order, on the host (cluster_finish).
#pragma once

#include "cluster_kernels.h"

static int cluster_check_params(const ps_cluster_params *prm, bool *core_on, bool *acc_on)
{
    *core_on = prm->core_max_d != UINT64_MAX;
    *acc_on = prm->acc_den != 0;
    if (!*core_on && !*acc_on)
        return ps_fail(PS_ERR_INVALID, "strain clusters need at least one criterion: core_max_d below UINT64_MAX or acc_den above 0");
    if (*acc_on && (prm->acc_num > prm->acc_den || prm->acc_den > (1u << 24)))
        return ps_fail(PS_ERR_INVALID, "the accessory criterion needs acc_num <= acc_den <= 2^24, not %u / %u", prm->acc_num, prm->acc_den);
    return PS_OK;
}

static ps_cl_args cluster_args(const ps_cluster_params *prm, uint64_t cg)
{
    ps_cl_args a;
    a.d_max = (uint32_t)std::min<uint64_t>(prm->core_max_d, 0xffffffffull);
    a.num = prm->acc_num;
    a.den = prm->acc_den;
    a.cg = cg;
    return a;
}

// rep[k]: any value below N that is equal exactly for the members of one cluster -> labels[k] = the smallest k of the
// cluster, and the summary fields that follow from the labels
static void cluster_finish(const uint32_t *rep, uint64_t N, uint32_t *labels, ps_cluster_t *o)
{
    std::vector<uint32_t> first(N, UINT32_MAX), size(N, 0);
    for (uint64_t k = 0; k < N; k++) {
        if (first[rep[k]] == UINT32_MAX) first[rep[k]] = (uint32_t)k;
        labels[k] = first[rep[k]];
        size[labels[k]]++;
    }
    for (uint64_t k = 0; k < N; k++) {
        const uint64_t s = size[k];
        if (!s) continue;
        o->clusters++;
        o->singletons += s == 1 ? 1 : 0;
        o->largest_cluster = std::max(o->largest_cluster, s);
        o->within_pairs += s * (s - 1) / 2;
    }
}

extern "C" int ps_clusters_from_counts(const uint32_t *r1, const uint32_t *r2, const uint32_t *core_h, const uint32_t *acc_inter,
                                       const uint32_t *acc_union, uint64_t n_pairs, uint64_t pop_size, uint64_t core_sites,
                                       uint64_t core_genes, const ps_cluster_params *prm, ps_cluster_t *out, uint32_t *labels)
{
    if (!prm || !out || !labels || (n_pairs && (!r1 || !r2))) return ps_fail(PS_ERR_INVALID, "null argument");
    bool core_on, acc_on;
    PSCHK(cluster_check_params(prm, &core_on, &acc_on));
    const pair_list pairs = { r1, r2, core_h, acc_inter, acc_union, n_pairs, pop_size };
    if (n_pairs && pairs.lacks(core_on, acc_on))
        return ps_fail(PS_ERR_INVALID, "null argument: an active criterion needs its numerators");
    if (pop_size < 2 || pop_size > 0xffffffffull) return ps_fail(PS_ERR_INVALID, "strain clusters need 2 <= pop_size < 2^32");
    for (uint64_t k = 0; k < n_pairs; k++) {
        PSCHK(pairs.check_indices(k));
        if (acc_on) PSCHK(pairs.check_acc(k, false));       // (no u16 limit: the edges are decided pair by pair)
    }
    const ps_cl_args a = cluster_args(prm, core_genes);
    // union-find, the smaller root kept: root(k) is the smallest member of k's set
    std::vector<uint32_t> parent(pop_size);
    for (uint64_t k = 0; k < pop_size; k++) parent[k] = (uint32_t)k;
    auto root = [&](uint32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    readout_head(out, pop_size, n_pairs, core_sites, core_genes);
    for (uint64_t k = 0; k < n_pairs; k++) {
        const uint32_t h = core_on ? core_h[k] : 0u, in = acc_on ? acc_inter[k] : 0u, un = acc_on ? acc_union[k] : 0u;
        bool undefined, edge;
        if (core_on && acc_on) edge = ps_cl_edge<true, true>(h, in, un, a, &undefined);
        else if (core_on) edge = ps_cl_edge<true, false>(h, in, un, a, &undefined);
        else edge = ps_cl_edge<false, true>(h, in, un, a, &undefined);
        out->undefined_pairs += undefined ? 1 : 0;
        if (!edge) continue;
        out->edges++;
        const uint32_t x = root(r1[k]), y = root(r2[k]);
        parent[std::max(x, y)] = std::min(x, y);
    }
    for (uint64_t k = 0; k < pop_size; k++) parent[k] = root((uint32_t)k);
    cluster_finish(parent.data(), pop_size, labels, out);
    return PS_OK;
}

// the scratch on the core handle: the two count words, the `changed` word, the labels, the bit matrix
static int cluster_scratch(ps_population *c0, uint64_t N, unsigned long long **words, uint32_t **changed, uint32_t **L,
                           unsigned long long **adj, uint64_t *bytes)
{
    scratch_layout lay;
    const uint64_t o_words = lay.add(PS_CL_WORDS * 8, 8), o_changed = lay.add(8, 8), o_lab = lay.add(N * 4, 8);
    const uint64_t o_adj = lay.add(N * ((N + 63) / 64) * 8, 8);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(c0->ro[PS_RO_CLUSTERS], lay.bytes, &base, "cannot allocate the %llu bytes of the adjacency bit matrix and the labels of %llu individuals",
                      (unsigned long long)N));
    *words = (unsigned long long *)(base + o_words);
    *changed = (uint32_t *)(base + o_changed);
    *L = (uint32_t *)(base + o_lab);
    *adj = (unsigned long long *)(base + o_adj);
    *bytes = lay.bytes;
    return PS_OK;
}

template <bool CORE, bool ACC>
static int cluster_edge_launch(const pair_pipeline &pl, uint32_t lo, uint32_t nrows, const ps_cl_args &a, unsigned long long *adj,
                               unsigned long long *words)
{
    const uint32_t N = (uint32_t)pl.c0->cfg.pop_size;
    // the rows over y (the grid of pair_hist_launch without bins in LDS)
    const uint32_t gx = pair_grid_x(N), gy = std::max(1u, std::min(std::min(nrows, 65535u), 2048u / gx));
    hipLaunchKernelGGL((pair_edge_kernel<CORE, ACC>), dim3(gx, gy), dim3(256), 0, pl.sc, (const uint32_t *)pl.c0->d_cdavg, pl.src.b.ld, pl.In(),
                       pl.A.ld, (const uint32_t *)pl.A.rowcnt, N, lo, nrows, a, adj, words);
    HIPCHK(hipGetLastError());
    return PS_OK;
}

// The call behind the device entries: src holds the bands (open in internal order with a core criterion; without one its counts
// are not asked for), `acc` lives on src.c0's device, both streams are idle; `slot` is c0's current row map (rows_current).
static int cluster_device(core_band_source &src, ps_population *acc, uint64_t L, const ps_cluster_params *prm, const uint32_t *slot,
                          ps_cluster_t *out, uint32_t *labels)
{
    ps_population *c0 = src.c0;
    const uint32_t N = (uint32_t)c0->cfg.pop_size;
    const uint64_t cg = acc->cfg.core_genes;
    bool core_on, acc_on;
    PSCHK(cluster_check_params(prm, &core_on, &acc_on));
    const ps_cl_args a = cluster_args(prm, cg);
    PSCHK(use_device(c0));
    unsigned long long *d_words, *d_adj;
    uint32_t *d_changed, *d_L;
    uint64_t bytes;
    PSCHK(cluster_scratch(c0, N, &d_words, &d_changed, &d_L, &d_adj, &bytes));
    pair_pipeline pl(src, acc);
    hipStream_t sc = pl.sc;
    readout_slot &ro = c0->ro[PS_RO_CLUSTERS];
    HIPCHK(hipMemsetAsync(d_words, 0, bytes, sc));
    cluster_init_kernel<<<(N + 255u) / 256u, 256, 0, sc>>>(d_L, N);
    HIPCHK(hipGetLastError());
    ro.timed = false;
    PSCHK(pl.open(acc_on));
    // timer groups: 0 = both count phases, 1 = the edges, 2 = the labels
    PSCHK(pl.for_bands([&](uint32_t lo, uint32_t nrows) -> int {
        if (core_on) PSCHK(pl.core_counts(0, lo, nrows));
        PSCHK(pl.acc_counts(0, lo, nrows));
        return pl.consume(1, [&]() {
            return core_on && acc_on ? cluster_edge_launch<true, true>(pl, lo, nrows, a, d_adj, d_words)
                   : core_on         ? cluster_edge_launch<true, false>(pl, lo, nrows, a, d_adj, d_words)
                                     : cluster_edge_launch<false, true>(pl, lo, nrows, a, d_adj, d_words);
        });
    }));
    // the label rounds: labels only decrease and a label crosses at least one more edge per round, so a hook round that moves
    // nothing comes within N rounds
    uint64_t rounds = 0;
    PSCHK(pl.timed(2, sc, [&]() -> int {
        for (;;) {
            if (rounds == N) return ps_fail(PS_ERR_STATE, "the labels of %u individuals still moved in round %u", N, N);
            rounds++;
            uint32_t changed = 0;
            HIPCHK(hipMemsetAsync(d_changed, 0, sizeof(uint32_t), sc));
            cluster_hook_kernel<<<std::min((N + 3u) / 4u, 2048u), 256, 0, sc>>>(d_adj, N, d_L, d_changed);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&changed, d_changed, sizeof changed, hipMemcpyDeviceToHost, sc));
            HIPCHK(hipStreamSynchronize(sc));
            if (!changed) return PS_OK;
            cluster_jump_kernel<<<(N + 255u) / 256u, 256, 0, sc>>>(N, d_L);
            HIPCHK(hipGetLastError());
        }
    }));
    unsigned long long w[PS_CL_WORDS];
    std::vector<uint32_t> rep(N);
    HIPCHK(hipMemcpyAsync(w, d_words, sizeof w, hipMemcpyDeviceToHost, sc));
    HIPCHK(hipMemcpyAsync(rep.data(), d_L, (uint64_t)N * sizeof(uint32_t), hipMemcpyDeviceToHost, sc));
    PSCHK(pl.finish(ro, 3));
    rows_permute(rep.data(), slot, N);
    readout_head(out, N, (uint64_t)N * (N - 1) / 2, L, cg);
    out->edges = w[PS_CL_EDGES];
    out->undefined_pairs = w[PS_CL_UNDEF];
    out->rounds = rounds;
    cluster_finish(rep.data(), N, labels, out);
    return PS_OK;
}

// behind pair_entry: ps_strain_clusters (m == nullptr) and ps_multi_strain_clusters (core, acc: shard 0's handles; the edges and
// the labels on shard 0 against its accessory replica, the row map from shard 0's simulation)
static auto cluster_entry(const ps_cluster_params *prm, ps_cluster_t *out, uint32_t *labels)
{
    return [=](ps_multi *m, ps_population *core, ps_population *acc) -> int {
        bool core_on, acc_on;
        PSCHK(cluster_check_params(prm, &core_on, &acc_on));
        core_band_source src;
        const uint32_t *slot = nullptr;
        PSCHK(pair_source_open(&src, "strain_clusters", "strain clusters need", "compares", m, core, acc, core_on, &slot));
        return cluster_device(src, acc, m ? m->prm.core_size : core->cfg.global_cols, prm, slot, out, labels);
    };
}

extern "C" int ps_strain_clusters(ps_population *core, ps_population *acc, const ps_cluster_params *prm, ps_cluster_t *out,
                                  uint32_t *labels)
{
    return pair_entry(core, acc, prm && out && labels, cluster_entry(prm, out, labels));
}

extern "C" int ps_sim_strain_clusters(ps_sim *s, const ps_cluster_params *prm, ps_cluster_t *out, uint32_t *labels)
{
    return pair_entry(s, prm && out && labels, cluster_entry(prm, out, labels));
}

extern "C" int ps_strain_clusters_timing(ps_population *core, double *counts_ms, double *edges_ms, double *labels_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_CLUSTERS], "no strain clusters have been computed on this handle", { counts_ms, edges_ms, labels_ms });
}

extern "C" int ps_multi_strain_clusters(ps_multi *m, const ps_cluster_params *prm, ps_cluster_t *out, uint32_t *labels)
{
    return pair_entry(m, prm && out && labels, cluster_entry(prm, out, labels));
}
