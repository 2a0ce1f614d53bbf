// nearest_neighbours.h -- ps_nearest_neighbours / ps_sim_nearest_neighbours / ps_multi_nearest_neighbours, the host restatement
// ps_neighbours_from_counts and the lineages ps_lineages_from_neighbours (include/pansim_hip.h; the definitions:
// docs/NEAREST_NEIGHBOURS.md).  Included by pansim_capi.hip behind pair_readout.h, whose pair-list reader, metric checks, band
// pipeline (pair_source_open, pair_pipeline) and entry bodies it reuses, and behind strain_clusters.h (cluster_finish).
//
// As the tree, everything on the device runs in INTERNAL row order: per band the numerators of the metric asked for (the other
// metric's count kernels are not launched), then knn_select_kernel on the core stream, which lists the k nearest columns of
// every row of the band.  A band holds complete rows, so nothing but the N k listed entries is kept.  The selection breaks ties
// by OUTPUT rows (out_row, the inverse of the row slot), so the lists are those of the reference's row order; the host maps
// rows and neighbours to output rows and fills the summary (knn_finish).
#pragma once

#include "knn_kernels.h"

static const metric_names KNN_NAMES = { "nearest neighbours", "PS_KNN_CORE", "PS_KNN_ACC" };

static int knn_check_params(const ps_knn_params *prm, uint64_t N)
{
    PSCHK(metric_check(prm->metric, KNN_NAMES));
    if (N < 2 || N > 0xffffffffull) return ps_fail(PS_ERR_INVALID, "nearest neighbours need 2 <= pop_size < 2^32");
    if (prm->k < 1 || prm->k > PS_KNN_MAX_K || prm->k > N - 1)
        return ps_fail(PS_ERR_INVALID, "nearest neighbours need 1 <= k <= min(pop_size - 1, %u), not k = %u of %llu individuals", PS_KNN_MAX_K,
                       prm->k, (unsigned long long)N);
    return PS_OK;
}

// The graph of the first r <= k entries of every list: `listed` = its directed entries {i -> j} (UINT32_MAX, i -> i and later
// copies of a j skipped), `mutual` = the unordered pairs listed from both ends; listed - mutual distinct unordered pairs.
// Every entry is UINT32_MAX or below N (the callers have checked).
static void knn_graph_counts(const uint32_t *nbr, uint64_t N, uint32_t k, uint32_t r, uint64_t *listed, uint64_t *mutual)
{
    std::vector<uint32_t> s(N * r, UINT32_MAX);                     // row i: its distinct neighbours ascending, then UINT32_MAX
    std::vector<uint32_t> len(N, 0);
    for (uint64_t i = 0; i < N; i++) {
        uint32_t *row = s.data() + i * r;
        uint32_t n = 0;
        for (uint32_t q = 0; q < r; q++) {
            const uint32_t j = nbr[i * k + q];
            if (j != UINT32_MAX && j != i) row[n++] = j;
        }
        std::sort(row, row + n);
        len[i] = (uint32_t)(std::unique(row, row + n) - row);
    }
    uint64_t d = 0, both = 0;
    for (uint64_t i = 0; i < N; i++) {
        const uint32_t *row = s.data() + i * r;
        d += len[i];
        for (uint32_t q = 0; q < len[i]; q++) {
            const uint32_t *other = s.data() + (uint64_t)row[q] * r;
            both += std::binary_search(other, other + len[row[q]], (uint32_t)i) ? 1 : 0;
        }
    }
    *listed = d;
    *mutual = both / 2;
}

// nbr, num, den in their final index space -> the summary fields that follow from them
static void knn_finish(ps_knn_t *o, const uint32_t *nbr, const uint64_t *den)
{
    const uint64_t N = o->pop_size, k = o->k;
    for (uint64_t e = 0; e < N * k; e++) o->undefined_neighbours += (nbr[e] != UINT32_MAX && den[e] == 0) ? 1 : 0;
    uint64_t listed, mutual;
    knn_graph_counts(nbr, N, (uint32_t)k, (uint32_t)k, &listed, &mutual);
    o->graph_edges = listed - mutual;
    o->mutual_edges = mutual;
}

extern "C" int ps_lineages_from_neighbours(const uint32_t *nbr, uint64_t pop_size, uint32_t k, uint32_t rank, ps_lineage_t *out,
                                           uint32_t *labels)
{
    if (!nbr || !out || !labels) return ps_fail(PS_ERR_INVALID, "null argument");
    if (pop_size < 1 || pop_size > 0xffffffffull) return ps_fail(PS_ERR_INVALID, "lineages need 1 <= pop_size < 2^32");
    if (k < 1) return ps_fail(PS_ERR_INVALID, "lineages need k >= 1");
    if (rank < 1 || rank > k) return ps_fail(PS_ERR_INVALID, "the rank of the lineages is 1 .. k = %u, not %u", k, rank);
    for (uint64_t e = 0; e < pop_size * k; e++)
        if (nbr[e] != UINT32_MAX && nbr[e] >= pop_size)
            return ps_fail(PS_ERR_INVALID, "entry %llu of individual %llu: index %u is not below pop_size %llu", (unsigned long long)(e % k),
                           (unsigned long long)(e / k), nbr[e], (unsigned long long)pop_size);
    // union-find, the smaller root kept: root(i) is the smallest member of i's set
    std::vector<uint32_t> parent(pop_size);
    for (uint64_t i = 0; i < pop_size; i++) parent[i] = (uint32_t)i;
    auto root = [&](uint32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    for (uint64_t i = 0; i < pop_size; i++)
        for (uint32_t q = 0; q < rank; q++) {
            const uint32_t j = nbr[i * k + q];
            if (j == UINT32_MAX) continue;
            const uint32_t x = root((uint32_t)i), y = root(j);
            parent[std::max(x, y)] = std::min(x, y);
        }
    for (uint64_t i = 0; i < pop_size; i++) parent[i] = root((uint32_t)i);
    ps_cluster_t c;
    memset(&c, 0, sizeof c);
    cluster_finish(parent.data(), pop_size, labels, &c);
    uint64_t listed, mutual;
    knn_graph_counts(nbr, pop_size, k, rank, &listed, &mutual);
    memset(out, 0, sizeof *out);
    out->pop_size = pop_size;
    out->rank = rank;
    out->edges = listed - mutual;
    out->lineages = c.clusters;
    out->largest_lineage = c.largest_cluster;
    out->within_pairs = c.within_pairs;
    return PS_OK;
}

extern "C" int ps_neighbours_from_counts(const uint32_t *r1, const uint32_t *r2, const uint32_t *core_h, const uint32_t *acc_inter,
                                         const uint32_t *acc_union, uint64_t n_pairs, uint64_t pop_size, uint64_t core_sites,
                                         uint64_t core_genes, const ps_knn_params *prm, ps_knn_t *out, uint32_t *nbr, uint64_t *num,
                                         uint64_t *den)
{
    if (!prm || !out || !nbr || !num || !den || (n_pairs && (!r1 || !r2))) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(knn_check_params(prm, pop_size));
    const bool acc = prm->metric == PS_KNN_ACC;
    const pair_list pairs = { r1, r2, core_h, acc_inter, acc_union, n_pairs, pop_size };
    if (n_pairs && pairs.lacks(!acc, acc))
        return ps_fail(PS_ERR_INVALID, "null argument: the metric needs its numerators");
    PSCHK(metric_check_core_genes(prm->metric, core_genes, KNN_NAMES));
    const uint32_t k = prm->k;
    // the partners of every individual in the order of the list (both ends of a pair): first[i] .. first[i + 1]
    std::vector<uint64_t> first(pop_size + 1, 0);
    for (uint64_t p = 0; p < n_pairs; p++) {
        PSCHK(pairs.check(p, acc));
        first[r1[p] + 1]++;
        first[r2[p] + 1]++;
    }
    for (uint64_t i = 0; i < pop_size; i++) first[i + 1] += first[i];
    struct cand { uint64_t num, den; uint32_t j; };
    std::vector<cand> all(2 * n_pairs);
    std::vector<uint64_t> fill(first.begin(), first.end() - 1);
    for (uint64_t p = 0; p < n_pairs; p++) {
        cand c;
        pairs.distance(p, acc, core_sites, core_genes, &c.num, &c.den);
        c.j = r2[p];
        all[fill[r1[p]]++] = c;
        c.j = r1[p];
        all[fill[r2[p]]++] = c;
    }
    for (uint64_t i = 0; i < pop_size; i++) {
        // stable: of the copies of a pair at one distance the earlier one of the list comes first; a neighbour is listed once
        std::stable_sort(all.begin() + first[i], all.begin() + first[i + 1],
                         [](const cand &a, const cand &b) { return ps_knn_less(a.num, a.den, a.j, b.num, b.den, b.j); });
        uint32_t n = 0;
        for (uint64_t e = first[i]; e < first[i + 1] && n < k; e++) {
            bool seen = false;
            for (uint32_t q = 0; q < n && !seen; q++) seen = nbr[i * k + q] == all[e].j;      // (n < k <= 128)
            if (seen) continue;
            nbr[i * k + n] = all[e].j;
            num[i * k + n] = all[e].num;
            den[i * k + n] = all[e].den;
            n++;
        }
        for (; n < k; n++) {
            nbr[i * k + n] = UINT32_MAX;
            num[i * k + n] = den[i * k + n] = 0;
        }
    }
    readout_head(out, pop_size, n_pairs, core_sites, core_genes);
    out->metric = (uint64_t)prm->metric;
    out->k = k;
    knn_finish(out, nbr, den);
    return PS_OK;
}

// the scratch on the core handle: out_row, then the lists (internal neighbour, num, and den under the accessory metric), N k each
struct knn_scratch {
    uint32_t *out_row = nullptr, *j = nullptr, *num = nullptr, *den = nullptr;
};

static int knn_scratch_get(ps_population *c0, uint64_t N, uint32_t k, bool acc, knn_scratch *s)
{
    scratch_layout lay;
    const uint64_t o_row = lay.add(N * 4, 16), o_j = lay.add(N * k * 4, 16), o_num = lay.add(N * k * 4, 16);
    const uint64_t o_den = acc ? lay.add(N * k * 4, 16) : 0;
    uint8_t *base = nullptr;
    PSCHK(scratch_get(c0->ro[PS_RO_KNN], lay.bytes, &base, "cannot allocate the %llu bytes of the %u nearest neighbours of %llu individuals", k,
                      (unsigned long long)N));
    s->out_row = (uint32_t *)(base + o_row);
    s->j = (uint32_t *)(base + o_j);
    s->num = (uint32_t *)(base + o_num);
    s->den = acc ? (uint32_t *)(base + o_den) : nullptr;
    return PS_OK;
}

static int knn_select_launch(const pair_pipeline &pl, bool acc, uint64_t cg, uint32_t lo, uint32_t nrows, uint32_t k, const knn_scratch &s)
{
    const uint32_t N = (uint32_t)pl.c0->cfg.pop_size;
    // one wave per row up to 4096 workgroups, the waves striding over the rows beyond
    const uint32_t gw = std::max(1u, std::min((nrows + 3u) / 4u, 4096u));
    if (acc)
        knn_select_kernel<true><<<gw, 256, 0, pl.sc>>>(nullptr, 0, pl.In(), pl.A.ld, (const uint32_t *)pl.A.rowcnt, cg, N, lo, nrows, k, s.out_row,
                                                       s.j, s.num, s.den);
    else
        knn_select_kernel<false><<<gw, 256, 0, pl.sc>>>((const uint32_t *)pl.c0->d_cdavg, pl.src.b.ld, nullptr, 0, nullptr, cg, N, lo, nrows, k,
                                                        s.out_row, s.j, s.num, s.den);
    HIPCHK(hipGetLastError());
    return PS_OK;
}

// The call behind the device entries: src holds the bands (open in internal order with the core metric; with the accessory
// metric its counts are not asked for), `acc` lives on src.c0's device, both streams are idle; `slot` is c0's current row map.
static int knn_device(core_band_source &src, ps_population *acc, uint64_t L, const ps_knn_params *prm, const uint32_t *slot, ps_knn_t *out,
                      uint32_t *nbr_out, uint64_t *num_out, uint64_t *den_out)
{
    ps_population *c0 = src.c0;
    const uint32_t N = (uint32_t)c0->cfg.pop_size, k = prm->k;
    const uint64_t cg = acc->cfg.core_genes, nk = (uint64_t)N * k;
    const bool acc_metric = prm->metric == PS_KNN_ACC;
    PSCHK(metric_check_core_genes(prm->metric, cg, KNN_NAMES));
    PSCHK(use_device(c0));
    knn_scratch s;
    PSCHK(knn_scratch_get(c0, N, k, acc_metric, &s));
    // out_row[i] = the output row of internal row i
    const std::vector<uint32_t> out_row = row_inverse(slot, N);
    readout_slot &ro = c0->ro[PS_RO_KNN];
    pair_pipeline pl(src, acc);
    hipStream_t sc = pl.sc;
    HIPCHK(hipMemcpyAsync(s.out_row, out_row.data(), (uint64_t)N * sizeof(uint32_t), hipMemcpyHostToDevice, sc));
    // (a row that no band covered would read as UINT32_MAX and fail the check below)
    HIPCHK(hipMemsetAsync(s.j, 0xff, nk * sizeof(uint32_t), sc));
    ro.timed = false;
    PSCHK(pl.open(acc_metric));
    // timer groups: 0 = the count phase, 1 = the select kernels
    PSCHK(pl.for_bands([&](uint32_t lo, uint32_t nrows) -> int {
        if (!acc_metric) PSCHK(pl.core_counts(0, lo, nrows));
        else PSCHK(pl.acc_counts(0, lo, nrows));
        return pl.consume(1, [&]() { return knn_select_launch(pl, acc_metric, cg, lo, nrows, k, s); });
    }));
    std::vector<uint32_t> hj(nk), hn(nk), hd(acc_metric ? nk : 0);
    HIPCHK(hipMemcpyAsync(hj.data(), s.j, nk * sizeof(uint32_t), hipMemcpyDeviceToHost, sc));
    HIPCHK(hipMemcpyAsync(hn.data(), s.num, nk * sizeof(uint32_t), hipMemcpyDeviceToHost, sc));
    if (acc_metric) HIPCHK(hipMemcpyAsync(hd.data(), s.den, nk * sizeof(uint32_t), hipMemcpyDeviceToHost, sc));
    PSCHK(pl.finish(ro, 2));
    // internal rows -> output rows, for the lists and for their entries; L back as the core den
    for (uint32_t i = 0; i < N; i++) {
        const uint64_t from = (uint64_t)i * k, to = (uint64_t)out_row[i] * k;
        for (uint32_t q = 0; q < k; q++) {
            const uint32_t j = hj[from + q];
            if (j >= N || j == i) return ps_fail(PS_ERR_STATE, "neighbour %u of internal row %u of %u is row %u", q, i, N, j);
            nbr_out[to + q] = out_row[j];
            num_out[to + q] = hn[from + q];
            den_out[to + q] = acc_metric ? (uint64_t)hd[from + q] : L;
        }
    }
    readout_head(out, N, (uint64_t)N * (N - 1) / 2, L, cg);
    out->metric = (uint64_t)prm->metric;
    out->k = k;
    knn_finish(out, nbr_out, den_out);
    return PS_OK;
}

// behind pair_entry: ps_nearest_neighbours (m == nullptr) and ps_multi_nearest_neighbours (core, acc: shard 0's handles; the
// selection on shard 0 against its accessory replica, the row map from shard 0's simulation)
static auto knn_entry(const ps_knn_params *prm, ps_knn_t *out, uint32_t *nbr, uint64_t *num, uint64_t *den)
{
    return [=](ps_multi *m, ps_population *core, ps_population *acc) -> int {
        PSCHK(knn_check_params(prm, core->cfg.pop_size));
        core_band_source src;
        const uint32_t *slot = nullptr;
        PSCHK(pair_source_open(&src, "nearest_neighbours", "nearest neighbours need", "compares", m, core, acc, prm->metric == PS_KNN_CORE, &slot));
        return knn_device(src, acc, m ? m->prm.core_size : core->cfg.global_cols, prm, slot, out, nbr, num, den);
    };
}

extern "C" int ps_nearest_neighbours(ps_population *core, ps_population *acc, const ps_knn_params *prm, ps_knn_t *out, uint32_t *nbr,
                                     uint64_t *num, uint64_t *den)
{
    return pair_entry(core, acc, prm && out && nbr && num && den, knn_entry(prm, out, nbr, num, den));
}

extern "C" int ps_sim_nearest_neighbours(ps_sim *s, const ps_knn_params *prm, ps_knn_t *out, uint32_t *nbr, uint64_t *num, uint64_t *den)
{
    return pair_entry(s, prm && out && nbr && num && den, knn_entry(prm, out, nbr, num, den));
}

extern "C" int ps_nearest_neighbours_timing(ps_population *core, double *counts_ms, double *select_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_KNN], "no nearest neighbours have been computed on this handle", { counts_ms, select_ms });
}

extern "C" int ps_multi_nearest_neighbours(ps_multi *m, const ps_knn_params *prm, ps_knn_t *out, uint32_t *nbr, uint64_t *num, uint64_t *den)
{
    return pair_entry(m, prm && out && nbr && num && den, knn_entry(prm, out, nbr, num, den));
}
