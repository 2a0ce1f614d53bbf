// neighbour_joining.h -- ps_neighbour_joining / ps_sim_neighbour_joining / ps_multi_neighbour_joining, the host restatement
// ps_nj_from_counts and ps_nj_newick (include/pansim_hip.h; the definitions: docs/NEIGHBOUR_JOINING.md).  Included by
// pansim_capi.hip behind pair_readout.h, whose frame (pair_source_open, pair_pipeline, pair_entry) it reuses, and behind
// upgma_tree.h, whose cap on the population (PS_UPGMA_MAX_POP) is this read-out's too.
//
// As the UPGMA tree, everything on the device runs in INTERNAL row order: per band the numerators of the metric asked for, then a
// store kernel on the core stream that widens them into the band's rows of a full N x N matrix of f64 distances; after the last
// band the initial row sums and the N - 1 joins on the core stream (nj_kernels.h), two launches each and nothing read back
// between them: the number of active nodes is N - t on the host as on the device.  The joins compare nodes by their ids, the
// smallest OUTPUT row of a node (out_row, the inverse of the row slot), so the tree is the one of the reference's row order.  One
// copy of the records comes back; the host maps their rows to nodes.
#pragma once

#include "nj_kernels.h"

static const metric_names NJ_NAMES = { "a neighbour-joining tree", "PS_TREE_CORE", "PS_TREE_ACC" };

// the limits: the cap that keeps the matrix at 2 GB, and those of the metric
static int nj_check_limits(const ps_tree_params *prm, uint64_t N, uint64_t L, uint64_t cg)
{
    if (N < 2 || N > PS_UPGMA_MAX_POP)
        return ps_fail(PS_ERR_INVALID, "a neighbour-joining tree needs 2 <= pop_size <= 16384 (the matrix of f64 distances holds 2 GB at the cap), not %llu",
                       (unsigned long long)N);
    if (L >= (1ull << 32))
        return ps_fail(PS_ERR_INVALID, "a neighbour-joining tree needs fewer than 2^32 core sites, not %llu", (unsigned long long)L);
    if (prm->metric != PS_TREE_ACC) return PS_OK;
    if (cg < 1)
        return ps_fail(PS_ERR_INVALID, "the accessory metric of a neighbour-joining tree needs core_genes >= 1 (a pair without genes would be 0 / 0)");
    return metric_check_core_genes(prm->metric, cg, NJ_NAMES);
}

// the summary's tail from the finished lists
static void nj_tail(ps_nj_t *o, int32_t metric, uint64_t joins, const double *len_left, const double *len_right)
{
    o->metric = (uint64_t)metric;
    o->joins = joins;
    for (uint64_t k = 0; k < joins; k++) o->negative_branches += (len_left[k] < 0.0) + (len_right[k] < 0.0);
}

extern "C" int ps_nj_from_counts(const uint32_t *r1, const uint32_t *r2, const uint32_t *core_h, const uint32_t *acc_inter,
                                 const uint32_t *acc_union, uint64_t n_pairs, uint64_t pop_size, uint64_t core_sites, uint64_t core_genes,
                                 const ps_tree_params *prm, ps_nj_t *out, uint32_t *left, uint32_t *right, double *len_left, double *len_right)
{
    if (!prm || !out || !left || !right || !len_left || !len_right || !r1 || !r2) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(metric_check(prm->metric, NJ_NAMES));
    const bool acc = prm->metric == PS_TREE_ACC;
    const pair_list pairs = { r1, r2, core_h, acc_inter, acc_union, n_pairs, pop_size };
    if (pairs.lacks(!acc, acc)) return ps_fail(PS_ERR_INVALID, "null argument: the metric needs its numerators");
    PSCHK(nj_check_limits(prm, pop_size, core_sites, core_genes));
    const uint64_t N = pop_size;
    if (n_pairs != N * (N - 1) / 2)
        return ps_fail(PS_ERR_INVALID, "a neighbour-joining tree needs the complete list of all %llu pairs of %llu individuals, not %llu: the row sums are undefined on a partial list",
                       (unsigned long long)(N * (N - 1) / 2), (unsigned long long)N, (unsigned long long)n_pairs);
    // (N x N doubles and N x N bytes, 2.3 GB at the cap: a failed allocation is an error of the call, not an exception through the C ABI)
    std::vector<double> D, r(N, 0.0);
    std::vector<uint8_t> seen;
    try {
        D.assign(N * N, 0.0);
        seen.assign(N * N, 0);
    } catch (const std::bad_alloc &) {
        return ps_fail(PS_ERR_OOM, "cannot allocate the %llu bytes of the distances of all pairs of %llu individuals on the host",
                       (unsigned long long)(N * N * 9), (unsigned long long)N);
    }
    for (uint64_t k = 0; k < n_pairs; k++) {
        PSCHK(pairs.check_indices(k));
        const uint64_t x = (uint64_t)r1[k] * N + r2[k], y = (uint64_t)r2[k] * N + r1[k];
        if (seen[x])
            return ps_fail(PS_ERR_INVALID, "pair %llu: the pair (%u, %u) is listed twice", (unsigned long long)k, std::min(r1[k], r2[k]),
                           std::max(r1[k], r2[k]));
        seen[x] = seen[y] = 1;
        if (acc) PSCHK(pairs.check_acc(k, true));
        D[x] = D[y] = acc ? ps_nj_acc_distance(acc_inter[k], acc_union[k], core_genes) : ps_nj_core_distance(core_h[k]);
    }
    // (n_pairs distinct pairs of N (N - 1) / 2 possible ones: the list is complete)
    // The plain O(N^3) loop over nj_rule.h.  A node lives in the row of its id, so lo < hi as rows; node[i] = the node in row i.
    std::vector<uint32_t> alive(N), node(N);
    for (uint64_t i = 0; i < N; i++) {
        alive[i] = node[i] = (uint32_t)i;
        for (uint64_t k = 0; k < N; k++)                  // (ascending row k, from +0.0)
            if (k != i) r[i] += D[i * N + k];
    }
    for (uint64_t t = 0; t + 1 < N; t++) {                // (N - 1 trips: each retires one node)
        const uint32_t n = (uint32_t)(N - t);
        ps_nj_key best = { 0.0, PS_NJ_NONE, PS_NJ_NONE };
        for (size_t x = 0; x < alive.size(); x++)
            for (size_t y = x + 1; y < alive.size(); y++) {      // (alive ascends: lo = alive[x])
                const uint32_t lo = alive[x], hi = alive[y];
                const ps_nj_key e = { ps_nj_q(n, D[(uint64_t)lo * N + hi], r[lo], r[hi]), lo, hi };
                if (best.lo == PS_NJ_NONE || ps_nj_less(e, best)) best = e;
            }
        const uint32_t lo = best.lo, hi = best.hi;
        const double dlh = D[(uint64_t)lo * N + hi], r_lo = r[lo], r_hi = r[hi];
        ps_nj_branches(n, dlh, r_lo, r_hi, &len_left[t], &len_right[t]);
        left[t] = node[lo];
        right[t] = node[hi];
        node[lo] = (uint32_t)(N + t);
        for (uint32_t k : alive) {
            if (k == lo || k == hi) continue;
            const double dlk = D[(uint64_t)lo * N + k], dhk = D[(uint64_t)hi * N + k], duk = ps_nj_duk(dlk, dhk, dlh);
            r[k] = ps_nj_r_other(r[k], dlk, dhk, duk);
            D[(uint64_t)lo * N + k] = D[(uint64_t)k * N + lo] = duk;
        }
        r[lo] = ps_nj_r_joined(n, r_lo, r_hi, dlh);
        alive.erase(std::find(alive.begin(), alive.end(), hi));
    }
    readout_head(out, N, n_pairs, core_sites, core_genes);
    nj_tail(out, prm->metric, N - 1, len_left, len_right);
    return PS_OK;
}

// One line of Newick text for the join list, in the usual unrooted form with three subtrees at the top: the last join is
// dissolved, its child that is an inner node (the right one if both are) is opened -- that node's two children stand at the top
// level, left then right -- and the other child stands beside them with the length of the last edge, the sum of the last join's
// two lengths.  Two leaves alone are "(left:len,right:len);".  The walk keeps its own stack: a caterpillar is as deep as the
// population.
extern "C" int ps_nj_newick(const uint32_t *left, const uint32_t *right, const double *len_left, const double *len_right, uint64_t pop_size,
                            double scale, char *buf, uint64_t cap, uint64_t *needed)
{
    if (!left || !right || !len_left || !len_right || !needed) return ps_fail(PS_ERR_INVALID, "null argument");
    if (pop_size < 2 || pop_size > 0x7fffffffull)
        return ps_fail(PS_ERR_INVALID, "the Newick text of a neighbour-joining tree needs 2 <= pop_size < 2^31");
    if (!(scale > 0.0) || !std::isfinite(scale)) return ps_fail(PS_ERR_INVALID, "the Newick text of a neighbour-joining tree needs a finite scale > 0");
    const uint64_t N = pop_size, M = N - 1;
    std::vector<uint8_t> used(N + M, 0);
    for (uint64_t k = 0; k < M; k++)
        for (uint32_t c : { left[k], right[k] }) {
            if (c >= N + k || used[c])
                return ps_fail(PS_ERR_INVALID, "join %llu: child %u is not an earlier node that is still free", (unsigned long long)k, c);
            used[c] = 1;
        }
    struct frame { uint32_t node; double len; uint8_t next; };      // next: the child to visit (0, 1) or 2 = close
    std::vector<frame> st;
    std::string out;
    char text[64];
    // the subtree below `top` and the branch above it
    auto subtree = [&](uint32_t top, double len) {
        st.push_back({ top, len, 0 });
        while (!st.empty()) {                             // (every node is pushed once and visited three times at most)
            frame &f = st.back();
            if (f.node >= N && f.next < 2) {
                out += f.next == 0 ? '(' : ',';
                const uint64_t k = f.node - N;
                const uint32_t child = f.next == 0 ? left[k] : right[k];
                const double above = f.next == 0 ? len_left[k] : len_right[k];
                f.next++;
                st.push_back({ child, above, 0 });        // (f is not used behind this line)
                continue;
            }
            if (f.node < N) {
                snprintf(text, sizeof text, "%u", f.node);
                out += text;
            } else out += ')';
            out += ':';
            out.append(text, (size_t)ps_fmt_f64(f.len / scale, text, sizeof text));
            st.pop_back();
        }
    };
    const uint32_t a = left[M - 1], b = right[M - 1];
    out += '(';
    if (a < N && b < N) {                                 // (N == 2)
        subtree(a, len_left[M - 1]);
        out += ',';
        subtree(b, len_right[M - 1]);
    } else {
        const uint32_t open = b >= N ? b : a, other = b >= N ? a : b;
        subtree(left[open - N], len_left[open - N]);
        out += ',';
        subtree(right[open - N], len_right[open - N]);
        out += ',';
        subtree(other, len_left[M - 1] + len_right[M - 1]);
    }
    out += ");";
    *needed = out.size() + 1;
    if (!buf) return PS_OK;                               // (the size alone)
    if (cap < *needed)
        return ps_fail(PS_ERR_INVALID, "the Newick text needs %llu bytes with its terminating zero, the buffer holds %llu", (unsigned long long)*needed,
                       (unsigned long long)cap);
    memcpy(buf, out.c_str(), *needed);
    return PS_OK;
}

// the scratch on the core handle: id and the candidates' columns (N u32 each), the row order (N u32), the row sums and the
// candidates' q (N f64 each), the N join records, the matrix (N rows of ldm f64)
struct nj_scratch {
    uint32_t *id = nullptr, *order = nullptr, *cand_j = nullptr;
    double *r = nullptr, *cand_q = nullptr, *D = nullptr;
    ps_nj_rec *rec = nullptr;
    uint64_t ldm = 0;
};

static int nj_scratch_get(ps_population *c0, uint64_t N, nj_scratch *s)
{
    scratch_layout lay;
    s->ldm = (N + 63) & ~63ull;
    const uint64_t o_id = lay.add(N * 4, 16), o_order = lay.add(N * 4, 16), o_cj = lay.add(N * 4, 16);
    const uint64_t o_r = lay.add(N * 8, 16), o_cq = lay.add(N * 8, 16), o_rec = lay.add(N * sizeof(ps_nj_rec), 16);
    const uint64_t o_D = lay.add(N * s->ldm * 8, 16);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(c0->ro[PS_RO_NJ], lay.bytes, &base, "cannot allocate the %llu bytes of the distances of all pairs of %llu individuals",
                      (unsigned long long)N));
    s->id = (uint32_t *)(base + o_id);
    s->order = (uint32_t *)(base + o_order);
    s->cand_j = (uint32_t *)(base + o_cj);
    s->r = (double *)(base + o_r);
    s->cand_q = (double *)(base + o_cq);
    s->rec = (ps_nj_rec *)(base + o_rec);
    s->D = (double *)(base + o_D);
    return PS_OK;
}

static int nj_store_launch(const pair_pipeline &pl, bool acc, uint64_t cg, uint32_t lo, uint32_t nrows, const nj_scratch &s)
{
    const uint32_t N = (uint32_t)pl.c0->cfg.pop_size;
    const uint32_t gx = (uint32_t)((s.ldm / 2u + 255u) / 256u), gy = std::max(1u, std::min(nrows, 4096u));
    if (acc) nj_store_acc_kernel<<<dim3(gx, gy), 256, 0, pl.sc>>>(pl.In(), pl.A.ld, (const uint32_t *)pl.A.rowcnt, cg, N, lo, nrows, s.D, s.ldm);
    else nj_store_core_kernel<<<dim3(gx, gy), 256, 0, pl.sc>>>((const uint32_t *)pl.c0->d_cdavg, pl.src.b.ld, N, lo, nrows, s.D, s.ldm);
    HIPCHK(hipGetLastError());
    return PS_OK;
}

// The call behind the device entries: src holds the bands (open in internal order with the core metric; with the accessory
// metric its counts are not asked for), `acc` lives on src.c0's device, both streams are idle; `slot` is c0's current row map.
static int nj_device(core_band_source &src, ps_population *acc, uint64_t L, const ps_tree_params *prm, const uint32_t *slot, ps_nj_t *out,
                     uint32_t *left, uint32_t *right, double *len_left, double *len_right)
{
    ps_population *c0 = src.c0;
    const uint32_t N = (uint32_t)c0->cfg.pop_size;
    const uint64_t cg = acc->cfg.core_genes;
    const bool acc_metric = prm->metric == PS_TREE_ACC;
    PSCHK(use_device(c0));
    nj_scratch s;
    PSCHK(nj_scratch_get(c0, N, &s));
    // out_row[i] = the output row of internal row i, the id of the leaf that starts there; order[k] = the internal row of output
    // row k (the inverse of the inverse: a permutation of 0 .. N - 1 by construction)
    const std::vector<uint32_t> out_row = row_inverse(slot, N);
    std::vector<uint32_t> order(N);
    for (uint32_t i = 0; i < N; i++) {
        if (out_row[i] >= N) return ps_fail(PS_ERR_STATE, "the row map of %u individuals names row %u", N, out_row[i]);
        order[out_row[i]] = i;
    }
    readout_slot &ro = c0->ro[PS_RO_NJ];
    pair_pipeline pl(src, acc);
    hipStream_t sc = pl.sc;
    HIPCHK(hipMemcpyAsync(s.id, out_row.data(), (uint64_t)N * sizeof(uint32_t), hipMemcpyHostToDevice, sc));
    HIPCHK(hipMemcpyAsync(s.order, order.data(), (uint64_t)N * sizeof(uint32_t), hipMemcpyHostToDevice, sc));
    ro.timed = false;
    PSCHK(pl.open(acc_metric));
    // timer groups: 0 = the count phase, 1 = the store kernels and the row sums, 2 = the joins
    PSCHK(pl.for_bands([&](uint32_t lo, uint32_t nrows) -> int {
        if (!acc_metric) PSCHK(pl.core_counts(0, lo, nrows));
        else PSCHK(pl.acc_counts(0, lo, nrows));
        // (no accessory genes: In() is null and the store writes 0 / core_genes for every pair)
        return pl.consume(1, [&]() { return nj_store_launch(pl, acc_metric, cg, lo, nrows, s); });
    }));
    PSCHK(pl.timed(1, sc, [&]() -> int {
        nj_row_sum_kernel<<<(N + 255u) / 256u, 256, 0, sc>>>(s.D, s.ldm, N, s.order, s.r);
        HIPCHK(hipGetLastError());
        return PS_OK;
    }));
    const uint32_t gw = std::min((N + 3u) / 4u, 4096u);
    PSCHK(pl.timed(2, sc, [&]() -> int {
        for (uint32_t t = 0; t + 1u < N; t++) {           // (N - 1 trips; nothing is read back between them)
            nj_row_min_kernel<<<gw, 256, 0, sc>>>(s.D, s.ldm, N, N - t, s.id, s.r, s.cand_j, s.cand_q);
            nj_join_kernel<<<1, PS_NJ_JOIN_THREADS, 0, sc>>>(s.D, s.ldm, N, N - t, t, s.id, s.r, s.cand_j, s.cand_q, s.rec);
            HIPCHK(hipGetLastError());
        }
        return PS_OK;
    }));
    std::vector<ps_nj_rec> rec(N - 1u);
    HIPCHK(hipMemcpyAsync(rec.data(), s.rec, (uint64_t)(N - 1u) * sizeof(ps_nj_rec), hipMemcpyDeviceToHost, sc));
    PSCHK(pl.finish(ro, 3));
    // node[i] = the node that lives in internal row i, PS_NJ_NONE once the row has retired
    std::vector<uint32_t> node(out_row);
    for (uint32_t t = 0; t + 1u < N; t++) {
        const uint32_t lo = rec[t].lo, hi = rec[t].hi;
        if (lo >= N || hi >= N || lo == hi || node[lo] == PS_NJ_NONE || node[hi] == PS_NJ_NONE)
            return ps_fail(PS_ERR_STATE, "join %u of the neighbour-joining tree of %u individuals names the rows %u and %u", t, N, lo, hi);
        left[t] = node[lo];
        right[t] = node[hi];
        len_left[t] = rec[t].b_lo;
        len_right[t] = rec[t].b_hi;
        node[lo] = N + t;
        node[hi] = PS_NJ_NONE;
    }
    readout_head(out, N, (uint64_t)N * (N - 1) / 2, L, cg);
    nj_tail(out, prm->metric, N - 1u, len_left, len_right);
    return PS_OK;
}

// behind pair_entry: ps_neighbour_joining (m == nullptr) and ps_multi_neighbour_joining (core, acc: shard 0's handles; the matrix
// and the joins on shard 0 against its accessory replica, the row map from shard 0's simulation)
static auto nj_entry(const ps_tree_params *prm, ps_nj_t *out, uint32_t *left, uint32_t *right, double *len_left, double *len_right)
{
    return [=](ps_multi *m, ps_population *core, ps_population *acc) -> int {
        PSCHK(metric_check(prm->metric, NJ_NAMES));
        core_band_source src;
        const uint32_t *slot = nullptr;
        // (the handles first, then this read-out's own limits, all before anything is queued)
        PSCHK(pair_handles(core, acc, m ? "ps_multi_neighbour_joining" : "ps_neighbour_joining", "a neighbour-joining tree needs"));
        const uint64_t L = m ? m->prm.core_size : core->cfg.global_cols;
        PSCHK(nj_check_limits(prm, core->cfg.pop_size, L, acc->cfg.core_genes));
        PSCHK(pair_source_open(&src, "neighbour_joining", "a neighbour-joining tree needs", "joins", m, core, acc, prm->metric == PS_TREE_CORE,
                               &slot));
        return nj_device(src, acc, L, prm, slot, out, left, right, len_left, len_right);
    };
}

extern "C" int ps_neighbour_joining(ps_population *core, ps_population *acc, const ps_tree_params *prm, ps_nj_t *out, uint32_t *left,
                                    uint32_t *right, double *len_left, double *len_right)
{
    return pair_entry(core, acc, prm && out && left && right && len_left && len_right, nj_entry(prm, out, left, right, len_left, len_right));
}

extern "C" int ps_sim_neighbour_joining(ps_sim *s, const ps_tree_params *prm, ps_nj_t *out, uint32_t *left, uint32_t *right, double *len_left,
                                        double *len_right)
{
    return pair_entry(s, prm && out && left && right && len_left && len_right, nj_entry(prm, out, left, right, len_left, len_right));
}

extern "C" int ps_multi_neighbour_joining(ps_multi *m, const ps_tree_params *prm, ps_nj_t *out, uint32_t *left, uint32_t *right, double *len_left,
                                          double *len_right)
{
    return pair_entry(m, prm && out && left && right && len_left && len_right, nj_entry(prm, out, left, right, len_left, len_right));
}

extern "C" int ps_neighbour_joining_timing(ps_population *core, double *counts_ms, double *store_ms, double *joins_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_NJ], "no neighbour-joining tree has been computed on this handle", { counts_ms, store_ms, joins_ms });
}
