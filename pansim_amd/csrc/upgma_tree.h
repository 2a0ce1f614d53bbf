// upgma_tree.h -- ps_upgma_tree / ps_sim_upgma_tree / ps_multi_upgma_tree, the host restatement ps_upgma_from_counts and
// ps_upgma_newick (include/pansim_hip.h; the definitions: docs/UPGMA_TREE.md).  Included by pansim_capi.hip behind pair_readout.h,
// whose pair-list reader, metric checks, band pipeline (pair_source_open, pair_pipeline) and entry bodies it reuses.
//
// As the single-linkage tree, everything on the device runs in INTERNAL row order: per band the numerators of the metric asked
// for (the other metric's count kernels are not launched), then a store kernel on the core stream that widens them into the
// band's rows of a full N x N matrix of u64 sums; after the last band the rounds of mutual nearest neighbours on the core
// stream (upgma_kernels.h) until N - 1 merges are listed.  The rounds compare clusters by their ids, the smallest OUTPUT row of
// a cluster (out_row, the inverse of the row slot), so the tree is the one of the reference's row order; the host links the
// listed merges into nodes and puts them into the order in which the sequential algorithm performs them (upgma_finish).
#pragma once

#include <queue>

#include "upgma_kernels.h"

#define PS_UPGMA_MAX_POP 16384ull

// one merge in output rows: the two cluster ids (a < b), their sizes before the merge, the distance as it is compared (the
// core den without the factor L)
struct upgma_merge {
    uint64_t num, den;
    uint32_t a, b, size_a, size_b;
};

static const metric_names UPGMA_NAMES = { "a UPGMA tree", "PS_TREE_CORE", "PS_TREE_ACC" };

// the limits that keep every sum in u64 and every cross product in 128 bits
static int upgma_check_limits(const ps_tree_params *prm, uint64_t N, uint64_t L, uint64_t cg)
{
    if (N < 2 || N > PS_UPGMA_MAX_POP)
        return ps_fail(PS_ERR_INVALID, "a UPGMA tree needs 2 <= pop_size <= 16384 (the sums of a cluster pair stay below 2^58), not %llu",
                       (unsigned long long)N);
    if (L >= (1ull << 32)) return ps_fail(PS_ERR_INVALID, "a UPGMA tree needs fewer than 2^32 core sites, not %llu", (unsigned long long)L);
    if (prm->metric != PS_TREE_ACC) return PS_OK;
    if (cg < 1)
        return ps_fail(PS_ERR_INVALID, "the accessory metric of a UPGMA tree needs core_genes >= 1 (a pair without genes would be 0 / 0)");
    return metric_check_core_genes(prm->metric, cg, UPGMA_NAMES);
}

// m[0 .. N - 1): the merges of a tree over the ids 0 .. N - 1, each set of pairs that merged at the same time in one piece (the
// rounds' list, or the sequential list itself) -> the five arrays in the order the sequential algorithm performs the merges,
// and the summary fields that follow from them.  Linking: cur[id] = the node that holds cluster id now.  Ordering: a node is
// ready once both children are out; of the ready nodes the smallest under (distance, lo id, hi id) is the next one, since the
// globally smallest pair of the current clusters is always a ready merge of the final tree.
static int upgma_finish(const std::vector<upgma_merge> &m, uint64_t N, uint64_t den_scale, ps_upgma_t *o, uint32_t *left, uint32_t *right,
                        uint32_t *size, uint64_t *num, uint64_t *den)
{
    const uint32_t M = (uint32_t)m.size();                // (N - 1)
    std::vector<uint32_t> cur(N), ca(M), cb(M), parent(M, PS_UP_NONE), pending(M, 0u);
    for (uint64_t k = 0; k < N; k++) cur[k] = (uint32_t)k;
    for (uint32_t t = 0; t < M; t++) {
        if (m[t].a >= m[t].b || m[t].b >= N || m[t].den == 0)
            return ps_fail(PS_ERR_STATE, "merge %u of the UPGMA tree joins the clusters %u and %u of %llu", t, m[t].a, m[t].b, (unsigned long long)N);
        ca[t] = cur[m[t].a];
        cb[t] = cur[m[t].b];
        if (ca[t] == PS_UP_NONE || cb[t] == PS_UP_NONE)   // (an absorbed id does not come back)
            return ps_fail(PS_ERR_STATE, "merge %u of the UPGMA tree joins a cluster that is gone", t);
        for (uint32_t c : { ca[t], cb[t] })
            if (c >= N) {
                parent[c - N] = t;
                pending[t]++;
            }
        cur[m[t].a] = (uint32_t)N + t;
        cur[m[t].b] = PS_UP_NONE;
    }
    auto key = [&](uint32_t t) { return ps_up_key{ m[t].num, m[t].den, m[t].a, m[t].b }; };
    auto later = [&](uint32_t x, uint32_t y) { return ps_up_less(key(y), key(x)); };
    std::priority_queue<uint32_t, std::vector<uint32_t>, decltype(later)> ready(later);
    for (uint32_t t = 0; t < M; t++)
        if (!pending[t]) ready.push(t);
    std::vector<uint32_t> seq(M, PS_UP_NONE);             // temporary node -> its place in the sequential order
    uint32_t k = 0;
    for (; !ready.empty(); k++) {                         // (M trips: every node is pushed once)
        const uint32_t t = ready.top();
        ready.pop();
        seq[t] = k;
        left[k] = ca[t] < N ? ca[t] : (uint32_t)N + seq[ca[t] - N];
        right[k] = cb[t] < N ? cb[t] : (uint32_t)N + seq[cb[t] - N];
        size[k] = m[t].size_a + m[t].size_b;
        num[k] = m[t].num;
        den[k] = m[t].den * den_scale;
        if (k == 0 || ps_up_dist_cmp(num[k - 1], den[k - 1], num[k], den[k]) != 0) o->distinct_heights++;
        if (parent[t] != PS_UP_NONE && --pending[parent[t]] == 0) ready.push(parent[t]);
    }
    if (k != M) return ps_fail(PS_ERR_STATE, "the UPGMA tree of %llu individuals orders %u of %u merges", (unsigned long long)N, k, M);
    o->merges = M;
    o->root_num = M ? num[M - 1] : 0;
    o->root_den = M ? den[M - 1] : 0;
    return PS_OK;
}

extern "C" int ps_upgma_from_counts(const uint32_t *r1, const uint32_t *r2, const uint32_t *core_h, const uint32_t *acc_inter,
                                    const uint32_t *acc_union, uint64_t n_pairs, uint64_t pop_size, uint64_t core_sites, uint64_t core_genes,
                                    const ps_tree_params *prm, ps_upgma_t *out, uint32_t *left, uint32_t *right, uint32_t *size, uint64_t *num,
                                    uint64_t *den)
{
    if (!prm || !out || !left || !right || !size || !num || !den || !r1 || !r2) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(metric_check(prm->metric, UPGMA_NAMES));
    const bool acc = prm->metric == PS_TREE_ACC;
    const pair_list pairs = { r1, r2, core_h, acc_inter, acc_union, n_pairs, pop_size };
    if (pairs.lacks(!acc, acc)) return ps_fail(PS_ERR_INVALID, "null argument: the metric needs its numerators");
    PSCHK(upgma_check_limits(prm, pop_size, core_sites, core_genes));
    const uint64_t N = pop_size;
    if (n_pairs != N * (N - 1) / 2)
        return ps_fail(PS_ERR_INVALID, "a UPGMA tree needs the complete list of all %llu pairs of %llu individuals, not %llu: average linkage is undefined on a partial list",
                       (unsigned long long)(N * (N - 1) / 2), (unsigned long long)N, (unsigned long long)n_pairs);
    std::vector<uint64_t> S(N * N, 0), B(acc ? N * N : 0, 0);
    std::vector<uint8_t> seen(N * N, 0);
    for (uint64_t k = 0; k < n_pairs; k++) {
        PSCHK(pairs.check_indices(k));
        const uint64_t x = (uint64_t)r1[k] * N + r2[k], y = (uint64_t)r2[k] * N + r1[k];
        if (seen[x])
            return ps_fail(PS_ERR_INVALID, "pair %llu: the pair (%u, %u) is listed twice", (unsigned long long)k, std::min(r1[k], r2[k]),
                           std::max(r1[k], r2[k]));
        seen[x] = seen[y] = 1;
        if (acc) PSCHK(pairs.check_acc(k, true));
        // (the sums of a cluster pair start as the pair's own distance; the core den, L for every pair, is not summed)
        uint64_t num, den;
        pairs.distance(k, acc, core_sites, core_genes, &num, &den);
        S[x] = S[y] = num;
        if (acc) B[x] = B[y] = den;
    }
    // (n_pairs distinct pairs of N (N - 1) / 2 possible ones: the list is complete)
    // The sequential algorithm: N - 1 times the smallest pair of the current clusters under (distance, lo id, hi id).  A cluster
    // lives in the row of its id.  nn[c] = the nearest other cluster of c under that order, kept across the merges: the smallest
    // pair of all is the smallest of the N pairs (c, nn[c]); after a merge only a cluster whose neighbour took part looks at
    // every other cluster again, any other one compares its neighbour with the merged cluster.  O(N^2) when few do, O(N^3) at worst.
    std::vector<uint32_t> alive(N), csize(N, 1u), nn(N, PS_UP_NONE);
    for (uint64_t k = 0; k < N; k++) alive[k] = (uint32_t)k;
    auto key = [&](uint32_t x, uint32_t y) {
        const uint32_t a = std::min(x, y), b = std::max(x, y);
        return ps_up_key{ S[(uint64_t)a * N + b], acc ? B[(uint64_t)a * N + b] : (uint64_t)csize[a] * csize[b], a, b };
    };
    auto scan = [&](uint32_t c) {
        nn[c] = PS_UP_NONE;
        for (uint32_t o : alive)
            if (o != c && (nn[c] == PS_UP_NONE || ps_up_less(key(c, o), key(c, nn[c])))) nn[c] = o;
    };
    for (uint32_t c : alive) scan(c);
    std::vector<upgma_merge> m;
    m.reserve(N - 1);
    while (alive.size() > 1) {                            // (N - 1 trips: each removes one cluster)
        uint32_t at = alive[0];
        for (uint32_t c : alive)
            if (ps_up_less(key(c, nn[c]), key(at, nn[at]))) at = c;
        const ps_up_key best = key(at, nn[at]);
        const uint32_t a = best.lo, b = best.hi;
        m.push_back({ best.num, best.den, a, b, csize[a], csize[b] });
        for (uint32_t c : alive) {
            if (c == a || c == b) continue;
            S[(uint64_t)std::min(a, c) * N + std::max(a, c)] += S[(uint64_t)std::min(b, c) * N + std::max(b, c)];
            if (acc) B[(uint64_t)std::min(a, c) * N + std::max(a, c)] += B[(uint64_t)std::min(b, c) * N + std::max(b, c)];
        }
        csize[a] += csize[b];
        alive.erase(std::find(alive.begin(), alive.end(), b));
        if (alive.size() == 1) break;
        for (uint32_t c : alive) {
            if (c == a || nn[c] == a || nn[c] == b) scan(c);
            else if (ps_up_less(key(c, a), key(c, nn[c]))) nn[c] = a;
        }
    }
    readout_head(out, N, n_pairs, core_sites, core_genes);
    out->metric = (uint64_t)prm->metric;
    return upgma_finish(m, N, acc ? 1 : core_sites, out, left, right, size, num, den);
}

// One line of Newick text for the merge list: leaves are output rows, children left then right, the branch above a child half the
// difference of the two nodes' distances (a leaf's is 0).  The walk keeps its own stack: a caterpillar is as deep as the population.
extern "C" int ps_upgma_newick(const uint32_t *left, const uint32_t *right, const uint64_t *num, const uint64_t *den, uint64_t pop_size,
                               char *buf, uint64_t cap, uint64_t *needed)
{
    if (!left || !right || !num || !den || !needed) return ps_fail(PS_ERR_INVALID, "null argument");
    if (pop_size < 2 || pop_size > 0x7fffffffull) return ps_fail(PS_ERR_INVALID, "the Newick text of a UPGMA tree needs 2 <= pop_size < 2^31");
    const uint64_t N = pop_size, M = N - 1;
    std::vector<uint8_t> used(N + M, 0);
    for (uint64_t k = 0; k < M; k++) {
        for (uint32_t c : { left[k], right[k] }) {
            if (c >= N + k || used[c])
                return ps_fail(PS_ERR_INVALID, "merge %llu: child %u is not an earlier node that is still free", (unsigned long long)k, c);
            used[c] = 1;
        }
        if (den[k] == 0) return ps_fail(PS_ERR_INVALID, "merge %llu: den is 0", (unsigned long long)k);
    }
    auto height = [&](uint32_t node) { return node < N ? 0.0 : (double)num[node - N] / (double)den[node - N]; };
    struct frame { uint32_t node, parent; uint8_t next; };     // next: the child to visit (0, 1) or 2 = close
    std::vector<frame> st;
    std::string out;
    char text[64];
    st.push_back({ (uint32_t)(N + M - 1), PS_UP_NONE, 0 });
    while (!st.empty()) {                                 // (every node is pushed once and visited three times at most)
        frame &f = st.back();
        if (f.node >= N && f.next < 2) {
            out += f.next == 0 ? '(' : ',';
            const uint32_t child = f.next == 0 ? left[f.node - N] : right[f.node - N], self = f.node;
            f.next++;
            st.push_back({ child, self, 0 });             // (f is not used behind this line)
            continue;
        }
        if (f.node < N) {
            snprintf(text, sizeof text, "%u", f.node);
            out += text;
        } else out += ')';
        if (f.parent == PS_UP_NONE) out += ';';
        else {
            out += ':';
            out.append(text, (size_t)ps_fmt_f64(0.5 * (height(f.parent) - height(f.node)), text, sizeof text));
        }
        st.pop_back();
    }
    *needed = out.size() + 1;
    if (!buf) return PS_OK;                               // (the size alone)
    if (cap < *needed)
        return ps_fail(PS_ERR_INVALID, "the Newick text needs %llu bytes with its terminating zero, the buffer holds %llu", (unsigned long long)*needed,
                       (unsigned long long)cap);
    memcpy(buf, out.c_str(), *needed);
    return PS_OK;
}

// the scratch on the core handle: the merge counter, five arrays of N u32, two of N u64, the N merge records, the one or two
// matrices (N rows of ldm u64)
enum { PS_UP_ID = 0, PS_UP_SIZE, PS_UP_ACTIVE, PS_UP_NN, PS_UP_MATE, PS_UP_ARRAYS };

struct upgma_scratch {
    uint32_t *count = nullptr, *arr[PS_UP_ARRAYS] = {};
    uint64_t *nn_num = nullptr, *nn_den = nullptr, *S = nullptr, *B = nullptr;
    ps_up_rec *rec = nullptr;
    uint64_t ldm = 0;
};

static int upgma_scratch_get(ps_population *c0, uint64_t N, bool acc, upgma_scratch *s)
{
    scratch_layout lay;
    uint64_t o_arr[PS_UP_ARRAYS];
    s->ldm = (N + 63) & ~63ull;
    const uint64_t o_count = lay.add(16, 16);
    for (uint64_t &o : o_arr) o = lay.add(N * 4, 16);
    const uint64_t o_num = lay.add(N * 8, 16), o_den = lay.add(N * 8, 16), o_rec = lay.add(N * sizeof(ps_up_rec), 16);
    const uint64_t o_S = lay.add(N * s->ldm * 8, 16), o_B = lay.add(acc ? N * s->ldm * 8 : 0, 16);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(c0->ro[PS_RO_UPGMA], lay.bytes, &base, "cannot allocate the %llu bytes of the cluster sums of all pairs of %llu individuals",
                      (unsigned long long)N));
    s->count = (uint32_t *)(base + o_count);
    for (int k = 0; k < PS_UP_ARRAYS; k++) s->arr[k] = (uint32_t *)(base + o_arr[k]);
    s->nn_num = (uint64_t *)(base + o_num);
    s->nn_den = (uint64_t *)(base + o_den);
    s->rec = (ps_up_rec *)(base + o_rec);
    s->S = (uint64_t *)(base + o_S);
    s->B = acc ? (uint64_t *)(base + o_B) : nullptr;
    return PS_OK;
}

static int upgma_store_launch(const pair_pipeline &pl, bool acc, uint64_t cg, uint32_t lo, uint32_t nrows, const upgma_scratch &s)
{
    const uint32_t N = (uint32_t)pl.c0->cfg.pop_size;
    const uint32_t gx = (uint32_t)((s.ldm / 2u + 255u) / 256u), gy = std::max(1u, std::min(nrows, 4096u));
    if (acc) upgma_store_acc_kernel<<<dim3(gx, gy), 256, 0, pl.sc>>>(pl.In(), pl.A.ld, (const uint32_t *)pl.A.rowcnt, cg, N, lo, nrows, s.S, s.B, s.ldm);
    else upgma_store_core_kernel<<<dim3(gx, gy), 256, 0, pl.sc>>>((const uint32_t *)pl.c0->d_cdavg, pl.src.b.ld, N, lo, nrows, s.S, s.ldm);
    HIPCHK(hipGetLastError());
    return PS_OK;
}

// The call behind the device entries: src holds the bands (open in internal order with the core metric; with the accessory
// metric its counts are not asked for), `acc` lives on src.c0's device, both streams are idle; `slot` is c0's current row map.
static int upgma_device(core_band_source &src, ps_population *acc, uint64_t L, const ps_tree_params *prm, const uint32_t *slot, ps_upgma_t *out,
                        uint32_t *left, uint32_t *right, uint32_t *size, uint64_t *num, uint64_t *den)
{
    ps_population *c0 = src.c0;
    const uint32_t N = (uint32_t)c0->cfg.pop_size;
    const uint64_t cg = acc->cfg.core_genes;
    const bool acc_metric = prm->metric == PS_TREE_ACC;
    PSCHK(use_device(c0));
    upgma_scratch s;
    PSCHK(upgma_scratch_get(c0, N, acc_metric, &s));
    // out_row[i] = the output row of internal row i: the id of the cluster that starts there
    const std::vector<uint32_t> out_row = row_inverse(slot, N);
    readout_slot &ro = c0->ro[PS_RO_UPGMA];
    pair_pipeline pl(src, acc);
    hipStream_t sc = pl.sc;
    const uint32_t gn = (N + 255u) / 256u;
    HIPCHK(hipMemsetAsync(s.count, 0, 16, sc));
    HIPCHK(hipMemcpyAsync(s.arr[PS_UP_ID], out_row.data(), (uint64_t)N * sizeof(uint32_t), hipMemcpyHostToDevice, sc));
    upgma_init_kernel<<<gn, 256, 0, sc>>>(s.arr[PS_UP_SIZE], s.arr[PS_UP_ACTIVE], N);
    HIPCHK(hipGetLastError());
    ro.timed = false;
    PSCHK(pl.open(acc_metric));
    // timer groups: 0 = the count phase, 1 = the store kernels, 2 = the rounds
    PSCHK(pl.for_bands([&](uint32_t lo, uint32_t nrows) -> int {
        if (!acc_metric) PSCHK(pl.core_counts(0, lo, nrows));
        else PSCHK(pl.acc_counts(0, lo, nrows));
        // (no accessory genes: In() is null and the store writes a = 0, b = core_genes for every pair)
        return pl.consume(1, [&]() { return upgma_store_launch(pl, acc_metric, cg, lo, nrows, s); });
    }));
    // the rounds: the smallest pair of all is mutual, so every round merges at least one pair
    uint64_t rounds = 0;
    uint32_t count = 0;
    const uint32_t gw = std::min((N + 3u) / 4u, 4096u), gc = (uint32_t)((s.ldm + 255u) / 256u);
    PSCHK(pl.timed(2, sc, [&]() -> int {
        while (count < N - 1u) {                          // (N - 1 trips at most: cut below)
            if (rounds == N - 1u) return ps_fail(PS_ERR_STATE, "the UPGMA tree of %u individuals holds %u merges after %u rounds", N, count, N - 1u);
            rounds++;
            if (acc_metric)
                upgma_row_nn_kernel<true><<<gw, 256, 0, sc>>>(s.S, s.B, s.ldm, N, s.arr[PS_UP_ACTIVE], s.arr[PS_UP_SIZE], s.arr[PS_UP_ID],
                                                              s.arr[PS_UP_NN], s.nn_num, s.nn_den);
            else
                upgma_row_nn_kernel<false><<<gw, 256, 0, sc>>>(s.S, nullptr, s.ldm, N, s.arr[PS_UP_ACTIVE], s.arr[PS_UP_SIZE], s.arr[PS_UP_ID],
                                                               s.arr[PS_UP_NN], s.nn_num, s.nn_den);
            upgma_mutual_kernel<<<gn, 256, 0, sc>>>(N, s.arr[PS_UP_NN], s.nn_num, s.nn_den, s.arr[PS_UP_SIZE], s.arr[PS_UP_ID], (uint32_t)rounds,
                                                    s.arr[PS_UP_MATE], s.count, s.rec);
            HIPCHK(hipGetLastError());
            const uint32_t first = count;
            HIPCHK(hipMemcpyAsync(&count, s.count, sizeof count, hipMemcpyDeviceToHost, sc));
            HIPCHK(hipStreamSynchronize(sc));
            if (count > N - 1u) return ps_fail(PS_ERR_STATE, "the UPGMA tree of %u individuals lists %u merges", N, count);
            if (count == first) return ps_fail(PS_ERR_STATE, "round %llu of the UPGMA tree of %u individuals merged nothing", (unsigned long long)rounds, N);
            if (count == N - 1u) break;                   // (one cluster is left: its sums are not needed)
            const uint32_t n = count - first;
            if (acc_metric) {
                upgma_merge_rows_kernel<true><<<dim3(gc, std::min(n, 1024u)), 256, 0, sc>>>(s.rec, first, n, s.S, s.B, s.ldm);
                upgma_merge_cols_kernel<true><<<gw, 256, 0, sc>>>(s.rec, first, n, N, s.arr[PS_UP_ACTIVE], s.arr[PS_UP_MATE], s.arr[PS_UP_ID], s.S,
                                                                  s.B, s.ldm);
            } else {
                upgma_merge_rows_kernel<false><<<dim3(gc, std::min(n, 1024u)), 256, 0, sc>>>(s.rec, first, n, s.S, nullptr, s.ldm);
                upgma_merge_cols_kernel<false><<<gw, 256, 0, sc>>>(s.rec, first, n, N, s.arr[PS_UP_ACTIVE], s.arr[PS_UP_MATE], s.arr[PS_UP_ID], s.S,
                                                                   nullptr, s.ldm);
            }
            upgma_retire_kernel<<<gn, 256, 0, sc>>>(N, s.arr[PS_UP_MATE], s.arr[PS_UP_ID], s.arr[PS_UP_SIZE], s.arr[PS_UP_ACTIVE]);
            HIPCHK(hipGetLastError());
        }
        return PS_OK;
    }));
    std::vector<ps_up_rec> rec(N - 1u);
    HIPCHK(hipMemcpyAsync(rec.data(), s.rec, (uint64_t)(N - 1u) * sizeof(ps_up_rec), hipMemcpyDeviceToHost, sc));
    PSCHK(pl.finish(ro, 3));
    std::vector<upgma_merge> m(N - 1u);
    for (uint32_t k = 0; k + 1u < N; k++) {
        // (the list ascends by round, which upgma_finish links by)
        if (rec[k].a >= N || rec[k].b >= N || (k && rec[k].round < rec[k - 1u].round))
            return ps_fail(PS_ERR_STATE, "merge %u of the UPGMA tree joins rows %u and %u of %u in round %u", k, rec[k].a, rec[k].b, N, rec[k].round);
        m[k] = { rec[k].num, rec[k].den, out_row[rec[k].a], out_row[rec[k].b], rec[k].size_a, rec[k].size_b };
    }
    readout_head(out, N, (uint64_t)N * (N - 1) / 2, L, cg);
    out->metric = (uint64_t)prm->metric;
    out->rounds = rounds;
    return upgma_finish(m, N, acc_metric ? 1 : L, out, left, right, size, num, den);
}

// behind pair_entry: ps_upgma_tree (m == nullptr) and ps_multi_upgma_tree (core, acc: shard 0's handles; the matrix and the
// rounds on shard 0 against its accessory replica, the row map from shard 0's simulation)
static auto upgma_entry(const ps_tree_params *prm, ps_upgma_t *out, uint32_t *left, uint32_t *right, uint32_t *size, uint64_t *num,
                        uint64_t *den)
{
    return [=](ps_multi *m, ps_population *core, ps_population *acc) -> int {
        PSCHK(metric_check(prm->metric, UPGMA_NAMES));
        core_band_source src;
        const uint32_t *slot = nullptr;
        // (the handles first -- their order, the 65535 genes -- then this read-out's own limits, all before anything is queued;
        // pair_source_open checks the handles once more, which costs nothing)
        PSCHK(pair_handles(core, acc, m ? "ps_multi_upgma_tree" : "ps_upgma_tree", "a UPGMA tree needs"));
        const uint64_t L = m ? m->prm.core_size : core->cfg.global_cols;
        PSCHK(upgma_check_limits(prm, core->cfg.pop_size, L, acc->cfg.core_genes));
        PSCHK(pair_source_open(&src, "upgma_tree", "a UPGMA tree needs", "averages", m, core, acc, prm->metric == PS_TREE_CORE, &slot));
        return upgma_device(src, acc, L, prm, slot, out, left, right, size, num, den);
    };
}

extern "C" int ps_upgma_tree(ps_population *core, ps_population *acc, const ps_tree_params *prm, ps_upgma_t *out, uint32_t *left, uint32_t *right,
                             uint32_t *size, uint64_t *num, uint64_t *den)
{
    return pair_entry(core, acc, prm && out && left && right && size && num && den, upgma_entry(prm, out, left, right, size, num, den));
}

extern "C" int ps_sim_upgma_tree(ps_sim *s, const ps_tree_params *prm, ps_upgma_t *out, uint32_t *left, uint32_t *right, uint32_t *size,
                                 uint64_t *num, uint64_t *den)
{
    return pair_entry(s, prm && out && left && right && size && num && den, upgma_entry(prm, out, left, right, size, num, den));
}

extern "C" int ps_upgma_tree_timing(ps_population *core, double *counts_ms, double *store_ms, double *rounds_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_UPGMA], "no UPGMA tree has been computed on this handle", { counts_ms, store_ms, rounds_ms });
}

extern "C" int ps_multi_upgma_tree(ps_multi *m, const ps_tree_params *prm, ps_upgma_t *out, uint32_t *left, uint32_t *right, uint32_t *size,
                                   uint64_t *num, uint64_t *den)
{
    return pair_entry(m, prm && out && left && right && size && num && den, upgma_entry(prm, out, left, right, size, num, den));
}
