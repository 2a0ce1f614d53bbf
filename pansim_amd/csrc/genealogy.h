// genealogy.h -- the recorded genealogy of a run (include/pansim_hip.h; the definitions: docs/GENEALOGY.md): the switch of the
// recording (ps_sim_record_ancestry; the copy itself sits in sim_accessory_half), the comb of the present population
// (ps_sim_genealogy / ps_multi_genealogy: ancestry_comb_kernel, the finish on the host) and the host-only read-outs of a comb
// (ps_genealogy_pair / _pairs / _clusters / _newick).  Included by pansim_capi.hip behind nearest_neighbours.h.
//
// The comb: order[r] = the output row of internal row r, coal[r] = the coalescence time of internal rows r and r + 1
// (PS_GEN_BEYOND: none inside the record).  Every parent map is non-decreasing in the internal row, so the time of any two
// internal rows i < j is max(coal[i .. j - 1]) and the individuals that share an ancestor are contiguous.
#pragma once

#include "ancestry_kernels.h"

// levels of the sparse table over the N - 1 entries of a comb: the largest range is N - 1 >= 2^(levels - 1)
static uint32_t gen_levels(uint64_t N)
{
    uint32_t k = 1;
    while (N > 1 && ((uint64_t)2 << (k - 1)) <= N - 1) k++;
    return k;
}

// range maxima on the host: level k holds max(coal[r .. r + 2^k - 1]); the same table ancestry_table_kernel builds
struct gen_host_table {
    std::vector<std::vector<uint32_t>> lev;
    explicit gen_host_table(const uint32_t *coal, uint64_t N)
    {
        const uint64_t n = N ? N - 1 : 0;
        lev.emplace_back(coal, coal + n);
        for (uint64_t half = 1; 2 * half <= n; half *= 2) {
            const std::vector<uint32_t> &p = lev.back();
            std::vector<uint32_t> q(n - 2 * half + 1);
            for (uint64_t r = 0; r < q.size(); r++) q[r] = std::max(p[r], p[r + half]);
            lev.push_back(std::move(q));
        }
    }
    // max(coal[i .. j - 1]) for internal rows i < j
    uint32_t tmrca(uint64_t i, uint64_t j) const
    {
        const uint32_t k = 63u - (uint32_t)__builtin_clzll(j - i);
        return std::max(lev[k][i], lev[k][j - ((uint64_t)1 << k)]);
    }
};

// order is a permutation of 0 .. N - 1 -> rank, its inverse (the internal row of every output row)
static int gen_rank(const uint32_t *order, uint64_t N, std::vector<uint32_t> *rank)
{
    if (N < 1 || N > 0xffffffffull) return ps_fail(PS_ERR_INVALID, "a genealogy needs 1 <= pop_size < 2^32");
    rank->assign(N, UINT32_MAX);
    for (uint64_t r = 0; r < N; r++) {
        if (order[r] >= N) return ps_fail(PS_ERR_INVALID, "order[%llu] = %u is not below pop_size %llu", (unsigned long long)r, order[r], (unsigned long long)N);
        if ((*rank)[order[r]] != UINT32_MAX) return ps_fail(PS_ERR_INVALID, "order lists row %u twice: it must be a permutation", order[r]);
        (*rank)[order[r]] = (uint32_t)r;
    }
    return PS_OK;
}

// the summary fields that follow from the comb (shared by the device path)
static void gen_finish(ps_genealogy_t *o, const uint32_t *coal)
{
    uint64_t beyond = 0;
    uint32_t mx = 0;
    for (uint64_t r = 0; r + 1 < o->pop_size; r++) {
        beyond += coal[r] == PS_GEN_BEYOND ? 1 : 0;
        mx = std::max(mx, coal[r]);
    }
    o->roots = 1 + beyond;
    o->tmrca = beyond ? 0 : mx;
}

extern "C" int ps_genealogy_pairs(const uint32_t *order, const uint32_t *coal, uint64_t pop_size, const uint32_t *r1, const uint32_t *r2,
                                  uint64_t n_pairs, uint32_t *t)
{
    if (!order || (pop_size > 1 && !coal) || !t || (n_pairs && (!r1 || !r2))) return ps_fail(PS_ERR_INVALID, "null argument");
    std::vector<uint32_t> rank;
    PSCHK(gen_rank(order, pop_size, &rank));
    const gen_host_table tab(coal, pop_size);
    for (uint64_t p = 0; p < n_pairs; p++) {
        if (r1[p] >= pop_size || r2[p] >= pop_size)
            return ps_fail(PS_ERR_INVALID, "pair %llu: index %u is not below pop_size %llu", (unsigned long long)p, std::max(r1[p], r2[p]),
                           (unsigned long long)pop_size);
        const uint32_t a = rank[r1[p]], b = rank[r2[p]];
        t[p] = a == b ? 0u : tab.tmrca(std::min(a, b), std::max(a, b));
    }
    return PS_OK;
}

extern "C" int ps_genealogy_pair(const uint32_t *order, const uint32_t *coal, uint64_t pop_size, uint32_t i, uint32_t j, uint32_t *t)
{
    return ps_genealogy_pairs(order, coal, pop_size, &i, &j, 1, t);
}

extern "C" int ps_genealogy_clusters(const uint32_t *order, const uint32_t *coal, uint64_t pop_size, uint32_t depth, uint32_t t,
                                     uint32_t *labels, ps_gen_clusters_t *out)
{
    if (!order || (pop_size > 1 && !coal) || !labels || !out) return ps_fail(PS_ERR_INVALID, "null argument");
    std::vector<uint32_t> rank;
    PSCHK(gen_rank(order, pop_size, &rank));
    if (t > depth)
        return ps_fail(PS_ERR_INVALID, "the look-back of the true clusters is 0 .. depth = %u generations, not %u: the record does not reach further", depth, t);
    // a cluster = a run of internal rows whose neighbours coalesce within t; its representative = the run's first row
    std::vector<uint32_t> rep(pop_size);
    uint32_t start = order[0];
    for (uint64_t r = 0; r < pop_size; r++) {
        if (r && coal[r - 1] > t) start = order[r];
        rep[order[r]] = start;
    }
    ps_cluster_t c;
    memset(&c, 0, sizeof c);
    cluster_finish(rep.data(), pop_size, labels, &c);
    memset(out, 0, sizeof *out);
    out->clusters = c.clusters;
    out->largest = c.largest_cluster;
    out->within_pairs = c.within_pairs;
    return PS_OK;
}

// The trees of the comb as text, one per root.  The tree of the leaves [a, b] (internal rows): the leaf's output row when
// a == b; else m = max(coal[a .. b - 1]), the segment split at EVERY position whose time is m, the parts in comb order as
// (child:len,...), len = m - the child's own height.  An explicit stack: a caterpillar is as deep as the population.
static std::string gen_newick(const uint32_t *order, const uint32_t *coal, uint64_t N)
{
    // leftmost position of the maximum of coal[x .. y]: sparse table of positions
    const uint64_t n = N - 1;
    std::vector<std::vector<uint32_t>> arg;
    {
        std::vector<uint32_t> id(n);
        for (uint64_t r = 0; r < n; r++) id[r] = (uint32_t)r;
        arg.push_back(std::move(id));
        for (uint64_t half = 1; 2 * half <= n; half *= 2) {
            const std::vector<uint32_t> &p = arg.back();
            std::vector<uint32_t> q(n - 2 * half + 1);
            for (uint64_t r = 0; r < q.size(); r++) q[r] = coal[p[r + half]] > coal[p[r]] ? p[r + half] : p[r];
            arg.push_back(std::move(q));
        }
    }
    auto argmax = [&](uint64_t x, uint64_t y) -> uint32_t {          // x <= y
        const uint32_t k = 63u - (uint32_t)__builtin_clzll(y - x + 1);
        const uint32_t l = arg[k][x], r = arg[k][y + 1 - ((uint64_t)1 << k)];
        return coal[r] > coal[l] ? r : l;
    };
    struct frame { uint64_t a, b, cursor; uint32_t m, parent_m; bool has_parent, opened; };
    std::string out;
    std::vector<frame> st;
    char num[32];
    auto close = [&](const frame &f, uint32_t height) {
        if (f.has_parent) {
            snprintf(num, sizeof num, ":%u", f.parent_m - height);
            out += num;
        } else out += ";\n";
    };
    for (uint64_t a = 0; a < N;) {
        uint64_t b = a;
        while (b + 1 < N && coal[b] != PS_GEN_BEYOND) b++;
        st.push_back({ a, b, a, 0u, 0u, false, false });
        while (!st.empty()) {
            frame &f = st.back();
            if (f.a == f.b) {
                snprintf(num, sizeof num, "%u", order[f.a]);
                out += num;
                close(f, 0u);
                st.pop_back();
                continue;
            }
            if (!f.opened) {
                f.m = coal[argmax(f.a, f.b - 1)];
                f.opened = true;
                out += '(';
            }
            if (f.cursor > f.b) {
                out += ')';
                close(f, f.m);
                st.pop_back();
                continue;
            }
            if (f.cursor != f.a) out += ',';
            // the next child ends at the next position of time m, or with the segment
            uint64_t p = f.b;
            if (f.cursor < f.b) {
                const uint32_t q = argmax(f.cursor, f.b - 1);
                if (coal[q] == f.m) p = q;
            }
            const frame child = { f.cursor, p, f.cursor, 0u, f.m, true, false };
            f.cursor = p + 1;
            st.push_back(child);          // (f is not used behind this line)
        }
        a = b + 1;
    }
    return out;
}

extern "C" int ps_genealogy_newick(const uint32_t *order, const uint32_t *coal, uint64_t pop_size, char *buf, uint64_t cap, uint64_t *needed)
{
    if (!order || (pop_size > 1 && !coal) || !needed) return ps_fail(PS_ERR_INVALID, "null argument");
    std::vector<uint32_t> rank;
    PSCHK(gen_rank(order, pop_size, &rank));
    for (uint64_t r = 0; r + 1 < pop_size; r++)
        if (coal[r] == 0) return ps_fail(PS_ERR_INVALID, "coal[%llu] = 0: two individuals coalesce at least one generation back", (unsigned long long)r);
    const std::string text = gen_newick(order, coal, pop_size);
    *needed = text.size() + 1;
    if (!buf) return PS_OK;                     // (the size alone)
    if (cap < *needed)
        return ps_fail(PS_ERR_INVALID, "the Newick text needs %llu bytes with its terminating zero, the buffer holds %llu", (unsigned long long)*needed,
                       (unsigned long long)cap);
    memcpy(buf, text.c_str(), *needed);
    return PS_OK;
}

extern "C" int ps_sim_record_ancestry(ps_sim *s, uint32_t capacity)
{
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    const uint64_t N = s->prm.pop_size;
    // capacity x N x 4 bytes in u64 arithmetic
    if (capacity && N && (uint64_t)capacity > (UINT64_MAX / 4) / N)
        return ps_fail(PS_ERR_INVALID, "a record of %u generations of %llu individuals exceeds the limit of capacity x pop_size x 4 < 2^64 bytes", capacity,
                       (unsigned long long)N);
    PSCHK(use_device(s->core));
    HIPCHK(hipStreamSynchronize(s->acc->stream));       // (the copies into the log that is about to go)
    HIPCHK(hipStreamSynchronize(s->core->stream));
    if (s->d_anc) HIPCHK(hipFree(s->d_anc));
    s->d_anc = nullptr;
    s->anc_capacity = 0;
    s->anc_written = 0;
    if (!capacity) return PS_OK;
    const uint64_t bytes = (uint64_t)capacity * N * sizeof(uint32_t);
    readout_slot log;       // (only the holder of the allocation, which s->d_anc keeps)
    uint8_t *base = nullptr;
    PSCHK(scratch_get(log, bytes, &base, "cannot allocate the %llu bytes of a record of %u generations of %llu individuals", capacity,
                      (unsigned long long)N));
    s->d_anc = (uint32_t *)base;
    s->anc_capacity = capacity;
    return PS_OK;
}

extern "C" int ps_multi_record_ancestry(ps_multi *m, uint32_t capacity)
{
    PSCHK(ps_needs_device());
    if (!m) return ps_fail(PS_ERR_INVALID, "null argument");
    // every shard draws the same parents: shard 0 records alone
    return ps_sim_record_ancestry(m->shard[0], capacity);
}

static int gen_recording(const ps_sim *s, const char *call, bool need_depth)
{
    if (!s->anc_capacity)
        return ps_fail(PS_ERR_STATE, "%s: this run records no ancestry: switch it on with ps_sim_record_ancestry before the generations", call);
    if (need_depth && s->anc_written == 0)
        return ps_fail(PS_ERR_STATE, "%s: no generation has been recorded since ps_sim_record_ancestry or the last reset of the record", call);
    return PS_OK;
}

// the table over the comb in the scratch of the core handle, `extra` bytes behind it: levels x N u32, level 0 = coal
static int gen_scratch_get(ps_population *c0, uint64_t N, uint32_t levels, uint64_t extra, uint32_t **table, void **tail)
{
    scratch_layout lay;
    const uint64_t o_tab = lay.add((uint64_t)levels * N * 4, 16), o_tail = lay.add(extra, 1);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(c0->ro[PS_RO_GEN], lay.bytes, &base, "cannot allocate the %llu bytes of the genealogy of %llu individuals", (unsigned long long)N));
    *table = (uint32_t *)(base + o_tab);
    if (tail) *tail = base + o_tail;
    return PS_OK;
}

// the comb of s's record into level 0 of `table`, on stream st of s's device (behind every copy into the log: the caller has
// synchronised the accessory stream or ordered st behind it)
static int gen_comb_launch(const ps_sim *s, uint32_t *table, hipStream_t st)
{
    const uint32_t N = (uint32_t)s->prm.pop_size;
    if (N < 2) return PS_OK;
    const uint32_t depth = (uint32_t)std::min<uint64_t>(s->anc_written, s->anc_capacity);
    ancestry_comb_kernel<<<(N - 1 + 255) / 256, 256, 0, st>>>(s->d_anc, N, s->anc_capacity, (uint32_t)(s->anc_written % s->anc_capacity), depth, table);
    HIPCHK(hipGetLastError());
    return PS_OK;
}

static int gen_device(ps_sim *s, ps_genealogy_t *out, uint32_t *order, uint32_t *coal)
{
    ps_population *c0 = s->core;
    const uint64_t N = s->prm.pop_size;
    if (N < 1 || N > 0xffffffffull) return ps_fail(PS_ERR_INVALID, "a genealogy needs 1 <= pop_size < 2^32");
    PSCHK(use_device(c0));
    const uint32_t *slot = nullptr;
    PSCHK(rows_current(c0, &slot));
    HIPCHK(hipStreamSynchronize(s->acc->stream));
    HIPCHK(hipStreamSynchronize(c0->stream));
    uint32_t *table = nullptr;
    PSCHK(gen_scratch_get(c0, N, 1, 0, &table, nullptr));
    PSCHK(gen_comb_launch(s, table, c0->stream));
    if (N > 1) HIPCHK(hipMemcpyAsync(coal, table, (N - 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, c0->stream));
    HIPCHK(hipStreamSynchronize(c0->stream));
    for (uint64_t k = 0; k < N; k++) order[slot ? slot[k] : k] = (uint32_t)k;
    memset(out, 0, sizeof *out);
    out->pop_size = N;
    out->generation = s->gens_done;
    out->capacity = s->anc_capacity;
    out->depth = std::min<uint64_t>(s->anc_written, s->anc_capacity);
    gen_finish(out, coal);
    return PS_OK;
}

extern "C" int ps_sim_genealogy(ps_sim *s, ps_genealogy_t *out, uint32_t *order, uint32_t *coal)
{
    PSCHK(ps_needs_device());
    if (!s || !out || !order || !coal) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(gen_recording(s, "ps_sim_genealogy", false));
    return gen_device(s, out, order, coal);
}

extern "C" int ps_multi_genealogy(ps_multi *m, ps_genealogy_t *out, uint32_t *order, uint32_t *coal)
{
    PSCHK(ps_needs_device());
    if (!m || !out || !order || !coal) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(gen_recording(m->shard[0], "ps_multi_genealogy", false));
    PSCHK(ps_multi_sync(m));
    return gen_device(m->shard[0], out, order, coal);
}
