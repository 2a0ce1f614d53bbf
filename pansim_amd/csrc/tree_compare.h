// tree_compare.h -- ps_tree_compare / ps_sim_tree_compare / ps_multi_tree_compare, the host restatement
// ps_tree_compare_from_merges, ps_levels_from_heights and ps_tree_compare_timing (include/pansim_hip.h; the definitions:
// docs/TREE_COMPARISON.md).  Included by pansim_capi.hip behind tree_parsimony.h, whose check of a merge list it shares.
//
// Both trees are merge lists over the reference's row order, and no matrix is read: a handle only supplies the device, the
// stream and the scratch.  On the host each tree is laid out in its own dendrogram order (tcmp_make_comb), which turns "the
// lowest common ancestor of two leaves" into a range maximum; the clades are compared there as well (tcmp_clades).  On the
// device: the two sparse tables, with triplets the rank table, then one pass of tree_pair_kernel over all pairs.
#pragma once

#include "tree_compare_kernels.h"

#define PS_TCMP_MAX_BINS 16384u         // 64 KB of u32 bins in LDS per workgroup
#define PS_TCMP_MAX_AXIS 1024u          // bins per tree

// one tree in its own dendrogram order: pos[leaf], order[pos], gap[r] (N - 1: the merge between positions r and r + 1 or
// PS_GEN_BEYOND), info[k] = { val, lo | hi << 16 } with [lo, hi) the positions of the merge's tie-top, top[k] that tie-top's
// merge index (top[k] == k: merge k is a clade), span = the largest val
struct tcmp_comb {
    pars_tree t;
    std::vector<uint32_t> pos, order, gap, top;
    std::vector<uint2> info;
    uint64_t span = 0, clades = 0;
};

static int tcmp_check_params(const ps_tree_compare_params *prm)
{
    if (prm->bins_a < 1 || prm->bins_b < 1) return ps_fail(PS_ERR_INVALID, "bins_a and bins_b must be >= 1");
    if (prm->bins_a > PS_TCMP_MAX_AXIS || prm->bins_b > PS_TCMP_MAX_AXIS)
        return ps_fail(PS_ERR_INVALID, "bins_a = %u, bins_b = %u exceed the limit of %u bins per tree", prm->bins_a, prm->bins_b, PS_TCMP_MAX_AXIS);
    if (((uint64_t)prm->bins_a + 1) * ((uint64_t)prm->bins_b + 1) > PS_TCMP_MAX_BINS)
        return ps_fail(PS_ERR_INVALID, "(bins_a + 1) x (bins_b + 1) = %llu exceeds the limit of %u bins (64 KB of LDS per workgroup)",
                       ((unsigned long long)prm->bins_a + 1) * ((unsigned long long)prm->bins_b + 1), PS_TCMP_MAX_BINS);
    if (prm->span_a > 0xffffffffull || prm->span_b > 0xffffffffull)
        return ps_fail(PS_ERR_INVALID, "span_a = %llu, span_b = %llu exceed the limit of 2^32 - 1", (unsigned long long)prm->span_a,
                       (unsigned long long)prm->span_b);
    return PS_OK;
}

// The merge list checked (pars_check_tree), its values checked, and the comb.  `which`: "a" or "b", for the messages.
static int tcmp_make_comb(const char *which, const uint32_t *left, const uint32_t *right, const uint32_t *val, uint64_t merges, uint64_t pop_size,
                          tcmp_comb *c)
{
    PSCHK(pars_check_tree(left, right, merges, pop_size, &c->t));
    const uint32_t N = c->t.N, M = c->t.M;
    const std::vector<int32_t> &parent = c->t.parent;
    c->info.assign(M, make_uint2(0u, 0u));
    c->span = 0;
    for (uint32_t k = 0; k < M; k++) {
        const uint32_t v = val ? val[k] : k + 1u;
        if (v < 1 || v > PS_TC_MAX_VAL)
            return ps_fail(PS_ERR_INVALID, "tree %s: the value %u of merge %u is outside 1 .. %u (2^18 - 1)", which, v, k, PS_TC_MAX_VAL);
        c->info[k].x = v;
        c->span = std::max<uint64_t>(c->span, v);
        for (uint32_t x : { left[k], right[k] })
            if (x >= N && c->info[x - N].x > v)
                return ps_fail(PS_ERR_INVALID, "tree %s: merge %u has the value %u below the %u of its child merge %u: values must not "
                                               "descend towards the root (1 .. %u)", which, k, v, c->info[x - N].x, x - N, PS_TC_MAX_VAL);
    }
    // the leaf order: depth first, left then right, the roots in ascending node id; an explicit stack (a caterpillar is as deep
    // as the population).  lo[k] / hi[k]: the positions of merge k's own leaves.
    c->pos.assign(N, 0u);
    c->order.assign(N, 0u);
    c->gap.assign(N > 1 ? N - 1 : 0, PS_GEN_BEYOND);
    std::vector<uint32_t> lo(M), hi(M), stack;
    uint32_t next = 0;
    for (uint32_t root = 0; root < N + M; root++) {
        if (parent[root] >= 0) continue;
        stack.push_back(root);
        while (!stack.empty()) {
            const uint32_t x = stack.back();
            stack.pop_back();
            if (x < N) {
                c->pos[x] = next;
                c->order[next++] = x;
                continue;
            }
            stack.push_back(right[x - N]);
            stack.push_back(left[x - N]);
        }
    }
    // (children precede their parents in the list: one ascending pass gives every merge its interval)
    auto first = [&](uint32_t x) { return x < N ? c->pos[x] : lo[x - N]; };
    auto end = [&](uint32_t x) { return x < N ? c->pos[x] + 1u : hi[x - N]; };
    for (uint32_t k = 0; k < M; k++) {
        lo[k] = first(left[k]);
        hi[k] = end(right[k]);
        c->gap[end(left[k]) - 1u] = k;
    }
    // tie-tops from the roots down: a merge whose parent carries the same value belongs to its parent's clade
    c->top.assign(M, 0u);
    c->clades = 0;
    for (uint32_t k = M; k-- > 0;) {
        const int32_t up = parent[N + k];
        const bool tied = up >= 0 && c->info[(uint32_t)up - N].x == c->info[k].x;
        c->top[k] = tied ? c->top[(uint32_t)up - N] : k;
        c->clades += tied ? 0 : 1;
        c->info[k].y = lo[c->top[k]] | (hi[c->top[k]] << 16);      // (hi <= 16384)
    }
    return PS_OK;
}

// in_b[k] (may be null) = 1 iff merge k of `a` is a clade whose leaf set is a clade of `b`; returns how many are.  The leaf
// set of a clade of `a` is an interval of a's order; it is a clade of `b` iff its positions in b are one interval (max - min
// + 1 = its size, from the children's extremes bottom up) and that interval is a tie-top's.
static uint64_t tcmp_shared(const tcmp_comb &a, const tcmp_comb &b, const uint32_t *left, const uint32_t *right, uint8_t *in_b)
{
    const uint32_t N = a.t.N, MA = a.t.M, MB = b.t.M;
    std::vector<uint64_t> clade_of_b;           // lo (N + 1) + hi of b's clades, sorted
    for (uint32_t k = 0; k < MB; k++)
        if (b.top[k] == k) clade_of_b.push_back((uint64_t)(b.info[k].y & 0xffffu) * (N + 1u) + (b.info[k].y >> 16));
    std::sort(clade_of_b.begin(), clade_of_b.end());
    std::vector<uint32_t> mn(MA), mx(MA);
    uint64_t shared = 0;
    for (uint32_t k = 0; k < MA; k++) {
        const uint32_t l = left[k], r = right[k];
        mn[k] = std::min(l < N ? b.pos[l] : mn[l - N], r < N ? b.pos[r] : mn[r - N]);
        mx[k] = std::max(l < N ? b.pos[l] : mx[l - N], r < N ? b.pos[r] : mx[r - N]);
        const uint32_t size = (a.info[k].y >> 16) - (a.info[k].y & 0xffffu);
        const bool hit = a.top[k] == k && mx[k] - mn[k] + 1u == size &&
                         std::binary_search(clade_of_b.begin(), clade_of_b.end(), (uint64_t)mn[k] * (N + 1u) + mx[k] + 1u);
        if (in_b) in_b[k] = hit ? 1 : 0;
        shared += hit ? 1 : 0;
    }
    return shared;
}

static ps_tc_args tcmp_args(const ps_tree_compare_params *prm, const tcmp_comb &a, const tcmp_comb &b)
{
    ps_tc_args x;
    x.Ba = prm->bins_a;
    x.Bb = prm->bins_b;
    x.Sa = prm->span_a ? prm->span_a : a.span;
    x.Sb = prm->span_b ? prm->span_b : b.span;
    x.a_scale = (float)((double)x.Ba / (double)x.Sa);
    x.b_scale = (float)((double)x.Bb / (double)x.Sb);
    return x;
}

static double tcmp_ratio(uint64_t num, uint64_t den) { return den ? (double)num / (double)den : 0.0; }

// everything of `out` that follows from the words (PS_TC_*), the combs and the clades
static void tcmp_finish(ps_tree_compare_t *o, const tcmp_comb &a, const tcmp_comb &b, const ps_tc_args &x, bool triplets, const uint64_t *w,
                        uint64_t shared_clades)
{
    memset(o, 0, sizeof *o);
    const uint64_t N = a.t.N;
    o->pop_size = N;
    o->merges_a = a.t.M;
    o->merges_b = b.t.M;
    o->pairs = N * (N - 1) / 2;
    o->joined_both = w[PS_TC_BOTH];
    o->joined_a_only = w[PS_TC_A_ONLY];
    o->joined_b_only = w[PS_TC_B_ONLY];
    o->joined_neither = w[PS_TC_NEITHER];
    o->sum_a = w[PS_TC_SUM_A];
    o->sum_b = w[PS_TC_SUM_B];
    o->sum_aa = w[PS_TC_SUM_AA];
    o->sum_bb = w[PS_TC_SUM_BB];
    o->sum_ab = w[PS_TC_SUM_AB];
    if (triplets) {
        o->triples = N * (N - 1) / 2 * (N - 2) / 3;
        o->resolved_a = w[PS_TC_RES_A];
        o->resolved_b = w[PS_TC_RES_B];
        o->shared_triplets = w[PS_TC_SHARED];
    }
    o->clades_a = a.clades;
    o->clades_b = b.clades;
    o->shared_clades = shared_clades;
    o->rf_distance = a.clades + b.clades - 2 * shared_clades;
    o->bins_a = x.Ba;
    o->bins_b = x.Bb;
    o->span_a = x.Sa;
    o->span_b = x.Sb;
    // the three integer terms exact in 128 bits (n < 2^27, the sums of squares < 2^63), then one conversion each
    const __int128 n = (__int128)o->joined_both, sa = (__int128)o->sum_a, sb = (__int128)o->sum_b;
    const __int128 cov = n * (__int128)o->sum_ab - sa * sb, va = n * (__int128)o->sum_aa - sa * sa, vb = n * (__int128)o->sum_bb - sb * sb;
    o->cophenetic_r = (o->joined_both && va != 0 && vb != 0) ? (double)cov / sqrt((double)va * (double)vb) : 0.0;
    o->triplet_recall = tcmp_ratio(o->shared_triplets, o->resolved_a);
    o->triplet_precision = tcmp_ratio(o->shared_triplets, o->resolved_b);
    o->clade_recall = tcmp_ratio(shared_clades, a.clades);
    o->clade_precision = tcmp_ratio(shared_clades, b.clades);
}

// the host part of every entry: parameters, both combs, the clades
struct tcmp_host {
    tcmp_comb a, b;
    ps_tc_args x;
    uint64_t shared_clades = 0;
    std::vector<uint32_t> pb;       // pb[p] = the position in b of the leaf at position p of a, padded with 0 to whole chunks
};

static int tcmp_prepare(uint64_t pop_size, const uint32_t *left_a, const uint32_t *right_a, const uint32_t *val_a, uint64_t merges_a,
                        const uint32_t *left_b, const uint32_t *right_b, const uint32_t *val_b, uint64_t merges_b,
                        const ps_tree_compare_params *prm, uint8_t *in_b, uint8_t *in_a, tcmp_host *h)
{
    PSCHK(tcmp_check_params(prm));
    PSCHK(tcmp_make_comb("a", left_a, right_a, val_a, merges_a, pop_size, &h->a));
    PSCHK(tcmp_make_comb("b", left_b, right_b, val_b, merges_b, pop_size, &h->b));
    h->x = tcmp_args(prm, h->a, h->b);
    h->shared_clades = tcmp_shared(h->a, h->b, left_a, right_a, in_b);
    (void)tcmp_shared(h->b, h->a, left_b, right_b, in_a);
    const uint32_t N = h->a.t.N;
    h->pb.assign(((size_t)N + 255u) & ~(size_t)255u, 0u);
    for (uint32_t p = 0; p < N; p++) h->pb[p] = h->b.pos[h->a.order[p]];
    return PS_OK;
}

extern "C" int ps_tree_compare_from_merges(uint64_t pop_size, const uint32_t *left_a, const uint32_t *right_a, const uint32_t *val_a,
                                           uint64_t merges_a, const uint32_t *left_b, const uint32_t *right_b, const uint32_t *val_b,
                                           uint64_t merges_b, const ps_tree_compare_params *prm, ps_tree_compare_t *out, uint64_t *joint,
                                           uint8_t *in_b, uint8_t *in_a)
{
    if (!prm || !out || !joint) return ps_fail(PS_ERR_INVALID, "null argument");
    tcmp_host h;
    PSCHK(tcmp_prepare(pop_size, left_a, right_a, val_a, merges_a, left_b, right_b, val_b, merges_b, prm, in_b, in_a, &h));
    const uint32_t N = h.a.t.N;
    const bool triplets = prm->triplets != 0;
    const gen_host_table ta(h.a.gap.data(), N), tb(h.b.gap.data(), N);
    // the rank table as the device builds it, row by row
    const size_t pitch = (size_t)N + 1;
    std::vector<uint16_t> R;
    if (triplets) {
        try {
            R.assign(pitch * pitch, 0);
        } catch (const std::bad_alloc &) {
            return ps_fail(PS_ERR_OOM, "cannot allocate the %llu bytes of the rank table of %u leaves", (unsigned long long)(pitch * pitch * 2), N);
        }
        for (size_t x = 1; x <= N; x++)
            for (size_t y = 0; y <= N; y++) R[x * pitch + y] = (uint16_t)(R[(x - 1) * pitch + y] + (h.pb[x - 1] < y ? 1 : 0));
    }
    const uint64_t nb = (uint64_t)h.x.Bb + 1, nbins = ((uint64_t)h.x.Ba + 1) * nb;
    memset(joint, 0, nbins * sizeof(uint64_t));
    ps_tc_sums t = {};
    for (uint32_t p = 0; p + 1 < N; p++)
        for (uint32_t q = p + 1; q < N; q++) {
            const uint32_t bp = h.pb[p], bq = h.pb[q];
            const uint32_t ma = ta.tmrca(p, q), mb = tb.tmrca(std::min(bp, bq), std::max(bp, bq));
            const bool ja = ma != PS_GEN_BEYOND, jb = mb != PS_GEN_BEYOND;
            const uint2 ia = ja ? h.a.info[ma] : make_uint2(0u, 0u), ib = jb ? h.b.info[mb] : make_uint2(0u, 0u);
            uint32_t rab = 0;
            if (triplets && ja && jb) {
                const size_t x0 = ia.y & 0xffffu, x1 = ia.y >> 16, y0 = ib.y & 0xffffu, y1 = ib.y >> 16;
                rab = ((uint32_t)R[x1 * pitch + y1] + R[x0 * pitch + y0]) - ((uint32_t)R[x0 * pitch + y1] + R[x1 * pitch + y0]);
            }
            ps_tc_pair(t, ja, jb, ia, ib, N, triplets, rab);
            const uint32_t ba = ja ? ps_clock_time_bin(ia.x, h.x.Ba, h.x.Sa, h.x.a_scale) : h.x.Ba;
            const uint32_t bb = jb ? ps_clock_time_bin(ib.x, h.x.Bb, h.x.Sb, h.x.b_scale) : h.x.Bb;
            joint[(uint64_t)ba * nb + bb]++;
        }
    uint64_t w[PS_TC_WORDS];
    for (int k = 0; k < PS_TC_WORDS; k++) w[k] = k < 4 ? t.n[k] : t.s[k - 4];
    tcmp_finish(out, h.a, h.b, h.x, triplets, w, h.shared_clades);
    return PS_OK;
}

extern "C" int ps_levels_from_heights(const uint64_t *num, const uint64_t *den, uint64_t merges, uint32_t *levels, uint64_t *distinct)
{
    if (merges && (!num || !den || !levels)) return ps_fail(PS_ERR_INVALID, "null argument");
    // the linkage tree's comparison, in 128 bits: a height with den == 0 is undefined, above every defined one and equal to
    // every other undefined one
    auto cmp = [&](uint64_t a, uint64_t b) -> int {
        if (den[a] == 0 || den[b] == 0) return den[a] == den[b] ? 0 : den[a] == 0 ? 1 : -1;
        const unsigned __int128 x = (unsigned __int128)num[a] * den[b], y = (unsigned __int128)num[b] * den[a];
        return x < y ? -1 : x > y ? 1 : 0;
    };
    uint64_t level = 0;
    for (uint64_t k = 0; k < merges; k++) {
        const int c = k ? cmp(k - 1, k) : -1;
        if (c > 0)
            return ps_fail(PS_ERR_INVALID, "height %llu (%llu / %llu) lies below height %llu (%llu / %llu): the heights must not decrease",
                           (unsigned long long)k, (unsigned long long)num[k], (unsigned long long)den[k], (unsigned long long)(k - 1),
                           (unsigned long long)num[k - 1], (unsigned long long)den[k - 1]);
        level += c < 0 ? 1 : 0;
        if (level > 0xffffffffull) return ps_fail(PS_ERR_INVALID, "more than 2^32 - 1 distinct heights");
        levels[k] = (uint32_t)level;
    }
    if (distinct) *distinct = level;
    return PS_OK;
}

// The call behind the three device entries on handle p: nothing of p but its device, stream, scratch slot and pop_size is used.
static int tcmp_device(ps_population *p, const uint32_t *left_a, const uint32_t *right_a, const uint32_t *val_a, uint64_t merges_a,
                       const uint32_t *left_b, const uint32_t *right_b, const uint32_t *val_b, uint64_t merges_b,
                       const ps_tree_compare_params *prm, ps_tree_compare_t *out, uint64_t *joint, uint8_t *in_b, uint8_t *in_a)
{
    tcmp_host h;
    PSCHK(tcmp_prepare(p->cfg.pop_size, left_a, right_a, val_a, merges_a, left_b, right_b, val_b, merges_b, prm, in_b, in_a, &h));
    const uint32_t N = h.a.t.N, MA = h.a.t.M, MB = h.b.t.M;
    const bool triplets = prm->triplets != 0;
    const uint32_t levels = gen_levels(N);
    const uint64_t nbins = ((uint64_t)h.x.Ba + 1) * ((uint64_t)h.x.Bb + 1), n_words = PS_TC_WORDS + nbins;
    const uint32_t pitch = (N + 1u + 63u) & ~63u;        // (u16 entries: rows of whole 128-byte lines)
    PSCHK(use_device(p));
    scratch_layout lay;
    const uint64_t o_words = lay.add(n_words * 8, 16);
    const uint64_t o_ta = lay.add((uint64_t)levels * N * 4, 16), o_tb = lay.add((uint64_t)levels * N * 4, 16);
    const uint64_t o_pb = lay.add((uint64_t)h.pb.size() * 4, 16);
    const uint64_t o_ia = lay.add((uint64_t)MA * 8, 16), o_ib = lay.add((uint64_t)MB * 8, 16);
    const uint64_t o_rank = lay.add(triplets ? (uint64_t)(N + 1u) * pitch * 2 : 0, 128);
    uint8_t *base = nullptr;
    readout_slot &ro = p->ro[PS_RO_TCMP];
    PSCHK(scratch_get(ro, lay.bytes, &base, "cannot allocate the %llu bytes of the tables of two trees of %u leaves%s", N,
                      triplets ? " and their rank table" : ""));
    ro.timed = false;
    hipStream_t st = p->stream;
    unsigned long long *d_words = (unsigned long long *)(base + o_words), *d_joint = d_words + PS_TC_WORDS;
    uint32_t *d_ta = (uint32_t *)(base + o_ta), *d_tb = (uint32_t *)(base + o_tb), *d_pb = (uint32_t *)(base + o_pb);
    uint2 *d_ia = (uint2 *)(base + o_ia), *d_ib = (uint2 *)(base + o_ib);
    uint16_t *d_rank = triplets ? (uint16_t *)(base + o_rank) : nullptr;
    event_timer tm;
    // timer groups: 0 = the uploads and the tables, 1 = the pairs
    PSCHK(tm.timed(0, st, [&]() -> int {
        HIPCHK(hipMemsetAsync(d_words, 0, n_words * 8, st));
        HIPCHK(hipMemcpyAsync(d_ta, h.a.gap.data(), (uint64_t)(N - 1) * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_tb, h.b.gap.data(), (uint64_t)(N - 1) * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_pb, h.pb.data(), (uint64_t)h.pb.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_ia, h.a.info.data(), (uint64_t)MA * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_ib, h.b.info.data(), (uint64_t)MB * 8, hipMemcpyHostToDevice, st));
        for (uint32_t *tab : { d_ta, d_tb })
            for (uint32_t k = 1; k < levels; k++)
                ancestry_table_kernel<<<(N - 1 + 255) / 256, 256, 0, st>>>(tab + (uint64_t)(k - 1) * N, tab + (uint64_t)k * N, N - 1, 1u << (k - 1));
        if (triplets) {
            const uint32_t g = (N + 1u + 255u) / 256u;
            tree_rank_kernel<<<dim3(g, (N + PS_TC_RANK_ROWS) / PS_TC_RANK_ROWS), 256, 0, st>>>(d_pb, N, pitch, d_rank);
        }
        HIPCHK(hipGetLastError());
        return PS_OK;
    }));
    PSCHK(tm.timed(1, st, [&]() -> int {
        auto kern = triplets ? tree_pair_kernel<true> : tree_pair_kernel<false>;
        const uint32_t lds = (uint32_t)nbins * 4u;
        dim3 grid;
        PSCHK(bin_grid((const void *)kern, N, N - 1, lds, 256u, &grid));
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, (const uint32_t *)d_ta, (const uint32_t *)d_tb, (const uint32_t *)d_pb,
                           (const uint2 *)d_ia, (const uint2 *)d_ib, (const uint16_t *)d_rank, pitch, N, h.x, d_words, d_joint);
        HIPCHK(hipGetLastError());
        return PS_OK;
    }));
    unsigned long long w[PS_TC_WORDS];
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the bins are copied as they are");
    HIPCHK(hipMemcpyAsync(w, d_words, sizeof w, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(joint, d_joint, nbins * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    PSCHK(tm.collect(ro, 2));
    uint64_t words[PS_TC_WORDS];
    for (int k = 0; k < PS_TC_WORDS; k++) words[k] = w[k];
    tcmp_finish(out, h.a, h.b, h.x, triplets, words, h.shared_clades);
    return PS_OK;
}

#define PS_TCMP_TREES left_a, right_a, val_a, merges_a, left_b, right_b, val_b, merges_b, prm, out, joint, in_b, in_a

extern "C" int ps_tree_compare(ps_population *any, const uint32_t *left_a, const uint32_t *right_a, const uint32_t *val_a, uint64_t merges_a,
                               const uint32_t *left_b, const uint32_t *right_b, const uint32_t *val_b, uint64_t merges_b,
                               const ps_tree_compare_params *prm, ps_tree_compare_t *out, uint64_t *joint, uint8_t *in_b, uint8_t *in_a)
{
    PSCHK(ps_needs_device());
    if (!any || !prm || !out || !joint) return ps_fail(PS_ERR_INVALID, "null argument");
    return tcmp_device(any, PS_TCMP_TREES);
}

extern "C" int ps_sim_tree_compare(ps_sim *s, const uint32_t *left_a, const uint32_t *right_a, const uint32_t *val_a, uint64_t merges_a,
                                   const uint32_t *left_b, const uint32_t *right_b, const uint32_t *val_b, uint64_t merges_b,
                                   const ps_tree_compare_params *prm, ps_tree_compare_t *out, uint64_t *joint, uint8_t *in_b, uint8_t *in_a)
{
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    return ps_tree_compare(s->core, PS_TCMP_TREES);
}

extern "C" int ps_multi_tree_compare(ps_multi *m, const uint32_t *left_a, const uint32_t *right_a, const uint32_t *val_a, uint64_t merges_a,
                                     const uint32_t *left_b, const uint32_t *right_b, const uint32_t *val_b, uint64_t merges_b,
                                     const ps_tree_compare_params *prm, ps_tree_compare_t *out, uint64_t *joint, uint8_t *in_b, uint8_t *in_a)
{
    PSCHK(ps_needs_device());
    if (!m) return ps_fail(PS_ERR_INVALID, "null argument");
    return ps_sim_tree_compare(m->shard[0], PS_TCMP_TREES);
}

#undef PS_TCMP_TREES

extern "C" int ps_tree_compare_timing(ps_population *any, double *tables_ms, double *pairs_ms)
{
    if (!any) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(any->ro[PS_RO_TCMP], "no tree comparison has been computed on this handle", { tables_ms, pairs_ms });
}
