// tree_parsimony.h -- ps_tree_parsimony / ps_sim_tree_parsimony / ps_multi_tree_parsimony, the host rules ps_merges_from_tree,
// ps_merges_from_genealogy and ps_parsimony_schedule, and the host restatement ps_parsimony_from_rows (include/pansim_hip.h;
// the definitions: docs/TREE_PARSIMONY.md).  Included by pansim_capi.hip behind group_differentiation.h.
//
// The tree arrives as a merge list over the reference's row order, the matrices are in internal order: the schedule of a
// handle (pars_make_schedule) names a leaf by the internal row its output row lives at (rows_current), an internal node by its
// position in (level, merge) order.  One pass over the core matrix on the core stream; the genes are expanded from the
// gene-major view to bytes in chunks and run through the same kernel on the accessory stream.  Branch counters come back per
// LDS slot and are mapped to node ids on the host.
#pragma once

#include "parsimony_kernels.h"

// a checked merge list: parent of every node (-1: a root), the level of every merge
struct pars_tree {
    uint32_t N = 0, M = 0, levels = 0;
    std::vector<int32_t> parent;
    std::vector<uint32_t> level_of;
    uint64_t trees = 0, covered = 0;
};

static int pars_check_tree(const uint32_t *left, const uint32_t *right, uint64_t merges, uint64_t pop_size, pars_tree *t)
{
    if (pop_size < 2 || pop_size > PS_PARS_MAX_POP)
        return ps_fail(PS_ERR_INVALID, "a tree for the parsimony needs 2 <= pop_size <= %u, not %llu", PS_PARS_MAX_POP, (unsigned long long)pop_size);
    if (merges < 1 || merges > pop_size - 1)
        return ps_fail(PS_ERR_INVALID, "a tree of %llu leaves has 1 .. %llu merges, not %llu", (unsigned long long)pop_size,
                       (unsigned long long)(pop_size - 1), (unsigned long long)merges);
    if (!left || !right) return ps_fail(PS_ERR_INVALID, "null argument");
    const uint32_t N = (uint32_t)pop_size, M = (uint32_t)merges;
    t->N = N;
    t->M = M;
    t->parent.assign((size_t)N + M, -1);
    t->level_of.assign(M, 0u);
    t->levels = 0;
    for (uint32_t k = 0; k < M; k++) {
        const uint32_t c[2] = { left[k], right[k] };
        if (c[0] == c[1]) return ps_fail(PS_ERR_INVALID, "merge %u joins node %u with itself", k, c[0]);
        uint32_t lev = 0;
        for (uint32_t x : c) {
            if (x >= N + k) return ps_fail(PS_ERR_INVALID, "merge %u has the child %u: not a node below %u", k, x, N + k);
            if (t->parent[x] >= 0) return ps_fail(PS_ERR_INVALID, "node %u is a child of merge %u and of merge %u", x, (uint32_t)t->parent[x] - N, k);
            t->parent[x] = (int32_t)(N + k);
            if (x >= N) lev = std::max(lev, t->level_of[x - N]);
        }
        t->level_of[k] = lev + 1u;
        t->levels = std::max(t->levels, lev + 1u);
    }
    t->trees = t->covered = 0;
    for (uint32_t x = 0; x < N + M; x++) {
        if (x < N && t->parent[x] >= 0) t->covered++;
        if (x >= N && t->parent[x] < 0) t->trees++;
    }
    return PS_OK;
}

extern "C" int ps_parsimony_schedule(const uint32_t *left, const uint32_t *right, uint64_t merges, uint64_t pop_size, uint32_t *level_of,
                                     uint32_t *levels)
{
    if (!level_of || !levels) return ps_fail(PS_ERR_INVALID, "null argument");
    pars_tree t;
    PSCHK(pars_check_tree(left, right, merges, pop_size, &t));
    memcpy(level_of, t.level_of.data(), (size_t)t.M * sizeof(uint32_t));
    *levels = t.levels;
    return PS_OK;
}

extern "C" int ps_merges_from_tree(const uint32_t *lo, const uint32_t *hi, uint64_t edges, uint64_t pop_size, uint32_t *left, uint32_t *right,
                                   uint64_t *merges)
{
    if (!merges || (edges && (!lo || !hi || !left || !right))) return ps_fail(PS_ERR_INVALID, "null argument");
    if (pop_size < 1 || pop_size > 0x7fffffffull) return ps_fail(PS_ERR_INVALID, "pop_size must be 1 .. 2^31 - 1");
    if (edges > pop_size - 1)
        return ps_fail(PS_ERR_INVALID, "%llu edges are more than a tree of %llu rows has", (unsigned long long)edges, (unsigned long long)pop_size);
    const uint32_t N = (uint32_t)pop_size;
    // union-find over the rows; per root: the node that stands for its cluster and the cluster's smallest row
    std::vector<uint32_t> up(N), node(N), low(N);
    for (uint32_t i = 0; i < N; i++) up[i] = node[i] = low[i] = i;
    auto root = [&](uint32_t x) {
        while (up[x] != x) x = up[x] = up[up[x]];
        return x;
    };
    for (uint64_t k = 0; k < edges; k++) {
        if (lo[k] >= N || hi[k] >= N) return ps_fail(PS_ERR_INVALID, "edge %llu names a row that is not below %u", (unsigned long long)k, N);
        uint32_t a = root(lo[k]), b = root(hi[k]);
        if (a == b)
            return ps_fail(PS_ERR_INVALID, "edge %llu (%u, %u) lies inside one cluster: the edges are not a forest", (unsigned long long)k, lo[k], hi[k]);
        if (low[b] < low[a]) std::swap(a, b);
        left[k] = node[a];
        right[k] = node[b];
        up[b] = a;
        node[a] = N + (uint32_t)k;
    }
    *merges = edges;
    return PS_OK;
}

extern "C" int ps_merges_from_genealogy(const uint32_t *order, const uint32_t *coal, uint64_t pop_size, uint32_t *left, uint32_t *right,
                                        uint32_t *height, uint64_t *merges)
{
    if (!order || !merges || (pop_size > 1 && (!coal || !left || !right))) return ps_fail(PS_ERR_INVALID, "null argument");
    if (pop_size < 1 || pop_size > 0x7fffffffull) return ps_fail(PS_ERR_INVALID, "pop_size must be 1 .. 2^31 - 1");
    const uint32_t N = (uint32_t)pop_size;
    std::vector<uint8_t> seen(N, 0);
    for (uint32_t r = 0; r < N; r++) {
        if (order[r] >= N || seen[order[r]]) return ps_fail(PS_ERR_INVALID, "order is not a permutation of 0 .. %u", N - 1);
        seen[order[r]] = 1;
    }
    std::vector<uint32_t> pos;
    for (uint32_t r = 0; r + 1 < N; r++)
        if (coal[r] != PS_GEN_BEYOND) pos.push_back(r);
    std::stable_sort(pos.begin(), pos.end(), [&](uint32_t a, uint32_t b) { return coal[a] < coal[b]; });
    // union-find over the internal rows; per root the node of its interval
    std::vector<uint32_t> up(N), node(N);
    for (uint32_t r = 0; r < N; r++) {
        up[r] = r;
        node[r] = order[r];
    }
    auto root = [&](uint32_t x) {
        while (up[x] != x) x = up[x] = up[up[x]];
        return x;
    };
    uint32_t k = 0;
    for (uint32_t r : pos) {
        const uint32_t a = root(r), b = root(r + 1);
        left[k] = node[a];
        right[k] = node[b];
        if (height) height[k] = coal[r];
        up[b] = a;
        node[a] = N + k;
        k++;
    }
    *merges = k;
    return PS_OK;
}

// what a pass over one matrix adds up (the device: the kernel's words)
struct pars_sums {
    uint64_t total = 0, changed = 0, maxc = 0, minc = 0, homo = 0, gains = 0;
    uint64_t hist[PS_PARS_BINS] = {};
    void add(const pars_sums &o)
    {
        total += o.total;
        changed += o.changed;
        maxc = std::max(maxc, o.maxc);
        minc += o.minc;
        homo += o.homo;
        gains += o.gains;
        for (int b = 0; b < PS_PARS_BINS; b++) hist[b] += o.hist[b];
    }
    void site(uint32_t ch, uint32_t classes, uint32_t gn)
    {
        total += ch;
        changed += ch != 0;
        maxc = std::max<uint64_t>(maxc, ch);
        minc += classes - 1;
        homo += ch > classes - 1;
        gains += gn;
        hist[std::min<uint32_t>(ch, PS_PARS_BINS - 1)]++;
    }
};

static void pars_summary(ps_parsimony_t *o, const pars_tree &t, uint64_t sites, const pars_sums &core, uint64_t genes, const pars_sums &gene,
                         bool gene_down)
{
    memset(o, 0, sizeof *o);
    o->pop_size = t.N;
    o->sites = sites;
    o->genes = genes;
    o->merges = t.M;
    o->trees = t.trees;
    o->covered_leaves = t.covered;
    o->spanning = t.M == t.N - 1u ? 1 : 0;
    o->total_changes = core.total;
    o->changed_sites = core.changed;
    o->max_changes = core.maxc;
    o->gene_total_changes = gene.total;
    if (gene_down) {
        o->gene_total_gains = gene.gains;
        o->gene_total_losses = gene.total - gene.gains;
    }
    if (o->spanning) {
        o->min_changes = core.minc;
        o->excess_changes = core.total - core.minc;
        o->homoplasic_sites = core.homo;
        o->ci = core.total ? (double)core.minc / (double)core.total : 0.0;
    }
}

// the optional outputs of a call (null: not asked for)
struct pars_outputs {
    uint32_t *site_changes;
    uint64_t *site_hist, *branch_changes;
    uint32_t *gene_changes, *gene_gains, *gene_losses;
    uint64_t *branch_gains, *branch_losses;
    bool gene_down() const { return gene_gains || gene_losses || branch_gains || branch_losses; }
    bool genes() const { return gene_changes || gene_down(); }
};

extern "C" int ps_parsimony_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, int genes, const uint32_t *left,
                                      const uint32_t *right, uint64_t merges, ps_parsimony_t *out, uint32_t *site_changes, uint64_t *site_hist,
                                      uint64_t *branch_changes, uint32_t *gene_changes, uint32_t *gene_gains, uint32_t *gene_losses,
                                      uint64_t *branch_gains, uint64_t *branch_losses)
{
    if (!out || (!rows && cols)) return ps_fail(PS_ERR_INVALID, "null argument");
    if (genes != 0 && genes != 1) return ps_fail(PS_ERR_INVALID, "genes must be 0 or 1, not %d", genes);
    const pars_outputs o = { site_changes, site_hist, branch_changes, gene_changes, gene_gains, gene_losses, branch_gains, branch_losses };
    if (genes ? (site_changes || site_hist || branch_changes) : o.genes())
        return ps_fail(PS_ERR_INVALID, genes ? "a matrix of genes fills the gene outputs only" : "a matrix of core cells fills the core outputs only");
    pars_tree t;
    PSCHK(pars_check_tree(left, right, merges, pop_size, &t));
    const uint32_t N = t.N, M = t.M;
    const bool down = genes ? o.gene_down() : branch_changes != nullptr;
    std::vector<uint64_t> br((size_t)N + M, 0), br2((size_t)N + M, 0);
    std::vector<uint32_t> S((size_t)N + M);
    pars_sums sums;
    for (uint64_t c0 = 0; c0 < cols; c0 += 4) {
        const uint32_t w = (uint32_t)std::min<uint64_t>(4, cols - c0);
        uint32_t all = 0;
        for (uint32_t i = 0; i < N; i++) {
            uint32_t x = 0;
            for (uint32_t j = 0; j < w; j++) {
                const uint8_t b = rows[(uint64_t)i * cols + c0 + j];
                x |= (uint32_t)(genes ? (b ? 2 : 1) : b) << (8 * j);
            }
            S[i] = ps_pars_classes(x);
            all |= S[i];
        }
        uint32_t ch[4] = { 0, 0, 0, 0 }, gn[4] = { 0, 0, 0, 0 };
        for (uint32_t k = 0; k < M; k++) {
            uint32_t z;
            S[N + k] = ps_pars_join(S[left[k]], S[right[k]], &z);
            for (uint32_t j = 0; j < 4; j++) ch[j] += (z >> (8 * j + 7)) & 1u;
        }
        if (down)
            for (uint32_t k = M; k-- > 0;) {
                const uint32_t v = S[N + k], xv = t.parent[N + k] < 0 ? ps_pars_root(v) : v;
                for (uint32_t c : { left[k], right[k] }) {
                    uint32_t d;
                    S[c] = ps_pars_pick(xv, S[c], &d);
                    const uint32_t g = genes ? ps_pars_gains(S[c], d) : 0u;
                    for (uint32_t j = 0; j < w; j++) {
                        const uint32_t dj = (d >> (8 * j + 7)) & 1u, gj = (g >> (8 * j + 7)) & 1u;
                        gn[j] += gj;
                        br[c] += genes ? gj : dj;
                        br2[c] += dj - gj;
                    }
                }
            }
        for (uint32_t j = 0; j < w; j++) {
            sums.site(ch[j], (uint32_t)__builtin_popcount((all >> (8 * j)) & 0x1Fu), gn[j]);
            if (site_changes) site_changes[c0 + j] = ch[j];
            if (gene_changes) gene_changes[c0 + j] = ch[j];
            if (gene_gains) gene_gains[c0 + j] = gn[j];
            if (gene_losses) gene_losses[c0 + j] = ch[j] - gn[j];
        }
    }
    if (site_hist) memcpy(site_hist, sums.hist, sizeof sums.hist);
    if (branch_changes) memcpy(branch_changes, br.data(), br.size() * sizeof(uint64_t));
    if (branch_gains) memcpy(branch_gains, br.data(), br.size() * sizeof(uint64_t));
    if (branch_losses) memcpy(branch_losses, br2.data(), br2.size() * sizeof(uint64_t));
    const pars_sums none;
    pars_summary(out, t, genes ? 0 : cols, genes ? none : sums, genes ? cols : 0, genes ? sums : none, down);
    return PS_OK;
}

// The schedule of one handle: sched[j] of the merges in (level, merge) order, level_off[levels + 1], and slot_of[node] -- a
// leaf's internal row (`slot`: the handle's row slot, null = the orders coincide), n_pad + j for the node of entry j
struct pars_schedule {
    uint32_t n_pad = 0;
    std::vector<uint32_t> sched, level_off, slot_of;
};

static void pars_make_schedule(const pars_tree &t, const uint32_t *left, const uint32_t *right, const uint32_t *slot, pars_schedule *s)
{
    const uint32_t N = t.N, M = t.M;
    s->n_pad = (N + 15u) & ~15u;
    s->level_off.assign(t.levels + 1u, 0u);
    for (uint32_t k = 0; k < M; k++) s->level_off[t.level_of[k]]++;
    for (uint32_t l = 1; l <= t.levels; l++) s->level_off[l] += s->level_off[l - 1u];
    // (level_off[l] is now the end of level l, numbered from 1: the start of the next)
    std::vector<uint32_t> next(s->level_off.begin(), s->level_off.end() - 1);
    s->slot_of.resize((size_t)N + M);
    for (uint32_t i = 0; i < N; i++) s->slot_of[i] = slot ? slot[i] : i;
    for (uint32_t k = 0; k < M; k++) s->slot_of[N + k] = s->n_pad + next[t.level_of[k] - 1u]++;
    s->sched.resize(M);
    for (uint32_t k = 0; k < M; k++)
        s->sched[s->slot_of[N + k] - s->n_pad] = s->slot_of[left[k]] | (s->slot_of[right[k]] << 16) | (t.parent[N + k] < 0 ? PS_PARS_ROOT : 0u);
}

// The pass over one matrix of handle p on its stream, complete when it returns: the core matrix (all sites, or one site
// shard: its own; timer group 1) or, `genes`, the accessory matrix chunk by chunk (group 2); the schedule's upload is group 0.
// per_col (null: not stored): the changes of every column; per_gain (genes with a down pass only): the gains.  `down`: br
// (and, genes, br2) receive the changing branches per NODE (genes: gains, losses), N + M values each.
static int pars_pass(ps_population *p, bool genes, event_timer &tm, const pars_tree &t, const uint32_t *left, const uint32_t *right, bool down,
                     uint32_t *per_col, uint32_t *per_gain, pars_sums *sums, uint64_t *br, uint64_t *br2)
{
    const uint32_t N = t.N, M = t.M;
    const uint32_t total = genes ? p->d.G : (uint32_t)p->cfg.ncols;
    PSCHK(use_device(p));
    const uint32_t *slot = nullptr;
    PSCHK(rows_current(p, &slot));
    pars_schedule sc;
    pars_make_schedule(t, left, right, slot, &sc);
    const uint32_t slots = sc.n_pad + M;
    const uint32_t pitch = genes ? (N + 127u) & ~127u : p->pitch;
    // genes: whole tiles of four per chunk, at most 32 MiB of bytes
    const uint32_t chunk = genes ? std::min(total, std::max(4u, ((32u << 20) / pitch) & ~3u)) : total;
    const bool gains = genes && down && per_gain;
    scratch_layout lay;
    const uint64_t o_words = lay.add(PS_PARS_WORDS * 8, 16), o_sched = lay.add((uint64_t)M * 4, 16);
    const uint64_t o_off = lay.add((uint64_t)sc.level_off.size() * 4, 16);
    const uint64_t o_col = lay.add(per_col ? (uint64_t)total * 4 : 0, 16), o_gain = lay.add(gains ? (uint64_t)total * 4 : 0, 16);
    const uint64_t o_br = lay.add(down ? (uint64_t)slots * 8 : 0, 16), o_br2 = lay.add(down && genes ? (uint64_t)slots * 8 : 0, 16);
    const uint64_t o_bytes = lay.add(genes ? (uint64_t)chunk * pitch : 0, 128);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(p->ro[PS_RO_PARS], lay.bytes, &base, "cannot allocate the %llu bytes of the schedule and the counters of a tree of %u merges over %u columns",
                      M, total));
    hipStream_t st = p->stream;
    unsigned long long *d_words = (unsigned long long *)(base + o_words), *d_br = (unsigned long long *)(base + o_br);
    unsigned long long *d_br2 = (unsigned long long *)(base + o_br2);
    uint32_t *d_sched = (uint32_t *)(base + o_sched), *d_off = (uint32_t *)(base + o_off);
    uint32_t *d_col = per_col ? (uint32_t *)(base + o_col) : nullptr, *d_gain = gains ? (uint32_t *)(base + o_gain) : nullptr;
    uint8_t *d_bytes = base + o_bytes;
    PSCHK(tm.timed(0, st, [&]() -> int {
        HIPCHK(hipMemsetAsync(d_words, 0, PS_PARS_WORDS * 8, st));
        if (down) HIPCHK(hipMemsetAsync(d_br, 0, (o_bytes - o_br), st));
        HIPCHK(hipMemcpyAsync(d_sched, sc.sched.data(), (uint64_t)M * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_off, sc.level_off.data(), (uint64_t)sc.level_off.size() * 4, hipMemcpyHostToDevice, st));
        return PS_OK;
    }));
    HIPCHK(hipStreamSynchronize(st));        // (the two sources are this function's own)
    if (total) {
        // the node dwords, and the branch counters behind them while both stay below 96 KiB; teams as wide as the tree needs
        const uint32_t node_bytes = slots * 4u, ctr_bytes = down ? node_bytes * (genes ? 2u : 1u) : 0u;
        const uint32_t lds_counters = down && node_bytes + ctr_bytes <= 96u * 1024u ? 1u : 0u;
        // ... and the schedule's copy behind both while the three stay below 64 KiB
        const uint32_t sched_bytes = (M + t.levels + 1u) * 4u;
        const uint32_t sched_lds = node_bytes + (lds_counters ? ctr_bytes : 0u) + sched_bytes <= 64u * 1024u ? 1u : 0u;
        const uint32_t lds = node_bytes + (lds_counters ? ctr_bytes : 0u) + (sched_lds ? sched_bytes : 0u);
        const uint32_t threads = N <= 1024u ? 64u : N <= 4096u ? 256u : 1024u;
        const uint32_t per_cu = std::max(1u, std::min(std::min(2048u / threads, 32u), (160u * 1024u) / (lds + 1024u)));
        auto kern = genes ? (down ? tree_fitch_kernel<true, true> : tree_fitch_kernel<true, false>)
                          : (down ? tree_fitch_kernel<false, true> : tree_fitch_kernel<false, false>);
        if (lds > 32768u) HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        PSCHK(tm.timed(genes ? 2 : 1, st, [&]() -> int {
            if (genes) PSCHK(ensure_gene_major(p, st));
            for (uint32_t first = 0; first < total; first += chunk) {
                const uint32_t rows = std::min(chunk, total - first);
                if (genes) {
                    const uint64_t pieces = (uint64_t)rows * (pitch >> 4);
                    pars_expand_genes_kernel<<<(uint32_t)std::min<uint64_t>((pieces + 255u) / 256u, 4096u), 256, 0, st>>>(p->G[0], p->d, first, rows,
                                                                                                                        pitch, d_bytes);
                    HIPCHK(hipGetLastError());
                }
                const uint32_t grid = std::max(1u, std::min((rows + 3u) / 4u, 256u * per_cu));
                hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, genes ? (const uint8_t *)d_bytes : (const uint8_t *)p->state, pitch, N,
                                   rows, (const uint32_t *)d_sched, (const uint32_t *)d_off, t.levels, M, sc.n_pad, lds_counters, sched_lds, d_words, d_col,
                                   d_gain, first, d_br, d_br2);
                HIPCHK(hipGetLastError());
            }
            return PS_OK;
        }));
    }
    unsigned long long words[PS_PARS_WORDS];
    std::vector<unsigned long long> hb(down ? (size_t)slots * (genes ? 2 : 1) : 0);
    HIPCHK(hipMemcpyAsync(words, d_words, sizeof words, hipMemcpyDeviceToHost, st));
    if (total && per_col) HIPCHK(hipMemcpyAsync(per_col, d_col, (uint64_t)total * 4, hipMemcpyDeviceToHost, st));
    if (total && gains) HIPCHK(hipMemcpyAsync(per_gain, d_gain, (uint64_t)total * 4, hipMemcpyDeviceToHost, st));
    if (down) HIPCHK(hipMemcpyAsync(hb.data(), d_br, (uint64_t)slots * 8, hipMemcpyDeviceToHost, st));
    if (down && genes) HIPCHK(hipMemcpyAsync(hb.data() + slots, d_br2, (uint64_t)slots * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    sums->total = words[PS_PARS_W_TOTAL];
    sums->changed = words[PS_PARS_W_CHANGED];
    sums->maxc = words[PS_PARS_W_MAX];
    sums->minc = words[PS_PARS_W_MIN];
    sums->homo = words[PS_PARS_W_HOMO];
    sums->gains = words[PS_PARS_W_GAINS];
    for (int b = 0; b < PS_PARS_BINS; b++) sums->hist[b] = words[PS_PARS_W_HIST + b];
    if (down)
        for (uint32_t x = 0; x < N + M; x++) {
            br[x] = hb[sc.slot_of[x]];
            if (genes) br2[x] = hb[(size_t)slots + sc.slot_of[x]];
        }
    return PS_OK;
}

static int pars_handles(const ps_population *core, const ps_population *acc, const char *call)
{
    if (!core->cfg.core) return ps_fail(PS_ERR_INVALID, "%s takes a core handle first", call);
    if (acc && acc->cfg.core) return ps_fail(PS_ERR_INVALID, "%s takes an accessory handle (or NULL) second", call);
    if (acc && core->cfg.pop_size != acc->cfg.pop_size)
        return ps_fail(PS_ERR_INVALID, "%s: the core handle holds %llu individuals, the accessory handle %llu", call,
                       (unsigned long long)core->cfg.pop_size, (unsigned long long)acc->cfg.pop_size);
    if (acc && core->device != acc->device) return ps_fail(PS_ERR_INVALID, "%s: the two handles live on different devices", call);
    if (core->cfg.pop_size > PS_PARS_MAX_POP)
        return ps_fail(PS_ERR_INVALID, "%s needs pop_size <= %u, not %llu", call, PS_PARS_MAX_POP, (unsigned long long)core->cfg.pop_size);
    return PS_OK;
}

// The call behind the three device entries.  m == nullptr: `core` answers for its own sites; else every shard's core handle
// does and the results add (core, acc: shard 0's handles).  Genes: from `acc` when a gene output is asked for.
static int pars_run(ps_multi *m, ps_population *core, ps_population *acc, const uint32_t *left, const uint32_t *right, uint64_t merges,
                    ps_parsimony_t *out, const pars_outputs &o)
{
    const char *call = m ? "ps_multi_tree_parsimony" : "ps_tree_parsimony";
    PSCHK(pars_handles(core, acc, call));
    pars_tree t;
    PSCHK(pars_check_tree(left, right, merges, core->cfg.pop_size, &t));
    if (!m && acc && core->cfg.ncols != core->cfg.global_cols)
        return ps_fail(PS_ERR_INVALID, "%s: this core handle is one site shard ([%llu, %llu) of %llu sites): with an accessory handle use "
                                       "ps_multi_tree_parsimony", call, (unsigned long long)core->cfg.col_offset,
                       (unsigned long long)(core->cfg.col_offset + core->cfg.ncols), (unsigned long long)core->cfg.global_cols);
    if (o.genes() && !acc) return ps_fail(PS_ERR_INVALID, "%s: the gene outputs need the accessory handle", call);
    // everything queued on either handle precedes the passes of both
    if (m) {
        PSCHK(ps_multi_sync(m));
    } else {
        PSCHK(use_device(core));
        if (acc) HIPCHK(hipStreamSynchronize(acc->stream));
        HIPCHK(hipStreamSynchronize(core->stream));
    }
    const size_t S = m ? m->shard.size() : 1, nodes = (size_t)t.N + t.M;
    const uint64_t G = o.genes() ? acc->d.G : 0;
    const bool down = o.branch_changes != nullptr, gene_down = o.gene_down();
    std::vector<pars_sums> sums(S);
    pars_sums gsum;
    std::vector<std::vector<uint64_t>> br(S, std::vector<uint64_t>(down ? nodes : 0));
    std::vector<uint64_t> gbr(gene_down ? nodes : 0), gbr2(gene_down ? nodes : 0);
    std::vector<uint32_t> gch(std::max<uint64_t>(G, 1)), ggn(std::max<uint64_t>(G, 1));
    auto shard_pass = [&](size_t k) -> int {
        ps_population *c = m ? m->shard[k]->core : core;
        const uint64_t off = m ? c->cfg.col_offset : 0;
        event_timer tm;
        readout_slot &ro = c->ro[PS_RO_PARS];
        ro.timed = false;
        PSCHK(pars_pass(c, false, tm, t, left, right, down, o.site_changes ? o.site_changes + off : nullptr, nullptr, &sums[k], br[k].data(),
                        nullptr));
        if (k == 0 && o.genes()) {
            PSCHK(pars_pass(acc, true, tm, t, left, right, gene_down, gch.data(), ggn.data(), &gsum, gbr.data(), gbr2.data()));
            PSCHK(use_device(c));
        }
        return tm.collect(ro, 3);
    };
    if (m) PSCHK(multi_for_each(m, shard_pass));
    else PSCHK(shard_pass(0));
    pars_sums all;
    for (size_t k = 0; k < S; k++) all.add(sums[k]);
    if (o.site_hist) memcpy(o.site_hist, all.hist, sizeof all.hist);
    if (down) {
        memset(o.branch_changes, 0, nodes * sizeof(uint64_t));
        for (size_t k = 0; k < S; k++)
            for (size_t x = 0; x < nodes; x++) o.branch_changes[x] += br[k][x];
    }
    for (uint64_t y = 0; y < G; y++) {
        if (o.gene_changes) o.gene_changes[y] = gch[y];
        if (o.gene_gains) o.gene_gains[y] = ggn[y];
        if (o.gene_losses) o.gene_losses[y] = gch[y] - ggn[y];
    }
    if (o.branch_gains) memcpy(o.branch_gains, gbr.data(), nodes * sizeof(uint64_t));
    if (o.branch_losses) memcpy(o.branch_losses, gbr2.data(), nodes * sizeof(uint64_t));
    pars_summary(out, t, m ? m->prm.core_size : core->cfg.ncols, all, G, gsum, gene_down);
    return PS_OK;
}

#define PS_PARS_OUTPUTS { site_changes, site_hist, branch_changes, gene_changes, gene_gains, gene_losses, branch_gains, branch_losses }

extern "C" int ps_tree_parsimony(ps_population *core, ps_population *acc, const uint32_t *left, const uint32_t *right, uint64_t merges,
                                 ps_parsimony_t *out, uint32_t *site_changes, uint64_t *site_hist, uint64_t *branch_changes,
                                 uint32_t *gene_changes, uint32_t *gene_gains, uint32_t *gene_losses, uint64_t *branch_gains,
                                 uint64_t *branch_losses)
{
    PSCHK(ps_needs_device());
    if (!core || !out) return ps_fail(PS_ERR_INVALID, "null argument");
    return pars_run(nullptr, core, acc, left, right, merges, out, PS_PARS_OUTPUTS);
}

extern "C" int ps_sim_tree_parsimony(ps_sim *s, const uint32_t *left, const uint32_t *right, uint64_t merges, ps_parsimony_t *out,
                                     uint32_t *site_changes, uint64_t *site_hist, uint64_t *branch_changes, uint32_t *gene_changes,
                                     uint32_t *gene_gains, uint32_t *gene_losses, uint64_t *branch_gains, uint64_t *branch_losses)
{
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    return ps_tree_parsimony(s->core, s->acc, left, right, merges, out, site_changes, site_hist, branch_changes, gene_changes, gene_gains,
                             gene_losses, branch_gains, branch_losses);
}

extern "C" int ps_multi_tree_parsimony(ps_multi *m, const uint32_t *left, const uint32_t *right, uint64_t merges, ps_parsimony_t *out,
                                       uint32_t *site_changes, uint64_t *site_hist, uint64_t *branch_changes, uint32_t *gene_changes,
                                       uint32_t *gene_gains, uint32_t *gene_losses, uint64_t *branch_gains, uint64_t *branch_losses)
{
    PSCHK(ps_needs_device());
    if (!m || !out) return ps_fail(PS_ERR_INVALID, "null argument");
    if (m->shard.size() == 1)
        return ps_sim_tree_parsimony(m->shard[0], left, right, merges, out, site_changes, site_hist, branch_changes, gene_changes, gene_gains,
                                     gene_losses, branch_gains, branch_losses);
    return pars_run(m, m->shard[0]->core, m->shard[0]->acc, left, right, merges, out, PS_PARS_OUTPUTS);
}

#undef PS_PARS_OUTPUTS

extern "C" int ps_tree_parsimony_timing(ps_population *core, double *schedule_ms, double *core_ms, double *gene_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_PARS], "no tree parsimony has been computed on this handle", { schedule_ms, core_ms, gene_ms });
}
