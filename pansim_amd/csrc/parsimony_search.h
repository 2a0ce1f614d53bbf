// parsimony_search.h -- ps_tree_nni_deltas / ps_tree_nni / ps_sim_tree_nni / ps_multi_tree_nni, the host restatements
// ps_nni_deltas_from_rows and ps_nni_from_rows, and the host rules ps_merges_canonical and ps_nni_apply (include/pansim_hip.h;
// the definitions: docs/PARSIMONY_SEARCH.md).  Included by pansim_capi.hip behind tree_parsimony.h.
//
// One PASS gives the length T of a tree and the change of T under each of its 2 (N - 3) nearest-neighbour interchanges: on
// the device tree_nni_kernel over the handle's sites on its stream (the schedule is tree_parsimony.h's; the deltas come back
// per schedule position, 16 M bytes, and are mapped to merges here), on the host the same per-node functions over rows.  The
// SEARCH (nni_search) is one loop over either kind of pass: selection, surgery and the canonical form (nni_moves.h) run on the
// host, a sharded run adds the shards' T and deltas before the one selection.
#pragma once

#include <functional>

#include "nni_kernels.h"
#include "nni_moves.h"

// The LDS of a pass: the node dwords (4 bytes per slot) and the pairs of the merges (8 bytes each), the counters behind them
// while both stay below 96 KiB (N <= 4096 has them, N = 4097 does not), the schedule's copy behind both while the three stay
// below 64 KiB (a tree of N = 2320 leaves with up to 148 levels has it, no tree of N = 2352 does)
#define PS_NNI_LDS_COUNTERS (96u * 1024u)
#define PS_NNI_LDS_SCHED (64u * 1024u)

static int nni_check_tree(const char *call, const uint32_t *left, const uint32_t *right, uint64_t merges, uint64_t pop_size, pars_tree *t)
{
    if (pop_size < 2 || pop_size > PS_NNI_MAX_POP)
        return ps_fail(PS_ERR_INVALID, "%s needs 2 <= pop_size <= %u (two LDS dwords per node), not %llu", call, PS_NNI_MAX_POP,
                       (unsigned long long)pop_size);
    if (merges != pop_size - 1)
        return ps_fail(PS_ERR_INVALID, "%s needs a spanning tree: %llu merges over %llu leaves, not %llu", call,
                       (unsigned long long)(pop_size - 1), (unsigned long long)pop_size, (unsigned long long)merges);
    return pars_check_tree(left, right, merges, pop_size, t);
}

// delta[2 M] of a checked spanning tree before a pass adds to it: 0 where merge k has candidates, PS_NNI_NONE where it has none
static void nni_blank_deltas(const pars_tree &t, const uint32_t *left, const uint32_t *right, int64_t *delta)
{
    const uint32_t N = t.N, M = t.M, root = N + M - 1u;
    for (uint32_t k = 0; k < M; k++) {
        const uint32_t c = N + k;
        const bool some = c != root && ((uint32_t)t.parent[c] != root || (left[M - 1u] == c && right[M - 1u] >= N));
        delta[2u * k] = delta[2u * k + 1u] = some ? 0 : PS_NNI_NONE;
    }
}

// One pass on the host over individual-major rows: *total and *minc are set, delta[2 M] is filled
static void nni_host_pass(const uint8_t *rows, uint64_t cols, const pars_tree &t, const uint32_t *left, const uint32_t *right, uint64_t *total,
                          uint64_t *minc, int64_t *delta)
{
    const uint32_t N = t.N, M = t.M;
    nni_blank_deltas(t, left, right, delta);
    std::vector<uint32_t> S((size_t)N + M), U((size_t)N + M, 0u);
    *total = *minc = 0;
    auto count = [&](uint32_t c, const uint32_t m[3]) {
        const int64_t cur = __builtin_popcount(m[0]);
        delta[2u * (c - N)] += __builtin_popcount(m[1]) - cur;
        delta[2u * (c - N) + 1u] += __builtin_popcount(m[2]) - cur;
    };
    for (uint64_t c0 = 0; c0 < cols; c0 += 4) {
        const uint32_t w = (uint32_t)std::min<uint64_t>(4, cols - c0);
        uint32_t all = 0;
        for (uint32_t i = 0; i < N; i++) {
            uint32_t x = 0;
            for (uint32_t j = 0; j < w; j++) x |= (uint32_t)rows[(uint64_t)i * cols + c0 + j] << (8 * j);
            S[i] = ps_pars_classes(x);
            all |= S[i];
        }
        for (uint32_t j = 0; j < w; j++) *minc += (uint32_t)__builtin_popcount((all >> (8 * j)) & 0x1Fu) - 1u;
        for (uint32_t k = 0; k < M; k++) {
            uint32_t z;
            S[N + k] = ps_pars_join(S[left[k]], S[right[k]], &z);
            *total += (uint32_t)__builtin_popcount(z);
        }
        for (uint32_t k = M; k-- > 0;) {
            const uint32_t l = left[k], r = right[k];
            uint32_t m[3], z;
            if (k == M - 1u) {
                U[l] = S[r];
                U[r] = S[l];
                if (l >= N && r >= N) {
                    ps_nni_edge(S[left[l - N]], S[right[l - N]], S[left[r - N]], S[right[r - N]], m);
                    count(l, m);
                }
                continue;
            }
            const uint32_t uv = U[N + k];
            U[l] = ps_pars_join(uv, S[r], &z);
            U[r] = ps_pars_join(uv, S[l], &z);
            for (uint32_t side = 0; side < 2u; side++) {
                const uint32_t c = side ? r : l;
                if (c < N) continue;
                ps_nni_edge(S[left[c - N]], S[right[c - N]], S[side ? l : r], uv, m);
                count(c, m);
            }
        }
    }
}

// One pass of handle p over its own sites on its stream, complete when it returns: *total, *minc and delta[2 M] are set.  The
// schedule's upload is timer group 0, the kernel group 1.
static int nni_device_pass(ps_population *p, event_timer &tm, const pars_tree &t, const uint32_t *left, const uint32_t *right, uint64_t *total,
                           uint64_t *minc, int64_t *delta)
{
    const uint32_t N = t.N, M = t.M, rows = (uint32_t)p->cfg.ncols;
    PSCHK(use_device(p));
    const uint32_t *slot = nullptr;
    PSCHK(rows_current(p, &slot));
    pars_schedule sc;
    pars_make_schedule(t, left, right, slot, &sc);
    for (uint32_t c : { left[M - 1u], right[M - 1u] })
        if (c >= N) sc.sched[sc.slot_of[c] - sc.n_pad] |= PS_NNI_BELOW_ROOT;
    const uint32_t slots = (sc.n_pad + M + 1u) & ~1u;
    scratch_layout lay;
    const uint64_t o_words = lay.add(PS_NNI_WORDS * 8, 16), o_delta = lay.add((uint64_t)M * 16, 16);
    const uint64_t o_sched = lay.add((uint64_t)M * 4, 16), o_off = lay.add((uint64_t)sc.level_off.size() * 4, 16);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(p->ro[PS_RO_NNI], lay.bytes, &base, "cannot allocate the %llu bytes of the schedule and the counters of the interchanges of a tree of %u merges", M));
    hipStream_t st = p->stream;
    unsigned long long *d_words = (unsigned long long *)(base + o_words), *d_delta = (unsigned long long *)(base + o_delta);
    uint32_t *d_sched = (uint32_t *)(base + o_sched), *d_off = (uint32_t *)(base + o_off);
    // (the sources of the two copies live until this function's last synchronisation)
    PSCHK(tm.timed(0, st, [&]() -> int {
        HIPCHK(hipMemsetAsync(d_words, 0, o_sched, st));
        HIPCHK(hipMemcpyAsync(d_sched, sc.sched.data(), (uint64_t)M * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_off, sc.level_off.data(), (uint64_t)sc.level_off.size() * 4, hipMemcpyHostToDevice, st));
        return PS_OK;
    }));
    if (rows) {
        const uint32_t node_bytes = slots * 4u + M * 8u, ctr_bytes = M * 8u, sched_bytes = (M + t.levels + 1u) * 4u;
        const uint32_t lds_counters = node_bytes + ctr_bytes <= PS_NNI_LDS_COUNTERS ? 1u : 0u;
        const uint32_t sched_lds = node_bytes + (lds_counters ? ctr_bytes : 0u) + sched_bytes <= PS_NNI_LDS_SCHED ? 1u : 0u;
        const uint32_t lds = node_bytes + (lds_counters ? ctr_bytes : 0u) + (sched_lds ? sched_bytes : 0u);
        const uint32_t threads = N <= 1024u ? 64u : N <= 4096u ? 256u : 1024u;
        const uint32_t per_cu = std::max(1u, std::min(std::min(2048u / threads, 32u), (160u * 1024u) / (lds + 1024u)));
        if (lds > 32768u) HIPCHK(hipFuncSetAttribute((const void *)tree_nni_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        PSCHK(tm.timed(1, st, [&]() -> int {
            const uint32_t grid = std::max(1u, std::min((rows + 3u) / 4u, 256u * per_cu));
            hipLaunchKernelGGL(tree_nni_kernel, dim3(grid), dim3(threads), lds, st, (const uint8_t *)p->state, p->pitch, N, rows,
                               (const uint32_t *)d_sched, (const uint32_t *)d_off, t.levels, M, sc.n_pad, lds_counters, sched_lds, d_words, d_delta);
            HIPCHK(hipGetLastError());
            return PS_OK;
        }));
    }
    unsigned long long words[PS_NNI_WORDS];
    std::vector<int64_t> by_slot((size_t)2 * M);
    HIPCHK(hipMemcpyAsync(words, d_words, sizeof words, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(by_slot.data(), d_delta, (uint64_t)M * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *total = words[PS_NNI_W_TOTAL];
    *minc = words[PS_NNI_W_MIN];
    nni_blank_deltas(t, left, right, delta);
    for (uint32_t k = 0; k < M; k++) {
        const uint32_t j = sc.slot_of[N + k] - sc.n_pad;
        if (delta[2u * k] == PS_NNI_NONE) continue;
        delta[2u * k] = by_slot[2u * j];
        delta[2u * k + 1u] = by_slot[2u * j + 1u];
    }
    return PS_OK;
}

// a pass over the tree of a canonical merge list: T, the sum of (classes - 1) over the sites, delta[2 M]
typedef std::function<int(const uint32_t *left, const uint32_t *right, uint64_t *total, uint64_t *minc, int64_t *delta)> nni_pass_fn;

// what a search returns besides the summary (any may be null; the moves: the first move_cap)
struct nni_outputs {
    uint32_t *left, *right;
    uint64_t *round_changes;
    uint32_t *move_round, *move_node, *move_kind;
    int64_t *move_delta;
    uint64_t move_cap;
};

static int nni_check_params(const ps_nni_params *prm, const ps_nni_t *out, const nni_outputs &o)
{
    if (!prm || !out) return ps_fail(PS_ERR_INVALID, "null argument");
    if (prm->max_rounds < 1) return ps_fail(PS_ERR_INVALID, "max_rounds must be at least 1, not 0");
    if (o.move_cap && (!o.move_round || !o.move_node || !o.move_kind || !o.move_delta))
        return ps_fail(PS_ERR_INVALID, "move_cap = %llu needs the four move arrays", (unsigned long long)o.move_cap);
    return PS_OK;
}

// The search loop of docs/PARSIMONY_SEARCH.md from a checked spanning tree
static int nni_search(uint32_t N, const uint32_t *left0, const uint32_t *right0, const ps_nni_params &prm, uint64_t sites, const nni_pass_fn &pass,
                      ps_nni_t *out, const nni_outputs &o)
{
    const uint32_t M = N - 1u;
    nni_topology top;
    nni_from_merges(N, left0, right0, &top);
    std::vector<uint32_t> left(M), right(M), nl(M), nr(M);
    nni_to_canonical(top, left.data(), right.data());
    std::vector<int64_t> delta((size_t)2 * M), nd((size_t)2 * M);
    uint64_t T = 0, minc = 0, rounds = 0, passes = 0, rollbacks = 0, moves = 0, improving = 0;
    PSCHK(pass(left.data(), right.data(), &T, &minc, delta.data()));
    passes++;
    const uint64_t start = T;
    if (o.round_changes) o.round_changes[0] = T;
    int optimum = 0;
    for (;;) {
        nni_from_merges(N, left.data(), right.data(), &top);
        std::vector<nni_candidate> batch = nni_select(top, delta.data(), prm.moves_per_round, &improving);
        if (batch.empty()) {
            optimum = 1;
            break;
        }
        if (rounds == prm.max_rounds) break;
        uint64_t T2 = 0, m2 = 0;
        for (;;) {
            nni_topology next = top;
            for (const nni_candidate &c : batch) nni_apply_move(next, c.node, c.kind);
            nni_to_canonical(next, nl.data(), nr.data());
            PSCHK(pass(nl.data(), nr.data(), &T2, &m2, nd.data()));
            passes++;
            // moves of one batch touch disjoint nodes but their deltas need not add: never worse than the best move alone
            if (batch.size() == 1 || (int64_t)T2 <= (int64_t)T + batch[0].delta) break;
            rollbacks++;
            batch.resize(1);
        }
        rounds++;
        for (const nni_candidate &c : batch) {
            if (moves < o.move_cap) {
                o.move_round[moves] = (uint32_t)rounds;
                o.move_node[moves] = c.node;
                o.move_kind[moves] = c.kind;
                o.move_delta[moves] = c.delta;
            }
            moves++;
        }
        T = T2;
        left.swap(nl);
        right.swap(nr);
        delta.swap(nd);
        if (o.round_changes) o.round_changes[rounds] = T;
    }
    memset(out, 0, sizeof *out);
    out->pop_size = N;
    out->sites = sites;
    out->merges = M;
    out->rounds = rounds;
    out->passes = passes;
    out->rollbacks = rollbacks;
    out->moves = moves;
    out->local_optimum = (uint64_t)optimum;
    out->start_changes = start;
    out->total_changes = T;
    out->min_changes = minc;
    out->candidates_last = improving;
    if (o.left) memcpy(o.left, left.data(), (size_t)M * sizeof(uint32_t));
    if (o.right) memcpy(o.right, right.data(), (size_t)M * sizeof(uint32_t));
    return PS_OK;
}

extern "C" int ps_merges_canonical(const uint32_t *left, const uint32_t *right, uint64_t merges, uint64_t pop_size, uint32_t *out_left,
                                   uint32_t *out_right)
{
    if (!out_left || !out_right) return ps_fail(PS_ERR_INVALID, "null argument");
    pars_tree t;
    PSCHK(nni_check_tree("ps_merges_canonical", left, right, merges, pop_size, &t));
    nni_topology top;
    nni_from_merges(t.N, left, right, &top);
    nni_to_canonical(top, out_left, out_right);
    return PS_OK;
}

extern "C" int ps_nni_apply(const uint32_t *left, const uint32_t *right, uint64_t merges, uint64_t pop_size, uint32_t node, uint32_t kind,
                            uint32_t *out_left, uint32_t *out_right)
{
    if (!out_left || !out_right) return ps_fail(PS_ERR_INVALID, "null argument");
    pars_tree t;
    PSCHK(nni_check_tree("ps_nni_apply", left, right, merges, pop_size, &t));
    if (kind > 1u) return ps_fail(PS_ERR_INVALID, "kind must be 0 or 1, not %u", kind);
    nni_topology top;
    nni_from_merges(t.N, left, right, &top);
    uint32_t touched[7];
    if (node < t.N || node >= t.N + t.M || !nni_touched(top, node, touched))
        return ps_fail(PS_ERR_INVALID, "node %u has no interchange in this tree (the root, its right child, its left child beside a leaf and "
                                       "the leaves have none)", node);
    nni_apply_move(top, node, kind);
    nni_to_canonical(top, out_left, out_right);
    return PS_OK;
}

extern "C" int ps_nni_deltas_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                       uint64_t merges, uint64_t *total, int64_t *delta)
{
    if (!total || !delta || (!rows && cols)) return ps_fail(PS_ERR_INVALID, "null argument");
    pars_tree t;
    PSCHK(nni_check_tree("ps_nni_deltas_from_rows", left, right, merges, pop_size, &t));
    uint64_t minc;
    nni_host_pass(rows, cols, t, left, right, total, &minc, delta);
    return PS_OK;
}

extern "C" int ps_nni_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                uint64_t merges, const ps_nni_params *prm, ps_nni_t *out, uint32_t *out_left, uint32_t *out_right,
                                uint64_t *round_changes, uint32_t *move_round, uint32_t *move_node, uint32_t *move_kind, int64_t *move_delta,
                                uint64_t move_cap)
{
    const nni_outputs o = { out_left, out_right, round_changes, move_round, move_node, move_kind, move_delta, move_cap };
    PSCHK(nni_check_params(prm, out, o));
    if (!rows && cols) return ps_fail(PS_ERR_INVALID, "null argument");
    pars_tree t;
    PSCHK(nni_check_tree("ps_nni_from_rows", left, right, merges, pop_size, &t));
    const nni_pass_fn pass = [&](const uint32_t *l, const uint32_t *r, uint64_t *total, uint64_t *minc, int64_t *delta) -> int {
        pars_tree tt;
        PSCHK(pars_check_tree(l, r, merges, pop_size, &tt));
        nni_host_pass(rows, cols, tt, l, r, total, minc, delta);
        return PS_OK;
    };
    return nni_search(t.N, left, right, *prm, cols, pass, out, o);
}

static int nni_handle(const ps_population *core, const char *call)
{
    if (!core->cfg.core) return ps_fail(PS_ERR_INVALID, "%s takes a core handle: the search is over core sites", call);
    return PS_OK;
}

// everything queued on the handle (the run) precedes the passes
static int nni_order_behind(ps_multi *m, ps_population *core)
{
    if (m) return ps_multi_sync(m);
    PSCHK(use_device(core));
    HIPCHK(hipStreamSynchronize(core->stream));
    return PS_OK;
}

extern "C" int ps_tree_nni_deltas(ps_population *core, const uint32_t *left, const uint32_t *right, uint64_t merges, uint64_t *total,
                                  int64_t *delta)
{
    PSCHK(ps_needs_device());
    if (!core || !total || !delta) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(nni_handle(core, "ps_tree_nni_deltas"));
    pars_tree t;
    PSCHK(nni_check_tree("ps_tree_nni_deltas", left, right, merges, core->cfg.pop_size, &t));
    PSCHK(nni_order_behind(nullptr, core));
    event_timer tm;
    readout_slot &ro = core->ro[PS_RO_NNI];
    ro.timed = false;
    uint64_t minc;
    PSCHK(nni_device_pass(core, tm, t, left, right, total, &minc, delta));
    return tm.collect(ro, 2);
}

// The call behind the three device entries.  m == nullptr: `core` answers for its own sites; else every shard's core handle
// does, and T and the deltas add before the selection
static int nni_run(ps_multi *m, ps_population *core, const uint32_t *left, const uint32_t *right, uint64_t merges, const ps_nni_params *prm,
                   ps_nni_t *out, const nni_outputs &o)
{
    const char *call = m ? "ps_multi_tree_nni" : "ps_tree_nni";
    PSCHK(nni_check_params(prm, out, o));
    PSCHK(nni_handle(core, call));
    pars_tree t;
    PSCHK(nni_check_tree(call, left, right, merges, core->cfg.pop_size, &t));
    PSCHK(nni_order_behind(m, core));
    const size_t S = m ? m->shard.size() : 1;
    std::vector<event_timer> tm(S);
    std::vector<uint64_t> tot(S), mn(S);
    std::vector<std::vector<int64_t>> dl(S, std::vector<int64_t>((size_t)2 * t.M));
    for (size_t k = 0; k < S; k++) (m ? m->shard[k]->core : core)->ro[PS_RO_NNI].timed = false;
    const nni_pass_fn pass = [&](const uint32_t *l, const uint32_t *r, uint64_t *total, uint64_t *minc, int64_t *delta) -> int {
        pars_tree tt;
        PSCHK(pars_check_tree(l, r, merges, core->cfg.pop_size, &tt));
        auto shard_pass = [&](size_t k) -> int {
            return nni_device_pass(m ? m->shard[k]->core : core, tm[k], tt, l, r, &tot[k], &mn[k], dl[k].data());
        };
        if (m) PSCHK(multi_for_each(m, shard_pass));
        else PSCHK(shard_pass(0));
        *total = *minc = 0;
        nni_blank_deltas(tt, l, r, delta);
        for (size_t k = 0; k < S; k++) {
            *total += tot[k];
            *minc += mn[k];
            for (size_t i = 0; i < (size_t)2 * tt.M; i++)
                if (delta[i] != PS_NNI_NONE) delta[i] += dl[k][i];
        }
        return PS_OK;
    };
    PSCHK(nni_search(t.N, left, right, *prm, m ? m->prm.core_size : core->cfg.ncols, pass, out, o));
    for (size_t k = 0; k < S; k++) {
        ps_population *c = m ? m->shard[k]->core : core;
        PSCHK(use_device(c));
        PSCHK(tm[k].collect(c->ro[PS_RO_NNI], 2));
    }
    return use_device(core);
}

#define PS_NNI_OUTPUTS { out_left, out_right, round_changes, move_round, move_node, move_kind, move_delta, move_cap }

extern "C" int ps_tree_nni(ps_population *core, const uint32_t *left, const uint32_t *right, uint64_t merges, const ps_nni_params *prm,
                           ps_nni_t *out, uint32_t *out_left, uint32_t *out_right, uint64_t *round_changes, uint32_t *move_round,
                           uint32_t *move_node, uint32_t *move_kind, int64_t *move_delta, uint64_t move_cap)
{
    PSCHK(ps_needs_device());
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return nni_run(nullptr, core, left, right, merges, prm, out, PS_NNI_OUTPUTS);
}

extern "C" int ps_sim_tree_nni(ps_sim *s, const uint32_t *left, const uint32_t *right, uint64_t merges, const ps_nni_params *prm, ps_nni_t *out,
                               uint32_t *out_left, uint32_t *out_right, uint64_t *round_changes, uint32_t *move_round, uint32_t *move_node,
                               uint32_t *move_kind, int64_t *move_delta, uint64_t move_cap)
{
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    return nni_run(nullptr, s->core, left, right, merges, prm, out, PS_NNI_OUTPUTS);
}

extern "C" int ps_multi_tree_nni(ps_multi *m, const uint32_t *left, const uint32_t *right, uint64_t merges, const ps_nni_params *prm,
                                 ps_nni_t *out, uint32_t *out_left, uint32_t *out_right, uint64_t *round_changes, uint32_t *move_round,
                                 uint32_t *move_node, uint32_t *move_kind, int64_t *move_delta, uint64_t move_cap)
{
    PSCHK(ps_needs_device());
    if (!m) return ps_fail(PS_ERR_INVALID, "null argument");
    if (m->shard.size() == 1) return nni_run(nullptr, m->shard[0]->core, left, right, merges, prm, out, PS_NNI_OUTPUTS);
    return nni_run(m, m->shard[0]->core, left, right, merges, prm, out, PS_NNI_OUTPUTS);
}

#undef PS_NNI_OUTPUTS

extern "C" int ps_tree_nni_timing(ps_population *core, double *schedule_ms, double *pass_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_NNI], "no tree search has been computed on this handle", { schedule_ms, pass_ms });
}
