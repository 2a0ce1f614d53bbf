// likelihood_search.h -- ps_tree_model_nni_deltas / ps_tree_model_nni with their ps_sim_ and ps_multi_ forms, the host restatements
// ps_model_nni_deltas_from_rows and ps_model_nni_from_rows, and the host rules ps_merges_canonical_lengths and ps_nni_apply_lengths
// (include/pansim_hip.h; the definitions: docs/LIKELIHOOD_SEARCH.md).  Included by pansim_capi.hip behind tree_model.h, whose
// model, length checks, device frame and branch-length optimiser it shares, and parsimony_search.h, whose candidate table it uses.
//
// One PASS gives lnL of a tree with branch lengths under the model and, for each of its 2 (N - 3) nearest-neighbour interchanges,
// the product over the sites of l' / l as (mantissa, exponent): on the device tree_model_nni_kernel over the handle's sites on its
// stream (the products come back per schedule position and are mapped to merges here), on the host the same subst_rule.h
// functions over rows, the sites in ascending order.  The SEARCH (mnni_search) is one loop over either kind of pass; selection,
// surgery and the canonical form (nni_moves.h) run on the host, a sharded run multiplies the shards' products in shard order
// before the one selection.
#pragma once

#include "model_nni_kernels.h"
#include "nni_moves.h"
#include "tree_model.h"

// what one pass returns: lnL, the missing cells, the sites of likelihood 0, and (mant, ex)[2 M] per merge and kind, mant = 0
// where there is no candidate
struct mnni_result {
    double lnl = 0.0;
    uint64_t missing = 0, zero_sites = 0;
    std::vector<double> mant;
    std::vector<int64_t> ex;
};

static int mnni_check_tree(const char *call, const uint32_t *left, const uint32_t *right, uint64_t merges, uint64_t pop_size, pars_tree *t)
{
    if (pop_size < 2 || pop_size > PS_MODEL_NNI_MAX_POP)
        return ps_fail(PS_ERR_INVALID, "%s needs 2 <= pop_size <= PS_MODEL_NNI_MAX_POP = %u (4 LDS bytes per leaf and 140 per merge), not %llu", call,
                       PS_MODEL_NNI_MAX_POP, (unsigned long long)pop_size);
    if (merges != pop_size - 1)
        return ps_fail(PS_ERR_INVALID, "%s needs a spanning tree: %llu merges over %llu leaves, not %llu", call,
                       (unsigned long long)(pop_size - 1), (unsigned long long)pop_size, (unsigned long long)merges);
    return pars_check_tree(left, right, merges, pop_size, t);
}

// whether merge k has candidates: the table of ps_tree_nni (nni_blank_deltas)
static bool mnni_has_candidates(const pars_tree &t, const uint32_t *left, const uint32_t *right, uint32_t k)
{
    const uint32_t N = t.N, M = t.M, root = N + M - 1u, c = N + k;
    return c != root && ((uint32_t)t.parent[c] != root || (left[M - 1u] == c && right[M - 1u] >= N));
}

// The LDS of a pass (model_nni_kernels.h): 4 n_pad + 140 Mp bytes and the schedule's copy behind them under PS_LIK_LDS_SCHED
static uint32_t mnni_lds_bytes(uint32_t N, uint32_t levels, uint32_t *sched_lds)
{
    const uint32_t n_pad = (N + 15u) & ~15u, M = N - 1u, Mp = (M + 1u) & ~1u;
    const uint32_t base = n_pad * 4u + Mp * 140u, sched = (M + levels + 1u) * 4u;
    *sched_lds = base + sched <= PS_LIK_LDS_SCHED ? 1u : 0u;
    return base + (*sched_lds ? sched : 0u);
}

// One pass on the host over individual-major rows, the sites in ascending order.  cls: the class of site 0 on (null: none);
// x[K][N + M]
static void mnni_host_pass(const uint8_t *rows, uint64_t cols, const pars_tree &t, const uint32_t *left, const uint32_t *right, const model_host &mh,
                           const uint8_t *cls, const double *x, mnni_result *res)
{
    const uint32_t N = t.N, M = t.M, nodes = N + M, K = mh.K();
    const double *pi = mh.a.freq, *rho = mh.a.root;
    std::vector<double> L((size_t)K * 4 * nodes), TP((size_t)4 * nodes), MS((size_t)4 * nodes), tmp((size_t)2 * M, 0.0);
    std::vector<int32_t> E((size_t)K * nodes, 0);
    std::vector<uint8_t> some(M);
    for (uint32_t k = 0; k < M; k++) some[k] = mnni_has_candidates(t, left, right, k);
    res->mant.assign((size_t)2 * M, 0.5);
    res->ex.assign((size_t)2 * M, 1);
    res->lnl = 0.0;
    res->missing = res->zero_sites = 0;
    for (uint64_t s = 0; s < cols; s++) {
        const bool assigned = cls || K == 1u;
        const uint32_t kb = assigned ? (cls ? cls[s] : 0u) : 0u, ke = assigned ? kb + 1u : K;
        double mant[PS_MODEL_MAX_CATEGORIES] = {}, post[PS_MODEL_MAX_CATEGORIES] = {};
        int32_t ex[PS_MODEL_MAX_CATEGORIES] = {};
        for (uint32_t i = 0; i < N; i++) res->missing += !ps_jc_known(rows[(uint64_t)i * cols + s]);
        for (uint32_t k = kb; k < ke; k++) {
            double *Lk = &L[(size_t)k * 4 * nodes];
            int32_t *Ek = &E[(size_t)k * nodes];
            const double *xk = x + (size_t)k * nodes;
            for (uint32_t i = 0; i < N; i++) ps_jc_leaf(rows[(uint64_t)i * cols + s], &Lk[4u * i]);
            for (uint32_t j = 0; j < M; j++) {
                const uint32_t l = left[j], r = right[j];
                double ml[4], mr[4];
                ps_subst_up(xk[l], pi, &Lk[4u * l], ml);
                ps_subst_up(xk[r], pi, &Lk[4u * r], mr);
                Ek[N + j] = (Ek[l] + Ek[r]) + ps_jc_join(ml, mr, &Lk[4u * (N + j)]);
            }
            mant[k] = ps_subst_site(rho, &Lk[4u * (nodes - 1u)]);
            ex[k] = Ek[nodes - 1u];
        }
        double sm;
        int32_t se;
        if (assigned) {
            sm = mant[kb];
            se = ex[kb];
            post[kb] = 1.0;
        } else
            sm = ps_subst_mix(K, mh.a.weight, mant, ex, &se, post);
        res->lnl += ps_jc_site_ln(sm, se);
        if (!(sm > 0.0)) {
            res->zero_sites++;
            continue;
        }
        for (uint32_t k = kb; k < ke; k++) {
            const double *Lk = &L[(size_t)k * 4 * nodes], *xk = x + (size_t)k * nodes;
            const bool first = k == kb, last = k + 1u == ke;
            auto count = [&](uint32_t j, const double l3[3]) {
                for (uint32_t kind = 0; kind < 2u; kind++) {
                    const size_t i = (size_t)2 * j + kind;
                    const double term = ps_subst_nni_term(post[k], l3[1u + kind], l3[0]), r = first ? term : tmp[i] + term;
                    if (last) {
                        int32_t e2;
                        res->mant[i] = ps_subst_prod(res->mant[i], r, &e2);
                        res->ex[i] += e2;
                    } else
                        tmp[i] = r;
                }
            };
            for (uint32_t j = M; j-- > 0;) {
                const uint32_t l = left[j], r = right[j], c = N + j;
                double Tv[4] = { rho[0], rho[1], rho[2], rho[3] }, ml[4], mr[4], l3[3];
                ps_subst_up(xk[l], pi, &Lk[4u * l], ml);
                ps_subst_up(xk[r], pi, &Lk[4u * r], mr);
                if (j == M - 1u) {
                    if (l >= N && r >= N) {
                        double ma[4], mb[4], mp[4], mq[4];
                        const uint32_t a = left[l - N], b = right[l - N], p = left[r - N], q = right[r - N];
                        ps_subst_up(xk[a], pi, &Lk[4u * a], ma);
                        ps_subst_up(xk[b], pi, &Lk[4u * b], mb);
                        ps_subst_up(xk[p], pi, &Lk[4u * p], mp);
                        ps_subst_up(xk[q], pi, &Lk[4u * q], mq);
                        ps_subst_nni_root_edge(xk[l], xk[r], pi, rho, ma, mb, mp, mq, l3);
                        count(l - N, l3);
                    }
                } else {
                    const double *Tp = &TP[4u * c], *ms = &MS[4u * c];
                    if ((uint32_t)t.parent[c] != nodes - 1u) {     // (the root's children have no interchange of their own)
                        ps_subst_nni_edge(xk[c], pi, ml, mr, ms, Tp, l3);
                        count(j, l3);
                    }
                    double U[4];
                    (void)ps_jc_join(ms, Tp, U);
                    ps_subst_down(xk[c], pi, U, Tv);
                }
                for (uint32_t side = 0; side < 2u; side++) {
                    const uint32_t ch = side ? r : l;
                    if (ch < N) continue;
                    memcpy(&TP[4u * ch], Tv, sizeof Tv);
                    memcpy(&MS[4u * ch], side ? ml : mr, sizeof ml);
                }
            }
        }
    }
    for (uint32_t k = 0; k < M; k++)
        if (!some[k]) {
            res->mant[2u * k] = res->mant[2u * k + 1u] = 0.0;
            res->ex[2u * k] = res->ex[2u * k + 1u] = 0;
        }
}

// One pass of handle p over its own sites on its stream, complete when it returns.  cls: the classes of p's own sites (null: none).
// Timer groups: 0 the uploads, 1 the kernel, 2 the product of the workgroups' rows.
static int mnni_device_pass(ps_population *p, event_timer &tm, const pars_tree &t, const uint32_t *left, const uint32_t *right, const model_host &mh,
                            const uint8_t *cls, const double *x, mnni_result *res)
{
    const uint32_t N = t.N, M = t.M, nodes = N + M, rows = (uint32_t)p->cfg.ncols, K = mh.K();
    PSCHK(use_device(p));
    const uint32_t *slot = nullptr;
    PSCHK(rows_current(p, &slot));
    pars_schedule sc;
    pars_make_schedule(t, left, right, slot, &sc);
    for (uint32_t c : { left[M - 1u], right[M - 1u] })
        if (c >= N) sc.sched[sc.slot_of[c] - sc.n_pad] |= PS_NNI_BELOW_ROOT;
    const uint32_t slots = sc.n_pad + M, n = 2u * M;
    std::vector<double> xs((size_t)K * slots, 1.0);
    for (uint32_t k = 0; k < K; k++)
        for (uint32_t c = 0; c + 1u < nodes; c++) xs[(size_t)k * slots + sc.slot_of[c]] = x[(size_t)k * nodes + c];
    uint32_t sched_lds = 0;
    const uint32_t lds = mnni_lds_bytes(N, t.levels, &sched_lds);
    const uint32_t threads = 64u;               // (N <= PS_MODEL_NNI_MAX_POP = 1024: tree_model_kernel's single wave)
    const uint32_t per_cu = std::max(1u, std::min(8u, (160u * 1024u) / (lds + 1024u + 512u)));
    const uint32_t grid = std::max(1u, std::min((rows + 3u) / 4u, 256u * per_cu));
    scratch_layout lay;
    const uint64_t o_counts = lay.add(16, 16), o_lnl = lay.add(8, 16), o_mant = lay.add((uint64_t)n * 8, 16), o_exp = lay.add((uint64_t)n * 8, 16);
    const uint64_t o_sched = lay.add((uint64_t)M * 4, 16), o_off = lay.add((uint64_t)sc.level_off.size() * 4, 16);
    const uint64_t o_x = lay.add((uint64_t)K * slots * 8, 16), o_cls = lay.add(cls ? (uint64_t)rows : 0, 16);
    const uint64_t o_pm = lay.add((uint64_t)grid * n * 8, 16), o_pe = lay.add((uint64_t)grid * n * 4, 16), o_pl = lay.add((uint64_t)grid * 8, 16);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(p->ro[PS_RO_MODEL_NNI], lay.bytes, &base,
                      "cannot allocate the %llu bytes of the schedule, the x table and the products of the interchanges of a tree of %u merges over %u sites",
                      M, rows));
    hipStream_t st = p->stream;
    unsigned long long *d_counts = (unsigned long long *)(base + o_counts);
    double *d_lnl = (double *)(base + o_lnl), *d_mant = (double *)(base + o_mant), *d_x = (double *)(base + o_x);
    long long *d_exp = (long long *)(base + o_exp);
    uint32_t *d_sched = (uint32_t *)(base + o_sched), *d_off = (uint32_t *)(base + o_off);
    uint8_t *d_cls = cls && rows ? base + o_cls : nullptr;
    double *d_pm = (double *)(base + o_pm), *d_pl = (double *)(base + o_pl);
    int32_t *d_pe = (int32_t *)(base + o_pe);
    // (the sources of the copies live until this function's last synchronisation)
    PSCHK(tm.timed(0, st, [&]() -> int {
        HIPCHK(hipMemsetAsync(d_counts, 0, o_sched, st));
        HIPCHK(hipMemcpyAsync(d_sched, sc.sched.data(), (uint64_t)M * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_off, sc.level_off.data(), (uint64_t)sc.level_off.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_x, xs.data(), (uint64_t)K * slots * 8, hipMemcpyHostToDevice, st));
        if (d_cls) HIPCHK(hipMemcpyAsync(d_cls, cls, rows, hipMemcpyHostToDevice, st));
        return PS_OK;
    }));
    if (rows) {
        if (lds > 32768u)
            HIPCHK(hipFuncSetAttribute((const void *)tree_model_nni_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        PSCHK(tm.timed(1, st, [&]() -> int {
            hipLaunchKernelGGL(tree_model_nni_kernel, dim3(grid), dim3(threads), lds, st, (const uint8_t *)p->state, p->pitch, N, rows,
                               (const uint32_t *)d_sched, (const uint32_t *)d_off, t.levels, M, sc.n_pad, (const double *)d_x, sched_lds, mh.a,
                               (const uint8_t *)d_cls, d_pm, d_pe, d_pl, d_counts);
            HIPCHK(hipGetLastError());
            return PS_OK;
        }));
        PSCHK(tm.timed(2, st, [&]() -> int {
            hipLaunchKernelGGL(model_nni_reduce_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, (const double *)d_pm, (const int32_t *)d_pe,
                               (const double *)d_pl, grid, n, d_mant, d_exp, d_lnl);
            HIPCHK(hipGetLastError());
            return PS_OK;
        }));
    }
    unsigned long long counts[2] = { 0, 0 };
    double lnl = 0.0;
    std::vector<double> by_m(n, 0.5);
    std::vector<long long> by_e(n, 1);
    HIPCHK(hipMemcpyAsync(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost, st));
    if (rows) {
        HIPCHK(hipMemcpyAsync(&lnl, d_lnl, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(by_m.data(), d_mant, (uint64_t)n * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(by_e.data(), d_exp, (uint64_t)n * 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    res->lnl = lnl;
    res->missing = counts[0];
    res->zero_sites = counts[1];
    res->mant.assign(n, 0.0);
    res->ex.assign(n, 0);
    for (uint32_t k = 0; k < M; k++) {
        if (!mnni_has_candidates(t, left, right, k)) continue;
        const uint32_t j = sc.slot_of[N + k] - sc.n_pad;
        for (uint32_t kind = 0; kind < 2u; kind++) {
            res->mant[2u * k + kind] = by_m[2u * j + kind];
            res->ex[2u * k + kind] = by_e[2u * j + kind];
        }
    }
    return PS_OK;
}

// a pass over a checked tree with x[K][N + M]
typedef std::function<int(const pars_tree &t, const uint32_t *left, const uint32_t *right, const double *x, mnni_result *res)> mnni_pass_fn;
// `body` run with the likelihood pass (tree_model.h) of a checked tree: what the branch-length optimiser is fed with
typedef std::function<int(const pars_tree &t, const uint32_t *left, const uint32_t *right, const std::function<int(const model_pass_fn &)> &body)>
    mnni_lengths_fn;

// what a search returns besides the summary (any may be null; the moves: the first move_cap)
struct mnni_outputs {
    uint32_t *left, *right;
    double *length, *round_lnl;
    uint32_t *move_round, *move_node, *move_kind;
    double *move_gain;
    uint64_t move_cap;
};

static int mnni_check_params(const ps_ml_nni_params *prm, const ps_ml_nni_t *out, const mnni_outputs &o)
{
    if (!prm || !out) return ps_fail(PS_ERR_INVALID, "null argument");
    if (prm->max_rounds < 1) return ps_fail(PS_ERR_INVALID, "max_rounds must be at least 1, not 0");
    if (!(prm->eps_gain > 0.0) || !std::isfinite(prm->eps_gain)) return ps_fail(PS_ERR_INVALID, "eps_gain must be a positive number, not %g", prm->eps_gain);
    if (o.move_cap && (!o.move_round || !o.move_node || !o.move_kind || !o.move_gain))
        return ps_fail(PS_ERR_INVALID, "move_cap = %llu needs the four move arrays", (unsigned long long)o.move_cap);
    return PS_OK;
}

// ln of a product
static double mnni_gain(double mant, int64_t ex) { return mant > 0.0 ? log(mant) + (double)ex * 0.6931471805599453094 : NAN; }

// The search loop of docs/LIKELIHOOD_SEARCH.md from a checked spanning tree and checked lengths
static int mnni_search(const char *call, const pars_tree &t0, const uint32_t *left0, const uint32_t *right0, const double *length0, const model_host &mh,
                       const ps_ml_nni_params &prm, uint64_t sites, const mnni_pass_fn &pass, const mnni_lengths_fn &with_lengths, ps_ml_nni_t *out,
                       const mnni_outputs &o)
{
    const uint32_t N = t0.N, M = t0.M, nodes = N + M;
    std::vector<double> used;
    uint64_t clamped = 0;
    PSCHK(lik_used_lengths(call, t0, length0, &used, &clamped));
    nni_topology top;
    nni_from_merges(N, left0, right0, &top);
    std::vector<uint32_t> left(M), right(M), nl(M), nr(M);
    std::vector<double> len(nodes), nlen(nodes), x, gain((size_t)2 * M), ngain((size_t)2 * M);
    nni_to_canonical_lengths(top, used.data(), left.data(), right.data(), len.data());
    uint64_t rounds = 0, passes = 0, length_passes = 0, rollbacks = 0, moves = 0, improving = 0;
    double start_lnl = 0.0;
    bool started = false;
    mnni_result res;
    // the lengths of a tree re-optimised (length_rounds > 0) in place, then one pass: res and gain[] are set
    auto evaluate = [&](const uint32_t *l, const uint32_t *r, std::vector<double> &tl, double *g) -> int {
        pars_tree tt;
        PSCHK(pars_check_tree(l, r, M, N, &tt));
        if (!started || prm.length_rounds)
            PSCHK(with_lengths(tt, l, r, [&](const model_pass_fn &mp) -> int {
                if (!started) {
                    model_result mr;
                    model_x(mh, tl, &x);
                    PSCHK(mp(x.data(), false, &mr));
                    length_passes++;
                    start_lnl = mr.lnl;
                    if (!std::isfinite(start_lnl))
                        return ps_fail(PS_ERR_INVALID, "%s: the start tree has lnL = %g under this model (a site of likelihood 0: an invariant class at a "
                                                       "variable site?): there is nothing to climb from", call, start_lnl);
                    started = true;
                }
                if (!prm.length_rounds) return PS_OK;
                const ps_ml_params ml = { prm.length_rounds, prm.eps_gain };
                ps_model_likelihood_t mo;
                std::vector<double> lo(nodes);
                PSCHK(model_optimise(call, tt, mh, l, r, tl.data(), sites, ml, mp, &mo, lo.data(), nullptr));
                length_passes += mo.passes;
                tl.swap(lo);
                return PS_OK;
            }));
        model_x(mh, tl, &x);
        PSCHK(pass(tt, l, r, x.data(), &res));
        passes++;
        for (size_t i = 0; i < (size_t)2 * M; i++) g[i] = mnni_gain(res.mant[i], res.ex[i]);
        return PS_OK;
    };
    PSCHK(evaluate(left.data(), right.data(), len, gain.data()));
    double lnl = res.lnl;
    uint64_t missing = res.missing, zero = res.zero_sites;
    if (o.round_lnl) o.round_lnl[0] = lnl;
    int optimum = 0;
    for (;;) {
        nni_from_merges(N, left.data(), right.data(), &top);
        std::vector<nni_gain_candidate> batch = nni_select_gains(top, gain.data(), prm.eps_gain, prm.moves_per_round, &improving);
        if (batch.empty()) {
            optimum = 1;
            break;
        }
        if (rounds == prm.max_rounds) break;
        for (;;) {
            nni_topology next = top;
            for (const nni_gain_candidate &c : batch) nni_apply_move(next, c.node, c.kind);
            nni_to_canonical_lengths(next, len.data(), nl.data(), nr.data(), nlen.data());
            PSCHK(evaluate(nl.data(), nr.data(), nlen, ngain.data()));
            // moves of one batch touch disjoint nodes but their gains need not add: never worse than the best move alone
            if (batch.size() == 1 || res.lnl >= lnl + batch[0].gain) break;
            rollbacks++;
            batch.resize(1);
        }
        if (!(res.lnl > lnl)) break;            // (a gain lost in the rounding of lnL: the tree stays, round_lnl ascends strictly)
        rounds++;
        for (const nni_gain_candidate &c : batch) {
            if (moves < o.move_cap) {
                o.move_round[moves] = (uint32_t)rounds;
                o.move_node[moves] = c.node;
                o.move_kind[moves] = c.kind;
                o.move_gain[moves] = c.gain;
            }
            moves++;
        }
        lnl = res.lnl;
        missing = res.missing;
        zero = res.zero_sites;
        left.swap(nl);
        right.swap(nr);
        len.swap(nlen);
        gain.swap(ngain);
        if (o.round_lnl) o.round_lnl[rounds] = lnl;
    }
    memset(out, 0, sizeof *out);
    out->pop_size = N;
    out->sites = sites;
    out->merges = M;
    out->rounds = rounds;
    out->passes = passes;
    out->length_passes = length_passes;
    out->rollbacks = rollbacks;
    out->moves = moves;
    out->local_optimum = (uint64_t)optimum;
    out->candidates_last = improving;
    out->zero_sites = zero;
    out->clamped_lengths = clamped;
    out->missing_cells = missing;
    out->start_lnl = start_lnl;
    out->lnl = lnl;
    if (o.left) memcpy(o.left, left.data(), (size_t)M * sizeof(uint32_t));
    if (o.right) memcpy(o.right, right.data(), (size_t)M * sizeof(uint32_t));
    if (o.length) memcpy(o.length, len.data(), (size_t)nodes * sizeof(double));
    return PS_OK;
}

// one pass on the list as given: *lnl, mant / ex[2 merges], *zero_sites (may be null)
static int mnni_deltas(const char *call, const pars_tree &t, const uint32_t *left, const uint32_t *right, const double *length, const model_host &mh,
                       const mnni_pass_fn &pass, double *lnl, double *delta_mant, int64_t *delta_exp, uint64_t *zero_sites)
{
    std::vector<double> used, x;
    uint64_t clamped = 0;
    PSCHK(lik_used_lengths(call, t, length, &used, &clamped));
    model_x(mh, used, &x);
    mnni_result res;
    PSCHK(pass(t, left, right, x.data(), &res));
    *lnl = res.lnl;
    memcpy(delta_mant, res.mant.data(), res.mant.size() * sizeof(double));
    memcpy(delta_exp, res.ex.data(), res.ex.size() * sizeof(int64_t));
    if (zero_sites) *zero_sites = res.zero_sites;
    return PS_OK;
}

extern "C" int ps_merges_canonical_lengths(const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges, uint64_t pop_size,
                                           uint32_t *out_left, uint32_t *out_right, double *length_out)
{
    if (!out_left || !out_right || !length || !length_out) return ps_fail(PS_ERR_INVALID, "null argument");
    pars_tree t;
    PSCHK(mnni_check_tree("ps_merges_canonical_lengths", left, right, merges, pop_size, &t));
    nni_topology top;
    nni_from_merges(t.N, left, right, &top);
    nni_to_canonical_lengths(top, length, out_left, out_right, length_out);
    return PS_OK;
}

extern "C" int ps_nni_apply_lengths(const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges, uint64_t pop_size, uint32_t node,
                                    uint32_t kind, uint32_t *out_left, uint32_t *out_right, double *length_out)
{
    if (!out_left || !out_right || !length || !length_out) return ps_fail(PS_ERR_INVALID, "null argument");
    pars_tree t;
    PSCHK(mnni_check_tree("ps_nni_apply_lengths", left, right, merges, pop_size, &t));
    if (kind > 1u) return ps_fail(PS_ERR_INVALID, "kind must be 0 or 1, not %u", kind);
    nni_topology top;
    nni_from_merges(t.N, left, right, &top);
    uint32_t touched[7];
    if (node < t.N || node >= t.N + t.M || !nni_touched(top, node, touched))
        return ps_fail(PS_ERR_INVALID, "node %u has no interchange in this tree (the root, its right child, its left child beside a leaf and "
                                       "the leaves have none)", node);
    nni_apply_move(top, node, kind);
    nni_to_canonical_lengths(top, length, out_left, out_right, length_out);
    return PS_OK;
}

static mnni_pass_fn mnni_rows_pass(const uint8_t *rows, uint64_t cols, const model_host &mh)
{
    return [=, &mh](const pars_tree &t, const uint32_t *l, const uint32_t *r, const double *x, mnni_result *res) -> int {
        mnni_host_pass(rows, cols, t, l, r, mh, mh.site_class, x, res);
        return PS_OK;
    };
}

extern "C" int ps_model_nni_deltas_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                             const double *length, uint64_t merges, const ps_subst_model *model, double *lnl, double *delta_mant,
                                             int64_t *delta_exp, uint64_t *zero_sites)
{
    const char *call = "ps_model_nni_deltas_from_rows";
    if (!lnl || !delta_mant || !delta_exp || (!rows && cols)) return ps_fail(PS_ERR_INVALID, "null argument");
    model_host mh;
    PSCHK(model_check(call, model, cols, &mh));
    pars_tree t;
    PSCHK(mnni_check_tree(call, left, right, merges, pop_size, &t));
    return mnni_deltas(call, t, left, right, length, mh, mnni_rows_pass(rows, cols, mh), lnl, delta_mant, delta_exp, zero_sites);
}

#define PS_MNNI_OUTPUTS { out_left, out_right, length_out, round_lnl, move_round, move_node, move_kind, move_gain, move_cap }

extern "C" int ps_model_nni_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                      const double *length_in, uint64_t merges, const ps_subst_model *model, const ps_ml_nni_params *prm,
                                      ps_ml_nni_t *out, uint32_t *out_left, uint32_t *out_right, double *length_out, double *round_lnl,
                                      uint32_t *move_round, uint32_t *move_node, uint32_t *move_kind, double *move_gain, uint64_t move_cap)
{
    const char *call = "ps_model_nni_from_rows";
    const mnni_outputs o = PS_MNNI_OUTPUTS;
    PSCHK(mnni_check_params(prm, out, o));
    if (!rows && cols) return ps_fail(PS_ERR_INVALID, "null argument");
    model_host mh;
    PSCHK(model_check(call, model, cols, &mh));
    pars_tree t;
    PSCHK(mnni_check_tree(call, left, right, merges, pop_size, &t));
    const mnni_lengths_fn with_lengths = [&](const pars_tree &tt, const uint32_t *l, const uint32_t *r,
                                             const std::function<int(const model_pass_fn &)> &body) -> int {
        return body(model_rows_pass(rows, cols, tt, l, r, mh));
    };
    return mnni_search(call, t, left, right, length_in, mh, *prm, cols, mnni_rows_pass(rows, cols, mh), with_lengths, out, o);
}

// What the device entries share, as model_device: m == nullptr: `core` answers for its own sites; else every shard's core handle
// does, and the products multiply in shard order.  global: site_class is indexed by the global site.
struct mnni_device {
    ps_multi *m;
    ps_population *core;
    const model_host &mh;
    bool global;
    std::vector<event_timer> tm;
    mnni_device(ps_multi *m_, ps_population *core_, const model_host &mh_, bool global_)
        : m(m_), core(core_), mh(mh_), global(global_), tm(m_ ? m_->shard.size() : 1) {}
    ps_population *handle(size_t k) const { return m ? m->shard[k]->core : core; }
    uint64_t sites() const { return m ? m->prm.core_size : core->cfg.ncols; }
    int begin()
    {
        if (m) PSCHK(ps_multi_sync(m));
        else {
            PSCHK(use_device(core));
            HIPCHK(hipStreamSynchronize(core->stream));
        }
        for (size_t k = 0; k < tm.size(); k++) handle(k)->ro[PS_RO_MODEL_NNI].timed = false;
        return PS_OK;
    }
    int pass(const pars_tree &t, const uint32_t *left, const uint32_t *right, const double *x, mnni_result *res)
    {
        const size_t S = tm.size();
        std::vector<mnni_result> part(S);
        auto shard_pass = [&](size_t k) -> int {
            ps_population *c = handle(k);
            const uint8_t *cls = mh.site_class ? mh.site_class + (global ? c->cfg.col_offset : 0) : nullptr;
            return mnni_device_pass(c, tm[k], t, left, right, mh, cls, x, &part[k]);
        };
        if (m) PSCHK(multi_for_each(m, shard_pass));
        else PSCHK(shard_pass(0));
        std::swap(*res, part[0]);
        for (size_t k = 1; k < S; k++) {
            res->lnl += part[k].lnl;
            res->missing += part[k].missing;
            res->zero_sites += part[k].zero_sites;
            for (size_t i = 0; i < res->mant.size(); i++) {
                if (!(res->mant[i] > 0.0)) continue;
                int32_t e2;
                res->mant[i] = ps_subst_prod(res->mant[i], part[k].mant[i], &e2);
                res->ex[i] += (int64_t)e2 + part[k].ex[i];
            }
        }
        return PS_OK;
    }
    // the likelihood passes of the branch-length optimiser on the same handles
    int with_lengths(const pars_tree &t, const uint32_t *left, const uint32_t *right, const std::function<int(const model_pass_fn &)> &body)
    {
        model_device dev(m, core, t, mh, left, right, global);
        PSCHK(dev.begin());
        PSCHK(body([&](const double *x, bool deriv, model_result *r) -> int { return dev.pass(x, deriv, r); }));
        return dev.end();
    }
    int end()
    {
        for (size_t k = 0; k < tm.size(); k++) {
            ps_population *c = handle(k);
            PSCHK(use_device(c));
            PSCHK(tm[k].collect(c->ro[PS_RO_MODEL_NNI], 3));
        }
        return use_device(core);
    }
};

static int mnni_deltas_run(const char *call, ps_multi *m, ps_population *core, bool global, const uint32_t *left, const uint32_t *right,
                           const double *length, uint64_t merges, const ps_subst_model *model, double *lnl, double *delta_mant, int64_t *delta_exp,
                           uint64_t *zero_sites)
{
    if (!lnl || !delta_mant || !delta_exp) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(lik_handle(core, call));
    model_host mh;
    PSCHK(model_check(call, model, model_class_sites(m, core, global), &mh));
    pars_tree t;
    PSCHK(mnni_check_tree(call, left, right, merges, core->cfg.pop_size, &t));
    std::vector<double> used;
    uint64_t clamped;
    PSCHK(lik_used_lengths(call, t, length, &used, &clamped));       // (an invalid length fails before any device work)
    mnni_device dev(m, core, mh, global);
    PSCHK(dev.begin());
    const mnni_pass_fn pass = [&](const pars_tree &tt, const uint32_t *l, const uint32_t *r, const double *x, mnni_result *res) -> int {
        return dev.pass(tt, l, r, x, res);
    };
    PSCHK(mnni_deltas(call, t, left, right, length, mh, pass, lnl, delta_mant, delta_exp, zero_sites));
    return dev.end();
}

static int mnni_run(const char *call, ps_multi *m, ps_population *core, bool global, const uint32_t *left, const uint32_t *right, const double *length_in,
                    uint64_t merges, const ps_subst_model *model, const ps_ml_nni_params *prm, ps_ml_nni_t *out, const mnni_outputs &o)
{
    PSCHK(mnni_check_params(prm, out, o));
    PSCHK(lik_handle(core, call));
    model_host mh;
    PSCHK(model_check(call, model, model_class_sites(m, core, global), &mh));
    pars_tree t;
    PSCHK(mnni_check_tree(call, left, right, merges, core->cfg.pop_size, &t));
    std::vector<double> used;
    uint64_t clamped;
    PSCHK(lik_used_lengths(call, t, length_in, &used, &clamped));
    mnni_device dev(m, core, mh, global);
    PSCHK(dev.begin());
    const mnni_pass_fn pass = [&](const pars_tree &tt, const uint32_t *l, const uint32_t *r, const double *x, mnni_result *res) -> int {
        return dev.pass(tt, l, r, x, res);
    };
    const mnni_lengths_fn with_lengths = [&](const pars_tree &tt, const uint32_t *l, const uint32_t *r,
                                             const std::function<int(const model_pass_fn &)> &body) -> int { return dev.with_lengths(tt, l, r, body); };
    PSCHK(mnni_search(call, t, left, right, length_in, mh, *prm, dev.sites(), pass, with_lengths, out, o));
    return dev.end();
}

extern "C" int ps_tree_model_nni_deltas(ps_population *core, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                        const ps_subst_model *model, double *lnl, double *delta_mant, int64_t *delta_exp, uint64_t *zero_sites)
{
    PSCHK(ps_needs_device());
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return mnni_deltas_run("ps_tree_model_nni_deltas", nullptr, core, false, left, right, length, merges, model, lnl, delta_mant, delta_exp, zero_sites);
}

extern "C" int ps_sim_tree_model_nni_deltas(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                            const ps_subst_model *model, double *lnl, double *delta_mant, int64_t *delta_exp, uint64_t *zero_sites)
{
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    return mnni_deltas_run("ps_sim_tree_model_nni_deltas", nullptr, s->core, true, left, right, length, merges, model, lnl, delta_mant, delta_exp,
                           zero_sites);
}

extern "C" int ps_multi_tree_model_nni_deltas(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                              const ps_subst_model *model, double *lnl, double *delta_mant, int64_t *delta_exp, uint64_t *zero_sites)
{
    PSCHK(ps_needs_device());
    if (!m) return ps_fail(PS_ERR_INVALID, "null argument");
    return mnni_deltas_run("ps_multi_tree_model_nni_deltas", m->shard.size() == 1 ? nullptr : m, m->shard[0]->core, true, left, right, length, merges,
                           model, lnl, delta_mant, delta_exp, zero_sites);
}

extern "C" int ps_tree_model_nni(ps_population *core, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                                 const ps_subst_model *model, const ps_ml_nni_params *prm, ps_ml_nni_t *out, uint32_t *out_left, uint32_t *out_right,
                                 double *length_out, double *round_lnl, uint32_t *move_round, uint32_t *move_node, uint32_t *move_kind,
                                 double *move_gain, uint64_t move_cap)
{
    PSCHK(ps_needs_device());
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return mnni_run("ps_tree_model_nni", nullptr, core, false, left, right, length_in, merges, model, prm, out, PS_MNNI_OUTPUTS);
}

extern "C" int ps_sim_tree_model_nni(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                                     const ps_subst_model *model, const ps_ml_nni_params *prm, ps_ml_nni_t *out, uint32_t *out_left,
                                     uint32_t *out_right, double *length_out, double *round_lnl, uint32_t *move_round, uint32_t *move_node,
                                     uint32_t *move_kind, double *move_gain, uint64_t move_cap)
{
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    return mnni_run("ps_sim_tree_model_nni", nullptr, s->core, true, left, right, length_in, merges, model, prm, out, PS_MNNI_OUTPUTS);
}

extern "C" int ps_multi_tree_model_nni(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                                       const ps_subst_model *model, const ps_ml_nni_params *prm, ps_ml_nni_t *out, uint32_t *out_left,
                                       uint32_t *out_right, double *length_out, double *round_lnl, uint32_t *move_round, uint32_t *move_node,
                                       uint32_t *move_kind, double *move_gain, uint64_t move_cap)
{
    PSCHK(ps_needs_device());
    if (!m) return ps_fail(PS_ERR_INVALID, "null argument");
    return mnni_run("ps_multi_tree_model_nni", m->shard.size() == 1 ? nullptr : m, m->shard[0]->core, true, left, right, length_in, merges, model, prm,
                    out, PS_MNNI_OUTPUTS);
}

#undef PS_MNNI_OUTPUTS

extern "C" int ps_tree_model_nni_timing(ps_population *core, double *schedule_ms, double *pass_ms, double *reduce_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_MODEL_NNI], "no likelihood tree search has been computed on this handle", { schedule_ms, pass_ms, reduce_ms });
}
