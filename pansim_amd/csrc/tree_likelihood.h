// tree_likelihood.h -- ps_tree_likelihood / ps_tree_ml_lengths with their ps_sim_ and ps_multi_ forms, the host restatements
// ps_likelihood_from_rows and ps_ml_lengths_from_rows, and the host rule ps_jc_lengths_from_changes (include/pansim_hip.h; the
// definitions: docs/TREE_LIKELIHOOD.md).  Included by pansim_capi.hip behind parsimony_search.h.
//
// One PASS gives lnL of a tree with branch lengths under Jukes-Cantor, optionally every site's (mantissa, exponent) and the
// derivative sums g, h of every branch: on the device tree_lik_kernel over the handle's sites on its stream (the schedule is
// tree_parsimony.h's; the sums come back per LDS slot and are mapped to nodes here), on the host the same jc_rule.h functions over
// rows, the sites in ascending order.  The evaluation (lik_evaluate) and the branch-length optimiser (lik_optimise) are one loop
// each over either kind of pass; a sharded run adds the shards' lnL, g and h in shard order before the one Newton step.
#pragma once

#include <functional>

#include "likelihood_kernels.h"

// The LDS of a pass: the leaf dwords (4 bytes per leaf), 36 bytes per merge, with derivatives 16 bytes of sums per slot -- and the
// schedule's copy behind them while the whole stays below 156 KiB (every tree of up to 1990 leaves has it; with derivatives a
// tree of 2048 leaves has it up to 1028 levels)
#define PS_LIK_LDS_SCHED (156u * 1024u)

static uint32_t lik_lds_bytes(uint32_t N, uint32_t levels, bool deriv, uint32_t *sched_lds)
{
    const uint32_t n_pad = (N + 15u) & ~15u, M = N - 1u, Mp = (M + 1u) & ~1u, slots = n_pad + M;
    const uint32_t base = n_pad * 4u + Mp * 36u + (deriv ? slots * 16u : 0u), sched = (M + levels + 1u) * 4u;
    *sched_lds = base + sched <= PS_LIK_LDS_SCHED ? 1u : 0u;
    return base + (*sched_lds ? sched : 0u);
}

static int lik_check_tree(const char *call, const uint32_t *left, const uint32_t *right, uint64_t merges, uint64_t pop_size, pars_tree *t)
{
    if (pop_size < 2 || pop_size > PS_LIK_MAX_POP)
        return ps_fail(PS_ERR_INVALID, "%s needs 2 <= pop_size <= %u (36 LDS bytes per node and 16 per branch), not %llu", call, PS_LIK_MAX_POP,
                       (unsigned long long)pop_size);
    if (merges != pop_size - 1)
        return ps_fail(PS_ERR_INVALID, "%s needs a spanning tree: %llu merges over %llu leaves, not %llu", call,
                       (unsigned long long)(pop_size - 1), (unsigned long long)pop_size, (unsigned long long)merges);
    return pars_check_tree(left, right, merges, pop_size, t);
}

// used[N + M] = the clamped lengths (the root's: 0), *clamped = how many entries the clamp changed
static int lik_used_lengths(const char *call, const pars_tree &t, const double *length, std::vector<double> *used, uint64_t *clamped)
{
    if (!length) return ps_fail(PS_ERR_INVALID, "null argument");
    const uint32_t nodes = t.N + t.M;
    used->assign(nodes, 0.0);
    *clamped = 0;
    for (uint32_t c = 0; c + 1u < nodes; c++) {
        if (!std::isfinite(length[c])) return ps_fail(PS_ERR_INVALID, "%s: the length of node %u is not a finite number", call, c);
        (*used)[c] = ps_jc_clamp(length[c]);
        *clamped += (*used)[c] != length[c];
    }
    return PS_OK;
}

// what one pass returns: mant / ex of every site (null: not asked for), g / h of every node (deriv only), lnL and the missing cells
struct lik_result {
    double *mant = nullptr;
    int32_t *ex = nullptr;
    std::vector<double> g, h;
    double lnl = 0.0;
    uint64_t missing = 0;
};

// a pass over the tree with x[N + M] (the root's entry is not read)
typedef std::function<int(const double *x, bool deriv, lik_result *res)> lik_pass_fn;

// One pass on the host over individual-major rows, the sites in ascending order
static void lik_host_pass(const uint8_t *rows, uint64_t cols, const pars_tree &t, const uint32_t *left, const uint32_t *right, const double *x,
                          bool deriv, lik_result *res)
{
    const uint32_t N = t.N, M = t.M, nodes = N + M;
    std::vector<double> L((size_t)4 * nodes), U((size_t)4 * nodes);
    std::vector<int32_t> E(nodes, 0);
    res->g.assign(deriv ? nodes : 0, 0.0);
    res->h.assign(deriv ? nodes : 0, 0.0);
    res->lnl = 0.0;
    res->missing = 0;
    for (uint64_t s = 0; s < cols; s++) {
        for (uint32_t i = 0; i < N; i++) {
            const uint8_t b = rows[(uint64_t)i * cols + s];
            ps_jc_leaf(b, &L[4u * i]);
            res->missing += !ps_jc_known(b);
        }
        for (uint32_t k = 0; k < M; k++) {
            const uint32_t l = left[k], r = right[k];
            double ml[4], mr[4];
            ps_jc_message(x[l], &L[4u * l], ml);
            ps_jc_message(x[r], &L[4u * r], mr);
            E[N + k] = (E[l] + E[r]) + ps_jc_join(ml, mr, &L[4u * (N + k)]);
        }
        const double mant = ps_jc_site(&L[4u * (nodes - 1u)]);
        if (res->mant) res->mant[s] = mant;
        if (res->ex) res->ex[s] = E[nodes - 1u];
        res->lnl += ps_jc_site_ln(mant, E[nodes - 1u]);
        if (!deriv) continue;
        for (uint32_t k = M; k-- > 0;) {
            const uint32_t l = left[k], r = right[k], c = N + k;
            double T[4] = { 1.0, 1.0, 1.0, 1.0 }, ml[4], mr[4];
            if (k != M - 1u) ps_jc_message(x[c], &U[4u * c], T);
            ps_jc_message(x[l], &L[4u * l], ml);
            ps_jc_message(x[r], &L[4u * r], mr);
            (void)ps_jc_join(mr, T, &U[4u * l]);
            (void)ps_jc_join(ml, T, &U[4u * r]);
            const double ra = ps_jc_ratio(x[l], &U[4u * l], &L[4u * l]), rb = ps_jc_ratio(x[r], &U[4u * r], &L[4u * r]);
            res->g[l] += ra;
            res->h[l] += ra * ra;
            res->g[r] += rb;
            res->h[r] += rb * rb;
        }
    }
}

// One pass of handle p over its own sites on its stream, complete when it returns.  res->mant / res->ex: of p's own sites.  Timer
// groups: 0 the uploads, 1 the kernel, 2 the sum of the workgroups' rows.
static int lik_device_pass(ps_population *p, event_timer &tm, const pars_tree &t, const uint32_t *left, const uint32_t *right, const double *x,
                           bool deriv, lik_result *res)
{
    const uint32_t N = t.N, M = t.M, nodes = N + M, rows = (uint32_t)p->cfg.ncols;
    PSCHK(use_device(p));
    const uint32_t *slot = nullptr;
    PSCHK(rows_current(p, &slot));
    pars_schedule sc;
    pars_make_schedule(t, left, right, slot, &sc);
    const uint32_t slots = sc.n_pad + M, stride = deriv ? 2u * slots + 1u : 1u;
    std::vector<double> xs(slots, 1.0);
    for (uint32_t c = 0; c + 1u < nodes; c++) xs[sc.slot_of[c]] = x[c];
    uint32_t sched_lds = 0;
    const uint32_t lds = lik_lds_bytes(N, t.levels, deriv, &sched_lds);
    const uint32_t threads = N <= 1024u ? 64u : 256u;
    const uint32_t per_cu = std::max(1u, std::min(8u, (160u * 1024u) / (lds + 1024u)));
    const uint32_t grid = std::max(1u, std::min((rows + 3u) / 4u, 256u * per_cu));
    scratch_layout lay;
    const uint64_t o_miss = lay.add(8, 16), o_out = lay.add((uint64_t)stride * 8, 16);
    const uint64_t o_sched = lay.add((uint64_t)M * 4, 16), o_off = lay.add((uint64_t)sc.level_off.size() * 4, 16);
    const uint64_t o_x = lay.add((uint64_t)slots * 8, 16);
    const uint64_t o_mant = lay.add(res->mant ? (uint64_t)rows * 8 : 0, 16), o_exp = lay.add(res->ex ? (uint64_t)rows * 4 : 0, 16);
    const uint64_t o_part = lay.add((uint64_t)grid * stride * 8, 16);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(p->ro[PS_RO_LIK], lay.bytes, &base, "cannot allocate the %llu bytes of the schedule and the sums of the likelihood of a tree of %u merges over %u sites",
                      M, rows));
    hipStream_t st = p->stream;
    unsigned long long *d_miss = (unsigned long long *)(base + o_miss);
    double *d_out = (double *)(base + o_out), *d_x = (double *)(base + o_x), *d_part = (double *)(base + o_part);
    uint32_t *d_sched = (uint32_t *)(base + o_sched), *d_off = (uint32_t *)(base + o_off);
    double *d_mant = res->mant ? (double *)(base + o_mant) : nullptr;
    int32_t *d_exp = res->ex ? (int32_t *)(base + o_exp) : nullptr;
    // (the sources of the three copies live until this function's last synchronisation)
    PSCHK(tm.timed(0, st, [&]() -> int {
        HIPCHK(hipMemsetAsync(d_miss, 0, o_sched, st));
        HIPCHK(hipMemcpyAsync(d_sched, sc.sched.data(), (uint64_t)M * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_off, sc.level_off.data(), (uint64_t)sc.level_off.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_x, xs.data(), (uint64_t)slots * 8, hipMemcpyHostToDevice, st));
        return PS_OK;
    }));
    if (rows) {
        auto kern = deriv ? tree_lik_kernel<true> : tree_lik_kernel<false>;
        if (lds > 32768u) HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        PSCHK(tm.timed(1, st, [&]() -> int {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, (const uint8_t *)p->state, p->pitch, N, rows, (const uint32_t *)d_sched,
                               (const uint32_t *)d_off, t.levels, M, sc.n_pad, (const double *)d_x, sched_lds, d_mant, d_exp, 0u, d_part, stride,
                               d_miss);
            HIPCHK(hipGetLastError());
            return PS_OK;
        }));
        PSCHK(tm.timed(2, st, [&]() -> int {
            hipLaunchKernelGGL(lik_reduce_kernel, dim3((stride + 255u) / 256u), dim3(256), 0, st, (const double *)d_part, grid, stride, d_out);
            HIPCHK(hipGetLastError());
            return PS_OK;
        }));
    }
    unsigned long long miss = 0;
    std::vector<double> out(stride);
    HIPCHK(hipMemcpyAsync(&miss, d_miss, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out.data(), d_out, (uint64_t)stride * 8, hipMemcpyDeviceToHost, st));
    if (rows && res->mant) HIPCHK(hipMemcpyAsync(res->mant, d_mant, (uint64_t)rows * 8, hipMemcpyDeviceToHost, st));
    if (rows && res->ex) HIPCHK(hipMemcpyAsync(res->ex, d_exp, (uint64_t)rows * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    res->lnl = out[stride - 1u];
    res->missing = miss;
    res->g.assign(deriv ? nodes : 0, 0.0);
    res->h.assign(deriv ? nodes : 0, 0.0);
    if (deriv)
        for (uint32_t c = 0; c + 1u < nodes; c++) {
            res->g[c] = out[sc.slot_of[c]];
            res->h[c] = out[(size_t)slots + sc.slot_of[c]];
        }
    return PS_OK;
}

static void lik_summary(ps_likelihood_t *o, const pars_tree &t, uint64_t sites, uint64_t clamped, uint64_t missing, const std::vector<double> &used)
{
    memset(o, 0, sizeof *o);
    o->pop_size = t.N;
    o->sites = sites;
    o->merges = t.M;
    o->clamped_lengths = clamped;
    o->missing_cells = missing;
    double sum = 0.0;
    for (uint32_t c = 0; c + 1u < t.N + t.M; c++) sum += used[c];
    o->tree_length = sum;
}

static void lik_x(const std::vector<double> &used, std::vector<double> *x)
{
    x->assign(used.size(), 1.0);
    for (size_t c = 0; c + 1u < used.size(); c++) (*x)[c] = ps_jc_x(used[c]);
}

// lnL of the tree with the lengths as given (clamped), one pass
static int lik_evaluate(const char *call, const pars_tree &t, const double *length, uint64_t sites, const lik_pass_fn &pass, ps_likelihood_t *out,
                        double *site_mant, int32_t *site_exp, double *branch_g, double *branch_h)
{
    std::vector<double> used, x;
    uint64_t clamped = 0;
    PSCHK(lik_used_lengths(call, t, length, &used, &clamped));
    lik_x(used, &x);
    lik_result res;
    res.mant = site_mant;
    res.ex = site_exp;
    const bool deriv = branch_g || branch_h;
    PSCHK(pass(x.data(), deriv, &res));
    lik_summary(out, t, sites, clamped, res.missing, used);
    out->passes = 1;
    out->lnl = out->start_lnl = res.lnl;
    if (branch_g) memcpy(branch_g, res.g.data(), res.g.size() * sizeof(double));
    if (branch_h) memcpy(branch_h, res.h.data(), res.h.size() * sizeof(double));
    return PS_OK;
}

static int lik_check_ml(const ps_ml_params *prm, const ps_likelihood_t *out, const double *round_lnl, uint64_t round_cap)
{
    if (!prm || !out) return ps_fail(PS_ERR_INVALID, "null argument");
    if (prm->max_rounds < 1) return ps_fail(PS_ERR_INVALID, "max_rounds must be at least 1, not 0");
    if (!(prm->eps_lnl > 0.0) || !std::isfinite(prm->eps_lnl)) return ps_fail(PS_ERR_INVALID, "eps_lnl must be a positive number, not %g", prm->eps_lnl);
    if (round_lnl && round_cap < (uint64_t)prm->max_rounds + 1u)
        return ps_fail(PS_ERR_INVALID, "round_lnl needs max_rounds + 1 = %llu values, round_cap is %llu", (unsigned long long)prm->max_rounds + 1u,
                       (unsigned long long)round_cap);
    return PS_OK;
}

// The optimiser of docs/TREE_LIKELIHOOD.md from a checked spanning tree
static int lik_optimise(const char *call, const pars_tree &t, const uint32_t *left, const uint32_t *right, const double *length, uint64_t sites,
                        const ps_ml_params &prm, const lik_pass_fn &pass, ps_likelihood_t *out, double *length_out, double *round_lnl)
{
    const uint32_t nodes = t.N + t.M, root = nodes - 1u, rl = left[t.M - 1u], rr = right[t.M - 1u];
    std::vector<double> used, x, cand, cx;
    uint64_t clamped = 0;
    PSCHK(lik_used_lengths(call, t, length, &used, &clamped));
    // only the sum of the two root branches is identified: whole above the left child, the right held at the lower bound
    used[rl] = ps_jc_clamp(used[rl] + used[rr]);
    used[rr] = PS_LIK_MIN_LENGTH;
    lik_x(used, &x);
    lik_result cur, next;
    PSCHK(pass(x.data(), true, &cur));
    uint64_t rounds = 0, passes = 1, rollbacks = 0, converged = 0;
    const double start = cur.lnl;
    if (round_lnl) round_lnl[0] = cur.lnl;
    double lambda = 1.0;
    while (rounds < prm.max_rounds && lambda >= 0x1p-20) {
        cand = used;
        for (uint32_t c = 0; c < root; c++)
            if (c != rr) cand[c] = ps_jc_newton(used[c], x[c], cur.g[c], cur.h[c], lambda);
        lik_x(cand, &cx);
        PSCHK(pass(cx.data(), true, &next));
        passes++;
        if (next.lnl < cur.lnl) {
            rollbacks++;
            lambda *= 0.5;
            continue;
        }
        if (next.lnl == cur.lnl) {           // (no gain at all: the lengths stay, nothing is recorded)
            converged = 1;
            break;
        }
        const double gain = next.lnl - cur.lnl;
        rounds++;
        used.swap(cand);
        x.swap(cx);
        std::swap(cur, next);
        if (round_lnl) round_lnl[rounds] = cur.lnl;
        lambda = 1.0;
        if (gain < prm.eps_lnl) {
            converged = 1;
            break;
        }
    }
    lik_summary(out, t, sites, clamped, cur.missing, used);
    out->rounds = rounds;
    out->passes = passes;
    out->rollbacks = rollbacks;
    out->converged = converged;
    out->lnl = cur.lnl;
    out->start_lnl = start;
    if (length_out) memcpy(length_out, used.data(), (size_t)nodes * sizeof(double));
    return PS_OK;
}

extern "C" int ps_jc_lengths_from_changes(const uint64_t *branch_changes, uint64_t nodes, uint64_t sites, double *length)
{
    if (nodes && (!branch_changes || !length)) return ps_fail(PS_ERR_INVALID, "null argument");
    for (uint64_t c = 0; c < nodes; c++) length[c] = ps_jc_length_from_changes(branch_changes[c], sites);
    return PS_OK;
}

static lik_pass_fn lik_rows_pass(const uint8_t *rows, uint64_t cols, const pars_tree &t, const uint32_t *left, const uint32_t *right)
{
    return [=, &t](const double *x, bool deriv, lik_result *res) -> int {
        lik_host_pass(rows, cols, t, left, right, x, deriv, res);
        return PS_OK;
    };
}

extern "C" int ps_likelihood_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                       const double *length, uint64_t merges, ps_likelihood_t *out, double *site_mant, int32_t *site_exp,
                                       double *branch_g, double *branch_h)
{
    if (!out || (!rows && cols)) return ps_fail(PS_ERR_INVALID, "null argument");
    pars_tree t;
    PSCHK(lik_check_tree("ps_likelihood_from_rows", left, right, merges, pop_size, &t));
    return lik_evaluate("ps_likelihood_from_rows", t, length, cols, lik_rows_pass(rows, cols, t, left, right), out, site_mant, site_exp, branch_g,
                        branch_h);
}

extern "C" int ps_ml_lengths_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                       const double *length_in, uint64_t merges, const ps_ml_params *prm, ps_likelihood_t *out,
                                       double *length_out, double *round_lnl, uint64_t round_cap)
{
    PSCHK(lik_check_ml(prm, out, round_lnl, round_cap));
    if (!rows && cols) return ps_fail(PS_ERR_INVALID, "null argument");
    pars_tree t;
    PSCHK(lik_check_tree("ps_ml_lengths_from_rows", left, right, merges, pop_size, &t));
    return lik_optimise("ps_ml_lengths_from_rows", t, left, right, length_in, cols, *prm, lik_rows_pass(rows, cols, t, left, right), out, length_out,
                        round_lnl);
}

// What the device entries share.  m == nullptr: `core` answers for its own sites; else every shard's core handle does, the
// per-site arrays land at the shard's offset and lnL, g, h add in shard order.  Everything queued on the handle (the run)
// precedes the passes; the timers are collected when the call ends.
struct lik_device {
    ps_multi *m;
    ps_population *core;
    const pars_tree &t;
    const uint32_t *left, *right;
    std::vector<event_timer> tm;
    lik_device(ps_multi *m_, ps_population *core_, const pars_tree &t_, const uint32_t *l, const uint32_t *r)
        : m(m_), core(core_), t(t_), left(l), right(r), tm(m_ ? m_->shard.size() : 1) {}
    ps_population *handle(size_t k) const { return m ? m->shard[k]->core : core; }
    uint64_t sites() const { return m ? m->prm.core_size : core->cfg.ncols; }
    int begin()
    {
        if (m) PSCHK(ps_multi_sync(m));
        else {
            PSCHK(use_device(core));
            HIPCHK(hipStreamSynchronize(core->stream));
        }
        for (size_t k = 0; k < tm.size(); k++) handle(k)->ro[PS_RO_LIK].timed = false;
        return PS_OK;
    }
    int pass(const double *x, bool deriv, lik_result *res)
    {
        const size_t S = tm.size();
        std::vector<lik_result> part(S);
        auto shard_pass = [&](size_t k) -> int {
            ps_population *c = handle(k);
            const uint64_t off = m ? c->cfg.col_offset : 0;
            part[k].mant = res->mant ? res->mant + off : nullptr;
            part[k].ex = res->ex ? res->ex + off : nullptr;
            return lik_device_pass(c, tm[k], t, left, right, x, deriv, &part[k]);
        };
        if (m) PSCHK(multi_for_each(m, shard_pass));
        else PSCHK(shard_pass(0));
        res->g.swap(part[0].g);
        res->h.swap(part[0].h);
        res->lnl = part[0].lnl;
        res->missing = part[0].missing;
        for (size_t k = 1; k < S; k++) {
            res->lnl += part[k].lnl;
            res->missing += part[k].missing;
            for (size_t c = 0; c < res->g.size(); c++) {
                res->g[c] += part[k].g[c];
                res->h[c] += part[k].h[c];
            }
        }
        return PS_OK;
    }
    int end()
    {
        for (size_t k = 0; k < tm.size(); k++) {
            ps_population *c = handle(k);
            PSCHK(use_device(c));
            PSCHK(tm[k].collect(c->ro[PS_RO_LIK], 3));
        }
        return use_device(core);
    }
};

static int lik_handle(const ps_population *core, const char *call)
{
    if (!core->cfg.core) return ps_fail(PS_ERR_INVALID, "%s takes a core handle: the likelihood is over core sites", call);
    return PS_OK;
}

static int lik_run(ps_multi *m, ps_population *core, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                   ps_likelihood_t *out, double *site_mant, int32_t *site_exp, double *branch_g, double *branch_h)
{
    const char *call = m ? "ps_multi_tree_likelihood" : "ps_tree_likelihood";
    if (!out) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(lik_handle(core, call));
    pars_tree t;
    PSCHK(lik_check_tree(call, left, right, merges, core->cfg.pop_size, &t));
    lik_device dev(m, core, t, left, right);
    std::vector<double> used;
    uint64_t clamped;
    PSCHK(lik_used_lengths(call, t, length, &used, &clamped));       // (an invalid length fails before any device work)
    PSCHK(dev.begin());
    const lik_pass_fn pass = [&](const double *x, bool deriv, lik_result *res) -> int { return dev.pass(x, deriv, res); };
    PSCHK(lik_evaluate(call, t, length, dev.sites(), pass, out, site_mant, site_exp, branch_g, branch_h));
    return dev.end();
}

static int lik_ml_run(ps_multi *m, ps_population *core, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                      const ps_ml_params *prm, ps_likelihood_t *out, double *length_out, double *round_lnl, uint64_t round_cap)
{
    const char *call = m ? "ps_multi_tree_ml_lengths" : "ps_tree_ml_lengths";
    PSCHK(lik_check_ml(prm, out, round_lnl, round_cap));
    PSCHK(lik_handle(core, call));
    pars_tree t;
    PSCHK(lik_check_tree(call, left, right, merges, core->cfg.pop_size, &t));
    lik_device dev(m, core, t, left, right);
    std::vector<double> used;
    uint64_t clamped;
    PSCHK(lik_used_lengths(call, t, length_in, &used, &clamped));
    PSCHK(dev.begin());
    const lik_pass_fn pass = [&](const double *x, bool deriv, lik_result *res) -> int { return dev.pass(x, deriv, res); };
    PSCHK(lik_optimise(call, t, left, right, length_in, dev.sites(), *prm, pass, out, length_out, round_lnl));
    return dev.end();
}

extern "C" int ps_tree_likelihood(ps_population *core, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                  ps_likelihood_t *out, double *site_mant, int32_t *site_exp, double *branch_g, double *branch_h)
{
    PSCHK(ps_needs_device());
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return lik_run(nullptr, core, left, right, length, merges, out, site_mant, site_exp, branch_g, branch_h);
}

extern "C" int ps_sim_tree_likelihood(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                      ps_likelihood_t *out, double *site_mant, int32_t *site_exp, double *branch_g, double *branch_h)
{
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    return lik_run(nullptr, s->core, left, right, length, merges, out, site_mant, site_exp, branch_g, branch_h);
}

extern "C" int ps_multi_tree_likelihood(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                        ps_likelihood_t *out, double *site_mant, int32_t *site_exp, double *branch_g, double *branch_h)
{
    PSCHK(ps_needs_device());
    if (!m) return ps_fail(PS_ERR_INVALID, "null argument");
    return lik_run(m->shard.size() == 1 ? nullptr : m, m->shard[0]->core, left, right, length, merges, out, site_mant, site_exp, branch_g, branch_h);
}

extern "C" int ps_tree_ml_lengths(ps_population *core, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                                  const ps_ml_params *prm, ps_likelihood_t *out, double *length_out, double *round_lnl, uint64_t round_cap)
{
    PSCHK(ps_needs_device());
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return lik_ml_run(nullptr, core, left, right, length_in, merges, prm, out, length_out, round_lnl, round_cap);
}

extern "C" int ps_sim_tree_ml_lengths(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                                      const ps_ml_params *prm, ps_likelihood_t *out, double *length_out, double *round_lnl, uint64_t round_cap)
{
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    return lik_ml_run(nullptr, s->core, left, right, length_in, merges, prm, out, length_out, round_lnl, round_cap);
}

extern "C" int ps_multi_tree_ml_lengths(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                                        const ps_ml_params *prm, ps_likelihood_t *out, double *length_out, double *round_lnl, uint64_t round_cap)
{
    PSCHK(ps_needs_device());
    if (!m) return ps_fail(PS_ERR_INVALID, "null argument");
    return lik_ml_run(m->shard.size() == 1 ? nullptr : m, m->shard[0]->core, left, right, length_in, merges, prm, out, length_out, round_lnl,
                      round_cap);
}

extern "C" int ps_tree_likelihood_timing(ps_population *core, double *schedule_ms, double *pass_ms, double *reduce_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_LIK], "no tree likelihood has been computed on this handle", { schedule_ms, pass_ms, reduce_ms });
}
