// ancestral_states.h -- ps_tree_ancestral_states with its ps_sim_ and ps_multi_ forms, ps_ancestral_states_timing and the host
// restatement ps_ancestral_from_rows (include/pansim_hip.h; the definitions: docs/ANCESTRAL_STATES.md).  Included by
// pansim_capi.hip behind tree_model.h, whose model and length checks, x table and schedule it shares, and behind
// isolate_samples.h, whose sample_make shapes the new handle.
//
// One PASS gives the marginal reconstruction of every inner node of a tree with branch lengths under ps_subst_model: on the device
// tree_anc_kernel over the handle's sites on its stream, writing the site rows of a new ps_population of merges rows; on the host
// the same subst_rule.h functions over rows, the sites in ascending order.  A sharded run writes every shard's block of site rows
// into one whole handle on shard 0's device and adds the shards' sums on the host in shard order.
#pragma once

#include "anc_kernels.h"

static_assert(PS_ANC_MAX_POP == PS_ANC_KERNEL_MAX_POP && PS_ANC_MAX_POP_MIX == PS_ANC_KERNEL_MAX_POP_MIX, "the limits of the header are the kernel's");

// what one pass returns: node_conf of every merge, branch_diff of every node (the root's 0), lnL and the counters
struct anc_result {
    std::vector<double> conf, diff;
    double lnl = 0.0;
    uint64_t missing = 0, masked = 0, zero = 0;
};

static bool anc_mixture(const model_host &mh) { return !mh.site_class && mh.K() > 1u; }

static int anc_check_tree(const char *call, const uint32_t *left, const uint32_t *right, uint64_t merges, uint64_t pop_size, const model_host &mh,
                          pars_tree *t)
{
    const bool mix = anc_mixture(mh);
    const uint32_t cap = mix ? PS_ANC_MAX_POP_MIX : PS_ANC_MAX_POP;
    if (pop_size < 2 || pop_size > cap)
        return ps_fail(PS_ERR_INVALID, "%s needs 2 <= pop_size <= %s = %u (12 LDS bytes per leaf and %u per merge), not %llu", call,
                       mix ? "PS_ANC_MAX_POP_MIX" : "PS_ANC_MAX_POP", cap, mix ? 88u : 56u, (unsigned long long)pop_size);
    if (merges != pop_size - 1)
        return ps_fail(PS_ERR_INVALID, "%s needs a spanning tree: %llu merges over %llu leaves, not %llu", call,
                       (unsigned long long)(pop_size - 1), (unsigned long long)pop_size, (unsigned long long)merges);
    return pars_check_tree(left, right, merges, pop_size, t);
}

static int anc_check_min(const char *call, double min_posterior)
{
    if (!(min_posterior >= 0.0 && min_posterior <= 1.0))
        return ps_fail(PS_ERR_INVALID, "%s: min_posterior must be a number in [0, 1], not %g", call, min_posterior);
    return PS_OK;
}

// The LDS of a pass (anc_kernels.h): 12 bytes per leaf, 56 per merge, a mixture 32 more per merge; the copies of the schedule and
// of node_of behind them while the whole stays within PS_LIK_LDS_SCHED
static uint32_t anc_lds_bytes(uint32_t N, uint32_t levels, bool mix, uint32_t *sched_lds)
{
    const uint32_t n_pad = (N + 15u) & ~15u, M = N - 1u, Mp = (M + 1u) & ~1u;
    const uint32_t base = n_pad * 12u + Mp * 36u + M * 20u + (mix ? M * 32u : 0u), sched = (2u * M + levels + 1u) * 4u;
    *sched_lds = base + sched <= PS_LIK_LDS_SCHED ? 1u : 0u;
    return base + (*sched_lds ? sched : 0u);
}

// One pass on the host over individual-major rows, the sites in ascending order.  cls: the class of site 0 on (null: none);
// anc_rows (null: not stored): merges x cols bytes, row k = node N + k
static void anc_host_pass(const uint8_t *rows, uint64_t cols, const pars_tree &t, const uint32_t *left, const uint32_t *right, const model_host &mh,
                          const uint8_t *cls, const double *x, double min_post, uint8_t *anc_rows, anc_result *res)
{
    const uint32_t N = t.N, M = t.M, nodes = N + M, K = mh.K();
    const double *pi = mh.a.freq, *rho = mh.a.root;
    std::vector<double> L((size_t)K * 4 * nodes), U((size_t)4 * nodes), acc((size_t)4 * M, 0.0);
    std::vector<int32_t> E((size_t)K * nodes, 0);
    res->conf.assign(M, 0.0);
    res->diff.assign(nodes, 0.0);
    res->lnl = 0.0;
    res->missing = res->masked = res->zero = 0;
    const bool assigned = cls || K == 1u;
    for (uint64_t s = 0; s < cols; s++) {
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
        if (anc_rows)
            for (uint32_t j = 0; j < M; j++) anc_rows[(uint64_t)j * cols + s] = 0;
        if (!(sm > 0.0)) {
            res->zero++;
            continue;
        }
        for (uint32_t k = kb; k < ke; k++) {
            const double *Lk = &L[(size_t)k * 4 * nodes], *xk = x + (size_t)k * nodes;
            const bool first = k == kb, last = k + 1u == ke;
            for (uint32_t j = M; j-- > 0;) {
                const uint32_t l = left[j], r = right[j], c = N + j;
                double T[4] = { rho[0], rho[1], rho[2], rho[3] }, ml[4], mr[4], w[4], p[4];
                if (j != M - 1u) ps_subst_down(xk[c], pi, &U[4u * c], T);
                ps_subst_up(xk[l], pi, &Lk[4u * l], ml);
                ps_subst_up(xk[r], pi, &Lk[4u * r], mr);
                const double sum = ps_subst_node_post(T, ml, mr, w);
                (void)ps_jc_join(mr, T, &U[4u * l]);
                (void)ps_jc_join(ml, T, &U[4u * r]);
                res->diff[l] += post[k] * ps_subst_pdiff(xk[l], pi, &U[4u * l], &Lk[4u * l]);
                res->diff[r] += post[k] * ps_subst_pdiff(xk[r], pi, &U[4u * r], &Lk[4u * r]);
                for (uint32_t a = 0; a < 4u; a++) {
                    p[a] = ps_subst_post_term(post[k], w[a], sum);
                    if (!first) p[a] = acc[4u * j + a] + p[a];
                    acc[4u * j + a] = p[a];
                }
                if (!last) continue;
                double pmax;
                const uint32_t best = ps_subst_map(p, &pmax);
                res->conf[j] += pmax;
                if (pmax < min_post) res->masked++;
                else if (anc_rows) anc_rows[(uint64_t)j * cols + s] = (uint8_t)(1u << best);
            }
        }
    }
}

// One pass of handle p over its own sites on its stream, complete when it returns.  cls: the classes of p's own sites (null: none).
// dst (null: no matrix): where the site rows of p's sites go, pitch_out bytes apart, on device dst_device.  Timer groups: 0 the
// uploads, 1 the kernel (and the copy to another device), 2 the sum of the workgroups' rows.
static int anc_device_pass(ps_population *p, event_timer &tm, const pars_tree &t, const uint32_t *left, const uint32_t *right, const model_host &mh,
                           const uint8_t *cls, const double *x, double min_post, uint8_t *dst, uint32_t pitch_out, int dst_device, anc_result *res)
{
    const uint32_t N = t.N, M = t.M, nodes = N + M, rows = (uint32_t)p->cfg.ncols, K = mh.K();
    const bool mix = anc_mixture(mh);
    PSCHK(use_device(p));
    const uint32_t *slot = nullptr;
    PSCHK(rows_current(p, &slot));
    pars_schedule sc;
    pars_make_schedule(t, left, right, slot, &sc);
    const uint32_t slots = sc.n_pad + M, stride = slots + M + 1u;
    std::vector<double> xs((size_t)K * slots, 1.0);
    for (uint32_t k = 0; k < K; k++)
        for (uint32_t c = 0; c + 1u < nodes; c++) xs[(size_t)k * slots + sc.slot_of[c]] = x[(size_t)k * nodes + c];
    std::vector<uint32_t> node_of(M);
    for (uint32_t k = 0; k < M; k++) node_of[sc.slot_of[N + k] - sc.n_pad] = k;
    uint32_t sched_lds = 0;
    const uint32_t lds = anc_lds_bytes(N, t.levels, mix, &sched_lds);
    const uint32_t threads = N <= 1024u ? 64u : 256u;
    const uint32_t per_cu = std::max(1u, std::min(8u, (160u * 1024u) / (lds + 1024u + 512u)));
    const uint32_t grid = std::max(1u, std::min((rows + 3u) / 4u, 256u * per_cu));
    scratch_layout lay;
    const uint64_t o_cnt = lay.add(24, 16), o_out = lay.add((uint64_t)stride * 8, 16);
    const uint64_t o_sched = lay.add((uint64_t)M * 4, 16), o_off = lay.add((uint64_t)sc.level_off.size() * 4, 16);
    const uint64_t o_node = lay.add((uint64_t)M * 4, 16);
    const uint64_t o_x = lay.add((uint64_t)K * slots * 8, 16), o_cls = lay.add(cls ? (uint64_t)rows : 0, 16);
    const uint64_t o_part = lay.add((uint64_t)grid * stride * 8, 16);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(p->ro[PS_RO_ANC], lay.bytes, &base,
                      "cannot allocate the %llu bytes of the schedule, the x table and the sums of the ancestral states of a tree of %u merges over %u sites", M,
                      rows));
    dev_tmp<uint8_t> stage;
    uint8_t *d_dst = dst;
    if (dst && rows && p->device != dst_device) {
        PSCHK(stage.alloc((uint64_t)rows * pitch_out));
        d_dst = stage.p;
    }
    hipStream_t st = p->stream;
    unsigned long long *d_cnt = (unsigned long long *)(base + o_cnt);
    double *d_out = (double *)(base + o_out), *d_x = (double *)(base + o_x), *d_part = (double *)(base + o_part);
    uint32_t *d_sched = (uint32_t *)(base + o_sched), *d_off = (uint32_t *)(base + o_off), *d_node = (uint32_t *)(base + o_node);
    uint8_t *d_cls = cls && rows ? base + o_cls : nullptr;
    // (the sources of the copies live until this function's last synchronisation)
    PSCHK(tm.timed(0, st, [&]() -> int {
        HIPCHK(hipMemsetAsync(d_cnt, 0, o_sched, st));
        HIPCHK(hipMemcpyAsync(d_sched, sc.sched.data(), (uint64_t)M * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_off, sc.level_off.data(), (uint64_t)sc.level_off.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_node, node_of.data(), (uint64_t)M * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_x, xs.data(), (uint64_t)K * slots * 8, hipMemcpyHostToDevice, st));
        if (d_cls) HIPCHK(hipMemcpyAsync(d_cls, cls, rows, hipMemcpyHostToDevice, st));
        return PS_OK;
    }));
    if (rows) {
        auto kern = mix ? tree_anc_kernel<true> : tree_anc_kernel<false>;
        if (lds > 32768u) HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        PSCHK(tm.timed(1, st, [&]() -> int {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, (const uint8_t *)p->state, p->pitch, N, rows, (const uint32_t *)d_sched,
                               (const uint32_t *)d_off, t.levels, M, sc.n_pad, (const double *)d_x, sched_lds, mh.a, (const uint8_t *)d_cls,
                               (const uint32_t *)d_node, min_post, d_dst, pitch_out, d_part, stride, d_cnt);
            HIPCHK(hipGetLastError());
            if (stage.p) HIPCHK(hipMemcpyPeerAsync(dst, dst_device, stage.p, p->device, (uint64_t)rows * pitch_out, st));
            return PS_OK;
        }));
        PSCHK(tm.timed(2, st, [&]() -> int {
            hipLaunchKernelGGL(lik_reduce_kernel, dim3((stride + 255u) / 256u), dim3(256), 0, st, (const double *)d_part, grid, stride, d_out);
            HIPCHK(hipGetLastError());
            return PS_OK;
        }));
    }
    unsigned long long cnt[3] = {};
    std::vector<double> out(stride);
    HIPCHK(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out.data(), d_out, (uint64_t)stride * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    res->lnl = out[stride - 1u];
    res->missing = cnt[0];
    res->masked = cnt[1];
    res->zero = cnt[2];
    res->conf.assign(M, 0.0);
    res->diff.assign(nodes, 0.0);
    for (uint32_t c = 0; c + 1u < nodes; c++) res->diff[c] = out[sc.slot_of[c]];
    for (uint32_t k = 0; k < M; k++) res->conf[k] = out[(size_t)slots + (sc.slot_of[N + k] - sc.n_pad)];
    return PS_OK;
}

static void anc_summary(ps_ancestral_t *o, const pars_tree &t, const model_host &mh, uint64_t sites, uint64_t clamped, const anc_result &res)
{
    memset(o, 0, sizeof *o);
    o->pop_size = t.N;
    o->sites = sites;
    o->merges = t.M;
    o->categories = mh.K();
    o->classed = mh.site_class ? 1 : 0;
    o->masked_cells = res.masked;
    o->zero_sites = res.zero;
    o->missing_cells = res.missing;
    o->clamped_lengths = clamped;
    o->lnl = res.lnl;
    double conf = 0.0, diff = 0.0;
    for (double v : res.conf) conf += v;
    for (double v : res.diff) diff += v;
    const uint64_t counted = sites - res.zero;
    o->mean_conf = counted ? conf / ((double)t.M * (double)counted) : 0.0;
    o->total_diff = diff;
}

extern "C" int ps_ancestral_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                      const double *length, uint64_t merges, const ps_subst_model *model, double min_posterior, ps_ancestral_t *out,
                                      uint8_t *anc_rows, double *node_conf, double *branch_diff)
{
    const char *call = "ps_ancestral_from_rows";
    if (!out || (!rows && cols)) return ps_fail(PS_ERR_INVALID, "null argument");
    model_host mh;
    PSCHK(model_check(call, model, cols, &mh));
    pars_tree t;
    PSCHK(anc_check_tree(call, left, right, merges, pop_size, mh, &t));
    PSCHK(anc_check_min(call, min_posterior));
    std::vector<double> used, x;
    uint64_t clamped = 0;
    PSCHK(lik_used_lengths(call, t, length, &used, &clamped));
    model_x(mh, used, &x);
    anc_result res;
    anc_host_pass(rows, cols, t, left, right, mh, mh.site_class, x.data(), min_posterior, anc_rows, &res);
    anc_summary(out, t, mh, cols, clamped, res);
    if (node_conf) memcpy(node_conf, res.conf.data(), res.conf.size() * sizeof(double));
    if (branch_diff) memcpy(branch_diff, res.diff.data(), res.diff.size() * sizeof(double));
    return PS_OK;
}

// m == nullptr: `core` answers for its own sites; else every shard's core handle does, each into its block of the one new handle.
// global: site_class is indexed by the global site (the ps_sim_ and ps_multi_ forms), else by the handle's own.
static int anc_run(const char *call, ps_multi *m, ps_population *core, bool global, const uint32_t *left, const uint32_t *right, const double *length,
                   uint64_t merges, const ps_subst_model *model, double min_posterior, ps_ancestral_t *out, ps_population **anc, double *node_conf,
                   double *branch_diff)
{
    if (anc) *anc = nullptr;
    if (!out) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(lik_handle(core, call));
    model_host mh;
    PSCHK(model_check(call, model, model_class_sites(m, core, global), &mh));
    pars_tree t;
    PSCHK(anc_check_tree(call, left, right, merges, core->cfg.pop_size, mh, &t));
    PSCHK(anc_check_min(call, min_posterior));
    std::vector<double> used, x;
    uint64_t clamped = 0;
    PSCHK(lik_used_lengths(call, t, length, &used, &clamped));       // (an invalid length fails before any device work)
    model_x(mh, used, &x);
    const size_t S = m ? m->shard.size() : 1;
    auto handle = [&](size_t k) { return m ? m->shard[k]->core : core; };
    if (m) PSCHK(ps_multi_sync(m));
    else {
        PSCHK(use_device(core));
        HIPCHK(hipStreamSynchronize(core->stream));
    }
    for (size_t k = 0; k < S; k++) handle(k)->ro[PS_RO_ANC].timed = false;
    ps_population *made = nullptr;
    bool onehot = true;
    for (size_t k = 0; k < S; k++) onehot = onehot && handle(k)->onehot_safe;
    if (anc) {
        if (m) PSCHK(sample_make(core, t.M, 0, core->cfg.global_cols, &made));
        else PSCHK(sample_make(core, t.M, core->cfg.col_offset, core->cfg.ncols, &made));
    }
    std::vector<event_timer> tm(S);
    std::vector<anc_result> part(S);
    auto shard_pass = [&](size_t k) -> int {
        ps_population *c = handle(k);
        const uint64_t off = m ? c->cfg.col_offset : 0;
        const uint8_t *cls = mh.site_class ? mh.site_class + (global ? c->cfg.col_offset : 0) : nullptr;
        uint8_t *dst = made ? made->state + off * made->pitch : nullptr;
        return anc_device_pass(c, tm[k], t, left, right, mh, cls, x.data(), min_posterior, dst, made ? made->pitch : 0u, made ? made->device : 0, &part[k]);
    };
    int rc = m ? multi_for_each(m, shard_pass) : shard_pass(0);
    for (size_t k = 0; rc == PS_OK && k < S; k++) {
        ps_population *c = handle(k);
        rc = use_device(c);
        if (rc == PS_OK) rc = tm[k].collect(c->ro[PS_RO_ANC], 3);
    }
    if (rc == PS_OK) rc = use_device(core);
    if (rc != PS_OK) {
        const std::string keep = g_err;
        if (made) ps_population_destroy(made);
        g_err = keep;
        return rc;
    }
    anc_result res;
    res.conf.swap(part[0].conf);
    res.diff.swap(part[0].diff);
    res.lnl = part[0].lnl;
    res.missing = part[0].missing;
    res.masked = part[0].masked;
    res.zero = part[0].zero;
    for (size_t k = 1; k < S; k++) {
        res.lnl += part[k].lnl;
        res.missing += part[k].missing;
        res.masked += part[k].masked;
        res.zero += part[k].zero;
        for (size_t c = 0; c < res.conf.size(); c++) res.conf[c] += part[k].conf[c];
        for (size_t c = 0; c < res.diff.size(); c++) res.diff[c] += part[k].diff[c];
    }
    const uint64_t sites = m ? m->prm.core_size : core->cfg.ncols;
    anc_summary(out, t, mh, sites, clamped, res);
    if (node_conf) memcpy(node_conf, res.conf.data(), res.conf.size() * sizeof(double));
    if (branch_diff) memcpy(branch_diff, res.diff.data(), res.diff.size() * sizeof(double));
    if (made) {
        made->nibble_safe = true;
        made->onehot_safe = onehot && res.masked == 0 && res.zero == 0;
        *anc = made;
    }
    return PS_OK;
}

extern "C" int ps_tree_ancestral_states(ps_population *core, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                        const ps_subst_model *model, double min_posterior, ps_ancestral_t *out, ps_population **anc,
                                        double *node_conf, double *branch_diff)
{
    if (anc) *anc = nullptr;
    PSCHK(ps_needs_device());
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return anc_run("ps_tree_ancestral_states", nullptr, core, false, left, right, length, merges, model, min_posterior, out, anc, node_conf, branch_diff);
}

extern "C" int ps_sim_tree_ancestral_states(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                            const ps_subst_model *model, double min_posterior, ps_ancestral_t *out, ps_population **anc,
                                            double *node_conf, double *branch_diff)
{
    if (anc) *anc = nullptr;
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    return anc_run("ps_sim_tree_ancestral_states", nullptr, s->core, true, left, right, length, merges, model, min_posterior, out, anc, node_conf,
                   branch_diff);
}

extern "C" int ps_multi_tree_ancestral_states(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                              const ps_subst_model *model, double min_posterior, ps_ancestral_t *out, ps_population **anc,
                                              double *node_conf, double *branch_diff)
{
    if (anc) *anc = nullptr;
    PSCHK(ps_needs_device());
    if (!m) return ps_fail(PS_ERR_INVALID, "null argument");
    return anc_run("ps_multi_tree_ancestral_states", m->shard.size() == 1 ? nullptr : m, m->shard[0]->core, true, left, right, length, merges, model,
                   min_posterior, out, anc, node_conf, branch_diff);
}

extern "C" int ps_ancestral_states_timing(ps_population *core, double *upload_ms, double *pass_ms, double *reduce_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_ANC], "no ancestral states have been computed on this handle", { upload_ms, pass_ms, reduce_ms });
}
