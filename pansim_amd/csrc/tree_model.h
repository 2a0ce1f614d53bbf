// tree_model.h -- ps_tree_model_likelihood / ps_tree_model_ml_lengths with their ps_sim_ and ps_multi_ forms, the host restatements
// ps_model_likelihood_from_rows and ps_model_ml_lengths_from_rows, and the host rule ps_f81_lengths_from_changes
// (include/pansim_hip.h; the definitions: docs/TREE_MODEL.md).  Included by pansim_capi.hip behind tree_likelihood.h, whose tree
// and length checks, optimiser parameters and device frame it shares.
//
// One PASS gives lnL of a tree with branch lengths under F81 with a root distribution and K rate categories, optionally every
// site's (mantissa, exponent) and posterior mean rate and the derivative sums g, h, q of every branch: on the device
// tree_model_kernel over the handle's sites on its stream, on the host the same subst_rule.h functions over rows, the sites in
// ascending order.  A sharded run adds the shards' lnL, g, h and q in shard order before the one Newton step.
#pragma once

#include "model_kernels.h"
#include "tree_likelihood.h"

// a checked ps_subst_model
struct model_host {
    model_args a{};
    double beta = 0.0, mean_rate = 0.0;
    bool reversible = false;            // root == freq bit for bit: only the sum of the two root branches is identified
    const uint8_t *site_class = nullptr;
    uint32_t K() const { return a.K; }
};

static int model_unit_sum(const char *call, const char *field, const double *v, uint32_t n)
{
    double s = 0.0;
    for (uint32_t i = 0; i < n; i++) s += v[i];
    if (!(fabs(s - 1.0) <= 1e-12)) return ps_fail(PS_ERR_INVALID, "%s: %s must sum to 1 within 1e-12, not to %.17g", call, field, s);
    return PS_OK;
}

// sites: how many entries site_class must have when it is given
static int model_check(const char *call, const ps_subst_model *m, uint64_t sites, model_host *h)
{
    if (!m) return ps_fail(PS_ERR_INVALID, "null argument");
    uint32_t zeros = 0;
    for (int i = 0; i < 4; i++) {
        if (!std::isfinite(m->freq[i]) || m->freq[i] < 0.0) return ps_fail(PS_ERR_INVALID, "%s: freq[%d] must be a number >= 0, not %g", call, i, m->freq[i]);
        if (!std::isfinite(m->root[i]) || !(m->root[i] > 0.0)) return ps_fail(PS_ERR_INVALID, "%s: root[%d] must be a number > 0, not %g", call, i, m->root[i]);
        zeros += m->freq[i] == 0.0;
    }
    if (zeros > 1) return ps_fail(PS_ERR_INVALID, "%s: freq may have at most one zero entry, not %u", call, zeros);
    PSCHK(model_unit_sum(call, "freq", m->freq, 4));
    PSCHK(model_unit_sum(call, "root", m->root, 4));
    if (m->categories < 1 || m->categories > PS_MODEL_MAX_CATEGORIES)
        return ps_fail(PS_ERR_INVALID, "%s: categories must be 1 .. %u, not %u", call, PS_MODEL_MAX_CATEGORIES, m->categories);
    for (uint32_t k = 0; k < m->categories; k++) {
        if (!std::isfinite(m->rate[k]) || m->rate[k] < 0.0) return ps_fail(PS_ERR_INVALID, "%s: rate[%u] must be a finite number >= 0, not %g", call, k, m->rate[k]);
        if (!std::isfinite(m->weight[k]) || !(m->weight[k] > 0.0)) return ps_fail(PS_ERR_INVALID, "%s: weight[%u] must be a number > 0, not %g", call, k, m->weight[k]);
    }
    PSCHK(model_unit_sum(call, "weight", m->weight, m->categories));
    if (m->site_class) {
        if (m->site_classes != sites)
            return ps_fail(PS_ERR_INVALID, "%s: site_class needs one entry per core site, site_classes = %llu, not %llu", call, (unsigned long long)sites,
                           (unsigned long long)m->site_classes);
        for (uint64_t s = 0; s < sites; s++)
            if (m->site_class[s] >= m->categories)
                return ps_fail(PS_ERR_INVALID, "%s: site_class[%llu] = %u is not below categories = %u", call, (unsigned long long)s, (unsigned)m->site_class[s],
                               m->categories);
    }
    *h = model_host();
    memcpy(h->a.freq, m->freq, sizeof h->a.freq);
    memcpy(h->a.root, m->root, sizeof h->a.root);
    h->a.K = m->categories;
    for (uint32_t k = 0; k < PS_MODEL_MAX_CATEGORIES; k++) {
        h->a.rate[k] = k < m->categories ? m->rate[k] : 0.0;
        h->a.weight[k] = k < m->categories ? m->weight[k] : 0.0;
        h->mean_rate += h->a.weight[k] * h->a.rate[k];
    }
    h->beta = ps_subst_beta(m->freq);
    h->reversible = memcmp(m->freq, m->root, sizeof m->freq) == 0;
    h->site_class = m->site_class;
    return PS_OK;
}

static int model_check_deriv(const char *call, uint64_t pop_size)
{
    if (pop_size > PS_MODEL_MAX_POP_DERIV)
        return ps_fail(PS_ERR_INVALID, "%s with derivatives needs pop_size <= PS_MODEL_MAX_POP_DERIV = %u (36 LDS bytes per node and 32 per branch), not %llu",
                       call, PS_MODEL_MAX_POP_DERIV, (unsigned long long)pop_size);
    return PS_OK;
}

// The LDS of a pass: tree_lik_kernel's, with derivatives 32 bytes of sums per slot (g, h, q, the temporary)
static uint32_t model_lds_bytes(uint32_t N, uint32_t levels, bool deriv, uint32_t *sched_lds)
{
    const uint32_t n_pad = (N + 15u) & ~15u, M = N - 1u, Mp = (M + 1u) & ~1u, slots = n_pad + M;
    const uint32_t base = n_pad * 4u + Mp * 36u + (deriv ? slots * 32u : 0u), sched = (M + levels + 1u) * 4u;
    *sched_lds = base + sched <= PS_LIK_LDS_SCHED ? 1u : 0u;
    return base + (*sched_lds ? sched : 0u);
}

// what one pass returns: mant / ex / rate of every site (null: not asked for), g / h / q of every node (deriv only), lnL, missing
struct model_result {
    double *mant = nullptr;
    int32_t *ex = nullptr;
    double *rate = nullptr;
    std::vector<double> g, h, q;
    double lnl = 0.0;
    uint64_t missing = 0;
};

// a pass over the tree with x[K][N + M] (the root's entries are not read)
typedef std::function<int(const double *x, bool deriv, model_result *res)> model_pass_fn;

// One pass on the host over individual-major rows, the sites in ascending order.  cls: the class of site 0 on (null: none)
static void model_host_pass(const uint8_t *rows, uint64_t cols, const pars_tree &t, const uint32_t *left, const uint32_t *right, const model_host &mh,
                            const uint8_t *cls, const double *x, bool deriv, model_result *res)
{
    const uint32_t N = t.N, M = t.M, nodes = N + M, K = mh.K();
    const double *pi = mh.a.freq, *rho = mh.a.root;
    std::vector<double> L((size_t)K * 4 * nodes), U((size_t)4 * nodes), tmp(nodes, 0.0);
    std::vector<int32_t> E((size_t)K * nodes, 0);
    res->g.assign(deriv ? nodes : 0, 0.0);
    res->h.assign(deriv ? nodes : 0, 0.0);
    res->q.assign(deriv ? nodes : 0, 0.0);
    res->lnl = 0.0;
    res->missing = 0;
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
        double sm, sr;
        int32_t se;
        if (assigned) {
            sm = mant[kb];
            se = ex[kb];
            sr = mh.a.rate[kb];
            post[kb] = 1.0;
        } else {
            sm = ps_subst_mix(K, mh.a.weight, mant, ex, &se, post);
            sr = ps_subst_mean_rate(K, post, mh.a.rate);
        }
        if (res->mant) res->mant[s] = sm;
        if (res->ex) res->ex[s] = se;
        if (res->rate) res->rate[s] = sr;
        res->lnl += ps_jc_site_ln(sm, se);
        if (!deriv) continue;
        for (uint32_t k = kb; k < ke; k++) {
            const double *Lk = &L[(size_t)k * 4 * nodes], *xk = x + (size_t)k * nodes;
            const double rk = mh.a.rate[k];
            const bool first = k == kb, last = k + 1u == ke;
            for (uint32_t j = M; j-- > 0;) {
                const uint32_t l = left[j], r = right[j], c = N + j;
                double T[4] = { rho[0], rho[1], rho[2], rho[3] }, ml[4], mr[4];
                if (j != M - 1u) ps_subst_down(xk[c], pi, &U[4u * c], T);
                ps_subst_up(xk[l], pi, &Lk[4u * l], ml);
                ps_subst_up(xk[r], pi, &Lk[4u * r], mr);
                (void)ps_jc_join(mr, T, &U[4u * l]);
                (void)ps_jc_join(ml, T, &U[4u * r]);
                for (const uint32_t v : { l, r }) {
                    const double ratio = ps_subst_ratio(xk[v], pi, &U[4u * v], &Lk[4u * v]);
                    res->q[v] += ps_subst_qterm(post[k], rk, xk[v], ratio);
                    const double term = ps_subst_dterm(post[k], rk, xk[v], ratio), d = first ? term : tmp[v] + term;
                    if (last) {
                        res->g[v] += d;
                        res->h[v] += d * d;
                    } else
                        tmp[v] = d;
                }
            }
        }
    }
}

// One pass of handle p over its own sites on its stream, complete when it returns.  cls: the classes of p's own sites (null: none).
// Timer groups: 0 the uploads, 1 the kernel, 2 the sum of the workgroups' rows.
static int model_device_pass(ps_population *p, event_timer &tm, const pars_tree &t, const uint32_t *left, const uint32_t *right, const model_host &mh,
                             const uint8_t *cls, const double *x, bool deriv, model_result *res)
{
    const uint32_t N = t.N, M = t.M, nodes = N + M, rows = (uint32_t)p->cfg.ncols, K = mh.K();
    PSCHK(use_device(p));
    const uint32_t *slot = nullptr;
    PSCHK(rows_current(p, &slot));
    pars_schedule sc;
    pars_make_schedule(t, left, right, slot, &sc);
    const uint32_t slots = sc.n_pad + M, stride = deriv ? 3u * slots + 1u : 1u;
    std::vector<double> xs((size_t)K * slots, 1.0);
    for (uint32_t k = 0; k < K; k++)
        for (uint32_t c = 0; c + 1u < nodes; c++) xs[(size_t)k * slots + sc.slot_of[c]] = x[(size_t)k * nodes + c];
    uint32_t sched_lds = 0;
    const uint32_t lds = model_lds_bytes(N, t.levels, deriv, &sched_lds);
    const uint32_t threads = N <= 1024u ? 64u : 256u;
    const uint32_t per_cu = std::max(1u, std::min(8u, (160u * 1024u) / (lds + 1024u + 512u)));
    const uint32_t grid = std::max(1u, std::min((rows + 3u) / 4u, 256u * per_cu));
    scratch_layout lay;
    const uint64_t o_miss = lay.add(8, 16), o_out = lay.add((uint64_t)stride * 8, 16);
    const uint64_t o_sched = lay.add((uint64_t)M * 4, 16), o_off = lay.add((uint64_t)sc.level_off.size() * 4, 16);
    const uint64_t o_x = lay.add((uint64_t)K * slots * 8, 16), o_cls = lay.add(cls ? (uint64_t)rows : 0, 16);
    const uint64_t o_mant = lay.add(res->mant ? (uint64_t)rows * 8 : 0, 16), o_exp = lay.add(res->ex ? (uint64_t)rows * 4 : 0, 16);
    const uint64_t o_rate = lay.add(res->rate ? (uint64_t)rows * 8 : 0, 16);
    const uint64_t o_part = lay.add((uint64_t)grid * stride * 8, 16);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(p->ro[PS_RO_MODEL], lay.bytes, &base,
                      "cannot allocate the %llu bytes of the schedule, the x table and the sums of the model likelihood of a tree of %u merges over %u sites", M,
                      rows));
    hipStream_t st = p->stream;
    unsigned long long *d_miss = (unsigned long long *)(base + o_miss);
    double *d_out = (double *)(base + o_out), *d_x = (double *)(base + o_x), *d_part = (double *)(base + o_part);
    uint32_t *d_sched = (uint32_t *)(base + o_sched), *d_off = (uint32_t *)(base + o_off);
    uint8_t *d_cls = cls && rows ? base + o_cls : nullptr;
    double *d_mant = res->mant ? (double *)(base + o_mant) : nullptr, *d_rate = res->rate ? (double *)(base + o_rate) : nullptr;
    int32_t *d_exp = res->ex ? (int32_t *)(base + o_exp) : nullptr;
    // (the sources of the copies live until this function's last synchronisation)
    PSCHK(tm.timed(0, st, [&]() -> int {
        HIPCHK(hipMemsetAsync(d_miss, 0, o_sched, st));
        HIPCHK(hipMemcpyAsync(d_sched, sc.sched.data(), (uint64_t)M * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_off, sc.level_off.data(), (uint64_t)sc.level_off.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_x, xs.data(), (uint64_t)K * slots * 8, hipMemcpyHostToDevice, st));
        if (d_cls) HIPCHK(hipMemcpyAsync(d_cls, cls, rows, hipMemcpyHostToDevice, st));
        return PS_OK;
    }));
    if (rows) {
        auto kern = deriv ? tree_model_kernel<true> : tree_model_kernel<false>;
        if (lds > 32768u) HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        PSCHK(tm.timed(1, st, [&]() -> int {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, (const uint8_t *)p->state, p->pitch, N, rows, (const uint32_t *)d_sched,
                               (const uint32_t *)d_off, t.levels, M, sc.n_pad, (const double *)d_x, sched_lds, mh.a, (const uint8_t *)d_cls, d_mant, d_exp,
                               d_rate, 0u, d_part, stride, d_miss);
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
    if (rows && res->rate) HIPCHK(hipMemcpyAsync(res->rate, d_rate, (uint64_t)rows * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    res->lnl = out[stride - 1u];
    res->missing = miss;
    res->g.assign(deriv ? nodes : 0, 0.0);
    res->h.assign(deriv ? nodes : 0, 0.0);
    res->q.assign(deriv ? nodes : 0, 0.0);
    if (deriv)
        for (uint32_t c = 0; c + 1u < nodes; c++) {
            res->g[c] = out[sc.slot_of[c]];
            res->h[c] = out[(size_t)slots + sc.slot_of[c]];
            res->q[c] = out[(size_t)2 * slots + sc.slot_of[c]];
        }
    return PS_OK;
}

static void model_summary(ps_model_likelihood_t *o, const pars_tree &t, const model_host &mh, uint64_t sites, uint64_t clamped, uint64_t missing,
                          const std::vector<double> &used)
{
    memset(o, 0, sizeof *o);
    o->pop_size = t.N;
    o->sites = sites;
    o->merges = t.M;
    o->clamped_lengths = clamped;
    o->missing_cells = missing;
    o->categories = mh.K();
    o->classed = mh.site_class ? 1 : 0;
    o->beta = mh.beta;
    o->mean_rate = mh.mean_rate;
    double sum = 0.0;
    for (uint32_t c = 0; c + 1u < t.N + t.M; c++) sum += used[c];
    o->tree_length = sum;
}

// x[K][nodes] of the used lengths (the root's entries 1)
static void model_x(const model_host &mh, const std::vector<double> &used, std::vector<double> *x)
{
    const size_t nodes = used.size();
    x->assign(mh.K() * nodes, 1.0);
    for (uint32_t k = 0; k < mh.K(); k++)
        for (size_t c = 0; c + 1u < nodes; c++) (*x)[k * nodes + c] = ps_subst_x(mh.a.rate[k], used[c], mh.beta);
}

// lnL of the tree with the lengths as given (clamped), one pass
static int model_evaluate(const char *call, const pars_tree &t, const model_host &mh, const double *length, uint64_t sites, const model_pass_fn &pass,
                          ps_model_likelihood_t *out, double *site_mant, int32_t *site_exp, double *site_rate, double *branch_g, double *branch_h,
                          double *branch_q)
{
    std::vector<double> used, x;
    uint64_t clamped = 0;
    PSCHK(lik_used_lengths(call, t, length, &used, &clamped));
    model_x(mh, used, &x);
    model_result res;
    res.mant = site_mant;
    res.ex = site_exp;
    res.rate = site_rate;
    const bool deriv = branch_g || branch_h || branch_q;
    PSCHK(pass(x.data(), deriv, &res));
    model_summary(out, t, mh, sites, clamped, res.missing, used);
    out->passes = 1;
    out->lnl = out->start_lnl = res.lnl;
    if (branch_g) memcpy(branch_g, res.g.data(), res.g.size() * sizeof(double));
    if (branch_h) memcpy(branch_h, res.h.data(), res.h.size() * sizeof(double));
    if (branch_q) memcpy(branch_q, res.q.data(), res.q.size() * sizeof(double));
    return PS_OK;
}

// The optimiser of docs/TREE_LIKELIHOOD.md fed with (dlnL/dt, d2lnL/dt2) of the model; the root rule only when it is reversible
static int model_optimise(const char *call, const pars_tree &t, const model_host &mh, const uint32_t *left, const uint32_t *right, const double *length,
                          uint64_t sites, const ps_ml_params &prm, const model_pass_fn &pass, ps_model_likelihood_t *out, double *length_out,
                          double *round_lnl)
{
    const uint32_t nodes = t.N + t.M, root = nodes - 1u, rl = left[t.M - 1u], rr = right[t.M - 1u];
    const uint32_t held = mh.reversible ? rr : root;
    std::vector<double> used, x, cand, cx;
    uint64_t clamped = 0;
    PSCHK(lik_used_lengths(call, t, length, &used, &clamped));
    if (mh.reversible) {
        used[rl] = ps_jc_clamp(used[rl] + used[rr]);
        used[rr] = PS_LIK_MIN_LENGTH;
    }
    model_x(mh, used, &x);
    model_result cur, next;
    PSCHK(pass(x.data(), true, &cur));
    uint64_t rounds = 0, passes = 1, rollbacks = 0, converged = 0;
    const double start = cur.lnl;
    if (round_lnl) round_lnl[0] = cur.lnl;
    double lambda = 1.0;
    while (rounds < prm.max_rounds && lambda >= 0x1p-20) {
        cand = used;
        for (uint32_t c = 0; c < root; c++)
            if (c != held) cand[c] = ps_subst_newton(used[c], ps_subst_dt(mh.beta, cur.g[c]), ps_subst_dt2(mh.beta, cur.q[c], cur.h[c]), lambda);
        model_x(mh, cand, &cx);
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
    model_summary(out, t, mh, sites, clamped, cur.missing, used);
    out->rounds = rounds;
    out->passes = passes;
    out->rollbacks = rollbacks;
    out->converged = converged;
    out->lnl = cur.lnl;
    out->start_lnl = start;
    if (length_out) memcpy(length_out, used.data(), (size_t)nodes * sizeof(double));
    return PS_OK;
}

static int model_check_ml(const ps_ml_params *prm, const ps_model_likelihood_t *out, const double *round_lnl, uint64_t round_cap)
{
    if (!out) return ps_fail(PS_ERR_INVALID, "null argument");
    const ps_likelihood_t unused{};
    return lik_check_ml(prm, &unused, round_lnl, round_cap);
}

extern "C" int ps_f81_lengths_from_changes(const uint64_t *branch_changes, uint64_t nodes, uint64_t sites, const double *freq, double *length)
{
    if (!freq || (nodes && (!branch_changes || !length))) return ps_fail(PS_ERR_INVALID, "null argument");
    ps_subst_model m{};
    memcpy(m.freq, freq, sizeof m.freq);
    m.root[0] = m.root[1] = m.root[2] = m.root[3] = 0.25;
    m.categories = 1;
    m.rate[0] = m.weight[0] = 1.0;
    model_host mh;
    PSCHK(model_check("ps_f81_lengths_from_changes", &m, 0, &mh));
    for (uint64_t c = 0; c < nodes; c++) length[c] = ps_subst_length_from_changes(branch_changes[c], sites, mh.beta);
    return PS_OK;
}

static model_pass_fn model_rows_pass(const uint8_t *rows, uint64_t cols, const pars_tree &t, const uint32_t *left, const uint32_t *right,
                                     const model_host &mh)
{
    return [=, &t, &mh](const double *x, bool deriv, model_result *res) -> int {
        model_host_pass(rows, cols, t, left, right, mh, mh.site_class, x, deriv, res);
        return PS_OK;
    };
}

extern "C" int ps_model_likelihood_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                             const double *length, uint64_t merges, const ps_subst_model *model, ps_model_likelihood_t *out,
                                             double *site_mant, int32_t *site_exp, double *site_rate, double *branch_g, double *branch_h,
                                             double *branch_q)
{
    const char *call = "ps_model_likelihood_from_rows";
    if (!out || (!rows && cols)) return ps_fail(PS_ERR_INVALID, "null argument");
    model_host mh;
    PSCHK(model_check(call, model, cols, &mh));
    pars_tree t;
    PSCHK(lik_check_tree(call, left, right, merges, pop_size, &t));
    if (branch_g || branch_h || branch_q) PSCHK(model_check_deriv(call, pop_size));
    return model_evaluate(call, t, mh, length, cols, model_rows_pass(rows, cols, t, left, right, mh), out, site_mant, site_exp, site_rate, branch_g,
                          branch_h, branch_q);
}

extern "C" int ps_model_ml_lengths_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                             const double *length_in, uint64_t merges, const ps_subst_model *model, const ps_ml_params *prm,
                                             ps_model_likelihood_t *out, double *length_out, double *round_lnl, uint64_t round_cap)
{
    const char *call = "ps_model_ml_lengths_from_rows";
    PSCHK(model_check_ml(prm, out, round_lnl, round_cap));
    if (!rows && cols) return ps_fail(PS_ERR_INVALID, "null argument");
    model_host mh;
    PSCHK(model_check(call, model, cols, &mh));
    pars_tree t;
    PSCHK(lik_check_tree(call, left, right, merges, pop_size, &t));
    PSCHK(model_check_deriv(call, pop_size));
    return model_optimise(call, t, mh, left, right, length_in, cols, *prm, model_rows_pass(rows, cols, t, left, right, mh), out, length_out, round_lnl);
}

// What the device entries share, as lik_device: m == nullptr: `core` answers for its own sites; else every shard's core handle
// does.  global: site_class is indexed by the global site (the ps_sim_ and ps_multi_ forms), else by the handle's own.
struct model_device {
    ps_multi *m;
    ps_population *core;
    const pars_tree &t;
    const model_host &mh;
    const uint32_t *left, *right;
    bool global;
    std::vector<event_timer> tm;
    model_device(ps_multi *m_, ps_population *core_, const pars_tree &t_, const model_host &mh_, const uint32_t *l, const uint32_t *r, bool global_)
        : m(m_), core(core_), t(t_), mh(mh_), left(l), right(r), global(global_), tm(m_ ? m_->shard.size() : 1) {}
    ps_population *handle(size_t k) const { return m ? m->shard[k]->core : core; }
    uint64_t sites() const { return m ? m->prm.core_size : core->cfg.ncols; }
    int begin()
    {
        if (m) PSCHK(ps_multi_sync(m));
        else {
            PSCHK(use_device(core));
            HIPCHK(hipStreamSynchronize(core->stream));
        }
        for (size_t k = 0; k < tm.size(); k++) handle(k)->ro[PS_RO_MODEL].timed = false;
        return PS_OK;
    }
    int pass(const double *x, bool deriv, model_result *res)
    {
        const size_t S = tm.size();
        std::vector<model_result> part(S);
        auto shard_pass = [&](size_t k) -> int {
            ps_population *c = handle(k);
            const uint64_t off = m ? c->cfg.col_offset : 0;
            part[k].mant = res->mant ? res->mant + off : nullptr;
            part[k].ex = res->ex ? res->ex + off : nullptr;
            part[k].rate = res->rate ? res->rate + off : nullptr;
            const uint8_t *cls = mh.site_class ? mh.site_class + (global ? c->cfg.col_offset : 0) : nullptr;
            return model_device_pass(c, tm[k], t, left, right, mh, cls, x, deriv, &part[k]);
        };
        if (m) PSCHK(multi_for_each(m, shard_pass));
        else PSCHK(shard_pass(0));
        res->g.swap(part[0].g);
        res->h.swap(part[0].h);
        res->q.swap(part[0].q);
        res->lnl = part[0].lnl;
        res->missing = part[0].missing;
        for (size_t k = 1; k < S; k++) {
            res->lnl += part[k].lnl;
            res->missing += part[k].missing;
            for (size_t c = 0; c < res->g.size(); c++) {
                res->g[c] += part[k].g[c];
                res->h[c] += part[k].h[c];
                res->q[c] += part[k].q[c];
            }
        }
        return PS_OK;
    }
    int end()
    {
        for (size_t k = 0; k < tm.size(); k++) {
            ps_population *c = handle(k);
            PSCHK(use_device(c));
            PSCHK(tm[k].collect(c->ro[PS_RO_MODEL], 3));
        }
        return use_device(core);
    }
};

// the entries of site_class a call needs: the handle's own sites, or all core sites of the run
static uint64_t model_class_sites(ps_multi *m, const ps_population *core, bool global)
{
    return m ? m->prm.core_size : (global ? core->cfg.global_cols : core->cfg.ncols);
}

static int model_run(const char *call, ps_multi *m, ps_population *core, bool global, const uint32_t *left, const uint32_t *right, const double *length,
                     uint64_t merges, const ps_subst_model *model, ps_model_likelihood_t *out, double *site_mant, int32_t *site_exp, double *site_rate,
                     double *branch_g, double *branch_h, double *branch_q)
{
    if (!out) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(lik_handle(core, call));
    model_host mh;
    PSCHK(model_check(call, model, model_class_sites(m, core, global), &mh));
    pars_tree t;
    PSCHK(lik_check_tree(call, left, right, merges, core->cfg.pop_size, &t));
    if (branch_g || branch_h || branch_q) PSCHK(model_check_deriv(call, core->cfg.pop_size));
    model_device dev(m, core, t, mh, left, right, global);
    std::vector<double> used;
    uint64_t clamped;
    PSCHK(lik_used_lengths(call, t, length, &used, &clamped));       // (an invalid length fails before any device work)
    PSCHK(dev.begin());
    const model_pass_fn pass = [&](const double *x, bool deriv, model_result *res) -> int { return dev.pass(x, deriv, res); };
    PSCHK(model_evaluate(call, t, mh, length, dev.sites(), pass, out, site_mant, site_exp, site_rate, branch_g, branch_h, branch_q));
    return dev.end();
}

static int model_ml_run(const char *call, ps_multi *m, ps_population *core, bool global, const uint32_t *left, const uint32_t *right,
                        const double *length_in, uint64_t merges, const ps_subst_model *model, const ps_ml_params *prm, ps_model_likelihood_t *out,
                        double *length_out, double *round_lnl, uint64_t round_cap)
{
    PSCHK(model_check_ml(prm, out, round_lnl, round_cap));
    PSCHK(lik_handle(core, call));
    model_host mh;
    PSCHK(model_check(call, model, model_class_sites(m, core, global), &mh));
    pars_tree t;
    PSCHK(lik_check_tree(call, left, right, merges, core->cfg.pop_size, &t));
    PSCHK(model_check_deriv(call, core->cfg.pop_size));
    model_device dev(m, core, t, mh, left, right, global);
    std::vector<double> used;
    uint64_t clamped;
    PSCHK(lik_used_lengths(call, t, length_in, &used, &clamped));
    PSCHK(dev.begin());
    const model_pass_fn pass = [&](const double *x, bool deriv, model_result *res) -> int { return dev.pass(x, deriv, res); };
    PSCHK(model_optimise(call, t, mh, left, right, length_in, dev.sites(), *prm, pass, out, length_out, round_lnl));
    return dev.end();
}

extern "C" int ps_tree_model_likelihood(ps_population *core, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                        const ps_subst_model *model, ps_model_likelihood_t *out, double *site_mant, int32_t *site_exp,
                                        double *site_rate, double *branch_g, double *branch_h, double *branch_q)
{
    PSCHK(ps_needs_device());
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return model_run("ps_tree_model_likelihood", nullptr, core, false, left, right, length, merges, model, out, site_mant, site_exp, site_rate, branch_g,
                     branch_h, branch_q);
}

extern "C" int ps_sim_tree_model_likelihood(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                            const ps_subst_model *model, ps_model_likelihood_t *out, double *site_mant, int32_t *site_exp,
                                            double *site_rate, double *branch_g, double *branch_h, double *branch_q)
{
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    return model_run("ps_sim_tree_model_likelihood", nullptr, s->core, true, left, right, length, merges, model, out, site_mant, site_exp, site_rate,
                     branch_g, branch_h, branch_q);
}

extern "C" int ps_multi_tree_model_likelihood(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                              const ps_subst_model *model, ps_model_likelihood_t *out, double *site_mant, int32_t *site_exp,
                                              double *site_rate, double *branch_g, double *branch_h, double *branch_q)
{
    PSCHK(ps_needs_device());
    if (!m) return ps_fail(PS_ERR_INVALID, "null argument");
    return model_run("ps_multi_tree_model_likelihood", m->shard.size() == 1 ? nullptr : m, m->shard[0]->core, true, left, right, length, merges, model,
                     out, site_mant, site_exp, site_rate, branch_g, branch_h, branch_q);
}

extern "C" int ps_tree_model_ml_lengths(ps_population *core, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                                        const ps_subst_model *model, const ps_ml_params *prm, ps_model_likelihood_t *out, double *length_out,
                                        double *round_lnl, uint64_t round_cap)
{
    PSCHK(ps_needs_device());
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return model_ml_run("ps_tree_model_ml_lengths", nullptr, core, false, left, right, length_in, merges, model, prm, out, length_out, round_lnl,
                        round_cap);
}

extern "C" int ps_sim_tree_model_ml_lengths(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                                            const ps_subst_model *model, const ps_ml_params *prm, ps_model_likelihood_t *out, double *length_out,
                                            double *round_lnl, uint64_t round_cap)
{
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    return model_ml_run("ps_sim_tree_model_ml_lengths", nullptr, s->core, true, left, right, length_in, merges, model, prm, out, length_out, round_lnl,
                        round_cap);
}

extern "C" int ps_multi_tree_model_ml_lengths(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                                              const ps_subst_model *model, const ps_ml_params *prm, ps_model_likelihood_t *out, double *length_out,
                                              double *round_lnl, uint64_t round_cap)
{
    PSCHK(ps_needs_device());
    if (!m) return ps_fail(PS_ERR_INVALID, "null argument");
    return model_ml_run("ps_multi_tree_model_ml_lengths", m->shard.size() == 1 ? nullptr : m, m->shard[0]->core, true, left, right, length_in, merges,
                        model, prm, out, length_out, round_lnl, round_cap);
}

extern "C" int ps_tree_model_timing(ps_population *core, double *schedule_ms, double *pass_ms, double *reduce_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_MODEL], "no tree model likelihood has been computed on this handle", { schedule_ms, pass_ms, reduce_ms });
}
