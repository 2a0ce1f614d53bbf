// tree_genes.h -- ps_tree_gene_likelihood / ps_tree_gene_ancestral / ps_tree_gene_fit with their ps_sim_ and ps_multi_ forms,
// ps_tree_gene_timing and the host restatements ps_gene_likelihood_from_rows, ps_gene_ancestral_from_rows and ps_gene_fit_from_rows
// (include/pansim_hip.h; the definitions: docs/GENE_MODEL.md).  Included by pansim_capi.hip behind ancestral_states.h, whose tree
// check, schedule and frame it shares, and behind isolate_samples.h, whose sample_make shapes the new handle.
//
// One PASS gives every gene's likelihood under ps_gene_model and, `down`, the marginal reconstruction of the inner nodes with the
// directed joints of the branches: on the device tree_gene_kernel over the gene-major view of the accessory handle on its stream,
// on the host the same gene_rule.h functions over rows, the genes in ascending order.  The fit (gene_fit) is one loop over either
// kind of pass and reads nothing of a pass but the genes' (mantissa, exponent) and posteriors, which are the same bits on both.
#pragma once

#include "gene_kernels.h"

static_assert(PS_GENE_MAX_POP == PS_GENE_KERNEL_MAX_POP && PS_GENE_MAX_POP_MIX == PS_GENE_KERNEL_MAX_POP_MIX, "the limits of the header are the kernel's");

// a checked ps_gene_model
struct gene_host {
    gene_args a{};
    double beta = 0.0, mean_rate = 0.0;
    const uint8_t *gene_class = nullptr;
    uint32_t K() const { return a.K; }
    bool mixture() const { return !gene_class && a.K > 1u; }
};

// genes: how many entries gene_class must have when it is given
static int gene_model_check(const char *call, const ps_gene_model *m, uint64_t genes, gene_host *h)
{
    if (!m) return ps_fail(PS_ERR_INVALID, "null argument");
    for (int i = 0; i < 2; i++) {
        if (!std::isfinite(m->freq[i]) || !(m->freq[i] > 0.0)) return ps_fail(PS_ERR_INVALID, "%s: freq[%d] must be a number > 0, not %g", call, i, m->freq[i]);
        if (!std::isfinite(m->root[i]) || !(m->root[i] > 0.0)) return ps_fail(PS_ERR_INVALID, "%s: root[%d] must be a number > 0, not %g", call, i, m->root[i]);
    }
    PSCHK(model_unit_sum(call, "freq", m->freq, 2));
    PSCHK(model_unit_sum(call, "root", m->root, 2));
    if (m->categories < 1 || m->categories > PS_MODEL_MAX_CATEGORIES)
        return ps_fail(PS_ERR_INVALID, "%s: categories must be 1 .. %u, not %u", call, PS_MODEL_MAX_CATEGORIES, m->categories);
    for (uint32_t k = 0; k < m->categories; k++) {
        if (!std::isfinite(m->rate[k]) || m->rate[k] < 0.0) return ps_fail(PS_ERR_INVALID, "%s: rate[%u] must be a finite number >= 0, not %g", call, k, m->rate[k]);
        if (!std::isfinite(m->weight[k]) || !(m->weight[k] > 0.0)) return ps_fail(PS_ERR_INVALID, "%s: weight[%u] must be a number > 0, not %g", call, k, m->weight[k]);
    }
    PSCHK(model_unit_sum(call, "weight", m->weight, m->categories));
    if (m->gene_class) {
        if (m->gene_classes != genes)
            return ps_fail(PS_ERR_INVALID, "%s: gene_class needs one entry per gene, gene_classes = %llu, not %llu", call, (unsigned long long)genes,
                           (unsigned long long)m->gene_classes);
        for (uint64_t g = 0; g < genes; g++)
            if (m->gene_class[g] >= m->categories)
                return ps_fail(PS_ERR_INVALID, "%s: gene_class[%llu] = %u is not below categories = %u", call, (unsigned long long)g, (unsigned)m->gene_class[g],
                               m->categories);
    }
    *h = gene_host();
    memcpy(h->a.freq, m->freq, sizeof h->a.freq);
    memcpy(h->a.root, m->root, sizeof h->a.root);
    h->a.K = m->categories;
    for (uint32_t k = 0; k < PS_MODEL_MAX_CATEGORIES; k++) {
        h->a.rate[k] = k < m->categories ? m->rate[k] : 0.0;
        h->a.weight[k] = k < m->categories ? m->weight[k] : 0.0;
        h->mean_rate += h->a.weight[k] * h->a.rate[k];
    }
    h->beta = ps_gene_beta(m->freq);
    h->gene_class = m->gene_class;
    return PS_OK;
}

static int gene_check_tree(const char *call, const uint32_t *left, const uint32_t *right, uint64_t merges, uint64_t pop_size, const gene_host &gh,
                           pars_tree *t)
{
    const bool mix = gh.mixture();
    const uint32_t cap = mix ? PS_GENE_MAX_POP_MIX : PS_GENE_MAX_POP;
    if (pop_size < 2 || pop_size > cap)
        return ps_fail(PS_ERR_INVALID, "%s needs 2 <= pop_size <= %s = %u (about %s LDS bytes per leaf), not %llu", call,
                       mix ? "PS_GENE_MAX_POP_MIX" : "PS_GENE_MAX_POP", cap, mix ? "84.25" : "68.25", (unsigned long long)pop_size);
    if (merges != pop_size - 1)
        return ps_fail(PS_ERR_INVALID, "%s needs a spanning tree: %llu merges over %llu leaves, not %llu", call,
                       (unsigned long long)(pop_size - 1), (unsigned long long)pop_size, (unsigned long long)merges);
    return pars_check_tree(left, right, merges, pop_size, t);
}

// used[N + M] = the lengths clamped below (the root's: 0), *clamped = how many entries the clamp changed
static int gene_used_lengths(const char *call, const pars_tree &t, const double *length, std::vector<double> *used, uint64_t *clamped)
{
    if (!length) return ps_fail(PS_ERR_INVALID, "null argument");
    const uint32_t nodes = t.N + t.M;
    used->assign(nodes, 0.0);
    *clamped = 0;
    for (uint32_t c = 0; c + 1u < nodes; c++) {
        if (!std::isfinite(length[c])) return ps_fail(PS_ERR_INVALID, "%s: the length of node %u is not a finite number", call, c);
        (*used)[c] = ps_gene_clamp(length[c]);
        *clamped += (*used)[c] != length[c];
    }
    return PS_OK;
}

// x[K][2][N + M] of the used lengths: per class the row of x and the row of y = 1 - x (libm on the host; the root's entries are
// 1 and 0 and never read)
static void gene_x(const gene_host &gh, const std::vector<double> &used, std::vector<double> *x)
{
    const size_t nodes = used.size();
    x->assign((size_t)gh.K() * 2 * nodes, 1.0);
    for (uint32_t k = 0; k < gh.K(); k++) {
        double *xk = &(*x)[(size_t)k * 2 * nodes], *yk = xk + nodes;
        yk[nodes - 1] = 0.0;
        for (size_t c = 0; c + 1 < nodes; c++) {
            xk[c] = ps_gene_x(gh.a.rate[k], used[c], gh.beta);
            yk[c] = ps_gene_y(gh.a.rate[k], used[c], gh.beta);
        }
    }
}

// The LDS of a pass (gene_kernels.h); the copies of the schedule and of node_of behind it while the whole stays within
// PS_LIK_LDS_SCHED
static uint32_t gene_lds_bytes(uint32_t N, uint32_t levels, bool mix, uint32_t *sched_lds)
{
    const uint32_t n_pad = (N + 15u) & ~15u, M = N - 1u, Mp = (M + 1u) & ~1u, slots = n_pad + M, W = (N + 63u) / 64u, Wm = (M + 63u) / 64u;
    const uint32_t base = Mp * 16u + slots * 16u + M * 16u + (mix ? M * 16u : 0u) + (W + Wm) * 8u + Mp * 4u, sched = (2u * M + levels + 1u) * 4u;
    *sched_lds = base + sched <= PS_LIK_LDS_SCHED ? 1u : 0u;
    return base + (*sched_lds ? sched : 0u);
}

// what one pass returns: per gene (null: not asked for) mant, ex, post[G x K], rate and, down, gains and losses; down: node_conf
// and node_genes of every merge, gains and losses of every node (the root's 0); lnL and the genes of likelihood 0
struct gene_result {
    double *mant = nullptr;
    int32_t *ex = nullptr;
    double *post = nullptr, *rate = nullptr, *ggain = nullptr, *gloss = nullptr;
    std::vector<double> conf, ngenes, bgain, bloss;
    double lnl = 0.0;
    uint64_t zero = 0;
};

// a pass under a model: `down` with the reconstruction (states into the pass's own destination)
typedef std::function<int(const gene_host &gh, bool down, gene_result *res)> gene_pass_fn;

// One pass on the host over individual-major rows, the genes in ascending order.  anc_rows (null: not stored): merges x cols
// bytes 0 / 1, row k = node N + k
static void gene_host_pass(const uint8_t *rows, uint64_t cols, const pars_tree &t, const uint32_t *left, const uint32_t *right, const gene_host &gh,
                           const double *x, bool down, uint8_t *anc_rows, gene_result *res)
{
    const uint32_t N = t.N, M = t.M, nodes = N + M, K = gh.K();
    const double *pi = gh.a.freq, *rho = gh.a.root;
    const uint8_t *cls = gh.gene_class;
    std::vector<double> L((size_t)K * 2 * nodes), U((size_t)2 * nodes), acc((size_t)2 * M, 0.0);
    std::vector<int32_t> E((size_t)K * nodes, 0);
    res->conf.assign(down ? M : 0, 0.0);
    res->ngenes.assign(down ? M : 0, 0.0);
    res->bgain.assign(down ? nodes : 0, 0.0);
    res->bloss.assign(down ? nodes : 0, 0.0);
    res->lnl = 0.0;
    res->zero = 0;
    const bool assigned = cls || K == 1u;
    for (uint64_t g = 0; g < cols; g++) {
        const uint32_t kb = assigned ? (cls ? cls[g] : 0u) : 0u, ke = assigned ? kb + 1u : K;
        double mant[PS_MODEL_MAX_CATEGORIES] = {}, post[PS_MODEL_MAX_CATEGORIES] = {};
        int32_t ex[PS_MODEL_MAX_CATEGORIES] = {};
        for (uint32_t k = kb; k < ke; k++) {
            double *Lk = &L[(size_t)k * 2 * nodes];
            int32_t *Ek = &E[(size_t)k * nodes];
            const double *xk = x + (size_t)k * 2 * nodes, *yk = xk + nodes;
            for (uint32_t i = 0; i < N; i++) ps_gene_leaf(rows[(uint64_t)i * cols + g] != 0, &Lk[2u * i]);
            for (uint32_t j = 0; j < M; j++) {
                const uint32_t l = left[j], r = right[j];
                double ml[2], mr[2];
                ps_gene_up(xk[l], yk[l], pi, &Lk[2u * l], ml);
                ps_gene_up(xk[r], yk[r], pi, &Lk[2u * r], mr);
                Ek[N + j] = (Ek[l] + Ek[r]) + ps_gene_join(ml, mr, &Lk[2u * (N + j)]);
            }
            mant[k] = ps_gene_site(rho, &Lk[2u * (nodes - 1u)]);
            ex[k] = Ek[nodes - 1u];
        }
        double sm, sr;
        int32_t se;
        if (assigned) {
            sm = mant[kb];
            se = ex[kb];
            sr = gh.a.rate[kb];
            post[kb] = 1.0;
        } else {
            sm = ps_subst_mix(K, gh.a.weight, mant, ex, &se, post);
            sr = ps_subst_mean_rate(K, post, gh.a.rate);
        }
        if (res->mant) res->mant[g] = sm;
        if (res->ex) res->ex[g] = se;
        if (res->rate) res->rate[g] = sr;
        if (res->post)
            for (uint32_t k = 0; k < K; k++) res->post[g * K + k] = post[k];
        res->lnl += ps_jc_site_ln(sm, se);
        if (!(sm > 0.0)) res->zero++;
        if (!down) continue;
        if (anc_rows)
            for (uint32_t j = 0; j < M; j++) anc_rows[(uint64_t)j * cols + g] = 0;
        double gg = 0.0, gl = 0.0, cg = 0.0, cl = 0.0;
        for (uint32_t k = kb; k < ke && sm > 0.0; k++) {
            const double *Lk = &L[(size_t)k * 2 * nodes], *xk = x + (size_t)k * 2 * nodes, *yk = xk + nodes;
            const bool first = k == kb, last = k + 1u == ke;
            for (uint32_t j = M; j-- > 0;) {
                const uint32_t l = left[j], r = right[j], c = N + j;
                double T[2] = { rho[0], rho[1] }, ml[2], mr[2], w[2];
                if (j != M - 1u) ps_gene_down(xk[c], yk[c], pi, &U[2u * c], T);
                ps_gene_up(xk[l], yk[l], pi, &Lk[2u * l], ml);
                ps_gene_up(xk[r], yk[r], pi, &Lk[2u * r], mr);
                const double sum = ps_gene_node_post(T, ml, mr, w);
                (void)ps_gene_join(mr, T, &U[2u * l]);
                (void)ps_gene_join(ml, T, &U[2u * r]);
                for (const uint32_t v : { l, r }) {
                    double ga, lo;
                    ps_gene_joints(xk[v], yk[v], pi, &U[2u * v], &Lk[2u * v], &ga, &lo);
                    ga = post[k] * ga;
                    lo = post[k] * lo;
                    res->bgain[v] += ga;
                    res->bloss[v] += lo;
                    gg = ps_gene_add(gg, ga, &cg);
                    gl = ps_gene_add(gl, lo, &cl);
                }
                double p0 = ps_subst_post_term(post[k], w[0], sum), p1 = ps_subst_post_term(post[k], w[1], sum);
                if (!first) {
                    p0 = acc[2u * j] + p0;
                    p1 = acc[2u * j + 1u] + p1;
                }
                acc[2u * j] = p0;
                acc[2u * j + 1u] = p1;
                if (!last) continue;
                double pmax;
                const uint32_t one = ps_gene_map(p0, p1, &pmax);
                res->conf[j] += pmax;
                res->ngenes[j] += p1;
                if (anc_rows) anc_rows[(uint64_t)j * cols + g] = (uint8_t)one;
            }
        }
        if (res->ggain) res->ggain[g] = gg + cg;
        if (res->gloss) res->gloss[g] = gl + cl;
    }
}

// One pass of the accessory handle p on its stream, complete when it returns.  made (null: no matrix): the new handle whose two
// views receive the states.  Timer groups: 0 the uploads, 1 the kernel (and the transpose), 2 the sum of the workgroups' rows.
static int gene_device_pass(ps_population *p, event_timer &tm, const pars_tree &t, const uint32_t *left, const uint32_t *right, const gene_host &gh,
                            const double *x, bool down, ps_population *made, gene_result *res)
{
    const uint32_t N = t.N, M = t.M, nodes = N + M, G = p->d.G, K = gh.K(), Wm = (M + 63u) / 64u;
    const bool mix = gh.mixture();
    PSCHK(use_device(p));
    const uint32_t *slot = nullptr;
    PSCHK(rows_current(p, &slot));
    pars_schedule sc;
    pars_make_schedule(t, left, right, slot, &sc);
    const uint32_t slots = sc.n_pad + M, stride = down ? 2u * slots + 2u * M + 1u : 1u;
    std::vector<double> xs((size_t)K * 2 * slots, 1.0);
    for (uint32_t k = 0; k < K; k++)
        for (uint32_t c = 0; c + 1u < nodes; c++) {
            xs[((size_t)k * 2) * slots + sc.slot_of[c]] = x[((size_t)k * 2) * nodes + c];
            xs[((size_t)k * 2 + 1) * slots + sc.slot_of[c]] = x[((size_t)k * 2 + 1) * nodes + c];
        }
    std::vector<uint32_t> node_of(M);
    for (uint32_t k = 0; k < M; k++) node_of[sc.slot_of[N + k] - sc.n_pad] = k;
    uint32_t sched_lds = 0;
    const uint32_t lds = gene_lds_bytes(N, t.levels, mix, &sched_lds);
    const uint32_t threads = p->gene_team ? p->gene_team : (N <= 256u ? 64u : 256u);
    const uint32_t per_cu = std::max(1u, std::min(threads == 64u ? 16u : 8u, (160u * 1024u) / (lds + 1024u + 512u)));
    const uint32_t grid = std::max(1u, std::min(G, 256u * per_cu));
    const uint8_t *cls = gh.gene_class;
    const bool want_gene = down && (res->ggain || res->gloss);
    scratch_layout lay;
    const uint64_t o_cnt = lay.add(8, 16), o_out = lay.add((uint64_t)stride * 8, 16);
    const uint64_t o_sched = lay.add((uint64_t)M * 4, 16), o_off = lay.add((uint64_t)sc.level_off.size() * 4, 16);
    const uint64_t o_node = lay.add((uint64_t)M * 4, 16);
    const uint64_t o_x = lay.add((uint64_t)K * 2 * slots * 8, 16), o_cls = lay.add(cls ? (uint64_t)G : 0, 16);
    const uint64_t o_mant = lay.add(res->mant ? (uint64_t)G * 8 : 0, 16), o_exp = lay.add(res->ex ? (uint64_t)G * 4 : 0, 16);
    const uint64_t o_post = lay.add(res->post ? (uint64_t)G * K * 8 : 0, 16), o_rate = lay.add(res->rate ? (uint64_t)G * 8 : 0, 16);
    const uint64_t o_gg = lay.add(want_gene ? (uint64_t)G * 8 : 0, 16), o_gl = lay.add(want_gene ? (uint64_t)G * 8 : 0, 16);
    const uint64_t o_part = lay.add((uint64_t)grid * stride * 8, 16);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(p->ro[PS_RO_GENE], lay.bytes, &base,
                      "cannot allocate the %llu bytes of the schedule, the x table and the sums of the gene model of a tree of %u merges over %u genes", M, G));
    hipStream_t st = p->stream;
    unsigned long long *d_cnt = (unsigned long long *)(base + o_cnt);
    double *d_out = (double *)(base + o_out), *d_x = (double *)(base + o_x), *d_part = (double *)(base + o_part);
    uint32_t *d_sched = (uint32_t *)(base + o_sched), *d_off = (uint32_t *)(base + o_off), *d_node = (uint32_t *)(base + o_node);
    uint8_t *d_cls = cls && G ? base + o_cls : nullptr;
    gene_outputs o{};
    o.mant = res->mant ? (double *)(base + o_mant) : nullptr;
    o.ex = res->ex ? (int32_t *)(base + o_exp) : nullptr;
    o.post = res->post ? (double *)(base + o_post) : nullptr;
    o.rate = res->rate ? (double *)(base + o_rate) : nullptr;
    o.gains = want_gene ? (double *)(base + o_gg) : nullptr;
    o.losses = want_gene ? (double *)(base + o_gl) : nullptr;
    o.states = down && made ? made->G[0] : nullptr;
    // (the sources of the copies live until this function's last synchronisation)
    PSCHK(tm.timed(0, st, [&]() -> int {
        HIPCHK(hipMemsetAsync(d_cnt, 0, o_sched, st));
        HIPCHK(hipMemcpyAsync(d_sched, sc.sched.data(), (uint64_t)M * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_off, sc.level_off.data(), (uint64_t)sc.level_off.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_node, node_of.data(), (uint64_t)M * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_x, xs.data(), (uint64_t)K * 2 * slots * 8, hipMemcpyHostToDevice, st));
        if (d_cls) HIPCHK(hipMemcpyAsync(d_cls, cls, G, hipMemcpyHostToDevice, st));
        return PS_OK;
    }));
    if (G) {
        auto kern = mix ? (down ? tree_gene_kernel<true, true> : tree_gene_kernel<true, false>)
                        : (down ? tree_gene_kernel<false, true> : tree_gene_kernel<false, false>);
        if (lds > 32768u) HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        PSCHK(tm.timed(1, st, [&]() -> int {
            PSCHK(ensure_gene_major(p, st));
            hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, (const uint64_t *)p->G[0], p->d.W, N, G, (const uint32_t *)d_sched,
                               (const uint32_t *)d_off, t.levels, M, sc.n_pad, (const double *)d_x, sched_lds, gh.a, (const uint8_t *)d_cls,
                               (const uint32_t *)d_node, Wm, o, d_part, stride, d_cnt);
            HIPCHK(hipGetLastError());
            if (o.states) {
                gene_g_to_i_kernel<<<dim3(made->d.W, made->d.GW), 64, 0, st>>>(made->G[0], made->I[made->cur], made->d);
                HIPCHK(hipGetLastError());
            }
            return PS_OK;
        }));
        PSCHK(tm.timed(2, st, [&]() -> int {
            hipLaunchKernelGGL(lik_reduce_kernel, dim3((stride + 255u) / 256u), dim3(256), 0, st, (const double *)d_part, grid, stride, d_out);
            HIPCHK(hipGetLastError());
            return PS_OK;
        }));
    }
    unsigned long long cnt = 0;
    std::vector<double> out(stride);
    HIPCHK(hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out.data(), d_out, (uint64_t)stride * 8, hipMemcpyDeviceToHost, st));
    if (G && o.mant) HIPCHK(hipMemcpyAsync(res->mant, o.mant, (uint64_t)G * 8, hipMemcpyDeviceToHost, st));
    if (G && o.ex) HIPCHK(hipMemcpyAsync(res->ex, o.ex, (uint64_t)G * 4, hipMemcpyDeviceToHost, st));
    if (G && o.post) HIPCHK(hipMemcpyAsync(res->post, o.post, (uint64_t)G * K * 8, hipMemcpyDeviceToHost, st));
    if (G && o.rate) HIPCHK(hipMemcpyAsync(res->rate, o.rate, (uint64_t)G * 8, hipMemcpyDeviceToHost, st));
    if (G && o.gains && res->ggain) HIPCHK(hipMemcpyAsync(res->ggain, o.gains, (uint64_t)G * 8, hipMemcpyDeviceToHost, st));
    if (G && o.losses && res->gloss) HIPCHK(hipMemcpyAsync(res->gloss, o.losses, (uint64_t)G * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    res->lnl = out[stride - 1u];
    res->zero = cnt;
    res->conf.assign(down ? M : 0, 0.0);
    res->ngenes.assign(down ? M : 0, 0.0);
    res->bgain.assign(down ? nodes : 0, 0.0);
    res->bloss.assign(down ? nodes : 0, 0.0);
    if (down) {
        for (uint32_t c = 0; c + 1u < nodes; c++) {
            res->bgain[c] = out[sc.slot_of[c]];
            res->bloss[c] = out[(size_t)slots + sc.slot_of[c]];
        }
        for (uint32_t k = 0; k < M; k++) {
            const uint32_t j = sc.slot_of[N + k] - sc.n_pad;
            res->conf[k] = out[(size_t)2 * slots + j];
            res->ngenes[k] = out[(size_t)2 * slots + M + j];
        }
    }
    return PS_OK;
}

static void gene_summary(ps_gene_t *o, const pars_tree &t, const gene_host &gh, uint64_t genes, uint64_t clamped, const gene_result &res)
{
    memset(o, 0, sizeof *o);
    o->pop_size = t.N;
    o->genes = genes;
    o->merges = t.M;
    o->categories = gh.K();
    o->classed = gh.gene_class ? 1 : 0;
    o->zero_genes = res.zero;
    o->clamped_lengths = clamped;
    o->lnl = o->start_lnl = res.lnl;
    o->beta = gh.beta;
    o->mean_rate = gh.mean_rate;
    double conf = 0.0;
    for (double v : res.bgain) o->total_gains += v;
    for (double v : res.bloss) o->total_losses += v;
    for (double v : res.conf) conf += v;
    for (double v : res.ngenes) o->total_genes += v;
    const uint64_t counted = genes - res.zero;
    o->mean_conf = counted && !res.conf.empty() ? conf / ((double)t.M * (double)counted) : 0.0;
}

// ---- the fit ----
// A one-dimensional search for the maximum of f over u in [lo, hi], fed one value at a time: next() is the point to evaluate,
// give() takes its value.  From u0 with f(u0) known: steps of h that double, towards the better side, until the value falls
// (the bracket a < b < c with f(b) the best); then golden section on [a, c] until c - a < tol.  best_u / best_f: the best point
// given so far (the start included), so the result is never below the start.
struct gene_search {
    double lo, hi, tol, h;
    double a, fa, b, fb, c, fc;      // the bracket (b the best of the three)
    double best_u, best_f, trial = 0.0;
    int phase = 0;                   // 0: first step up, 1: first step down, 2: expanding, 3: golden section, 4: done
    int dir = 1, steps = 0;
    void start(double u0, double f0, double lo_, double hi_, double h_, double tol_)
    {
        lo = lo_;
        hi = hi_;
        h = h_;
        tol = tol_;
        u0 = u0 < lo ? lo : (u0 > hi ? hi : u0);
        b = best_u = u0;
        fb = best_f = f0;
        phase = 0;
        steps = 0;
        set_trial(std::min(hi, u0 + h));
    }
    bool done() const { return phase == 4; }
    void set_trial(double u)
    {
        trial = u;
        if (u == b || (phase == 3 && !(c - a > tol)) || steps >= 80) phase = 4;
    }
    double next() const { return done() ? best_u : trial; }
    void golden()
    {
        // the larger of the two parts of the bracket is cut at its golden point from b
        const double g = 0.3819660112501051;
        set_trial(c - b > b - a ? b + g * (c - b) : b - g * (b - a));
    }
    void give(double f)
    {
        if (done()) return;
        steps++;
        const double u = trial;
        if (f > best_f) {
            best_f = f;
            best_u = u;
        }
        if (phase == 0) {
            if (f > fb) {                // upwards is better: expand upwards
                a = b;
                fa = fb;
                b = u;
                fb = f;
                dir = 1;
                phase = 2;
                h *= 2.0;
                set_trial(std::min(hi, b + h));
                if (done()) phase = 4;
            } else {
                c = u;
                fc = f;
                phase = 1;
                set_trial(std::max(lo, b - h));
                if (done()) {            // (u0 sits on the lower bound)
                    a = b;
                    fa = fb;
                }
            }
            return;
        }
        if (phase == 1) {
            if (f > fb) {                // downwards is better: the old middle becomes the upper end
                c = b;
                fc = fb;
                b = u;
                fb = f;
                dir = -1;
                phase = 2;
                h *= 2.0;
                set_trial(std::max(lo, b - h));
            } else {
                a = u;
                fa = f;
                phase = 3;
                golden();
            }
            return;
        }
        if (phase == 2) {
            if (f > fb) {
                if (dir > 0) {
                    a = b;
                    fa = fb;
                } else {
                    c = b;
                    fc = fb;
                }
                b = u;
                fb = f;
                h *= 2.0;
                set_trial(dir > 0 ? std::min(hi, b + h) : std::max(lo, b - h));
            } else {
                if (dir > 0) {
                    c = u;
                    fc = f;
                } else {
                    a = u;
                    fa = f;
                }
                phase = 3;
                golden();
            }
            return;
        }
        // golden section: u lies in (a, b) or (b, c)
        if (u > b) {
            if (f > fb) {
                a = b;
                fa = fb;
                b = u;
                fb = f;
            } else {
                c = u;
                fc = f;
            }
        } else {
            if (f > fb) {
                c = b;
                fc = fb;
                b = u;
                fb = f;
            } else {
                a = u;
                fa = f;
            }
        }
        golden();
    }
};

#define PS_GENE_FIT_LN_RATE_MIN (-34.5)        /* r from 1e-15 ... */
#define PS_GENE_FIT_LN_RATE_MAX 34.5           /* ... to 1e15 */
#define PS_GENE_FIT_LOGIT_MAX 20.7             /* pi_1 from 1e-9 to 1 - 1e-9 */
#define PS_GENE_FIT_TOL 1e-4                   /* the width at which a golden section ends, in ln r and in logit pi_1 */
#define PS_GENE_FIT_EM_STEPS 8u

static int gene_fit(const char *call, const gene_pass_fn &pass, const pars_tree &t, uint64_t genes, uint64_t clamped, const gene_host &start,
                    const ps_gene_fit_params *prm, ps_gene_t *out, double *rate_out, double *weight_out, double *freq_out, double *round_lnl,
                    uint64_t round_cap)
{
    if (!prm || !out) return ps_fail(PS_ERR_INVALID, "null argument");
    if (prm->max_rounds < 1) return ps_fail(PS_ERR_INVALID, "%s: max_rounds must be >= 1", call);
    if (!(prm->eps_lnl > 0.0) || !std::isfinite(prm->eps_lnl)) return ps_fail(PS_ERR_INVALID, "%s: eps_lnl must be a number > 0, not %g", call, prm->eps_lnl);
    if (prm->fit_rates > 1u || prm->fit_freq > 1u || prm->fit_weights > 1u) return ps_fail(PS_ERR_INVALID, "%s: fit_rates, fit_freq and fit_weights are 0 or 1", call);
    const uint32_t K = start.K();
    const bool assigned = !start.mixture();
    gene_host cur = start;
    std::vector<double> mant(std::max<uint64_t>(genes, 1)), post(std::max<uint64_t>(genes, 1) * K);
    std::vector<int32_t> ex(std::max<uint64_t>(genes, 1));
    uint64_t passes = 0, zero = 0;
    // one up pass under gh -> lnL (the genes in ascending order) and, assigned, lnL of every class; `post` is the pass's
    auto evaluate = [&](gene_host &gh, double *lnl, double *lnl_k) -> int {
        gh.beta = ps_gene_beta(gh.a.freq);
        gh.mean_rate = 0.0;
        for (uint32_t k = 0; k < K; k++) gh.mean_rate += gh.a.weight[k] * gh.a.rate[k];
        gene_result res;
        res.mant = mant.data();
        res.ex = ex.data();
        res.post = post.data();
        PSCHK(pass(gh, false, &res));
        passes++;
        zero = res.zero;
        double s = 0.0, sk[PS_MODEL_MAX_CATEGORIES] = {};
        for (uint64_t g = 0; g < genes; g++) {
            const double l = ps_jc_site_ln(mant[g], ex[g]);
            s += l;
            if (lnl_k) sk[gh.gene_class ? gh.gene_class[g] : 0u] += l;
        }
        *lnl = s;
        if (lnl_k) memcpy(lnl_k, sk, sizeof sk);
        return PS_OK;
    };
    double lnl = 0.0, lnl_k[PS_MODEL_MAX_CATEGORIES] = {};
    PSCHK(evaluate(cur, &lnl, assigned ? lnl_k : nullptr));
    const double start_lnl = lnl;
    if (std::isnan(lnl)) return ps_fail(PS_ERR_INVALID, "%s: lnL of the start model is not a number", call);
    uint64_t rounds = 0, converged = 0;
    if (round_lnl && round_cap) round_lnl[0] = lnl;
    for (uint32_t r = 0; r < prm->max_rounds; r++) {
        const double before = lnl;
        if (prm->fit_rates && assigned) {
            // K searches in lockstep: one pass evaluates one trial rate of every class
            gene_search s[PS_MODEL_MAX_CATEGORIES];
            bool any = false;
            for (uint32_t k = 0; k < K; k++) {
                s[k].phase = 4;
                s[k].best_u = 0.0;
                if (cur.a.rate[k] > 0.0) {
                    s[k].start(log(cur.a.rate[k]), lnl_k[k], PS_GENE_FIT_LN_RATE_MIN, PS_GENE_FIT_LN_RATE_MAX, 0.6931471805599453, PS_GENE_FIT_TOL);
                    any = any || !s[k].done();
                }
            }
            while (any) {
                gene_host trial = cur;
                for (uint32_t k = 0; k < K; k++)
                    if (cur.a.rate[k] > 0.0) trial.a.rate[k] = exp(s[k].next());
                double tl, tk[PS_MODEL_MAX_CATEGORIES];
                PSCHK(evaluate(trial, &tl, tk));
                any = false;
                for (uint32_t k = 0; k < K; k++) {
                    s[k].give(tk[k]);
                    any = any || !s[k].done();
                }
            }
            gene_host trial = cur;
            bool moved = false;
            for (uint32_t k = 0; k < K; k++)
                if (cur.a.rate[k] > 0.0 && s[k].best_f > lnl_k[k]) {
                    trial.a.rate[k] = exp(s[k].best_u);
                    moved = true;
                }
            if (moved) {
                double tl, tk[PS_MODEL_MAX_CATEGORIES];
                PSCHK(evaluate(trial, &tl, tk));
                if (tl >= lnl) {
                    cur = trial;
                    lnl = tl;
                    memcpy(lnl_k, tk, sizeof tk);
                }
            }
        } else if (prm->fit_rates) {
            // a mixture: the rates in turn on the whole lnL
            for (uint32_t k = 0; k < K; k++) {
                if (!(cur.a.rate[k] > 0.0)) continue;
                gene_search s;
                s.start(log(cur.a.rate[k]), lnl, PS_GENE_FIT_LN_RATE_MIN, PS_GENE_FIT_LN_RATE_MAX, 0.6931471805599453, PS_GENE_FIT_TOL);
                while (!s.done()) {
                    gene_host trial = cur;
                    trial.a.rate[k] = exp(s.next());
                    double tl;
                    PSCHK(evaluate(trial, &tl, nullptr));
                    s.give(tl);
                }
                if (s.best_f > lnl) {
                    gene_host trial = cur;
                    trial.a.rate[k] = exp(s.best_u);
                    double tl;
                    PSCHK(evaluate(trial, &tl, nullptr));
                    if (tl >= lnl) {
                        cur = trial;
                        lnl = tl;
                    }
                }
            }
        }
        if (prm->fit_weights && !assigned && genes) {
            // EM on the weights: w_k <- mean_g post_gk under the current model, while each update raises lnL
            double tl;
            PSCHK(evaluate(cur, &tl, nullptr));                  // (the posteriors of the current model)
            for (uint32_t it = 0; it < PS_GENE_FIT_EM_STEPS; it++) {
                gene_host trial = cur;
                double sum = 0.0;
                for (uint32_t k = 0; k < K; k++) {
                    double w = 0.0;
                    for (uint64_t g = 0; g < genes; g++) w += post[g * K + k];
                    w /= (double)genes;
                    trial.a.weight[k] = w > 1e-300 ? w : 1e-300;
                    sum += trial.a.weight[k];
                }
                for (uint32_t k = 0; k < K; k++) trial.a.weight[k] /= sum;
                PSCHK(evaluate(trial, &tl, nullptr));            // (leaves the posteriors of the trial for the next update)
                if (!(tl > lnl)) break;
                cur = trial;
                lnl = tl;
            }
        }
        if (prm->fit_freq) {
            gene_search s;
            s.start(log(cur.a.freq[1] / cur.a.freq[0]), lnl, -PS_GENE_FIT_LOGIT_MAX, PS_GENE_FIT_LOGIT_MAX, 0.5, PS_GENE_FIT_TOL);
            auto with_logit = [&](double u) {
                gene_host trial = cur;
                const double p1 = 1.0 / (1.0 + exp(-u));
                trial.a.freq[1] = p1;
                trial.a.freq[0] = 1.0 - p1;
                return trial;
            };
            while (!s.done()) {
                gene_host trial = with_logit(s.next());
                double tl;
                PSCHK(evaluate(trial, &tl, nullptr));
                s.give(tl);
            }
            if (s.best_f > lnl) {
                gene_host trial = with_logit(s.best_u);
                double tl, tk[PS_MODEL_MAX_CATEGORIES];
                PSCHK(evaluate(trial, &tl, assigned ? tk : nullptr));
                if (tl >= lnl) {
                    cur = trial;
                    lnl = tl;
                    if (assigned) memcpy(lnl_k, tk, sizeof tk);
                }
            }
        }
        rounds++;
        if (round_lnl && rounds < round_cap) round_lnl[rounds] = lnl;
        if (!(lnl - before >= prm->eps_lnl)) {
            converged = 1;
            break;
        }
    }
    // the returned model's own pass: its counters and lnL
    PSCHK(evaluate(cur, &lnl, nullptr));
    gene_result res;
    res.lnl = lnl;
    res.zero = zero;
    gene_summary(out, t, cur, genes, clamped, res);
    out->start_lnl = start_lnl;
    out->rounds = rounds;
    out->passes = passes;
    out->converged = converged;
    if (round_lnl && rounds < round_cap) round_lnl[rounds] = lnl;
    if (rate_out) memcpy(rate_out, cur.a.rate, K * sizeof(double));
    if (weight_out) memcpy(weight_out, cur.a.weight, K * sizeof(double));
    if (freq_out) memcpy(freq_out, cur.a.freq, 2 * sizeof(double));
    return PS_OK;
}

// ---- the host entries ----
struct gene_frame {
    gene_host gh;
    pars_tree t;
    std::vector<double> used;
    uint64_t clamped = 0;
};

static int gene_frame_make(const char *call, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges, uint64_t pop_size,
                           uint64_t genes, const ps_gene_model *model, gene_frame *f)
{
    PSCHK(gene_model_check(call, model, genes, &f->gh));
    PSCHK(gene_check_tree(call, left, right, merges, pop_size, f->gh, &f->t));
    return gene_used_lengths(call, f->t, length, &f->used, &f->clamped);
}

static gene_pass_fn gene_host_fn(const uint8_t *rows, uint64_t cols, const gene_frame &f, const uint32_t *left, const uint32_t *right, uint8_t *anc_rows)
{
    return [=, &f](const gene_host &gh, bool down, gene_result *res) -> int {
        std::vector<double> x;
        gene_x(gh, f.used, &x);
        gene_host_pass(rows, cols, f.t, left, right, gh, x.data(), down, anc_rows, res);
        return PS_OK;
    };
}

// the optional outputs of the ancestral call
struct gene_anc_outputs {
    double *node_conf, *node_genes, *branch_gains, *branch_losses, *gene_gains, *gene_losses;
};

static void gene_anc_copy(const gene_anc_outputs &o, const gene_result &res)
{
    if (o.node_conf) memcpy(o.node_conf, res.conf.data(), res.conf.size() * sizeof(double));
    if (o.node_genes) memcpy(o.node_genes, res.ngenes.data(), res.ngenes.size() * sizeof(double));
    if (o.branch_gains) memcpy(o.branch_gains, res.bgain.data(), res.bgain.size() * sizeof(double));
    if (o.branch_losses) memcpy(o.branch_losses, res.bloss.data(), res.bloss.size() * sizeof(double));
}

extern "C" int ps_gene_likelihood_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                            const double *length, uint64_t merges, const ps_gene_model *model, ps_gene_t *out, double *gene_mant,
                                            int32_t *gene_exp, double *gene_post, double *gene_rate)
{
    const char *call = "ps_gene_likelihood_from_rows";
    if (!out || (!rows && cols)) return ps_fail(PS_ERR_INVALID, "null argument");
    gene_frame f;
    PSCHK(gene_frame_make(call, left, right, length, merges, pop_size, cols, model, &f));
    gene_result res;
    res.mant = gene_mant;
    res.ex = gene_exp;
    res.post = gene_post;
    res.rate = gene_rate;
    PSCHK(gene_host_fn(rows, cols, f, left, right, nullptr)(f.gh, false, &res));
    gene_summary(out, f.t, f.gh, cols, f.clamped, res);
    return PS_OK;
}

extern "C" int ps_gene_ancestral_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                           const double *length, uint64_t merges, const ps_gene_model *model, ps_gene_t *out, uint8_t *anc_rows,
                                           double *node_conf, double *node_genes, double *branch_gains, double *branch_losses, double *gene_gains,
                                           double *gene_losses)
{
    const char *call = "ps_gene_ancestral_from_rows";
    if (!out || (!rows && cols)) return ps_fail(PS_ERR_INVALID, "null argument");
    gene_frame f;
    PSCHK(gene_frame_make(call, left, right, length, merges, pop_size, cols, model, &f));
    gene_result res;
    res.ggain = gene_gains;
    res.gloss = gene_losses;
    PSCHK(gene_host_fn(rows, cols, f, left, right, anc_rows)(f.gh, true, &res));
    gene_summary(out, f.t, f.gh, cols, f.clamped, res);
    gene_anc_copy({ node_conf, node_genes, branch_gains, branch_losses, gene_gains, gene_losses }, res);
    return PS_OK;
}

extern "C" int ps_gene_fit_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                     const double *length, uint64_t merges, const ps_gene_model *model, const ps_gene_fit_params *prm, ps_gene_t *out,
                                     double *rate_out, double *weight_out, double *freq_out, double *round_lnl, uint64_t round_cap)
{
    const char *call = "ps_gene_fit_from_rows";
    if (!out || (!rows && cols)) return ps_fail(PS_ERR_INVALID, "null argument");
    gene_frame f;
    PSCHK(gene_frame_make(call, left, right, length, merges, pop_size, cols, model, &f));
    return gene_fit(call, gene_host_fn(rows, cols, f, left, right, nullptr), f.t, cols, f.clamped, f.gh, prm, out, rate_out, weight_out, freq_out,
                    round_lnl, round_cap);
}

// ---- the device entries ----
// what kind of call: the likelihood, the reconstruction, the fit
struct gene_call {
    const char *name;
    ps_gene_t *out;
    // the likelihood
    double *gene_mant = nullptr;
    int32_t *gene_exp = nullptr;
    double *gene_post = nullptr, *gene_rate = nullptr;
    // the reconstruction
    bool down = false;
    ps_population **anc = nullptr;
    gene_anc_outputs ao{};
    // the fit
    const ps_gene_fit_params *prm = nullptr;
    double *rate_out = nullptr, *weight_out = nullptr, *freq_out = nullptr, *round_lnl = nullptr;
    uint64_t round_cap = 0;
};

static int gene_run(ps_population *acc, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges, const ps_gene_model *model,
                    const gene_call &c)
{
    if (c.anc) *c.anc = nullptr;
    if (!c.out) return ps_fail(PS_ERR_INVALID, "null argument");
    if (acc->cfg.core) return ps_fail(PS_ERR_INVALID, "%s takes an accessory handle, not a core handle", c.name);
    gene_frame f;
    PSCHK(gene_frame_make(c.name, left, right, length, merges, acc->cfg.pop_size, acc->d.G, model, &f));   // (fails before any device work)
    PSCHK(use_device(acc));
    HIPCHK(hipStreamSynchronize(acc->stream));
    acc->ro[PS_RO_GENE].timed = false;
    ps_population *made = nullptr;
    if (c.anc) PSCHK(sample_make(acc, f.t.M, 0, acc->cfg.ncols, &made));
    event_timer tm;
    gene_pass_fn pass = [&](const gene_host &gh, bool down, gene_result *res) -> int {
        std::vector<double> x;
        gene_x(gh, f.used, &x);
        return gene_device_pass(acc, tm, f.t, left, right, gh, x.data(), down, made, res);
    };
    int rc;
    gene_result res;
    if (c.prm) {
        rc = gene_fit(c.name, pass, f.t, acc->d.G, f.clamped, f.gh, c.prm, c.out, c.rate_out, c.weight_out, c.freq_out, c.round_lnl, c.round_cap);
    } else {
        res.mant = c.gene_mant;
        res.ex = c.gene_exp;
        res.post = c.gene_post;
        res.rate = c.gene_rate;
        res.ggain = c.ao.gene_gains;
        res.gloss = c.ao.gene_losses;
        rc = pass(f.gh, c.down, &res);
    }
    if (rc == PS_OK) rc = use_device(acc);
    if (rc == PS_OK) rc = tm.collect(acc->ro[PS_RO_GENE], 3);
    if (rc != PS_OK) {
        const std::string keep = g_err;
        if (made) ps_population_destroy(made);
        g_err = keep;
        return rc;
    }
    if (!c.prm) {
        gene_summary(c.out, f.t, f.gh, acc->d.G, f.clamped, res);
        if (c.down) gene_anc_copy(c.ao, res);
    }
    if (made) {
        made->g_valid = true;               // (the kernel wrote the gene-major view, the transpose the rows)
        made->counts_fresh = false;
        made->edit_epoch++;
        *c.anc = made;
    }
    return PS_OK;
}

extern "C" int ps_tree_gene_likelihood(ps_population *acc, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                       const ps_gene_model *model, ps_gene_t *out, double *gene_mant, int32_t *gene_exp, double *gene_post,
                                       double *gene_rate)
{
    PSCHK(ps_needs_device());
    if (!acc) return ps_fail(PS_ERR_INVALID, "null argument");
    gene_call c{ "ps_tree_gene_likelihood", out };
    c.gene_mant = gene_mant;
    c.gene_exp = gene_exp;
    c.gene_post = gene_post;
    c.gene_rate = gene_rate;
    return gene_run(acc, left, right, length, merges, model, c);
}

extern "C" int ps_tree_gene_ancestral(ps_population *acc, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                      const ps_gene_model *model, ps_gene_t *out, ps_population **anc, double *node_conf, double *node_genes,
                                      double *branch_gains, double *branch_losses, double *gene_gains, double *gene_losses)
{
    if (anc) *anc = nullptr;
    PSCHK(ps_needs_device());
    if (!acc) return ps_fail(PS_ERR_INVALID, "null argument");
    gene_call c{ "ps_tree_gene_ancestral", out };
    c.down = true;
    c.anc = anc;
    c.ao = { node_conf, node_genes, branch_gains, branch_losses, gene_gains, gene_losses };
    return gene_run(acc, left, right, length, merges, model, c);
}

extern "C" int ps_tree_gene_fit(ps_population *acc, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                const ps_gene_model *model, const ps_gene_fit_params *prm, ps_gene_t *out, double *rate_out, double *weight_out,
                                double *freq_out, double *round_lnl, uint64_t round_cap)
{
    PSCHK(ps_needs_device());
    if (!acc || !prm) return ps_fail(PS_ERR_INVALID, "null argument");
    gene_call c{ "ps_tree_gene_fit", out };
    c.prm = prm;
    c.rate_out = rate_out;
    c.weight_out = weight_out;
    c.freq_out = freq_out;
    c.round_lnl = round_lnl;
    c.round_cap = round_cap;
    return gene_run(acc, left, right, length, merges, model, c);
}

// the accessory handle a run answers with: a simulation's own, shard 0's replica of a sharded run (the shards' accessory matrices
// are bit-identical); everything queued on the run is complete first
static int gene_sim_acc(ps_sim *s, ps_population **acc)
{
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(ps_sim_sync(s));
    *acc = s->acc;
    return PS_OK;
}

static int gene_multi_acc(ps_multi *m, ps_population **acc)
{
    if (!m) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(ps_multi_sync(m));
    *acc = m->shard[0]->acc;
    return PS_OK;
}

extern "C" int ps_sim_tree_gene_likelihood(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                           const ps_gene_model *model, ps_gene_t *out, double *gene_mant, int32_t *gene_exp, double *gene_post,
                                           double *gene_rate)
{
    PSCHK(ps_needs_device());
    ps_population *acc = nullptr;
    PSCHK(gene_sim_acc(s, &acc));
    return ps_tree_gene_likelihood(acc, left, right, length, merges, model, out, gene_mant, gene_exp, gene_post, gene_rate);
}

extern "C" int ps_multi_tree_gene_likelihood(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                             const ps_gene_model *model, ps_gene_t *out, double *gene_mant, int32_t *gene_exp, double *gene_post,
                                             double *gene_rate)
{
    PSCHK(ps_needs_device());
    ps_population *acc = nullptr;
    PSCHK(gene_multi_acc(m, &acc));
    return ps_tree_gene_likelihood(acc, left, right, length, merges, model, out, gene_mant, gene_exp, gene_post, gene_rate);
}

extern "C" int ps_sim_tree_gene_ancestral(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                          const ps_gene_model *model, ps_gene_t *out, ps_population **anc, double *node_conf, double *node_genes,
                                          double *branch_gains, double *branch_losses, double *gene_gains, double *gene_losses)
{
    if (anc) *anc = nullptr;
    PSCHK(ps_needs_device());
    ps_population *acc = nullptr;
    PSCHK(gene_sim_acc(s, &acc));
    return ps_tree_gene_ancestral(acc, left, right, length, merges, model, out, anc, node_conf, node_genes, branch_gains, branch_losses, gene_gains,
                                  gene_losses);
}

extern "C" int ps_multi_tree_gene_ancestral(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                            const ps_gene_model *model, ps_gene_t *out, ps_population **anc, double *node_conf, double *node_genes,
                                            double *branch_gains, double *branch_losses, double *gene_gains, double *gene_losses)
{
    if (anc) *anc = nullptr;
    PSCHK(ps_needs_device());
    ps_population *acc = nullptr;
    PSCHK(gene_multi_acc(m, &acc));
    return ps_tree_gene_ancestral(acc, left, right, length, merges, model, out, anc, node_conf, node_genes, branch_gains, branch_losses, gene_gains,
                                  gene_losses);
}

extern "C" int ps_sim_tree_gene_fit(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                    const ps_gene_model *model, const ps_gene_fit_params *prm, ps_gene_t *out, double *rate_out, double *weight_out,
                                    double *freq_out, double *round_lnl, uint64_t round_cap)
{
    PSCHK(ps_needs_device());
    ps_population *acc = nullptr;
    PSCHK(gene_sim_acc(s, &acc));
    return ps_tree_gene_fit(acc, left, right, length, merges, model, prm, out, rate_out, weight_out, freq_out, round_lnl, round_cap);
}

extern "C" int ps_multi_tree_gene_fit(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                      const ps_gene_model *model, const ps_gene_fit_params *prm, ps_gene_t *out, double *rate_out, double *weight_out,
                                      double *freq_out, double *round_lnl, uint64_t round_cap)
{
    PSCHK(ps_needs_device());
    ps_population *acc = nullptr;
    PSCHK(gene_multi_acc(m, &acc));
    return ps_tree_gene_fit(acc, left, right, length, merges, model, prm, out, rate_out, weight_out, freq_out, round_lnl, round_cap);
}

extern "C" int ps_tree_gene_timing(ps_population *acc, double *upload_ms, double *pass_ms, double *reduce_ms)
{
    if (!acc) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(acc->ro[PS_RO_GENE], "no gene model has been computed on this handle", { upload_ms, pass_ms, reduce_ms });
}
