// bootstrap_support.h -- ps_bootstrap_support / ps_sim_bootstrap_support / ps_multi_bootstrap_support, the draw rule restated
// (ps_bootstrap_sites) and the clade counting alone (ps_bootstrap_from_merges) (include/pansim_hip.h; the definitions:
// docs/BOOTSTRAP_SUPPORT.md).  Included by pansim_capi.hip behind neighbour_joining.h: the three trees' device bodies
// (tree_device, upgma_device, nj_device) run here as they are, first on the band source of the matrix -- the reference tree --
// and then, per replicate, on the same source bound to the replicate's site lists (core_band_source::bind).
//
// Per replicate and core handle: the sites drawn (or read from the caller's list) and counted, scanned and expanded into an
// ascending list (bootstrap_kernels.h); the strings packed through the list; the method's body; one copy of its merge list;
// the counting on the host.  The counting lays the reference tree's leaves out in its dendrogram order with leaf 0 first, so
// that every set it looks for is an interval, and finds an interval through two tables without a hash (boot_counter).
#pragma once

#include "bootstrap_kernels.h"
#include "bootstrap_count.h"

static_assert(PS_BOOT_LINKAGE == 0 && PS_BOOT_UPGMA == 1 && PS_BOOT_NJ == 2, "the methods of ps_bootstrap_params");

extern "C" int ps_bootstrap_sites(uint64_t seed, uint32_t replicate, uint64_t core_sites, uint64_t draws, uint64_t first, uint64_t count,
                                  uint32_t *out_sites)
{
    if (count && !out_sites) return ps_fail(PS_ERR_INVALID, "null argument");
    if (core_sites < 1 || core_sites >= (1ull << 32)) return ps_fail(PS_ERR_INVALID, "the bootstrap's draw needs 1 <= core_sites < 2^32, not %llu", (unsigned long long)core_sites);
    if (draws < 1 || draws >= (1ull << 31)) return ps_fail(PS_ERR_INVALID, "the bootstrap's draw needs 1 <= draws < 2^31, not %llu", (unsigned long long)draws);
    if (first > draws || count > draws - first)
        return ps_fail(PS_ERR_INVALID, "the draws [%llu, %llu + %llu) are not among the %llu of a replicate", (unsigned long long)first,
                       (unsigned long long)first, (unsigned long long)count, (unsigned long long)draws);
    for (uint64_t k = 0; k < count; k++)
        out_sites[k] = ps_boot_draw(first + k, replicate, (uint32_t)core_sites, (uint32_t)seed, (uint32_t)(seed >> 32));
    return PS_OK;
}

extern "C" int ps_bootstrap_from_merges(const uint32_t *ref_left, const uint32_t *ref_right, const uint32_t *rep_left, const uint32_t *rep_right,
                                        uint64_t replicates, uint64_t pop_size, int unrooted, uint32_t *support, uint32_t *shared)
{
    if (!ref_left || !ref_right || !support || (replicates && (!rep_left || !rep_right || !shared))) return ps_fail(PS_ERR_INVALID, "null argument");
    if (pop_size < 2 || pop_size > 0x7fffffffull) return ps_fail(PS_ERR_INVALID, "the bootstrap's counting needs 2 <= pop_size < 2^31");
    if (replicates >= (1ull << 32)) return ps_fail(PS_ERR_INVALID, "the bootstrap's counting needs fewer than 2^32 replicates");
    const uint32_t N = (uint32_t)pop_size;
    boot_counter cnt;
    PSCHK(cnt.init(ref_left, ref_right, N, unrooted != 0));
    memset(support, 0, (size_t)(N - 1u) * sizeof(uint32_t));
    for (uint64_t b = 0; b < replicates; b++)
        PSCHK(cnt.add(rep_left + b * (N - 1u), rep_right + b * (N - 1u), b, support, &shared[b]));
    return PS_OK;
}

// the parameters against the limits of the call and of its method; *draws: the draws of a replicate (0 asked: the core sites)
static int boot_check_params(const ps_bootstrap_params *prm, uint64_t N, uint64_t L, uint64_t cg, uint64_t *draws)
{
    const ps_tree_params tp = { PS_TREE_CORE };
    if (prm->method != PS_BOOT_LINKAGE && prm->method != PS_BOOT_UPGMA && prm->method != PS_BOOT_NJ)
        return ps_fail(PS_ERR_INVALID, "the method of bootstrap support is PS_BOOT_LINKAGE (0), PS_BOOT_UPGMA (1) or PS_BOOT_NJ (2), not %d", (int)prm->method);
    if (prm->method == PS_BOOT_UPGMA) PSCHK(upgma_check_limits(&tp, N, L, cg));
    if (prm->method == PS_BOOT_NJ) PSCHK(nj_check_limits(&tp, N, L, cg));
    if (prm->replicates < 1 || prm->replicates > 65535)
        return ps_fail(PS_ERR_INVALID, "bootstrap support needs 1 <= replicates <= 65535, not %u", prm->replicates);
    if (L < 1 || L >= (1ull << 32)) return ps_fail(PS_ERR_INVALID, "bootstrap support needs 1 <= core sites < 2^32, not %llu", (unsigned long long)L);
    *draws = prm->draws ? prm->draws : L;
    if (*draws >= (1ull << 31))
        return ps_fail(PS_ERR_INVALID, "bootstrap support needs 1 <= draws < 2^31 (the resampled count of a pair stays in 32 bits), not %llu",
                       (unsigned long long)*draws);
    return PS_OK;
}

// the scratch on one core handle: the total word, the counts of its sites, the block sums, the replicate's list (at most all
// draws), one replicate of the caller's lists (if there are any)
struct boot_scratch {
    uint32_t *total = nullptr, *w = nullptr, *bsum = nullptr, *list = nullptr, *sites = nullptr;
    uint32_t nblocks = 0;
};

static int boot_scratch_get(ps_population *c, uint64_t draws, bool supplied, boot_scratch *s)
{
    scratch_layout lay;
    const uint64_t ncols = c->cfg.ncols;
    s->nblocks = (uint32_t)((ncols + PS_BOOT_BLOCK - 1u) / PS_BOOT_BLOCK);
    const uint64_t o_total = lay.add(16, 16), o_w = lay.add(ncols * 4, 16), o_bsum = lay.add((uint64_t)s->nblocks * 4, 16);
    const uint64_t o_list = lay.add(draws * 4, 16), o_sites = lay.add(supplied ? draws * 4 : 0, 16);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(c->ro[PS_RO_BOOT], lay.bytes, &base, "cannot allocate the %llu bytes of the site lists of %llu draws", (unsigned long long)draws));
    s->total = (uint32_t *)(base + o_total);
    s->w = (uint32_t *)(base + o_w);
    s->bsum = (uint32_t *)(base + o_bsum);
    s->list = (uint32_t *)(base + o_list);
    s->sites = supplied ? (uint32_t *)(base + o_sites) : nullptr;
    return PS_OK;
}

// the list of replicate `rep` on handle c (its device current), on its stream: *n = the entries, read back
static int boot_build_list(ps_population *c, const boot_scratch &s, uint64_t seed, uint32_t rep, const uint32_t *sites, uint32_t L, uint32_t draws,
                           uint32_t *n)
{
    const uint32_t ncols = (uint32_t)c->cfg.ncols, off = (uint32_t)c->cfg.col_offset;
    hipStream_t st = c->stream;
    *n = 0;
    if (!ncols) return PS_OK;
    HIPCHK(hipMemsetAsync(s.w, 0, (uint64_t)ncols * sizeof(uint32_t), st));
    if (sites) {
        HIPCHK(hipMemcpyAsync(s.sites, sites, (uint64_t)draws * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        boot_list_kernel<<<std::max(1u, std::min((draws + 255u) / 256u, 4096u)), 256, 0, st>>>(s.sites, draws, off, ncols, s.w);
    } else {
        const uint32_t blocks = (draws + 1u) / 2u;
        boot_draw_kernel<<<std::max(1u, std::min((blocks + 255u) / 256u, 4096u)), 256, 0, st>>>((uint32_t)seed, (uint32_t)(seed >> 32), rep, draws, L, off,
                                                                                             ncols, s.w);
    }
    boot_block_sum_kernel<<<s.nblocks, 256, 0, st>>>(s.w, ncols, s.bsum);
    boot_scan_blocks_kernel<<<1, 256, 0, st>>>(s.bsum, s.nblocks, s.total);
    boot_expand_kernel<<<s.nblocks, 256, 0, st>>>(s.w, ncols, s.bsum, s.list, draws);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(n, s.total, sizeof *n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return PS_OK;
}

// what the trees return beside their merge lists, kept for the length of a call
struct boot_tree_tmp {
    std::vector<uint32_t> a, b;
    std::vector<uint64_t> num, den;
    std::vector<double> len_a, len_b;
    explicit boot_tree_tmp(uint32_t N) : a(N), b(N), num(N), den(N), len_a(N), len_b(N) {}
};

static int boot_method_slot(int32_t method) { return method == PS_BOOT_LINKAGE ? PS_RO_TREE : method == PS_BOOT_UPGMA ? PS_RO_UPGMA : PS_RO_NJ; }

// the tree of the method on whatever the source is bound to, as its own entry runs it -> the merge list
static int boot_tree(int32_t method, core_band_source &src, ps_population *acc, uint64_t L, const uint32_t *slot, uint32_t *left, uint32_t *right,
                     boot_tree_tmp &t)
{
    const ps_tree_params tp = { PS_TREE_CORE };
    const uint64_t N = src.c0->cfg.pop_size;
    if (method == PS_BOOT_UPGMA) {
        ps_upgma_t o;
        return upgma_device(src, acc, L, &tp, slot, &o, left, right, t.a.data(), t.num.data(), t.den.data());
    }
    if (method == PS_BOOT_NJ) {
        ps_nj_t o;
        return nj_device(src, acc, L, &tp, slot, &o, left, right, t.len_a.data(), t.len_b.data());
    }
    ps_tree_t o;
    uint64_t merges = 0;
    PSCHK(tree_device(src, acc, L, &tp, slot, &o, t.a.data(), t.b.data(), t.num.data(), t.den.data()));
    if (o.edges != N - 1) return ps_fail(PS_ERR_STATE, "the linkage tree of %llu individuals holds %llu edges", (unsigned long long)N, (unsigned long long)o.edges);
    return ps_merges_from_tree(t.a.data(), t.b.data(), o.edges, N, left, right, &merges);
}

// The call behind the device entries: src is open on the matrix in internal order, everything has been checked.
static int boot_device(core_band_source &src, ps_population *acc, uint64_t L, uint64_t draws, const ps_bootstrap_params *prm, const uint32_t *sites,
                       const uint32_t *slot, ps_bootstrap_t *out, uint32_t *left, uint32_t *right, uint32_t *support, uint32_t *shared)
{
    ps_population *c0 = src.c0;
    ps_multi *m = src.m;
    const uint32_t N = (uint32_t)c0->cfg.pop_size, R = prm->replicates;
    const size_t K = src.src.size();
    readout_slot &ro = c0->ro[PS_RO_BOOT], &ro_tree = c0->ro[boot_method_slot(prm->method)];
    ro.timed = false;
    std::vector<boot_scratch> sc(K);
    for (size_t k = 0; k < K; k++) {
        PSCHK(use_device(src.core(k)));
        PSCHK(boot_scratch_get(src.core(k), draws, sites != nullptr, &sc[k]));
    }
    PSCHK(use_device(c0));
    boot_tree_tmp t(N);
    PSCHK(boot_tree(prm->method, src, acc, L, slot, left, right, t));
    // (the method's own times stay those of the reference tree, on every way out)
    struct keep_times {
        readout_slot &ro;
        double ms[5];
        bool timed;
        explicit keep_times(readout_slot &r) : ro(r), timed(r.timed) { memcpy(ms, r.ms, sizeof ms); }
        ~keep_times()
        {
            memcpy(ro.ms, ms, sizeof ms);
            ro.timed = timed;
        }
    } keep(ro_tree);
    boot_counter cnt;
    PSCHK(cnt.init(left, right, N, prm->method == PS_BOOT_NJ));
    memset(support, 0, (size_t)(N - 1u) * sizeof(uint32_t));
    std::vector<uint32_t> rep_left(N), rep_right(N), n_list(K);
    std::vector<core_site_list> lists(K);
    double ms[3] = { 0.0, 0.0, 0.0 };
    for (uint32_t b = 0; b < R; b++) {
        // timer groups: 0 = the lists (shard 0's), 1 = the pack (shard 0's); the counts, the store and the tree in the method's own
        event_timer bt;
        const uint32_t *mine = sites ? sites + (uint64_t)b * draws : nullptr;
        auto build = [&](size_t k) -> int {
            ps_population *c = src.core(k);
            PSCHK(use_device(c));
            auto work = [&]() { return boot_build_list(c, sc[k], prm->seed, b, mine, (uint32_t)L, (uint32_t)draws, &n_list[k]); };
            return k == 0 ? bt.timed(0, c->stream, work) : work();
        };
        if (m) PSCHK(multi_for_each(m, build));
        else PSCHK(build(0));
        PSCHK(use_device(c0));
        uint64_t listed = 0;
        for (size_t k = 0; k < K; k++) {
            lists[k] = { sc[k].list, n_list[k] };
            listed += n_list[k];
        }
        if (listed != draws)
            return ps_fail(PS_ERR_STATE, "replicate %u lists %llu sites for %llu draws", b, (unsigned long long)listed, (unsigned long long)draws);
        PSCHK(bt.timed(1, c0->stream, [&]() { return src.bind(lists.data()); }));
        PSCHK(boot_tree(prm->method, src, acc, draws, slot, rep_left.data(), rep_right.data(), t));
        double lists_ms = 0.0, pack_ms = 0.0;
        PSCHK(bt.total_ms(0, &lists_ms));
        PSCHK(bt.total_ms(1, &pack_ms));
        ms[0] += lists_ms;
        ms[1] += pack_ms + ro_tree.ms[0] + ro_tree.ms[1];
        ms[2] += ro_tree.ms[2];
        PSCHK(cnt.add(rep_left.data(), rep_right.data(), b, support, &shared[b]));
    }
    readout_head(out, N, (uint64_t)N * (N - 1) / 2, L, acc->cfg.core_genes);
    out->method = (uint64_t)prm->method;
    out->replicates = R;
    out->draws = draws;
    out->merges = N - 1u;
    for (uint32_t k = 0; k + 1u < N; k++) {
        out->support_sum += support[k];
        if (k + 2u == N) break;                           // (the last merge holds all leaves)
        out->supported_50 += (uint64_t)support[k] * 100 >= 50ull * R;
        out->supported_70 += (uint64_t)support[k] * 100 >= 70ull * R;
        out->supported_95 += (uint64_t)support[k] * 100 >= 95ull * R;
    }
    for (int g = 0; g < 3; g++) ro.ms[g] = ms[g];
    ro.timed = true;
    return PS_OK;
}

// behind pair_entry: ps_bootstrap_support (m == nullptr) and ps_multi_bootstrap_support (core, acc: shard 0's handles).  Every
// refusal stands before the source is opened, i.e. before anything is queued.
static auto boot_entry(const ps_bootstrap_params *prm, const uint32_t *sites, ps_bootstrap_t *out, uint32_t *left, uint32_t *right, uint32_t *support,
                       uint32_t *shared)
{
    return [=](ps_multi *m, ps_population *core, ps_population *acc) -> int {
        PSCHK(pair_handles(core, acc, m ? "ps_multi_bootstrap_support" : "ps_bootstrap_support", "bootstrap support needs"));
        const uint64_t L = m ? m->prm.core_size : core->cfg.global_cols;
        uint64_t draws = 0;
        PSCHK(boot_check_params(prm, core->cfg.pop_size, L, acc->cfg.core_genes, &draws));
        bool onehot = core->core_davg_form != 3;
        for (size_t k = 0; k < (m ? m->shard.size() : 1); k++) onehot = onehot && (m ? m->shard[k]->core : core)->onehot_safe;
        if (!onehot)
            return ps_fail(PS_ERR_INVALID, "bootstrap support: the resampled form of the core strings exists for one-hot matrices only (every byte 1, 2, 4 "
                                           "or 8, core_davg_form not 3)");
        if (sites)
            for (uint64_t b = 0; b < prm->replicates; b++)
                for (uint64_t k = 0; k < draws; k++)
                    if (sites[b * draws + k] >= L)
                        return ps_fail(PS_ERR_INVALID, "replicate %llu, position %llu: site %u is not below the %llu core sites", (unsigned long long)b,
                                       (unsigned long long)k, sites[b * draws + k], (unsigned long long)L);
        core_band_source src;
        const uint32_t *slot = nullptr;
        PSCHK(pair_source_open(&src, "bootstrap_support", "bootstrap support needs", "resamples", m, core, acc, true, &slot));
        return boot_device(src, acc, L, draws, prm, sites, slot, out, left, right, support, shared);
    };
}

extern "C" int ps_bootstrap_support(ps_population *core, ps_population *acc, const ps_bootstrap_params *prm, const uint32_t *sites, ps_bootstrap_t *out,
                                    uint32_t *left, uint32_t *right, uint32_t *support, uint32_t *shared)
{
    return pair_entry(core, acc, prm && out && left && right && support && shared, boot_entry(prm, sites, out, left, right, support, shared));
}

extern "C" int ps_sim_bootstrap_support(ps_sim *s, const ps_bootstrap_params *prm, const uint32_t *sites, ps_bootstrap_t *out, uint32_t *left,
                                        uint32_t *right, uint32_t *support, uint32_t *shared)
{
    return pair_entry(s, prm && out && left && right && support && shared, boot_entry(prm, sites, out, left, right, support, shared));
}

extern "C" int ps_multi_bootstrap_support(ps_multi *m, const ps_bootstrap_params *prm, const uint32_t *sites, ps_bootstrap_t *out, uint32_t *left,
                                          uint32_t *right, uint32_t *support, uint32_t *shared)
{
    return pair_entry(m, prm && out && left && right && support && shared, boot_entry(prm, sites, out, left, right, support, shared));
}

extern "C" int ps_bootstrap_timing(ps_population *core, double *lists_ms, double *operands_ms, double *trees_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_BOOT], "no bootstrap support has been computed on this handle", { lists_ms, operands_ms, trees_ms });
}
