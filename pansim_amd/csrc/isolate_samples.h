// isolate_samples.h -- isolate samples (include/pansim_hip.h; the definitions: docs/ISOLATE_SAMPLES.md): rows of one or more
// populations gathered into a NEW ps_population on the device (ps_population_pool, ps_population_subset, ps_sim_subset,
// ps_multi_subset, ps_population_subset_timing), so that every read-out applies to a sample as it applies to a population, and the
// recorded genealogy restricted to a sample on the host (ps_genealogy_restrict).  The kernels: sample_kernels.h; the form and the
// grid of the core gather: sample_plan.h.  Included by pansim_capi.hip behind allele_profiles.h.
//
// The new handle is made by pop_create_impl without an initial vector (the gather writes every byte of the matrix, the pad
// included, once); the sources are read on their own streams behind whatever is queued there and never written.
#pragma once

// one launch of the core gather on `st`: the bytes [off, own_end) of the output rows of the L sites of `in`
static int core_gather_launch(int form, const uint8_t *in, uint32_t pitch_in, uint64_t L, uint8_t *out, uint32_t pitch_out, const uint32_t *d_idx,
                              uint32_t n, uint32_t off, uint32_t own_end, hipStream_t st)
{
    if (!L || own_end <= off) return PS_OK;
    const gather_plan g = core_gather_plan(form, pitch_in, n, off, own_end, L);
    const dim3 grid(g.tiles, g.runs), block(g.tx, g.sy);
    auto launch = [&](auto kern) -> int {
        if (g.lds > 32768u) HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));
        hipLaunchKernelGGL(kern, grid, block, g.lds, st, in, pitch_in, out, pitch_out, d_idx, n, off, own_end, L, g.sites_per_wg);
        HIPCHK(hipGetLastError());
        return PS_OK;
    };
    if (g.direct) return launch(core_gather_rows_kernel<1, true>);
    if (g.ch == 1) return launch(core_gather_rows_kernel<1, false>);
    if (g.ch == 2) return launch(core_gather_rows_kernel<2, false>);
    return launch(core_gather_rows_kernel<(int)PS_GATHER_MAX_CHUNKS, false>);
}

// every source stream is drained on every way out: the launches read this call's own device lists and the caller's host memory
struct sample_drain {
    std::vector<ps_population *> srcs;
    ~sample_drain()
    {
        for (size_t k = srcs.size(); k-- > 0;) {
            (void)hipSetDevice(srcs[k]->device);
            (void)hipStreamSynchronize(srcs[k]->stream);
        }
    }
};

// One part of a gather: `n` rows of `src` (host list `rows`, nullptr = all of them in order), written behind `off` rows of the
// output
struct sample_part {
    ps_population *src = nullptr;
    const uint32_t *rows = nullptr;
    uint32_t n = 0, off = 0;
    bool last = false;                  // the part whose launch writes the zeros of the pad
};

// the device list idx = slot o rows of one part, on the part's device and stream
static int sample_index(const sample_part &pt, dev_tmp<uint32_t> *d_rows, dev_tmp<uint32_t> *d_idx)
{
    ps_population *p = pt.src;
    const uint32_t *slot = nullptr;
    PSCHK(rows_current(p, &slot));
    PSCHK(use_device(p));
    if (pt.rows) {
        PSCHK(d_rows->alloc(pt.n));
        HIPCHK(hipMemcpyAsync(d_rows->p, pt.rows, (uint64_t)pt.n * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    }
    PSCHK(d_idx->alloc(pt.n));
    sample_index_kernel<<<(pt.n + 255u) / 256u, 256, 0, p->stream>>>(d_rows->p, slot ? p->d_row_slot : nullptr, pt.n, d_idx->p);
    HIPCHK(hipGetLastError());
    return PS_OK;
}

// the handle of a sample of `total` rows, shaped like `like` but holding the columns [col_offset, col_offset + ncols)
static int sample_make(const ps_population *like, uint64_t total, uint64_t col_offset, uint64_t ncols, ps_population **out)
{
    ps_population *p = new ps_population();
    p->cfg = like->cfg;
    p->cfg.pop_size = total;
    p->cfg.col_offset = col_offset;
    p->cfg.ncols = ncols;
    p->cfg.device = like->device;
    const int rc = pop_create_impl(&p->cfg, nullptr, p);
    if (rc != PS_OK) {
        const std::string keep = g_err;
        ps_population_destroy(p);
        g_err = keep;
        return rc;
    }
    p->g_valid = false;                 // (the gene-major view rebuilds itself on first use, as after ps_load_matrix)
    p->counts_fresh = false;
    *out = p;
    return PS_OK;
}

// The gathers of every part into `made` (core: the sites [made_site0, made_site0 + src ncols) of it), each on its source's
// stream, timed by events there.  The core block of a site shard on another device is gathered into a buffer of this call on the
// shard's device and copied to `made` on the shard's stream (the source handle's own scratch is not touched).
static int sample_fill(ps_population *made, const std::vector<sample_part> &parts, const std::vector<uint64_t> &made_site0, event_timer &tm)
{
    const size_t K = parts.size();
    std::vector<dev_tmp<uint32_t>> d_rows(K), d_idx(K);
    std::vector<dev_tmp<uint8_t>> stage(K);
    sample_drain drain;
    for (size_t k = 0; k < K; k++) {
        const sample_part &pt = parts[k];
        ps_population *p = pt.src;
        if (!pt.n && !pt.last) continue;
        drain.srcs.push_back(p);
        PSCHK(sample_index(pt, &d_rows[k], &d_idx[k]));
        if (made->cfg.core) {
            const uint64_t L = p->cfg.ncols;
            uint8_t *dst = made->state + made_site0[k] * made->pitch;
            if (p->device != made->device && L) {
                PSCHK(stage[k].alloc(L * made->pitch));
                dst = stage[k].p;
            }
            const uint32_t own_end = pt.last ? made->pitch : pt.off + pt.n;
            PSCHK(tm.timed(0, p->stream, [&]() -> int {
                PSCHK(core_gather_launch(p->gather_form, p->state, p->pitch, L, dst, made->pitch, d_idx[k].p, pt.n, pt.off, own_end, p->stream));
                if (stage[k].p)
                    HIPCHK(hipMemcpyPeerAsync(made->state + made_site0[k] * made->pitch, made->device, stage[k].p, p->device, L * made->pitch, p->stream));
                return PS_OK;
            }));
        } else if (pt.n && p->d.GW) {
            const uint64_t words = (uint64_t)pt.n * p->d.GW;
            PSCHK(tm.timed(0, p->stream, [&]() -> int {
                acc_gather_rows_kernel<<<(uint32_t)std::min<uint64_t>((words + 255) / 256, 65536), 256, 0, p->stream>>>(
                    p->I[p->cur], made->I[made->cur] + (uint64_t)pt.off * p->d.GW, d_idx[k].p, pt.n, p->d.GW);
                HIPCHK(hipGetLastError());
                return PS_OK;
            }));
        }
    }
    for (ps_population *p : drain.srcs) {
        PSCHK(use_device(p));
        PSCHK(sync_checked(p));
    }
    PSCHK(use_device(made));
    return PS_OK;
}

// the list of one part: null = all rows (n is then the part's pop_size), else every entry below the part's pop_size
static int sample_check_rows(const ps_population *p, const uint32_t *rows, uint64_t n, size_t part)
{
    if (!rows) {
        if (n != p->cfg.pop_size)
            return ps_fail(PS_ERR_INVALID, "n_rows[%zu] = %llu, but rows[%zu] is null (all rows) and the part has pop_size %llu", part,
                           (unsigned long long)n, part, (unsigned long long)p->cfg.pop_size);
        return PS_OK;
    }
    for (uint64_t j = 0; j < n; j++)
        if (rows[j] >= p->cfg.pop_size)
            return ps_fail(PS_ERR_INVALID, "rows[%zu][%llu] = %u is not below the pop_size %llu of part %zu", part, (unsigned long long)j, rows[j],
                           (unsigned long long)p->cfg.pop_size, part);
    return PS_OK;
}

// what ps_population_create accepts
static int sample_check_total(uint64_t total)
{
    if (total < 1) return ps_fail(PS_ERR_INVALID, "the sum of n_rows is 0: a sample has at least one row");
    if (total > 0xFFFFFFFFull - 128) return ps_fail(PS_ERR_INVALID, "the sum of n_rows = %llu does not fit the 32 bits of pop_size", (unsigned long long)total);
    return PS_OK;
}

extern "C" int ps_population_pool(ps_population *const *parts, const uint32_t *const *rows, const uint64_t *n_rows, uint32_t n_parts,
                                  ps_population **out)
{
    if (out) *out = nullptr;
    if (!parts || !n_rows || !out) return ps_fail(PS_ERR_INVALID, "null argument");
    if (n_parts < 1) return ps_fail(PS_ERR_INVALID, "n_parts is 0: a pool has at least one part");
    for (uint32_t k = 0; k < n_parts; k++)
        if (!parts[k]) return ps_fail(PS_ERR_INVALID, "null argument: parts[%u]", k);
    uint64_t total = 0;
    for (uint32_t k = 0; k < n_parts; k++) {
        if (n_rows[k] > 0xFFFFFFFFull) return ps_fail(PS_ERR_INVALID, "n_rows[%u] = %llu does not fit 32 bits", k, (unsigned long long)n_rows[k]);
        total += n_rows[k];
    }
    if (total < 1) return sample_check_total(total);
    PSCHK(ps_needs_device());
    const ps_population *p0 = parts[0];
    for (uint32_t k = 1; k < n_parts; k++) {
        const ps_population *p = parts[k];
        if (p->cfg.core != p0->cfg.core)
            return ps_fail(PS_ERR_INVALID, "parts[%u] is %s matrix and parts[0] %s: the parts of a pool are all core or all accessory", k,
                           p->cfg.core ? "a core" : "an accessory", p0->cfg.core ? "a core" : "an accessory");
        if (p->cfg.ncols != p0->cfg.ncols) return ps_fail(PS_ERR_INVALID, "ncols of parts[%u] is %llu, of parts[0] %llu", k, (unsigned long long)p->cfg.ncols, (unsigned long long)p0->cfg.ncols);
        if (p->cfg.col_offset != p0->cfg.col_offset) return ps_fail(PS_ERR_INVALID, "col_offset of parts[%u] is %llu, of parts[0] %llu", k, (unsigned long long)p->cfg.col_offset, (unsigned long long)p0->cfg.col_offset);
        if (p->cfg.global_cols != p0->cfg.global_cols) return ps_fail(PS_ERR_INVALID, "global_cols of parts[%u] is %llu, of parts[0] %llu", k, (unsigned long long)p->cfg.global_cols, (unsigned long long)p0->cfg.global_cols);
        if (p->cfg.core_genes != p0->cfg.core_genes) return ps_fail(PS_ERR_INVALID, "core_genes of parts[%u] is %llu, of parts[0] %llu", k, (unsigned long long)p->cfg.core_genes, (unsigned long long)p0->cfg.core_genes);
        if (p->device != p0->device) return ps_fail(PS_ERR_INVALID, "parts[%u] is on device %d and parts[0] on device %d", k, p->device, p0->device);
    }
    PSCHK(sample_check_total(total));
    for (uint32_t k = 0; k < n_parts; k++) PSCHK(sample_check_rows(parts[k], rows ? rows[k] : nullptr, n_rows[k], k));
    std::vector<sample_part> pts(n_parts);
    bool nibble = true, onehot = true;
    uint64_t off = 0;
    size_t last = 0;
    for (uint32_t k = 0; k < n_parts; k++) {
        pts[k].src = parts[k];
        pts[k].rows = rows ? rows[k] : nullptr;
        pts[k].n = (uint32_t)n_rows[k];
        pts[k].off = (uint32_t)off;
        off += n_rows[k];
        if (n_rows[k]) last = k;
        nibble = nibble && parts[k]->nibble_safe;
        onehot = onehot && parts[k]->onehot_safe;
    }
    pts[last].last = true;
    ps_population *made = nullptr;
    PSCHK(sample_make(p0, total, p0->cfg.col_offset, p0->cfg.ncols, &made));
    made->nibble_safe = nibble;
    made->onehot_safe = onehot;
    event_timer tm;
    int rc = sample_fill(made, pts, std::vector<uint64_t>(n_parts, 0), tm);
    if (rc == PS_OK) rc = tm.total_ms(0, &made->sample_ms);
    if (rc != PS_OK) {
        const std::string keep = g_err;
        ps_population_destroy(made);
        g_err = keep;
        return rc;
    }
    made->sample_timed = true;
    *out = made;
    return PS_OK;
}

extern "C" int ps_population_subset(ps_population *src, const uint32_t *rows, uint64_t n_rows, ps_population **out)
{
    if (out) *out = nullptr;
    if (!src || !out) return ps_fail(PS_ERR_INVALID, "null argument");
    return ps_population_pool(&src, &rows, &n_rows, 1, out);
}

// both samples of a run's two handles from the same rows; either out pointer may be null
static int sample_pair(ps_population *core, ps_population *acc, const uint32_t *rows, uint64_t n_rows, ps_population **core_out, ps_population **acc_out)
{
    if (core_out) PSCHK(ps_population_subset(core, rows, n_rows, core_out));
    if (acc_out) {
        const int rc = ps_population_subset(acc, rows, n_rows, acc_out);
        if (rc != PS_OK && core_out) {
            const std::string keep = g_err;
            ps_population_destroy(*core_out);
            *core_out = nullptr;
            g_err = keep;
        }
        return rc;
    }
    return PS_OK;
}

extern "C" int ps_sim_subset(ps_sim *s, const uint32_t *rows, uint64_t n_rows, ps_population **core_out, ps_population **acc_out)
{
    if (core_out) *core_out = nullptr;
    if (acc_out) *acc_out = nullptr;
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    if (!core_out && !acc_out) return ps_fail(PS_ERR_INVALID, "null argument: core_out and acc_out");
    if (n_rows < 1) return sample_check_total(n_rows);
    PSCHK(ps_needs_device());
    // (no ps_sim_sync: the gathers are ordered behind the run on the handles' streams)
    return sample_pair(s->core, s->acc, rows, n_rows, core_out, acc_out);
}

// the core sample of a sharded run: a WHOLE handle on shard 0's device; shard k's block of sites lands contiguously at
// state + col_offset_k x pitch
static int sample_multi_core(ps_multi *m, const uint32_t *rows, uint64_t n_rows, ps_population **out)
{
    ps_population *c0 = m->shard[0]->core;
    PSCHK(sample_check_total(n_rows));
    PSCHK(sample_check_rows(c0, rows, n_rows, 0));
    const size_t K = m->shard.size();
    std::vector<sample_part> pts(K);
    std::vector<uint64_t> site0(K);
    bool nibble = true, onehot = true;
    for (size_t k = 0; k < K; k++) {
        ps_population *c = m->shard[k]->core;
        pts[k].src = c;
        pts[k].rows = rows;
        pts[k].n = (uint32_t)n_rows;
        pts[k].last = true;                      // (every shard writes the pad of its own site rows)
        site0[k] = c->cfg.col_offset;
        nibble = nibble && c->nibble_safe;
        onehot = onehot && c->onehot_safe;
    }
    ps_population *made = nullptr;
    PSCHK(sample_make(c0, n_rows, 0, c0->cfg.global_cols, &made));
    made->nibble_safe = nibble;
    made->onehot_safe = onehot;
    event_timer tm;
    int rc = sample_fill(made, pts, site0, tm);
    if (rc == PS_OK) rc = tm.total_ms(0, &made->sample_ms);
    if (rc != PS_OK) {
        const std::string keep = g_err;
        ps_population_destroy(made);
        g_err = keep;
        return rc;
    }
    made->sample_timed = true;
    *out = made;
    return PS_OK;
}

extern "C" int ps_multi_subset(ps_multi *m, const uint32_t *rows, uint64_t n_rows, ps_population **core_out, ps_population **acc_out)
{
    if (core_out) *core_out = nullptr;
    if (acc_out) *acc_out = nullptr;
    if (!m) return ps_fail(PS_ERR_INVALID, "null argument");
    if (!core_out && !acc_out) return ps_fail(PS_ERR_INVALID, "null argument: core_out and acc_out");
    if (n_rows < 1) return sample_check_total(n_rows);
    PSCHK(ps_needs_device());
    if (m->shard.size() == 1) return ps_sim_subset(m->shard[0], rows, n_rows, core_out, acc_out);
    // (the shards' blocks meet in one handle: everything queued on every shard is complete first, as before the other read-outs
    // that join shards)
    PSCHK(ps_multi_sync(m));
    if (core_out) PSCHK(sample_multi_core(m, rows, n_rows, core_out));
    if (acc_out) {
        // (shard 0's replica: the shards' accessory matrices are bit-identical)
        const int rc = ps_population_subset(m->shard[0]->acc, rows, n_rows, acc_out);
        if (rc != PS_OK && core_out) {
            const std::string keep = g_err;
            ps_population_destroy(*core_out);
            *core_out = nullptr;
            g_err = keep;
        }
        return rc;
    }
    return PS_OK;
}

extern "C" int ps_population_subset_timing(ps_population *made, double *gather_ms)
{
    if (!made) return ps_fail(PS_ERR_INVALID, "null argument");
    if (!made->sample_timed) return ps_fail(PS_ERR_STATE, "this handle was not made by ps_population_pool or a ps_*_subset call");
    if (gather_ms) *gather_ms = made->sample_ms;
    return PS_OK;
}

extern "C" int ps_genealogy_restrict(const uint32_t *order, const uint32_t *coal, uint64_t n, const uint32_t *rows, uint64_t n_rows,
                                     uint32_t *order_out, uint32_t *coal_out)
{
    if (!order || (n > 1 && !coal) || !rows || !order_out || (n_rows > 1 && !coal_out)) return ps_fail(PS_ERR_INVALID, "null argument");
    if (n_rows < 1 || n_rows > 0xFFFFFFFFull) return ps_fail(PS_ERR_INVALID, "n_rows = %llu: a restricted genealogy has 1 .. 2^32 - 1 rows", (unsigned long long)n_rows);
    std::vector<uint32_t> rank;
    PSCHK(gen_rank(order, n, &rank));
    // the entries in (internal position, index in rows) order: a counting sort over the positions keeps the indices ascending
    std::vector<uint64_t> start(n + 1, 0);
    for (uint64_t j = 0; j < n_rows; j++) {
        if (rows[j] >= n) return ps_fail(PS_ERR_INVALID, "rows[%llu] = %u is not below pop_size %llu", (unsigned long long)j, rows[j], (unsigned long long)n);
        start[rank[rows[j]] + 1]++;
    }
    for (uint64_t r = 0; r < n; r++) start[r + 1] += start[r];
    for (uint64_t j = 0; j < n_rows; j++) order_out[start[rank[rows[j]]]++] = (uint32_t)j;
    const gen_host_table tab(coal, n);
    for (uint64_t q = 0; q + 1 < n_rows; q++) {
        const uint32_t a = rank[rows[order_out[q]]], b = rank[rows[order_out[q + 1]]];
        coal_out[q] = a == b ? 0u : tab.tmrca(a, b);
    }
    return PS_OK;
}
