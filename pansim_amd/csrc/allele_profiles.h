// allele_profiles.h -- ps_allele_profiles / ps_sim_allele_profiles / ps_multi_allele_profiles, the host form
// ps_profiles_from_alleles and ps_allele_profiles_timing (include/pansim_hip.h; the definitions: docs/ALLELE_PROFILES.md).
// Included by pansim_capi.hip behind strain_clusters.h, whose label kernels (cluster_init_kernel, cluster_hook_kernel,
// cluster_jump_kernel) contract the adjacency bit matrix that mlst_pair_kernel writes.
//
// One routine serves every entry: a list of `parts` (the core handle; or the core handles of the shards of a run).  The loci
// go in bands so that the fingerprint table (16 bytes per locus and individual) stays within a budget; per band every part
// fingerprints the sites it holds on its own stream, part 0 adds the others' tables and numbers the alleles, the
// representatives go back and every part verifies its own sites.  Only the u16 allele numbers are kept across bands; the
// pairs and the labels run on part 0 in output row order.
#pragma once

#include <unordered_map>

#include "cluster_kernels.h"
#include "mlst_kernels.h"

#define PS_MLST_MAX_BINS 16384u         // 64 KB of u32 bins in LDS per workgroup
#define PS_MLST_MAX_LOCI 65535u         // a pair differs at no more loci than a u16 holds
#define PS_MLST_MAX_POP 65536u          // allele numbers are u16
#define PS_MLST_MAX_CELLS (1ull << 30)  // n_loci x pop_size
#define PS_MLST_TABLE_BYTES (256ull << 20)      // the fingerprints of one band

static int mlst_check_params(const ps_mlst_params *prm, uint64_t N)
{
    if (N < 2 || N > PS_MLST_MAX_POP) return ps_fail(PS_ERR_INVALID, "pop_size must be 2 .. %u, not %llu", PS_MLST_MAX_POP, (unsigned long long)N);
    if (prm->n_loci < 1 || prm->n_loci > PS_MLST_MAX_LOCI)
        return ps_fail(PS_ERR_INVALID, "n_loci must be 1 .. %u, not %u", PS_MLST_MAX_LOCI, prm->n_loci);
    if ((uint64_t)prm->n_loci * N > PS_MLST_MAX_CELLS)
        return ps_fail(PS_ERR_INVALID, "n_loci x pop_size = %llu exceeds the limit of 2^30 allele numbers", (unsigned long long)prm->n_loci * N);
    if (prm->dist_bins < 1 || prm->dist_bins > PS_MLST_MAX_BINS)
        return ps_fail(PS_ERR_INVALID, "dist_bins must be 1 .. %u, not %u", PS_MLST_MAX_BINS, prm->dist_bins);
    if (prm->complex_max > prm->n_loci) return ps_fail(PS_ERR_INVALID, "complex_max = %u exceeds n_loci = %u", prm->complex_max, prm->n_loci);
    if (prm->key_bits < 1 || prm->key_bits > 64) return ps_fail(PS_ERR_INVALID, "key_bits must be 1 .. 64, not %u", prm->key_bits);
    return PS_OK;
}

// the n_loci + 1 site bounds of the loci over L sites: the caller's, checked, or the even cut
static int mlst_bounds(const ps_mlst_params *prm, const uint64_t *bounds, uint64_t L, std::vector<unsigned long long> *out)
{
    const uint64_t n = prm->n_loci;
    out->resize(n + 1);
    if (!bounds) {
        if (n > L) return ps_fail(PS_ERR_INVALID, "n_loci = %llu exceeds the %llu core sites: a locus would be empty", (unsigned long long)n, (unsigned long long)L);
        for (uint64_t g = 0; g <= n; g++) (*out)[g] = (unsigned long long)((unsigned __int128)g * L / n);
        return PS_OK;
    }
    for (uint64_t g = 0; g <= n; g++) {
        if (g && bounds[g] <= bounds[g - 1])
            return ps_fail(PS_ERR_INVALID, "bounds %llu: the bounds must be strictly ascending (%llu after %llu)", (unsigned long long)g,
                           (unsigned long long)bounds[g], (unsigned long long)bounds[g - 1]);
        (*out)[g] = bounds[g];
    }
    if (bounds[n] > L) return ps_fail(PS_ERR_INVALID, "bounds %llu: %llu is beyond the %llu core sites", (unsigned long long)n, (unsigned long long)bounds[n], (unsigned long long)L);
    return PS_OK;
}

// rep[k]: any value below N that is equal exactly for the members of one class -> labels[k] = the smallest k of the class;
// the number of classes, of classes of one, the largest, and the pairs inside classes
static void mlst_classes(const uint32_t *rep, uint64_t N, uint32_t *labels, uint64_t *classes, uint64_t *singletons, uint64_t *largest,
                         uint64_t *within)
{
    std::vector<uint32_t> first(N, UINT32_MAX), size(N, 0);
    for (uint64_t k = 0; k < N; k++) {
        if (first[rep[k]] == UINT32_MAX) first[rep[k]] = (uint32_t)k;
        labels[k] = first[rep[k]];
        size[labels[k]]++;
    }
    *classes = *singletons = *largest = *within = 0;
    for (uint64_t k = 0; k < N; k++) {
        const uint64_t s = size[k];
        if (!s) continue;
        ++*classes;
        *singletons += s == 1 ? 1 : 0;
        *largest = std::max(*largest, s);
        *within += s * (s - 1) / 2;
    }
}

// the fields that follow from the sizes, the per-locus counts, the labels (st, cx: as mlst_classes takes them) and the pair words
static void mlst_finish(ps_mlst_t *o, uint64_t N, uint64_t L, uint64_t covered, const ps_mlst_params *prm, const uint32_t *locus_alleles,
                        const uint32_t *st_rep, const uint32_t *cx_rep, uint32_t *st, uint32_t *cx, uint64_t sum_d, uint64_t min_d, uint64_t max_d,
                        uint64_t identical, uint64_t edges, uint64_t rounds)
{
    memset(o, 0, sizeof *o);
    o->pop_size = N;
    o->pairs = N * (N - 1) / 2;
    o->core_sites = L;
    o->loci = prm->n_loci;
    o->sites_covered = covered;
    for (uint32_t g = 0; g < prm->n_loci; g++) {
        o->alleles_total += locus_alleles[g];
        o->max_alleles = std::max<uint64_t>(o->max_alleles, locus_alleles[g]);
        o->monomorphic_loci += locus_alleles[g] == 1 ? 1 : 0;
    }
    uint64_t within, singles;
    mlst_classes(st_rep, N, st, &o->sequence_types, &o->singleton_sts, &o->largest_st, &within);
    mlst_classes(cx_rep, N, cx, &o->complexes, &singles, &o->largest_complex, &within);
    o->identical_pairs = identical;
    o->edges = edges;
    o->sum_d = sum_d;
    o->min_d = min_d;
    o->max_d = max_d;
    o->mean_distance = (double)sum_d / (double)o->pairs / (double)o->loci;
    o->dist_bins = prm->dist_bins;
    o->complex_max = prm->complex_max;
    o->rounds = rounds;
}

extern "C" int ps_profiles_from_alleles(const uint32_t *alleles, uint64_t pop_size, const ps_mlst_params *prm, ps_mlst_t *out, uint32_t *locus_alleles,
                                        uint64_t *locus_same_pairs, uint32_t *st, uint32_t *complex_of, uint64_t *hist, uint16_t *profiles)
{
    if (!alleles || !prm || !out || !locus_alleles || !locus_same_pairs || !st || !complex_of || !hist) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(mlst_check_params(prm, pop_size));
    const uint64_t N = pop_size, M = prm->n_loci;
    // dense numbers by first appearance, locus-major
    std::vector<uint16_t> id(M * N);
    for (uint64_t g = 0; g < M; g++) {
        std::unordered_map<uint32_t, uint32_t> number;
        std::vector<uint64_t> count;
        for (uint64_t k = 0; k < N; k++) {
            const auto it = number.emplace(alleles[k * M + g], (uint32_t)number.size()).first;
            if (it->second == count.size()) count.push_back(0);
            count[it->second]++;
            id[g * N + k] = (uint16_t)it->second;
        }
        locus_alleles[g] = (uint32_t)count.size();
        locus_same_pairs[g] = 0;
        for (uint64_t c : count) locus_same_pairs[g] += c * (c - 1) / 2;
    }
    if (profiles)
        for (uint64_t k = 0; k < N; k++)
            for (uint64_t g = 0; g < M; g++) profiles[k * M + g] = id[g * N + k];
    // union-find, the smaller root kept, once per relation
    std::vector<uint32_t> ps(N), pc(N), d(N);
    for (uint64_t k = 0; k < N; k++) ps[k] = pc[k] = (uint32_t)k;
    auto root = [](std::vector<uint32_t> &parent, uint32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    memset(hist, 0, prm->dist_bins * sizeof(uint64_t));
    uint64_t sum_d = 0, min_d = UINT64_MAX, max_d = 0, identical = 0, edges = 0;
    for (uint64_t i = 0; i + 1 < N; i++) {
        std::fill(d.begin() + i + 1, d.end(), 0u);
        for (uint64_t g = 0; g < M; g++) {
            const uint16_t *row = id.data() + g * N;
            const uint16_t a = row[i];
            for (uint64_t j = i + 1; j < N; j++) d[j] += row[j] != a ? 1u : 0u;
        }
        for (uint64_t j = i + 1; j < N; j++) {
            const uint64_t dd = d[j];
            hist[dd * prm->dist_bins / (M + 1)]++;
            sum_d += dd;
            min_d = std::min(min_d, dd);
            max_d = std::max(max_d, dd);
            if (dd == 0) {
                identical++;
                const uint32_t x = root(ps, (uint32_t)i), y = root(ps, (uint32_t)j);
                ps[std::max(x, y)] = std::min(x, y);
            }
            if (dd <= prm->complex_max) {
                edges++;
                const uint32_t x = root(pc, (uint32_t)i), y = root(pc, (uint32_t)j);
                pc[std::max(x, y)] = std::min(x, y);
            }
        }
    }
    for (uint64_t k = 0; k < N; k++) {
        ps[k] = root(ps, (uint32_t)k);
        pc[k] = root(pc, (uint32_t)k);
    }
    mlst_finish(out, N, 0, 0, prm, locus_alleles, ps.data(), pc.data(), st, complex_of, sum_d, min_d, max_d, identical, edges, 0);
    return PS_OK;
}

// what the phases of mlst_run share
struct mlst_geom {
    uint32_t N = 0, M = 0, ldn = 0, rows = 0, W = 0, band = 0, T = 0, canon_grid = 0, canon_lds = 0;
    uint64_t mask = 0;
    bool adj = false;
    size_t K = 1;
};

// The call's scratch on one part.  Part 0: words | bins | allele numbers | adjacency matrix -- zeroed per call -- then the
// per-locus counts, the two label arrays, `changed`, and what every part has: bounds | one band of fingerprints | one band of
// representatives; behind them on part 0 the landing table (with several parts) and the tables of the canonicalise workgroups
// (where they do not fit the LDS).  The other parts keep their own words (the count of the verification).
struct mlst_scratch {
    unsigned long long *words = nullptr, *hist = nullptr, *adj = nullptr, *same = nullptr, *bounds = nullptr;
    uint16_t *ids = nullptr;
    uint32_t *alleles = nullptr, *st = nullptr, *cx = nullptr, *changed = nullptr, *rep = nullptr, *work = nullptr;
    ulonglong2 *F = nullptr, *land = nullptr;
    uint8_t *base = nullptr;
    uint64_t zero_bytes = 0;
};

static int mlst_scratch_get(ps_population *p, const mlst_geom &g, const ps_mlst_params *prm, bool first, mlst_scratch *s)
{
    scratch_layout lay;
    const uint64_t cells = (uint64_t)g.band * g.N;
    const uint64_t o_words = lay.add(PS_MLST_WORDS * 8, 256), o_hist = lay.add(first ? prm->dist_bins * 8ull : 0, 256);
    const uint64_t o_ids = lay.add(first ? (uint64_t)g.rows * g.ldn * 2 : 0, 256), o_adj = lay.add(first && g.adj ? (uint64_t)g.N * g.W * 8 : 0, 256);
    const uint64_t zero_bytes = lay.bytes;
    const uint64_t o_alleles = lay.add(first ? g.M * 4ull : 0, 256), o_same = lay.add(first ? g.M * 8ull : 0, 256);
    const uint64_t o_st = lay.add(first ? g.N * 4ull : 0, 256), o_cx = lay.add(first ? g.N * 4ull : 0, 256), o_changed = lay.add(first ? 8 : 0, 256);
    const uint64_t o_bounds = lay.add((g.M + 1ull) * 8, 256), o_F = lay.add(cells * 16, 256), o_rep = lay.add(cells * 4, 256);
    const uint64_t o_land = lay.add(first && g.K > 1 ? cells * 16 : 0, 256);
    const uint64_t o_work = lay.add(first && !g.canon_lds ? (uint64_t)g.canon_grid * ((uint64_t)g.T + 2ull * g.N) * 4 : 0, 256);
    uint8_t *base = nullptr;
    PSCHK(scratch_get(p->ro[PS_RO_MLST], lay.bytes, &base, "cannot allocate the %llu bytes of the allele numbers of %u loci and the fingerprints of one band of %u",
                      g.M, g.band));
    s->base = base;
    s->zero_bytes = zero_bytes;
    s->words = (unsigned long long *)(base + o_words);
    s->hist = (unsigned long long *)(base + o_hist);
    s->ids = (uint16_t *)(base + o_ids);
    s->adj = (unsigned long long *)(base + o_adj);
    s->alleles = (uint32_t *)(base + o_alleles);
    s->same = (unsigned long long *)(base + o_same);
    s->st = (uint32_t *)(base + o_st);
    s->cx = (uint32_t *)(base + o_cx);
    s->changed = (uint32_t *)(base + o_changed);
    s->bounds = (unsigned long long *)(base + o_bounds);
    s->F = (ulonglong2 *)(base + o_F);
    s->rep = (uint32_t *)(base + o_rep);
    s->land = (ulonglong2 *)(base + o_land);
    s->work = (uint32_t *)(base + o_work);
    return PS_OK;
}

// every stream the call has touched is drained on every way out: the uploads read this call's own host memory
struct mlst_drain {
    const std::vector<ps_population *> &parts;
    ~mlst_drain()
    {
        for (size_t k = parts.size(); k-- > 0;) {      // (part 0 last: its device stays the current one)
            (void)hipSetDevice(parts[k]->device);
            (void)hipStreamSynchronize(parts[k]->stream);
        }
    }
};

// with several parts everything queued on every handle is complete (ps_multi_sync); L: the sites of all parts
static int mlst_run(const std::vector<ps_population *> &parts, uint64_t L, const ps_mlst_params *prm, const uint64_t *bounds, ps_mlst_t *out,
                    uint32_t *locus_alleles, uint64_t *locus_same_pairs, uint32_t *st, uint32_t *complex_of, uint64_t *hist, uint16_t *profiles)
{
    ps_population *p0 = parts[0];
    const size_t K = parts.size();
    const uint64_t N64 = p0->cfg.pop_size;
    PSCHK(mlst_check_params(prm, N64));
    std::vector<unsigned long long> h_bounds;
    PSCHK(mlst_bounds(prm, bounds, L, &h_bounds));
    mlst_geom g;
    g.N = (uint32_t)N64;
    g.M = prm->n_loci;
    g.K = K;
    g.ldn = (g.N + PS_MLST_TILE - 1u) & ~(PS_MLST_TILE - 1u);
    g.rows = (g.M + 2u * PS_MLST_CHUNK - 1u) / (2u * PS_MLST_CHUNK) * (2u * PS_MLST_CHUNK);
    g.W = (g.N + 63u) / 64u;
    g.mask = prm->key_bits >= 64 ? ~0ull : (1ull << prm->key_bits) - 1ull;
    g.adj = prm->complex_max >= 1;
    g.band = p0->mlst_band ? p0->mlst_band : (uint32_t)std::max<uint64_t>(1, PS_MLST_TABLE_BYTES / 16 / g.N);
    g.band = std::min(g.band, g.M);
    g.T = 2;
    while (g.T < 2u * g.N) g.T <<= 1;
    g.canon_grid = std::min(g.band, 1024u);
    const uint64_t canon_bytes = ((uint64_t)g.T + 2ull * g.N) * 4;
    // (in LDS up to N = 1024: 16 KB a workgroup, several of them on a CU; beyond that in global memory, where L2 serves the atomics)
    g.canon_lds = canon_bytes <= 16384 ? (uint32_t)canon_bytes : 0u;
    const uint32_t canon_threads = g.N > 256u ? 1024u : 256u;
    // the row maps: every part's own (the shards of a run draw the same parents)
    std::vector<const uint32_t *> d_slot(K, nullptr);
    for (size_t k = 0; k < K; k++) {
        const uint32_t *slot = nullptr;
        PSCHK(rows_current(parts[k], &slot));
        d_slot[k] = slot ? parts[k]->d_row_slot : nullptr;
    }
    // timer groups: 0 = the fingerprints, 1 = the allele numbers, 2 = the verification, 3 = the pairs, 4 = the label rounds
    event_timer tm;
    readout_slot &ro = p0->ro[PS_RO_MLST];
    ro.timed = false;
    std::vector<mlst_scratch> S(K);
    std::vector<unsigned long long> h_bad(K, 0ull);
    unsigned long long w[PS_MLST_WORDS] = {};
    std::vector<uint32_t> h_st(g.N), h_cx(g.N);
    std::vector<uint16_t> h_ids;
    mlst_drain drain{ parts };
    for (size_t k = 0; k < K; k++) {
        ps_population *p = parts[k];
        PSCHK(use_device(p));
        PSCHK(mlst_scratch_get(p, g, prm, k == 0, &S[k]));
        HIPCHK(hipMemsetAsync(S[k].base, 0, S[k].zero_bytes, p->stream));
        HIPCHK(hipMemcpyAsync(S[k].bounds, h_bounds.data(), (g.M + 1ull) * 8, hipMemcpyHostToDevice, p->stream));
    }
    const mlst_scratch &s = S[0];
    hipStream_t s0 = p0->stream;
    auto fingerprint = [&](size_t k, uint32_t lo, uint32_t nb) -> int {
        ps_population *p = parts[k];
        const dim3 grid((g.N + 255u) / 256u, std::min(nb, 65535u));
        hipLaunchKernelGGL(mlst_fingerprint_kernel, grid, dim3(256), 0, p->stream, (const uint8_t *)p->state, p->pitch, g.N, (uint64_t)p->cfg.col_offset,
                           (uint64_t)p->cfg.ncols, (const unsigned long long *)S[k].bounds, lo, nb, (uint64_t)prm->key_seed, g.mask, S[k].F);
        HIPCHK(hipGetLastError());
        return PS_OK;
    };
    auto verify = [&](size_t k, uint32_t lo, uint32_t nb) -> int {
        ps_population *p = parts[k];
        const dim3 grid((g.N + 255u) / 256u, std::min(nb, 65535u));
        hipLaunchKernelGGL(mlst_verify_kernel, grid, dim3(256), 0, p->stream, (const uint8_t *)p->state, p->pitch, g.N, (uint64_t)p->cfg.col_offset,
                           (uint64_t)p->cfg.ncols, (const unsigned long long *)S[k].bounds, d_slot[k], lo, nb, (const uint32_t *)S[k].rep,
                           S[k].words + PS_MLST_BAD);
        HIPCHK(hipGetLastError());
        return PS_OK;
    };
    for (uint32_t lo = 0; lo < g.M; lo += g.band) {
        const uint32_t nb = std::min(g.band, g.M - lo);
        const uint64_t cells = (uint64_t)nb * g.N;
        for (size_t k = 1; k < K; k++) {
            PSCHK(use_device(parts[k]));
            PSCHK(fingerprint(k, lo, nb));
            HIPCHK(hipStreamSynchronize(parts[k]->stream));
        }
        PSCHK(use_device(p0));
        PSCHK(tm.timed(0, s0, [&]() { return fingerprint(0, lo, nb); }));
        for (size_t k = 1; k < K; k++) {
            PSCHK(tm.timed(0, s0, [&]() -> int {
                HIPCHK(hipMemcpyPeerAsync(s.land, p0->device, S[k].F, parts[k]->device, cells * 16, s0));
                mlst_add_kernel<<<(uint32_t)((cells * 2 + 255) / 256), 256, 0, s0>>>((unsigned long long *)s.F, (const unsigned long long *)s.land, cells * 2);
                HIPCHK(hipGetLastError());
                return PS_OK;
            }));
        }
        PSCHK(tm.timed(1, s0, [&]() -> int {
            hipLaunchKernelGGL(mlst_canon_kernel, dim3(std::min(nb, g.canon_grid)), dim3(canon_threads), g.canon_lds, s0, (const ulonglong2 *)s.F, g.N,
                               d_slot[0], lo, nb, g.T, g.canon_lds ? nullptr : s.work, s.rep, s.ids, g.ldn, s.alleles, s.same);
            HIPCHK(hipGetLastError());
            return PS_OK;
        }));
        PSCHK(tm.timed(2, s0, [&]() { return verify(0, lo, nb); }));
        if (K > 1) {
            HIPCHK(hipStreamSynchronize(s0));
            for (size_t k = 1; k < K; k++) {
                PSCHK(use_device(parts[k]));
                HIPCHK(hipMemcpyPeerAsync(S[k].rep, parts[k]->device, s.rep, p0->device, cells * 4, parts[k]->stream));
                PSCHK(verify(k, lo, nb));
                HIPCHK(hipStreamSynchronize(parts[k]->stream));      // (the next band writes rep and F again)
            }
            PSCHK(use_device(p0));
        }
    }
    for (size_t k = 1; k < K; k++) {
        PSCHK(use_device(parts[k]));
        HIPCHK(hipMemcpyAsync(&h_bad[k], S[k].words + PS_MLST_BAD, 8, hipMemcpyDeviceToHost, parts[k]->stream));
        HIPCHK(hipStreamSynchronize(parts[k]->stream));
    }
    PSCHK(use_device(p0));
    // the pairs and the labels, in output row order
    const uint32_t lds = prm->dist_bins * 4u, nt = (g.N + PS_MLST_TILE - 1u) / PS_MLST_TILE;
    const uint32_t per_cu = std::max(1u, std::min(4u, (160u * 1024u) / (lds + 9216u)));
    const uint32_t pair_grid = (uint32_t)std::min<uint64_t>((uint64_t)nt * (nt + 1) / 2, 256ull * per_cu);
    if (lds > 32768u) HIPCHK(hipFuncSetAttribute((const void *)mlst_pair_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    PSCHK(tm.timed(3, s0, [&]() -> int {
        cluster_init_kernel<<<(g.N + 255u) / 256u, 256, 0, s0>>>(s.st, g.N);
        HIPCHK(hipGetLastError());
        cluster_init_kernel<<<(g.N + 255u) / 256u, 256, 0, s0>>>(s.cx, g.N);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(mlst_pair_kernel, dim3(pair_grid), dim3(256), lds, s0, (const uint16_t *)s.ids, g.ldn, g.N, g.M, prm->dist_bins,
                           prm->complex_max, s.hist, s.words, s.st, g.adj ? s.adj : nullptr);
        HIPCHK(hipGetLastError());
        return PS_OK;
    }));
    // the label rounds of cluster_device: labels only decrease, so a hook round that moves nothing comes within N rounds
    uint64_t rounds = 0;
    if (g.adj) {
        PSCHK(tm.timed(4, s0, [&]() -> int {
            for (;;) {
                if (rounds == g.N) return ps_fail(PS_ERR_STATE, "the labels of %u individuals still moved in round %u", g.N, g.N);
                rounds++;
                uint32_t changed = 0;
                HIPCHK(hipMemsetAsync(s.changed, 0, sizeof(uint32_t), s0));
                cluster_hook_kernel<<<std::min((g.N + 3u) / 4u, 2048u), 256, 0, s0>>>(s.adj, g.N, s.cx, s.changed);
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpyAsync(&changed, s.changed, sizeof changed, hipMemcpyDeviceToHost, s0));
                HIPCHK(hipStreamSynchronize(s0));
                if (!changed) return PS_OK;
                cluster_jump_kernel<<<(g.N + 255u) / 256u, 256, 0, s0>>>(g.N, s.cx);
                HIPCHK(hipGetLastError());
            }
        }));
    }
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the bins and the per-locus pairs are copied as they are");
    HIPCHK(hipMemcpyAsync(w, s.words, sizeof w, hipMemcpyDeviceToHost, s0));
    HIPCHK(hipMemcpyAsync(hist, s.hist, prm->dist_bins * 8ull, hipMemcpyDeviceToHost, s0));
    HIPCHK(hipMemcpyAsync(locus_alleles, s.alleles, g.M * 4ull, hipMemcpyDeviceToHost, s0));
    HIPCHK(hipMemcpyAsync(locus_same_pairs, s.same, g.M * 8ull, hipMemcpyDeviceToHost, s0));
    HIPCHK(hipMemcpyAsync(h_st.data(), s.st, g.N * 4ull, hipMemcpyDeviceToHost, s0));
    HIPCHK(hipMemcpyAsync(h_cx.data(), g.adj ? s.cx : s.st, g.N * 4ull, hipMemcpyDeviceToHost, s0));
    if (profiles) {
        h_ids.resize((uint64_t)g.M * g.ldn);
        HIPCHK(hipMemcpyAsync(h_ids.data(), s.ids, (uint64_t)g.M * g.ldn * 2, hipMemcpyDeviceToHost, s0));
    }
    HIPCHK(hipStreamSynchronize(s0));
    PSCHK(tm.collect(ro, 5));
    uint64_t bad = w[PS_MLST_BAD];
    for (size_t k = 1; k < K; k++) bad += h_bad[k];
    if (bad)
        return ps_fail(PS_ERR_STATE, "%llu (locus, individual) entries differ from the representative of their fingerprint class: the %u-bit "
                                     "fingerprints collided; call again with another key_seed", (unsigned long long)bad, prm->key_bits);
    if (profiles)
        for (uint64_t k = 0; k < g.N; k++)
            for (uint64_t l = 0; l < g.M; l++) profiles[k * g.M + l] = h_ids[l * g.ldn + k];
    mlst_finish(out, g.N, L, h_bounds[g.M] - h_bounds[0], prm, locus_alleles, h_st.data(), h_cx.data(), st, complex_of, w[PS_MLST_SUM],
                0xFFFFFFFFull - w[PS_MLST_MININV], w[PS_MLST_MAX], w[PS_MLST_IDENT], w[PS_MLST_EDGES], rounds);
    return PS_OK;
}

static int mlst_core_handle(const ps_population *p, const char *call)
{
    if (!p->cfg.core) return ps_fail(PS_ERR_INVALID, "%s cuts the core matrix into loci: it takes a core handle", call);
    return PS_OK;
}

extern "C" int ps_allele_profiles(ps_population *core, const ps_mlst_params *prm, const uint64_t *bounds, ps_mlst_t *out, uint32_t *locus_alleles,
                                  uint64_t *locus_same_pairs, uint32_t *st, uint32_t *complex_of, uint64_t *hist, uint16_t *profiles)
{
    PSCHK(ps_needs_device());
    if (!core || !prm || !out || !locus_alleles || !locus_same_pairs || !st || !complex_of || !hist) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(mlst_core_handle(core, "ps_allele_profiles"));
    if (core->cfg.ncols != core->cfg.global_cols)
        return ps_fail(PS_ERR_INVALID, "ps_allele_profiles cuts all %llu core sites into loci; this handle is one site shard ([%llu, %llu)): use "
                                       "ps_multi_allele_profiles", (unsigned long long)core->cfg.global_cols, (unsigned long long)core->cfg.col_offset,
                       (unsigned long long)(core->cfg.col_offset + core->cfg.ncols));
    return mlst_run({ core }, core->cfg.ncols, prm, bounds, out, locus_alleles, locus_same_pairs, st, complex_of, hist, profiles);
}

extern "C" int ps_sim_allele_profiles(ps_sim *s, const ps_mlst_params *prm, const uint64_t *bounds, ps_mlst_t *out, uint32_t *locus_alleles,
                                      uint64_t *locus_same_pairs, uint32_t *st, uint32_t *complex_of, uint64_t *hist, uint16_t *profiles)
{
    PSCHK(ps_needs_device());
    if (!s) return ps_fail(PS_ERR_INVALID, "null argument");
    // (no ps_sim_sync: the call is ordered behind the run on the core stream)
    return ps_allele_profiles(s->core, prm, bounds, out, locus_alleles, locus_same_pairs, st, complex_of, hist, profiles);
}

extern "C" int ps_multi_allele_profiles(ps_multi *m, const ps_mlst_params *prm, const uint64_t *bounds, ps_mlst_t *out, uint32_t *locus_alleles,
                                        uint64_t *locus_same_pairs, uint32_t *st, uint32_t *complex_of, uint64_t *hist, uint16_t *profiles)
{
    PSCHK(ps_needs_device());
    if (!m || !prm || !out || !locus_alleles || !locus_same_pairs || !st || !complex_of || !hist) return ps_fail(PS_ERR_INVALID, "null argument");
    if (m->shard.size() == 1) return ps_sim_allele_profiles(m->shard[0], prm, bounds, out, locus_alleles, locus_same_pairs, st, complex_of, hist, profiles);
    // (part 0 reads the others' tables only after their streams have been synchronised, and they its representatives)
    PSCHK(ps_multi_sync(m));
    std::vector<ps_population *> parts;
    for (ps_sim *s : m->shard) parts.push_back(s->core);
    return mlst_run(parts, m->prm.core_size, prm, bounds, out, locus_alleles, locus_same_pairs, st, complex_of, hist, profiles);
}

extern "C" int ps_allele_profiles_timing(ps_population *core, double *fingerprint_ms, double *canon_ms, double *verify_ms, double *pairs_ms,
                                         double *labels_ms)
{
    if (!core) return ps_fail(PS_ERR_INVALID, "null argument");
    return readout_timing(core->ro[PS_RO_MLST], "no allele profiles have been computed on this handle",
                          { fingerprint_ms, canon_ms, verify_ms, pairs_ms, labels_ms });
}
