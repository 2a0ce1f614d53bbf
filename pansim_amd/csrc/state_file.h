// state_file.h -- ps_sim_save / ps_sim_load / ps_state_info (include/pansim_hip.h; the format: docs/STATE_FORMAT.md).
// Included by pansim_capi.hip behind struct ps_sim and the row-map code it reads and restores.
//
// The core section is streamed in CHUNKS of site rows: one chunk buffer on the device (packed form only), two pinned ones on
// the host; the device pass + copy of chunk k overlaps the file I/O of chunk k -+ 1, as ps_write does for _core_genome.csv.
// Peak extra memory is three chunks whatever L is (64 MiB each by default; PANSIM_STATE_CHUNK_ROWS sets the rows per chunk:
// a test hook, the file does not depend on it).
#pragma once

#include "state_kernels.h"

#define PS_STATE_HEADER_BYTES 4096u
#define PS_STATE_VERSION 1u
static const char PS_STATE_MAGIC[8] = { 'P', 'A', 'N', 'S', 'I', 'M', 'S', 'T' };
static const char *const PS_STATE_SECTION[4] = { "core", "accessory", "row-map", "per-generation" };

struct state_hdr {
    ps_state_header pub{};
    ps_sim_params prm{};
    uint64_t sum[4] = {};      // core, accessory, row maps, per generation
};

// sum of ps_state_mix over the little-endian u32 words of `data` (bytes: a multiple of 4), the first one at index j0
static uint64_t state_checksum(const void *data, uint64_t bytes, uint64_t j0 = 0)
{
    const uint8_t *b = (const uint8_t *)data;
    uint64_t sum = 0;
    for (uint64_t j = 0; j < bytes / 4; j++) {
        uint32_t w;
        memcpy(&w, b + 4 * j, 4);
        sum += ps_state_mix(w, j0 + j);
    }
    return sum;
}

static uint64_t state_align(uint64_t x) { return (x + 4095ull) & ~4095ull; }

// section table of a file from its geometry (the decoder recomputes it: a header that disagrees is refused)
static void state_layout(ps_state_header *h, uint64_t N, uint64_t per_gen_rows)
{
    const uint64_t L = h->site_end - h->site_begin, GW = (h->pan_size + 63) / 64;
    h->pitch = (N + 127) / 128 * 128;
    h->core_offset = PS_STATE_HEADER_BYTES;
    h->core_bytes = L * (h->core_encoding == PS_STATE_PACKED2 ? h->pitch / 4 : h->pitch);
    h->acc_offset = state_align(h->core_offset + h->core_bytes);
    h->acc_bytes = N * GW * 8;
    h->maps_offset = state_align(h->acc_offset + h->acc_bytes);
    h->maps_bytes = 2 * N * 4;
    h->per_gen_offset = state_align(h->maps_offset + h->maps_bytes);
    h->per_gen_bytes = h->has_per_gen ? per_gen_rows * 32 : 0;
}

template <typename T>
static void state_put(uint8_t *hdr, size_t off, T v) { memcpy(hdr + off, &v, sizeof v); }
template <typename T>
static T state_get(const uint8_t *hdr, size_t off) { T v; memcpy(&v, hdr + off, sizeof v); return v; }

static void state_encode_header(const state_hdr &h, uint8_t *out /* PS_STATE_HEADER_BYTES */)
{
    memset(out, 0, PS_STATE_HEADER_BYTES);
    const ps_state_header &p = h.pub;
    memcpy(out, PS_STATE_MAGIC, 8);
    state_put<uint32_t>(out, 8, p.version);
    state_put<uint32_t>(out, 12, PS_STATE_HEADER_BYTES);
    state_put<uint32_t>(out, 24, p.core_encoding);
    state_put<uint32_t>(out, 28, (p.has_row_maps ? 1u : 0u) | (p.core_rows_overridden ? 2u : 0u) | (p.acc_rows_overridden ? 4u : 0u)
                                     | (p.has_per_gen ? 8u : 0u));
    state_put<uint64_t>(out, 32, p.generations_done);
    state_put<uint64_t>(out, 40, p.pan_size);
    state_put<uint64_t>(out, 48, p.site_begin);
    state_put<uint64_t>(out, 56, p.site_end);
    state_put<uint64_t>(out, 64, p.pitch);
    state_put<uint64_t>(out, 72, (p.pan_size + 63) / 64);
    const uint64_t sec[4][2] = { { p.core_offset, p.core_bytes }, { p.acc_offset, p.acc_bytes }, { p.maps_offset, p.maps_bytes },
                                 { p.per_gen_offset, p.per_gen_bytes } };
    for (int k = 0; k < 4; k++) {
        state_put<uint64_t>(out, 80 + 24 * k, sec[k][0]);
        state_put<uint64_t>(out, 88 + 24 * k, sec[k][1]);
        state_put<uint64_t>(out, 96 + 24 * k, h.sum[k]);
    }
    const ps_sim_params &q = h.prm;
    size_t o = 192;
    auto u = [&](uint64_t v) { state_put<uint64_t>(out, o, v); o += 8; };
    auto i = [&](int64_t v) { state_put<int64_t>(out, o, v); o += 8; };
    auto d = [&](double v) { state_put<double>(out, o, v); o += 8; };
    u(q.pop_size); u(q.core_size); u(q.pan_genes); u(q.core_genes);
    d(q.avg_gene_freq); d(q.HR_rate); d(q.HGT_rate);
    i(q.n_gen); u(q.max_distances);
    d(q.core_mu); d(q.rate_genes1); d(q.rate_genes2); d(q.prop_genes2); d(q.prop_positive); d(q.pos_lambda); d(q.neg_lambda);
    u(q.seed);
    i(q.print_dist); i(q.print_matrices); i(q.print_selection); i(q.verbose); i(q.no_control_genome_size);
    d(q.genome_size_penalty); d(q.competition_strength);
    i(q.shard_rank); i(q.shard_count); i(q.device); i(q.reference_seed_stream);
    state_put<uint64_t>(out, 16, state_checksum(out, PS_STATE_HEADER_BYTES));      // (computed with the field itself zero)
}

// read and check the header of an open file: magic, version, checksum, section table, length
static int state_decode_header(FILE *f, const char *path, state_hdr *h)
{
    uint8_t raw[PS_STATE_HEADER_BYTES];
    if (fseek(f, 0, SEEK_END) != 0) return ps_fail(PS_ERR_IO, "%s: cannot seek", path);
    const long long flen = ftello(f);
    if (fseek(f, 0, SEEK_SET) != 0 || flen < (long long)PS_STATE_HEADER_BYTES || fread(raw, 1, sizeof raw, f) != sizeof raw)
        return ps_fail(PS_ERR_IO, "%s: truncated header (a state file starts with %u bytes of header)", path, PS_STATE_HEADER_BYTES);
    if (memcmp(raw, PS_STATE_MAGIC, 8) != 0) return ps_fail(PS_ERR_IO, "%s: header: bad magic, not a pansim state file", path);
    const uint32_t version = state_get<uint32_t>(raw, 8);
    if (version != PS_STATE_VERSION || state_get<uint32_t>(raw, 12) != PS_STATE_HEADER_BYTES)
        return ps_fail(PS_ERR_IO, "%s: header: unsupported format version %u (this library reads version %u)", path, version, PS_STATE_VERSION);
    {
        const uint64_t stored = state_get<uint64_t>(raw, 16);
        uint8_t tmp[PS_STATE_HEADER_BYTES];
        memcpy(tmp, raw, sizeof tmp);
        memset(tmp + 16, 0, 8);
        if (state_checksum(tmp, sizeof tmp) != stored) return ps_fail(PS_ERR_IO, "%s: header: checksum mismatch", path);
    }
    ps_state_header &p = h->pub;
    p.version = version;
    p.core_encoding = state_get<uint32_t>(raw, 24);
    const uint32_t flags = state_get<uint32_t>(raw, 28);
    p.has_row_maps = (flags & 1u) != 0;
    p.core_rows_overridden = (flags & 2u) != 0;
    p.acc_rows_overridden = (flags & 4u) != 0;
    p.has_per_gen = (flags & 8u) != 0;
    p.generations_done = state_get<uint64_t>(raw, 32);
    p.pan_size = state_get<uint64_t>(raw, 40);
    p.site_begin = state_get<uint64_t>(raw, 48);
    p.site_end = state_get<uint64_t>(raw, 56);
    ps_sim_params &q = h->prm;
    memset(&q, 0, sizeof q);
    size_t o = 192;
    auto u = [&]() { const uint64_t v = state_get<uint64_t>(raw, o); o += 8; return v; };
    auto i = [&]() { const int64_t v = state_get<int64_t>(raw, o); o += 8; return (int32_t)v; };
    auto d = [&]() { const double v = state_get<double>(raw, o); o += 8; return v; };
    q.pop_size = u(); q.core_size = u(); q.pan_genes = u(); q.core_genes = u();
    q.avg_gene_freq = d(); q.HR_rate = d(); q.HGT_rate = d();
    q.n_gen = i(); q.max_distances = u();
    q.core_mu = d(); q.rate_genes1 = d(); q.rate_genes2 = d(); q.prop_genes2 = d(); q.prop_positive = d(); q.pos_lambda = d(); q.neg_lambda = d();
    q.seed = u();
    q.print_dist = i(); q.print_matrices = i(); q.print_selection = i(); q.verbose = i(); q.no_control_genome_size = i();
    q.genome_size_penalty = d(); q.competition_strength = d();
    q.shard_rank = i(); q.shard_count = i(); q.device = i(); q.reference_seed_stream = i();
    // the geometry must be the one the parameters give, and the section table the one the geometry gives
    ps_derived der{};
    if (ps_sim_derive(&q, &der) != PS_OK || der.pan_size != p.pan_size || q.shard_count < 1 || q.shard_rank < 0 || q.shard_rank >= q.shard_count
        || p.site_begin != q.core_size * (uint64_t)q.shard_rank / (uint64_t)q.shard_count
        || p.site_end != q.core_size * ((uint64_t)q.shard_rank + 1) / (uint64_t)q.shard_count
        || q.pop_size < 1 || q.pop_size > 0xFFFFFFFFull - 128 || q.core_size > 0xFFFFFFFFull || p.pan_size > 65536
        || p.generations_done > 0xFFFFFFFFull || (p.core_encoding != PS_STATE_PACKED2 && p.core_encoding != PS_STATE_RAW8))
        return ps_fail(PS_ERR_IO, "%s: header: the geometry does not follow from the stored parameters", path);
    state_layout(&p, q.pop_size, p.generations_done);
    const uint64_t sec[4][2] = { { p.core_offset, p.core_bytes }, { p.acc_offset, p.acc_bytes }, { p.maps_offset, p.maps_bytes },
                                 { p.per_gen_offset, p.per_gen_bytes } };
    if (state_get<uint64_t>(raw, 64) != p.pitch || state_get<uint64_t>(raw, 72) != (p.pan_size + 63) / 64)
        return ps_fail(PS_ERR_IO, "%s: header: pitch or accessory row words do not follow from the geometry", path);
    for (int k = 0; k < 4; k++) {
        if (state_get<uint64_t>(raw, 80 + 24 * k) != sec[k][0] || state_get<uint64_t>(raw, 88 + 24 * k) != sec[k][1])
            return ps_fail(PS_ERR_IO, "%s: header: the %s section is not where the geometry puts it", path, PS_STATE_SECTION[k]);
        h->sum[k] = state_get<uint64_t>(raw, 96 + 24 * k);
        if ((uint64_t)flen < sec[k][0] + sec[k][1])
            return ps_fail(PS_ERR_IO, "%s: truncated: the %s section ends at byte %llu, the file has %lld", path, PS_STATE_SECTION[k],
                           (unsigned long long)(sec[k][0] + sec[k][1]), flen);
    }
    return PS_OK;
}

// read a small section whole and check its sum
static int state_read_section(FILE *f, const char *path, int k, uint64_t offset, uint64_t bytes, uint64_t want, void *out)
{
    if (bytes == 0) return PS_OK;
    if (fseeko(f, (off_t)offset, SEEK_SET) != 0 || fread(out, 1, bytes, f) != bytes)
        return ps_fail(PS_ERR_IO, "%s: %s section: short read", path, PS_STATE_SECTION[k]);
    if (state_checksum(out, bytes) != want) return ps_fail(PS_ERR_IO, "%s: %s section: checksum mismatch", path, PS_STATE_SECTION[k]);
    return PS_OK;
}

extern "C" int ps_state_info(const char *path, ps_sim_params *params_out, ps_state_header *hdr_out, double *per_gen_out, uint64_t cap)
{
    if (!path) return ps_fail(PS_ERR_INVALID, "null argument");
    FILE *f = fopen(path, "rb");
    if (!f) return ps_fail(PS_ERR_IO, "cannot open %s", path);
    state_hdr h;
    int rc = state_decode_header(f, path, &h);
    if (rc == PS_OK && per_gen_out) {
        if (!h.pub.has_per_gen) rc = ps_fail(PS_ERR_INVALID, "%s has no per-generation section", path);
        else if (cap < h.pub.per_gen_bytes / 8) rc = ps_fail(PS_ERR_INVALID, "the per-generation section holds %llu doubles, the buffer %llu",
                                                             (unsigned long long)(h.pub.per_gen_bytes / 8), (unsigned long long)cap);
        else rc = state_read_section(f, path, 3, h.pub.per_gen_offset, h.pub.per_gen_bytes, h.sum[3], per_gen_out);
    }
    fclose(f);
    if (rc != PS_OK) return rc;
    if (params_out) *params_out = h.prm;
    if (hdr_out) *hdr_out = h.pub;
    return PS_OK;
}

// site rows per chunk of the core section: 64 MiB of file bytes, or PANSIM_STATE_CHUNK_ROWS; a chunk's 16-cell pieces fit 31 bits
static uint64_t state_chunk_rows(uint64_t L, uint64_t row_file_bytes, uint32_t cpr)
{
    uint64_t rows = std::max<uint64_t>(1, (64ull << 20) / row_file_bytes);
    const long long v = env_int("PANSIM_STATE_CHUNK_ROWS", 0);
    if (v >= 1) rows = (uint64_t)v;
    rows = std::min<uint64_t>(rows, std::max<uint64_t>(1, (1ull << 30) / row_file_bytes));
    rows = std::min<uint64_t>(rows, ((1ull << 31) - 1) / cpr);
    return std::max<uint64_t>(1, std::min(rows, L));
}

struct state_bufs {
    hipStream_t st = nullptr;
    uint8_t *d_chunk = nullptr, *h[2] = { nullptr, nullptr };
    unsigned long long *d_sum = nullptr;      // [0] the checksum, [1] the "not one-hot" flag
    int alloc(uint64_t bytes, bool device_chunk)
    {
        if ((device_chunk && hipMalloc(&d_chunk, bytes) != hipSuccess) || hipMalloc(&d_sum, 16) != hipSuccess
            || hipHostMalloc(&h[0], bytes) != hipSuccess || hipHostMalloc(&h[1], bytes) != hipSuccess) {
            (void)hipGetLastError();
            return ps_fail(PS_ERR_OOM, "cannot allocate the chunk buffers of the state file (%llu bytes each)", (unsigned long long)bytes);
        }
        HIPCHK(hipMemsetAsync(d_sum, 0, 16, st));
        return PS_OK;
    }
    ~state_bufs()
    {
        if (st) (void)hipStreamSynchronize(st);      // (an early return leaves a copy in flight)
        if (d_chunk) (void)hipFree(d_chunk);
        if (d_sum) (void)hipFree(d_sum);
        for (auto *p : h) if (p) (void)hipHostFree(p);
    }
};

static uint32_t state_blocks(uint32_t items) { return std::min<uint32_t>((items + 255u) / 256u, 4096u); }

// the core section of handle c to the file at its current position; packed form: *bad_out = a cell is not 1 / 2 / 4 / 8
static int state_save_core(ps_population *c, FILE *f, const char *path, uint32_t enc, uint64_t *sum_out, bool *bad_out)
{
    const uint64_t L = c->cfg.ncols;
    const uint32_t N = (uint32_t)c->cfg.pop_size, pitch = c->pitch, cpr = c->cpr;
    const bool packed = enc == PS_STATE_PACKED2;
    *sum_out = 0;
    *bad_out = false;
    if (!L) return PS_OK;
    const uint64_t rb = packed ? pitch / 4 : pitch;
    const uint64_t chunk = state_chunk_rows(L, rb, cpr);
    state_bufs b;
    b.st = c->stream;
    PSCHK(b.alloc(chunk * rb, packed));
    uint64_t host_sum = 0, pending_bytes = 0, pending_j0 = 0;
    int pending = -1, k = 0;
    auto flush = [&]() -> int {
        if (pending < 0) return PS_OK;
        if (!packed) host_sum += state_checksum(b.h[pending], pending_bytes, pending_j0);
        if (fwrite(b.h[pending], 1, pending_bytes, f) != pending_bytes) return ps_fail(PS_ERR_IO, "short write to %s", path);
        return PS_OK;
    };
    for (uint64_t r0 = 0; r0 < L; r0 += chunk, k ^= 1) {
        const uint64_t nr = std::min(chunk, L - r0), bytes = nr * rb;
        const uint8_t *rows = c->state + r0 * pitch;
        if (packed) {
            const uint32_t items = (uint32_t)(nr * cpr);
            core_state_pack2_kernel<<<state_blocks(items), 256, 0, b.st>>>(rows, (uint32_t *)b.d_chunk, items, cpr, N, r0 * cpr, b.d_sum,
                                                                         (uint32_t *)(b.d_sum + 1));
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(b.h[k], b.d_chunk, bytes, hipMemcpyDeviceToHost, b.st));
        } else {
            HIPCHK(hipMemcpyAsync(b.h[k], rows, bytes, hipMemcpyDeviceToHost, b.st));
        }
        PSCHK(flush());                               // (the chunk before, while this one is produced)
        HIPCHK(hipStreamSynchronize(b.st));
        pending = k;
        pending_bytes = bytes;
        pending_j0 = r0 * rb / 4;
    }
    PSCHK(flush());
    if (packed) {
        unsigned long long res[2] = { 0, 0 };
        HIPCHK(hipMemcpyAsync(res, b.d_sum, 16, hipMemcpyDeviceToHost, b.st));
        HIPCHK(hipStreamSynchronize(b.st));
        *sum_out = res[0];
        *bad_out = (uint32_t)res[1] != 0u;
    } else {
        *sum_out = host_sum;
    }
    return PS_OK;
}

// the inverse: the core section of the file into the handle's matrix, checksum compared at the end
static int state_load_core(ps_population *c, FILE *f, const char *path, const state_hdr &h)
{
    const uint64_t L = c->cfg.ncols;
    const uint32_t N = (uint32_t)c->cfg.pop_size, pitch = c->pitch, cpr = c->cpr;
    const bool packed = h.pub.core_encoding == PS_STATE_PACKED2;
    c->nibble_safe = c->onehot_safe = true;
    if (!L) return PS_OK;
    const uint64_t rb = packed ? pitch / 4 : pitch;
    const uint64_t chunk = state_chunk_rows(L, rb, cpr);
    state_bufs b;
    b.st = c->stream;
    PSCHK(b.alloc(chunk * rb, packed));
    if (fseeko(f, (off_t)h.pub.core_offset, SEEK_SET) != 0) return ps_fail(PS_ERR_IO, "%s: core section: cannot seek", path);
    auto read_chunk = [&](uint64_t r0, int k) -> int {
        const uint64_t bytes = std::min(chunk, L - r0) * rb;
        if (fread(b.h[k], 1, bytes, f) != bytes) return ps_fail(PS_ERR_IO, "%s: core section: short read", path);
        return PS_OK;
    };
    PSCHK(read_chunk(0, 0));
    uint64_t host_sum = 0;
    bool nibble = true, onehot = true;
    int k = 0;
    for (uint64_t r0 = 0; r0 < L; r0 += chunk, k ^= 1) {
        const uint64_t nr = std::min(chunk, L - r0), bytes = nr * rb;
        uint8_t *rows = c->state + r0 * pitch;
        if (packed) {
            const uint32_t items = (uint32_t)(nr * cpr);
            HIPCHK(hipMemcpyAsync(b.d_chunk, b.h[k], bytes, hipMemcpyHostToDevice, b.st));
            core_state_unpack2_kernel<<<state_blocks(items), 256, 0, b.st>>>((const uint32_t *)b.d_chunk, rows, items, cpr, N, r0 * cpr, b.d_sum);
            HIPCHK(hipGetLastError());
        } else {
            // rows as they are: the sum over what the file holds, then zeros into the padding cells, and what ps_load_matrix
            // would have found out about the bytes
            host_sum += state_checksum(b.h[k], bytes, r0 * rb / 4);
            for (uint64_t r = 0; r < nr; r++) {
                uint8_t *row = b.h[k] + r * pitch;
                for (uint32_t i = 0; i < N; i++) {
                    const uint8_t v = row[i];
                    if (v > 15) nibble = false;
                    if (v != 1 && v != 2 && v != 4 && v != 8) onehot = false;
                }
                memset(row + N, 0, pitch - N);
            }
            HIPCHK(hipMemcpyAsync(rows, b.h[k], bytes, hipMemcpyHostToDevice, b.st));
        }
        if (r0 + chunk < L) PSCHK(read_chunk(r0 + chunk, k ^ 1));       // (the next chunk, while this one is consumed)
        HIPCHK(hipStreamSynchronize(b.st));
    }
    uint64_t sum = host_sum;
    if (packed) {
        unsigned long long res[2] = { 0, 0 };
        HIPCHK(hipMemcpyAsync(res, b.d_sum, 16, hipMemcpyDeviceToHost, b.st));
        HIPCHK(hipStreamSynchronize(b.st));
        sum = res[0];
    }
    if (sum != h.sum[0]) return ps_fail(PS_ERR_IO, "%s: core section: checksum mismatch", path);
    c->nibble_safe = nibble;
    c->onehot_safe = onehot;
    return PS_OK;
}

static int state_pad_to(FILE *f, const char *path, uint64_t offset)
{
    static const uint8_t zeros[4096] = {};
    const long long at = ftello(f);
    if (at < 0 || (uint64_t)at > offset) return ps_fail(PS_ERR_IO, "%s: a section ran past its place", path);
    for (uint64_t left = offset - (uint64_t)at; left;) {
        const uint64_t n = std::min<uint64_t>(left, sizeof zeros);
        if (fwrite(zeros, 1, n, f) != n) return ps_fail(PS_ERR_IO, "short write to %s", path);
        left -= n;
    }
    return PS_OK;
}

static int state_write_section(FILE *f, const char *path, uint64_t offset, const void *data, uint64_t bytes, uint64_t *sum)
{
    PSCHK(state_pad_to(f, path, offset));
    *sum = state_checksum(data, bytes);
    if (bytes && fwrite(data, 1, bytes, f) != bytes) return ps_fail(PS_ERR_IO, "short write to %s", path);
    return PS_OK;
}

static int sim_save_impl(ps_sim *s, FILE *f, const char *path, const double *per_gen)
{
    ps_population *core = s->core, *acc = s->acc;
    const uint64_t N = s->prm.pop_size;
    state_hdr h;
    h.prm = s->prm;
    ps_state_header &p = h.pub;
    p.version = PS_STATE_VERSION;
    p.generations_done = s->gens_done;
    p.pan_size = acc->cfg.ncols;
    p.site_begin = core->cfg.col_offset;
    p.site_end = core->cfg.col_offset + core->cfg.ncols;
    p.has_per_gen = per_gen != nullptr;
    p.core_rows_overridden = core->rows_overridden;
    p.acc_rows_overridden = acc->rows_overridden;
    // row maps: sigma of the last generation (output row -> internal row), and the last draws named by the output rows of
    // the generation before -- what sim_refresh_rows and ps_sim_last_parents answer right now
    std::vector<uint32_t> maps(2 * N, 0u);
    if (s->step_count) {
        PSCHK(sim_refresh_rows(s));
        memcpy(maps.data(), s->sigma.data(), N * sizeof(uint32_t));
        PSCHK(ps_sim_last_parents(s, maps.data() + N));
        p.has_row_maps = 1;
    }
    uint8_t raw[PS_STATE_HEADER_BYTES] = {};
    if (fwrite(raw, 1, sizeof raw, f) != sizeof raw) return ps_fail(PS_ERR_IO, "short write to %s", path);
    // the handle's onehot_safe decides the encoding up front; the pack pass's own check is the safety net
    p.core_encoding = core->onehot_safe ? PS_STATE_PACKED2 : PS_STATE_RAW8;
    state_layout(&p, N, p.generations_done);
    bool bad = false;
    PSCHK(state_save_core(core, f, path, p.core_encoding, &h.sum[0], &bad));
    if (bad) {
        p.core_encoding = PS_STATE_RAW8;
        state_layout(&p, N, p.generations_done);
        if (fseeko(f, (off_t)p.core_offset, SEEK_SET) != 0) return ps_fail(PS_ERR_IO, "%s: cannot seek", path);
        PSCHK(state_save_core(core, f, path, p.core_encoding, &h.sum[0], &bad));
    }
    {
        std::vector<uint64_t> rows(std::max<uint64_t>(p.acc_bytes / 8, 1));
        if (p.acc_bytes) {
            HIPCHK(hipMemcpyAsync(rows.data(), acc->I[acc->cur], p.acc_bytes, hipMemcpyDeviceToHost, acc->stream));
            HIPCHK(hipStreamSynchronize(acc->stream));
        }
        PSCHK(state_write_section(f, path, p.acc_offset, rows.data(), p.acc_bytes, &h.sum[1]));
    }
    PSCHK(state_write_section(f, path, p.maps_offset, maps.data(), p.maps_bytes, &h.sum[2]));
    PSCHK(state_write_section(f, path, p.per_gen_offset, per_gen, p.per_gen_bytes, &h.sum[3]));
    state_encode_header(h, raw);
    if (fseeko(f, 0, SEEK_SET) != 0 || fwrite(raw, 1, sizeof raw, f) != sizeof raw || fflush(f) != 0)
        return ps_fail(PS_ERR_IO, "short write to %s", path);
    return PS_OK;
}

extern "C" int ps_sim_save(ps_sim *s, const char *path, const double *per_gen)
{
    if (!s || !path) return ps_fail(PS_ERR_INVALID, "null argument");
    PSCHK(ps_sim_sync(s));
    FILE *f = fopen(path, "wb");
    if (!f) return ps_fail(PS_ERR_IO, "cannot create %s", path);
    const int rc = sim_save_impl(s, f, path, per_gen);
    if (fclose(f) != 0 && rc == PS_OK) { (void)remove(path); return ps_fail(PS_ERR_IO, "cannot finish %s", path); }
    if (rc != PS_OK) (void)remove(path);
    return rc;
}

static int sim_load_impl(ps_sim *s, FILE *f, const char *path, const state_hdr &h)
{
    ps_population *core = s->core, *acc = s->acc;
    const ps_state_header &p = h.pub;
    const uint64_t N = s->prm.pop_size;
    PSCHK(use_device(core));
    PSCHK(state_load_core(core, f, path, h));
    if (p.acc_bytes) {
        std::vector<uint64_t> rows(p.acc_bytes / 8);
        PSCHK(state_read_section(f, path, 1, p.acc_offset, p.acc_bytes, h.sum[1], rows.data()));
        const uint64_t GW = acc->d.GW, G = acc->d.G;
        if (G % 64)       // (bits beyond the last gene are zero in the device's rows)
            for (uint64_t i = 0; i < N; i++) rows[i * GW + GW - 1] &= (1ull << (G % 64)) - 1ull;
        HIPCHK(hipMemcpyAsync(acc->I[acc->cur], rows.data(), p.acc_bytes, hipMemcpyHostToDevice, acc->stream));
        HIPCHK(hipStreamSynchronize(acc->stream));
    }
    acc->g_valid = false;
    acc->counts_fresh = false;
    acc->snap_valid = false;
    acc->edit_epoch++;
    s->avg_prefetched = false;
    std::vector<uint32_t> maps(2 * N);
    PSCHK(state_read_section(f, path, 2, p.maps_offset, p.maps_bytes, h.sum[2], maps.data()));
    if (p.has_row_maps) {
        // sigma must be a permutation and the parents rows: kernels gather through them
        std::vector<uint8_t> seen(N, 0);
        for (uint64_t k = 0; k < N; k++) {
            if (maps[k] >= N || seen[maps[k]] || maps[N + k] >= N) return ps_fail(PS_ERR_IO, "%s: row-map section: not a permutation of the rows", path);
            seen[maps[k]] = 1;
        }
        // As if one generation had been drawn whose stable sort is sigma: the draws "sigma" themselves sort to sigma (a
        // permutation is its own rank), so the NEXT generation finds the right previous order in that slot; until then
        // ps_sim_last_parents answers the stored parents through a lookup that sends sigma[k] to them.
        s->step_count = 1;
        s->last_slot = 0;
        s->prev_slot = -1;
        memcpy(s->h_draw[0], maps.data(), N * sizeof(uint32_t));
        s->sigma.assign(maps.begin(), maps.begin() + N);
        s->sigma_prev_inv.assign(N, 0u);
        for (uint64_t k = 0; k < N; k++) s->sigma_prev_inv[maps[k]] = maps[N + k];
        for (ps_population *q : { core, acc }) {
            q->row_slot = s->sigma;
            if (!q->d_row_slot) HIPCHK(hipMalloc(&q->d_row_slot, N * sizeof(uint32_t)));
            HIPCHK(hipMemcpyAsync(q->d_row_slot, s->sigma.data(), N * sizeof(uint32_t), hipMemcpyHostToDevice, q->stream));
            HIPCHK(hipStreamSynchronize(q->stream));
        }
        s->sigma_step = s->step_count;
    }
    core->rows_overridden = p.core_rows_overridden != 0;
    acc->rows_overridden = p.acc_rows_overridden != 0;
    s->gens_done = p.generations_done;
    return PS_OK;
}

extern "C" int ps_sim_load(const char *path, const ps_sim_params *params, ps_sim **out)
{
    if (!path || !out) return ps_fail(PS_ERR_INVALID, "null argument");
    *out = nullptr;
    PSCHK(ps_needs_device());
    FILE *f = fopen(path, "rb");
    if (!f) return ps_fail(PS_ERR_IO, "cannot open %s", path);
    state_hdr h;
    ps_sim *s = nullptr;
    int rc = state_decode_header(f, path, &h);
    ps_sim_params q = h.prm;
    if (rc == PS_OK) {
        if (params) {
            q = *params;
#define PS_STATE_SAME(field_)                                                                                                              \
    if (rc == PS_OK && q.field_ != h.prm.field_)                                                                                           \
        rc = ps_fail(PS_ERR_INVALID, "%s was saved with " #field_ " %lld, the parameters say %lld: a branch keeps the sizes and the shard", \
                     path, (long long)h.prm.field_, (long long)q.field_);
            PS_STATE_SAME(pop_size)
            PS_STATE_SAME(core_size)
            PS_STATE_SAME(pan_genes)
            PS_STATE_SAME(core_genes)
            PS_STATE_SAME(shard_rank)
            PS_STATE_SAME(shard_count)
#undef PS_STATE_SAME
        } else {
            q.device = -1;      // (the saved ordinal belongs to the machine that saved)
        }
    }
    if (rc == PS_OK) rc = ps_sim_create(&q, &s);
    if (rc == PS_OK) rc = sim_load_impl(s, f, path, h);
    fclose(f);
    if (rc != PS_OK) {
        const std::string keep = g_err;
        ps_sim_destroy(s);
        g_err = keep;
        return rc;
    }
    *out = s;
    return PS_OK;
}

extern "C" uint32_t ps_sim_generations_done(ps_sim *s) { return s ? (uint32_t)s->gens_done : 0u; }
