// sample_plan.h -- the host arithmetic of the core gather of the isolate samples (isolate_samples.h, sample_kernels.h;
// docs/ISOLATE_SAMPLES.md): which form a launch takes and its grid.  Plain C++ without HIP, so that a host program of its own can
// hold it to its invariants (tests/sample_plan_check.cpp).
#pragma once

#include <algorithm>
#include <cstdint>

// source rows of at most this many bytes are staged in LDS (their indices then fit 16 bits)
#define PS_GATHER_LDS_PITCH 65536u
// the LDS a workgroup of the LDS form stages at most when a source row leaves the choice (blockDim.y rows; five workgroups to a CU)
#define PS_GATHER_LDS_BYTES 32768u
// threads of a workgroup of the LDS form, at least: those without a chunk of their own still stage the source rows
#define PS_GATHER_MIN_THREADS 256u
// 16-byte chunks of an output row that one thread of core_gather_rows_kernel assembles, at most
#define PS_GATHER_MAX_CHUNKS 4u
// the direct form is chosen for PS_GATHER_DIRECT_RATIO x n < pitch.  Measured on an MI355X at L = 1.2 M sites
// (profiles/isolate_samples.md): the LDS form costs one pass over the source whatever n is, the direct form grows with n (a byte
// load moves a cache line): within 5 % of it from n = 32 to 64 at pitch 1024, and across it between n = 128 and 192 at pitch 8192
#define PS_GATHER_DIRECT_RATIO 48u

// THE switch between the two forms of core_gather_rows_kernel.  form: the tuning key "gather_form" of the source handle (0 =
// choose, 1 = LDS, 2 = direct); a source row that does not fit the LDS is gathered directly whatever the key says.
static inline bool core_gather_direct(int form, uint32_t pitch_in, uint64_t n)
{
    if (pitch_in > PS_GATHER_LDS_PITCH) return true;
    if (form) return form == 2;
    return (uint64_t)PS_GATHER_DIRECT_RATIO * n < pitch_in;
}

// One launch of core_gather_rows_kernel<ch, direct>: block (tx, sy), grid (tiles, runs), `lds` bytes of dynamic LDS
struct gather_plan {
    bool direct = false;
    uint32_t ch = 1, tx = 1, sy = 1, tiles = 1, runs = 1, sites_per_wg = 1, lds = 0;
};

// the launch that writes the bytes [off, own_end) of the output rows of L sites from source rows of pitch_in bytes (n = the
// gathered bytes in front of the zeros; own_end > off, L >= 1)
static inline gather_plan core_gather_plan(int form, uint32_t pitch_in, uint32_t n, uint32_t off, uint32_t own_end, uint64_t L)
{
    gather_plan g;
    g.direct = core_gather_direct(form, pitch_in, n);
    const uint64_t nchunks = ((uint64_t)own_end + 15u) / 16u - off / 16u;
    g.ch = g.direct || nchunks <= 1024u ? 1u : nchunks <= 2048u ? 2u : PS_GATHER_MAX_CHUNKS;
    const uint64_t need = (nchunks + g.ch - 1u) / g.ch;          // threads along x
    g.tx = 1u;
    while (g.tx < 1024u && g.tx < need) g.tx <<= 1;
    g.sy = std::max(1u, PS_GATHER_MIN_THREADS / g.tx);
    if (!g.direct) g.sy = std::max(1u, std::min(g.sy, PS_GATHER_LDS_BYTES / pitch_in));
    g.sy = (uint32_t)std::min<uint64_t>(g.sy, L);
    if (!g.direct)
        while (g.tx * g.sy < PS_GATHER_MIN_THREADS) g.tx <<= 1;
    g.tiles = (uint32_t)((need + g.tx - 1u) / g.tx);
    g.lds = g.direct ? 0u : g.sy * pitch_in;
    // runs of sites: about 4096 workgroups per tile column, and at least four rounds of sy sites per workgroup, which pay for
    // the index registers
    uint64_t per = std::max<uint64_t>(4ull * g.sy, (L + 4095u) / 4096u);
    per = (per + g.sy - 1u) / g.sy * g.sy;
    per = std::min<uint64_t>(per, 0x7FFFFF00ull);
    g.sites_per_wg = (uint32_t)per;
    g.runs = (uint32_t)((L + per - 1u) / per);
    return g;
}
