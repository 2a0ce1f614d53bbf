// diversity_kernels.h -- gfx950 kernel of the core allele counts and diversity summary (ps_site_allele_counts /
// ps_core_diversity, include/pansim_hip.h; the definitions: docs/CORE_DIVERSITY.md).
//
// The core matrix is site-major, so the N cells of a site are one contiguous row and its four base counts come from one
// streaming read of it: one WAVE per site row, 16 bytes per lane per load (nontemporal, as the sweeps' ps_load_row16) -- a
// row of N <= 1024 cells is one load per lane, a wider one is walked in 1 KiB pieces by the same wave, the next piece (or the
// wave's next row) in flight while the current one is counted.  Counting is by bit plane: plane a of a dword is
// w & (0x01010101 << a) and its population count is that dword's number of cells of base a (v_and + an accumulating v_bcnt: 8
// vector instructions per dword for the four bases).  That is exact as long as no byte of the row has two bits set or a bit
// above 8 -- every simulated state; a wave that meets such a byte (matrices of arbitrary bytes, ps_load_matrix) recounts the
// row with the exact form, which drops the bytes that are not 1 / 2 / 4 / 8.  Zero bytes count in no plane in either form.
// Cells at index >= N are masked out explicitly: nothing depends on what the pad bytes hold.  Planned at ~60 vector
// instructions per 1 KiB piece and ~50 per row for the reduction and the summary -- under the ~150 at which the row stream
// leaves its memory ceiling.
//
// The wave reduction is a transposing one: after the xor-32 and xor-16 exchanges a lane carries ONE base (lane / 16) of its
// four-lane column, four more steps finish it -- 7 exchanges instead of 24 -- and lanes 0 / 16 / 32 / 48 hold A / C / G / T.
// Everything behind it is wave-uniform integer arithmetic (ps_div_site_terms, shared with the host's ps_diversity_from_counts).
// Integer adds commute: results do not depend on the launch geometry or on the order of the atomics.
#pragma once

#include "state_kernels.h"

// words of the summary the kernel accumulates (u64 each)
enum { PS_DIV_PAIR = 0, PS_DIV_SEG = 1, PS_DIV_OTHER = 2, PS_DIV_BASE = 3, PS_DIV_WORDS = 8 };

// The per-site terms over the five classes A, C, G, T, other (docs/CORE_DIVERSITY.md): pairs of individuals that differ at
// the site, (N^2 - sum n_c^2) / 2 -- the difference is twice a sum of products, hence even --, whether at least two classes
// are non-empty, and the minor count N - max n_c (the spectrum bin).  N < 2^32, so nothing overflows 64 bits.
PS_HD void ps_div_site_terms(uint64_t N, uint64_t a, uint64_t c, uint64_t g, uint64_t t, uint64_t *pair, uint32_t *seg,
                             uint64_t *other, uint64_t *minor)
{
    const uint64_t o = N - (a + c + g + t);
    uint64_t mx = a > c ? a : c;
    const uint64_t m2 = g > t ? g : t;
    mx = mx > m2 ? mx : m2;
    mx = mx > o ? mx : o;
    *pair = (N * N - (a * a + c * c + g * g + t * t + o * o)) >> 1;
    *seg = ((a != 0) + (c != 0) + (g != 0) + (t != 0) + (o != 0)) >= 2 ? 1u : 0u;
    *other = o;
    *minor = N - mx;
}

// a dword whose set bits mark the bytes the plane counts cannot take as they are: two bits of the low nibble, or a high bit
__device__ __forceinline__ uint32_t ps_div_suspect(uint32_t w)
{
    // (per byte b: (b | 0x80) - 1 never borrows from its neighbour, and b & (b - 1) != 0 iff b has two bits)
    return (w & ((w | 0x80808080u) - 0x01010101u)) | (w & 0xF0F0F0F0u);
}

// the exact form: bit 0 of every byte of the result is set iff that byte is 1, 2, 4 or 8
__device__ __forceinline__ uint32_t ps_div_onehot(uint32_t w)
{
    const uint32_t m = 0x01010101u;
    const uint32_t p0 = w & m, p1 = (w >> 1) & m, p2 = (w >> 2) & m, p3 = (w >> 3) & m;
    uint32_t h = w & 0xF0F0F0F0u;
    h |= h >> 2;
    h |= h >> 1;
    const uint32_t two = (p0 & p1) | (p2 & p3) | ((p0 | p1) & (p2 | p3));
    return (p0 | p1 | p2 | p3) & ~(two | (h >> 4));
}

// state: rows x pitch bytes (pitch a multiple of 128), N live cells per row.  STORE: counts[4 * row + a] = cells of the row
// equal to 1 << a.  SUMMARY: sums[PS_DIV_*] and spectrum[0 .. N] (u64, zeroed by the caller) accumulate the terms of every
// row; lds_bins = N + 1 when the spectrum is kept in an LDS histogram per workgroup (dynamic LDS: lds_bins u32), 0 when the
// bins do not fit and every row adds to the global one.  Any grid of whole waves is valid: waves stride over the rows.
template <bool STORE, bool SUMMARY>
__global__ void __launch_bounds__(1024) core_site_counts_kernel(const uint8_t *state, uint32_t pitch, uint32_t N, uint32_t rows,
                                                                uint32_t *counts, unsigned long long *sums,
                                                                unsigned long long *spectrum, uint32_t lds_bins)
{
    extern __shared__ uint32_t div_hist[];
    __shared__ unsigned long long div_acc[PS_DIV_WORDS];
    const uint32_t lane = threadIdx.x & 63u, wpb = blockDim.x >> 6;
    if (SUMMARY) {
        for (uint32_t b = threadIdx.x; b < lds_bins; b += blockDim.x) div_hist[b] = 0u;
        if (threadIdx.x < (uint32_t)PS_DIV_WORDS) div_acc[threadIdx.x] = 0ull;
        __syncthreads();
    }
    const uint32_t steps = (pitch + 1023u) >> 10;
    const uint32_t nwaves = gridDim.x * wpb;
    const uint32_t lofs = lane * 16u;
    uint64_t s_pair = 0, s_seg = 0, s_other = 0, s_a = 0, s_c = 0, s_g = 0, s_t = 0;
    // (wave-uniform, and said so: the row loop, its addresses and the summary arithmetic go to the scalar unit)
    uint32_t row = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * wpb + (threadIdx.x >> 6)));
    uint4 cur = make_uint4(0u, 0u, 0u, 0u);
    if (row < rows && lofs < pitch) cur = ps_load_row16(state + (size_t)row * pitch + lofs, true);
    while (row < rows) {
        uint32_t n[4] = { 0u, 0u, 0u, 0u };
        uint32_t suspect = 0u;
        for (uint32_t s = 0; s < steps; s++) {
            // the piece behind this one: the row's next 1 KiB, or the first of the wave's next row
            const bool last = s + 1u == steps;
            const uint32_t nrow = last ? row + nwaves : row;
            const uint32_t nofs = (last ? 0u : (s + 1u) << 10) + lofs;
            uint4 nxt = make_uint4(0u, 0u, 0u, 0u);
            if (nrow < rows && nofs < pitch) nxt = ps_load_row16(state + (size_t)nrow * pitch + nofs, true);
            uint32_t x[4] = { cur.x, cur.y, cur.z, cur.w };
            const uint32_t c0 = (s << 10) + lofs;
            if (c0 + 16u > N) {          // (the last pieces of a row only; lanes past the pitch hold zeros)
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) x[q] &= ps_state_cell_mask(c0 + 4u * q, N);
            }
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) {
#pragma unroll
                for (uint32_t a = 0; a < 4; a++) n[a] += (uint32_t)__popc(x[q] & (0x01010101u << a));
                suspect |= ps_div_suspect(x[q]);
            }
            cur = nxt;
        }
        if (__any(suspect != 0u)) {
            // a byte that is not 0 / 1 / 2 / 4 / 8: count the row again, bytes that are 1 / 2 / 4 / 8 only
#pragma unroll
            for (uint32_t a = 0; a < 4; a++) n[a] = 0u;
            for (uint32_t s = 0; s < steps; s++) {
                const uint32_t c0 = (s << 10) + lofs;
                if (c0 >= pitch) continue;
                const uint4 v = ps_load_row16(state + (size_t)row * pitch + c0, false);
                const uint32_t x[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) {
                    const uint32_t w = x[q] & ps_state_cell_mask(c0 + 4u * q, N);
                    const uint32_t ok = ps_div_onehot(w) * 0x0Fu;      // (bits 0-3 of the bytes that count)
#pragma unroll
                    for (uint32_t a = 0; a < 4; a++) n[a] += (uint32_t)__popc(w & ok & (0x01010101u << a));
                }
            }
        }
        // transposing reduction: halves swap two bases, quarters one, then four steps inside the 16-lane groups
        const bool hi = (lane & 32u) != 0u, q1 = (lane & 16u) != 0u;
        uint32_t k0 = (hi ? n[2] : n[0]) + (uint32_t)__shfl_xor((int)(hi ? n[0] : n[2]), 32, 64);
        uint32_t k1 = (hi ? n[3] : n[1]) + (uint32_t)__shfl_xor((int)(hi ? n[1] : n[3]), 32, 64);
        uint32_t k = (q1 ? k1 : k0) + (uint32_t)__shfl_xor((int)(q1 ? k0 : k1), 16, 64);
#pragma unroll
        for (int o = 8; o; o >>= 1) k += (uint32_t)__shfl_xor((int)k, o, 64);
        // (lane 16 a now holds the row's count of base a)
        if (STORE && (lane & 15u) == 0u) counts[(size_t)row * 4u + (lane >> 4)] = k;
        if (SUMMARY) {
            const uint32_t na = (uint32_t)__builtin_amdgcn_readlane((int)k, 0), nc = (uint32_t)__builtin_amdgcn_readlane((int)k, 16);
            const uint32_t ng = (uint32_t)__builtin_amdgcn_readlane((int)k, 32), nt = (uint32_t)__builtin_amdgcn_readlane((int)k, 48);
            uint64_t pair, other, minor;
            uint32_t seg;
            ps_div_site_terms(N, na, nc, ng, nt, &pair, &seg, &other, &minor);
            s_pair += pair;
            s_seg += seg;
            s_other += other;
            s_a += na;
            s_c += nc;
            s_g += ng;
            s_t += nt;
            if (lane == 0u) {
                if (lds_bins) atomicAdd(&div_hist[(uint32_t)minor], 1u);
                else atomicAdd(&spectrum[minor], 1ull);
            }
        }
        row += nwaves;
    }
    if (SUMMARY) {
        if (lane == 0u) {
            atomicAdd(&div_acc[PS_DIV_PAIR], (unsigned long long)s_pair);
            atomicAdd(&div_acc[PS_DIV_SEG], (unsigned long long)s_seg);
            atomicAdd(&div_acc[PS_DIV_OTHER], (unsigned long long)s_other);
            atomicAdd(&div_acc[PS_DIV_BASE + 0], (unsigned long long)s_a);
            atomicAdd(&div_acc[PS_DIV_BASE + 1], (unsigned long long)s_c);
            atomicAdd(&div_acc[PS_DIV_BASE + 2], (unsigned long long)s_g);
            atomicAdd(&div_acc[PS_DIV_BASE + 3], (unsigned long long)s_t);
        }
        __syncthreads();
        // the flush: one atomic per workgroup and word, one per non-empty bin
        if (threadIdx.x < (uint32_t)PS_DIV_WORDS && div_acc[threadIdx.x] != 0ull) atomicAdd(&sums[threadIdx.x], div_acc[threadIdx.x]);
        for (uint32_t b = threadIdx.x; b < lds_bins; b += blockDim.x) {
            const uint32_t v = div_hist[b];
            if (v) atomicAdd(&spectrum[b], (unsigned long long)v);
        }
    }
}
