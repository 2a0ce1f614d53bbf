// state_kernels.h -- gfx950 kernels of the state file (ps_sim_save / ps_sim_load, docs/STATE_FORMAT.md).
//
// The core matrix of a simulated population is one-hot (1 / 2 / 4 / 8 per cell), so the file holds it at 2 bits per cell:
// the site-major rows are contiguous in HBM (pitch is a multiple of 128), hence "16 cells -> one dword" is a flat stream
// over the chunk -- item t reads bytes [16 t, 16 t + 16) and writes dword t.  One 16-byte nontemporal load per lane (as the
// sweeps' ps_load_row16), one dword store: a wave turns 1 KiB of a row into 256 contiguous bytes, 1.25 bytes of traffic per
// cell.  Per 1 KiB the pack pass is planned at ~70 vector instructions (4 x (pack 9 + check 7) + checksum 14 + addressing),
// the unpack pass at ~75 -- half of the ~150 at which the row stream leaves its memory ceiling; the compiled
// kernels hold 207 / 175 vector instructions in all, row-tail path, prologue and the final reduction included.
// No LDS, no scratch, 256 threads, 18 / 22 VGPRs: both may run beside a sweep.
#pragma once

#include "core_kernels.h"

// The section checksum: the sum modulo 2^64 of ps_state_mix(w_j, j) over the section's little-endian u32 words w_j.
// Both halves are bijections of w for a fixed j, so any change of one word -- hence of one byte -- changes the sum; the
// sum does not depend on the order of the words, so the device accumulates it per lane and adds the lanes up with atomics.
__host__ __device__ __forceinline__ uint64_t ps_state_mix(uint32_t w, uint64_t j)
{
    const uint32_t jl = (uint32_t)j, jh = (uint32_t)(j >> 32);
    uint32_t a = w + jl * 0x9E3779B1u + jh * 0x85EBCA77u;
    a ^= a >> 16;
    a *= 0x7FEB352Du;
    a ^= a >> 15;
    a *= 0x846CA68Bu;
    a ^= a >> 16;
    const uint32_t b = w * 0xC2B2AE3Du + jl;
    return ((uint64_t)a << 32) | (uint64_t)b;
}

// four one-hot bytes -> their four 2-bit codes (log2 of the allele) in bits 0..7, cell k in bits 2k
__device__ __forceinline__ uint32_t ps_state_pack4(uint32_t x)
{
    const uint32_t c = (((x >> 1) | (x >> 3)) & 0x01010101u) | (((x >> 1) | (x >> 2)) & 0x02020202u);
    return (c * 0x01041040u) >> 24;      // byte k's two bits to bits 24 + 2k (the partial products do not meet)
}

// the inverse: 8 bits of codes -> four one-hot bytes
__device__ __forceinline__ uint32_t ps_state_unpack4(uint32_t b)
{
    uint32_t s = (b | (b << 12)) & 0x000F000Fu;
    s = (s | (s << 6)) & 0x03030303u;                    // code k in byte k
    const uint32_t r = 0x01010101u + (s & 0x01010101u);  // 1 or 2
    const uint32_t m = ((s >> 1) & 0x01010101u) * 0xFFu; // bytes whose code is 2 or 3
    return (r & ~m) | ((r << 2) & m);
}

// byte mask of the cells of a dword that lie inside [0, N): cells first .. first + 3
__device__ __forceinline__ uint32_t ps_state_cell_mask(uint32_t first, uint32_t N)
{
    if (first + 4u <= N) return 0xFFFFFFFFu;
    if (first >= N) return 0u;
    return (1u << (8u * (N - first))) - 1u;
}

__device__ __forceinline__ void ps_state_reduce(uint64_t acc, uint32_t bad, unsigned long long *sum, uint32_t *flag)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        acc += (uint64_t)__shfl_xor((unsigned long long)acc, o);
        bad |= (uint32_t)__shfl_xor((int)bad, o);
    }
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(sum, (unsigned long long)acc);
        if (bad) atomicOr(flag, 1u);
    }
}

// rows: `items` 16-cell pieces of whole site rows (cpr pieces per row); out: one dword per piece; j0: index of the chunk's
// first dword in the section (checksum).  *flag becomes 1 if a cell inside [0, N) is not 1 / 2 / 4 / 8.  Cells [N, pitch)
// pack as code 0 whatever they hold.
__global__ void __launch_bounds__(256) core_state_pack2_kernel(const uint8_t *rows, uint32_t *out, uint32_t items, uint32_t cpr,
                                                               uint32_t N, uint64_t j0, unsigned long long *sum, uint32_t *flag)
{
    const uint32_t stride = gridDim.x * 256u;
    uint32_t t = blockIdx.x * 256u + threadIdx.x;
    uint32_t c = t % cpr;
    const uint32_t dc = stride % cpr;
    uint64_t acc = 0;
    uint32_t bad = 0;
    for (; t < items; t += stride) {
        const uint4 v = ps_load_row16(rows + (size_t)t * 16u, true);
        uint32_t x[4] = { v.x, v.y, v.z, v.w };
        if (c * 16u + 16u > N) {          // (the last pieces of a row only)
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) {
                const uint32_t m = ps_state_cell_mask(c * 16u + 4u * q, N);
                x[q] = (x[q] & m) | (0x01010101u & ~m);
            }
        }
        uint32_t pk = 0, hi = 0, pc = 0, nz = 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            pk |= ps_state_pack4(x[q]) << (8u * q);
            hi |= x[q] & 0xF0F0F0F0u;
            pc += (uint32_t)__popc(x[q]);
            uint32_t n = x[q] | (x[q] >> 1);
            n |= n >> 2;
            nz &= n;
        }
        bad |= (hi != 0u || pc != 16u || (nz & 0x01010101u) != 0x01010101u) ? 1u : 0u;
        __builtin_nontemporal_store(pk, out + t);
        acc += ps_state_mix(pk, j0 + t);
        c += dc;
        if (c >= cpr) c -= cpr;
    }
    ps_state_reduce(acc, bad, sum, flag);
}

// in: one dword per 16-cell piece; rows: the site rows they expand to.  Cells [N, pitch) are written as zeros whatever
// the file holds; *sum accumulates the checksum of the words as read, for the host to compare.
__global__ void __launch_bounds__(256) core_state_unpack2_kernel(const uint32_t *in, uint8_t *rows, uint32_t items, uint32_t cpr,
                                                                 uint32_t N, uint64_t j0, unsigned long long *sum)
{
    const uint32_t stride = gridDim.x * 256u;
    uint32_t t = blockIdx.x * 256u + threadIdx.x;
    uint32_t c = t % cpr;
    const uint32_t dc = stride % cpr;
    uint64_t acc = 0;
    for (; t < items; t += stride) {
        const uint32_t pk = __builtin_nontemporal_load(in + t);
        uint32_t x[4];
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) x[q] = ps_state_unpack4((pk >> (8u * q)) & 0xFFu);
        if (c * 16u + 16u > N) {
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) x[q] &= ps_state_cell_mask(c * 16u + 4u * q, N);
        }
        ps_store_row16(rows + (size_t)t * 16u, make_uint4(x[0], x[1], x[2], x[3]), true);
        acc += ps_state_mix(pk, j0 + t);
        c += dc;
        if (c >= cpr) c -= cpr;
    }
    ps_state_reduce(acc, 0u, sum, nullptr);
}
