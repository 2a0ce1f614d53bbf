// bootstrap_kernels.h -- the site lists of the bootstrap's replicates on the device (docs/BOOTSTRAP_SUPPORT.md): the draw of a
// replicate's sites or the reading of the caller's, counted per site of one core handle (u32, vector atomics), the exclusive
// scan of the counts in blocks of PS_BOOT_BLOCK sites and the expansion into an ascending list of local sites with repeats,
// through which core_packT_kernel's LIST form (core_kernels.h) packs the replicate's strings.  Included by bootstrap_support.h.
#pragma once

#include "ps_common.h"

#define PS_BOOT_ITEMS 8u                        // consecutive sites per thread
#define PS_BOOT_BLOCK (256u * PS_BOOT_ITEMS)    // sites per workgroup of the block sums and of the expansion
#define PS_BOOT_WAVE_FILL 32u                   // a site drawn more often than this is written by its whole wave

// w[s - off]++ for every draw of replicate `rep` that falls into the handle's sites [off, off + ncols); two draws per block
__global__ void __launch_bounds__(256) boot_draw_kernel(uint32_t k0, uint32_t k1, uint32_t rep, uint32_t draws, uint32_t L, uint32_t off,
                                                        uint32_t ncols, uint32_t *w)
{
    const uint32_t blocks = (draws + 1u) >> 1;
    for (uint32_t m = blockIdx.x * 256u + threadIdx.x; m < blocks; m += gridDim.x * 256u) {
        const ps_u4 r = ps_philox(m, rep, 0u, PS_STREAM_BOOTSTRAP, k0, k1);
        const uint32_t s0 = ps_boot_site(r.x, r.y, L) - off;         // (a site below `off` wraps above ncols)
        if (s0 < ncols) atomicAdd(w + s0, 1u);
        if (2u * m + 1u < draws) {
            const uint32_t s1 = ps_boot_site(r.z, r.w, L) - off;
            if (s1 < ncols) atomicAdd(w + s1, 1u);
        }
    }
}

// the same from one replicate of the caller's lists (every entry below the number of all sites: checked on the host)
__global__ void __launch_bounds__(256) boot_list_kernel(const uint32_t *sites, uint32_t draws, uint32_t off, uint32_t ncols, uint32_t *w)
{
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < draws; k += gridDim.x * 256u) {
        const uint32_t s = sites[k] - off;
        if (s < ncols) atomicAdd(w + s, 1u);
    }
}

// the counts of a thread's PS_BOOT_ITEMS sites (0 past ncols) -> their sum; `first` in 64 bits: the last block of a handle
// with nearly 2^32 sites ends past them
__device__ __forceinline__ uint32_t boot_load_items(const uint32_t *w, uint32_t ncols, uint64_t first, uint32_t (&v)[PS_BOOT_ITEMS])
{
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < PS_BOOT_ITEMS; j++) {
        v[j] = first + j < ncols ? w[first + j] : 0u;
        sum += v[j];
    }
    return sum;
}

// exclusive scan of one value per thread over the 256 threads of a workgroup; tot: 4 words of LDS; *all = the workgroup's sum
__device__ __forceinline__ uint32_t boot_block_exscan(uint32_t v, uint32_t *tot, uint32_t *all)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63u) tot[wv] = inc;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t t = tot[k];
        before += k < wv ? t : 0u;
        sum += t;
    }
    __syncthreads();                                    // (tot may be written again)
    *all = sum;
    return before + inc - v;
}

// bsum[g] = the draws that fell into the sites of block g
__global__ void __launch_bounds__(256) boot_block_sum_kernel(const uint32_t *w, uint32_t ncols, uint32_t *bsum)
{
    __shared__ uint32_t tot[4];
    uint32_t v[PS_BOOT_ITEMS], all;
    const uint32_t sum = boot_load_items(w, ncols, (uint64_t)blockIdx.x * PS_BOOT_BLOCK + threadIdx.x * PS_BOOT_ITEMS, v);
    (void)boot_block_exscan(sum, tot, &all);
    if (threadIdx.x == 0) bsum[blockIdx.x] = all;
}

// bsum <- its exclusive scan, *total = the sum of all: one workgroup, 256 blocks per trip with a carry (the sum stays below 2^31)
__global__ void __launch_bounds__(256) boot_scan_blocks_kernel(uint32_t *bsum, uint32_t nblocks, uint32_t *total)
{
    __shared__ uint32_t tot[4];
    uint32_t carry = 0;
    for (uint32_t g0 = 0; g0 < nblocks; g0 += 256u) {
        const uint32_t g = g0 + threadIdx.x, v = g < nblocks ? bsum[g] : 0u;
        uint32_t all;
        const uint32_t ex = boot_block_exscan(v, tot, &all);
        if (g < nblocks) bsum[g] = carry + ex;
        carry += all;
    }
    if (threadIdx.x == 0) *total = carry;
}

// list[scan[s] .. scan[s] + w[s]) = s for every local site s: the ascending list of the replicate's sites.  A thread writes the
// few repeats of its own sites; a site drawn more than PS_BOOT_WAVE_FILL times is handed to the 64 lanes of its wave.  `cap`:
// the entries the list holds -- nothing is written behind it.
__global__ void __launch_bounds__(256) boot_expand_kernel(const uint32_t *w, uint32_t ncols, const uint32_t *bsum, uint32_t *list, uint32_t cap)
{
    __shared__ uint32_t tot[4];
    uint32_t v[PS_BOOT_ITEMS], all;
    const uint64_t first = (uint64_t)blockIdx.x * PS_BOOT_BLOCK + threadIdx.x * PS_BOOT_ITEMS;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t sum = boot_load_items(w, ncols, first, v);
    uint32_t pos = bsum[blockIdx.x] + boot_block_exscan(sum, tot, &all);
#pragma unroll
    for (uint32_t j = 0; j < PS_BOOT_ITEMS; j++) {
        const uint32_t n = v[j];
        const bool heavy = n > PS_BOOT_WAVE_FILL;
        if (!heavy)
            for (uint32_t r = 0; r < n; r++)
                if (pos + r < cap) list[pos + r] = (uint32_t)(first + j);      // (n > 0: the site exists)
        // (every lane of the wave reaches this line: the ballot and the shuffles are over all 64)
        for (unsigned long long todo = __ballot(heavy); todo; todo &= todo - 1ull) {
            const int src = __ffsll((long long)todo) - 1;
            const uint32_t p0 = __shfl(pos, src, 64), cnt = __shfl(n, src, 64), site = __shfl((uint32_t)(first + j), src, 64);
            for (uint32_t r = lane; r < cnt; r += 64u)
                if (p0 + r < cap) list[p0 + r] = site;
        }
        pos += n;
    }
}
