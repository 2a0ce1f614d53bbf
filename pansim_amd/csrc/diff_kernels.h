// diff_kernels.h -- gfx950 kernels of the group differentiation (ps_group_differentiation, include/pansim_hip.h; the
// definitions: docs/GROUP_DIFFERENTIATION.md).
//
// Per-group column counts of the site-major byte matrix are a small GEMM, (sites x individuals) . (individuals x groups), and
// the i8 matrix cores take the left operand straight from the bytes as they lie in memory: a WAVE owns tiles of 16 site rows,
// and per chunk of 64 individuals lane l holds 16 bytes of row l & 15 at byte 64 chunk + 16 (l >> 4) -- the A operand of
// v_mfma_i32_16x16x64_i8.  Plane a of a dword is w & (0x01010101 << a): bytes 0 or 2^a, valid i8 values, so the accumulator of
// plane a holds 2^a x count (at most 8 x 65536) and is shifted once per tile.  The B operand is the membership fragment of the
// chunk, built once per call by group_fragments_kernel in the same (lane, byte) <-> individual map: byte j of lane l is 1 iff
// internal individual 64 chunk + 16 (l >> 4) + j belongs to group l & 15.  Unassigned individuals and the pad cells of a row have
// an all-zero membership: nothing is masked.  Four MFMAs per chunk; a step takes the 128-byte line of each of the 16 rows
// (two chunks), the next step's loads in flight.  The fragments stay in LDS while they fit, else they are read from global
// memory (1 KiB per chunk: L2-resident).  Bytes that are not 1 / 2 / 4 / 8 count in no plane: a step in which any lane sees
// one (ps_div_suspect) is cleaned with ps_div_onehot before its planes are formed.
//
// The result of a tile has the group on lane & 15 and site 4 (lane >> 4) + reg in the registers.  The products over all pairs
// of groups are rotations inside the 16-lane rows: rotation d pairs group g with (g + d) & 15, and d = 0 .. min(K - 1, 8)
// reaches every pair once (d = 8 twice: the lane with the smaller group keeps it).  The per-site terms are ps_diff_site_terms,
// shared with the host's ps_differentiation_from_counts.  Integer adds commute: results do not depend on the launch geometry.
#pragma once

#include "diversity_kernels.h"

// rotations of the epilogue, and the u64 words the core kernel accumulates: differences and fixed / monomorphic sites per
// (rotation, group), then the `other` cells per group
enum { PS_DIFF_ROT = 9, PS_DIFF_W_DIFF = 0, PS_DIFF_W_FIXED = 16 * PS_DIFF_ROT, PS_DIFF_W_OTHER = 32 * PS_DIFF_ROT,
       PS_DIFF_WORDS = 32 * PS_DIFF_ROT + 16 };

typedef int ps_i32x4 __attribute__((ext_vector_type(4)));

// One site, the groups g and h by their counts of the five classes A, C, G, T, other (docs/GROUP_DIFFERENTIATION.md): the
// (pair, site) differences n_g n_h - sum_c c_g c_h -- within one group (n^2 - sum c^2) / 2, the difference being twice a sum of
// products -- and whether the two share no class (one group: whether it is monomorphic).  n <= 65536: nothing overflows.
PS_HD void ps_diff_site_terms(uint64_t ng, uint64_t nh, const uint32_t *cg, const uint32_t *ch, bool same, uint64_t *diff,
                              uint32_t *fixed)
{
    uint64_t dot = 0;
#pragma unroll
    for (int c = 0; c < 5; c++) dot += (uint64_t)cg[c] * (uint64_t)ch[c];
    if (same) {
        *diff = (ng * ng - dot) >> 1;
        *fixed = dot == ng * ng ? 1u : 0u;
    } else {
        *diff = ng * nh - dot;
        *fixed = dot == 0 ? 1u : 0u;
    }
}

// the pair of groups that rotation d gives lane-group g is kept there: both below K, and of the two lanes that meet at d = 8
// the one with the smaller group
PS_HD bool ps_diff_keeps(uint32_t g, uint32_t d, uint32_t K)
{
    const uint32_t h = (g + d) & 15u;
    return g < K && h < K && (d != 8u || g < h);
}

// group_int[i] = the group of INTERNAL row i (any value above 15: none) -> frag[64 chunk + l], the B fragment of lane l
__global__ void __launch_bounds__(256) group_fragments_kernel(const uint32_t *group_int, uint32_t N, uint32_t nchunks, uint4 *frag)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks * 64u) return;
    const uint32_t lane = t & 63u, base = (t >> 6) * 64u + 16u * (lane >> 4), g = lane & 15u;
    uint32_t w[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++)
        if (base + j < N && group_int[base + j] == g) w[j >> 2] |= 1u << (8u * (j & 3u));
    frag[t] = make_uint4(w[0], w[1], w[2], w[3]);
}

// the same membership as [K][W] bit rows over the internal rows (the gene-major view's words)
__global__ void __launch_bounds__(256) group_masks_kernel(const uint32_t *group_int, uint32_t N, uint32_t W, uint32_t K,
                                                          unsigned long long *masks)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= K * W) return;
    const uint32_t g = t / W, w = t % W;
    unsigned long long m = 0ull;
    for (uint32_t b = 0; b < 64u; b++) {
        const uint32_t i = w * 64u + b;
        if (i < N && group_int[i] == g) m |= 1ull << b;
    }
    masks[t] = m;
}

// state: rows x pitch bytes (pitch a multiple of 128).  frag: pitch / 64 fragments of 64 uint4; lds_chunks = pitch / 64 when they
// are kept in LDS (dynamic: 1 KiB per chunk), 0 when they are read where they are.  group_size: 16 values, 0 from K on; Na their
// sum.  words[PS_DIFF_WORDS] (zeroed by the caller) accumulate.  SITES: site_within / site_total[rows].  STORE: counts[(row K + g)
// 4 + a].  Any grid of whole waves is valid: waves stride over the tiles.  Rows past the last load zeros and store nothing.
template <bool STORE, bool SITES>
__global__ void __launch_bounds__(1024) core_group_counts_kernel(const uint8_t *state, uint32_t pitch, uint32_t rows, uint32_t K,
                                                                 const uint4 *frag, uint32_t lds_chunks, const uint32_t *group_size,
                                                                 uint32_t Na, unsigned long long *words, uint32_t *site_within,
                                                                 uint32_t *site_total, uint32_t *counts)
{
    extern __shared__ uint4 diff_frag[];
    __shared__ unsigned long long diff_acc[PS_DIFF_WORDS];
    const uint32_t lane = threadIdx.x & 63u, wpb = blockDim.x >> 6;
    for (uint32_t i = threadIdx.x; i < lds_chunks * 64u; i += blockDim.x) diff_frag[i] = frag[i];
    for (uint32_t i = threadIdx.x; i < (uint32_t)PS_DIFF_WORDS; i += blockDim.x) diff_acc[i] = 0ull;
    __syncthreads();
    const uint32_t g = lane & 15u, q = lane >> 4;
    const uint32_t ng = group_size[g];
    const uint32_t nrot = (K - 1u < 8u ? K - 1u : 8u) + 1u;
    const uint32_t steps = pitch >> 7, ntiles = (rows + 15u) >> 4, nwaves = gridDim.x * wpb;
    const bool in_lds = lds_chunks != 0u;
    uint64_t diff[PS_DIFF_ROT];
    uint32_t fix[PS_DIFF_ROT], nh[PS_DIFF_ROT];
    uint64_t oth = 0;
#pragma unroll
    for (uint32_t d = 0; d < (uint32_t)PS_DIFF_ROT; d++) {
        diff[d] = 0;
        fix[d] = 0u;
        nh[d] = (uint32_t)__shfl((int)ng, (int)((lane & 48u) | ((lane + d) & 15u)), 64);
    }
    // (wave-uniform, and said so: the tile loop and its addresses go to the scalar unit)
    uint32_t tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * wpb + (threadIdx.x >> 6)));
    // the two pieces of a lane in step s of a tile: row g of the tile, bytes 128 s + 16 q and 64 further
    auto load2 = [&](uint32_t t, uint32_t s, uint4 &lo, uint4 &hi) {
        lo = hi = make_uint4(0u, 0u, 0u, 0u);
        const uint32_t row = t * 16u + g;
        if (t < ntiles && row < rows) {
            const uint8_t *p = state + (size_t)row * pitch + (s << 7) + 16u * q;
            lo = ps_load_row16(p, true);
            hi = ps_load_row16(p + 64, true);
        }
    };
    uint4 cur0, cur1;
    load2(tile, 0u, cur0, cur1);
    while (tile < ntiles) {
        ps_i32x4 acc[4];
#pragma unroll
        for (int a = 0; a < 4; a++) acc[a] = ps_i32x4{ 0, 0, 0, 0 };
        for (uint32_t s = 0; s < steps; s++) {
            // the step behind this one: the rows' next line, or the first of the wave's next tile
            const bool last = s + 1u == steps;
            uint4 nxt0, nxt1;
            load2(last ? tile + nwaves : tile, last ? 0u : s + 1u, nxt0, nxt1);
            uint32_t x[8] = { cur0.x, cur0.y, cur0.z, cur0.w, cur1.x, cur1.y, cur1.z, cur1.w };
            uint32_t suspect = 0u;
#pragma unroll
            for (int i = 0; i < 8; i++) suspect |= ps_div_suspect(x[i]);
            if (__any(suspect != 0u)) {
                // a byte that is not 0 / 1 / 2 / 4 / 8: keep the bytes that are 1 / 2 / 4 / 8 only
#pragma unroll
                for (int i = 0; i < 8; i++) x[i] &= ps_div_onehot(x[i]) * 0x0Fu;
            }
#pragma unroll
            for (uint32_t c = 0; c < 2u; c++) {
                const uint32_t fi = (2u * s + c) * 64u + lane;
                const uint4 bv = in_lds ? diff_frag[fi] : frag[fi];
                const ps_i32x4 b = { (int)bv.x, (int)bv.y, (int)bv.z, (int)bv.w };
#pragma unroll
                for (uint32_t a = 0; a < 4u; a++) {
                    const uint32_t m = 0x01010101u << a;
                    const ps_i32x4 av = { (int)(x[4u * c] & m), (int)(x[4u * c + 1u] & m), (int)(x[4u * c + 2u] & m),
                                          (int)(x[4u * c + 3u] & m) };
                    acc[a] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, b, acc[a], 0, 0, 0);
                }
            }
            cur0 = nxt0;
            cur1 = nxt1;
        }
        // the tile's counts: group g of site 4 q + r in register r of plane a, times 2^a
#pragma unroll
        for (uint32_t r = 0; r < 4u; r++) {
            const uint32_t site = tile * 16u + 4u * q + r;
            const bool valid = site < rows;
            uint32_t c[5];
#pragma unroll
            for (uint32_t a = 0; a < 4u; a++) c[a] = (uint32_t)acc[a][r] >> a;
            c[4] = valid ? ng - (c[0] + c[1] + c[2] + c[3]) : 0u;
            if (STORE && valid && g < K) ((uint4 *)counts)[(size_t)site * K + g] = make_uint4(c[0], c[1], c[2], c[3]);
            oth += c[4];
#pragma unroll
            for (uint32_t d = 0; d < (uint32_t)PS_DIFF_ROT; d++) {
                if (d < nrot) {
                    uint32_t h[5];
                    const int src = (int)((lane & 48u) | ((lane + d) & 15u));
#pragma unroll
                    for (int k = 0; k < 5; k++) h[k] = d == 0u ? c[k] : (uint32_t)__shfl((int)c[k], src, 64);
                    uint64_t df;
                    uint32_t fx;
                    ps_diff_site_terms(ng, nh[d], c, h, d == 0u, &df, &fx);
                    if (valid) {
                        diff[d] += df;
                        fix[d] += fx;
                    }
                    if (SITES && d == 0u) {
                        // the two per-site words: a 16-lane row reduction of the within terms and of the pooled counts
                        uint32_t w = (uint32_t)df, tot[5] = { c[0], c[1], c[2], c[3], c[4] };
#pragma unroll
                        for (int o = 8; o; o >>= 1) {
                            w += (uint32_t)__shfl_xor((int)w, o, 64);
#pragma unroll
                            for (int k = 0; k < 5; k++) tot[k] += (uint32_t)__shfl_xor((int)tot[k], o, 64);
                        }
                        uint64_t tt;
                        uint32_t tf;
                        ps_diff_site_terms(Na, Na, tot, tot, true, &tt, &tf);
                        if (valid && g == 0u) {
                            site_within[site] = w;
                            site_total[site] = (uint32_t)tt;
                        }
                    }
                }
            }
        }
        tile += nwaves;
    }
    // the wave's sums: the four quarters of a lane column hold the same group; then one LDS atomic per word and wave
#pragma unroll
    for (uint32_t d = 0; d < (uint32_t)PS_DIFF_ROT; d++) {
        if (d < nrot) {
            unsigned long long v = diff[d], f = fix[d];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            f += __shfl_xor(f, 16, 64);
            f += __shfl_xor(f, 32, 64);
            if (q == 0u && ps_diff_keeps(g, d, K)) {
                atomicAdd(&diff_acc[PS_DIFF_W_DIFF + d * 16u + g], v);
                atomicAdd(&diff_acc[PS_DIFF_W_FIXED + d * 16u + g], f);
            }
        }
    }
    {
        unsigned long long v = oth;
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (q == 0u && g < K) atomicAdd(&diff_acc[PS_DIFF_W_OTHER + g], v);
    }
    __syncthreads();
    // the flush: one atomic per workgroup and non-zero word
    for (uint32_t i = threadIdx.x; i < (uint32_t)PS_DIFF_WORDS; i += blockDim.x)
        if (diff_acc[i] != 0ull) atomicAdd(&words[i], diff_acc[i]);
}

// accG: the gene-major view, G rows of W words over the internal rows; masks: [K][W] (group_masks_kernel).  One wave per gene,
// lanes over the words: gene_counts[gene K + g] = the members of g that carry the gene.  Any grid of whole waves is valid.
__global__ void __launch_bounds__(256) acc_group_gene_counts_kernel(const uint64_t *accG, const unsigned long long *masks, acc_dims d,
                                                                    uint32_t K, uint32_t *gene_counts)
{
    const uint32_t lane = threadIdx.x & 63u, nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t gene = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; gene < d.G; gene += nwaves) {
        uint32_t n[16];
#pragma unroll
        for (uint32_t g = 0; g < 16u; g++) n[g] = 0u;
        for (uint32_t w = lane; w < d.W; w += 64u) {
            const unsigned long long word = accG[(uint64_t)gene * d.W + w];
#pragma unroll
            for (uint32_t g = 0; g < 16u; g++)
                if (g < K) n[g] += (uint32_t)__popcll(word & masks[(uint64_t)g * d.W + w]);
        }
#pragma unroll
        for (uint32_t g = 0; g < 16u; g++) {
            if (g < K) {
                uint32_t v = n[g];
#pragma unroll
                for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
                if (lane == 0u) gene_counts[(uint64_t)gene * K + g] = v;
            }
        }
    }
}
