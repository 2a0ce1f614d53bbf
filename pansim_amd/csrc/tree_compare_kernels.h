// tree_compare_kernels.h -- the kernels of ps_tree_compare (docs/TREE_COMPARISON.md): the rank table over the two leaf orders and
// the comparison of two trees over ALL pairs of leaves.
//
// Each tree arrives as a comb over its OWN dendrogram order (tree_compare.h): gap[r] is the merge that joins positions r and
// r + 1 (PS_GEN_BEYOND between two roots), a parent's index exceeds its children's, so the lowest common ancestor of positions
// p < q is max(gap[p .. q - 1]) -- two reads of the sparse table ancestry_table_kernel builds, as pair_clock_kernel reads a
// divergence time.  The pairs are walked in A's order; pb[p] is the position in B of the leaf at position p of A.  Per merge
// one uint2 { val, lo | hi << 16 }: its value and the half-open position interval of its tie-top (its clade).  Every sum is
// an integer sum: nothing depends on the launch geometry.
#pragma once

#include <stdint.h>

#include "ancestry_kernels.h"

// the summary words of tree_pair_kernel (u64 each), in front of the joint bins
enum {
    PS_TC_BOTH = 0, PS_TC_A_ONLY, PS_TC_B_ONLY, PS_TC_NEITHER,      // the pairs by where they are joined
    PS_TC_SUM_A, PS_TC_SUM_B, PS_TC_SUM_AA, PS_TC_SUM_BB, PS_TC_SUM_AB,    // over the pairs joined in both
    PS_TC_RES_A, PS_TC_RES_B, PS_TC_SHARED,                          // the triplet sums (TRIPLETS only)
    PS_TC_WORDS
};

#define PS_TC_MAX_VAL 262143u           // 2^18 - 1: fewer than 2^27 pairs times a square below 2^36 stay below 2^63
#define PS_TC_RANK_ROWS 256u            // rows of the rank table per workgroup of tree_rank_kernel

struct ps_tc_args {
    uint32_t Ba, Bb;         // value bins of the two trees; row Ba and column Bb hold the pairs not joined
    uint64_t Sa, Sb;         // spans (>= 1)
    float a_scale, b_scale;  // ~ B / S
};

// what one pair adds: to the four counters, the five moments and (TRIPLETS: rab = |C_A & C_B|) the three triplet sums.  ia, ib:
// the info words of the pair's merges (only read where joined).  Shared by the kernel and the host restatement.
struct ps_tc_sums {
    uint32_t n[4];
    uint64_t s[PS_TC_WORDS - 4];
};

__host__ __device__ __forceinline__ void ps_tc_pair(ps_tc_sums &t, bool ja, bool jb, uint2 ia, uint2 ib, uint32_t N, bool triplets,
                                                    uint32_t rab)
{
    // (constant indices: the counters stay in registers)
    t.n[PS_TC_BOTH] += ja && jb ? 1u : 0u;
    t.n[PS_TC_A_ONLY] += ja && !jb ? 1u : 0u;
    t.n[PS_TC_B_ONLY] += !ja && jb ? 1u : 0u;
    t.n[PS_TC_NEITHER] += !ja && !jb ? 1u : 0u;
    const uint32_t ca = (ia.y >> 16) - (ia.y & 0xffffu), cb = (ib.y >> 16) - (ib.y & 0xffffu);
    if (ja && jb) {
        const uint64_t va = ia.x, vb = ib.x;
        t.s[PS_TC_SUM_A - 4] += va;
        t.s[PS_TC_SUM_B - 4] += vb;
        t.s[PS_TC_SUM_AA - 4] += va * va;
        t.s[PS_TC_SUM_BB - 4] += vb * vb;
        t.s[PS_TC_SUM_AB - 4] += va * vb;
        // (the leaves outside both clades: N - |C_A u C_B| >= 0)
        if (triplets) t.s[PS_TC_SHARED - 4] += N + rab - ca - cb;
    }
    if (triplets && ja) t.s[PS_TC_RES_A - 4] += N - ca;
    if (triplets && jb) t.s[PS_TC_RES_B - 4] += N - cb;
}

// The rank table: R[x][y] = #{p < x : pb[p] < y} for 0 <= x, y <= N, u16 at `pitch` entries per row (the largest entry is N <=
// 16384).  One thread per column y and PS_TC_RANK_ROWS rows: it counts the rows in front of its own from pb (wave-uniform
// reads), then writes its rows top down, one 128-byte line per wave and row.  Grid: x over the columns, y over the row groups.
__global__ void __launch_bounds__(256) tree_rank_kernel(const uint32_t *__restrict__ pb, uint32_t N, uint32_t pitch, uint16_t *__restrict__ R)
{
    const uint32_t y = blockIdx.x * 256u + threadIdx.x, x0 = blockIdx.y * PS_TC_RANK_ROWS;
    if (y > N || x0 > N) return;
    uint32_t cnt = 0;
    for (uint32_t p = 0; p < x0; p++) cnt += pb[p] < y ? 1u : 0u;
    const uint32_t x1 = x0 + PS_TC_RANK_ROWS < N + 1u ? x0 + PS_TC_RANK_ROWS : N + 1u;
    for (uint32_t x = x0; x < x1; x++) {
        R[(size_t)x * pitch + y] = (uint16_t)cnt;
        if (x < N) cnt += pb[x] < y ? 1u : 0u;
    }
}

// All pairs p < q of positions in A's order.  Grid, row / chunk ownership and masks as pair_clock_kernel's: x = workgroups of
// four waves striding over the 256-column chunks of a row from the chunk that holds p + 1, four columns per lane, y strides
// over the rows; any grid is valid.  tab_a, tab_b: the levels of the two sparse tables, N u32 each; pb: N entries rounded up to
// whole chunks (the pad is never used as a pair).  Dynamic LDS: (Ba + 1)(Bb + 1) u32 bins.  R (TRIPLETS): the rank table.
template <bool TRIPLETS>
__global__ void __launch_bounds__(256) tree_pair_kernel(const uint32_t *__restrict__ tab_a, const uint32_t *__restrict__ tab_b,
                                                        const uint32_t *__restrict__ pb, const uint2 *__restrict__ info_a,
                                                        const uint2 *__restrict__ info_b, const uint16_t *__restrict__ R, uint32_t pitch,
                                                        uint32_t N, ps_tc_args a, unsigned long long *words, unsigned long long *joint)
{
    extern __shared__ uint32_t tc_bins[];
    __shared__ unsigned long long tc_acc[PS_TC_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t nb = a.Bb + 1u, nbins = (a.Ba + 1u) * nb;
    for (uint32_t b = tid; b < nbins; b += 256u) tc_bins[b] = 0u;
    if (tid < (uint32_t)PS_TC_WORDS) tc_acc[tid] = 0ull;
    __syncthreads();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (tid >> 6)));
    const uint32_t nwaves = gridDim.x * 4u, nchunk = (N + 255u) >> 8;
    ps_tc_sums t = {};
    for (uint32_t p = blockIdx.y; p + 1u < N; p += gridDim.y) {
        const uint32_t bp = pb[p];
        for (uint32_t c = ((p + 1u) >> 8) + wave; c < nchunk; c += nwaves) {
            const uint32_t q0 = (c << 8) + lane * 4u;
            if (q0 >= N || q0 + 3u <= p) continue;
            const uint4 b4 = *(const uint4 *)(pb + q0);
            const uint32_t bq[4] = { b4.x, b4.y, b4.z, b4.w };
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) {
                const uint32_t q = q0 + u;
                if (q <= p || q >= N) continue;
                // the lowest common ancestors: max(gap[p .. q - 1]) in A, max(gap_b[lo .. hi - 1]) in B, two overlapping
                // power-of-two ranges each (k <= log2(N - 1): inside the tables)
                const uint32_t ka = 31u - (uint32_t)__clz((int)(q - p));
                const uint32_t *la = tab_a + (size_t)ka * N;
                const uint32_t ma = max(la[p], la[q - (1u << ka)]);
                const uint32_t lo = min(bp, bq[u]), hi = max(bp, bq[u]);
                const uint32_t kb = 31u - (uint32_t)__clz((int)(hi - lo));
                const uint32_t *lb = tab_b + (size_t)kb * N;
                const uint32_t mb = max(lb[lo], lb[hi - (1u << kb)]);
                const bool ja = ma != 0xffffffffu, jb = mb != 0xffffffffu;
                const uint2 ia = ja ? info_a[ma] : make_uint2(0u, 0u), ib = jb ? info_b[mb] : make_uint2(0u, 0u);
                uint32_t rab = 0u;
                if (TRIPLETS && ja && jb) {
                    // |C_A & C_B|: the leaves with a position in [lo_a, hi_a) of A and in [lo_b, hi_b) of B
                    const uint16_t *r0 = R + (size_t)(ia.y & 0xffffu) * pitch, *r1 = R + (size_t)(ia.y >> 16) * pitch;
                    const uint32_t y0 = ib.y & 0xffffu, y1 = ib.y >> 16;
                    rab = ((uint32_t)r1[y1] + (uint32_t)r0[y0]) - ((uint32_t)r0[y1] + (uint32_t)r1[y0]);
                }
                ps_tc_pair(t, ja, jb, ia, ib, N, TRIPLETS, rab);
                const uint32_t ba = ja ? ps_clock_time_bin(ia.x, a.Ba, a.Sa, a.a_scale) : a.Ba;
                const uint32_t bb = jb ? ps_clock_time_bin(ib.x, a.Bb, a.Sb, a.b_scale) : a.Bb;
                atomicAdd(&tc_bins[ba * nb + bb], 1u);
            }
        }
    }
    // the words per wave, then per workgroup; then one global atomic per non-zero word and non-empty bin
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)PS_TC_WORDS; w++) {
        if (!TRIPLETS && w >= (uint32_t)PS_TC_RES_A) break;
        const unsigned long long v = ps_ph_wave_sum(w < 4u ? (unsigned long long)t.n[w] : (unsigned long long)t.s[w - 4u]);
        if (lane == 0u && v) atomicAdd(&tc_acc[w], v);
    }
    __syncthreads();
    if (tid < (uint32_t)PS_TC_WORDS && tc_acc[tid]) atomicAdd(&words[tid], tc_acc[tid]);
    for (uint32_t b = tid; b < nbins; b += 256u) {
        const uint32_t v = tc_bins[b];
        if (v) atomicAdd(&joint[b], (unsigned long long)v);
    }
}
