// ancestry_kernels.h -- the kernels of the recorded genealogy (docs/GENEALOGY.md): the comb of the present population from the
// log of parent draws, the sparse table of range maxima over it, and the binning of ALL pairs by (divergence time, distance).
//
// Everything runs in INTERNAL row order.  A generation's parent map (ps_sim::d_idx[slot], one row of the log) is non-decreasing
// in the internal row (children are stored in ascending parent order), and so is every composition of them: for
// internal rows i < j, tmrca(i, j) = max(coal[i], ..., coal[j - 1]) with coal[r] the coalescence time of rows r and r + 1.
// PS_GEN_BEYOND (UINT32_MAX: no common ancestor inside the record) dominates every maximum as it is.
#pragma once

#include <stdint.h>

#include "pair_hist_kernels.h"

// the summary words of pair_clock_kernel (u64 each), in front of the per-time sums and the joint bins
enum { PS_CK_UNDEF = 0, PS_CK_CLAMP, PS_CK_WORDS };

// the time row of a pair that coalesced t >= 1 generations back: min(Bt - 1, floor((t - 1) Bt / St)); the quotient is below
// Bt <= 4096 wherever it is formed and (t - 1) Bt below 2^44, so ps_ph_div makes the f32 estimate exact
__host__ __device__ __forceinline__ uint32_t ps_clock_time_bin(uint32_t t, uint32_t Bt, uint64_t St, float t_scale)
{
    const uint64_t x = (uint64_t)(t - 1u);
    if (x >= St) return Bt - 1u;
    const uint32_t q = ps_ph_div(x * Bt, St, (float)(t - 1u) * t_scale);
    return q < Bt - 1u ? q : Bt - 1u;
}

// coal[r], r = 0 .. N - 2: one thread per r follows the ancestors of rows r and r + 1 back through the log until they are one
// individual.  log: `capacity` rows of N parents, the most recent generation in row (head + capacity - 1) % capacity.  The two
// chains of a thread are dependent gathers from a read-only log; no thread waits for another.
__global__ void __launch_bounds__(256) ancestry_comb_kernel(const uint32_t *__restrict__ log, uint32_t N, uint32_t capacity, uint32_t head,
                                                            uint32_t depth, uint32_t *__restrict__ coal)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r + 1u >= N) return;
    uint32_t a = r, b = r + 1u, t_coal = 0xffffffffu;
    uint32_t ring = head;                        // (the same for every thread: the ring index stays in a scalar register)
    // at most `depth` steps: depth <= capacity rows of the log have been written since the last reset
    for (uint32_t t = 1; t <= depth; t++) {
        ring = ring ? ring - 1u : capacity - 1u;
        const uint32_t *row = log + (size_t)ring * N;
        // (parents are rows of the generation before: below N; the clamp keeps a damaged log from leading outside it)
        a = row[a < N ? a : N - 1u];
        b = row[b < N ? b : N - 1u];
        if (a == b) {
            t_coal = t;
            break;
        }
    }
    coal[r] = t_coal;
}

// level k >= 1 of the sparse table from level k - 1 (`half` = 2^(k - 1), n = N - 1 entries in level 0):
// T[k][r] = max(coal[r .. r + 2^k - 1]) for r + 2^k <= n; the entries beyond are never read
__global__ void __launch_bounds__(256) ancestry_table_kernel(const uint32_t *__restrict__ prev, uint32_t *__restrict__ next, uint32_t n,
                                                             uint32_t half)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint32_t x = prev[r], y = r + half < n ? prev[r + half] : 0u;
    next[r] = x > y ? x : y;
}

struct ps_clock_args {
    ps_ph_args d;        // the distance axis: Bc = Ba = dist_bins, the histogram's own rules
    uint32_t Bt;         // time bins; row Bt holds the pairs beyond the record
    uint64_t St;         // time span (>= 1)
    float t_scale;       // ~ Bt / St
};

// Input per band as pair_hist_kernel's: the u32 numerators h (pitch ldc) when !ACC, the u16 intersections (pitch ldi) with the
// rows' gene counts when ACC (In == nullptr: no accessory genes, I = U = 0).  Same grid, row / chunk ownership and masks.
// table: the levels of the sparse table, N u32 each.  Dynamic LDS: (Bt + 1) dist_bins u32 bins, then 2 (Bt + 1) u64 sums.
// sums: per time row (sum of num, sum of den; the den sum only when ACC -- the core den is L for every pair).
// A lane keeps the sums of its current time row in registers and adds them to the LDS when the row changes: along a row of the
// matrix the time never decreases, so this happens a few times per row.
template <bool ACC>
__global__ void __launch_bounds__(256) pair_clock_kernel(const uint32_t *C, uint64_t ldc, const uint16_t *In, uint32_t ldi,
                                                         const uint32_t *rowcnt, const uint32_t *__restrict__ table, uint32_t N, uint32_t lo,
                                                         uint32_t nrows, ps_clock_args a, unsigned long long *words,
                                                         unsigned long long *sums, unsigned long long *joint)
{
    extern __shared__ unsigned long long ck_lds[];
    __shared__ unsigned long long ck_acc[PS_CK_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t Bx = a.d.Bc, nt = a.Bt + 1u, nbins = nt * Bx;
    unsigned long long *ck_sums = ck_lds;                        // 2 nt u64 (8-byte aligned in front of the u32 bins)
    uint32_t *ck_bins = (uint32_t *)(ck_lds + 2u * nt);
    for (uint32_t b = tid; b < nbins; b += 256u) ck_bins[b] = 0u;
    for (uint32_t b = tid; b < 2u * nt; b += 256u) ck_sums[b] = 0ull;
    if (tid < (uint32_t)PS_CK_WORDS) ck_acc[tid] = 0ull;
    __syncthreads();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (tid >> 6)));
    const uint32_t nwaves = gridDim.x * 4u, nchunk = (N + 255u) >> 8;
    uint32_t n_undef = 0, n_clamp = 0;
    uint32_t last_t = 0u, cur = 0u;              // the time row of the last pair (t = 0 never occurs: cur is set before it is used)
    uint64_t cur_num = 0, cur_den = 0;
    for (uint32_t r = blockIdx.y; r < nrows; r += gridDim.y) {
        const uint32_t i = lo + r;
        if (i + 1u >= N) break;                 // (rows ascend: nothing right of the diagonal from here on)
        const uint32_t ci = (ACC && In) ? rowcnt[i] : 0u;
        for (uint32_t c = ((i + 1u) >> 8) + wave; c < nchunk; c += nwaves) {
            const uint32_t j0 = (c << 8) + lane * 4u;
            if (j0 >= N || j0 + 3u <= i) continue;
            // (the pitches cover N rounded up to 64 and 128: four columns from a multiple of four below N stay inside the row)
            uint32_t hv[4] = { 0u, 0u, 0u, 0u }, iv[4] = { 0u, 0u, 0u, 0u }, cj[4] = { 0u, 0u, 0u, 0u };
            if (!ACC) {
                const uint4 h4 = *(const uint4 *)(C + (size_t)r * ldc + j0);
                hv[0] = h4.x; hv[1] = h4.y; hv[2] = h4.z; hv[3] = h4.w;
            } else if (In) {
                const uint2 i2 = *(const uint2 *)(In + (size_t)r * ldi + j0);
                const uint4 c4 = *(const uint4 *)(rowcnt + j0);
                iv[0] = i2.x & 0xffffu; iv[1] = i2.x >> 16; iv[2] = i2.y & 0xffffu; iv[3] = i2.y >> 16;
                cj[0] = c4.x; cj[1] = c4.y; cj[2] = c4.z; cj[3] = c4.w;
            }
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) {
                const uint32_t j = j0 + q;
                if (j <= i || j >= N) continue;
                // tmrca = max(coal[i .. j - 1]): two overlapping power-of-two ranges (k <= log2(N - 1): inside the table)
                const uint32_t k = 31u - (uint32_t)__clz((int)(j - i));
                const uint32_t *lev = table + (size_t)k * N;
                const uint32_t t = max(lev[i], lev[j - (1u << k)]);
                uint32_t num, den, bx;
                bool skip = false;
                if (ACC) {
                    const uint32_t un = ci + cj[q] - iv[q];
                    bx = ps_ph_acc_bin(iv[q], un, a.d, &skip);
                    num = un - iv[q];
                    den = un + (uint32_t)a.d.cg;             // (b == 0 is skipped; b < 2^32: the driver has checked core_genes)
                    n_undef += skip ? 1u : 0u;
                } else {
                    bool clamped;
                    num = hv[q] >> 1;
                    den = 0u;
                    bx = ps_ph_core_bin(num, a.d, &clamped);
                    n_clamp += clamped ? 1u : 0u;
                }
                if (skip) continue;
                if (t != last_t) {
                    if (cur_num) atomicAdd(&ck_sums[2u * cur], (unsigned long long)cur_num);
                    if (ACC && cur_den) atomicAdd(&ck_sums[2u * cur + 1u], (unsigned long long)cur_den);
                    cur_num = cur_den = 0;
                    last_t = t;
                    cur = t == 0xffffffffu ? a.Bt : ps_clock_time_bin(t, a.Bt, a.St, a.t_scale);
                }
                cur_num += num;
                cur_den += den;
                atomicAdd(&ck_bins[cur * Bx + bx], 1u);
            }
        }
    }
    if (cur_num) atomicAdd(&ck_sums[2u * cur], (unsigned long long)cur_num);
    if (ACC && cur_den) atomicAdd(&ck_sums[2u * cur + 1u], (unsigned long long)cur_den);
    // the two counters per wave, then per workgroup; then one global atomic per non-empty word, sum and bin
    {
        const unsigned long long u = ps_ph_wave_sum(n_undef), k = ps_ph_wave_sum(n_clamp);
        if (lane == 0u) {
            if (u) atomicAdd(&ck_acc[PS_CK_UNDEF], u);
            if (k) atomicAdd(&ck_acc[PS_CK_CLAMP], k);
        }
    }
    __syncthreads();
    if (tid < (uint32_t)PS_CK_WORDS && ck_acc[tid]) atomicAdd(&words[tid], ck_acc[tid]);
    for (uint32_t b = tid; b < 2u * nt; b += 256u) {
        const unsigned long long v = ck_sums[b];
        if (v) atomicAdd(&sums[b], v);
    }
    for (uint32_t b = tid; b < nbins; b += 256u) {
        const uint32_t v = ck_bins[b];
        if (v) atomicAdd(&joint[b], (unsigned long long)v);
    }
}
