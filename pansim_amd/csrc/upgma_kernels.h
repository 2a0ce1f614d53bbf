// upgma_kernels.h -- the kernels of ps_upgma_tree (docs/UPGMA_TREE.md) and the 128-bit integer order on cluster distances they
// share with the host finish and the host restatement (ps_upgma_from_counts).
//
// Everything runs in INTERNAL row order over a full N x N matrix of u64 sums: S[i][j] = the sum of d over all cross pairs of the
// clusters that live in rows i and j (and, under the accessory metric, a second matrix of the sums of b).  A cluster lives in
// the row of its member cluster with the smaller id; id[i] = out_row[i] is the smallest OUTPUT row of the cluster and never
// changes for a row that stays active, since the merged cluster keeps the smaller id.  The store kernels widen a band's counts
// into the matrices (both contractions write the whole rectangle of a band, so the matrices are complete and symmetric once every
// band has passed; nothing is mirrored).  A round: the nearest other cluster of every active row under (distance, lo id, hi id),
// the pairs that chose each other appended to the list and marked, their rows added, their columns added, the absorbed rows
// retired.  Only integers are added and the order on pairs is strict, so nothing depends on the grid or on the order of the atomics.
#pragma once

#include <stdint.h>

#define PS_UP_NONE 0xffffffffu

// -1 / 0 / +1: num1 / den1 below / equal to / above num2 / den2, by num1 den2 against num2 den1 in 128 bits (the sums reach
// 2^58, so a u64 product is not enough; ps_tr_dist_cmp multiplies in u64).  Every den is > 0.  No floating point.
__host__ __device__ __forceinline__ int ps_up_dist_cmp(uint64_t num1, uint64_t den1, uint64_t num2, uint64_t den2)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t xh = __umul64hi(num1, den2), xl = num1 * den2, yh = __umul64hi(num2, den1), yl = num2 * den1;
    if (xh != yh) return xh < yh ? -1 : 1;
    return xl < yl ? -1 : xl > yl ? 1 : 0;
#else
    const unsigned __int128 x = (unsigned __int128)num1 * den2, y = (unsigned __int128)num2 * den1;
    return x < y ? -1 : x > y ? 1 : 0;
#endif
}

// a pair of clusters under the total order (distance, lo id, hi id)
struct ps_up_key {
    uint64_t num, den;
    uint32_t lo, hi;
};

__host__ __device__ __forceinline__ bool ps_up_less(const ps_up_key &a, const ps_up_key &b)
{
    const int c = ps_up_dist_cmp(a.num, a.den, b.num, b.den);
    if (c) return c < 0;
    return a.lo != b.lo ? a.lo < b.lo : a.hi < b.hi;
}

// Store, core metric.  S[i][j] = h(i, j) / 2 for the band's rows i = lo + r < N (C: the band's u32 counts, row pitch ldc; a
// shard sum is halved here, behind the sum) and the columns j < ldm (N rounded up to 64); columns >= N are stored as 0.  Two
// columns per thread: one 8-byte load, one 16-byte store.  Grid: x over the column pairs, y strides over the band's rows (loop
// bound: nrows / gridDim.y); any grid is valid.
__global__ void __launch_bounds__(256) upgma_store_core_kernel(const uint32_t *C, uint64_t ldc, uint32_t N, uint32_t lo, uint32_t nrows,
                                                               uint64_t *S, uint64_t ldm)
{
    const uint32_t j = (blockIdx.x * 256u + threadIdx.x) * 2u;
    if (j >= ldm) return;                                 // (ldm is even and j + 1 < ldm <= ldc: the load stays inside the band's row)
    for (uint32_t r = blockIdx.y; r < nrows; r += gridDim.y) {
        const uint32_t i = lo + r;
        if (i >= N) break;                                // (rows ascend: pad rows from here on)
        const uint2 v = *(const uint2 *)(C + (size_t)r * ldc + j);
        ulonglong2 w;
        w.x = j + 0u < N ? (unsigned long long)(v.x >> 1) : 0ull;
        w.y = j + 1u < N ? (unsigned long long)(v.y >> 1) : 0ull;
        *(ulonglong2 *)(S + (size_t)i * ldm + j) = w;
    }
}

// Store, accessory metric.  From the u16 intersections I of the band's rows (In, row pitch ldi; nullptr: no accessory genes, I = U = 0
// for every pair) and the rows' gene counts: A[i][j] = a = U - I and B[i][j] = b = U + cg with U = cnt[i] + cnt[j] - I.  The
// same grid and the same bounds as the core form (j + 1 < ldm <= ldi).
__global__ void __launch_bounds__(256) upgma_store_acc_kernel(const uint16_t *In, uint32_t ldi, const uint32_t *rowcnt, uint64_t cg, uint32_t N,
                                                              uint32_t lo, uint32_t nrows, uint64_t *A, uint64_t *B, uint64_t ldm)
{
    const uint32_t j = (blockIdx.x * 256u + threadIdx.x) * 2u;
    if (j >= ldm) return;
    const uint32_t c0 = (In && j + 0u < N) ? rowcnt[j] : 0u, c1 = (In && j + 1u < N) ? rowcnt[j + 1u] : 0u;
    for (uint32_t r = blockIdx.y; r < nrows; r += gridDim.y) {
        const uint32_t i = lo + r;
        if (i >= N) break;
        const uint32_t v = In ? *(const uint32_t *)(In + (size_t)r * ldi + j) : 0u, ci = In ? rowcnt[i] : 0u;
        const uint32_t i0 = v & 0xffffu, i1 = v >> 16;
        const uint32_t u0 = ci + c0 - i0, u1 = ci + c1 - i1;
        ulonglong2 a, b;
        a.x = j + 0u < N ? (unsigned long long)(u0 - i0) : 0ull;
        a.y = j + 1u < N ? (unsigned long long)(u1 - i1) : 0ull;
        b.x = j + 0u < N ? (unsigned long long)u0 + cg : 0ull;
        b.y = j + 1u < N ? (unsigned long long)u1 + cg : 0ull;
        *(ulonglong2 *)(A + (size_t)i * ldm + j) = a;
        *(ulonglong2 *)(B + (size_t)i * ldm + j) = b;
    }
}

// size[i] = 1, active[i] = 1; id[i] = out_row[i] is uploaded by the host
__global__ void __launch_bounds__(256) upgma_init_kernel(uint32_t *size, uint32_t *active, uint32_t N)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < N) size[i] = active[i] = 1u;
}

// Row nearest neighbour.  One wave per active row i (the waves stride over the rows: N / waves trips); lane l the columns
// l + 64 q (N / 64 trips), coalesced u64 loads.  The lane minimum under ps_up_less over the active j != i, then six shuffle
// steps to the wave's.  nn[i] = PS_UP_NONE for an inactive row and for the last cluster.  ACC: the distance is S[i][j] / B[i][j];
// else S[i][j] / (size[i] size[j]).
template <bool ACC>
__global__ void __launch_bounds__(256) upgma_row_nn_kernel(const uint64_t *S, const uint64_t *B, uint64_t ldm, uint32_t N, const uint32_t *active,
                                                           const uint32_t *size, const uint32_t *id, uint32_t *nn, uint64_t *nn_num,
                                                           uint64_t *nn_den)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    for (uint32_t i = wave; i < N; i += gridDim.x * 4u) {
        if (!active[i]) {                                 // (the same in every lane)
            if (lane == 0u) nn[i] = PS_UP_NONE;
            continue;
        }
        const uint32_t oi = id[i];
        const uint64_t si = size[i];
        ps_up_key best;
        best.num = 0ull; best.den = 1ull; best.lo = PS_UP_NONE; best.hi = PS_UP_NONE;
        uint32_t best_j = PS_UP_NONE;
        for (uint32_t j = lane; j < N; j += 64u) {        // (j < N <= ldm: every load stays inside row i)
            if (j == i || !active[j]) continue;
            const uint32_t oj = id[j];
            ps_up_key e;
            e.num = S[(size_t)i * ldm + j];
            e.den = ACC ? B[(size_t)i * ldm + j] : si * (uint64_t)size[j];
            e.lo = min(oi, oj);
            e.hi = max(oi, oj);
            if (best_j == PS_UP_NONE || ps_up_less(e, best)) {
                best = e;
                best_j = j;
            }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            ps_up_key e;
            e.num = (uint64_t)__shfl_xor((unsigned long long)best.num, o, 64);
            e.den = (uint64_t)__shfl_xor((unsigned long long)best.den, o, 64);
            e.lo = (uint32_t)__shfl_xor((int)best.lo, o, 64);
            e.hi = (uint32_t)__shfl_xor((int)best.hi, o, 64);
            const uint32_t ej = (uint32_t)__shfl_xor((int)best_j, o, 64);
            if (ej != PS_UP_NONE && (best_j == PS_UP_NONE || ps_up_less(e, best))) {
                best = e;
                best_j = ej;
            }
        }
        if (lane == 0u) {
            nn[i] = best_j;
            nn_num[i] = best.num;
            nn_den[i] = best.den;
        }
    }
}

// one merge as the rounds list it: the two rows (A: the smaller id, the row that stays), their sizes before the merge, the
// distance at which they merge and the round (from 1) that found it
struct ps_up_rec {
    uint64_t num, den;
    uint32_t a, b, size_a, size_b, round, pad;
};

// Mutual.  One thread per row i; no loop.  mate[i] = nn[i] when i and nn[i] chose each other, else PS_UP_NONE (every thread
// writes its own mate[i], so nothing of the last round is left).  The row with the smaller id appends the pair through one
// atomic counter, in any order; a write past N - 1 is masked (a tree has N - 1 merges).
__global__ void __launch_bounds__(256) upgma_mutual_kernel(uint32_t N, const uint32_t *nn, const uint64_t *nn_num, const uint64_t *nn_den,
                                                           const uint32_t *size, const uint32_t *id, uint32_t round, uint32_t *mate,
                                                           uint32_t *count, ps_up_rec *rec)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const uint32_t j = nn[i];                             // (PS_UP_NONE or < N; nn[j] is then read inside the array)
    const bool mutual = j != PS_UP_NONE && nn[j] == i;
    mate[i] = mutual ? j : PS_UP_NONE;
    if (!mutual || id[i] > id[j]) return;
    const uint32_t k = atomicAdd(count, 1u);
    if (k + 1u < N) {
        ps_up_rec r;
        r.num = nn_num[i];
        r.den = nn_den[i];
        r.a = i;
        r.b = j;
        r.size_a = size[i];
        r.size_b = size[j];
        r.round = round;
        r.pad = 0u;
        rec[k] = r;
    }
}

// Merge, the rows.  For every pair (A, B) of this round -- rec[first .. first + n) with first + n <= N - 1 -- row A += row B over
// all ldm columns, coalesced.  A row is in one pair at most and no row B is written, so the pairs do not meet here.  Grid: x
// over the columns, y strides over the pairs (loop bound: n / gridDim.y).  BOTH: the second matrix as well.
template <bool BOTH>
__global__ void __launch_bounds__(256) upgma_merge_rows_kernel(const ps_up_rec *rec, uint32_t first, uint32_t n, uint64_t *S, uint64_t *B,
                                                               uint64_t ldm)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= ldm) return;
    for (uint32_t p = blockIdx.y; p < n; p += gridDim.y) {
        const uint32_t a = rec[first + p].a, b = rec[first + p].b;    // (rows < N, written by upgma_mutual_kernel)
        S[(size_t)a * ldm + c] += S[(size_t)b * ldm + c];
        if (BOTH) B[(size_t)a * ldm + c] += B[(size_t)b * ldm + c];
    }
}

// Merge, the columns (behind the rows).  For every row R that stays -- active and not the absorbed side of a pair of this round --
// and every pair (C, D) of this round: R[C] += R[D].  One wave per row (the waves stride over the rows: N / waves trips), its
// lanes over the pairs (n / 64 trips).  The C and D of a round are all distinct, so the adds of a row do not meet; column D is
// not read again once its row and column are retired.
template <bool BOTH>
__global__ void __launch_bounds__(256) upgma_merge_cols_kernel(const ps_up_rec *rec, uint32_t first, uint32_t n, uint32_t N, const uint32_t *active,
                                                               const uint32_t *mate, const uint32_t *id, uint64_t *S, uint64_t *B, uint64_t ldm)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    for (uint32_t r = wave; r < N; r += gridDim.x * 4u) {
        if (!active[r]) continue;
        const uint32_t m = mate[r];
        if (m != PS_UP_NONE && id[r] > id[m]) continue;   // (the absorbed side: its row is retired)
        for (uint32_t p = lane; p < n; p += 64u) {
            const uint32_t c = rec[first + p].a, d = rec[first + p].b;
            S[(size_t)r * ldm + c] += S[(size_t)r * ldm + d];
            if (BOTH) B[(size_t)r * ldm + c] += B[(size_t)r * ldm + d];
        }
    }
}

// Retire (behind the columns).  One thread per row; no loop.  The row that stays takes the absorbed one's members, the absorbed
// one goes inactive.  size[mate] is read by the staying row only and written by nobody.
__global__ void __launch_bounds__(256) upgma_retire_kernel(uint32_t N, const uint32_t *mate, const uint32_t *id, uint32_t *size, uint32_t *active)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const uint32_t m = mate[i];
    if (m == PS_UP_NONE) return;
    if (id[i] < id[m]) size[i] += size[m];
    else active[i] = 0u;
}
