// nj_kernels.h -- the kernels of ps_neighbour_joining (docs/NEIGHBOUR_JOINING.md).  Their arithmetic is nj_rule.h, line for line.
//
// Everything runs in INTERNAL row order over a full N x N matrix of f64 distances (row pitch ldm, N rounded up to 64): D[i][j] =
// the distance of the nodes that live in rows i and j.  A node lives in the row of its leaf with the smallest OUTPUT row, and that
// output row is its id: id[i] = out_row[i] while row i is active, PS_NJ_NONE once it has retired (the joined node keeps the
// smaller id, so the id of a row that stays never changes).  The store kernels widen a band's counts into the matrix (both
// contractions write the whole rectangle of a band, so the matrix is complete and symmetric bit for bit once every band has
// passed; nothing is mirrored).  A join: the smallest pair of every active row under (q, lo id, hi id), then ONE workgroup that
// reduces the rows' candidates to the pair, writes the record and updates row lo, column lo and the row sums.  The order on pairs
// is strict and every update touches its own element only, so nothing depends on the grid or on the order in which waves run.
// No kernel waits for another workgroup.
#pragma once

#include <stdint.h>

#include "nj_rule.h"

// Store, core metric.  D[i][j] = (double)(h(i, j) >> 1) for the band's rows i = lo + r < N (C: the band's u32 counts, row pitch
// ldc) and the columns j < ldm; columns >= N are stored as 0.  Two columns per thread: one 8-byte load, one 16-byte store.  Grid:
// x over the column pairs, y strides over the band's rows (loop bound: nrows / gridDim.y); any grid is valid.
__global__ void __launch_bounds__(256) nj_store_core_kernel(const uint32_t *C, uint64_t ldc, uint32_t N, uint32_t lo, uint32_t nrows, double *D,
                                                            uint64_t ldm)
{
    const uint32_t j = (blockIdx.x * 256u + threadIdx.x) * 2u;
    if (j >= ldm) return;                                 // (ldm is even and j + 1 < ldm <= ldc: the load stays inside the band's row)
    for (uint32_t r = blockIdx.y; r < nrows; r += gridDim.y) {
        const uint32_t i = lo + r;
        if (i >= N) break;                                // (rows ascend: pad rows from here on)
        const uint2 v = *(const uint2 *)(C + (size_t)r * ldc + j);
        double2 w;
        w.x = j + 0u < N ? ps_nj_core_distance(v.x) : 0.0;
        w.y = j + 1u < N ? ps_nj_core_distance(v.y) : 0.0;
        *(double2 *)(D + (size_t)i * ldm + j) = w;
    }
}

// Store, accessory metric.  From the u16 intersections I of the band's rows (In, row pitch ldi; nullptr: no accessory genes, I = U
// = 0 for every pair) and the rows' gene counts: D[i][j] = (U - I) / (U + cg) with U = cnt[i] + cnt[j] - I and cg >= 1.  The same
// grid and the same bounds as the core form (j + 1 < ldm <= ldi).
__global__ void __launch_bounds__(256) nj_store_acc_kernel(const uint16_t *In, uint32_t ldi, const uint32_t *rowcnt, uint64_t cg, uint32_t N,
                                                           uint32_t lo, uint32_t nrows, double *D, uint64_t ldm)
{
    const uint32_t j = (blockIdx.x * 256u + threadIdx.x) * 2u;
    if (j >= ldm) return;
    const uint32_t c0 = (In && j + 0u < N) ? rowcnt[j] : 0u, c1 = (In && j + 1u < N) ? rowcnt[j + 1u] : 0u;
    for (uint32_t r = blockIdx.y; r < nrows; r += gridDim.y) {
        const uint32_t i = lo + r;
        if (i >= N) break;
        const uint32_t v = In ? *(const uint32_t *)(In + (size_t)r * ldi + j) : 0u, ci = In ? rowcnt[i] : 0u;
        const uint32_t i0 = v & 0xffffu, i1 = v >> 16;
        double2 w;
        w.x = j + 0u < N ? ps_nj_acc_distance(i0, ci + c0 - i0, cg) : 0.0;
        w.y = j + 1u < N ? ps_nj_acc_distance(i1, ci + c1 - i1, cg) : 0.0;
        *(double2 *)(D + (size_t)i * ldm + j) = w;
    }
}

// Initial row sums.  One thread per internal row i: r[i] = the sum of d(i, k) over the other rows, accumulated from +0.0 in
// ascending OUTPUT row k (order[k] = the internal row of output row k; N trips).  The matrix is symmetric, so the thread reads
// D[order[k]][i]: neighbouring threads read neighbouring columns of one row.
__global__ void __launch_bounds__(256) nj_row_sum_kernel(const double *D, uint64_t ldm, uint32_t N, const uint32_t *order, double *r)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    double s = 0.0;
    for (uint32_t k = 0; k < N; k++) {                    // (N trips; order[k] < N, checked by the host before the upload)
        const uint32_t row = order[k];
        if (row != i) s += D[(size_t)row * ldm + i];
    }
    r[i] = s;
}

#define PS_NJ_CHUNKS 8u

// The smallest pair of every row among n active nodes.  One wave per active row i (the waves stride over the rows: N / waves
// trips); every pair is looked at once, from the row with the smaller internal index: lane l takes the columns l + 64 c above i,
// coalesced f64 loads; a retired column is skipped before the load.  q in the fixed orientation (lo = the smaller id), the lane
// minimum under ps_nj_less, then six shuffle steps to the wave's.  cand_j[i] = the column of row i's smallest pair, PS_NJ_NONE
// for a retired row and for a row without an active column above it; cand_q[i] its q.
__global__ void __launch_bounds__(256) nj_row_min_kernel(const double *D, uint64_t ldm, uint32_t N, uint32_t n, const uint32_t *id, const double *r,
                                                         uint32_t *cand_j, double *cand_q)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    for (uint32_t i = wave; i < N; i += gridDim.x * 4u) {
        const uint32_t oi = id[i];                        // (the same in every lane)
        if (oi == PS_NJ_NONE) {
            if (lane == 0u) cand_j[i] = PS_NJ_NONE;
            continue;
        }
        const double ri = r[i];
        ps_nj_key best;
        best.q = 0.0; best.lo = PS_NJ_NONE; best.hi = PS_NJ_NONE;
        uint32_t best_j = PS_NJ_NONE;
        // (eight chunks of 64 columns per trip, their loads issued together: a row is one chain of dependent loads otherwise)
        for (uint32_t j0 = ((i + 1u) & ~63u) + lane; j0 < N; j0 += 64u * PS_NJ_CHUNKS) {      // (N / 512 trips)
            uint32_t oj[PS_NJ_CHUNKS];
            double d[PS_NJ_CHUNKS], rj[PS_NJ_CHUNKS];
#pragma unroll
            for (uint32_t c = 0; c < PS_NJ_CHUNKS; c++) {
                const uint32_t j = j0 + 64u * c;
                oj[c] = (j > i && j < N) ? id[j] : PS_NJ_NONE;      // (j <= i: the first chunk alone)
            }
#pragma unroll
            for (uint32_t c = 0; c < PS_NJ_CHUNKS; c++) {
                const uint32_t j = j0 + 64u * c;
                const bool live = oj[c] != PS_NJ_NONE;              // (then j < N <= ldm: the load stays inside row i)
                d[c] = live ? D[(size_t)i * ldm + j] : 0.0;
                rj[c] = live ? r[j] : 0.0;
            }
#pragma unroll
            for (uint32_t c = 0; c < PS_NJ_CHUNKS; c++) {
                if (oj[c] == PS_NJ_NONE) continue;
                ps_nj_key e;
                e.lo = min(oi, oj[c]);
                e.hi = max(oi, oj[c]);
                e.q = oi < oj[c] ? ps_nj_q(n, d[c], ri, rj[c]) : ps_nj_q(n, d[c], rj[c], ri);
                if (best_j == PS_NJ_NONE || ps_nj_less(e, best)) {
                    best = e;
                    best_j = j0 + 64u * c;
                }
            }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            ps_nj_key e;
            e.q = __shfl_xor(best.q, o, 64);
            e.lo = (uint32_t)__shfl_xor((int)best.lo, o, 64);
            e.hi = (uint32_t)__shfl_xor((int)best.hi, o, 64);
            const uint32_t ej = (uint32_t)__shfl_xor((int)best_j, o, 64);
            if (ej != PS_NJ_NONE && (best_j == PS_NJ_NONE || ps_nj_less(e, best))) {
                best = e;
                best_j = ej;
            }
        }
        if (lane == 0u) {
            cand_j[i] = best_j;
            cand_q[i] = best.q;
        }
    }
}

// one join as the device lists it: the two internal rows (lo: the smaller id, the row that stays) and the two lengths
struct ps_nj_rec {
    double b_lo, b_hi;
    uint32_t lo, hi;
};

#define PS_NJ_JOIN_THREADS 1024u

// a candidate pair of the join kernel's reduction: the key and the two internal rows (row_lo holds the smaller id)
struct nj_cand {
    ps_nj_key key;
    uint32_t row_lo, row_hi;
};

__device__ __forceinline__ void nj_cand_take(nj_cand &best, const nj_cand &e)
{
    if (e.row_lo != PS_NJ_NONE && (best.row_lo == PS_NJ_NONE || ps_nj_less(e.key, best.key))) best = e;
}

// The join (behind nj_row_min_kernel of the same n), ONE workgroup of 1024 threads; t = the join's number, n = N - t.  The
// rows' candidates are reduced to the pair (N / 1024 trips, six shuffle steps, sixteen waves through the LDS); thread 0 writes
// the record (masked past N - 1 records).  Then thread k of every active k other than lo and hi (N / 1024 trips): duk, r[k],
// D[lo][k] and D[k][lo] -- its own elements only.  r[lo], r[hi] and d(lo, hi) are read by every thread before the barrier behind
// which thread 0 writes r[lo] and retires hi; d(lo, hi) itself is written by nobody.  Without a candidate (a state the host
// reports from the record) nothing but the record is written.
__global__ void __launch_bounds__(PS_NJ_JOIN_THREADS) nj_join_kernel(double *D, uint64_t ldm, uint32_t N, uint32_t n, uint32_t t, uint32_t *id,
                                                                     double *r, const uint32_t *cand_j, const double *cand_q, ps_nj_rec *rec)
{
    __shared__ nj_cand part[PS_NJ_JOIN_THREADS / 64u];
    nj_cand best;
    best.key.q = 0.0; best.key.lo = PS_NJ_NONE; best.key.hi = PS_NJ_NONE;
    best.row_lo = PS_NJ_NONE; best.row_hi = PS_NJ_NONE;
    for (uint32_t i = threadIdx.x; i < N; i += PS_NJ_JOIN_THREADS) {      // (i < N: the arrays are N long)
        const uint32_t j = cand_j[i], oi = id[i];
        if (j >= N || oi == PS_NJ_NONE) continue;         // (a retired row carries PS_NJ_NONE)
        const uint32_t oj = id[j];
        if (oj == PS_NJ_NONE) continue;
        nj_cand e;
        e.key.q = cand_q[i];
        e.key.lo = min(oi, oj);
        e.key.hi = max(oi, oj);
        e.row_lo = oi < oj ? i : j;
        e.row_hi = oi < oj ? j : i;
        nj_cand_take(best, e);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        nj_cand e;
        e.key.q = __shfl_xor(best.key.q, o, 64);
        e.key.lo = (uint32_t)__shfl_xor((int)best.key.lo, o, 64);
        e.key.hi = (uint32_t)__shfl_xor((int)best.key.hi, o, 64);
        e.row_lo = (uint32_t)__shfl_xor((int)best.row_lo, o, 64);
        e.row_hi = (uint32_t)__shfl_xor((int)best.row_hi, o, 64);
        nj_cand_take(best, e);
    }
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = best;
    __syncthreads();
    best = part[0];
#pragma unroll
    for (uint32_t w = 1; w < PS_NJ_JOIN_THREADS / 64u; w++) nj_cand_take(best, part[w]);      // (every thread: the same winner)
    const uint32_t lo = best.row_lo, hi = best.row_hi;
    if (lo == PS_NJ_NONE) {
        if (threadIdx.x == 0u && t + 1u < N) {
            ps_nj_rec none;
            none.b_lo = 0.0; none.b_hi = 0.0; none.lo = PS_NJ_NONE; none.hi = PS_NJ_NONE;
            rec[t] = none;
        }
        return;                                           // (the same in every thread: no barrier is left behind)
    }
    // lo, hi < N and lo != hi: cand_j[i] is a column j < N other than i
    const double r_lo = r[lo], r_hi = r[hi], dlh = D[(size_t)lo * ldm + hi];
    __syncthreads();
    if (threadIdx.x == 0u) {
        if (t + 1u < N) {
            ps_nj_rec out;
            ps_nj_branches(n, dlh, r_lo, r_hi, &out.b_lo, &out.b_hi);
            out.lo = lo;
            out.hi = hi;
            rec[t] = out;
        }
        r[lo] = ps_nj_r_joined(n, r_lo, r_hi, dlh);
        id[hi] = PS_NJ_NONE;
    }
    for (uint32_t k = threadIdx.x; k < N; k += PS_NJ_JOIN_THREADS) {      // (k < N <= ldm)
        if (k == lo || k == hi || id[k] == PS_NJ_NONE) continue;          // (id[hi] is skipped by k == hi, whichever value it holds by now)
        const double dlk = D[(size_t)lo * ldm + k], dhk = D[(size_t)hi * ldm + k];
        const double duk = ps_nj_duk(dlk, dhk, dlh);
        r[k] = ps_nj_r_other(r[k], dlk, dhk, duk);
        D[(size_t)lo * ldm + k] = duk;
        D[(size_t)k * ldm + lo] = duk;
    }
}
