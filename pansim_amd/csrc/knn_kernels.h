// knn_kernels.h -- the selection kernel of ps_nearest_neighbours (docs/NEAREST_NEIGHBOURS.md).
//
// knn_select_kernel consumes the per-band input of pair_hist_kernel and tree_row_min_kernel -- the u32 Hamming numerators
// h(i, j) of rows [lo, lo + nrows) against all N columns, or the u16 accessory intersections of the same rows with the rows'
// gene counts -- and lists, for every row of the band, its k nearest other rows under the strict order (distance, OUTPUT row of
// the neighbour); the distances compare as in the tree (ps_tr_dist_cmp, linkage_kernels.h).  Both contractions write the whole
// rectangle of a band, so a band's scratch holds complete rows and no N x N matrix is kept: the lists take O(N k).
//
// One wave owns one row and makes k passes over it.  Pass r takes the wave's minimum over the columns j != i whose key is
// strictly above the key taken in pass r - 1; that one key is all a wave carries from pass to pass.  The order is strict, so
// the passes list the k smallest keys in ascending order whatever the grid; no atomics, no waiting.
#pragma once

#include <stdint.h>

#include "linkage_kernels.h"

// (num1, den1, row1) below (num2, den2, row2) under (distance, row)
__host__ __device__ __forceinline__ bool ps_knn_less(uint64_t num1, uint64_t den1, uint32_t row1, uint64_t num2, uint64_t den2, uint32_t row2)
{
    const int c = ps_tr_dist_cmp(num1, den1, num2, den2);
    return c ? c < 0 : row1 < row2;
}

// Grid: workgroups of four waves, the waves stride over the band's rows (loop bound: nrows / waves); any grid is valid.  Lane l
// reads the columns l + 64 q, coalesced; every lane of a wave makes the same (N + 63) / 64 trips with its own column masked, so
// the shuffles behind the loop see all 64 lanes.  C: h with pitch ldc (core metric); In / rowcnt: the intersections with pitch
// ldi and the rows' gene counts (accessory metric; In == nullptr: no accessory genes, I = U = 0 for every pair).  Row i = lo + r
// writes nbr_j, nbr_num (and nbr_den when ACC) [i k, i k + k): the neighbour's INTERNAL row, num = d = h / 2 or a = U - I,
// den = b = U + cg (d < 2^31, a <= 65535, b < 2^32: u32 each).  1 <= k <= N - 1: every pass finds a column.
template <bool ACC>
__global__ void __launch_bounds__(256) knn_select_kernel(const uint32_t *C, uint64_t ldc, const uint16_t *In, uint32_t ldi,
                                                         const uint32_t *rowcnt, uint64_t cg, uint32_t N, uint32_t lo, uint32_t nrows,
                                                         uint32_t k, const uint32_t *out_row, uint32_t *nbr_j, uint32_t *nbr_num,
                                                         uint32_t *nbr_den)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t trips = (uint32_t)__builtin_amdgcn_readfirstlane((int)((N + 63u) >> 6));
    for (uint32_t r = wave; r < nrows; r += gridDim.x * 4u) {
        const uint32_t i = lo + r;
        if (i >= N) break;                                // (rows ascend: pad rows from here on)
        const size_t out = (size_t)i * k;
        if (!ACC) {
            // key = d << 32 | output row: d < 2^31, so ~0 is no key; the keys of a row are distinct
            const uint32_t *row = C + (size_t)r * ldc;
            uint64_t prev = 0ull;
            for (uint32_t p = 0; p < k; p++) {            // (k passes)
                uint64_t best = ~0ull;
                uint32_t best_j = PS_TR_NONE;
#pragma unroll 4
                for (uint32_t q = 0; q < trips; q++) {    // (N / 64 trips; j < N <= ldc: every load stays inside the band's row)
                    const uint32_t j = lane + (q << 6);
                    if (j >= N || j == i) continue;
                    const uint64_t key = ((uint64_t)(row[j] >> 1) << 32) | out_row[j];
                    if ((p == 0u || key > prev) && key < best) {
                        best = key;
                        best_j = j;
                    }
                }
                uint64_t m = best;
#pragma unroll
                for (int o = 32; o; o >>= 1) {
                    const uint64_t other = (uint64_t)__shfl_xor((unsigned long long)m, o, 64);
                    m = other < m ? other : m;
                }
                if (best == m && best_j != PS_TR_NONE) {  // (one lane: the keys are distinct)
                    nbr_j[out + p] = best_j;
                    nbr_num[out + p] = (uint32_t)(m >> 32);
                }
                prev = m;
            }
        } else {
            // an entry as a ps_tr_edge with lo = the neighbour's output row and hi = 0: ps_tr_less is the order (distance, row)
            const uint16_t *row = In ? In + (size_t)r * ldi : nullptr;
            const uint32_t cnt_i = In ? rowcnt[i] : 0u;
            ps_tr_edge prev;
            prev.num = 0ull; prev.den = 0ull; prev.lo = 0u; prev.hi = 0u;
            for (uint32_t p = 0; p < k; p++) {            // (k passes)
                ps_tr_edge best;
                best.num = 0ull; best.den = 0ull; best.lo = PS_TR_NONE; best.hi = 0u;
                uint32_t best_j = PS_TR_NONE;
                for (uint32_t q = 0; q < trips; q++) {    // (N / 64 trips; j < N <= ldi, rowcnt holds at least N entries)
                    const uint32_t j = lane + (q << 6);
                    if (j >= N || j == i) continue;
                    uint32_t in = 0u, un = 0u;
                    if (In) {
                        in = row[j];
                        un = cnt_i + rowcnt[j] - in;
                    }
                    ps_tr_edge e;
                    ps_tr_acc_distance(in, un, cg, &e.num, &e.den);
                    e.lo = out_row[j];
                    e.hi = 0u;
                    if (p != 0u && !ps_tr_less(prev, e)) continue;
                    if (best_j == PS_TR_NONE || ps_tr_less(e, best)) {
                        best = e;
                        best_j = j;
                    }
                }
                // (a lane without a candidate carries best_j = PS_TR_NONE; the output rows are distinct, so one lane wins)
                ps_tr_edge m = best;
                uint32_t m_j = best_j;
#pragma unroll
                for (int o = 32; o; o >>= 1) {
                    ps_tr_edge e;
                    e.num = (uint64_t)__shfl_xor((unsigned long long)m.num, o, 64);
                    e.den = (uint64_t)__shfl_xor((unsigned long long)m.den, o, 64);
                    e.lo = (uint32_t)__shfl_xor((int)m.lo, o, 64);
                    e.hi = 0u;
                    const uint32_t ej = (uint32_t)__shfl_xor((int)m_j, o, 64);
                    if (ej != PS_TR_NONE && (m_j == PS_TR_NONE || ps_tr_less(e, m))) {
                        m = e;
                        m_j = ej;
                    }
                }
                if (best_j != PS_TR_NONE && best_j == m_j) {
                    nbr_j[out + p] = m_j;
                    nbr_num[out + p] = (uint32_t)m.num;   // (a <= 65535, b < 2^32)
                    nbr_den[out + p] = (uint32_t)m.den;
                }
                prev = m;
            }
        }
    }
}
