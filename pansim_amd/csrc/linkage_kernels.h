// linkage_kernels.h -- the kernels of ps_linkage_tree (docs/LINKAGE_TREE.md) and the integer edge order they share with the
// host restatement (ps_tree_from_counts).
//
// The store kernels keep the per-band input of pair_hist_kernel -- the u32 Hamming numerators h(i, j) of rows [lo, lo + nrows)
// against all N columns, or the u16 accessory intersections of the same rows -- as rows [lo, lo + nrows) of a full N x N matrix.
// Both contractions write the whole rectangle of a band (core_allpairs_mfma_fp4_kernel<true>, core_band_counts_simple,
// acc_intersections_mfma_kernel: every column tile), so the matrix is complete -- both (i, j) and (j, i) -- once every band has
// passed; nothing is mirrored.  The Boruvka kernels then work on comp[N] (the component of each internal row, always the row
// index of its root) until one component is left: the minimum edge of each row out of its component, the minimum of each
// component over its rows, the hooks of the components across their edges, pointer jumping to the new roots.  The order on
// edges is strict (ps_tr_less), so the tree is unique and none of this depends on the grid or on the order of the atomics.
#pragma once

#include <stdint.h>

#define PS_TR_NONE 0xffffffffu

// an edge under the total order (distance, lo, hi): distance = num / den, den == 0 = undefined; lo < hi in OUTPUT rows
struct ps_tr_edge {
    uint64_t num, den;
    uint32_t lo, hi;
};

// -1 / 0 / +1: num1 / den1 below / equal to / above num2 / den2.  An undefined distance is above every defined one and equal
// to every other undefined one.  Equal denominators (every core pair of a call) compare by their numerators; otherwise the
// cross products, in u64: the accessory a <= 65535 and b = U + core_genes < 2^32 keep them below 2^48.  No floating point.
__host__ __device__ __forceinline__ int ps_tr_dist_cmp(uint64_t num1, uint64_t den1, uint64_t num2, uint64_t den2)
{
    if (den1 == den2) return num1 < num2 ? -1 : num1 > num2 ? 1 : 0;
    if (den1 == 0ull) return 1;
    if (den2 == 0ull) return -1;
    const uint64_t x = num1 * den2, y = num2 * den1;
    return x < y ? -1 : x > y ? 1 : 0;
}

__host__ __device__ __forceinline__ bool ps_tr_less(const ps_tr_edge &a, const ps_tr_edge &b)
{
    const int c = ps_tr_dist_cmp(a.num, a.den, b.num, b.den);
    if (c) return c < 0;
    return a.lo != b.lo ? a.lo < b.lo : a.hi < b.hi;
}

// the accessory distance of a pair from its intersection and union: a / b, or 0 / 0 for b == 0 (the reference's NaN)
__host__ __device__ __forceinline__ void ps_tr_acc_distance(uint32_t in, uint32_t un, uint64_t cg, uint64_t *num, uint64_t *den)
{
    *den = (uint64_t)un + cg;
    *num = *den ? (uint64_t)(un - in) : 0ull;
}

__device__ __forceinline__ ps_tr_edge ps_tr_make(uint64_t num, uint64_t den, uint32_t oi, uint32_t oj)
{
    ps_tr_edge e;
    e.num = num;
    e.den = den;
    e.lo = min(oi, oj);
    e.hi = max(oi, oj);
    return e;
}

// M[i][j] = C[i - lo][j] for the band's rows i = lo + r < N and the columns j < ldm (ldm: N rounded up to 64, so a row is
// whole uint4s); columns >= N are stored as 0.  Grid: x over the uint4s of a row, y strides over the band's rows (loop bound:
// nrows / gridDim.y); any grid is valid.
__global__ void __launch_bounds__(256) tree_store_core_kernel(const uint32_t *C, uint64_t ldc, uint32_t N, uint32_t lo, uint32_t nrows,
                                                              uint32_t *M, uint64_t ldm)
{
    const uint32_t j = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (j >= ldm) return;                                 // (j + 3 < ldm <= ldc: the uint4 load stays inside the band's row)
    for (uint32_t r = blockIdx.y; r < nrows; r += gridDim.y) {
        const uint32_t i = lo + r;
        if (i >= N) break;                                // (rows ascend: pad rows from here on)
        uint4 v = *(const uint4 *)(C + (size_t)r * ldc + j);
        if (j + 0u >= N) v.x = 0u;
        if (j + 1u >= N) v.y = 0u;
        if (j + 2u >= N) v.z = 0u;
        if (j + 3u >= N) v.w = 0u;
        *(uint4 *)(M + (size_t)i * ldm + j) = v;
    }
}

// The same for the u16 intersections: two columns per thread as one dword (ldi and ldm are even and the rows dword-aligned).
__global__ void __launch_bounds__(256) tree_store_acc_kernel(const uint16_t *In, uint32_t ldi, uint32_t N, uint32_t lo, uint32_t nrows,
                                                             uint16_t *M, uint64_t ldm)
{
    const uint32_t j = (blockIdx.x * 256u + threadIdx.x) * 2u;
    if (j >= ldm) return;                                 // (j + 1 < ldm <= ldi)
    for (uint32_t r = blockIdx.y; r < nrows; r += gridDim.y) {
        const uint32_t i = lo + r;
        if (i >= N) break;
        uint32_t v = *(const uint32_t *)(In + (size_t)r * ldi + j);
        if (j + 0u >= N) v &= 0xffff0000u;
        if (j + 1u >= N) v &= 0x0000ffffu;
        *(uint32_t *)(M + (size_t)i * ldm + j) = v;
    }
}

// comp[i] = parent[i] = i; out_row[slot[k]] = k is uploaded by the host
__global__ void __launch_bounds__(256) tree_init_kernel(uint32_t *comp, uint32_t *parent, uint32_t N)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < N) comp[i] = parent[i] = i;
}

// Row minimum.  One wave per row i (the waves stride over the rows: N / waves trips); lane l the columns l + 64 q (N / 64 trips),
// coalesced.  The lane minimum under ps_tr_less over the j with comp[j] != comp[i], then six shuffle steps to the wave's.
// cand_j[i] = PS_TR_NONE when the row's component is everything.  ACC: Ma holds the intersections (nullptr: no accessory genes,
// I = U = 0 for every pair) and rowcnt the rows' gene counts; else Mc holds h and every den is 1 (equal: compared by num = h / 2).
template <bool ACC>
__global__ void __launch_bounds__(256) tree_row_min_kernel(const uint32_t *Mc, const uint16_t *Ma, uint64_t ldm, const uint32_t *rowcnt,
                                                           uint64_t cg, uint32_t N, const uint32_t *comp, const uint32_t *out_row,
                                                           uint32_t *cand_j, uint32_t *cand_num, uint32_t *cand_den)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    for (uint32_t i = wave; i < N; i += gridDim.x * 4u) {
        const uint32_t ci = comp[i], oi = out_row[i];
        const uint32_t cnt_i = (ACC && Ma) ? rowcnt[i] : 0u;
        ps_tr_edge best;
        best.num = 0ull; best.den = 0ull; best.lo = PS_TR_NONE; best.hi = PS_TR_NONE;
        uint32_t best_j = PS_TR_NONE;
        for (uint32_t j = lane; j < N; j += 64u) {        // (j < N <= ldm: every load stays inside row i)
            if (comp[j] == ci) continue;
            uint64_t num, den;
            if (ACC) {
                uint32_t in = 0u, un = 0u;
                if (Ma) {
                    in = Ma[(size_t)i * ldm + j];
                    un = cnt_i + rowcnt[j] - in;
                }
                ps_tr_acc_distance(in, un, cg, &num, &den);
            } else {
                num = Mc[(size_t)i * ldm + j] >> 1;
                den = 1ull;
            }
            const ps_tr_edge e = ps_tr_make(num, den, oi, out_row[j]);
            if (best_j == PS_TR_NONE || ps_tr_less(e, best)) {
                best = e;
                best_j = j;
            }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            ps_tr_edge e;
            e.num = (uint64_t)__shfl_xor((unsigned long long)best.num, o, 64);
            e.den = (uint64_t)__shfl_xor((unsigned long long)best.den, o, 64);
            e.lo = (uint32_t)__shfl_xor((int)best.lo, o, 64);
            e.hi = (uint32_t)__shfl_xor((int)best.hi, o, 64);
            const uint32_t ej = (uint32_t)__shfl_xor((int)best_j, o, 64);
            if (ej != PS_TR_NONE && (best_j == PS_TR_NONE || ps_tr_less(e, best))) {
                best = e;
                best_j = ej;
            }
        }
        if (lane == 0u) {
            cand_j[i] = best_j;
            cand_num[i] = (uint32_t)best.num;             // (d < 2^31, a <= 65535, b < 2^32)
            cand_den[i] = (uint32_t)best.den;
        }
    }
}

// the edge that row r proposes (cand_j[r] != PS_TR_NONE)
__device__ __forceinline__ ps_tr_edge ps_tr_cand(uint32_t r, const uint32_t *cand_j, const uint32_t *cand_num, const uint32_t *cand_den,
                                                 const uint32_t *out_row)
{
    return ps_tr_make(cand_num[r], cand_den[r], out_row[r], out_row[cand_j[r]]);
}

// Component minimum.  One thread per row; best[c] (PS_TR_NONE before the kernel) is lowered by compare-and-swap to the row of
// component c whose candidate is the smallest.  The candidates do not change during the kernel and every successful exchange
// lowers the slot strictly in the total order, so a slot changes fewer than N times and a thread fails fewer than N times: the
// loop is bounded by N (and cut there).  No thread waits for another.
__global__ void __launch_bounds__(256) tree_comp_min_kernel(uint32_t N, const uint32_t *comp, const uint32_t *out_row, const uint32_t *cand_j,
                                                            const uint32_t *cand_num, const uint32_t *cand_den, uint32_t *best)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N || cand_j[i] == PS_TR_NONE) return;
    const ps_tr_edge mine = ps_tr_cand(i, cand_j, cand_num, cand_den, out_row);
    uint32_t *slot = best + comp[i];                      // (comp[i] < N)
    uint32_t cur = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t tries = 0; tries < N; tries++) {
        if (cur != PS_TR_NONE && !ps_tr_less(mine, ps_tr_cand(cur, cand_j, cand_num, cand_den, out_row))) return;
        const uint32_t seen = atomicCAS(slot, cur, i);
        if (seen == cur) return;
        cur = seen;
    }
}

// Link.  One thread per row, at work for the roots c (comp[c] == c) only.  c hooks to c2, the component across its edge
// (r, j) = (best[c], cand_j[best[c]]); when c2 chose the same edge -- exactly one pair of every new tree did -- the smaller of the
// two stays a root.  Every root's edge goes to the list (through one atomic counter; any order), the shared one once.  comp, best
// and the candidates are only read; parent[c] is written by c's thread alone.  No loop.
__global__ void __launch_bounds__(256) tree_link_kernel(uint32_t N, const uint32_t *comp, const uint32_t *cand_j, const uint32_t *cand_num,
                                                        const uint32_t *cand_den, const uint32_t *best, uint32_t *parent, uint32_t *count,
                                                        uint32_t *e_i, uint32_t *e_j, uint32_t *e_num, uint32_t *e_den)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= N || comp[c] != c) return;
    const uint32_t r = best[c];
    if (r == PS_TR_NONE) {                                // (one component is left)
        parent[c] = c;
        return;
    }
    const uint32_t j = cand_j[r], c2 = comp[j], r2 = best[c2];
    const bool shared = r2 == j && cand_j[r2] == r;       // (r2 != PS_TR_NONE: c2 has a way out, to c at the least)
    const bool stays = shared && c < c2;
    parent[c] = stays ? c : c2;
    if (shared && !stays) return;
    const uint32_t k = atomicAdd(count, 1u);
    if (k + 1u < N) {                                     // (a spanning forest has at most N - 1 edges: the lists hold N)
        e_i[k] = r;
        e_j[k] = j;
        e_num[k] = cand_num[r];
        e_den[k] = cand_den[r];
    }
}

// Jump.  comp[i] <- the root above comp[i].  parent is not written here and its hooks form a forest over the old roots, so the
// chain ends within N steps (and the loop is cut there); each thread writes its own comp[i] only.
__global__ void __launch_bounds__(256) tree_jump_kernel(uint32_t N, const uint32_t *parent, uint32_t *comp)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    uint32_t c = comp[i];
    for (uint32_t steps = 0; steps < N; steps++) {
        const uint32_t p = parent[c];                     // (c < N and parent[c] < N throughout)
        if (p == c) break;
        c = p;
    }
    comp[i] = c;
}
