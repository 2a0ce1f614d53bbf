// nni_kernels.h -- the gfx950 kernel of the parsimony tree search (ps_tree_nni, include/pansim_hip.h; the definitions:
// docs/PARSIMONY_SEARCH.md): the change of the tree's length under every nearest-neighbour interchange, in one pass over the
// core matrix.
//
// The team and the tile are tree_fitch_kernel's (parsimony_kernels.h): a workgroup owns four site rows, loads them with
// ps_load_row16, maps the bytes to class bits and leaves one dword per node in LDS with the four sites in its bytes: S, the
// Fitch up-set of the subtree below the node.  The up pass fills S level by level and counts the length T.  The search needs U,
// the Fitch set of everything OUTSIDE a node's subtree (U(c) = join(U(v), S(s)) for a node c with parent v and sibling s; below
// the root U(c) = S(s)), and for an internal node c = (a, b) the local term of the edge v - c
//     f(X, Y | Z, W) = e(X, Y) + e(Z, W) + e(join(X, Y), join(Z, W)),   e = 1 where the intersection is empty
// for the tree as it stands, f(Sa, Sb | Ss, Uv), and for the two interchanges, f(Sa, Ss | Sb, Uv) and f(Ss, Sb | Sa, Uv); on the
// root's edge the four sets are Sa, Sb, Sp, Sq of the quartet.  The rest of the length does not depend on the interchange, so
// the two signed differences are exact.  So every MERGE has a second pair of dwords in LDS, (U(v), S(s)): what its parent knows
// and it needs.  The down pass walks the levels back, a lane per merge c: one read of its schedule entry, then S of its two
// children and its pair side by side -- two dependent LDS trips per level, as the existing kernel's down pass has -- then the
// three terms, two counters of its own (i32 in LDS while they fit, else 64-bit global atomics on the non-zero values: a merge
// has one lane, so no atomics in LDS), and the pairs of its internal children, (U(c), S(the other child)).  Leaves need no
// pair: nothing reads the outside of a leaf.  The root's lane hands (S(s), S(s)) down, whose join is S(s), and counts the
// quartet of its two children on the left one; the driver marks the root's children in the schedule (PS_NNI_BELOW_ROOT), which
// have no interchange of their own.  S is never overwritten, and a barrier separates the levels.
//
// Integer adds commute: results do not depend on the launch geometry.
#pragma once

#include "parsimony_kernels.h"

// a schedule entry of tree_fitch_kernel with one more flag, in the bit between the two slots: the merge's parent is the root
#define PS_NNI_BELOW_ROOT 0x8000u

// u64 words the kernel accumulates
enum { PS_NNI_W_TOTAL = 0, PS_NNI_W_MIN = 1, PS_NNI_WORDS = 2 };

// the local term of four sets, four sites at once: the empties of the three intersections side by side in bits 7, 6, 5 of
// every byte (one popcount counts them all)
PS_HD uint32_t ps_nni_term(uint32_t x, uint32_t y, uint32_t z, uint32_t w)
{
    uint32_t e0, e1, e2;
    const uint32_t xy = ps_pars_join(x, y, &e0), zw = ps_pars_join(z, w, &e1);
    (void)ps_pars_join(xy, zw, &e2);
    return e0 | (e1 >> 1) | (e2 >> 2);
}

// The edge above c = (a, b): the term masks of the tree as it stands and of kind 0 and kind 1, (x, y | z, w) -> (x, z | y, w),
// (z, y | x, w).  Below an inner node (x, y, z, w) = (Sa, Sb, Ss, Uv); on the root's edge (Sa, Sb, Sp, Sq), where the second
// form (p, b | a, q) is the term of kind 1's tree (a, q | p, b) with its two sides exchanged.  The caller counts the bits.
PS_HD void ps_nni_edge(uint32_t x, uint32_t y, uint32_t z, uint32_t w, uint32_t m[3])
{
    m[0] = ps_nni_term(x, y, z, w);
    m[1] = ps_nni_term(x, z, y, w);
    m[2] = ps_nni_term(z, y, x, w);
}

// state, pitch, N, rows, sched, level_off, levels, M, n_pad: as tree_fitch_kernel takes them, of a SPANNING tree (M = N - 1, one
// root: the only entry of the last level), the entries of the root's internal children marked PS_NNI_BELOW_ROOT.  Dynamic LDS:
// n_pad + M node dwords rounded up to an even number, M pairs of dwords behind them, with lds_counters 2 M i32 counters behind
// those, with sched_lds M + levels + 1 dwords of schedule behind those.  words[PS_NNI_WORDS] and delta[2 M] (both zeroed by the
// caller) accumulate: delta[2 j + kind] of the merge at schedule position j, two's complement in u64.  Any grid is valid:
// workgroups stride over the tiles.  Rows past the last count as monomorphic.
__global__ void __launch_bounds__(1024) tree_nni_kernel(const uint8_t *state, uint32_t pitch, uint32_t N, uint32_t rows, const uint32_t *sched,
                                                        const uint32_t *level_off, uint32_t levels, uint32_t M, uint32_t n_pad,
                                                        uint32_t lds_counters, uint32_t sched_lds, unsigned long long *words,
                                                        unsigned long long *delta)
{
    extern __shared__ uint4 nni_lds[];            // (16-byte aligned: the leaves are stored four nodes at a time)
    uint32_t *S = (uint32_t *)nni_lds;
    __shared__ unsigned long long nni_acc[PS_NNI_WORDS];
    __shared__ uint32_t nni_or, nni_and;
    const uint32_t tid = threadIdx.x, T = blockDim.x, lane = tid & 63u;
    const uint32_t slots = (n_pad + M + 1u) & ~1u;
    uint2 *PQ = (uint2 *)(S + slots);             // per merge: (U of its parent, S of its sibling)
    int32_t *cnt = (int32_t *)(PQ + M);
    if (lds_counters)
        for (uint32_t i = tid; i < 2u * M; i += T) cnt[i] = 0;
    if (tid < (uint32_t)PS_NNI_WORDS) nni_acc[tid] = 0ull;
    // the schedule where the levels read it: its LDS copy (made here; the first tile's barrier orders it) or global memory
    uint32_t *ls = (uint32_t *)cnt + (lds_counters ? 2u * M : 0u), *lo = ls + M;
    if (sched_lds) {
        for (uint32_t i = tid; i < M; i += T) ls[i] = sched[i];
        for (uint32_t i = tid; i <= levels; i += T) lo[i] = level_off[i];
    }
    auto entry = [&](uint32_t j) { return sched_lds ? ls[j] : sched[j]; };
    auto level = [&](uint32_t l) { return sched_lds ? lo[l] : level_off[l]; };
    auto count = [&](uint32_t j, int32_t d0, int32_t d1) {
        if (lds_counters) {
            cnt[2u * j] += d0;
            cnt[2u * j + 1u] += d1;
        } else {
            if (d0) atomicAdd(&delta[2u * j], (unsigned long long)(long long)d0);
            if (d1) atomicAdd(&delta[2u * j + 1u], (unsigned long long)(long long)d1);
        }
    };
    uint64_t s_min = 0;
    const uint32_t ntiles = (rows + 3u) >> 2;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tid == 0u) {
            nni_or = 0u;
            nni_and = 0xFFFFFFFFu;
        }
        __syncthreads();
        // the leaves: 16 cells of each of the four rows per thread and trip, transposed to one dword per leaf
        uint32_t orw = 0u, andw = 0xFFFFFFFFu;
        for (uint32_t base = tid * 16u; base < n_pad; base += T * 16u) {
            uint32_t r[4][4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                const uint32_t row = tile * 4u + k;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (row < rows) v = ps_load_row16(state + (size_t)row * pitch + base, true);
                r[k][0] = v.x;
                r[k][1] = v.y;
                r[k][2] = v.z;
                r[k][3] = v.w;
            }
            uint32_t bad = 0u;
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++)
#pragma unroll
                for (uint32_t q = 0; q < 4u; q++)
                    bad |= ps_div_suspect(r[k][q]) | (~ps_pars_nonzero(r[k][q] & 0x0F0F0F0Fu) & 0x80808080u);
            if (__any(bad != 0u)) {
                // a byte that is not 1 / 2 / 4 / 8 somewhere in the wave's piece: the exact map
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++)
#pragma unroll
                    for (uint32_t q = 0; q < 4u; q++) r[k][q] = ps_pars_classes(r[k][q]);
            }
            uint32_t w[16];
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) {
                const uint32_t a = r[0][q], b = r[1][q], c = r[2][q], d = r[3][q];
                const uint32_t t0 = (a & 0x00FF00FFu) | ((b & 0x00FF00FFu) << 8), t1 = ((a >> 8) & 0x00FF00FFu) | (b & 0xFF00FF00u);
                const uint32_t t2 = (c & 0x00FF00FFu) | ((d & 0x00FF00FFu) << 8), t3 = ((c >> 8) & 0x00FF00FFu) | (d & 0xFF00FF00u);
                w[4u * q] = (t0 & 0xFFFFu) | (t2 << 16);
                w[4u * q + 1u] = (t1 & 0xFFFFu) | (t3 << 16);
                w[4u * q + 2u] = (t0 >> 16) | (t2 & 0xFFFF0000u);
                w[4u * q + 3u] = (t1 >> 16) | (t3 & 0xFFFF0000u);
            }
#pragma unroll
            for (uint32_t i = 0; i < 16u; i++)
                if (base + i < N) {
                    orw |= w[i];
                    andw &= w[i];
                }
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++)
                *(uint4 *)(S + base + 4u * q) = make_uint4(w[4u * q], w[4u * q + 1u], w[4u * q + 2u], w[4u * q + 3u]);
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            orw |= (uint32_t)__shfl_xor((int)orw, o, 64);
            andw &= (uint32_t)__shfl_xor((int)andw, o, 64);
        }
        if (lane == 0u) {
            atomicOr(&nni_or, orw);
            atomicAnd(&nni_and, andw);
        }
        __syncthreads();
        const uint32_t all_or = nni_or, all_and = nni_and;
        __syncthreads();                  // (both are read before the next tile resets them)
        if (all_or != all_and) {          // (team-uniform; a tile whose leaves all agree changes no length)
            uint32_t changes = 0u;
            for (uint32_t lev = 0; lev < levels; lev++) {
                const uint32_t hi = level(lev + 1u);
                for (uint32_t j = level(lev) + tid; j < hi; j += T) {
                    const uint32_t e = entry(j);
                    uint32_t z;
                    S[n_pad + j] = ps_pars_join(S[e & PS_PARS_SLOT], S[(e >> 16) & PS_PARS_SLOT], &z);
                    changes += (uint32_t)__popc(z);
                }
                __syncthreads();
            }
            for (uint32_t lev = levels; lev-- > 0u;) {
                const uint32_t hi = level(lev + 1u);
                for (uint32_t j = level(lev) + tid; j < hi; j += T) {
                    const uint32_t e = entry(j);
                    const uint32_t cl = e & PS_PARS_SLOT, cr = (e >> 16) & PS_PARS_SLOT;
                    const uint32_t sl = S[cl], sr = S[cr];
                    uint32_t m[3];
                    if (e & PS_PARS_ROOT) {
                        // the root's edge: the quartet of its two children, counted on the left one
                        if (cl >= n_pad && cr >= n_pad) {
                            const uint32_t ec = entry(cl - n_pad), es = entry(cr - n_pad);
                            ps_nni_edge(S[ec & PS_PARS_SLOT], S[(ec >> 16) & PS_PARS_SLOT], S[es & PS_PARS_SLOT], S[(es >> 16) & PS_PARS_SLOT], m);
                            const int32_t cur = (int32_t)__popc(m[0]);
                            count(cl - n_pad, (int32_t)__popc(m[1]) - cur, (int32_t)__popc(m[2]) - cur);
                        }
                        if (cl >= n_pad) PQ[cl - n_pad] = make_uint2(sr, sr);
                        if (cr >= n_pad) PQ[cr - n_pad] = make_uint2(sl, sl);
                    } else {
                        const uint2 pq = PQ[j];
                        uint32_t z;
                        const uint32_t u = ps_pars_join(pq.x, pq.y, &z);
                        if (!(e & PS_NNI_BELOW_ROOT)) {
                            ps_nni_edge(sl, sr, pq.y, pq.x, m);
                            const int32_t cur = (int32_t)__popc(m[0]);
                            count(j, (int32_t)__popc(m[1]) - cur, (int32_t)__popc(m[2]) - cur);
                        }
                        if (cl >= n_pad) PQ[cl - n_pad] = make_uint2(u, sr);
                        if (cr >= n_pad) PQ[cr - n_pad] = make_uint2(u, sl);
                    }
                }
                __syncthreads();
            }
#pragma unroll
            for (int o = 32; o; o >>= 1) changes += (uint32_t)__shfl_xor((int)changes, o, 64);
            if (lane == 0u && changes) atomicAdd(&nni_acc[PS_NNI_W_TOTAL], (unsigned long long)changes);
        }
        if (tid < 4u && tile * 4u + tid < rows) s_min += (uint32_t)__popc((all_or >> (8u * tid)) & 0x1Fu) - 1u;
    }
    if (tid < 4u && s_min) atomicAdd(&nni_acc[PS_NNI_W_MIN], (unsigned long long)s_min);
    __syncthreads();
    // the flush: one atomic per workgroup and non-zero word
    if (tid < (uint32_t)PS_NNI_WORDS && nni_acc[tid] != 0ull) atomicAdd(&words[tid], nni_acc[tid]);
    if (lds_counters)
        for (uint32_t i = tid; i < 2u * M; i += T)
            if (cnt[i]) atomicAdd(&delta[i], (unsigned long long)(long long)cnt[i]);
}
