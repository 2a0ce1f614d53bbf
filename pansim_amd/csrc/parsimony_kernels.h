// parsimony_kernels.h -- gfx950 kernels of the parsimony of a matrix on a tree (ps_tree_parsimony, include/pansim_hip.h; the
// definitions: docs/TREE_PARSIMONY.md).
//
// Fitch parsimony of a column is a dependent chain of one set operation per merge, so the parallel axes are the sites and
// the merges of one LEVEL of the tree (level of a merge = 1 + the larger of its children's, leaves at 0): merges of one level
// are independent, only level boundaries order anything.  A TEAM -- one workgroup: a single wave for N <= 1024, 256 or 1024
// threads above -- owns a tile of four site rows.  It loads the rows with ps_load_row16, maps every byte to its class bit
// (1, 2, 4, 8, anything else 0x10; free for clean data: ps_div_suspect and a zero test decide per dword), transposes 4 x 4
// bytes in registers and leaves in LDS one dword per NODE with the four sites in its bytes: leaves at their internal row,
// merge j of the level-ordered schedule at n_pad + j.  The schedule itself is copied to LDS once per workgroup while it fits: a
// level is a handful of instructions, and a global load per level and tile would be all the time there is.  The up pass walks the levels, a lane per merge: two LDS reads, the
// byte-parallel ps_pars_join, one LDS write; the down pass walks them back over the same dwords, overwriting the sets S with
// the picks X (ps_pars_pick) and counting the branches that change -- in LDS counters per node while they fit beside the
// node dwords (a node is the child of one merge, so a counter has one writer per tile: no atomics), else with global atomics.
// A barrier separates the levels; for the single-wave team it is a wave-local fence.  A tile whose leaves all agree (team-wide
// OR == AND) skips both passes.  Both per-node functions are shared with the host's ps_parsimony_from_rows.
//
// Integer adds commute: results do not depend on the launch geometry.
#pragma once

#include "diversity_kernels.h"

// u64 words the kernel accumulates; the histogram of the sites by their changes follows
enum { PS_PARS_W_TOTAL = 0, PS_PARS_W_CHANGED = 1, PS_PARS_W_MAX = 2, PS_PARS_W_MIN = 3, PS_PARS_W_HOMO = 4, PS_PARS_W_GAINS = 5,
       PS_PARS_W_HIST = 8, PS_PARS_WORDS = 8 + 64 };

// a schedule entry: the LDS slots of the two children in bits 0 .. 14 and 16 .. 30, bit 31 = the merge's node is a root
#define PS_PARS_ROOT 0x80000000u
#define PS_PARS_SLOT 0x7FFFu

// 0x80 in every byte of w that is not zero (bytes below 0x80: the sum never carries into the next byte)
PS_HD uint32_t ps_pars_nonzero(uint32_t w) { return ((w + 0x7F7F7F7Fu) | w) & 0x80808080u; }

// the class bits of four cells: 1, 2, 4, 8 stay, every other byte (zero included) is the fifth class 0x10
PS_HD uint32_t ps_pars_classes(uint32_t w)
{
    const uint32_t m = 0x01010101u;
    const uint32_t p0 = w & m, p1 = (w >> 1) & m, p2 = (w >> 2) & m, p3 = (w >> 3) & m;
    uint32_t h = w & 0xF0F0F0F0u;
    h |= h >> 2;
    h |= h >> 1;
    const uint32_t two = (p0 & p1) | (p2 & p3) | ((p0 | p1) & (p2 | p3));
    const uint32_t keep = ((p0 | p1 | p2 | p3) & ~(two | (h >> 4))) * 0xFFu;
    return (w & keep) | (0x10101010u & ~keep);
}

// Up pass, four sites at once: S(node) = S(l) & S(r) where that is not empty, else S(l) | S(r); *empty has 0x80 in the bytes
// whose intersection was empty (one change each)
PS_HD uint32_t ps_pars_join(uint32_t a, uint32_t b, uint32_t *empty)
{
    const uint32_t i = a & b;
    const uint32_t z = ~ps_pars_nonzero(i) & 0x80808080u;
    *empty = z;
    return i | ((a | b) & ((z >> 7) * 0xFFu));
}

// the pick of a root: the lowest set bit of every byte (no byte of a set is zero, so the subtraction never borrows)
PS_HD uint32_t ps_pars_root(uint32_t s) { return s & ~(s - 0x01010101u); }

// Down pass, four sites at once: X(c) = X(v) where X(v) & S(c) is not empty, else the lowest bit of S(c); *changed has 0x80
// in the bytes where X(c) != X(v) (the branch above c changes)
PS_HD uint32_t ps_pars_pick(uint32_t xv, uint32_t sc, uint32_t *changed)
{
    const uint32_t keep = ps_pars_nonzero(xv & sc);
    const uint32_t km = (keep >> 7) * 0xFFu;
    *changed = ~keep & 0x80808080u;
    return (xv & km) | (ps_pars_root(sc) & ~km);
}

// of the changing bytes, those whose new state is 2: gains of a gene (the others are losses)
PS_HD uint32_t ps_pars_gains(uint32_t xc, uint32_t changed) { return changed & (xc << 6); }

// accG: the gene-major view (G rows of W words over the internal rows) -> bytes[(gene - first) pitch + i] = 2 if internal
// individual i carries the gene, else 1; i < pitch (a multiple of 16; cells from N on are 1 and never read as leaves)
__global__ void __launch_bounds__(256) pars_expand_genes_kernel(const uint64_t *accG, acc_dims d, uint32_t first, uint32_t count,
                                                                uint32_t pitch, uint8_t *bytes)
{
    const uint32_t per_row = pitch >> 4;
    const uint64_t n = (uint64_t)count * per_row;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t g = (uint32_t)(t / per_row), c = (uint32_t)(t % per_row) * 16u;
        const uint32_t wi = c >> 6;
        const uint64_t word = wi < d.W ? accG[(uint64_t)(first + g) * d.W + wi] : 0ull;
        const uint32_t bits = (uint32_t)(word >> (c & 63u)) & 0xFFFFu;
        uint32_t o[4];
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++) {
            uint32_t w = 0x01010101u;
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++)
                if (c + 4u * q + j < d.N && ((bits >> (4u * q + j)) & 1u)) w += 1u << (8u * j);
            o[q] = w;
        }
        *(uint4 *)(bytes + (size_t)g * pitch + c) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// state: rows x pitch bytes, N live cells per row (pitch >= n_pad = N rounded up to 16).  sched[M]: the merges in (level, merge)
// order, level_off[levels + 1] their level boundaries.  Dynamic LDS: n_pad + M node dwords, and with lds_counters as many u32
// counters behind them (GENES: twice, gains then losses), and with sched_lds M + levels + 1 dwords of schedule behind those.  words[PS_PARS_WORDS] (zeroed by the caller) accumulate;
// site_changes / site_gains[site_base + row] (either may be null); DOWN: branch[slot] and, GENES, branch_loss[slot] (u64, zeroed
// by the caller) accumulate the changing branches per LDS slot of their lower node (GENES: gains in branch).  Any grid is
// valid: workgroups stride over the tiles.  Rows past the last count as monomorphic and store nothing.
template <bool GENES, bool DOWN>
__global__ void __launch_bounds__(1024) tree_fitch_kernel(const uint8_t *state, uint32_t pitch, uint32_t N, uint32_t rows,
                                                          const uint32_t *sched, const uint32_t *level_off, uint32_t levels, uint32_t M,
                                                          uint32_t n_pad, uint32_t lds_counters, uint32_t sched_lds,
                                                          unsigned long long *words,
                                                          uint32_t *site_changes, uint32_t *site_gains, uint32_t site_base,
                                                          unsigned long long *branch, unsigned long long *branch_loss)
{
    extern __shared__ uint4 pars_lds[];           // (16-byte aligned: the leaves are stored four nodes at a time)
    uint32_t *pars_nodes = (uint32_t *)pars_lds;
    __shared__ uint32_t pars_hist[64];
    __shared__ unsigned long long pars_acc[8];
    __shared__ uint32_t pars_or, pars_and, pars_chg[2], pars_gain[2];
    const uint32_t tid = threadIdx.x, T = blockDim.x, lane = tid & 63u;
    const uint32_t slots = n_pad + M;
    uint32_t *cnt = pars_nodes + slots, *cnt2 = cnt + slots;
    if (DOWN && lds_counters)
        for (uint32_t i = tid; i < slots * (GENES ? 2u : 1u); i += T) cnt[i] = 0u;
    if (tid < 64u) pars_hist[tid] = 0u;
    if (tid < 8u) pars_acc[tid] = 0ull;
    // the schedule where the levels read it: its LDS copy (made here; the first tile's barrier orders it) or global memory
    uint32_t *ls = pars_nodes + slots * (1u + (DOWN && lds_counters ? (GENES ? 2u : 1u) : 0u)), *lo = ls + M;
    if (sched_lds) {
        for (uint32_t i = tid; i < M; i += T) ls[i] = sched[i];
        for (uint32_t i = tid; i <= levels; i += T) lo[i] = level_off[i];
    }
    auto entry = [&](uint32_t j) { return sched_lds ? ls[j] : sched[j]; };
    auto level = [&](uint32_t l) { return sched_lds ? lo[l] : level_off[l]; };
    // the summary terms of the sites that threads 0 .. 3 finish
    uint64_t s_total = 0, s_changed = 0, s_max = 0, s_min = 0, s_homo = 0, s_gains = 0;
    const uint32_t ntiles = (rows + 3u) >> 2;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tid == 0u) {
            pars_or = 0u;
            pars_and = 0xFFFFFFFFu;
            pars_chg[0] = pars_chg[1] = pars_gain[0] = pars_gain[1] = 0u;
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
                *(uint4 *)(pars_nodes + base + 4u * q) = make_uint4(w[4u * q], w[4u * q + 1u], w[4u * q + 2u], w[4u * q + 3u]);
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            orw |= (uint32_t)__shfl_xor((int)orw, o, 64);
            andw &= (uint32_t)__shfl_xor((int)andw, o, 64);
        }
        if (lane == 0u) {
            atomicOr(&pars_or, orw);
            atomicAnd(&pars_and, andw);
        }
        __syncthreads();
        const uint32_t all_or = pars_or, all_and = pars_and;
        __syncthreads();                  // (both are read before the next tile resets them)
        if (all_or != all_and) {          // (team-uniform)
            // changes of sites 0, 2 and of sites 1, 3 of the tile in 16-bit fields: a site has at most M < 2^15 in all
            uint32_t c02 = 0u, c13 = 0u, g02 = 0u, g13 = 0u;
            for (uint32_t lev = 0; lev < levels; lev++) {
                const uint32_t hi = level(lev + 1u);
                for (uint32_t j = level(lev) + tid; j < hi; j += T) {
                    const uint32_t e = entry(j);
                    uint32_t z;
                    pars_nodes[n_pad + j] = ps_pars_join(pars_nodes[e & PS_PARS_SLOT], pars_nodes[(e >> 16) & PS_PARS_SLOT], &z);
                    c02 += (z >> 7) & 0x00010001u;
                    c13 += (z >> 15) & 0x00010001u;
                }
                __syncthreads();
            }
            if (DOWN) {
                for (uint32_t lev = levels; lev-- > 0u;) {
                    const uint32_t hi = level(lev + 1u);
                    for (uint32_t j = level(lev) + tid; j < hi; j += T) {
                        const uint32_t e = entry(j);
                        const uint32_t v = pars_nodes[n_pad + j];
                        const uint32_t xv = (e & PS_PARS_ROOT) ? ps_pars_root(v) : v;
#pragma unroll
                        for (uint32_t side = 0; side < 2u; side++) {
                            const uint32_t c = (side ? e >> 16 : e) & PS_PARS_SLOT;
                            uint32_t ch;
                            const uint32_t xc = ps_pars_pick(xv, pars_nodes[c], &ch);
                            pars_nodes[c] = xc;
                            const uint32_t nch = (uint32_t)__popc(ch);
                            if (GENES) {
                                const uint32_t gn = ps_pars_gains(xc, ch), ng = (uint32_t)__popc(gn);
                                g02 += (gn >> 7) & 0x00010001u;
                                g13 += (gn >> 15) & 0x00010001u;
                                if (lds_counters) {
                                    cnt[c] += ng;
                                    cnt2[c] += nch - ng;
                                } else {
                                    if (ng) atomicAdd(&branch[c], (unsigned long long)ng);
                                    if (nch - ng) atomicAdd(&branch_loss[c], (unsigned long long)(nch - ng));
                                }
                            } else if (lds_counters) {
                                cnt[c] += nch;
                            } else if (nch) {
                                atomicAdd(&branch[c], (unsigned long long)nch);
                            }
                        }
                    }
                    __syncthreads();
                }
            }
#pragma unroll
            for (int o = 32; o; o >>= 1) {
                c02 += (uint32_t)__shfl_xor((int)c02, o, 64);
                c13 += (uint32_t)__shfl_xor((int)c13, o, 64);
                if (GENES && DOWN) {
                    g02 += (uint32_t)__shfl_xor((int)g02, o, 64);
                    g13 += (uint32_t)__shfl_xor((int)g13, o, 64);
                }
            }
            if (lane == 0u) {
                if (c02) atomicAdd(&pars_chg[0], c02);
                if (c13) atomicAdd(&pars_chg[1], c13);
                if (GENES && DOWN) {
                    if (g02) atomicAdd(&pars_gain[0], g02);
                    if (g13) atomicAdd(&pars_gain[1], g13);
                }
            }
            __syncthreads();
        }
        if (tid < 4u) {
            const uint32_t site = tile * 4u + tid;
            if (site < rows) {
                const uint32_t sh = 16u * (tid >> 1);
                const uint32_t ch = (pars_chg[tid & 1u] >> sh) & 0xFFFFu, gn = (pars_gain[tid & 1u] >> sh) & 0xFFFFu;
                const uint32_t classes = (uint32_t)__popc((all_or >> (8u * tid)) & 0x1Fu);
                if (site_changes) site_changes[site_base + site] = ch;
                if (GENES && DOWN && site_gains) site_gains[site_base + site] = gn;
                s_total += ch;
                s_changed += ch != 0u;
                s_max = ch > s_max ? ch : s_max;
                s_min += classes - 1u;
                s_homo += ch > classes - 1u;
                s_gains += gn;
                atomicAdd(&pars_hist[ch < 63u ? ch : 63u], 1u);
            }
        }
    }
    if (tid < 4u) {
        atomicAdd(&pars_acc[PS_PARS_W_TOTAL], (unsigned long long)s_total);
        atomicAdd(&pars_acc[PS_PARS_W_CHANGED], (unsigned long long)s_changed);
        atomicMax(&pars_acc[PS_PARS_W_MAX], (unsigned long long)s_max);
        atomicAdd(&pars_acc[PS_PARS_W_MIN], (unsigned long long)s_min);
        atomicAdd(&pars_acc[PS_PARS_W_HOMO], (unsigned long long)s_homo);
        atomicAdd(&pars_acc[PS_PARS_W_GAINS], (unsigned long long)s_gains);
    }
    __syncthreads();
    // the flush: one atomic per workgroup and non-zero word
    if (tid < 8u && pars_acc[tid] != 0ull) {
        if (tid == (uint32_t)PS_PARS_W_MAX) atomicMax(&words[tid], pars_acc[tid]);
        else atomicAdd(&words[tid], pars_acc[tid]);
    }
    if (tid < 64u && pars_hist[tid] != 0u) atomicAdd(&words[PS_PARS_W_HIST + tid], (unsigned long long)pars_hist[tid]);
    if (DOWN && lds_counters)
        for (uint32_t i = tid; i < slots; i += T) {
            if (cnt[i]) atomicAdd(&branch[i], (unsigned long long)cnt[i]);
            if (GENES && cnt2[i]) atomicAdd(&branch_loss[i], (unsigned long long)cnt2[i]);
        }
}
