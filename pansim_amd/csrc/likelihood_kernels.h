// likelihood_kernels.h -- the gfx950 kernels of the Jukes-Cantor likelihood of a tree (ps_tree_likelihood, include/pansim_hip.h;
// the definitions: docs/TREE_LIKELIHOOD.md): every site's likelihood, their log sum and, DERIV, the two derivative sums of every
// branch, in one pass over the core matrix.
//
// The team, the tile and the schedule are tree_fitch_kernel's (parsimony_kernels.h): a workgroup -- a single wave for N <= 1024,
// 256 threads above -- owns four site rows, loads them with ps_load_row16, maps the bytes to class bytes and leaves one dword per
// LEAF in LDS with the four sites in its bytes.  The four sites are then walked one after the other: an internal node has four
// f64 and one i32 in LDS (its partial L, rescaled, and its binary exponent; structure of arrays, so a level's lanes write
// neighbouring words), a leaf's partial is formed from its byte on the fly.  The up pass walks the levels, a lane per merge: the
// partials of its two children, their messages along the two branches (x = exp(-4 t / 3) per branch comes from the host: no
// transcendental function here), the product, frexp / ldexp.  The root's lane -- thread 0 of the last level -- stores the site's
// (mantissa, exponent) and adds its logarithm to the workgroup's lnL.  DERIV: the down pass walks the levels back; the lane of
// merge c = (a, b) holds U(c), the outside partial at the top of its branch (the root: the message from above is all ones),
// forms T(c), U(a) and U(b), finishes r and r r of both child branches, adds them to the LDS sums of the two branches (a branch is
// the child of one merge: one writer, no atomics) and writes U over L of its internal children -- the parent has read L of both
// its children by then, and a lane needs only its own children's L.  A barrier separates the levels.
//
// Sums in floating point do not commute, so nothing is added atomically: a workgroup walks its tiles (blockIdx.x, + gridDim.x,
// ...) and their sites in order and writes its sums to its own row of `part`; lik_reduce_kernel adds the rows in workgroup order.
// The same grid on the same device gives the same bits.  The count of missing cells is an integer.
#pragma once

#include "jc_rule.h"
#include "parsimony_kernels.h"

// the partial of the node in LDS slot c for site k of the tile: a leaf's from its class byte, an internal node's from its words
#define PS_LIK_LOAD(c, L, e)                                              \
    do {                                                                  \
        if ((c) < n_pad) {                                                \
            ps_jc_leaf((leaf[(c)] >> (8u * k)) & 0xFFu, (L));             \
            (e) = 0;                                                      \
        } else {                                                          \
            const uint32_t i_ = (c) - n_pad;                              \
            (L)[0] = P0[i_];                                              \
            (L)[1] = P1[i_];                                              \
            (L)[2] = P2[i_];                                              \
            (L)[3] = P3[i_];                                              \
            (e) = E[i_];                                                  \
        }                                                                 \
    } while (0)

// state, pitch, N, rows, sched, level_off, levels, M, n_pad: as tree_fitch_kernel takes them, of a SPANNING tree (M = N - 1, one
// root: the only entry of the last level).  xs[n_pad + M]: x of the branch above every LDS slot (the root's and the pad's are
// never read).  Dynamic LDS: n_pad leaf dwords; 4 Mp f64 and Mp i32 of the merges (Mp = M rounded up to even); DERIV: 2 (n_pad +
// M) f64 of sums; sched_lds: M + levels + 1 dwords of schedule behind those.  site_mant / site_exp[site_base
// + row] (either may be null).  part: gridDim.x rows of `stride` f64, a workgroup's row = g of every slot, then h of every slot
// (DERIV only), then its lnL last.  missing (zeroed by the caller): the cells that are none of 1 / 2 / 4 / 8.  Any grid is valid:
// workgroups stride over the tiles.
template <bool DERIV>
__global__ void __launch_bounds__(256) tree_lik_kernel(const uint8_t *state, uint32_t pitch, uint32_t N, uint32_t rows, const uint32_t *sched,
                                                       const uint32_t *level_off, uint32_t levels, uint32_t M, uint32_t n_pad, const double *xs,
                                                       uint32_t sched_lds, double *site_mant, int32_t *site_exp, uint32_t site_base,
                                                       double *part, uint32_t stride, unsigned long long *missing)
{
    extern __shared__ uint4 lik_lds[];            // (16-byte aligned: the leaves are stored four nodes at a time)
    uint32_t *leaf = (uint32_t *)lik_lds;
    const uint32_t tid = threadIdx.x, T = blockDim.x, lane = tid & 63u;
    const uint32_t Mp = (M + 1u) & ~1u, slots = n_pad + M;
    double *P0 = (double *)(leaf + n_pad), *P1 = P0 + Mp, *P2 = P1 + Mp, *P3 = P2 + Mp;
    int32_t *E = (int32_t *)(P3 + Mp);
    double *G = (double *)(E + Mp), *H = G + slots;
    uint32_t *ls = (uint32_t *)(DERIV ? H + slots : G), *lo = ls + M;
    if (DERIV)
        for (uint32_t i = tid; i < 2u * slots; i += T) G[i] = 0.0;
    // the schedule where the levels read it: its LDS copy (made here; the first tile's barrier orders it) or global memory.  x stays
    // in global memory: its 8 bytes per slot are read by every site alike and live in the vector cache, while the same bytes of
    // LDS cost a workgroup per CU (measured: profiles/tree_likelihood.md)
    if (sched_lds) {
        for (uint32_t i = tid; i < M; i += T) ls[i] = sched[i];
        for (uint32_t i = tid; i <= levels; i += T) lo[i] = level_off[i];
    }
    auto entry = [&](uint32_t j) { return sched_lds ? ls[j] : sched[j]; };
    auto level = [&](uint32_t l) { return sched_lds ? lo[l] : level_off[l]; };
    auto xof = [&](uint32_t c) { return xs[c]; };
    double lnl = 0.0;                             // (thread 0: the root is the only entry of the last level)
    uint32_t miss = 0u;
    const uint32_t ntiles = (rows + 3u) >> 2;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t live = min(4u, rows - tile * 4u);
        const uint32_t rowmask = live == 4u ? 0xFFFFFFFFu : (1u << (8u * live)) - 1u;
        __syncthreads();                          // (the last site of the tile before has been read)
        // the leaves: 16 cells of each of the four rows per thread and trip, transposed to one dword per leaf
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
            const bool exact = __any(bad != 0u);
            if (exact) {
                // a byte that is not 1 / 2 / 4 / 8 somewhere in the wave's piece: the exact map (such a byte becomes 0x10)
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
            if (exact) {
#pragma unroll
                for (uint32_t i = 0; i < 16u; i++)
                    if (base + i < N) miss += (uint32_t)__popc(w[i] & 0x10101010u & rowmask);
            }
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++)
                *(uint4 *)(leaf + base + 4u * q) = make_uint4(w[4u * q], w[4u * q + 1u], w[4u * q + 2u], w[4u * q + 3u]);
        }
        __syncthreads();
        for (uint32_t k = 0; k < live; k++) {
            const uint32_t site = site_base + tile * 4u + k;
            for (uint32_t lev = 0; lev < levels; lev++) {
                const uint32_t hi = level(lev + 1u);
                for (uint32_t j = level(lev) + tid; j < hi; j += T) {
                    const uint32_t e = entry(j);
                    const uint32_t cl = e & PS_PARS_SLOT, cr = (e >> 16) & PS_PARS_SLOT;
                    double Ll[4], Lr[4], ml[4], mr[4], L[4];
                    int32_t el, er;
                    PS_LIK_LOAD(cl, Ll, el);
                    PS_LIK_LOAD(cr, Lr, er);
                    ps_jc_message(xof(cl), Ll, ml);
                    ps_jc_message(xof(cr), Lr, mr);
                    const int32_t ex = (el + er) + ps_jc_join(ml, mr, L);
                    P0[j] = L[0];
                    P1[j] = L[1];
                    P2[j] = L[2];
                    P3[j] = L[3];
                    E[j] = ex;
                    if (e & PS_PARS_ROOT) {
                        const double mant = ps_jc_site(L);
                        if (site_mant) site_mant[site] = mant;
                        if (site_exp) site_exp[site] = ex;
                        lnl += ps_jc_site_ln(mant, ex);
                    }
                }
                __syncthreads();
            }
            if (DERIV) {
                for (uint32_t lev = levels; lev-- > 0u;) {
                    const uint32_t hi = level(lev + 1u);
                    for (uint32_t j = level(lev) + tid; j < hi; j += T) {
                        const uint32_t e = entry(j);
                        const uint32_t cl = e & PS_PARS_SLOT, cr = (e >> 16) & PS_PARS_SLOT;
                        double Tv[4], Ll[4], Lr[4], ml[4], mr[4], Ua[4], Ub[4];
                        int32_t el, er;
                        if (e & PS_PARS_ROOT) {
                            Tv[0] = Tv[1] = Tv[2] = Tv[3] = 1.0;
                        } else {
                            const double U[4] = { P0[j], P1[j], P2[j], P3[j] };
                            ps_jc_message(xof(n_pad + j), U, Tv);
                        }
                        PS_LIK_LOAD(cl, Ll, el);
                        PS_LIK_LOAD(cr, Lr, er);
                        const double xl = xof(cl), xr = xof(cr);
                        ps_jc_message(xl, Ll, ml);
                        ps_jc_message(xr, Lr, mr);
                        (void)ps_jc_join(mr, Tv, Ua);
                        (void)ps_jc_join(ml, Tv, Ub);
                        const double ra = ps_jc_ratio(xl, Ua, Ll), rb = ps_jc_ratio(xr, Ub, Lr);
                        G[cl] += ra;
                        H[cl] += ra * ra;
                        G[cr] += rb;
                        H[cr] += rb * rb;
                        if (cl >= n_pad) {
                            const uint32_t i = cl - n_pad;
                            P0[i] = Ua[0];
                            P1[i] = Ua[1];
                            P2[i] = Ua[2];
                            P3[i] = Ua[3];
                        }
                        if (cr >= n_pad) {
                            const uint32_t i = cr - n_pad;
                            P0[i] = Ub[0];
                            P1[i] = Ub[1];
                            P2[i] = Ub[2];
                            P3[i] = Ub[3];
                        }
                        (void)el;
                        (void)er;
                    }
                    __syncthreads();
                }
            }
        }
    }
    // the flush: the workgroup's own row, and one integer atomic per wave that met a missing cell
    __syncthreads();
    double *row = part + (size_t)blockIdx.x * stride;
    if (DERIV)
        for (uint32_t i = tid; i < 2u * slots; i += T) row[i] = G[i];
    if (tid == 0u) row[stride - 1u] = lnl;
#pragma unroll
    for (int o = 32; o; o >>= 1) miss += (uint32_t)__shfl_xor((int)miss, o, 64);
    if (lane == 0u && miss) atomicAdd(missing, (unsigned long long)miss);
}

#undef PS_LIK_LOAD

// out[i] = the sum of part[w stride + i] over the workgroups w = 0 .. nrows - 1, in that order; i < stride
__global__ void __launch_bounds__(256) lik_reduce_kernel(const double *part, uint32_t nrows, uint32_t stride, double *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= stride) return;
    double s = 0.0;
    for (uint32_t w = 0; w < nrows; w++) s += part[(size_t)w * stride + i];
    out[i] = s;
}
