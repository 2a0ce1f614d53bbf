// model_kernels.h -- the gfx950 kernel of the likelihood of a tree under F81 with a root distribution and rate categories
// (ps_tree_model_likelihood, include/pansim_hip.h; the definitions: docs/TREE_MODEL.md): every site's likelihood and posterior
// mean rate, their log sum and, DERIV, the three derivative sums of every branch, in one pass over the core matrix.
//
// The team, the tile loader, the level schedule, the class bytes and the missing-data rule are tree_lik_kernel's
// (likelihood_kernels.h): a workgroup -- a single wave for N <= 1024, 256 threads above -- owns four site rows, leaves one dword
// per LEAF in LDS and walks the four sites one after the other, an internal node being four f64 and one i32 of LDS.  What differs:
//   x        a table xs[K][n_pad + M] in global memory, one row per rate category (it stays in the vector cache as xs[] does);
//   site     an ASSIGNED site (site_class given, or K = 1) runs one up pass and, DERIV, one down pass with its class's row.  A
//            MIXTURE site runs K up passes that leave only the K root pairs (mantissa, exponent) in LDS; thread 0 -- the root's
//            lane -- forms the mixture, the posterior and the posterior mean rate from them (ps_subst_mix).  DERIV: for every k the
//            up pass again (the partials of class k were overwritten) and the down pass; the lane of a merge accumulates D_sc of
//            its two child branches over k in an LDS temporary and, after the last category, adds D to g and D D to h; q is added
//            per (site, category).  A branch is the child of one merge: one writer, no atomics;
//   sums     a workgroup's row of `part` is g, h, q of every slot, then its lnL; lik_reduce_kernel adds the rows in workgroup order.
// No floating-point atomics: the same grid on the same device gives the same bits.
#pragma once

#include "likelihood_kernels.h"
#include "subst_rule.h"

// pi, rho, the rates and the weights of the K categories: a kernel argument
struct model_args {
    double freq[4], root[4], rate[PS_MODEL_MAX_CATEGORIES], weight[PS_MODEL_MAX_CATEGORIES];
    uint32_t K;
};

#define PS_MODEL_LOAD(c, L, e)                                            \
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

// state .. n_pad, sched_lds, site_base, missing: as tree_lik_kernel takes them.  xs[K][n_pad + M]: x of the branch above every LDS
// slot in every category.  site_class[rows] (null: K = 1 or a mixture): the class of every site of this handle.  Dynamic LDS: n_pad
// leaf dwords; 4 Mp f64 and Mp i32 of the merges; DERIV: 4 (n_pad + M) f64 (g, h, q, the temporary); sched_lds: the schedule
// behind those.  Static LDS: 320 bytes of rates, weights, rho and the site's K pairs and posterior.  site_mant / site_exp / site_rate
// [site_base + row] (each may be null).  part: gridDim.x rows of `stride` f64 = g, h, q of every slot (DERIV only), lnL last.
template <bool DERIV>
__global__ void __launch_bounds__(256) tree_model_kernel(const uint8_t *state, uint32_t pitch, uint32_t N, uint32_t rows, const uint32_t *sched,
                                                         const uint32_t *level_off, uint32_t levels, uint32_t M, uint32_t n_pad, const double *xs,
                                                         uint32_t sched_lds, model_args a, const uint8_t *site_class, double *site_mant,
                                                         int32_t *site_exp, double *site_rate, uint32_t site_base, double *part, uint32_t stride,
                                                         unsigned long long *missing)
{
    extern __shared__ uint4 model_lds[];
    __shared__ double s_rate[PS_MODEL_MAX_CATEGORIES], s_w[PS_MODEL_MAX_CATEGORIES], s_mant[PS_MODEL_MAX_CATEGORIES], s_post[PS_MODEL_MAX_CATEGORIES];
    __shared__ double s_rho[4];
    __shared__ int32_t s_ex[PS_MODEL_MAX_CATEGORIES];
    uint32_t *leaf = (uint32_t *)model_lds;
    const uint32_t tid = threadIdx.x, T = blockDim.x, lane = tid & 63u;
    const uint32_t Mp = (M + 1u) & ~1u, slots = n_pad + M, K = a.K;
    double *P0 = (double *)(leaf + n_pad), *P1 = P0 + Mp, *P2 = P1 + Mp, *P3 = P2 + Mp;
    int32_t *E = (int32_t *)(P3 + Mp);
    double *G = (double *)(E + Mp), *H = G + slots, *Q = H + slots, *Tm = Q + slots;
    uint32_t *ls = (uint32_t *)(DERIV ? Tm + slots : G), *lo = ls + M;
    const double pi[4] = { a.freq[0], a.freq[1], a.freq[2], a.freq[3] };
    if (DERIV)
        for (uint32_t i = tid; i < 3u * slots; i += T) G[i] = 0.0;
#pragma unroll
    for (uint32_t i = 0; i < PS_MODEL_MAX_CATEGORIES; i++)
        if (tid == i) {
            s_rate[i] = a.rate[i];
            s_w[i] = a.weight[i];
            if (i < 4u) s_rho[i] = a.root[i];
        }
    if (sched_lds) {
        for (uint32_t i = tid; i < M; i += T) ls[i] = sched[i];
        for (uint32_t i = tid; i <= levels; i += T) lo[i] = level_off[i];
    }
    auto entry = [&](uint32_t j) { return sched_lds ? ls[j] : sched[j]; };
    auto level = [&](uint32_t l) { return sched_lds ? lo[l] : level_off[l]; };
    double lnl = 0.0;                             // (thread 0: the root is the only entry of the last level)
    uint32_t miss = 0u;
    const uint32_t ntiles = (rows + 3u) >> 2;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t live = min(4u, rows - tile * 4u);
        const uint32_t rowmask = live == 4u ? 0xFFFFFFFFu : (1u << (8u * live)) - 1u;
        __syncthreads();                          // (the last site of the tile before has been read; the first: s_rate and the schedule)
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
                const uint32_t a0 = r[0][q], b = r[1][q], c = r[2][q], d = r[3][q];
                const uint32_t t0 = (a0 & 0x00FF00FFu) | ((b & 0x00FF00FFu) << 8), t1 = ((a0 >> 8) & 0x00FF00FFu) | (b & 0xFF00FF00u);
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
            const uint32_t row = tile * 4u + k, site = site_base + row;
            // the up pass with the row xk of the table; the root's lane leaves the category's pair in s_mant / s_ex[pair]
            auto up = [&](const double *xk, uint32_t pair) {
                for (uint32_t lev = 0; lev < levels; lev++) {
                    const uint32_t hi = level(lev + 1u);
                    for (uint32_t j = level(lev) + tid; j < hi; j += T) {
                        const uint32_t e = entry(j);
                        const uint32_t cl = e & PS_PARS_SLOT, cr = (e >> 16) & PS_PARS_SLOT;
                        double Ll[4], Lr[4], ml[4], mr[4], L[4];
                        int32_t el, er;
                        PS_MODEL_LOAD(cl, Ll, el);
                        PS_MODEL_LOAD(cr, Lr, er);
                        ps_subst_up(xk[cl], pi, Ll, ml);
                        ps_subst_up(xk[cr], pi, Lr, mr);
                        const int32_t ex = (el + er) + ps_jc_join(ml, mr, L);
                        P0[j] = L[0];
                        P1[j] = L[1];
                        P2[j] = L[2];
                        P3[j] = L[3];
                        E[j] = ex;
                        if (e & PS_PARS_ROOT) {
                            s_mant[pair] = ps_subst_site(s_rho, L);
                            s_ex[pair] = ex;
                        }
                    }
                    __syncthreads();
                }
            };
            // the down pass of category kc with posterior `post`; first / last: of the categories of this site
            auto down = [&](const double *xk, uint32_t kc, double post, bool first, bool last) {
                const double rk = s_rate[kc];
                for (uint32_t lev = levels; lev-- > 0u;) {
                    const uint32_t hi = level(lev + 1u);
                    for (uint32_t j = level(lev) + tid; j < hi; j += T) {
                        const uint32_t e = entry(j);
                        const uint32_t cl = e & PS_PARS_SLOT, cr = (e >> 16) & PS_PARS_SLOT;
                        double Tv[4], Ll[4], Lr[4], ml[4], mr[4], Ua[4], Ub[4];
                        int32_t el, er;
                        if (e & PS_PARS_ROOT) {
                            Tv[0] = s_rho[0];
                            Tv[1] = s_rho[1];
                            Tv[2] = s_rho[2];
                            Tv[3] = s_rho[3];
                        } else {
                            const double U[4] = { P0[j], P1[j], P2[j], P3[j] };
                            ps_subst_down(xk[n_pad + j], pi, U, Tv);
                        }
                        PS_MODEL_LOAD(cl, Ll, el);
                        PS_MODEL_LOAD(cr, Lr, er);
                        const double xl = xk[cl], xr = xk[cr];
                        ps_subst_up(xl, pi, Ll, ml);
                        ps_subst_up(xr, pi, Lr, mr);
                        (void)ps_jc_join(mr, Tv, Ua);
                        (void)ps_jc_join(ml, Tv, Ub);
                        const double ra = ps_subst_ratio(xl, pi, Ua, Ll), rb = ps_subst_ratio(xr, pi, Ub, Lr);
                        Q[cl] += ps_subst_qterm(post, rk, xl, ra);
                        Q[cr] += ps_subst_qterm(post, rk, xr, rb);
                        const double ta = ps_subst_dterm(post, rk, xl, ra), tb = ps_subst_dterm(post, rk, xr, rb);
                        const double da = first ? ta : Tm[cl] + ta, db = first ? tb : Tm[cr] + tb;
                        if (last) {
                            G[cl] += da;
                            H[cl] += da * da;
                            G[cr] += db;
                            H[cr] += db * db;
                        } else {
                            Tm[cl] = da;
                            Tm[cr] = db;
                        }
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
            };
            // the categories of the site: its class's alone (assigned), or all K (a mixture)
            const bool assigned = site_class != nullptr || K == 1u;
            const uint32_t kb = assigned ? (site_class ? (uint32_t)site_class[row] : 0u) : 0u, ke = assigned ? kb + 1u : K;
            for (uint32_t kc = kb; kc < ke; kc++) up(xs + (size_t)kc * slots, kc);
            if (tid == 0u) {
                double mant, rate;
                int32_t ex;
                if (assigned) {
                    mant = s_mant[kb];
                    ex = s_ex[kb];
                    rate = s_rate[kb];
                    s_post[kb] = 1.0;
                } else {
                    mant = ps_subst_mix(K, s_w, s_mant, s_ex, &ex, s_post);
                    rate = ps_subst_mean_rate(K, s_post, s_rate);
                }
                if (site_mant) site_mant[site] = mant;
                if (site_exp) site_exp[site] = ex;
                if (site_rate) site_rate[site] = rate;
                lnl += ps_jc_site_ln(mant, ex);
            }
            if (DERIV) {
                __syncthreads();                  // (the posterior)
                for (uint32_t kc = kb; kc < ke; kc++) {
                    const double *xk = xs + (size_t)kc * slots;
                    if (!assigned) up(xk, kc);    // (the partials of class kc were overwritten; an assigned site's are still there)
                    down(xk, kc, s_post[kc], kc == kb, kc + 1u == ke);
                }
            }
        }
    }
    // the flush: the workgroup's own row, and one integer atomic per wave that met a missing cell
    __syncthreads();
    double *out = part + (size_t)blockIdx.x * stride;
    if (DERIV)
        for (uint32_t i = tid; i < 3u * slots; i += T) out[i] = G[i];
    if (tid == 0u) out[stride - 1u] = lnl;
#pragma unroll
    for (int o = 32; o; o >>= 1) miss += (uint32_t)__shfl_xor((int)miss, o, 64);
    if (lane == 0u && miss) atomicAdd(missing, (unsigned long long)miss);
}

#undef PS_MODEL_LOAD
