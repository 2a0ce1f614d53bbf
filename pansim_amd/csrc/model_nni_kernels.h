// model_nni_kernels.h -- the gfx950 kernels of the likelihood tree search (ps_tree_model_nni, include/pansim_hip.h; the
// definitions: docs/LIKELIHOOD_SEARCH.md): lnL of a tree under F81 with a root distribution and rate categories and the exact ratio
// of the likelihood of every nearest-neighbour interchange to it, in one pass over the core matrix.  The likelihood twin of
// tree_nni_kernel (nni_kernels.h).
//
// The team, the tile loader, the level schedule, the class bytes, the missing-data rule and the table xs[K][n_pad + M] are
// tree_model_kernel<true>'s (model_kernels.h); there are no g / h / q sums.  What differs is the down pass.  The likelihood of a
// neighbour tree around the edge v - c, c = (a, b) with sibling s, is a function of four pieces -- the messages m^a, m^b, m^s and
// T(v), the message into v from above -- and the lane of c has the first two from its own children.  The other two come the way
// tree_nni_kernel hands (U(v), S(s)): the PARENT's lane, which forms T(v) and the messages of both its children anyway, leaves the
// pair (T(v), m^s) of eight f64 for every internal child.  So the inside partials are never overwritten (tree_model_kernel writes
// the outside partial over them), and a lane's level costs two dependent LDS trips: its schedule entry, then its pair, the
// partials of its two children and its accumulators side by side.  The alternative -- the lane reads its sibling's partial itself
// -- saves 28 bytes per merge and needs the parent's and the sibling's position of every merge in the schedule, a third kind of
// entry the schedule does not have.  The root's lane evaluates the quartet of its two children (three trips: its entry, the
// children's entries, the four grandchildren) and counts it on the left one; the root's children are marked PS_NNI_BELOW_ROOT and
// have no interchange of their own.
//
// The lane of c forms l0, l1, l2 (ps_subst_nni_edge) for the site and category, adds post_k l_kind / l0 over the categories of a
// mixture in an LDS temporary and, after the last category, multiplies the site's two ratios into its own two (mantissa,
// exponent) accumulators (ps_subst_prod): one writer per candidate, no atomics, no log.  A site whose likelihood is 0 in this tree
// takes part in no product and is counted.  At the end a workgroup writes its accumulators and its lnL to its own row of the
// scratch; model_nni_reduce_kernel multiplies the rows in workgroup order.  The same grid on the same device gives the same bits.
//
// Dynamic LDS: 4 n_pad + 140 Mp bytes, Mp = M rounded up to even: the leaf dwords; per merge 32 bytes of inside partial, 64 of the
// pair, 16 of the two mantissas, 16 of the mixture's temporary, 4 of the partial's exponent and 8 of the two exponents; behind
// them the schedule's copy of 4 (M + levels + 1) bytes while the whole stays within PS_LIK_LDS_SCHED.  N = 1024: 147 456 bytes and
// at most 8 188 of schedule; N = 1280 would need 184 320: PS_MODEL_NNI_MAX_POP = 1024, the team a single wave.
#pragma once

#include "model_kernels.h"
#include "nni_kernels.h"

#define PS_MNNI_LOAD(c, L, e)                                             \
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

// state .. missing: as tree_model_kernel takes them, the entries of the root's internal children marked PS_NNI_BELOW_ROOT.
// part_mant / part_exp: gridDim.x rows of 2 M values, [2 j + kind] of the merge at schedule position j (the empty product where it
// has no candidate); part_lnl: gridDim.x values.  counts[0] += the missing cells, counts[1] += the sites of likelihood 0.
__global__ void __launch_bounds__(256) tree_model_nni_kernel(const uint8_t *state, uint32_t pitch, uint32_t N, uint32_t rows, const uint32_t *sched,
                                                             const uint32_t *level_off, uint32_t levels, uint32_t M, uint32_t n_pad, const double *xs,
                                                             uint32_t sched_lds, model_args a, const uint8_t *site_class, double *part_mant,
                                                             int32_t *part_exp, double *part_lnl, unsigned long long *counts)
{
    extern __shared__ uint4 mnni_lds[];
    __shared__ double s_rate[PS_MODEL_MAX_CATEGORIES], s_w[PS_MODEL_MAX_CATEGORIES], s_mant[PS_MODEL_MAX_CATEGORIES], s_post[PS_MODEL_MAX_CATEGORIES];
    __shared__ double s_rho[4];
    __shared__ int32_t s_ex[PS_MODEL_MAX_CATEGORIES];
    __shared__ uint32_t s_zero;
    uint32_t *leaf = (uint32_t *)mnni_lds;
    const uint32_t tid = threadIdx.x, T = blockDim.x, lane = tid & 63u;
    const uint32_t Mp = (M + 1u) & ~1u, slots = n_pad + M, K = a.K;
    double *P0 = (double *)(leaf + n_pad), *P1 = P0 + Mp, *P2 = P1 + Mp, *P3 = P2 + Mp;
    double *TQ = P3 + Mp;                         // the pair of merge i: T(parent) in TQ[q Mp + i], m^sibling in TQ[(4 + q) Mp + i]
    double *A0 = TQ + 8u * Mp, *A1 = A0 + Mp;     // the mantissas of the two products of merge i
    double *R0 = A1 + Mp, *R1 = R0 + Mp;          // the temporary of a mixture site
    int32_t *E = (int32_t *)(R1 + Mp), *X0 = E + Mp, *X1 = X0 + Mp;
    uint32_t *ls = (uint32_t *)(X1 + Mp), *lo = ls + M;
    const double pi[4] = { a.freq[0], a.freq[1], a.freq[2], a.freq[3] };
    for (uint32_t i = tid; i < Mp; i += T) {
        A0[i] = A1[i] = 0.5;                      // (1/2, 1): the empty product
        X0[i] = X1[i] = 1;
    }
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
    uint32_t miss = 0u, zero = 0u;
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
            const uint32_t row = tile * 4u + k;
            // the up pass with the row xk of the table; the root's lane leaves the category's pair in s_mant / s_ex[pair]
            auto up = [&](const double *xk, uint32_t pair) {
                for (uint32_t lev = 0; lev < levels; lev++) {
                    const uint32_t hi = level(lev + 1u);
                    for (uint32_t j = level(lev) + tid; j < hi; j += T) {
                        const uint32_t e = entry(j);
                        const uint32_t cl = e & PS_PARS_SLOT, cr = (e >> 16) & PS_PARS_SLOT;
                        double Ll[4], Lr[4], ml[4], mr[4], L[4];
                        int32_t el, er;
                        PS_MNNI_LOAD(cl, Ll, el);
                        PS_MNNI_LOAD(cr, Lr, er);
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
            // the site's ratios of candidate position i after category kc: summed over the categories, multiplied in after the last
            auto count = [&](uint32_t i, const double l[3], double post, bool first, bool last) {
                const double t0 = ps_subst_nni_term(post, l[1], l[0]), t1 = ps_subst_nni_term(post, l[2], l[0]);
                const double r0 = first ? t0 : R0[i] + t0, r1 = first ? t1 : R1[i] + t1;
                if (last) {
                    int32_t k0, k1;
                    A0[i] = ps_subst_prod(A0[i], r0, &k0);
                    A1[i] = ps_subst_prod(A1[i], r1, &k1);
                    X0[i] += k0;
                    X1[i] += k1;
                } else {
                    R0[i] = r0;
                    R1[i] = r1;
                }
            };
            // the down pass of category kc with posterior `post`; first / last: of the categories of this site
            auto down = [&](const double *xk, double post, bool first, bool last) {
                for (uint32_t lev = levels; lev-- > 0u;) {
                    const uint32_t hi = level(lev + 1u);
                    for (uint32_t j = level(lev) + tid; j < hi; j += T) {
                        const uint32_t e = entry(j);
                        const uint32_t cl = e & PS_PARS_SLOT, cr = (e >> 16) & PS_PARS_SLOT;
                        double Tv[4], Ll[4], Lr[4], ml[4], mr[4], l[3];
                        int32_t el, er;
                        PS_MNNI_LOAD(cl, Ll, el);
                        PS_MNNI_LOAD(cr, Lr, er);
                        ps_subst_up(xk[cl], pi, Ll, ml);
                        ps_subst_up(xk[cr], pi, Lr, mr);
                        if (e & PS_PARS_ROOT) {
                            Tv[0] = s_rho[0];
                            Tv[1] = s_rho[1];
                            Tv[2] = s_rho[2];
                            Tv[3] = s_rho[3];
                            // the root's edge: the quartet of its two children, counted on the left one
                            if (cl >= n_pad && cr >= n_pad) {
                                const uint32_t ec = entry(cl - n_pad), es = entry(cr - n_pad);
                                const uint32_t ca = ec & PS_PARS_SLOT, cb = (ec >> 16) & PS_PARS_SLOT, cp = es & PS_PARS_SLOT, cq = (es >> 16) & PS_PARS_SLOT;
                                double La[4], ma[4], mb[4], mp[4], mq[4];
                                int32_t ea;
                                PS_MNNI_LOAD(ca, La, ea);
                                ps_subst_up(xk[ca], pi, La, ma);
                                PS_MNNI_LOAD(cb, La, ea);
                                ps_subst_up(xk[cb], pi, La, mb);
                                PS_MNNI_LOAD(cp, La, ea);
                                ps_subst_up(xk[cp], pi, La, mp);
                                PS_MNNI_LOAD(cq, La, ea);
                                ps_subst_up(xk[cq], pi, La, mq);
                                (void)ea;
                                ps_subst_nni_root_edge(xk[cl], xk[cr], pi, s_rho, ma, mb, mp, mq, l);
                                count(cl - n_pad, l, post, first, last);
                            }
                        } else {
                            const double Tp[4] = { TQ[j], TQ[Mp + j], TQ[2u * Mp + j], TQ[3u * Mp + j] };
                            const double ms[4] = { TQ[4u * Mp + j], TQ[5u * Mp + j], TQ[6u * Mp + j], TQ[7u * Mp + j] };
                            const double xc = xk[n_pad + j];
                            if (!(e & PS_NNI_BELOW_ROOT)) {
                                ps_subst_nni_edge(xc, pi, ml, mr, ms, Tp, l);
                                count(j, l, post, first, last);
                            }
                            double U[4];
                            (void)ps_jc_join(ms, Tp, U);
                            ps_subst_down(xc, pi, U, Tv);
                        }
                        if (cl >= n_pad) {
                            const uint32_t i = cl - n_pad;
#pragma unroll
                            for (uint32_t q = 0; q < 4u; q++) {
                                TQ[q * Mp + i] = Tv[q];
                                TQ[(4u + q) * Mp + i] = mr[q];
                            }
                        }
                        if (cr >= n_pad) {
                            const uint32_t i = cr - n_pad;
#pragma unroll
                            for (uint32_t q = 0; q < 4u; q++) {
                                TQ[q * Mp + i] = Tv[q];
                                TQ[(4u + q) * Mp + i] = ml[q];
                            }
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
                double mant;
                int32_t ex;
                if (assigned) {
                    mant = s_mant[kb];
                    ex = s_ex[kb];
                    s_post[kb] = 1.0;
                } else
                    mant = ps_subst_mix(K, s_w, s_mant, s_ex, &ex, s_post);
                lnl += ps_jc_site_ln(mant, ex);
                s_zero = mant > 0.0 ? 0u : 1u;
                zero += mant > 0.0 ? 0u : 1u;
            }
            __syncthreads();                      // (the posterior and s_zero)
            if (s_zero == 0u)                     // (team-uniform; the barrier of the next up pass or tile orders the next write of s_zero)
                for (uint32_t kc = kb; kc < ke; kc++) {
                    const double *xk = xs + (size_t)kc * slots;
                    if (!assigned) up(xk, kc);    // (the partials of class kc were overwritten; an assigned site's are still there)
                    down(xk, s_post[kc], kc == kb, kc + 1u == ke);
                }
        }
    }
    // the flush: the workgroup's own rows, and one integer atomic per wave that met a missing cell
    __syncthreads();
    double *om = part_mant + (size_t)blockIdx.x * 2u * M;
    int32_t *oe = part_exp + (size_t)blockIdx.x * 2u * M;
    for (uint32_t i = tid; i < M; i += T) {
        om[2u * i] = A0[i];
        om[2u * i + 1u] = A1[i];
        oe[2u * i] = X0[i];
        oe[2u * i + 1u] = X1[i];
    }
    if (tid == 0u) {
        part_lnl[blockIdx.x] = lnl;
        if (zero) atomicAdd(&counts[1], (unsigned long long)zero);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) miss += (uint32_t)__shfl_xor((int)miss, o, 64);
    if (lane == 0u && miss) atomicAdd(&counts[0], (unsigned long long)miss);
}

#undef PS_MNNI_LOAD

// The products of the workgroups' rows in workgroup order, exponents in i64: out_mant / out_exp[i], i < n; thread 0 adds the rows'
// lnL in the same order
__global__ void __launch_bounds__(256) model_nni_reduce_kernel(const double *part_mant, const int32_t *part_exp, const double *part_lnl, uint32_t nrows,
                                                               uint32_t n, double *out_mant, long long *out_exp, double *out_lnl)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0u) {
        double s = 0.0;
        for (uint32_t w = 0; w < nrows; w++) s += part_lnl[w];
        *out_lnl = s;
    }
    if (i >= n) return;
    double m = 0.5;
    long long e = 1;
    for (uint32_t w = 0; w < nrows; w++) {
        int32_t k;
        m = ps_subst_prod(m, part_mant[(size_t)w * n + i], &k);
        e += (long long)k + (long long)part_exp[(size_t)w * n + i];
    }
    out_mant[i] = m;
    out_exp[i] = e;
}
