// anc_kernels.h -- the gfx950 kernel of the marginal ancestral states of a tree under F81 with a root distribution and rate
// categories (ps_tree_ancestral_states, include/pansim_hip.h; the definitions: docs/ANCESTRAL_STATES.md): every inner node's
// most probable state at every site as a one-hot byte of a NEW site-major matrix, the nodes' summed confidences, the branches'
// summed probabilities of a difference between their two ends, and lnL, in one pass over the core matrix.
//
// The team, the four-site tile loader with its transposed leaf dwords, the level schedule, the class bytes, the missing-data rule,
// the table xs[K][n_pad + M] and model_args are tree_model_kernel's (model_kernels.h); so are the up pass and the messages of the
// down pass.  What differs: no g / h / q sums.  In the down pass the lane of merge j holds Tv (the message into node j from above,
// rho at the root) and ml, mr (its children's messages): their product, normalised, is the node's posterior in the category
// (ps_subst_node_post), and the two children's outside partials give pdiff of the two child branches (ps_subst_pdiff).  An assigned
// site uses them as they are; a mixture site accumulates post_k p_{k,a} over k in an LDS temporary and adds post_k pdiff_k per
// (site, category).  After a site's last category the lane takes the arg max (ps_subst_map), adds pmax to its node's confidence and
// ORs the one-hot byte into byte `site of the tile` of the node's output dword -- the leaf dword's layout.  A node and a branch have
// one writer each: no atomics on floating point.
//
// After the four sites of a tile the workgroup transposes the output dwords back into four site rows of the new matrix (the inverse
// of the loader's transpose) and writes them with 16-byte stores over the whole pitch, the pad as zeros.
//
// Dynamic LDS, in this order: n_pad leaf dwords; 4 Mp f64 of partials; slots f64 of branch_diff; M f64 of node_conf; MIX only:
// 4 M f64 of the posterior accumulated over the categories; Mp i32 of exponents; M output dwords; sched_lds: the schedule and
// node_of behind those.  Assigned (site_class given, or K = 1): 12 n_pad + 56 M bytes (+ 36 when M is odd); a mixture: 32 M more.
#pragma once

#include "model_kernels.h"

// the largest multiples of 256 whose layout above fits the CU's 160 KiB beside the 336 bytes of static LDS:
// 68 N - 20 <= 163 504 -> 2304 (156 652 bytes), 100 N - 52 <= 163 504 -> 1536 (153 548 bytes)
#define PS_ANC_KERNEL_MAX_POP 2304u
#define PS_ANC_KERNEL_MAX_POP_MIX 1536u

#define PS_ANC_LOAD(c, L, e)                                              \
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

// state .. site_class: as tree_model_kernel takes them.  node_of[M]: the merge (row of the new matrix) of every schedule entry.
// min_post: a cell whose pmax is below it is written 0 and counted in counts[1].  out (null: no matrix is stored): the new matrix,
// `rows` site rows of pitch_out bytes (a multiple of 16), row `row` at out + row pitch_out.  part: gridDim.x rows of `stride` f64
// = branch_diff of every slot, node_conf of every schedule entry, lnL last.  counts: missing cells, masked cells, zero sites.
template <bool MIX>
__global__ void __launch_bounds__(256) tree_anc_kernel(const uint8_t *state, uint32_t pitch, uint32_t N, uint32_t rows, const uint32_t *sched,
                                                       const uint32_t *level_off, uint32_t levels, uint32_t M, uint32_t n_pad, const double *xs,
                                                       uint32_t sched_lds, model_args a, const uint8_t *site_class, const uint32_t *node_of,
                                                       double min_post, uint8_t *out, uint32_t pitch_out, double *part, uint32_t stride,
                                                       unsigned long long *counts)
{
    extern __shared__ uint4 anc_lds[];
    __shared__ double s_rate[PS_MODEL_MAX_CATEGORIES], s_w[PS_MODEL_MAX_CATEGORIES], s_mant[PS_MODEL_MAX_CATEGORIES], s_post[PS_MODEL_MAX_CATEGORIES];
    __shared__ double s_rho[4];
    __shared__ int32_t s_ex[PS_MODEL_MAX_CATEGORIES];
    __shared__ uint32_t s_zero;
    uint32_t *leaf = (uint32_t *)anc_lds;
    const uint32_t tid = threadIdx.x, T = blockDim.x, lane = tid & 63u;
    const uint32_t Mp = (M + 1u) & ~1u, slots = n_pad + M, K = a.K;
    double *P0 = (double *)(leaf + n_pad), *P1 = P0 + Mp, *P2 = P1 + Mp, *P3 = P2 + Mp;
    double *BD = P3 + Mp, *NC = BD + slots;
    double *Q0 = NC + M, *Q1 = Q0 + M, *Q2 = Q1 + M, *Q3 = Q2 + M;             // (MIX only: the assigned form has no such region)
    int32_t *E = (int32_t *)(MIX ? Q3 + M : NC + M);
    uint32_t *OW = (uint32_t *)(E + Mp);
    uint32_t *ls = OW + M, *ln = ls + M, *lo = ln + M;
    const double pi[4] = { a.freq[0], a.freq[1], a.freq[2], a.freq[3] };
    for (uint32_t i = tid; i < slots + M; i += T) BD[i] = 0.0;
#pragma unroll
    for (uint32_t i = 0; i < PS_MODEL_MAX_CATEGORIES; i++)
        if (tid == i) {
            s_rate[i] = a.rate[i];
            s_w[i] = a.weight[i];
            if (i < 4u) s_rho[i] = a.root[i];
        }
    if (sched_lds) {
        for (uint32_t i = tid; i < M; i += T) {
            ls[i] = sched[i];
            ln[i] = node_of[i];
        }
        for (uint32_t i = tid; i <= levels; i += T) lo[i] = level_off[i];
    }
    auto entry = [&](uint32_t j) { return sched_lds ? ls[j] : sched[j]; };
    auto level = [&](uint32_t l) { return sched_lds ? lo[l] : level_off[l]; };
    auto merge_of = [&](uint32_t j) { return sched_lds ? ln[j] : node_of[j]; };
    double lnl = 0.0;                             // (thread 0: the root is the only entry of the last level)
    uint32_t miss = 0u, masked = 0u, zero = 0u;
    const uint32_t ntiles = (rows + 3u) >> 2;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t live = min(4u, rows - tile * 4u);
        const uint32_t rowmask = live == 4u ? 0xFFFFFFFFu : (1u << (8u * live)) - 1u;
        __syncthreads();                          // (the tile before has been stored; the first: s_rate and the schedule)
        for (uint32_t i = tid; i < M; i += T) OW[i] = 0u;
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
                        PS_ANC_LOAD(cl, Ll, el);
                        PS_ANC_LOAD(cr, Lr, er);
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
            auto down = [&](const double *xk, double post, bool first, bool last) {
                for (uint32_t lev = levels; lev-- > 0u;) {
                    const uint32_t hi = level(lev + 1u);
                    for (uint32_t j = level(lev) + tid; j < hi; j += T) {
                        const uint32_t e = entry(j);
                        const uint32_t cl = e & PS_PARS_SLOT, cr = (e >> 16) & PS_PARS_SLOT;
                        double Tv[4], Ll[4], Lr[4], ml[4], mr[4], Ua[4], Ub[4], w[4], p[4];
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
                        PS_ANC_LOAD(cl, Ll, el);
                        PS_ANC_LOAD(cr, Lr, er);
                        const double xl = xk[cl], xr = xk[cr];
                        ps_subst_up(xl, pi, Ll, ml);
                        ps_subst_up(xr, pi, Lr, mr);
                        const double sum = ps_subst_node_post(Tv, ml, mr, w);
                        (void)ps_jc_join(mr, Tv, Ua);
                        (void)ps_jc_join(ml, Tv, Ub);
                        BD[cl] += post * ps_subst_pdiff(xl, pi, Ua, Ll);
                        BD[cr] += post * ps_subst_pdiff(xr, pi, Ub, Lr);
                        p[0] = ps_subst_post_term(post, w[0], sum);
                        p[1] = ps_subst_post_term(post, w[1], sum);
                        p[2] = ps_subst_post_term(post, w[2], sum);
                        p[3] = ps_subst_post_term(post, w[3], sum);
                        if (MIX && !first) {
                            p[0] = Q0[j] + p[0];
                            p[1] = Q1[j] + p[1];
                            p[2] = Q2[j] + p[2];
                            p[3] = Q3[j] + p[3];
                        }
                        if (!MIX || last) {
                            double pmax;
                            const uint32_t best = ps_subst_map(p, &pmax);
                            NC[j] += pmax;
                            if (pmax < min_post) masked++;
                            else OW[merge_of(j)] |= (1u << best) << (8u * k);
                        } else {
                            Q0[j] = p[0];
                            Q1[j] = p[1];
                            Q2[j] = p[2];
                            Q3[j] = p[3];
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
            const uint32_t kb = MIX ? 0u : (site_class ? (uint32_t)site_class[row] : 0u), ke = MIX ? K : kb + 1u;
            for (uint32_t kc = kb; kc < ke; kc++) up(xs + (size_t)kc * slots, kc);
            if (tid == 0u) {
                double mant;
                int32_t ex;
                if (!MIX) {
                    mant = s_mant[kb];
                    ex = s_ex[kb];
                    s_post[kb] = 1.0;
                } else
                    mant = ps_subst_mix(K, s_w, s_mant, s_ex, &ex, s_post);
                lnl += ps_jc_site_ln(mant, ex);
                s_zero = mant > 0.0 ? 0u : 1u;
                zero += mant > 0.0 ? 0u : 1u;
            }
            __syncthreads();                      // (the posterior, and whether the site has a likelihood at all)
            if (s_zero) continue;                 // (a site of likelihood 0: byte 0 at every node, nothing added)
            for (uint32_t kc = kb; kc < ke; kc++) {
                const double *xk = xs + (size_t)kc * slots;
                if (MIX) up(xk, kc);              // (the partials of class kc were overwritten; an assigned site's are still there)
                down(xk, s_post[kc], kc == kb, kc + 1u == ke);
            }
        }
        // the store: the inverse of the loader's transpose, 16 nodes of each of the four rows per thread and trip
        if (out) {
            __syncthreads();
            for (uint32_t base = tid * 16u; base < pitch_out; base += T * 16u) {
                uint32_t w[16];
#pragma unroll
                for (uint32_t i = 0; i < 16u; i++) w[i] = base + i < M ? OW[base + i] : 0u;
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++) {
                    const uint32_t row = tile * 4u + k;
                    uint32_t r[4];
#pragma unroll
                    for (uint32_t q = 0; q < 4u; q++)
                        r[q] = ((w[4u * q] >> (8u * k)) & 0xFFu) | (((w[4u * q + 1u] >> (8u * k)) & 0xFFu) << 8) |
                               (((w[4u * q + 2u] >> (8u * k)) & 0xFFu) << 16) | (((w[4u * q + 3u] >> (8u * k)) & 0xFFu) << 24);
                    if (row < rows) *(uint4 *)(out + (size_t)row * pitch_out + base) = make_uint4(r[0], r[1], r[2], r[3]);
                }
            }
        }
    }
    // the flush: the workgroup's own row, and one integer atomic per wave and counter that is not 0
    __syncthreads();
    double *prow = part + (size_t)blockIdx.x * stride;
    for (uint32_t i = tid; i < slots + M; i += T) prow[i] = BD[i];
    if (tid == 0u) prow[stride - 1u] = lnl;
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        miss += (uint32_t)__shfl_xor((int)miss, o, 64);
        masked += (uint32_t)__shfl_xor((int)masked, o, 64);
    }
    if (lane == 0u && miss) atomicAdd(counts, (unsigned long long)miss);
    if (lane == 0u && masked) atomicAdd(counts + 1, (unsigned long long)masked);
    if (tid == 0u && zero) atomicAdd(counts + 2, (unsigned long long)zero);
}

#undef PS_ANC_LOAD
