// gene_kernels.h -- the gfx950 kernels of the gain / loss model of the accessory genes on a tree (ps_tree_gene_likelihood,
// ps_tree_gene_ancestral, ps_tree_gene_fit, include/pansim_hip.h; the definitions: docs/GENE_MODEL.md).
//
// tree_gene_kernel<MIX, DOWN>: every gene's likelihood (and, K > 1, its class posteriors and posterior mean rate), lnL and, DOWN,
// the marginal reconstruction of every inner node with the directed joints of every branch, in one pass over the gene-major view
// of the accessory matrix.  The level schedule, node_of, the rule for the schedule's LDS copy and the
// rows of partial sums are tree_anc_kernel's (anc_kernels.h).  What differs:
//   table    xs[K][2][n_pad + M]: per class the row of x and behind it the row of y = 1 - x (gene_rule.h) of every LDS slot;
//   team     a workgroup -- one wave for N <= 256, 256 threads above (the tuning key "gene_team" forces either) -- owns ONE gene per
//            trip and strides over the genes.  The core kernels' tile of four columns buys a four-byte leaf dword; a gene's leaves
//            are bits already, W words that the team copies to LDS as they are, and there are few genes: a trip per gene gives
//            four times as many trips to spread over the chip.  At cfg2 the four-wave team takes 0.79 of the single wave's
//            time (profiles/gene_model.md); the tile itself was not built for genes;
//   leaves   leaf i of the tree is OUTPUT row i, internal row slot[i] = its LDS slot: bit (slot & 63) of word slot >> 6;
//   node     two f64 of partial and one i32 exponent per merge;
//   sums     DOWN: per slot gain and loss, per schedule entry pmax (node_conf) and p_1 (node_genes); a slot is the child of one
//            merge and an entry is one lane's: one writer each, no floating-point atomics.  Per gene: every lane keeps the gains and
//            losses of the branches it visited with their rounding errors (ps_gene_add), a butterfly over the wave and the waves
//            in order give the gene's two sums;
//   states   the lane of merge j ORs bit (node_of[j] & 31) into dword node_of[j] >> 5 of the gene's row of inner nodes in LDS
//            (integer LDS OR), the team stores the row's 64-bit words to the gene-major view of the NEW handle.
// gene_g_to_i_kernel then builds the new handle's individual-major view from it.
//
// Dynamic LDS, in this order: 2 Mp f64 of partials; 2 slots f64 of gains and losses; 2 M f64 of node_conf and node_genes; MIX only:
// 2 M f64 of (p_0, p_1) accumulated over the classes; W u64 of leaf words; Wm u64 of state words; Mp i32 of exponents; sched_lds:
// the schedule, node_of and the level offsets behind those.  With n_pad = N, M = N - 1, Mp = N, W = Wm = N / 64 (N a multiple of
// 256): 68.25 N - 32 bytes assigned, 84.25 N - 48 a mixture.
#pragma once

#include "anc_kernels.h"
#include "gene_rule.h"

// the largest multiples of 256 whose layout above fits the CU's 160 KiB beside the 512 bytes kept for static LDS:
// 68.25 N - 32 <= 163 328 -> 2304 (157 216 bytes), 84.25 N - 48 <= 163 328 -> 1792 (150 928 bytes)
#define PS_GENE_KERNEL_MAX_POP 2304u
#define PS_GENE_KERNEL_MAX_POP_MIX 1792u

// pi, rho, the rates and the weights of the K classes: a kernel argument
struct gene_args {
    double freq[2], root[2], rate[PS_MODEL_MAX_CATEGORIES], weight[PS_MODEL_MAX_CATEGORIES];
    uint32_t K;
};

// what the kernel writes per gene and per call (each pointer may be null)
struct gene_outputs {
    double *mant;               // G
    int32_t *ex;                // G
    double *post;               // G x K
    double *rate;               // G
    double *gains, *losses;     // G (DOWN)
    uint64_t *states;           // G x Wm: the gene-major view of the new handle (DOWN)
};

#define PS_GENE_LOAD(c, L, e)                                             \
    do {                                                                  \
        if ((c) < n_pad) {                                                \
            ps_gene_leaf((uint32_t)(LW[(c) >> 6] >> ((c) & 63u)) & 1u, (L)); \
            (e) = 0;                                                      \
        } else {                                                          \
            const uint32_t i_ = (c) - n_pad;                              \
            (L)[0] = P0[i_];                                              \
            (L)[1] = P1[i_];                                              \
            (e) = E[i_];                                                  \
        }                                                                 \
    } while (0)

// accG: the gene-major view, `genes` rows of W words over the internal rows.  sched .. sched_lds, node_of: as tree_anc_kernel takes
// them.  gene_class[genes] (null: K = 1 or a mixture).  Wm = the words of a row of the new view, (M + 63) / 64.  part: gridDim.x
// rows of `stride` f64 = gain then loss of every slot, node_conf then node_genes of every schedule entry (DOWN only), lnL last.
// counts[0]: the genes of likelihood 0.
template <bool MIX, bool DOWN>
__global__ void __launch_bounds__(256) tree_gene_kernel(const uint64_t *accG, uint32_t W, uint32_t N, uint32_t genes, const uint32_t *sched,
                                                        const uint32_t *level_off, uint32_t levels, uint32_t M, uint32_t n_pad, const double *xs,
                                                        uint32_t sched_lds, gene_args a, const uint8_t *gene_class, const uint32_t *node_of,
                                                        uint32_t Wm, gene_outputs o, double *part, uint32_t stride, unsigned long long *counts)
{
    extern __shared__ uint4 gene_lds[];
    __shared__ double s_rate[PS_MODEL_MAX_CATEGORIES], s_w[PS_MODEL_MAX_CATEGORIES], s_mant[PS_MODEL_MAX_CATEGORIES], s_post[PS_MODEL_MAX_CATEGORIES];
    __shared__ double s_rho[2], s_red[16];
    __shared__ int32_t s_ex[PS_MODEL_MAX_CATEGORIES];
    __shared__ uint32_t s_zero;
    const uint32_t tid = threadIdx.x, T = blockDim.x, lane = tid & 63u, wave = tid >> 6, waves = T >> 6;
    const uint32_t Mp = (M + 1u) & ~1u, slots = n_pad + M, K = a.K;
    double *P0 = (double *)gene_lds, *P1 = P0 + Mp;
    double *BG = P1 + Mp, *BL = BG + slots, *NC = BL + slots, *NG = NC + M;
    double *Q0 = NG + M, *Q1 = Q0 + M;                                          // (MIX only: the assigned form has no such region)
    uint64_t *LW = (uint64_t *)(MIX ? Q1 + M : NG + M), *OW = LW + W;
    int32_t *E = (int32_t *)(OW + Wm);
    uint32_t *ls = (uint32_t *)(E + Mp), *ln = ls + M, *lo = ln + M;
    uint32_t *OW32 = (uint32_t *)OW;
    const double pi[2] = { a.freq[0], a.freq[1] };
    if (DOWN)
        for (uint32_t i = tid; i < 2u * slots + 2u * M; i += T) BG[i] = 0.0;
#pragma unroll
    for (uint32_t i = 0; i < PS_MODEL_MAX_CATEGORIES; i++)
        if (tid == i) {
            s_rate[i] = a.rate[i];
            s_w[i] = a.weight[i];
            if (i < 2u) s_rho[i] = a.root[i];
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
    uint32_t zero = 0u;
    for (uint32_t g = blockIdx.x; g < genes; g += gridDim.x) {
        __syncthreads();                          // (the gene before has been stored; the first: s_rate and the schedule)
        for (uint32_t i = tid; i < W; i += T) LW[i] = accG[(size_t)g * W + i];
        if (DOWN)
            for (uint32_t i = tid; i < Wm; i += T) OW[i] = 0ull;
        __syncthreads();
        // the up pass with the row xk of the table; the root's lane leaves the class's pair in s_mant / s_ex[pair]
        auto up = [&](const double *xk, uint32_t pair) {
            const double *yk = xk + slots;
            for (uint32_t lev = 0; lev < levels; lev++) {
                const uint32_t hi = level(lev + 1u);
                for (uint32_t j = level(lev) + tid; j < hi; j += T) {
                    const uint32_t e = entry(j);
                    const uint32_t cl = e & PS_PARS_SLOT, cr = (e >> 16) & PS_PARS_SLOT;
                    double Ll[2], Lr[2], ml[2], mr[2], L[2];
                    int32_t el, er;
                    PS_GENE_LOAD(cl, Ll, el);
                    PS_GENE_LOAD(cr, Lr, er);
                    ps_gene_up(xk[cl], yk[cl], pi, Ll, ml);
                    ps_gene_up(xk[cr], yk[cr], pi, Lr, mr);
                    const int32_t ex = (el + er) + ps_gene_join(ml, mr, L);
                    P0[j] = L[0];
                    P1[j] = L[1];
                    E[j] = ex;
                    if (e & PS_PARS_ROOT) {
                        s_mant[pair] = ps_gene_site(s_rho, L);
                        s_ex[pair] = ex;
                    }
                }
                __syncthreads();
            }
        };
        double ggain = 0.0, gloss = 0.0, cgain = 0.0, closs = 0.0;      // (DOWN: the joints of the branches this lane visits, ps_gene_add)
        // the down pass of a class with posterior `post`; first / last: of the classes of this gene
        auto down = [&](const double *xk, double post, bool first, bool last) {
            const double *yk = xk + slots;
            for (uint32_t lev = levels; lev-- > 0u;) {
                const uint32_t hi = level(lev + 1u);
                for (uint32_t j = level(lev) + tid; j < hi; j += T) {
                    const uint32_t e = entry(j);
                    const uint32_t cl = e & PS_PARS_SLOT, cr = (e >> 16) & PS_PARS_SLOT;
                    double Tv[2], Ll[2], Lr[2], ml[2], mr[2], Ua[2], Ub[2], w[2];
                    int32_t el, er;
                    if (e & PS_PARS_ROOT) {
                        Tv[0] = s_rho[0];
                        Tv[1] = s_rho[1];
                    } else {
                        const double U[2] = { P0[j], P1[j] };
                        ps_gene_down(xk[n_pad + j], yk[n_pad + j], pi, U, Tv);
                    }
                    PS_GENE_LOAD(cl, Ll, el);
                    PS_GENE_LOAD(cr, Lr, er);
                    const double xl = xk[cl], xr = xk[cr], yl = yk[cl], yr = yk[cr];
                    ps_gene_up(xl, yl, pi, Ll, ml);
                    ps_gene_up(xr, yr, pi, Lr, mr);
                    const double sum = ps_gene_node_post(Tv, ml, mr, w);
                    (void)ps_gene_join(mr, Tv, Ua);
                    (void)ps_gene_join(ml, Tv, Ub);
                    double ga, la, gb, lb;
                    ps_gene_joints(xl, yl, pi, Ua, Ll, &ga, &la);
                    ps_gene_joints(xr, yr, pi, Ub, Lr, &gb, &lb);
                    ga = post * ga;
                    la = post * la;
                    gb = post * gb;
                    lb = post * lb;
                    BG[cl] += ga;
                    BL[cl] += la;
                    BG[cr] += gb;
                    BL[cr] += lb;
                    ggain = ps_gene_add(ggain, ga, &cgain);
                    ggain = ps_gene_add(ggain, gb, &cgain);
                    gloss = ps_gene_add(gloss, la, &closs);
                    gloss = ps_gene_add(gloss, lb, &closs);
                    double p0 = ps_subst_post_term(post, w[0], sum), p1 = ps_subst_post_term(post, w[1], sum);
                    if (MIX && !first) {
                        p0 = Q0[j] + p0;
                        p1 = Q1[j] + p1;
                    }
                    if (!MIX || last) {
                        double pmax;
                        const uint32_t one = ps_gene_map(p0, p1, &pmax);
                        NC[j] += pmax;
                        NG[j] += p1;
                        if (one) {
                            const uint32_t m = merge_of(j);
                            atomicOr(&OW32[m >> 5], 1u << (m & 31u));
                        }
                    } else {
                        Q0[j] = p0;
                        Q1[j] = p1;
                    }
                    if (cl >= n_pad) {
                        const uint32_t i = cl - n_pad;
                        P0[i] = Ua[0];
                        P1[i] = Ua[1];
                    }
                    if (cr >= n_pad) {
                        const uint32_t i = cr - n_pad;
                        P0[i] = Ub[0];
                        P1[i] = Ub[1];
                    }
                    (void)el;
                    (void)er;
                }
                __syncthreads();
            }
        };
        // the classes of the gene: its own alone (assigned), or all K (a mixture)
        const uint32_t kb = MIX ? 0u : (gene_class ? (uint32_t)gene_class[g] : 0u), ke = MIX ? K : kb + 1u;
        for (uint32_t kc = kb; kc < ke; kc++) up(xs + (size_t)kc * 2u * slots, kc);
        if (tid == 0u) {
            double mant, rate;
            int32_t ex;
            if (!MIX) {
                mant = s_mant[kb];
                ex = s_ex[kb];
                rate = s_rate[kb];
                for (uint32_t k = 0; k < K; k++) s_post[k] = k == kb ? 1.0 : 0.0;
            } else {
                mant = ps_subst_mix(K, s_w, s_mant, s_ex, &ex, s_post);
                rate = ps_subst_mean_rate(K, s_post, s_rate);
            }
            if (o.mant) o.mant[g] = mant;
            if (o.ex) o.ex[g] = ex;
            if (o.rate) o.rate[g] = rate;
            if (o.post)
                for (uint32_t k = 0; k < K; k++) o.post[(size_t)g * K + k] = s_post[k];
            lnl += ps_jc_site_ln(mant, ex);
            s_zero = mant > 0.0 ? 0u : 1u;
            zero += mant > 0.0 ? 0u : 1u;
        }
        if (!DOWN) continue;
        __syncthreads();                          // (the posterior, and whether the gene has a likelihood at all)
        if (!s_zero) {                            // (a gene of likelihood 0: absent at every node, nothing added)
            for (uint32_t kc = kb; kc < ke; kc++) {
                const double *xk = xs + (size_t)kc * 2u * slots;
                if (MIX) up(xk, kc);              // (the partials of class kc were overwritten; an assigned gene's are still there)
                down(xk, s_post[kc], kc == kb, kc + 1u == ke);
            }
        }
        // the gene's two sums: a butterfly over the wave, then the waves in order
#pragma unroll
        for (int d = 32; d; d >>= 1) {
            const double og = __shfl_xor(ggain, d, 64), ocg = __shfl_xor(cgain, d, 64);
            const double ol = __shfl_xor(gloss, d, 64), ocl = __shfl_xor(closs, d, 64);
            ggain = ps_gene_add(ggain, og, &cgain);
            cgain += ocg;
            gloss = ps_gene_add(gloss, ol, &closs);
            closs += ocl;
        }
        if (lane == 0u) {
            s_red[wave] = ggain;
            s_red[4u + wave] = cgain;
            s_red[8u + wave] = gloss;
            s_red[12u + wave] = closs;
        }
        __syncthreads();
        if (tid == 0u) {
            double sg = s_red[0], cg = s_red[4], sl = s_red[8], cl = s_red[12];
            for (uint32_t v = 1; v < waves; v++) {
                sg = ps_gene_add(sg, s_red[v], &cg);
                cg += s_red[4u + v];
                sl = ps_gene_add(sl, s_red[8u + v], &cl);
                cl += s_red[12u + v];
            }
            if (o.gains) o.gains[g] = sg + cg;
            if (o.losses) o.losses[g] = sl + cl;
        }
        if (o.states)
            for (uint32_t i = tid; i < Wm; i += T) o.states[(size_t)g * Wm + i] = OW[i];
    }
    // the flush: the workgroup's own row, and one integer atomic per workgroup that met a gene of likelihood 0
    __syncthreads();
    double *prow = part + (size_t)blockIdx.x * stride;
    if (DOWN)
        for (uint32_t i = tid; i < 2u * slots + 2u * M; i += T) prow[i] = BG[i];
    if (tid == 0u) {
        prow[stride - 1u] = lnl;
        if (zero) atomicAdd(counts, (unsigned long long)zero);
    }
}

#undef PS_GENE_LOAD

// The gene-major view of d.G rows of d.W words -> the individual-major view of d.N rows of d.GW words: one wave per (word of
// individuals w, word of genes gw), lane = gene; a ballot per individual is its word.  Genes from d.G on read as 0: the pad bits of
// the last word of every row are zero.
__global__ void __launch_bounds__(64) gene_g_to_i_kernel(const uint64_t *accG, uint64_t *accI, acc_dims d)
{
    const uint32_t w = blockIdx.x, gw = blockIdx.y, lane = threadIdx.x;
    const uint32_t g = gw * 64u + lane;
    const uint64_t mine = g < d.G ? accG[(uint64_t)g * d.W + w] : 0ull;
    for (uint32_t b = 0; b < 64u; b++) {
        const uint32_t i = w * 64u + b;
        if (i >= d.N) break;
        const uint64_t word = __ballot((mine >> b) & 1ull);
        if (lane == 0u) accI[(uint64_t)i * d.GW + gw] = word;
    }
}
