// gene_rule.h -- the arithmetic of the gain / loss likelihood of the accessory genes on a tree (docs/GENE_MODEL.md): F81 on the two
// states 0 = absent, 1 = present, with a root distribution and up to 8 rate classes per gene.  Written as subst_rule.h is: every
// line one fixed sequence of IEEE-754 binary64 operations in one association, no fused multiply-add (-ffp-contract=off),
// __host__ __device__ under hipcc and plain C++17 under g++.  The kernel (gene_kernels.h), the host restatement (tree_genes.h) and a
// stand-alone check (tests/gene_rule_check.cpp) include this one header, so a gene's (mantissa, exponent), its posteriors and every
// cell's node posterior are the same bits wherever they are formed.
//
// The model: P(t) = x I + y 1 pi^T, x = exp(-(r t) / beta) the probability that no event hit the branch and y = 1 - x, beta = 1 -
// pi_0^2 - pi_1^2; the root's state is drawn from rho.  In gain / loss terms the gain rate is r pi_1 / beta and the loss rate
// r pi_0 / beta.  y is formed on the host as -expm1(-(r t) / beta) and travels beside x: on a branch at the lower clamp 1 - x has
// eight digits left, and a gene whose only explanation is a change on such a branch would have a likelihood no better than that.
// The mixture over the classes, the posterior and the posterior mean rate are ps_subst_mix / ps_subst_mean_rate as they are.
#pragma once

#include "subst_rule.h"

PS_JC_FN double ps_gene_dot(const double p[2], const double L[2]) { return p[0] * L[0] + p[1] * L[1]; }

// beta = 1 - pi_0^2 - pi_1^2 (host)
PS_JC_FN double ps_gene_beta(const double pi[2]) { return 1.0 - (pi[0] * pi[0] + pi[1] * pi[1]); }

// x of a used length t in a class of rate r (host: the kernel sees x only); r = 0 gives 1, a long branch underflows to 0
PS_JC_FN double ps_gene_x(double r, double t, double beta) { return exp(-(r * t) / beta); }

// y = 1 - x of the same branch to full precision (host)
PS_JC_FN double ps_gene_y(double r, double t, double beta) { return -expm1(-(r * t) / beta); }

// a length as it is used: clamped below only (a tree in generations is legitimate input)
PS_JC_FN double ps_gene_clamp(double t) { return t < PS_LIK_MIN_LENGTH ? PS_LIK_MIN_LENGTH : t; }

// the partial of a leaf: the indicator of its state (any byte but 0 is present)
PS_JC_FN void ps_gene_leaf(uint32_t present, double L[2])
{
    L[0] = present ? 0.0 : 1.0;
    L[1] = present ? 1.0 : 0.0;
}

// up: the message of the inside partial L of a child to its parent, m_a = y (pi . L) + x L_a
PS_JC_FN void ps_gene_up(double x, double y, const double pi[2], const double L[2], double m[2])
{
    const double s = y * ps_gene_dot(pi, L);
    m[0] = s + x * L[0];
    m[1] = s + x * L[1];
}

// down: the message of the outside partial U at the top of a branch to its lower end, T_a = (y pi_a)(U_0 + U_1) + x U_a
PS_JC_FN void ps_gene_down(double x, double y, const double pi[2], const double U[2], double T[2])
{
    const double su = U[0] + U[1];
    T[0] = (y * pi[0]) * su + x * U[0];
    T[1] = (y * pi[1]) * su + x * U[1];
}

// the two entries scaled by the power of two that brings the larger into [0.5, 1), by ps_jc_rescale itself
PS_JC_FN int32_t ps_gene_rescale(double L[2])
{
    double q[4] = { L[0], L[1], 0.0, 0.0 };
    const int32_t k = ps_jc_rescale(q);
    L[0] = q[0];
    L[1] = q[1];
    return k;
}

// the partial of a node from the messages of its two children (and an outside partial from the sibling's message and the message
// from above), rescaled
PS_JC_FN int32_t ps_gene_join(const double ml[2], const double mr[2], double L[2])
{
    L[0] = ml[0] * mr[0];
    L[1] = ml[1] * mr[1];
    return ps_gene_rescale(L);
}

// the mantissa of a class's gene likelihood from the root's rescaled partial, rho_0 L_0 + rho_1 L_1; its exponent is the root's
PS_JC_FN double ps_gene_site(const double rho[2], const double L[2]) { return ps_gene_dot(rho, L); }

// The marginal posterior of an inner node from the three pieces that meet there: w_a = (T_a ml_a) mr_a; returns w_0 + w_1
PS_JC_FN double ps_gene_node_post(const double T[2], const double ml[2], const double mr[2], double w[2])
{
    w[0] = (T[0] * ml[0]) * mr[0];
    w[1] = (T[1] * ml[1]) * mr[1];
    return w[0] + w[1];
}

// the state of a node from (p_0, p_1): 1 iff p_1 > p_0 (an exact tie is absent); *pmax = the larger
PS_JC_FN uint32_t ps_gene_map(double p0, double p1, double *pmax)
{
    const bool one = p1 > p0;
    *pmax = one ? p1 : p0;
    return one ? 1u : 0u;
}

// Branch c with x and y, outside partial U (top of the branch) and inside partial L: the gene's likelihood is den = y A + x D up to
// one power of two, A = (pi . L)(U_0 + U_1), D = U_0 L_0 + U_1 L_1.  The two directed joints of the branch:
//   gain = (U_0 (y pi_1)) L_1 / den    the posterior probability of absent above and present below
//   loss = (U_1 (y pi_0)) L_0 / den    ... of present above and absent below
// Products of non-negative terms: no difference is taken.  den = 0 (a class of likelihood 0) returns 0 for both.
PS_JC_FN void ps_gene_joints(double x, double y, const double pi[2], const double U[2], const double L[2], double *gain, double *loss)
{
    const double A = ps_gene_dot(pi, L) * (U[0] + U[1]);
    const double D = U[0] * L[0] + U[1] * L[1];
    const double den = y * A + x * D;
    if (!(den > 0.0)) {
        *gain = 0.0;
        *loss = 0.0;
        return;
    }
    *gain = ((U[0] * (y * pi[1])) * L[1]) / den;
    *loss = ((U[1] * (y * pi[0])) * L[0]) / den;
}

// A running sum kept with its rounding errors (a gene's gains and losses over thousands of branches): returns s + v and adds the
// exact error of that addition to *c (Knuth's two-sum, valid for any two doubles; it needs the library's -fno-fast-math).  The sum
// is s + c at the end: within a rounding or two of the exact sum of non-negative terms, whatever the order.
PS_JC_FN double ps_gene_add(double s, double v, double *c)
{
    const double t = s + v, bp = t - s;
    *c += (s - (t - bp)) + (v - bp);
    return t;
}
