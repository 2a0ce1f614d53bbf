// subst_rule.h -- the arithmetic of the likelihood of a tree under F81 with a root distribution and up to 8 rate categories per
// site (docs/TREE_MODEL.md), written as jc_rule.h is: every line one fixed sequence of IEEE-754 binary64 operations in one
// association, no fused multiply-add (-ffp-contract=off), __host__ __device__ under hipcc and plain C++17 under g++.  The kernel
// (model_kernels.h), the host restatement (tree_model.h) and a stand-alone check (tests/subst_rule_check.cpp) include this one
// header, so a site's (mantissa, exponent), posterior and derivative terms are the same bits wherever they are formed.
//
// The model: P(t) = x I + (1 - x) 1 pi^T, x = exp(-(r t) / beta) the probability that no event hit the branch, beta = 1 - sum pi_a^2;
// the root's state is drawn from rho.  With pi = rho = 1/4 and r = 1 every scaling below is a power of two and every result is
// the same bits as jc_rule.h's (the associations are chosen for that).
#pragma once

#include "jc_rule.h"

#define PS_MODEL_MAX_CATEGORIES 8u

PS_JC_FN double ps_subst_dot(const double p[4], const double L[4]) { return (p[0] * L[0] + p[1] * L[1]) + (p[2] * L[2] + p[3] * L[3]); }

// beta = 1 - sum pi_a^2: the expected substitutions per event (host)
PS_JC_FN double ps_subst_beta(const double pi[4]) { return 1.0 - ((pi[0] * pi[0] + pi[1] * pi[1]) + (pi[2] * pi[2] + pi[3] * pi[3])); }

// x of a used length t in a category of rate r (host: the kernel sees x only); r = 0 gives exp(-0) = 1
PS_JC_FN double ps_subst_x(double r, double t, double beta) { return exp(-(r * t) / beta); }

// up: the message of the inside partial L of a child to its parent, m_a = (1 - x)(pi . L) + x L_a
PS_JC_FN void ps_subst_up(double x, const double pi[4], const double L[4], double m[4])
{
    const double s = (1.0 - x) * ps_subst_dot(pi, L);
    m[0] = s + x * L[0];
    m[1] = s + x * L[1];
    m[2] = s + x * L[2];
    m[3] = s + x * L[3];
}

// down: the message of the outside partial U at the top of a branch to its lower end, T_a = (1 - x) pi_a sum U + x U_a
PS_JC_FN void ps_subst_down(double x, const double pi[4], const double U[4], double T[4])
{
    const double y = 1.0 - x, su = ps_jc_sum(U);
    T[0] = (y * pi[0]) * su + x * U[0];
    T[1] = (y * pi[1]) * su + x * U[1];
    T[2] = (y * pi[2]) * su + x * U[2];
    T[3] = (y * pi[3]) * su + x * U[3];
}

// the mantissa of a category's site likelihood from the root's rescaled partial; its exponent is the root's
PS_JC_FN double ps_subst_site(const double rho[4], const double L[4]) { return ps_subst_dot(rho, L); }

// Branch c with x, outside partial U (top of the branch) and inside partial L: the site likelihood is (1 - x) A + x D up to one
// power of two, A = (pi . L)(sum U), D = sum U_a L_a, and the ratio (D - A) / ((1 - x) A + x D) is its derivative with respect
// to x over itself (the denominator a sum of non-negative terms, as in ps_jc_ratio)
PS_JC_FN double ps_subst_ratio(double x, const double pi[4], const double U[4], const double L[4])
{
    const double A = ps_subst_dot(pi, L) * ps_jc_sum(U);
    const double D = (U[0] * L[0] + U[1] * L[1]) + (U[2] * L[2] + U[3] * L[3]);
    return (D - A) / ((1.0 - x) * A + x * D);
}

// The mixture of K category pairs (mant_k, e_k) with weights w: e = the largest exponent of a category whose mantissa is not 0 (a
// category of likelihood 0 -- an invariant class at a variable site -- has no exponent to speak of; e_0 when all are 0),
// mix = sum_k w_k ldexp(mant_k, e_k - e), k ascending, not renormalised: K = 1 with w = 1 returns the category's own pair.
// post_k = (w_k ldexp(mant_k, e_k - e)) / mix.  Returns mix.
PS_JC_FN double ps_subst_mix(uint32_t K, const double *w, const double *mant, const int32_t *ex, int32_t *e_out, double *post)
{
    int32_t e = ex[0];
    bool any = mant[0] > 0.0;
    for (uint32_t k = 1; k < K; k++)
        if (mant[k] > 0.0 && (!any || ex[k] > e)) {
            e = ex[k];
            any = true;
        }
    double mix = 0.0;
    for (uint32_t k = 0; k < K; k++) {
        post[k] = w[k] * ldexp(mant[k], mant[k] > 0.0 ? ex[k] - e : 0);
        mix = k == 0u ? post[0] : mix + post[k];
    }
    for (uint32_t k = 0; k < K; k++) post[k] = mix > 0.0 ? post[k] / mix : w[k];       // (a site of likelihood 0: the prior)
    *e_out = e;
    return mix;
}

// the posterior mean rate of a site, sum_k post_k r_k, k ascending
PS_JC_FN double ps_subst_mean_rate(uint32_t K, const double *post, const double *rate)
{
    double s = post[0] * rate[0];
    for (uint32_t k = 1; k < K; k++) s += post[k] * rate[k];
    return s;
}

// What category k adds to D_sc of a branch: post_k ((r_k x_ck) ratio); a category of rate 0 adds nothing (its ratio may be 0 / 0).
// What it adds to q is r_k times that, formed as (post_k r_k) ((r_k x_ck) ratio).
PS_JC_FN double ps_subst_dterm(double post, double r, double x, double ratio) { return r == 0.0 ? 0.0 : post * ((r * x) * ratio); }

PS_JC_FN double ps_subst_qterm(double post, double r, double x, double ratio) { return r == 0.0 ? 0.0 : (post * r) * ((r * x) * ratio); }

// The derivatives with respect to t of a branch from its sums g, h, q (host)
PS_JC_FN double ps_subst_dt(double beta, double g) { return -g / beta; }

PS_JC_FN double ps_subst_dt2(double beta, double q, double h) { return (q - h) / (beta * beta); }

// One damped Newton step of a used length t from the derivatives themselves (host): the step rule of ps_jc_newton
PS_JC_FN double ps_subst_newton(double t, double gt, double ht, double lambda)
{
    double d = ht < 0.0 ? -gt / ht : (gt > 0.0 ? t : (gt < 0.0 ? -t : 0.0));
    const double lo = -0.5 * t, hi = t > 1e-3 ? t : 1e-3;
    d = d < lo ? lo : (d > hi ? hi : d);
    return ps_jc_clamp(t + lambda * d);
}

// A start length from the parsimony changes of a branch over `sites` sites (host): the F81 correction -beta ln(1 - p / beta) of
// p = changes / sites, PS_LIK_MAX_LENGTH from p = 0.98 beta on (beta is the pole), PS_LIK_MIN_LENGTH without sites
PS_JC_FN double ps_subst_length_from_changes(uint64_t changes, uint64_t sites, double beta)
{
    if (sites == 0u) return PS_LIK_MIN_LENGTH;
    const double p = (double)changes / (double)sites;
    if (p >= 0.98 * beta) return PS_LIK_MAX_LENGTH;
    return -beta * log(1.0 - p / beta);
}

// ---- the likelihood of a neighbour tree (docs/LIKELIHOOD_SEARCH.md) ----
// An internal edge v - c, c = (a, b), with sibling s: the four pieces around it are the messages m^a, m^b, m^s (ps_subst_up of the
// inside partials) and T(v), the message into v from above (rho at the root).  A nearest-neighbour interchange regroups them into
// an inside pair I (joined below the edge) and an outside pair O (joined above it) and changes none of them, nor x_c.

// the join of two pieces, NOT rescaled: the three arrangements of an edge share one scale, so their ratios need no exponent
PS_JC_FN void ps_subst_pair(const double a[4], const double b[4], double out[4])
{
    out[0] = a[0] * b[0];
    out[1] = a[1] * b[1];
    out[2] = a[2] * b[2];
    out[3] = a[3] * b[3];
}

// the site likelihood with I below and O above an edge with x, up to the common power of two: (1 - x)(pi . I)(sum O) + x sum O_a I_a,
// the shape of ps_subst_ratio's denominator, a sum of non-negative terms
PS_JC_FN double ps_subst_nni_lik(double x, const double pi[4], const double I[4], const double O[4])
{
    const double A = ps_subst_dot(pi, I) * ps_jc_sum(O);
    const double D = (O[0] * I[0] + O[1] * I[1]) + (O[2] * I[2] + O[3] * I[3]);
    return (1.0 - x) * A + x * D;
}

// the same on the root's edge, the root between c (x_c, I below it) and s (x_s, O below it): sum_a rho_a up(x_c, I)_a up(x_s, O)_a
PS_JC_FN double ps_subst_nni_root(double xc, double xs, const double pi[4], const double rho[4], const double I[4], const double O[4])
{
    double u[4], w[4];
    ps_subst_up(xc, pi, I, u);
    ps_subst_up(xs, pi, O, w);
    return ((rho[0] * u[0]) * w[0] + (rho[1] * u[1]) * w[1]) + ((rho[2] * u[2]) * w[2] + (rho[3] * u[3]) * w[3]);
}

// The three arrangements below an inner node, (m^a, m^b | m^s, T(v)): l[0] the tree as it stands, l[1] kind 0 (b <-> s:
// (a, s | b, T)), l[2] kind 1 (a <-> s: (s, b | a, T))
PS_JC_FN void ps_subst_nni_edge(double x, const double pi[4], const double px[4], const double py[4], const double pz[4], const double pw[4],
                                double l[3])
{
    double I[4], O[4];
    ps_subst_pair(px, py, I);
    ps_subst_pair(pz, pw, O);
    l[0] = ps_subst_nni_lik(x, pi, I, O);
    ps_subst_pair(px, pz, I);
    ps_subst_pair(py, pw, O);
    l[1] = ps_subst_nni_lik(x, pi, I, O);
    ps_subst_pair(pz, py, I);
    ps_subst_pair(px, pw, O);
    l[2] = ps_subst_nni_lik(x, pi, I, O);
}

// The three arrangements on the root's edge, c = (a, b) with x_c beside s = (p, q) with x_s, both keeping their lengths: l[0] the
// tree as it stands, l[1] kind 0 (b <-> p: c = (a, p), s = (b, q)), l[2] kind 1 (b <-> q: c = (a, q), s = (p, b))
PS_JC_FN void ps_subst_nni_root_edge(double xc, double xs, const double pi[4], const double rho[4], const double pa[4], const double pb[4],
                                     const double pp[4], const double pq[4], double l[3])
{
    double I[4], O[4];
    ps_subst_pair(pa, pb, I);
    ps_subst_pair(pp, pq, O);
    l[0] = ps_subst_nni_root(xc, xs, pi, rho, I, O);
    ps_subst_pair(pa, pp, I);
    ps_subst_pair(pb, pq, O);
    l[1] = ps_subst_nni_root(xc, xs, pi, rho, I, O);
    ps_subst_pair(pa, pq, I);
    ps_subst_pair(pp, pb, O);
    l[2] = ps_subst_nni_root(xc, xs, pi, rho, I, O);
}

// What category k adds to a site's ratio l' / l of an interchange: post_k (l'_k / l_k); a category whose likelihood is 0 in this tree
// adds nothing (its posterior is 0 and its ratio 0 / 0).  An assigned site has post = 1: the ratio itself.
PS_JC_FN double ps_subst_nni_term(double post, double lk, double l0) { return l0 > 0.0 ? post * (lk / l0) : 0.0; }

// A running product kept as (mantissa in [1/2, 1), exponent): the mantissa times r, rescaled; *k = the binary exponent taken out,
// which the caller adds to the product's.  One (1/2, 1) is the empty product.  frexp is exact.
PS_JC_FN double ps_subst_prod(double mant, double r, int32_t *k)
{
    int e = 0;
    const double m = frexp(mant * r, &e);
    *k = (int32_t)e;
    return m;
}

// ---- marginal ancestral states (docs/ANCESTRAL_STATES.md) ----
// The marginal posterior of an inner node from the three pieces that meet there -- T, the message into the node from above (rho at
// the root), and the messages ml, mr of its two children: w_a = (T_a ml_a) mr_a, p_a = w_a / sum.  Returns the sum,
// (w_0 + w_1) + (w_2 + w_3): the site likelihood of the category up to the pieces' powers of two.
PS_JC_FN double ps_subst_node_post(const double T[4], const double ml[4], const double mr[4], double w[4])
{
    w[0] = (T[0] * ml[0]) * mr[0];
    w[1] = (T[1] * ml[1]) * mr[1];
    w[2] = (T[2] * ml[2]) * mr[2];
    w[3] = (T[3] * ml[3]) * mr[3];
    return (w[0] + w[1]) + (w[2] + w[3]);
}

// What category k adds to p_a of a node: post_k (w_a / sum); a category whose sum is 0 adds nothing.  An assigned site has post = 1.
PS_JC_FN double ps_subst_post_term(double post, double w, double sum) { return sum > 0.0 ? post * (w / sum) : 0.0; }

// Branch c with x, outside partial U (top of the branch) and inside partial L: the posterior probability that its two ends carry
// different states, (1 - x) max(A - S, 0) / ((1 - x) A + x D) with A and D of ps_subst_ratio and S = sum_a pi_a (U_a L_a), the
// products formed first.  A - S >= 0 in exact arithmetic: the max guards its rounding.  A denominator of 0 (a category of
// likelihood 0) returns 0.
PS_JC_FN double ps_subst_pdiff(double x, const double pi[4], const double U[4], const double L[4])
{
    const double A = ps_subst_dot(pi, L) * ps_jc_sum(U);
    const double ul[4] = { U[0] * L[0], U[1] * L[1], U[2] * L[2], U[3] * L[3] };
    const double D = (ul[0] + ul[1]) + (ul[2] + ul[3]);
    const double S = ps_subst_dot(pi, ul);
    const double y = 1.0 - x, den = y * A + x * D, d = A - S;
    if (!(den > 0.0)) return 0.0;
    return (y * (d > 0.0 ? d : 0.0)) / den;
}

// the index of the largest p_a, exact binary64 ties to the lowest a; *pmax = that p_a
PS_JC_FN uint32_t ps_subst_map(const double p[4], double *pmax)
{
    uint32_t best = 0u;
    double m = p[0];
    if (p[1] > m) {
        m = p[1];
        best = 1u;
    }
    if (p[2] > m) {
        m = p[2];
        best = 2u;
    }
    if (p[3] > m) {
        m = p[3];
        best = 3u;
    }
    *pmax = m;
    return best;
}
