// jc_rule.h -- the arithmetic of the Jukes-Cantor likelihood of a tree (docs/TREE_LIKELIHOOD.md), every line one fixed sequence of
// IEEE-754 binary64 operations in one association: the kernel (likelihood_kernels.h), the host restatement
// (ps_likelihood_from_rows, ps_ml_lengths_from_rows) and a stand-alone check (tests/jc_rule_check.cpp) include this one header, so
// a site's (mantissa, exponent) and a site's derivative ratio r are the same bits wherever they are formed.  Plain C++17 under g++;
// under hipcc every function is __host__ __device__.  The library is built with -ffp-contract=off -fno-fast-math: no line below
// may become a fused multiply-add, and a host program that includes this header is built the same way.  frexp and ldexp are exact.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PS_JC_FN __host__ __device__ __forceinline__
#else
#define PS_JC_FN static inline
#endif

// every branch length is used as min(max(t, PS_LIK_MIN_LENGTH), PS_LIK_MAX_LENGTH), in expected substitutions per site
#define PS_LIK_MIN_LENGTH 1e-8
#define PS_LIK_MAX_LENGTH 10.0

PS_JC_FN double ps_jc_clamp(double t) { return t < PS_LIK_MIN_LENGTH ? PS_LIK_MIN_LENGTH : (t > PS_LIK_MAX_LENGTH ? PS_LIK_MAX_LENGTH : t); }

// x = exp(-4 t / 3) of a used length: the probability that no substitution event has hit the branch (host: the kernel sees x only)
PS_JC_FN double ps_jc_x(double t) { return exp((-4.0 * t) / 3.0); }

// the partial of a leaf from its byte (or its class byte): the indicator of the base 1 / 2 / 4 / 8, (1, 1, 1, 1) for any other byte
PS_JC_FN bool ps_jc_known(uint32_t b) { return b == 1u || b == 2u || b == 4u || b == 8u; }

PS_JC_FN void ps_jc_leaf(uint32_t b, double L[4])
{
    const bool known = ps_jc_known(b);
    L[0] = !known || b == 1u ? 1.0 : 0.0;
    L[1] = !known || b == 2u ? 1.0 : 0.0;
    L[2] = !known || b == 4u ? 1.0 : 0.0;
    L[3] = !known || b == 8u ? 1.0 : 0.0;
}

PS_JC_FN double ps_jc_sum(const double L[4]) { return (L[0] + L[1]) + (L[2] + L[3]); }

// the message of a partial along a branch with x: m_a = q S + x L_a, q = (1 - x) / 4.  Up: L of the child, to its parent; down: U of
// a node, to its children (T)
PS_JC_FN void ps_jc_message(double x, const double L[4], double m[4])
{
    const double q = (1.0 - x) * 0.25, qs = q * ps_jc_sum(L);
    m[0] = qs + x * L[0];
    m[1] = qs + x * L[1];
    m[2] = qs + x * L[2];
    m[3] = qs + x * L[3];
}

// the four entries scaled by the power of two that brings the largest into [0.5, 1); returns the binary exponent taken out
PS_JC_FN int32_t ps_jc_rescale(double L[4])
{
    const double m01 = L[0] > L[1] ? L[0] : L[1], m23 = L[2] > L[3] ? L[2] : L[3];
    int k = 0;
    (void)frexp(m01 > m23 ? m01 : m23, &k);
    L[0] = ldexp(L[0], -k);
    L[1] = ldexp(L[1], -k);
    L[2] = ldexp(L[2], -k);
    L[3] = ldexp(L[3], -k);
    return (int32_t)k;
}

// the partial of a node from the messages of its two children (and the outside partial of a node from its sibling's message and
// the message from above), rescaled
PS_JC_FN int32_t ps_jc_join(const double ml[4], const double mr[4], double L[4])
{
    L[0] = ml[0] * mr[0];
    L[1] = ml[1] * mr[1];
    L[2] = ml[2] * mr[2];
    L[3] = ml[3] * mr[3];
    return ps_jc_rescale(L);
}

// the mantissa of the site likelihood from the root's partial; its exponent is the root's
PS_JC_FN double ps_jc_site(const double L[4]) { return 0.25 * ps_jc_sum(L); }

// ln of a site likelihood (log is not shared between host and device: within 1 ulp of each other)
PS_JC_FN double ps_jc_site_ln(double mant, int32_t e) { return log(mant) + (double)e * 0.6931471805599453094; }

// Branch c with x, outside partial U and inside partial L: the site likelihood is A + x B up to one power of two, and
// r = B / (A + x B) is what the branch adds to g (and r r to h).  With D = A + B the denominator is formed as (1 - x) A + x D, a sum
// of non-negative terms: A + x B itself cancels on a short branch between unlike neighbours (A = -B (1 - 1e-8)), and the error of r
// would grow with 1 / likelihood squared.  Only B = D - A is a difference, with an absolute error of a rounding of max(A, D).
PS_JC_FN double ps_jc_ratio(double x, const double U[4], const double L[4])
{
    const double A = (ps_jc_sum(L) * ps_jc_sum(U)) * 0.0625;
    const double D = ((U[0] * L[0] + U[1] * L[1]) + (U[2] * L[2] + U[3] * L[3])) * 0.25;
    return (D - A) / ((1.0 - x) * A + x * D);
}

// The derivatives with respect to t of a branch from its sums g = sum r, h = sum r r (host)
PS_JC_FN double ps_jc_dt(double x, double g) { return -((4.0 * x) / 3.0) * g; }

PS_JC_FN double ps_jc_dt2(double x, double g, double h) { return ((16.0 * (x * x)) / 9.0) * (-h) + ((16.0 * x) / 9.0) * g; }

// One damped Newton step of a used length t (host): delta = -g_t / h_t where the curvature is negative, else a whole t in the
// gradient's direction; limited to [-t / 2, max(t, 1e-3)]; t' = clamp(t + lambda delta)
PS_JC_FN double ps_jc_newton(double t, double x, double g, double h, double lambda)
{
    const double gt = ps_jc_dt(x, g), ht = ps_jc_dt2(x, g, h);
    double d = ht < 0.0 ? -gt / ht : (gt > 0.0 ? t : (gt < 0.0 ? -t : 0.0));
    const double lo = -0.5 * t, hi = t > 1e-3 ? t : 1e-3;
    d = d < lo ? lo : (d > hi ? hi : d);
    return ps_jc_clamp(t + lambda * d);
}

// A start length from the parsimony changes of a branch over `sites` sites (host): the Jukes-Cantor correction of p = changes /
// sites, PS_LIK_MAX_LENGTH from p = 0.74 on (0.75 is the pole), PS_LIK_MIN_LENGTH without sites
PS_JC_FN double ps_jc_length_from_changes(uint64_t changes, uint64_t sites)
{
    if (sites == 0u) return PS_LIK_MIN_LENGTH;
    const double p = (double)changes / (double)sites;
    if (p >= 0.74) return PS_LIK_MAX_LENGTH;
    return -0.75 * log(1.0 - (4.0 * p) / 3.0);
}
