// nj_rule.h -- the arithmetic of the neighbour-joining tree (docs/NEIGHBOUR_JOINING.md), every line one fixed sequence of IEEE-754
// binary64 operations in one association: the kernels (nj_kernels.h), the host restatement (ps_nj_from_counts) and a stand-alone
// check (tests/nj_rule_check.cpp) include this one header, so the three cannot drift apart.  Plain C++17 under g++; under hipcc
// every function is __host__ __device__.  The library is built with -ffp-contract=off -fno-fast-math: no line below may become a
// fused multiply-add, and a host program that includes this header is built the same way.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define PS_NJ_FN __host__ __device__ __forceinline__
#else
#define PS_NJ_FN static inline
#endif

#define PS_NJ_NONE 0xffffffffu

// entry distances: core d = h / 2 (a shard sum is halved behind the sum) in differing sites, an exact integer below 2^32;
// accessory a / b with a = U - I and b = U + core_genes >= 1, one correctly rounded division
PS_NJ_FN double ps_nj_core_distance(uint32_t h) { return (double)(h >> 1); }

PS_NJ_FN double ps_nj_acc_distance(uint32_t in, uint32_t un, uint64_t cg) { return (double)(un - in) / (double)((uint64_t)un + cg); }

// q of the pair (lo, hi), lo the node with the smaller id, among n active nodes: (x - r_lo) - r_hi and (x - r_hi) - r_lo round
// differently, so the orientation is part of the rule
PS_NJ_FN double ps_nj_q(uint32_t n, double d, double r_lo, double r_hi) { return ((double)(n - 2u) * d - r_lo) - r_hi; }

// a pair under the strict total order (q as a number, lo id, hi id)
struct ps_nj_key {
    double q;
    uint32_t lo, hi;
};

PS_NJ_FN bool ps_nj_less(const ps_nj_key &a, const ps_nj_key &b)
{
    if (a.q < b.q) return true;
    if (b.q < a.q) return false;
    return a.lo != b.lo ? a.lo < b.lo : a.hi < b.hi;
}

// the branch above lo of a join among n > 2 active nodes; the branch above hi is dlh - b_lo
PS_NJ_FN double ps_nj_branch_lo(uint32_t n, double dlh, double r_lo, double r_hi)
{
    return 0.5 * dlh + (r_lo - r_hi) / (2.0 * (double)(n - 2u));
}

// the distance of the new node to another active node k, and k's row sum behind the join
PS_NJ_FN double ps_nj_duk(double dlk, double dhk, double dlh) { return 0.5 * ((dlk + dhk) - dlh); }

PS_NJ_FN double ps_nj_r_other(double rk, double dlk, double dhk, double duk) { return ((rk - dlk) - dhk) + duk; }

// the row sum of the new node: in exact arithmetic the sum of its duk; here the definition, never recomputed
PS_NJ_FN double ps_nj_r_joined(uint32_t n, double r_lo, double r_hi, double dlh) { return 0.5 * ((r_lo + r_hi) - (double)n * dlh); }

// the two lengths of one join among n >= 2 active nodes (n == 2: the last edge whole above lo, 0 above hi)
PS_NJ_FN void ps_nj_branches(uint32_t n, double dlh, double r_lo, double r_hi, double *b_lo, double *b_hi)
{
    if (n > 2u) {
        *b_lo = ps_nj_branch_lo(n, dlh, r_lo, r_hi);
        *b_hi = dlh - *b_lo;
    } else {
        *b_lo = dlh;
        *b_hi = 0.0;
    }
}
