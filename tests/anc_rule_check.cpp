// anc_rule_check.cpp -- a host program of its own over the three functions pansim_amd/csrc/subst_rule.h adds for the marginal
// ancestral states (docs/ANCESTRAL_STATES.md): ps_subst_node_post, ps_subst_pdiff and ps_subst_map, with ps_subst_post_term
// (tests/test_anc_rule.py builds it with the address and undefined-behaviour sanitizers and runs it; nothing is loaded into
// Python).  Random inputs against the same quantities in long double written out term by term, zeros, one-hot partials, the ends
// of x, exact ties, and products so small that the sums are denormal.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>

#include "../pansim_amd/csrc/subst_rule.h"

static int failures = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            printf("MISMATCH " __VA_ARGS__);   \
            printf("\n");                      \
            failures++;                        \
        }                                      \
    } while (0)

static const double EPS = 0x1p-53;

static void random4(std::mt19937_64 &rng, double v[4], bool sparse)
{
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (int a = 0; a < 4; a++) v[a] = sparse && u(rng) < 0.3 ? 0.0 : std::ldexp(u(rng), -(int)(rng() % 40));
}

static void random_pi(std::mt19937_64 &rng, double pi[4], bool zero)
{
    std::uniform_real_distribution<double> u(0.05, 1.0);
    double s = 0.0;
    for (int a = 0; a < 4; a++) s += pi[a] = (zero && a == 0) ? 0.0 : u(rng);
    for (int a = 0; a < 4; a++) pi[a] /= s;
}

int main()
{
    std::mt19937_64 rng(20240607);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    uint64_t posts = 0, diffs = 0, maps = 0, ties = 0, denormal = 0;

    // ---- ps_subst_node_post and ps_subst_post_term
    for (int it = 0; it < 20000; it++) {
        double T[4], ml[4], mr[4], w[4];
        random4(rng, T, it % 3 == 0);
        random4(rng, ml, it % 5 == 0);
        random4(rng, mr, it % 7 == 0);
        const double sum = ps_subst_node_post(T, ml, mr, w);
        long double exact = 0.0L;
        for (int a = 0; a < 4; a++) {
            CHECK(w[a] == (T[a] * ml[a]) * mr[a], "node_post w[%d] of trial %d", a, it);
            exact += (long double)T[a] * ml[a] * mr[a];
        }
        CHECK(sum == (w[0] + w[1]) + (w[2] + w[3]), "node_post association of trial %d", it);
        CHECK(std::fabs((double)(sum - exact)) <= 6.0 * EPS * (double)exact, "node_post sum of trial %d: %.17g against %.17Lg", it, sum, exact);
        double total = 0.0;
        for (int a = 0; a < 4; a++) {
            const double p = ps_subst_post_term(1.0, w[a], sum);
            CHECK(p >= 0.0 && p <= 1.0, "posterior %g of trial %d outside [0, 1]", p, it);
            if (sum > 0.0) CHECK(p == w[a] / sum, "post_term with post = 1 is the quotient itself (trial %d)", it);
            const double half = ps_subst_post_term(0.5, w[a], sum);
            CHECK(half == (sum > 0.0 ? 0.5 * (w[a] / sum) : 0.0), "post_term association of trial %d", it);
            total += p;
        }
        if (sum > 0.0) CHECK(std::fabs(total - 1.0) <= 8.0 * EPS, "posteriors of trial %d sum to %.17g", it, total);
        else CHECK(total == 0.0, "a sum of 0 adds nothing (trial %d)", it);
        posts++;
    }
    {
        // zeros: every product 0 -> the sum is 0 and nothing is added, whatever the posterior of the category
        const double z[4] = { 0.0, 0.0, 0.0, 0.0 }, o[4] = { 1.0, 1.0, 1.0, 1.0 };
        double w[4];
        CHECK(ps_subst_node_post(z, o, o, w) == 0.0 && w[0] == 0.0 && w[3] == 0.0, "zeros");
        CHECK(ps_subst_post_term(0.7, 0.0, 0.0) == 0.0 && ps_subst_post_term(1.0, 1.0, 0.0) == 0.0, "post_term at sum 0");
        // disjoint supports: T allows only base 0, the children only base 1
        const double t0[4] = { 1.0, 0.0, 0.0, 0.0 }, c1[4] = { 0.0, 0.5, 0.0, 0.0 };
        CHECK(ps_subst_node_post(t0, c1, c1, w) == 0.0, "disjoint supports");
    }
    // denormal sums: three factors near 2^-360 each; the products are denormal or 0, the quotients still posteriors
    for (int it = 0; it < 2000; it++) {
        double T[4], ml[4], mr[4], w[4];
        for (int a = 0; a < 4; a++) {
            T[a] = std::ldexp(0.5 + 0.5 * u(rng), -340 - (int)(rng() % 20));
            ml[a] = std::ldexp(0.5 + 0.5 * u(rng), -350 - (int)(rng() % 20));
            mr[a] = std::ldexp(0.5 + 0.5 * u(rng), -350 - (int)(rng() % 20));
        }
        const double sum = ps_subst_node_post(T, ml, mr, w);
        CHECK(std::isfinite(sum) && sum >= 0.0 && sum < 0x1p-1022, "denormal trial %d has the sum %g", it, sum);
        double total = 0.0, pmax;
        double p[4];
        for (int a = 0; a < 4; a++) {
            p[a] = ps_subst_post_term(1.0, w[a], sum);
            CHECK(std::isfinite(p[a]) && p[a] >= 0.0 && p[a] <= 1.0, "denormal posterior %g of trial %d", p[a], it);
            total += p[a];
        }
        // (a sum of up to four denormals is exact: the quotients sum to 1 within their own roundings, or nothing was added)
        CHECK(sum > 0.0 ? std::fabs(total - 1.0) <= 8.0 * EPS : total == 0.0, "denormal posteriors of trial %d sum to %.17g", it, total);
        const uint32_t best = ps_subst_map(p, &pmax);
        CHECK(best < 4u && pmax == p[best], "denormal map of trial %d", it);
        denormal += sum > 0.0;
    }

    // ---- ps_subst_pdiff
    for (int it = 0; it < 20000; it++) {
        double U[4], L[4], pi[4];
        random4(rng, U, it % 3 == 0);
        random4(rng, L, it % 4 == 0);
        random_pi(rng, pi, it % 4 == 1);
        const double x = it % 11 == 0 ? 0.0 : it % 11 == 1 ? 1.0 : it % 11 == 2 ? std::exp(-1e-8) : u(rng);
        const double got = ps_subst_pdiff(x, pi, U, L);
        // the joint of the two ends, P[a][b] = x [a = b] + (1 - x) pi_b, term by term in long double
        long double all = 0.0L, off = 0.0L, A = 0.0L;
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) {
                const long double term = (long double)U[a] * ((a == b ? (long double)x : 0.0L) + (1.0L - x) * pi[b]) * L[b];
                all += term;
                if (a != b) off += term;
                A += (long double)U[a] * pi[b] * L[b];
            }
        CHECK(got >= 0.0 && got <= 1.0 + 8.0 * EPS, "pdiff %g of trial %d outside [0, 1]", got, it);
        if (all == 0.0L) {
            CHECK(got == 0.0, "pdiff of trial %d with a denominator of 0 is %g", it, got);
            continue;
        }
        // the only difference is A - S: A carries six roundings, S four and the difference one, an absolute error of at most
        // 11 roundings of A, times (1 - x) / denominator; the factors around it (1 - x, the product, the denominator's eight
        // roundings, the quotient) add 11 relative ones: 16 of each bounds both
        const long double want = off / all, bound = 16.0L * EPS * ((1.0L - x) * A / all + want);
        CHECK(std::fabs((double)(got - want)) <= (double)bound, "pdiff of trial %d: %.17g against %.17Lg (bound %.3Lg)", it, got, want, bound);
        if (x == 1.0) CHECK(got == 0.0, "pdiff at x = 1 is %g", got);
        diffs++;
    }
    {
        const double pi[4] = { 0.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0 }, jc[4] = { 0.25, 0.25, 0.25, 0.25 };
        const double z[4] = { 0.0, 0.0, 0.0, 0.0 };
        for (int a = 0; a < 4; a++) {
            double e[4] = { 0.0, 0.0, 0.0, 0.0 };
            e[a] = 1.0;
            // both ends surely the same base: no difference, and never a negative one
            CHECK(ps_subst_pdiff(0.3, jc, e, e) == 0.0, "one-hot ends, base %d", a);
            CHECK(ps_subst_pdiff(0.3, pi, e, e) == 0.0, "one-hot ends under the simulator's pi, base %d", a);
            CHECK(ps_subst_pdiff(0.3, jc, z, e) == 0.0 && ps_subst_pdiff(0.3, jc, e, z) == 0.0, "a zero partial, base %d", a);
            // the ends surely different: a difference for certain
            double o[4] = { 0.0, 0.0, 0.0, 0.0 };
            o[(a + 1) % 4] = 1.0;
            if ((a + 1) % 4 != 0) CHECK(ps_subst_pdiff(0.3, pi, e, o) == 1.0, "unlike one-hot ends, base %d", a);
        }
        // the lost base below a branch that was surely hit is impossible under the simulator's pi: a likelihood of 0
        const double e0[4] = { 1.0, 0.0, 0.0, 0.0 }, e1[4] = { 0.0, 1.0, 0.0, 0.0 };
        CHECK(ps_subst_pdiff(0.0, pi, e1, e0) == 0.0, "a denominator of 0");
        // tiny partials: the denominator is denormal, the quotient still a probability
        const double tU[4] = { 0x1p-530, 0x1p-531, 0x1p-532, 0x1p-533 }, tL[4] = { 0x1p-520, 0x1p-521, 0x1p-519, 0x1p-522 };
        const double tiny = ps_subst_pdiff(0.5, jc, tU, tL);
        CHECK(std::isfinite(tiny) && tiny >= 0.0 && tiny <= 1.0, "denormal pdiff %g", tiny);
    }

    // ---- ps_subst_map
    for (int it = 0; it < 20000; it++) {
        double p[4], pmax = -1.0;
        for (int a = 0; a < 4; a++) p[a] = it % 2 ? (double)(rng() % 3) * 0.25 : u(rng);       // (odd trials: many exact ties)
        const uint32_t best = ps_subst_map(p, &pmax);
        CHECK(best < 4u && pmax == p[best], "map returns its own maximum (trial %d)", it);
        bool tie = false;
        for (uint32_t a = 0; a < 4u; a++) {
            CHECK(p[a] <= pmax, "map missed a larger entry (trial %d)", it);
            if (a < best) CHECK(p[a] < pmax, "a tie does not go to the lowest index (trial %d)", it);
            tie = tie || (a != best && p[a] == pmax);
        }
        ties += tie;
        maps++;
    }
    {
        const double q[4] = { 0.25, 0.25, 0.25, 0.25 }, z[4] = { 0.0, 0.0, 0.0, 0.0 }, last[4] = { 0.1, 0.2, 0.3, 0.4 };
        const double mid[4] = { 0.2, 0.4, 0.4, 0.0 };
        double m;
        CHECK(ps_subst_map(q, &m) == 0u && m == 0.25, "four equal entries");
        CHECK(ps_subst_map(z, &m) == 0u && m == 0.0, "four zeros");
        CHECK(ps_subst_map(last, &m) == 3u && m == 0.4, "the last entry");
        CHECK(ps_subst_map(mid, &m) == 1u && m == 0.4, "a tie in the middle");
    }
    printf("%llu posteriors, %llu denormal sums, %llu differences, %llu maps with %llu ties\n", (unsigned long long)posts, (unsigned long long)denormal,
           (unsigned long long)diffs, (unsigned long long)maps, (unsigned long long)ties);
    printf(failures ? "%d steps differ\n" : "every step matches\n", failures);
    return failures ? 1 : 0;
}
