// gene_rule_check.cpp -- a host program of its own over pansim_amd/csrc/gene_rule.h, the arithmetic of the gene gain / loss model
// (docs/GENE_MODEL.md); tests/test_gene_rule.py builds it with the address and undefined-behaviour sanitizers and runs it; nothing
// is loaded into Python.  Random inputs against the same quantities in long double written out term by term from the 2 x 2
// transition matrix, zeros, one-hot partials, the ends of x, exact ties, and products so small that the sums are denormal.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>

#include "../pansim_amd/csrc/gene_rule.h"

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

static void random2(std::mt19937_64 &rng, double v[2], bool sparse)
{
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (int a = 0; a < 2; a++) v[a] = sparse && u(rng) < 0.3 ? 0.0 : std::ldexp(u(rng), -(int)(rng() % 40));
}

static bool near(double got, long double want, double roundings) { return std::fabs((double)(got - want)) <= roundings * EPS * (double)std::fabs(want); }

int main()
{
    std::mt19937_64 rng(20240911);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    uint64_t messages = 0, joins = 0, posts = 0, joints = 0, with_lik = 0, ties = 0, denormal = 0;

    // ---- x and y, the clamp, the leaf
    for (int it = 0; it < 2000; it++) {
        const double r = it % 9 == 0 ? 0.0 : std::ldexp(u(rng), (int)(rng() % 12) - 6), t = std::pow(10.0, -8.0 + 12.0 * u(rng));
        const double p1 = 0.05 + 0.9 * u(rng), pi[2] = { 1.0 - p1, p1 }, beta = ps_gene_beta(pi);
        const double x = ps_gene_x(r, t, beta), y = ps_gene_y(r, t, beta);
        CHECK(x >= 0.0 && x <= 1.0 && y >= 0.0 && y <= 1.0, "x = %g, y = %g of trial %d", x, y, it);
        CHECK(std::fabs((x + y) - 1.0) <= 2.0 * EPS, "x + y = %.17g of trial %d", x + y, it);
        if (r == 0.0) CHECK(x == 1.0 && y == 0.0, "a rate of 0 never changes (trial %d)", it);
        // (1 minus a sum of squares near 1: three roundings of a number below 1, absolute, and pi_0 + pi_1 is 1 within one more)
        CHECK(std::fabs((double)(beta - 2.0L * pi[0] * pi[1])) <= 4.0 * EPS, "beta of trial %d", it);
    }
    CHECK(ps_gene_x(1000.0, 1e4, 0.5) == 0.0 && ps_gene_y(1000.0, 1e4, 0.5) == 1.0, "a long branch underflows to x = 0");
    CHECK(ps_gene_y(1.0, 1e-8, 0.5) > 1.9999999e-8 && ps_gene_y(1.0, 1e-8, 0.5) < 2.0e-8, "y on the shortest branch keeps its digits");
    CHECK(ps_gene_clamp(0.0) == PS_LIK_MIN_LENGTH && ps_gene_clamp(-3.0) == PS_LIK_MIN_LENGTH && ps_gene_clamp(1e4) == 1e4 && ps_gene_clamp(1e-8) == 1e-8,
          "the clamp is below only");
    {
        double L[2];
        ps_gene_leaf(0u, L);
        CHECK(L[0] == 1.0 && L[1] == 0.0, "an absent leaf");
        ps_gene_leaf(1u, L);
        CHECK(L[0] == 0.0 && L[1] == 1.0, "a present leaf");
        ps_gene_leaf(200u, L);
        CHECK(L[0] == 0.0 && L[1] == 1.0, "any byte but 0 is present");
    }

    // ---- the messages against the matrix P[a][b] = x [a = b] + y pi_b, the join and the rescale
    for (int it = 0; it < 20000; it++) {
        double L[2], U[2], m[2], T[2];
        random2(rng, L, it % 3 == 0);
        random2(rng, U, it % 5 == 0);
        const double p1 = 0.02 + 0.96 * u(rng), pi[2] = { 1.0 - p1, p1 };
        const double x = it % 11 == 0 ? 0.0 : it % 11 == 1 ? 1.0 : it % 11 == 2 ? std::exp(-1e-8) : u(rng);
        const double y = it % 11 == 2 ? -std::expm1(-1e-8) : 1.0 - x;
        ps_gene_up(x, y, pi, L, m);
        ps_gene_down(x, y, pi, U, T);
        for (int a = 0; a < 2; a++) {
            long double up = 0.0L, dn = 0.0L;
            for (int b = 0; b < 2; b++) {
                up += ((a == b ? (long double)x : 0.0L) + (long double)y * pi[b]) * L[b];
                dn += (long double)U[b] * ((a == b ? (long double)x : 0.0L) + (long double)y * pi[a]);
            }
            CHECK(near(m[a], up, 8.0), "up[%d] of trial %d: %.17g against %.17Lg", a, it, m[a], up);
            CHECK(near(T[a], dn, 8.0), "down[%d] of trial %d: %.17g against %.17Lg", a, it, T[a], dn);
            CHECK(m[a] >= 0.0 && T[a] >= 0.0, "a negative message in trial %d", it);
        }
        CHECK(m[0] == y * (pi[0] * L[0] + pi[1] * L[1]) + x * L[0], "the association of up (trial %d)", it);
        CHECK(T[1] == (y * pi[1]) * (U[0] + U[1]) + x * U[1], "the association of down (trial %d)", it);
        messages++;
        double J[2];
        const int32_t k = ps_gene_join(m, T, J);
        const double big = J[0] > J[1] ? J[0] : J[1];
        if (m[0] * T[0] > 0.0 || m[1] * T[1] > 0.0) {
            CHECK(big >= 0.5 && big < 1.0, "the join of trial %d is not rescaled: %g", it, big);
            CHECK(std::ldexp(J[0], k) == m[0] * T[0] && std::ldexp(J[1], k) == m[1] * T[1], "the rescale of trial %d is not exact", it);
        } else
            CHECK(k == 0 && J[0] == 0.0 && J[1] == 0.0, "the join of zeros (trial %d)", it);
        // the same exponent and the same bits as ps_jc_rescale on the padded four
        double q[4] = { m[0] * T[0], m[1] * T[1], 0.0, 0.0 };
        CHECK(ps_jc_rescale(q) == k && q[0] == J[0] && q[1] == J[1], "ps_gene_rescale is ps_jc_rescale (trial %d)", it);
        joins++;
    }

    // ---- the node posterior and the state
    for (int it = 0; it < 20000; it++) {
        double T[2], ml[2], mr[2], w[2];
        random2(rng, T, it % 3 == 0);
        random2(rng, ml, it % 5 == 0);
        random2(rng, mr, it % 7 == 0);
        if (it % 4 == 1) {                                  // (every fourth trial: the two states alike, an exact tie)
            T[1] = T[0];
            ml[1] = ml[0];
            mr[1] = mr[0];
        }
        const double sum = ps_gene_node_post(T, ml, mr, w);
        CHECK(w[0] == (T[0] * ml[0]) * mr[0] && w[1] == (T[1] * ml[1]) * mr[1] && sum == w[0] + w[1], "node_post of trial %d", it);
        const double p0 = ps_subst_post_term(1.0, w[0], sum), p1 = ps_subst_post_term(1.0, w[1], sum);
        double pmax;
        const uint32_t one = ps_gene_map(p0, p1, &pmax);
        CHECK(one == (p1 > p0 ? 1u : 0u) && pmax == (p1 > p0 ? p1 : p0), "map of trial %d", it);
        if (sum > 0.0) CHECK(std::fabs((p0 + p1) - 1.0) <= 4.0 * EPS && pmax >= 0.5 - 2.0 * EPS, "posteriors of trial %d sum to %.17g", it, p0 + p1);
        else CHECK(p0 == 0.0 && p1 == 0.0 && one == 0u, "a sum of 0 adds nothing and is absent (trial %d)", it);
        if (p0 == p1) {
            CHECK(one == 0u, "an exact tie is absent (trial %d)", it);
            ties++;
        }
        posts++;
    }
    // denormal sums: three factors near 2^-350 each
    for (int it = 0; it < 2000; it++) {
        double T[2], ml[2], mr[2], w[2];
        for (int a = 0; a < 2; a++) {
            T[a] = std::ldexp(0.5 + 0.5 * u(rng), -340 - (int)(rng() % 20));
            ml[a] = std::ldexp(0.5 + 0.5 * u(rng), -350 - (int)(rng() % 20));
            mr[a] = std::ldexp(0.5 + 0.5 * u(rng), -350 - (int)(rng() % 20));
        }
        const double sum = ps_gene_node_post(T, ml, mr, w);
        CHECK(std::isfinite(sum) && sum >= 0.0 && sum < 0x1p-1022, "denormal trial %d has the sum %g", it, sum);
        const double p0 = ps_subst_post_term(1.0, w[0], sum), p1 = ps_subst_post_term(1.0, w[1], sum);
        CHECK(sum > 0.0 ? std::fabs((p0 + p1) - 1.0) <= 4.0 * EPS : p0 + p1 == 0.0, "denormal posteriors of trial %d sum to %.17g", it, p0 + p1);
        denormal += sum > 0.0;
    }

    // ---- the two directed joints against the joint of the branch's two ends, term by term
    for (int it = 0; it < 20000; it++) {
        double U[2], L[2];
        random2(rng, U, it % 3 == 0);
        random2(rng, L, it % 4 == 0);
        const double p1 = 0.02 + 0.96 * u(rng), pi[2] = { 1.0 - p1, p1 };
        const double x = it % 11 == 0 ? 0.0 : it % 11 == 1 ? 1.0 : it % 11 == 2 ? std::exp(-1e-8) : u(rng);
        const double y = it % 11 == 2 ? -std::expm1(-1e-8) : 1.0 - x;
        double gain, loss;
        ps_gene_joints(x, y, pi, U, L, &gain, &loss);
        long double all = 0.0L, j01 = 0.0L, j10 = 0.0L;
        for (int a = 0; a < 2; a++)
            for (int b = 0; b < 2; b++) {
                const long double term = (long double)U[a] * ((a == b ? (long double)x : 0.0L) + (long double)y * pi[b]) * L[b];
                all += term;
                if (a == 0 && b == 1) j01 = term;
                if (a == 1 && b == 0) j10 = term;
            }
        joints++;
        if (all == 0.0L) {
            CHECK(gain == 0.0 && loss == 0.0, "joints of trial %d with a denominator of 0: %g, %g", it, gain, loss);
            continue;
        }
        // no difference anywhere: the numerator three roundings, the denominator eight, the quotient one
        CHECK(near(gain, j01 / all, 16.0) && near(loss, j10 / all, 16.0), "joints of trial %d: %.17g, %.17g against %.17Lg, %.17Lg", it, gain, loss,
              j01 / all, j10 / all);
        CHECK(gain >= 0.0 && loss >= 0.0 && gain + loss <= 1.0 + 8.0 * EPS, "joints of trial %d outside [0, 1]", it);
        if (y == 0.0) CHECK(gain == 0.0 && loss == 0.0, "no change at x = 1 (trial %d)", it);
        with_lik++;
    }
    {
        const double pi[2] = { 0.7, 0.3 }, e0[2] = { 1.0, 0.0 }, e1[2] = { 0.0, 1.0 }, z[2] = { 0.0, 0.0 };
        double g, l;
        ps_gene_joints(0.4, 0.6, pi, e0, e1, &g, &l);
        CHECK(g == 1.0 && l == 0.0, "absent above, present below: a gain for certain, %g %g", g, l);
        ps_gene_joints(0.4, 0.6, pi, e1, e0, &g, &l);
        CHECK(g == 0.0 && l == 1.0, "present above, absent below: a loss for certain, %g %g", g, l);
        ps_gene_joints(0.4, 0.6, pi, e1, e1, &g, &l);
        CHECK(g == 0.0 && l == 0.0, "one-hot ends that agree");
        ps_gene_joints(0.4, 0.6, pi, z, e1, &g, &l);
        CHECK(g == 0.0 && l == 0.0, "a zero partial");
        ps_gene_joints(1.0, 0.0, pi, e0, e1, &g, &l);
        CHECK(g == 0.0 && l == 0.0, "a denominator of 0: an invariant class at a changing branch");
        const double tU[2] = { 0x1p-530, 0x1p-531 }, tL[2] = { 0x1p-520, 0x1p-521 };
        ps_gene_joints(0.5, 0.5, pi, tU, tL, &g, &l);
        CHECK(std::isfinite(g) && std::isfinite(l) && g >= 0.0 && l >= 0.0 && g + l <= 1.0, "denormal joints %g %g", g, l);
        const double rho[2] = { 0.25, 0.75 }, L[2] = { 0.5, 0.125 };
        CHECK(ps_gene_site(rho, L) == 0.25 * 0.5 + 0.75 * 0.125, "the gene likelihood");
    }
    // ---- the running sum with its rounding errors: thousands of non-negative terms in two orders, each within two roundings of
    // the sum in long double, where the plain sum loses tens
    for (int it = 0; it < 50; it++) {
        static double v[5000];
        long double exact = 0.0L;
        for (double &e : v) exact += e = std::ldexp(u(rng), -(int)(rng() % 30));
        double s = 0.0, c = 0.0, r = 0.0, cr = 0.0;
        for (int i = 0; i < 5000; i++) s = ps_gene_add(s, v[i], &c);
        for (int i = 5000; i-- > 0;) r = ps_gene_add(r, v[i], &cr);
        CHECK(near(s + c, exact, 2.0) && near(r + cr, exact, 2.0), "the compensated sum of trial %d: %.17g, %.17g against %.17Lg", it, s + c, r + cr, exact);
    }
    printf("%llu messages, %llu joins, %llu posteriors with %llu ties, %llu denormal sums, %llu joints, %llu with a likelihood\n",
           (unsigned long long)messages, (unsigned long long)joins, (unsigned long long)posts, (unsigned long long)ties, (unsigned long long)denormal,
           (unsigned long long)joints, (unsigned long long)with_lik);
    printf(failures ? "%d steps differ\n" : "every step matches\n", failures);
    return failures ? 1 : 0;
}
