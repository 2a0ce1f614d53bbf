// subst_rule_check.cpp -- a host program of its own over pansim_amd/csrc/subst_rule.h (tests/test_subst_rule.py builds it with the
// address and undefined-behaviour sanitizers and runs it; nothing is loaded into Python).  The plain loops over the header's
// functions, written here once more -- the up pass, the mixture, the posterior and the down pass of docs/TREE_MODEL.md -- walk
// random trees of 2 to 6 leaves with lengths from 1e-8 to 10, junk bytes, random pi (every fourth with a zero entry), rho and
// rate categories (assigned and mixture, a zero rate among them): every category's site likelihood, the mixture, the posterior,
// the posterior mean rate and the ratio of every branch against the sum over all assignments of the internal nodes; the JC69
// anchor bit for bit against jc_rule.h; the Newton step's limits; the start lengths.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../pansim_amd/csrc/subst_rule.h"

struct tree {
    uint32_t N, M;
    std::vector<uint32_t> left, right;
};

static tree random_tree(std::mt19937_64 &rng, uint32_t N)
{
    tree t{ N, N - 1, {}, {} };
    std::vector<uint32_t> nodes(N);
    for (uint32_t i = 0; i < N; i++) nodes[i] = i;
    while (nodes.size() > 1) {
        const size_t i = rng() % nodes.size();
        const uint32_t a = nodes[i];
        nodes.erase(nodes.begin() + (long)i);
        const size_t j = rng() % nodes.size();
        const uint32_t b = nodes[j];
        nodes.erase(nodes.begin() + (long)j);
        nodes.push_back(N + (uint32_t)t.left.size());
        t.left.push_back(a);
        t.right.push_back(b);
    }
    return t;
}

// the likelihood of one column in one category as the sum over all 4^M assignments with P(a | p) = (1 - x) pi_a + x [a = p] and
// the root from rho; branch `c` (if below the node count) with x replaced by xc
static double brute(const tree &t, const std::vector<uint8_t> &col, const double *x, const double pi[4], const double rho[4], uint32_t c, double xc)
{
    const uint32_t N = t.N, M = t.M;
    double total = 0.0;
    for (uint64_t code = 0; code < (1ull << (2 * M)); code++) {
        double p = rho[(code >> (2 * (M - 1))) & 3u];
        for (uint32_t k = 0; k < M; k++) {
            const uint32_t sp = (uint32_t)(code >> (2 * k)) & 3u;
            for (uint32_t ch : { t.left[k], t.right[k] }) {
                const double xx = ch == c ? xc : x[ch];
                if (ch >= N) {
                    const uint32_t sc = (uint32_t)(code >> (2 * (ch - N))) & 3u;
                    p *= (1.0 - xx) * pi[sc] + (sc == sp ? xx : 0.0);
                } else if (ps_jc_known(col[ch])) {
                    const uint32_t sc = col[ch] == 1 ? 0u : col[ch] == 2 ? 1u : col[ch] == 4 ? 2u : 3u;
                    p *= (1.0 - xx) * pi[sc] + (sc == sp ? xx : 0.0);
                }
                // (a missing leaf sums to one)
            }
        }
        total += p;
    }
    return total;
}

static int failures = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            failures++;                        \
            printf("MISMATCH " __VA_ARGS__);   \
            printf("\n");                      \
        }                                      \
    } while (0)

static void unit(std::mt19937_64 &rng, double *v, uint32_t n, bool one_zero, double floor)
{
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    for (;;) {
        double s = 0.0;
        for (uint32_t i = 0; i < n; i++) s += (v[i] = floor + uni(rng));
        if (one_zero) {
            s -= v[0];
            v[0] = 0.0;
        }
        for (uint32_t i = 0; i < n; i++) v[i] /= s;
        double again = 0.0;
        for (uint32_t i = 0; i < n; i++) again += v[i];
        if (std::fabs(again - 1.0) <= 1e-12) return;
    }
}

int main()
{
    std::mt19937_64 rng(20260202);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    const uint8_t bases[4] = { 1, 2, 4, 8 };
    uint64_t trees = 0, sites = 0, mixtures = 0, anchors = 0;
    for (uint32_t trial = 0; trial < 3000; trial++) {
        const uint32_t N = 2 + trial % 5, M = N - 1, cols = 1 + trial % 3, nodes = 2 * N - 1;
        const tree t = random_tree(rng, N);
        const bool anchor = trial % 7 == 0, assigned = trial % 2 == 1;
        const uint32_t K = anchor ? 1u : 1u + (uint32_t)(rng() % 8);
        double pi[4], rho[4], rate[8] = {}, w[8] = {};
        unit(rng, pi, 4, trial % 4 == 3, 0.05);
        unit(rng, rho, 4, false, 0.05);
        unit(rng, w, K, false, 0.05);
        for (uint32_t k = 0; k < K; k++) rate[k] = 3.0 * uni(rng);
        if (K > 2 && trial % 3 == 0) rate[0] = 0.0;
        if (anchor) {
            for (int a = 0; a < 4; a++) pi[a] = rho[a] = 0.25;
            rate[0] = w[0] = 1.0;
        }
        const double beta = ps_subst_beta(pi);
        CHECK(beta > 0.0 && beta <= 0.75, "beta %g", beta);
        std::vector<uint8_t> rows((size_t)N * cols);
        for (uint8_t &b : rows) b = uni(rng) < 0.1 ? (uint8_t)(rng() & 0xFF) : bases[rng() & 3];
        std::vector<double> used(nodes, 0.0), x((size_t)K * nodes, 1.0);
        for (uint32_t c = 0; c + 1 < nodes; c++) {
            used[c] = ps_jc_clamp(std::pow(10.0, -9.0 + 10.2 * uni(rng)));
            for (uint32_t k = 0; k < K; k++) {
                const double xx = x[(size_t)k * nodes + c] = ps_subst_x(rate[k], used[c], beta);
                CHECK(xx >= 0.0 && xx <= 1.0 && (rate[k] > 0.0 || xx == 1.0), "x of t = %g, r = %g is %g", used[c], rate[k], xx);
                if (anchor) CHECK(xx == ps_jc_x(used[c]), "the anchor's x %a against %a", xx, ps_jc_x(used[c]));
            }
        }
        std::vector<double> L((size_t)K * 4 * nodes), U(4 * nodes), Lj(4 * nodes), Uj(4 * nodes);
        std::vector<int32_t> E((size_t)K * nodes, 0), Ej(nodes, 0);
        std::vector<uint8_t> col(N);
        for (uint32_t s = 0; s < cols; s++) {
            const uint32_t cls = (uint32_t)(rng() % K), kb = assigned ? cls : 0u, ke = assigned ? cls + 1u : K;
            double mant[8] = {}, post[8] = {}, lik[8] = {};
            int32_t ex[8] = {};
            for (uint32_t i = 0; i < N; i++) col[i] = rows[(size_t)i * cols + s];
            for (uint32_t k = kb; k < ke; k++) {
                double *Lk = &L[(size_t)k * 4 * nodes];
                int32_t *Ek = &E[(size_t)k * nodes];
                const double *xk = &x[(size_t)k * nodes];
                for (uint32_t i = 0; i < N; i++) ps_jc_leaf(col[i], &Lk[4 * i]);
                for (uint32_t j = 0; j < M; j++) {
                    const uint32_t l = t.left[j], r = t.right[j];
                    double ml[4], mr[4];
                    ps_subst_up(xk[l], pi, &Lk[4 * l], ml);
                    ps_subst_up(xk[r], pi, &Lk[4 * r], mr);
                    Ek[N + j] = (Ek[l] + Ek[r]) + ps_jc_join(ml, mr, &Lk[4 * (N + j)]);
                    if (anchor) {
                        double jl[4], jr[4];
                        if (j == 0)
                            for (uint32_t i = 0; i < N; i++) ps_jc_leaf(col[i], &Lj[4 * i]);
                        ps_jc_message(xk[l], &Lj[4 * l], jl);
                        ps_jc_message(xk[r], &Lj[4 * r], jr);
                        Ej[N + j] = (Ej[l] + Ej[r]) + ps_jc_join(jl, jr, &Lj[4 * (N + j)]);
                        CHECK(memcmp(&Lj[4 * (N + j)], &Lk[4 * (N + j)], 32) == 0 && Ej[N + j] == Ek[N + j], "the anchor's partial of node %u", N + j);
                    }
                }
                mant[k] = ps_subst_site(rho, &Lk[4 * (nodes - 1)]);
                ex[k] = Ek[nodes - 1];
                lik[k] = brute(t, col, xk, pi, rho, nodes, 0.0);
                CHECK(std::fabs(std::ldexp(mant[k], ex[k]) - lik[k]) <= 1e-12 * lik[k], "category %u: %g against %g", k, std::ldexp(mant[k], ex[k]), lik[k]);
                if (anchor) CHECK(mant[k] == ps_jc_site(&Lj[4 * (nodes - 1)]), "the anchor's mantissa");
            }
            double sm, sr, want = 0.0, want_rate = 0.0;
            int32_t se;
            if (assigned) {
                sm = mant[cls];
                se = ex[cls];
                sr = rate[cls];
                post[cls] = 1.0;
                want = lik[cls];
                want_rate = rate[cls];
            } else {
                sm = ps_subst_mix(K, w, mant, ex, &se, post);
                sr = ps_subst_mean_rate(K, post, rate);
                for (uint32_t k = 0; k < K; k++) want += w[k] * lik[k];
                double psum = 0.0;
                for (uint32_t k = 0; k < K; k++) {
                    CHECK(std::fabs(post[k] - w[k] * lik[k] / want) <= 1e-12, "posterior of category %u: %g against %g", k, post[k], w[k] * lik[k] / want);
                    want_rate += w[k] * lik[k] / want * rate[k];
                    psum += post[k];
                }
                CHECK(std::fabs(psum - 1.0) <= 1e-14, "the posterior sums to %.17g", psum);
                if (K == 1) CHECK(sm == mant[0] && se == ex[0] && post[0] == 1.0, "K = 1 returns the category's own pair");
                mixtures++;
            }
            CHECK((want > 0.0 || (assigned && rate[cls] == 0.0)) && std::fabs(std::ldexp(sm, se) - want) <= 1e-12 * want, "site likelihood %g against %g", std::ldexp(sm, se), want);
            CHECK(std::fabs(sr - want_rate) <= 1e-12 * want_rate + 1e-300, "mean rate %g against %g", sr, want_rate);
            // the down pass: the ratio of every branch and category against A = l(x_c = 0), A + B = l(x_c = 1)
            for (uint32_t k = kb; k < ke; k++) {
                const double *Lk = &L[(size_t)k * 4 * nodes], *xk = &x[(size_t)k * nodes];
                for (uint32_t j = M; j-- > 0;) {
                    const uint32_t l = t.left[j], r = t.right[j], c = N + j;
                    double T[4] = { rho[0], rho[1], rho[2], rho[3] }, ml[4], mr[4];
                    if (j != M - 1) ps_subst_down(xk[c], pi, &U[4 * c], T);
                    ps_subst_up(xk[l], pi, &Lk[4 * l], ml);
                    ps_subst_up(xk[r], pi, &Lk[4 * r], mr);
                    (void)ps_jc_join(mr, T, &U[4 * l]);
                    (void)ps_jc_join(ml, T, &U[4 * r]);
                    if (anchor) {
                        double Tj[4] = { 1.0, 1.0, 1.0, 1.0 }, jl[4], jr[4];
                        if (j != M - 1) ps_jc_message(xk[c], &Uj[4 * c], Tj);
                        ps_jc_message(xk[l], &Lj[4 * l], jl);
                        ps_jc_message(xk[r], &Lj[4 * r], jr);
                        (void)ps_jc_join(jr, Tj, &Uj[4 * l]);
                        (void)ps_jc_join(jl, Tj, &Uj[4 * r]);
                    }
                    for (uint32_t ch : { l, r }) {
                        const double rr = ps_subst_ratio(xk[ch], pi, &U[4 * ch], &Lk[4 * ch]);
                        if (anchor) {
                            const double rj = ps_jc_ratio(xk[ch], &Uj[4 * ch], &Lj[4 * ch]);
                            CHECK(memcmp(&rr, &rj, 8) == 0, "the anchor's ratio of branch %u: %a against %a", ch, rr, rj);
                            anchors++;
                        }
                        if (lik[k] == 0.0) {          // (an invariant category at a variable site: no likelihood, no term)
                            CHECK(rate[k] == 0.0 && ps_subst_dterm(post[k], rate[k], xk[ch], rr) == 0.0 && ps_subst_qterm(post[k], rate[k], xk[ch], rr) == 0.0,
                                  "a category without likelihood adds a term");
                            continue;
                        }
                        const double A = brute(t, col, xk, pi, rho, ch, 0.0), AB = brute(t, col, xk, pi, rho, ch, 1.0);
                        CHECK(std::fabs(rr - (AB - A) / lik[k]) <= 1e-10 * (std::fabs(A) + std::fabs(AB)) / lik[k], "ratio of branch %u: %g against %g", ch, rr,
                              (AB - A) / lik[k]);
                        const double dt = ps_subst_dterm(post[k], rate[k], xk[ch], rr), qt = ps_subst_qterm(post[k], rate[k], xk[ch], rr);
                        CHECK(rate[k] == 0.0 ? (dt == 0.0 && qt == 0.0)
                                             : (dt == post[k] * ((rate[k] * xk[ch]) * rr) && std::fabs(qt - rate[k] * dt) <= 1e-15 * std::fabs(qt)),
                              "the terms of branch %u", ch);
                    }
                }
            }
        }
        trees++;
        sites += cols;
    }
    // the derivatives from the sums, the Newton step's limits, the start lengths
    CHECK(ps_subst_dt(0.75, 3.0) == -4.0 && ps_subst_dt2(0.5, 3.0, 1.0) == 8.0, "derivatives from the sums");
    for (int i = 0; i < 2000; i++) {
        const double t0 = ps_jc_clamp(std::pow(10.0, -9.0 + 10.2 * uni(rng))), gt = 2000.0 * (uni(rng) - 0.5), ht = 2000.0 * (uni(rng) - 0.7);
        const double lam = std::ldexp(1.0, -(int)(rng() % 5)), t1 = ps_subst_newton(t0, gt, ht, lam);
        CHECK(t1 >= PS_LIK_MIN_LENGTH && t1 <= PS_LIK_MAX_LENGTH && t1 >= t0 * 0.5 * (1.0 - 1e-15) && t1 <= t0 + std::fmax(t0, 1e-3) * (1.0 + 1e-15),
              "a step from %g to %g is outside its limits", t0, t1);
        CHECK((gt > 0.0) == (t1 > t0) || t1 == t0 || t0 == PS_LIK_MAX_LENGTH || t0 == PS_LIK_MIN_LENGTH, "a step against the gradient");
    }
    const double sim[4] = { 0.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0 }, bs = ps_subst_beta(sim);
    CHECK(std::fabs(bs - 2.0 / 3.0) < 1e-15, "beta of the simulator's pi");
    CHECK(ps_subst_length_from_changes(0, 100, bs) == 0.0 && ps_subst_length_from_changes(66, 100, bs) == PS_LIK_MAX_LENGTH &&
              ps_subst_length_from_changes(65, 100, bs) < PS_LIK_MAX_LENGTH, "start lengths and their cap at 0.98 beta");
    CHECK(std::fabs(ps_subst_length_from_changes(30, 100, bs) + bs * std::log(1.0 - 0.3 / bs)) < 1e-15, "start length of p = 0.3");
    CHECK(ps_subst_length_from_changes(5, 0, bs) == PS_LIK_MIN_LENGTH, "start length without sites");
    CHECK(std::fabs(ps_subst_length_from_changes(30, 100, 0.75) - ps_jc_length_from_changes(30, 100)) < 1e-15, "the JC69 correction");
    printf("%llu trees, %llu sites, %llu mixtures, %llu anchored ratios\n", (unsigned long long)trees, (unsigned long long)sites,
           (unsigned long long)mixtures, (unsigned long long)anchors);
    if (failures) {
        printf("%d mismatches\n", failures);
        return 1;
    }
    printf("every step matches\n");
    return 0;
}
