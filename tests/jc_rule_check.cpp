// jc_rule_check.cpp -- a host program of its own over pansim_amd/csrc/jc_rule.h (tests/test_jc_rule.py builds it with the address
// and undefined-behaviour sanitizers and runs it; nothing is loaded into Python).  The plain loops over the header's functions,
// written here once more -- the up pass, the down pass and the branch-length optimiser of docs/TREE_LIKELIHOOD.md -- walk random
// trees of 2 to 9 leaves with lengths from 1e-8 to 10 and junk bytes: the site likelihood and A, A + B of every branch against
// the sum over all assignments of the internal nodes, the invariants of the rescaling, the limits of a Newton step, and an
// optimiser whose lnL never falls and whose lengths stay inside the bounds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../pansim_amd/csrc/jc_rule.h"

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

// the likelihood of one column as the sum over all 4^M assignments; branch `c` (if below the node count) with x replaced by xc
static double brute(const tree &t, const std::vector<uint8_t> &col, const std::vector<double> &x, uint32_t c, double xc)
{
    const uint32_t N = t.N, M = t.M;
    double total = 0.0;
    for (uint64_t code = 0; code < (1ull << (2 * M)); code++) {
        double p = 0.25;
        for (uint32_t k = 0; k < M; k++) {
            const uint32_t sp = (uint32_t)(code >> (2 * k)) & 3u;
            for (uint32_t ch : { t.left[k], t.right[k] }) {
                const double xx = ch == c ? xc : x[ch], same = (1.0 + 3.0 * xx) / 4.0, diff = (1.0 - xx) / 4.0;
                if (ch >= N) p *= ((uint32_t)(code >> (2 * (ch - N))) & 3u) == sp ? same : diff;
                else if (ps_jc_known(col[ch])) p *= col[ch] == (1u << sp) ? same : diff;
                // (a missing leaf sums to one)
            }
        }
        total += p;
    }
    return total;
}

struct pass_out {
    double lnl = 0.0;
    std::vector<double> g, h;
};

static int failures = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            failures++;                        \
            printf("MISMATCH " __VA_ARGS__);   \
            printf("\n");                      \
        }                                      \
    } while (0)

// one pass over rows (individual-major, cols columns); verify: against the brute force
static pass_out pass(const tree &t, const std::vector<uint8_t> &rows, uint32_t cols, const std::vector<double> &x, bool verify)
{
    const uint32_t N = t.N, M = t.M, nodes = N + M;
    pass_out out;
    out.g.assign(nodes, 0.0);
    out.h.assign(nodes, 0.0);
    std::vector<double> L(4 * nodes), U(4 * nodes);
    std::vector<int32_t> E(nodes, 0);
    std::vector<uint8_t> col(N);
    for (uint32_t s = 0; s < cols; s++) {
        for (uint32_t i = 0; i < N; i++) {
            col[i] = rows[(size_t)i * cols + s];
            ps_jc_leaf(col[i], &L[4 * i]);
        }
        for (uint32_t k = 0; k < M; k++) {
            const uint32_t l = t.left[k], r = t.right[k];
            double ml[4], mr[4];
            ps_jc_message(x[l], &L[4 * l], ml);
            ps_jc_message(x[r], &L[4 * r], mr);
            E[N + k] = (E[l] + E[r]) + ps_jc_join(ml, mr, &L[4 * (N + k)]);
            double mx = 0.0;
            for (int a = 0; a < 4; a++) mx = std::fmax(mx, L[4 * (N + k) + a]);
            CHECK(mx >= 0.5 && mx < 1.0, "rescale: the largest entry of node %u is %g", N + k, mx);
            for (int a = 0; a < 4; a++) CHECK(L[4 * (N + k) + a] > 0.0, "partial of node %u not positive", N + k);
        }
        const double mant = ps_jc_site(&L[4 * (nodes - 1)]);
        const int32_t ex = E[nodes - 1];
        out.lnl += ps_jc_site_ln(mant, ex);
        const double lik = verify ? brute(t, col, x, nodes, 0.0) : 0.0;
        if (verify) CHECK(std::fabs(std::ldexp(mant, ex) - lik) <= 1e-12 * lik, "site likelihood %g against %g", std::ldexp(mant, ex), lik);
        for (uint32_t k = M; k-- > 0;) {
            const uint32_t l = t.left[k], r = t.right[k], c = N + k;
            double T[4] = { 1.0, 1.0, 1.0, 1.0 }, ml[4], mr[4];
            if (k != M - 1) ps_jc_message(x[c], &U[4 * c], T);
            ps_jc_message(x[l], &L[4 * l], ml);
            ps_jc_message(x[r], &L[4 * r], mr);
            (void)ps_jc_join(mr, T, &U[4 * l]);
            (void)ps_jc_join(ml, T, &U[4 * r]);
            for (uint32_t ch : { l, r }) {
                const double rr = ps_jc_ratio(x[ch], &U[4 * ch], &L[4 * ch]);
                out.g[ch] += rr;
                out.h[ch] += rr * rr;
                if (verify) {
                    const double A = brute(t, col, x, ch, 0.0), AB = brute(t, col, x, ch, 1.0);
                    CHECK(std::fabs(rr - (AB - A) / lik) <= 1e-10 * (std::fabs(A) + std::fabs(AB)) / lik, "r of branch %u: %g against %g", ch, rr,
                          (AB - A) / lik);
                }
            }
        }
    }
    return out;
}

int main()
{
    std::mt19937_64 rng(20260101);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    const uint8_t bases[4] = { 1, 2, 4, 8 };
    uint64_t trees = 0, sites = 0, rounds_all = 0, rollbacks_all = 0;
    for (uint32_t trial = 0; trial < 3000; trial++) {
        const uint32_t N = 2 + trial % 8, cols = 1 + trial % 5, nodes = 2 * N - 1;
        const tree t = random_tree(rng, N);
        std::vector<uint8_t> rows((size_t)N * cols);
        for (uint8_t &b : rows) b = uni(rng) < 0.1 ? (uint8_t)(rng() & 0xFF) : bases[rng() & 3];
        std::vector<double> len(nodes), x(nodes, 1.0);
        for (uint32_t c = 0; c < nodes; c++) len[c] = std::pow(10.0, -9.0 + 10.2 * uni(rng));
        for (uint32_t c = 0; c + 1 < nodes; c++) {
            const double used = ps_jc_clamp(len[c]);
            CHECK(used >= PS_LIK_MIN_LENGTH && used <= PS_LIK_MAX_LENGTH, "clamp");
            x[c] = ps_jc_x(used);
            CHECK(x[c] > 0.0 && x[c] < 1.0, "x of %g is %g", used, x[c]);
        }
        const bool verify = N <= 6;                 // (4^5 assignments a column and branch at the most)
        pass_out cur = pass(t, rows, cols, x, verify);
        CHECK(std::isfinite(cur.lnl) && cur.lnl <= 0.0, "lnL %g", cur.lnl);
        trees++;
        sites += cols;
        if (trial % 3) continue;
        // the optimiser, restated: the root rule, damped Newton steps on all other branches at once, rollbacks
        std::vector<double> used(nodes, 0.0), cand, cx(nodes, 1.0);
        for (uint32_t c = 0; c + 1 < nodes; c++) used[c] = ps_jc_clamp(len[c]);
        const uint32_t rl = t.left[N - 2], rr = t.right[N - 2];
        used[rl] = ps_jc_clamp(used[rl] + used[rr]);
        used[rr] = PS_LIK_MIN_LENGTH;
        for (uint32_t c = 0; c + 1 < nodes; c++) x[c] = ps_jc_x(used[c]);
        cur = pass(t, rows, cols, x, false);
        double lambda = 1.0;
        uint32_t rounds = 0;
        while (rounds < 12 && lambda >= 0x1p-20) {
            cand = used;
            for (uint32_t c = 0; c + 1 < nodes; c++) {
                if (c == rr) continue;
                cand[c] = ps_jc_newton(used[c], x[c], cur.g[c], cur.h[c], lambda);
                CHECK(cand[c] >= PS_LIK_MIN_LENGTH && cand[c] <= PS_LIK_MAX_LENGTH, "a step leaves the bounds: %g", cand[c]);
                CHECK(cand[c] >= used[c] * 0.5 * (1.0 - 1e-15) && cand[c] <= used[c] + std::fmax(used[c], 1e-3) * (1.0 + 1e-15),
                      "a step from %g to %g is outside its limits", used[c], cand[c]);
            }
            for (uint32_t c = 0; c + 1 < nodes; c++) cx[c] = ps_jc_x(cand[c]);
            pass_out next = pass(t, rows, cols, cx, false);
            if (next.lnl < cur.lnl) {
                rollbacks_all++;
                lambda *= 0.5;
                continue;
            }
            if (next.lnl == cur.lnl) break;
            CHECK(next.lnl > cur.lnl, "an accepted round lowers lnL");
            rounds++;
            used = cand;
            x = cx;
            cur = next;
            lambda = 1.0;
        }
        rounds_all += rounds;
    }
    // start lengths: the Jukes-Cantor correction and its cap
    CHECK(ps_jc_length_from_changes(0, 100) == 0.0 && ps_jc_length_from_changes(74, 100) == PS_LIK_MAX_LENGTH, "start lengths");
    CHECK(std::fabs(ps_jc_length_from_changes(30, 100) + 0.75 * std::log(0.6)) < 1e-15, "start length of p = 0.3");
    CHECK(ps_jc_length_from_changes(5, 0) == PS_LIK_MIN_LENGTH, "start length without sites");
    printf("%llu trees, %llu sites, %llu rounds, %llu rollbacks\n", (unsigned long long)trees, (unsigned long long)sites,
           (unsigned long long)rounds_all, (unsigned long long)rollbacks_all);
    if (failures) {
        printf("%d mismatches\n", failures);
        return 1;
    }
    printf("every step matches\n");
    return 0;
}
