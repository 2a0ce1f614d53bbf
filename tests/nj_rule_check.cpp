// nj_rule_check.cpp -- a host program of its own over pansim_amd/csrc/nj_rule.h (tests/test_neighbour_joining.py builds it with the
// address and undefined-behaviour sanitizers and runs it; nothing is loaded into Python).  The plain loop over the header's
// functions, written here once more, recomputes the five-taxon example of the Wikipedia article on neighbour joining and
// recovers planted additive trees with integer branches exactly: every path length of the joined tree equals its input.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../pansim_amd/csrc/nj_rule.h"

struct joined {
    std::vector<uint32_t> left, right;
    std::vector<double> len_left, len_right;
};

// D: n x n, symmetric, zero diagonal (changed in place); ids are rows
static joined join(std::vector<double> D, uint32_t N)
{
    joined out;
    std::vector<double> r(N, 0.0);
    std::vector<uint32_t> alive(N), node(N);
    for (uint32_t i = 0; i < N; i++) {
        alive[i] = node[i] = i;
        for (uint32_t k = 0; k < N; k++)
            if (k != i) r[i] += D[(size_t)i * N + k];
    }
    for (uint32_t t = 0; t + 1 < N; t++) {
        const uint32_t n = N - t;
        ps_nj_key best = { 0.0, PS_NJ_NONE, PS_NJ_NONE };
        for (size_t x = 0; x < alive.size(); x++)
            for (size_t y = x + 1; y < alive.size(); y++) {
                const ps_nj_key e = { ps_nj_q(n, D[(size_t)alive[x] * N + alive[y]], r[alive[x]], r[alive[y]]), alive[x], alive[y] };
                if (best.lo == PS_NJ_NONE || ps_nj_less(e, best)) best = e;
            }
        const uint32_t lo = best.lo, hi = best.hi;
        const double dlh = D[(size_t)lo * N + hi], r_lo = r[lo], r_hi = r[hi];
        double b_lo, b_hi;
        ps_nj_branches(n, dlh, r_lo, r_hi, &b_lo, &b_hi);
        out.left.push_back(node[lo]);
        out.right.push_back(node[hi]);
        out.len_left.push_back(b_lo);
        out.len_right.push_back(b_hi);
        node[lo] = N + t;
        for (uint32_t k : alive) {
            if (k == lo || k == hi) continue;
            const double dlk = D[(size_t)lo * N + k], dhk = D[(size_t)hi * N + k], duk = ps_nj_duk(dlk, dhk, dlh);
            r[k] = ps_nj_r_other(r[k], dlk, dhk, duk);
            D[(size_t)lo * N + k] = D[(size_t)k * N + lo] = duk;
        }
        r[lo] = ps_nj_r_joined(n, r_lo, r_hi, dlh);
        alive.erase(std::find(alive.begin(), alive.end(), hi));
    }
    return out;
}

// the path metric of a join list over N leaves
static std::vector<double> paths(const joined &t, uint32_t N)
{
    std::vector<uint32_t> parent(2 * N - 1, PS_NJ_NONE);
    std::vector<double> above(2 * N - 1, 0.0);
    for (uint32_t k = 0; k + 1 < N; k++) {
        parent[t.left[k]] = parent[t.right[k]] = N + k;
        above[t.left[k]] = t.len_left[k];
        above[t.right[k]] = t.len_right[k];
    }
    std::vector<double> D((size_t)N * N, 0.0);
    for (uint32_t i = 0; i < N; i++)
        for (uint32_t j = i + 1; j < N; j++) {
            uint32_t a = i, b = j;
            double s = 0.0;
            while (a != b) {                              // (a parent's number is above its children's)
                if (a < b) { s += above[a]; a = parent[a]; }
                else { s += above[b]; b = parent[b]; }
            }
            D[(size_t)i * N + j] = D[(size_t)j * N + i] = s;
        }
    return D;
}

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint32_t draw(uint32_t below)
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((state >> 33) % below);
}

int main()
{
    int bad = 0;
    {
        const double d[5][5] = { { 0, 5, 9, 9, 8 }, { 5, 0, 10, 10, 9 }, { 9, 10, 0, 8, 7 }, { 9, 10, 8, 0, 3 }, { 8, 9, 7, 3, 0 } };
        std::vector<double> D(25);
        for (int i = 0; i < 5; i++)
            for (int j = 0; j < 5; j++) D[i * 5 + j] = d[i][j];
        const joined t = join(D, 5);
        const uint32_t left[4] = { 0, 5, 6, 7 }, right[4] = { 1, 2, 3, 4 };
        const double ll[4] = { 2, 3, 2, 1 }, lr[4] = { 3, 4, 2, 0 };
        for (int k = 0; k < 4; k++)
            if (t.left[k] != left[k] || t.right[k] != right[k] || t.len_left[k] != ll[k] || t.len_right[k] != lr[k]) {
                printf("BAD five taxa, join %d: (%u:%g, %u:%g)\n", k, t.left[k], t.len_left[k], t.right[k], t.len_right[k]);
                bad++;
            }
    }
    for (uint32_t N : { 2u, 3u, 4u, 9u, 33u, 70u }) {
        joined planted;
        std::vector<uint32_t> nodes(N);
        for (uint32_t i = 0; i < N; i++) nodes[i] = i;
        for (uint32_t k = 0; k + 1 < N; k++) {
            uint32_t pick[2];
            for (uint32_t &p : pick) {
                const uint32_t at = draw((uint32_t)nodes.size());
                p = nodes[at];
                nodes.erase(nodes.begin() + at);
            }
            planted.left.push_back(pick[0]);
            planted.right.push_back(pick[1]);
            planted.len_left.push_back(1.0 + draw(9));
            planted.len_right.push_back(1.0 + draw(9));
            nodes.push_back(N + k);
        }
        const std::vector<double> D = paths(planted, N);
        const joined t = join(D, N);
        const std::vector<double> back = paths(t, N);
        double total = 0.0, want = 0.0;
        for (uint32_t k = 0; k + 1 < N; k++) {
            total += t.len_left[k] + t.len_right[k];
            want += planted.len_left[k] + planted.len_right[k];
            if (t.len_left[k] < 0.0 || t.len_right[k] < 0.0) {
                printf("BAD N = %u, join %u: a negative branch\n", N, k);
                bad++;
            }
        }
        if (back != D || total != want) {
            printf("BAD N = %u: the joined tree's paths differ from the planted ones (length %g, planted %g)\n", N, total, want);
            bad++;
        } else printf("N = %u: %u joins, every path exact, length %g\n", N, N - 1, total);
    }
    if (bad) return 1;
    printf("the rule holds\n");
    return 0;
}
