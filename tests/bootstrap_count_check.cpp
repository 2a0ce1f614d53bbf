// The clade counting of the bootstrap (boot_counter of pansim_amd/csrc/bootstrap_count.h) against a restatement on sorted leaf
// sets, in a host program of its own (no device, nothing loaded into Python):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o bootstrap_count_check tests/bootstrap_count_check.cpp
// (tests/test_bootstrap_support.py does both)
//   ./bootstrap_count_check       (exit status 1 on a difference)
// Random trees, caterpillars and replicates that share most clades with the reference, rooted and unrooted, at sizes from 2 to a
// few hundred leaves; malformed lists must be refused without a read outside them.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>

#include "../include/pansim_hip.h"

static char g_msg[512];
static int ps_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return code;
}
#define PSCHK(expr)                   \
    do {                              \
        int rc_ = (expr);             \
        if (rc_ != PS_OK) return rc_; \
    } while (0)

#include "../pansim_amd/csrc/bootstrap_count.h"

typedef std::vector<uint32_t> list;
struct tree { list left, right; };

static tree random_tree(std::mt19937 &rng, uint32_t n)
{
    list free_nodes(n);
    tree t;
    for (uint32_t i = 0; i < n; i++) free_nodes[i] = i;
    for (uint32_t k = 0; k + 1 < n; k++) {
        for (list *side : { &t.left, &t.right }) {
            const size_t i = rng() % free_nodes.size();
            side->push_back(free_nodes[i]);
            free_nodes.erase(free_nodes.begin() + i);
        }
        free_nodes.push_back(n + k);
    }
    return t;
}

static tree caterpillar(uint32_t n)
{
    tree t;
    for (uint32_t k = 0; k + 1 < n; k++) {
        t.left.push_back(k ? n + k - 1 : 0);
        t.right.push_back(k + 1);
    }
    return t;
}

// two leaves exchanged: most clades survive
static tree swapped(const tree &t, uint32_t n, uint32_t i, uint32_t j)
{
    tree o = t;
    for (list *side : { &o.left, &o.right })
        for (uint32_t &c : *side)
            if (c < n) c = c == i ? j : c == j ? i : c;
    return o;
}

// what every merge is looked for by: its leaf set, or unrooted the side of its split without leaf 0 (empty: in every tree)
static std::vector<std::set<uint32_t>> looked_for(const tree &t, uint32_t n, bool unrooted, std::vector<bool> *always)
{
    std::vector<std::set<uint32_t>> below(n), out;
    for (uint32_t i = 0; i < n; i++) below[i].insert(i);
    always->clear();
    for (uint32_t k = 0; k + 1 < n; k++) {
        std::set<uint32_t> s = below[t.left[k]];
        s.insert(below[t.right[k]].begin(), below[t.right[k]].end());
        below.push_back(s);
        if (unrooted && s.count(0)) {
            std::set<uint32_t> other;
            for (uint32_t i = 0; i < n; i++)
                if (!s.count(i)) other.insert(i);
            s = other;
        }
        const bool trivial = unrooted && (s.size() < 2 || s.size() + 1 >= n);
        always->push_back(trivial);
        out.push_back(trivial ? std::set<uint32_t>() : s);
    }
    return out;
}

static int bad = 0;

static void compare(const tree &ref, const std::vector<tree> &reps, uint32_t n, bool unrooted)
{
    boot_counter cnt;
    list support(n - 1, 0), shared(reps.size(), 0), want_support(n - 1, 0), want_shared(reps.size(), 0);
    if (cnt.init(ref.left.data(), ref.right.data(), n, unrooted) != PS_OK) {
        printf("init refused a good tree of %u leaves: %s\n", n, g_msg);
        bad++;
        return;
    }
    std::vector<bool> always, rep_always;
    const auto want = looked_for(ref, n, unrooted, &always);
    for (size_t b = 0; b < reps.size(); b++) {
        if (cnt.add(reps[b].left.data(), reps[b].right.data(), b, support.data(), &shared[b]) != PS_OK) {
            printf("add refused a good tree of %u leaves: %s\n", n, g_msg);
            bad++;
            return;
        }
        const auto have_list = looked_for(reps[b], n, unrooted, &rep_always);
        const std::set<std::set<uint32_t>> have(have_list.begin(), have_list.end());
        for (uint32_t k = 0; k + 1 < n; k++)
            if (always[k] || (!want[k].empty() && have.count(want[k]))) {
                want_support[k]++;
                want_shared[b]++;
            }
    }
    if (support != want_support || shared != want_shared) {
        printf("N = %u, %s: the counts differ from the restatement\n", n, unrooted ? "unrooted" : "rooted");
        bad++;
    }
}

int main()
{
    std::mt19937 rng(20);
    for (uint32_t n : { 2u, 3u, 4u, 5u, 8u, 33u, 64u, 65u, 257u }) {
        for (int round = 0; round < (n < 10 ? 40 : 4); round++) {
            const tree ref = round % 4 == 3 ? caterpillar(n) : random_tree(rng, n);
            std::vector<tree> reps = { ref, random_tree(rng, n), caterpillar(n) };
            for (int s = 0; s < 5 && n > 2; s++) reps.push_back(swapped(ref, n, rng() % n, rng() % n));
            if (n > 2) reps.push_back(swapped(swapped(ref, n, 0, n - 1), n, 1 % n, n / 2));
            compare(ref, reps, n, false);
            compare(ref, reps, n, true);
        }
    }
    // malformed lists: refused, nothing read outside them
    {
        const uint32_t n = 6;
        const tree good = caterpillar(n);
        boot_counter cnt;
        list support(n - 1, 0);
        uint32_t shared = 0;
        std::vector<tree> broken(4, good);
        broken[0].left[2] = 4000000000u;        // no node at all
        broken[1].right[1] = n + 1;             // not an earlier node
        broken[2].right[3] = 1;                 // a leaf twice
        broken[3].left[4] = n;                  // an inner node twice
        for (const tree &t : broken) {
            if (cnt.init(t.left.data(), t.right.data(), n, true) != PS_ERR_INVALID) bad++, printf("init accepted a malformed reference tree\n");
            if (cnt.init(good.left.data(), good.right.data(), n, true) != PS_OK) bad++;
            if (cnt.add(t.left.data(), t.right.data(), 0, support.data(), &shared) != PS_ERR_INVALID) bad++, printf("add accepted a malformed replicate\n");
        }
    }
    if (bad) return 1;
    printf("bootstrap counting ok\n");
    return 0;
}
