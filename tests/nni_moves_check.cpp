// nni_moves_check.cpp -- the host rules of the parsimony tree search (pansim_amd/csrc/nni_moves.h) against clade sets: a host
// program of its own (no device, nothing loaded into Python), built with the address and undefined-behaviour sanitizers by
// tests/test_nni_moves.py.  A random walk over trees: every step applies a random interchange and takes the canonical form, and
// the clades of the result must be those of the tree before with exactly the clades the interchange names replaced; the list
// must be a valid merge list in canonical order; a selected batch must touch every node at most once, be sorted and, applied as
// one, change exactly the clades of its moves.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

#include "../pansim_amd/csrc/nni_moves.h"

typedef std::set<uint32_t> clade;

static int failures = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            printf("MISMATCH " __VA_ARGS__); \
            printf("\n");                \
            failures++;                  \
        }                                \
    } while (0)

// the leaves below every node of a topology
static std::vector<clade> below(const nni_topology &t)
{
    std::vector<clade> out((size_t)2 * t.N - 1);
    std::vector<uint32_t> order, stack{ t.root };
    while (!stack.empty()) {
        const uint32_t x = stack.back();
        stack.pop_back();
        order.push_back(x);
        if (x >= t.N) {
            stack.push_back(t.left(x));
            stack.push_back(t.right(x));
        }
    }
    for (size_t i = order.size(); i-- > 0;) {
        const uint32_t x = order[i];
        if (x < t.N) out[x] = { x };
        else {
            out[x] = out[t.left(x)];
            out[x].insert(out[t.right(x)].begin(), out[t.right(x)].end());
        }
    }
    return out;
}

static std::set<clade> internal_clades(const nni_topology &t)
{
    const std::vector<clade> b = below(t);
    return std::set<clade>(b.begin() + t.N, b.end());
}

static clade join(const clade &a, const clade &b)
{
    clade out = a;
    out.insert(b.begin(), b.end());
    return out;
}

// the clades candidate (c, kind) removes from and adds to the tree, by the table of docs/PARSIMONY_SEARCH.md
static void expected_change(const nni_topology &t, const std::vector<clade> &b, uint32_t c, uint32_t kind, std::set<clade> *gone,
                            std::set<clade> *come)
{
    const uint32_t v = t.parent[c], s = t.sibling(c), a = t.left(c), bb = t.right(c);
    gone->insert(b[c]);
    if (v != t.root) {
        come->insert(kind == 0 ? join(b[a], b[s]) : join(b[s], b[bb]));
    } else {
        const uint32_t p = t.left(s), q = t.right(s);
        gone->insert(b[s]);
        come->insert(kind == 0 ? join(b[a], b[p]) : join(b[a], b[q]));
        come->insert(kind == 0 ? join(b[bb], b[q]) : join(b[p], b[bb]));
    }
}

// a valid merge list in canonical order?
static void check_canonical(uint32_t N, const std::vector<uint32_t> &left, const std::vector<uint32_t> &right)
{
    const uint32_t M = N - 1;
    std::vector<uint32_t> level((size_t)N + M, 0), low((size_t)N + M), used((size_t)N + M, 0);
    for (uint32_t i = 0; i < N; i++) low[i] = i;
    for (uint32_t k = 0; k < M; k++) {
        const uint32_t l = left[k], r = right[k];
        CHECK(l < N + k && r < N + k && l != r, "merge %u has a child that is not below it", k);
        if (l >= N + k || r >= N + k) return;
        CHECK(!used[l] && !used[r], "merge %u takes a node a second time", k);
        used[l] = used[r] = 1;
        level[N + k] = 1 + std::max(level[l], level[r]);
        low[N + k] = std::min(low[l], low[r]);
        CHECK(low[l] < low[r], "merge %u: left is not the child with the smaller smallest leaf", k);
        if (k)
            CHECK(level[N + k - 1] < level[N + k] || (level[N + k - 1] == level[N + k] && low[N + k - 1] < low[N + k]),
                  "merge %u is not in (level, smallest leaf) order", k);
    }
}

int main()
{
    std::mt19937_64 rng(12345);
    uint64_t steps = 0, batches = 0, batch_moves = 0;
    for (uint32_t trial = 0; trial < 120; trial++) {
        const uint32_t N = 4 + (uint32_t)(rng() % 37), M = N - 1;
        // a random spanning merge list
        std::vector<uint32_t> live(N), left(M), right(M), nl(M), nr(M);
        for (uint32_t i = 0; i < N; i++) live[i] = i;
        for (uint32_t k = 0; k < M; k++) {
            const size_t i = rng() % live.size();
            left[k] = live[i];
            live.erase(live.begin() + i);
            const size_t j = rng() % live.size();
            right[k] = live[j];
            live[j] = N + k;
        }
        nni_topology t;
        nni_from_merges(N, left.data(), right.data(), &t);
        const std::set<clade> start = internal_clades(t);
        nni_to_canonical(t, nl.data(), nr.data());
        check_canonical(N, nl, nr);
        left = nl;
        right = nr;
        nni_from_merges(N, left.data(), right.data(), &t);
        CHECK(internal_clades(t) == start, "trial %u: the canonical form changed the clades", trial);
        for (uint32_t step = 0; step < 30; step++) {
            const std::vector<clade> b = below(t);
            const std::set<clade> before(b.begin() + N, b.end());
            std::set<clade> gone, come;
            nni_topology next = t;
            if (step % 5 == 4) {
                // a batch by made-up deltas: every candidate improving, in random order of delta
                std::vector<int64_t> delta((size_t)2 * M);
                for (uint32_t k = 0; k < M; k++) {
                    uint32_t touched[7];
                    const bool some = nni_touched(t, N + k, touched) != 0;
                    for (uint32_t kind = 0; kind < 2; kind++) delta[2 * k + kind] = some ? -(int64_t)(1 + rng() % 6) : INT64_MAX;
                }
                uint64_t improving = 0;
                const uint32_t cap = (uint32_t)(rng() % 4);
                const std::vector<nni_candidate> batch = nni_select(t, delta.data(), cap, &improving);
                CHECK(improving == 2ull * (N - 3), "trial %u: %llu improving candidates of %u", trial, (unsigned long long)improving, 2 * (N - 3));
                CHECK(!batch.empty() && (!cap || batch.size() <= cap), "trial %u: a batch of %zu under the cap %u", trial, batch.size(), cap);
                std::vector<uint32_t> marks((size_t)N + M, 0);
                for (size_t i = 0; i < batch.size(); i++) {
                    uint32_t touched[7];
                    const uint32_t n = nni_touched(t, batch[i].node, touched);
                    for (uint32_t j = 0; j < n; j++) CHECK(!marks[touched[j]]++, "trial %u: node %u is touched twice", trial, touched[j]);
                    if (i)
                        CHECK(batch[i - 1].delta < batch[i].delta || (batch[i - 1].delta == batch[i].delta && batch[i - 1].node <= batch[i].node),
                              "trial %u: the batch is not sorted", trial);
                    CHECK(batch[i].delta == delta[2 * (batch[i].node - N) + batch[i].kind], "trial %u: a delta that is not the candidate's", trial);
                    expected_change(t, b, batch[i].node, batch[i].kind, &gone, &come);
                    nni_apply_move(next, batch[i].node, batch[i].kind);
                }
                batches++;
                batch_moves += batch.size();
            } else {
                uint32_t c, touched[7], kind = (uint32_t)(rng() & 1);
                do c = N + (uint32_t)(rng() % M);
                while (!nni_touched(t, c, touched));
                expected_change(t, b, c, kind, &gone, &come);
                nni_apply_move(next, c, kind);
            }
            std::set<clade> want = before;
            for (const clade &g : gone) want.erase(g);
            want.insert(come.begin(), come.end());
            CHECK(want.size() == M, "trial %u step %u: the expected clades are not a tree", trial, step);
            for (uint32_t x = 0; x < N + M; x++)
                if (x != next.root) CHECK(next.left(next.parent[x]) == x || next.right(next.parent[x]) == x, "trial %u: parent of %u", trial, x);
            nni_to_canonical(next, nl.data(), nr.data());
            check_canonical(N, nl, nr);
            left = nl;
            right = nr;
            nni_from_merges(N, left.data(), right.data(), &t);
            CHECK(internal_clades(t) == want, "trial %u step %u: the clades after the move", trial, step);
            std::vector<uint32_t> l2(M), r2(M);
            nni_to_canonical(t, l2.data(), r2.data());
            CHECK(l2 == left && r2 == right, "trial %u step %u: the canonical form is not idempotent", trial, step);
            steps++;
        }
    }
    printf("%llu steps, %llu batches of %llu moves\n", (unsigned long long)steps, (unsigned long long)batches, (unsigned long long)batch_moves);
    if (failures) {
        printf("%d mismatches\n", failures);
        return 1;
    }
    printf("every step matches\n");
    return 0;
}
