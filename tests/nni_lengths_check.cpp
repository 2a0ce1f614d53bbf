// nni_lengths_check.cpp -- the host rules of the likelihood tree search (pansim_amd/csrc/nni_moves.h: the canonical form that
// carries branch lengths, the selection over binary64 gains) against clade sets: a host program of its own (no device, nothing
// loaded into Python), built with the address and undefined-behaviour sanitizers by tests/test_nni_lengths.py.  Every leaf and
// every merge gets a length of its own; a random walk applies interchanges -- one at a time, or a selected batch -- and takes the
// canonical form with lengths.  The map clade -> length must stay as it was for every clade the move keeps, and the regrouped
// nodes (c; on the root's edge c and s) must carry their old lengths to their new clades; a batch must be sorted by (gain
// descending, node, kind), hold only gains above eps, touch every node once and respect the cap.
#include <cstdio>
#include <cstdlib>
#include <map>
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

static std::map<clade, double> clade_lengths(const nni_topology &t, const std::vector<double> &length)
{
    const std::vector<clade> b = below(t);
    std::map<clade, double> out;
    for (uint32_t x = 0; x < 2 * t.N - 1; x++) out[b[x]] = length[x];
    return out;
}

int main()
{
    std::mt19937_64 rng(2024);
    uint64_t steps = 0, batches = 0, batch_moves = 0;
    for (uint32_t trial = 0; trial < 120; trial++) {
        const uint32_t N = 4 + (uint32_t)(rng() % 37), M = N - 1, nodes = N + M;
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
        std::vector<double> length(nodes), nlen(nodes);
        for (uint32_t x = 0; x < nodes; x++) length[x] = 1.0 + x + 1000.0 * trial;      // (one value per node: a misplaced one shows)
        nni_topology t;
        nni_from_merges(N, left.data(), right.data(), &t);
        const std::map<clade, double> start = clade_lengths(t, length);
        nni_to_canonical_lengths(t, length.data(), nl.data(), nr.data(), nlen.data());
        left = nl;
        right = nr;
        length = nlen;
        nni_from_merges(N, left.data(), right.data(), &t);
        CHECK(clade_lengths(t, length) == start, "trial %u: the canonical form moved a length", trial);
        for (uint32_t step = 0; step < 30; step++) {
            const std::vector<clade> b = below(t);
            const std::map<clade, double> before = clade_lengths(t, length);
            std::vector<uint32_t> regrouped;          // the nodes whose clade changes: they keep their lengths
            nni_topology next = t;
            auto take = [&](uint32_t c, uint32_t kind) {
                regrouped.push_back(c);
                if (t.parent[c] == t.root) regrouped.push_back(t.sibling(c));
                nni_apply_move(next, c, kind);
            };
            if (step % 5 == 4) {
                // a batch by made-up gains: some below eps, some equal
                const double eps = 0.5;
                std::vector<double> gain((size_t)2 * M);
                uint64_t above = 0;
                for (uint32_t k = 0; k < M; k++) {
                    uint32_t touched[7];
                    const bool some = nni_touched(t, N + k, touched) != 0;
                    for (uint32_t kind = 0; kind < 2; kind++) {
                        gain[2 * k + kind] = some ? 0.25 * (double)(rng() % 12) : NAN;
                        above += some && gain[2 * k + kind] > eps;
                    }
                }
                uint64_t improving = 0;
                const uint32_t cap = (uint32_t)(rng() % 4);
                const std::vector<nni_gain_candidate> batch = nni_select_gains(t, gain.data(), eps, cap, &improving);
                CHECK(improving == above, "trial %u: %llu candidates above eps, not %llu", trial, (unsigned long long)improving, (unsigned long long)above);
                CHECK((batch.empty() == (above == 0)) && (!cap || batch.size() <= cap), "trial %u: a batch of %zu under the cap %u", trial, batch.size(), cap);
                std::vector<uint32_t> marks(nodes, 0);
                for (size_t i = 0; i < batch.size(); i++) {
                    uint32_t touched[7];
                    const uint32_t n = nni_touched(t, batch[i].node, touched);
                    for (uint32_t j = 0; j < n; j++) CHECK(!marks[touched[j]]++, "trial %u: node %u is touched twice", trial, touched[j]);
                    if (i)
                        CHECK(batch[i - 1].gain > batch[i].gain || (batch[i - 1].gain == batch[i].gain && batch[i - 1].node <= batch[i].node),
                              "trial %u: the batch is not sorted", trial);
                    CHECK(batch[i].gain > eps && batch[i].gain == gain[2 * (batch[i].node - N) + batch[i].kind], "trial %u: a gain that is not the candidate's",
                          trial);
                    take(batch[i].node, batch[i].kind);
                }
                if (!batch.empty()) {
                    double best = 0.0;
                    for (double g : gain) best = g > best ? g : best;
                    CHECK(batch[0].gain == best, "trial %u: the first of the batch is not the best candidate", trial);
                }
                batches++;
                batch_moves += batch.size();
            } else {
                uint32_t c, touched[7], kind = (uint32_t)(rng() & 1);
                do c = N + (uint32_t)(rng() % M);
                while (!nni_touched(t, c, touched));
                take(c, kind);
            }
            nni_to_canonical_lengths(next, length.data(), nl.data(), nr.data(), nlen.data());
            nni_topology after_t;
            nni_from_merges(N, nl.data(), nr.data(), &after_t);
            const std::map<clade, double> after = clade_lengths(after_t, nlen);
            // every clade the move keeps has the length it had
            std::multiset<double> lost, found;
            for (const auto &kv : before) {
                const auto it = after.find(kv.first);
                if (it == after.end()) lost.insert(kv.second);
                else CHECK(it->second == kv.second, "trial %u step %u: a kept clade changed its length", trial, step);
            }
            for (const auto &kv : after)
                if (!before.count(kv.first)) found.insert(kv.second);
            std::multiset<double> kept;
            for (uint32_t x : regrouped) kept.insert(length[x]);
            CHECK(lost == kept && found == kept, "trial %u step %u: the regrouped nodes did not keep their lengths", trial, step);
            CHECK(lost.size() == regrouped.size(), "trial %u step %u: %zu clades changed for %zu regrouped nodes", trial, step, lost.size(), regrouped.size());
            // the same list as the canonical form without lengths; idempotent
            std::vector<uint32_t> l2(M), r2(M);
            nni_to_canonical(next, l2.data(), r2.data());
            CHECK(l2 == nl && r2 == nr, "trial %u step %u: the two canonical forms differ", trial, step);
            std::vector<double> len2(nodes);
            nni_to_canonical_lengths(after_t, nlen.data(), l2.data(), r2.data(), len2.data());
            CHECK(l2 == nl && r2 == nr && len2 == nlen, "trial %u step %u: the canonical form with lengths is not idempotent", trial, step);
            left = nl;
            right = nr;
            length = nlen;
            nni_from_merges(N, left.data(), right.data(), &t);
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
