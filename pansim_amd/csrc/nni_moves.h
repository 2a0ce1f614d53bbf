// nni_moves.h -- the host rules of the parsimony tree search (ps_tree_nni, include/pansim_hip.h; the definitions:
// docs/PARSIMONY_SEARCH.md): the canonical form of a rooted binary tree, the nodes a nearest-neighbour interchange touches,
// its surgery and the greedy selection of a round.  Plain C++ with no HIP include: shared by the driver (parsimony_search.h),
// the host entries and tests/nni_moves_check.cpp.  Every function takes a checked spanning tree (pars_check_tree's rules, M =
// N - 1): nothing here reports an error.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#define NNI_NO_NODE 0xFFFFFFFFu

// A rooted binary tree over the leaves 0 .. N - 1 whose internal nodes N .. 2N - 2 are in ANY order (a move breaks the rule
// that a parent's id is above its children's; nni_to_canonical restores it): kid[2 (x - N) + side], parent[x]
struct nni_topology {
    uint32_t N = 0, root = NNI_NO_NODE;
    std::vector<uint32_t> kid, parent;
    uint32_t left(uint32_t x) const { return kid[2u * (x - N)]; }
    uint32_t right(uint32_t x) const { return kid[2u * (x - N) + 1u]; }
    uint32_t sibling(uint32_t x) const
    {
        const uint32_t v = parent[x];
        return left(v) == x ? right(v) : left(v);
    }
};

static void nni_from_merges(uint32_t N, const uint32_t *left, const uint32_t *right, nni_topology *t)
{
    const uint32_t M = N - 1u;
    t->N = N;
    t->kid.resize((size_t)2 * M);
    t->parent.assign((size_t)N + M, NNI_NO_NODE);
    for (uint32_t k = 0; k < M; k++) {
        t->kid[2u * k] = left[k];
        t->kid[2u * k + 1u] = right[k];
        t->parent[left[k]] = t->parent[right[k]] = N + k;
    }
    t->root = N + M - 1u;       // (the last merge can be nobody's child)
}

// The canonical merge list of a topology: internal nodes in (level, smallest leaf of the clade) order, the k-th as node N + k,
// left the child whose clade has the smaller smallest leaf.  level_out (may be null): the level of every new merge.
static void nni_to_canonical(const nni_topology &t, uint32_t *left, uint32_t *right, uint32_t *level_out = nullptr)
{
    const uint32_t N = t.N, M = N - 1u;
    std::vector<uint32_t> level((size_t)N + M, 0u), low((size_t)N + M), order, stack;
    for (uint32_t i = 0; i < N; i++) low[i] = i;
    // internal nodes, parents before children; walked backwards every node follows its children
    order.reserve(M);
    if (M) stack.push_back(t.root);
    while (!stack.empty()) {
        const uint32_t x = stack.back();
        stack.pop_back();
        order.push_back(x);
        for (uint32_t c : { t.left(x), t.right(x) })
            if (c >= N) stack.push_back(c);
    }
    for (size_t i = order.size(); i-- > 0;) {
        const uint32_t x = order[i], l = t.left(x), r = t.right(x);
        level[x] = 1u + std::max(level[l], level[r]);
        low[x] = std::min(low[l], low[r]);
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return level[a] != level[b] ? level[a] < level[b] : low[a] < low[b]; });
    std::vector<uint32_t> id((size_t)N + M);
    for (uint32_t i = 0; i < N; i++) id[i] = i;
    for (uint32_t k = 0; k < M; k++) id[order[k]] = N + k;
    for (uint32_t k = 0; k < M; k++) {
        uint32_t l = t.left(order[k]), r = t.right(order[k]);
        if (low[r] < low[l]) std::swap(l, r);
        left[k] = id[l];
        right[k] = id[r];
        if (level_out) level_out[k] = level[order[k]];
    }
}

// The nodes candidate (c, kind) touches -- {v, c, a, b, s}, or {root, l, r, a, b, p, q} on the root's edge -- and their number;
// 0: node c has no candidates (the root, the root's right child, the root's left child beside a leaf)
static uint32_t nni_touched(const nni_topology &t, uint32_t c, uint32_t touched[7])
{
    if (c < t.N || c == t.root) return 0u;
    const uint32_t v = t.parent[c], s = t.sibling(c);
    if (v != t.root) {
        const uint32_t n[5] = { v, c, t.left(c), t.right(c), s };
        std::copy(n, n + 5, touched);
        return 5u;
    }
    if (t.left(v) != c || s < t.N) return 0u;
    const uint32_t n[7] = { v, c, s, t.left(c), t.right(c), t.left(s), t.right(s) };
    std::copy(n, n + 7, touched);
    return 7u;
}

// Candidate (c, kind) applied in place (c must have candidates).  Below an inner node v: kind 0 swaps b with the sibling s, kind
// 1 swaps a with s.  On the root's edge: kind 0 swaps b with p, kind 1 swaps b with q.  Every node keeps its id.
static void nni_apply_move(nni_topology &t, uint32_t c, uint32_t kind)
{
    const uint32_t N = t.N, v = t.parent[c], s = t.sibling(c);
    uint32_t x_at, y_at;        // the two places in kid[] whose nodes change hands
    if (v != t.root) {
        x_at = 2u * (c - N) + (kind ? 0u : 1u);
        y_at = 2u * (v - N) + (t.left(v) == s ? 0u : 1u);
    } else {
        x_at = 2u * (c - N) + 1u;
        y_at = 2u * (s - N) + (kind ? 1u : 0u);
    }
    const uint32_t x = t.kid[x_at], y = t.kid[y_at];
    t.kid[x_at] = y;
    t.kid[y_at] = x;
    std::swap(t.parent[x], t.parent[y]);
}

struct nni_candidate {
    int64_t delta;
    uint32_t node, kind;
};

// The round's batch: the improving candidates of delta[2 M] (numbered in t's merge list: node N + k, kind) in (delta, node,
// kind) order, taken greedily while no node they touch is marked, at most `cap` (0: no cap).  *improving = their number before
// the selection.  The first of the batch is the best candidate.
static std::vector<nni_candidate> nni_select(const nni_topology &t, const int64_t *delta, uint32_t cap, uint64_t *improving)
{
    const uint32_t N = t.N, M = N - 1u;
    std::vector<nni_candidate> all, batch;
    for (uint32_t k = 0; k < M; k++)
        for (uint32_t kind = 0; kind < 2u; kind++)
            if (delta[2u * k + kind] < 0) all.push_back({ delta[2u * k + kind], N + k, kind });
    std::sort(all.begin(), all.end(), [](const nni_candidate &a, const nni_candidate &b) {
        return a.delta != b.delta ? a.delta < b.delta : a.node != b.node ? a.node < b.node : a.kind < b.kind;
    });
    *improving = all.size();
    std::vector<uint8_t> marked((size_t)N + M, 0);
    for (const nni_candidate &c : all) {
        if (cap && batch.size() >= cap) break;
        uint32_t touched[7];
        const uint32_t n = nni_touched(t, c.node, touched);
        bool is_free = n != 0u;
        for (uint32_t i = 0; i < n; i++) is_free = is_free && !marked[touched[i]];
        if (!is_free) continue;
        for (uint32_t i = 0; i < n; i++) marked[touched[i]] = 1;
        batch.push_back(c);
    }
    return batch;
}

// ---- branch lengths and binary64 gains: the likelihood search (ps_tree_model_nni; docs/LIKELIHOOD_SEARCH.md) ----
// A length belongs to the node below its branch, and every node keeps its id through nni_apply_move: a move carries
// length[N + M] along as it is.  Only the canonical form renumbers.  (inline: a program that includes this header for the
// parsimony rules alone does not use them.)

// nni_to_canonical with the lengths carried to the new ids: length_out[new id of x] = length_in[x] (the root's too)
static inline void nni_to_canonical_lengths(const nni_topology &t, const double *length_in, uint32_t *left, uint32_t *right, double *length_out)
{
    const uint32_t N = t.N, M = N - 1u;
    nni_to_canonical(t, left, right);
    // the new id of every old node, children first: the merge of the canonical list that joins the new ids of its two children
    std::vector<std::pair<uint64_t, uint32_t>> joins(M);
    for (uint32_t k = 0; k < M; k++) joins[k] = { ((uint64_t)std::min(left[k], right[k]) << 32) | std::max(left[k], right[k]), N + k };
    std::sort(joins.begin(), joins.end());
    std::vector<uint32_t> id((size_t)N + M, NNI_NO_NODE), order, stack;
    for (uint32_t i = 0; i < N; i++) id[i] = i;
    if (M) stack.push_back(t.root);
    while (!stack.empty()) {
        const uint32_t x = stack.back();
        stack.pop_back();
        order.push_back(x);
        for (uint32_t c : { t.left(x), t.right(x) })
            if (c >= N) stack.push_back(c);
    }
    for (size_t i = order.size(); i-- > 0;) {
        const uint32_t x = order[i], l = id[t.left(x)], r = id[t.right(x)];
        const uint64_t key = ((uint64_t)std::min(l, r) << 32) | std::max(l, r);
        id[x] = std::lower_bound(joins.begin(), joins.end(), std::make_pair(key, 0u))->second;
    }
    for (uint32_t x = 0; x < N + M; x++) length_out[id[x]] = length_in[x];
}

struct nni_gain_candidate {
    double gain;
    uint32_t node, kind;
};

// The round's batch over binary64 gains: the candidates of gain[2 M] (NaN: no candidate) with gain > eps in (gain descending,
// node, kind) order, taken greedily while no node they touch is marked, at most `cap` (0: no cap).  *improving = their number
// before the selection.  The first of the batch is the best candidate.
static inline std::vector<nni_gain_candidate> nni_select_gains(const nni_topology &t, const double *gain, double eps, uint32_t cap, uint64_t *improving)
{
    const uint32_t N = t.N, M = N - 1u;
    std::vector<nni_gain_candidate> all, batch;
    for (uint32_t k = 0; k < M; k++)
        for (uint32_t kind = 0; kind < 2u; kind++)
            if (gain[2u * k + kind] > eps) all.push_back({ gain[2u * k + kind], N + k, kind });
    std::sort(all.begin(), all.end(), [](const nni_gain_candidate &a, const nni_gain_candidate &b) {
        return a.gain != b.gain ? a.gain > b.gain : a.node != b.node ? a.node < b.node : a.kind < b.kind;
    });
    *improving = all.size();
    std::vector<uint8_t> marked((size_t)N + M, 0);
    for (const nni_gain_candidate &c : all) {
        if (cap && batch.size() >= cap) break;
        uint32_t touched[7];
        const uint32_t n = nni_touched(t, c.node, touched);
        bool is_free = n != 0u;
        for (uint32_t i = 0; i < n; i++) is_free = is_free && !marked[touched[i]];
        if (!is_free) continue;
        for (uint32_t i = 0; i < n; i++) marked[touched[i]] = 1;
        batch.push_back(c);
    }
    return batch;
}
