// bootstrap_count.h -- the clade counting of the bootstrap (docs/BOOTSTRAP_SUPPORT.md) on the host: the check of a merge list and
// boot_counter.  Included by bootstrap_support.h; it needs nothing of HIP, only ps_fail, PSCHK and the error codes of its
// includer, so that a host program of its own can hold it to a set restatement under the sanitizers
// (tests/bootstrap_count_check.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

static const uint32_t PS_BOOT_NONE = 0xffffffffu;

// a merge list of N - 1 merges as ps_nj_newick checks it: every child an earlier node that is still free
static int boot_check_merges(const char *which, uint64_t rep, const uint32_t *left, const uint32_t *right, uint32_t N, std::vector<uint8_t> &used)
{
    used.assign((size_t)2u * N - 1u, 0);
    for (uint32_t k = 0; k + 1u < N; k++)
        for (uint32_t c : { left[k], right[k] }) {
            if (c >= N + k || used[c])
                return ps_fail(PS_ERR_INVALID, "%s %llu, merge %u: child %u is not an earlier node that is still free", which, (unsigned long long)rep, k, c);
            used[c] = 1;
        }
    return PS_OK;
}

// The counting of docs/BOOTSTRAP_SUPPORT.md.  init() takes the reference tree: pos[] is its dendrogram order, at every merge the
// child that holds leaf 0 first, so that leaf 0 stands at position 0, the set below a merge is an interval and -- unrooted -- the
// complement of a set with leaf 0 is a suffix.  The sets looked for (rooted: the merges' sets; unrooted: of every split the side
// without leaf 0, two merges below the last join sharing one) are a laminar family of intervals: of those that end at one
// position only the widest can be the widest of its start too, so every member is the widest of its end (by_end) or of its
// start (by_start), and an interval is a member iff one of the two tables names it.  A split with fewer than two leaves on a side
// is in every tree (`always`).  add() counts one replicate in O(N).
struct boot_counter {
    struct entry { uint32_t lo, hi, k1, k2; uint64_t stamp; };
    uint32_t N = 0;
    bool unrooted = false;
    std::vector<uint32_t> pos, by_end, by_start, parent, mn, mx, sz, path;
    std::vector<entry> ent;
    std::vector<uint8_t> always, used;

    // parent[] of a checked list; mn, mx, sz of every node in the order pos (which init() has filled before)
    void spans(const uint32_t *left, const uint32_t *right)
    {
        for (uint32_t i = 0; i < N; i++) {
            mn[i] = mx[i] = pos[i];
            sz[i] = 1u;
        }
        for (uint32_t k = 0; k + 1u < N; k++) {
            const uint32_t a = left[k], b = right[k], v = N + k;
            parent[a] = parent[b] = v;
            mn[v] = std::min(mn[a], mn[b]);
            mx[v] = std::max(mx[a], mx[b]);
            sz[v] = sz[a] + sz[b];
        }
    }
    // the merges above leaf 0, from its parent to the root
    void path_of_zero()
    {
        path.clear();
        for (uint32_t v = parent[0]; ; v = parent[v]) {
            path.push_back(v);
            if (v == 2u * N - 2u) break;
        }
    }
    bool in_every_tree(uint32_t size) const { return size < 2u || size + 1u >= N; }

    int init(const uint32_t *left, const uint32_t *right, uint32_t pop_size, bool unrooted_)
    {
        N = pop_size;
        unrooted = unrooted_;
        PSCHK(boot_check_merges("the reference tree", 0, left, right, N, used));
        const uint32_t nodes = 2u * N - 1u, M = N - 1u;
        pos.assign(N, 0u);
        parent.assign(nodes, PS_BOOT_NONE);
        mn.assign(nodes, 0u);
        mx.assign(nodes, 0u);
        sz.assign(nodes, 0u);
        for (uint32_t k = 0; k < M; k++) parent[left[k]] = parent[right[k]] = N + k;
        path_of_zero();
        std::vector<uint8_t> on_path(nodes, 0);
        on_path[0] = 1;
        for (uint32_t v : path) on_path[v] = 1;
        // the dendrogram order, with a stack of its own: a caterpillar is as deep as the population
        std::vector<uint32_t> st(1, nodes - 1u);
        uint32_t next = 0;
        while (!st.empty()) {
            const uint32_t v = st.back();
            st.pop_back();
            if (v < N) {
                pos[v] = next++;
                continue;
            }
            const uint32_t a = left[v - N], b = right[v - N];
            const bool b_first = on_path[b];
            st.push_back(b_first ? a : b);               // (visited second)
            st.push_back(b_first ? b : a);
        }
        spans(left, right);
        // what is looked for per merge: [lo[k], hi[k]], or `always`
        std::vector<uint32_t> lo(M), hi(M), min_start(N, PS_BOOT_NONE), max_end(N, 0u);
        always.assign(M, 0);
        for (uint32_t k = 0; k < M; k++) {
            lo[k] = mn[N + k];
            hi[k] = mx[N + k];
            uint32_t size = sz[N + k];
            if (unrooted) {
                if (lo[k] == 0u) {                        // (leaf 0 below the merge: the other side, a suffix)
                    lo[k] = hi[k] + 1u;
                    hi[k] = N - 1u;
                    size = N - size;
                }
                always[k] = in_every_tree(size);
            }
            if (always[k]) continue;
            min_start[hi[k]] = std::min(min_start[hi[k]], lo[k]);
            max_end[lo[k]] = std::max(max_end[lo[k]], hi[k]);
        }
        by_end.assign(N, PS_BOOT_NONE);
        by_start.assign(N, PS_BOOT_NONE);
        ent.clear();
        for (uint32_t k = 0; k < M; k++) {
            if (always[k]) continue;
            uint32_t *cell = min_start[hi[k]] == lo[k] ? &by_end[hi[k]] : max_end[lo[k]] == hi[k] ? &by_start[lo[k]] : nullptr;
            if (!cell) return ps_fail(PS_ERR_STATE, "merge %u of the reference tree crosses another merge", k);
            if (*cell == PS_BOOT_NONE) {
                *cell = (uint32_t)ent.size();
                ent.push_back({ lo[k], hi[k], k, PS_BOOT_NONE, 0 });
                continue;
            }
            entry &e = ent[*cell];
            if (e.lo != lo[k] || e.hi != hi[k] || e.k2 != PS_BOOT_NONE)
                return ps_fail(PS_ERR_STATE, "merge %u of the reference tree repeats the set of two others", k);
            e.k2 = k;
        }
        return PS_OK;
    }

    // the interval [a, b] of the replicate `stamp`: the reference merges with that set are counted once per replicate
    uint32_t found(uint32_t a, uint32_t b, uint64_t stamp, uint32_t *support)
    {
        uint32_t e = by_end[b];
        if (e == PS_BOOT_NONE || ent[e].lo != a) {
            e = by_start[a];
            if (e == PS_BOOT_NONE || ent[e].hi != b) return 0u;
        }
        if (ent[e].stamp == stamp) return 0u;
        ent[e].stamp = stamp;
        support[ent[e].k1]++;
        if (ent[e].k2 == PS_BOOT_NONE) return 1u;
        support[ent[e].k2]++;
        return 2u;
    }

    // replicate `rep`: support[k]++ for every reference merge found in it, *shared = their number
    int add(const uint32_t *left, const uint32_t *right, uint64_t rep, uint32_t *support, uint32_t *shared)
    {
        PSCHK(boot_check_merges("replicate", rep, left, right, N, used));
        const uint64_t stamp = rep + 1;
        uint32_t n = 0;
        spans(left, right);
        if (unrooted) {
            path_of_zero();
            for (uint32_t v : path) used[v] = 2;          // (1 everywhere behind the check)
        }
        for (uint32_t k = 0; k + 1u < N; k++) {
            const uint32_t v = N + k;
            if (unrooted && (used[v] == 2 || in_every_tree(sz[v]))) continue;
            if (mx[v] - mn[v] + 1u == sz[v]) n += found(mn[v], mx[v], stamp, support);
        }
        if (unrooted) {
            // the other side of the merges above leaf 0, from the root down: what hangs beside the path so far
            uint32_t c_mn = PS_BOOT_NONE, c_mx = 0u, c_sz = 0u;
            for (size_t i = path.size(); i-- > 1;) {
                const uint32_t v = path[i], below = path[i - 1], a = left[v - N], b = right[v - N], other = a == below ? b : a;
                c_mn = std::min(c_mn, mn[other]);
                c_mx = std::max(c_mx, mx[other]);
                c_sz += sz[other];
                if (!in_every_tree(c_sz) && c_mx - c_mn + 1u == c_sz) n += found(c_mn, c_mx, stamp, support);
            }
            for (uint32_t k = 0; k + 1u < N; k++)
                if (always[k]) {
                    support[k]++;
                    n++;
                }
        }
        *shared = n;
        return PS_OK;
    }
};
