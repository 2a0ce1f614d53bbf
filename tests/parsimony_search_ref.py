"""A NumPy restatement of docs/PARSIMONY_SEARCH.md for the tests: every delta by RESCORING the neighbour tree from scratch
(never from the sets outside a subtree, which is what the kernel and the host entries use), the canonical form, the
search loop.  A tree is a dict kids[node] = (left, right) over arbitrary internal ids plus its root."""
import numpy as np

NONE = 2**63 - 1
BASES = np.array([1, 2, 4, 8], np.uint8)


def class_bits(m):
    m = np.asarray(m, np.uint8)
    return np.where(np.isin(m, BASES), m, np.uint8(16)).astype(np.uint8)


def tree_of(left, right, N):
    kids = {N + k: (int(a), int(b)) for k, (a, b) in enumerate(zip(left, right))}
    return kids, N + len(left) - 1


def postorder(kids, root):
    out, stack = [], [root]
    while stack:
        x = stack.pop()
        if x in kids:
            out.append(x)
            stack += list(kids[x])
    return out[::-1]


def score(kids, root, st):
    """total changes of the class bits st (N, L) on the tree, by the up pass alone"""
    S, total = {}, 0
    for x in postorder(kids, root):
        l, r = kids[x]
        a, b = S[l] if l in S else st[l], S[r] if r in S else st[r]
        i = a & b
        e = i == 0
        total += int(e.sum())
        S[x] = np.where(e, a | b, i)
    return total


def parents(kids):
    return {c: v for v, pair in kids.items() for c in pair}


def neighbour(kids, root, c, kind):
    """candidate (c, kind) as the table of docs/PARSIMONY_SEARCH.md words it -> (the new kids, the touched set), or None"""
    par = parents(kids)
    if c not in kids or c == root:
        return None
    a, b = kids[c]
    v = par[c]
    s = kids[v][1] if kids[v][0] == c else kids[v][0]
    new = dict(kids)
    if v != root:
        # kind 0: c becomes (a, s), v keeps c and takes b; kind 1: c becomes (s, b), v keeps c and takes a
        new[c] = (a, s) if kind == 0 else (s, b)
        gone = b if kind == 0 else a
        new[v] = tuple(gone if x == s else x for x in kids[v])
        return new, {v, c, a, b, s}
    if kids[v][0] != c or s not in kids:
        return None
    p, q = kids[s]
    # only the quartet exists: kind 0 swaps b and p, kind 1 swaps b and q
    new[c] = (a, p) if kind == 0 else (a, q)
    new[s] = (b, q) if kind == 0 else (p, b)
    return new, {v, c, s, a, b, p, q}


def deltas(st, left, right):
    """(T, delta[M, 2]) of the merge list as given: every neighbour tree is scored from scratch"""
    N = st.shape[0]
    kids, root = tree_of(left, right, N)
    T = score(kids, root, st)
    out = np.full((len(left), 2), NONE, np.int64)
    for k in range(len(left)):
        for kind in (0, 1):
            nb = neighbour(kids, root, N + k, kind)
            if nb is not None:
                out[k, kind] = score(nb[0], root, st) - T
    return T, out


def canonical(kids, root, N):
    """(left, right) of the canonical form: internal nodes by (level, smallest leaf), left the child with the smaller one"""
    level, low = {}, {}
    for x in postorder(kids, root):
        l, r = kids[x]
        level[x] = 1 + max(level.get(l, 0), level.get(r, 0))
        low[x] = min(low.get(l, l), low.get(r, r))
    order = sorted(kids, key=lambda x: (level[x], low[x]))
    ident = {x: N + k for k, x in enumerate(order)}
    left, right = [], []
    for x in order:
        l, r = kids[x]
        if low.get(r, r) < low.get(l, l):
            l, r = r, l
        left.append(ident.get(l, l))
        right.append(ident.get(r, r))
    return np.array(left, np.uint32), np.array(right, np.uint32)


def clades(left, right, N):
    """the leaf sets of the internal nodes"""
    below = {i: frozenset([i]) for i in range(N)}
    for k, (a, b) in enumerate(zip(left, right)):
        below[N + k] = below[int(a)] | below[int(b)]
    return {below[N + k] for k in range(len(left))}


def root_split(left, right, N):
    """the two clades below the root, left first"""
    below = {i: frozenset([i]) for i in range(N)}
    for k, (a, b) in enumerate(zip(left, right)):
        below[N + k] = below[int(a)] | below[int(b)]
    return below[int(left[-1])], below[int(right[-1])]


def search(m, left, right, max_rounds=1000, moves_per_round=0):
    """the search loop of the document over rescored deltas -> a dict of the summary fields, the tree, round_changes, moves"""
    st = class_bits(m)
    N, L = st.shape
    left, right = canonical(*tree_of(left, right, N), N)
    T, d = deltas(st, left, right)
    out = dict(pop_size=N, sites=L, merges=N - 1, rounds=0, passes=1, rollbacks=0, local_optimum=False, start_changes=T,
               min_changes=int(sum(len(np.unique(st[:, s])) - 1 for s in range(L))))
    round_changes, moves = [T], []
    while True:
        cands = sorted((int(d[k, kind]), N + k, kind) for k in range(N - 1) for kind in (0, 1) if d[k, kind] < 0)
        out["candidates_last"] = len(cands)
        if not cands:
            out["local_optimum"] = True
            break
        if out["rounds"] == max_rounds:
            break
        kids, root = tree_of(left, right, N)
        marked, batch = set(), []
        for delta, node, kind in cands:
            if moves_per_round and len(batch) >= moves_per_round:
                break
            touched = neighbour(kids, root, node, kind)[1]
            if touched & marked:
                continue
            marked |= touched
            batch.append((delta, node, kind))

        def applied(batch):
            cur = kids
            for _, node, kind in batch:
                cur = neighbour(cur, root, node, kind)[0]
            return canonical(cur, root, N)
        nl, nr = applied(batch)
        T2, d2 = deltas(st, nl, nr)
        out["passes"] += 1
        if len(batch) > 1 and T2 > T + batch[0][0]:
            out["rollbacks"] += 1
            batch = batch[:1]
            nl, nr = applied(batch)
            T2, d2 = deltas(st, nl, nr)
            out["passes"] += 1
        out["rounds"] += 1
        moves += [(out["rounds"], node, kind, delta) for delta, node, kind in batch]
        left, right, T, d = nl, nr, T2, d2
        round_changes.append(T)
    out.update(total_changes=T, n_moves=len(moves))
    return out, left, right, round_changes, moves


def assert_search_equal(got, want):
    """a ParsimonySearch against the tuple of search(): every field, the tree, the rounds and the moves"""
    summary, left, right, round_changes, moves = want
    for name, value in summary.items():
        assert getattr(got, name) == value, (name, getattr(got, name), value)
    assert np.array_equal(got.left, left) and np.array_equal(got.right, right)
    assert got.round_changes.tolist() == round_changes
    assert [tuple(int(x) for x in mv) for mv in got.moves] == moves


def random_tree(rng, N):
    """a spanning merge list: random pairs of the live nodes are joined"""
    live, left, right = list(range(N)), [], []
    for k in range(N - 1):
        i, j = rng.choice(len(live), 2, replace=False)
        a, b = live[i], live[j]
        live = [x for x in live if x not in (a, b)] + [N + k]
        left.append(a)
        right.append(b)
    return np.array(left, np.uint32), np.array(right, np.uint32)


def caterpillar(N, order=None):
    order = list(range(N)) if order is None else [int(x) for x in order]
    left = [order[0]] + [N + k for k in range(N - 2)]
    return np.array(left, np.uint32), np.array(order[1:], np.uint32)


def balanced(N):
    """leaves joined pairwise level by level (an odd one waits for the next level)"""
    live, left, right, k = list(range(N)), [], [], 0
    while len(live) > 1:
        nxt = []
        for i in range(0, len(live) - 1, 2):
            left.append(live[i])
            right.append(live[i + 1])
            nxt.append(N + k)
            k += 1
        if len(live) % 2:
            nxt.append(live[-1])
        live = nxt
    return np.array(left, np.uint32), np.array(right, np.uint32)


def onehot(rng, shape, states=4):
    return BASES[rng.integers(0, states, shape)]
