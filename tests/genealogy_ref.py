"""Plain restatement of the recorded genealogy (docs/GENEALOGY.md) for the tests: everything by brute force from the parent
draws of every generation in OUTPUT rows (what ps_sim_last_parents returns), Python integers and numpy only.  Nothing here uses
the comb's order of storage or the monotonicity of the parent maps: the truth is the all-pairs matrix of divergence times, and
the read-outs of a comb are restated from that matrix."""
import numpy as np

BEYOND = 0xFFFFFFFF
CORE, ACC = 0, 1


def tmrca_matrix(parents, N):
    """parents: the draws of the recorded generations, oldest first; parents[g][k] = the row (of the outputs of the generation
    before) that row k of generation g descends from.  -> (N, N) uint32: the smallest t at which the ancestors t generations
    back are one individual, 0 on the diagonal, BEYOND where the record ends first."""
    T = np.full((N, N), BEYOND, np.uint32)
    np.fill_diagonal(T, 0)
    anc = np.arange(N)
    for t, par in enumerate(reversed(list(parents)), start=1):
        anc = np.asarray(par, np.int64)[anc]
        same = anc[:, None] == anc[None, :]
        T[same & (T == BEYOND)] = t
    return T


def matrix_of_comb(order, coal):
    """the all-pairs matrix a comb stands for, in output rows: the time of two individuals is the largest coal between them"""
    N = len(order)
    T = np.zeros((N, N), np.uint32)
    for a in range(N):
        for b in range(a + 1, N):
            T[order[a], order[b]] = T[order[b], order[a]] = max(int(c) for c in coal[a:b])
    return T


def summary(T, depth, capacity, generation):
    N = T.shape[0]
    lab = clusters(T, BEYOND - 1)[0]
    roots = len(set(lab.tolist()))
    return dict(pop_size=N, generation=generation, capacity=capacity, depth=depth, roots=roots,
                tmrca=int(T.max()) if roots == 1 else 0)


def clusters(T, t):
    """labels[i] = the smallest row j with T[i, j] <= t; the summary"""
    N = T.shape[0]
    labels = np.array([int(np.flatnonzero(T[i] <= t)[0]) for i in range(N)], np.uint32)
    sizes = np.bincount(labels, minlength=N)
    sizes = sizes[sizes > 0]
    return labels, dict(clusters=int(sizes.size), largest=int(sizes.max()), within_pairs=int((sizes * (sizes - 1) // 2).sum()))


def newick(order, T):
    """the trees in the leaf order `order`: the leaves of a tree fall into the classes of `closer than the largest time among
    them` (an equivalence: the times are an ultrametric), listed in leaf order"""
    def tree(leaves):
        if len(leaves) == 1:
            return str(leaves[0]), 0
        m = max(int(T[a, b]) for a in leaves for b in leaves)
        parts, seen = [], set()
        for a in leaves:
            if a in seen:
                continue
            group = [b for b in leaves if int(T[a, b]) < m]
            seen.update(group)
            text, height = tree(group)
            parts.append("%s:%d" % (text, m - height))
        return "(" + ",".join(parts) + ")", m

    leaves = [int(x) for x in order]
    out, seen = [], set()
    for a in leaves:
        if a in seen:
            continue
        group = [b for b in leaves if int(T[a, b]) != BEYOND]
        seen.update(group)
        out.append(tree(group)[0] + ";\n")
    return "".join(out)


def clock_from_counts(metric, tmrca, h, inter, union, depth, L, cg, Bt, Bx, time_span=0, core_span=0):
    """-> dict(joint (Bt + 1, Bx), per_time (Bt + 1, 3), and the summary fields).  Whole arrays at a time in int64: every product
    stays below 2^63 (times and numerators below 2^32, at most 16384 bins), and so does every sum the tests can reach."""
    t = np.asarray(tmrca, np.int64)
    P = t.size
    St = int(time_span) or int(depth)
    bt = np.where(t == BEYOND, Bt, np.minimum(Bt - 1, (t - 1) * Bt // St))
    undefined = clamped = S = 0
    if metric == CORE:
        num = np.asarray(h, np.int64) // 2
        den = np.full(P, int(L), np.int64)
        S = int(core_span) or int(num.max()) + 1
        clamped = int((num >= S).sum())
        bx = np.minimum(Bx - 1, num * Bx // S)
        keep = np.ones(P, bool)
    else:
        num = np.asarray(union, np.int64) - np.asarray(inter, np.int64)
        den = np.asarray(union, np.int64) + int(cg)
        keep = den != 0
        undefined = int(P - keep.sum())
        bx = np.minimum(Bx - 1, num * Bx // np.maximum(den, 1))
    joint = np.bincount((bt * Bx + bx)[keep], minlength=(Bt + 1) * Bx).reshape(Bt + 1, Bx).astype(np.uint64)
    per_time = np.zeros((Bt + 1, 3), np.uint64)
    for row in range(Bt + 1):
        sel = keep & (bt == row)
        per_time[row] = (int(sel.sum()), int(num[sel].sum()), int(den[sel].sum()))
    return dict(joint=joint, per_time=per_time, pairs=P, core_sites=int(L), core_genes=int(cg), metric=metric,
                time_bins=Bt, dist_bins=Bx, time_span=St, core_span=S, depth=int(depth), undefined_pairs=undefined,
                core_clamped=clamped, beyond_pairs=int(per_time[Bt, 0]), binned_pairs=P - undefined,
                num_sum=int(per_time[:, 1].sum()), den_sum=int(per_time[:, 2].sum()))


def assert_clock(got, want):
    assert np.array_equal(got.joint, want["joint"]), (got.joint, want["joint"])
    assert np.array_equal(got.per_time, want["per_time"]), (got.per_time, want["per_time"])
    for name, value in want.items():
        if name not in ("joint", "per_time"):
            assert getattr(got, name) == value, (name, getattr(got, name), value)


def all_pairs(N):
    i, j = np.triu_indices(N, 1)
    return i.astype(np.uint32), j.astype(np.uint32)


# the files of pansim --print_genealogy
def genealogy_tsv(order, coal):
    N = len(order)
    lines = []
    for r in range(N):
        c = "" if r + 1 == N else "beyond" if int(coal[r]) == BEYOND else str(int(coal[r]))
        lines.append("%d\t%d\t%s\n" % (r, int(order[r]), c))
    return "".join(lines)


def clock_tsv(joint):
    return "".join("%d\t%d\t%d\n" % (t, x, int(joint[t, x])) for t in range(joint.shape[0]) for x in range(joint.shape[1]) if joint[t, x])


def clock_summary_tsv(clock, gen):
    names = ("pop_size", "pairs", "core_sites", "core_genes", "metric", "time_bins", "dist_bins", "time_span", "core_span", "generation",
             "capacity", "depth", "roots", "tmrca", "undefined_pairs", "core_clamped", "beyond_pairs", "binned_pairs", "num_sum", "den_sum")
    both = dict(gen)
    both.update({k: v for k, v in clock.items() if k not in ("joint", "per_time")})
    text = "".join("%s\t%d\n" % (n, int(both[n])) for n in names)
    pt = clock["per_time"]
    return text + "".join("time\t%d\t%d\t%d\t%d\n" % (t, int(pt[t, 0]), int(pt[t, 1]), int(pt[t, 2])) for t in range(pt.shape[0]) if pt[t, 0])
