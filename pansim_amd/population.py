"""Host-side mirror of the reference's `Population` API (pansim/src/population.rs:164-897)
over the C ABI of libpansim_hip.so.  Method names and argument meaning follow the
reference so that parity tests read like tests of the reference would.

All computation happens in the HIP library; this module only marshals buffers.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import PS_GROUPS_MAX, ClusterParams, Clusters, Config, CoreDiversity, Diff, DiffParams, Knn, KnnParams, Lineages, PairHist, PairHistParams, Tree, TreeParams, Upgma, check


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def hamming_bitwise_fast(x, y):
    """distances.rs:22-52"""
    x = np.ascontiguousarray(x, np.uint8)
    y = np.ascontiguousarray(y, np.uint8)
    if x.size != y.size:
        raise ValueError("slices must have the same length (distances.rs:24 assert_eq)")
    out = C.c_uint32()
    check(_lib.load().ps_hamming_bitwise_fast(x, y, x.size, C.byref(out)))
    return out.value


def jaccard_distance_fast(x, y):
    """distances.rs:55-77 -> (intersection, union)"""
    x = np.ascontiguousarray(x, np.uint8)
    y = np.ascontiguousarray(y, np.uint8)
    if x.size != y.size:
        raise ValueError("slices must have the same length (distances.rs:56 assert_eq)")
    a, b = C.c_uint32(), C.c_uint32()
    check(_lib.load().ps_jaccard_distance_fast(x, y, x.size, C.byref(a), C.byref(b)))
    return a.value, b.value


def standard_deviation(values):
    """population.rs:87-94 -> (std, mean)"""
    v = _f64(values)
    s, m = C.c_double(), C.c_double()
    check(_lib.load().ps_standard_deviation(v, v.size, C.byref(s), C.byref(m)))
    return s.value, m.value


def int_to_base(n):
    """population.rs:154-162"""
    return _lib.load().ps_int_to_base(int(n)).decode()


def fmt_f64(v):
    """Rust `{}` Display of an f64 (main.rs:481, :496, :546)."""
    buf = C.create_string_buffer(512)
    rc = _lib.load().ps_fmt_f64(float(v), buf, 512)
    if rc < 0:
        check(rc)
    return buf.value.decode()


def init_vector(seed, core, ncols, avg_gene_freq=0.0, col_offset=0):
    out = np.zeros(ncols, np.uint8)
    check(_lib.load().ps_init_vector(int(seed), int(bool(core)), int(col_offset), int(ncols),
                                     float(avg_gene_freq), out))
    return out


def sample_weights(num_genes, logw, n_genes, avg_gene_num, avg_pairwise_dists,
                   no_control_genome_size, genome_size_penalty, competition_strength):
    """population.rs:293-437 (host half of sample_indices)"""
    ng = np.ascontiguousarray(num_genes, np.int32)
    w = np.zeros(ng.size, np.float64)
    check(_lib.load().ps_sample_weights(ng, _f64(logw), ng.size, int(n_genes), int(avg_gene_num),
                                        _f64(avg_pairwise_dists), int(no_control_genome_size),
                                        float(genome_size_penalty), float(competition_strength), w))
    return w


def _weights(w, n_comp, cols, what):
    """n_comp x cols f32, row-major (one vector is taken as one compartment); None stays None"""
    if w is None:
        return None
    w = np.ascontiguousarray(w, np.float32)
    if w.ndim == 1:
        w = w.reshape(1, -1)
    if w.shape != (n_comp, cols):
        raise ValueError("%s weights must be (%d compartments, %d global columns)" % (what, n_comp, cols))
    return w


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _pair_arrays(r1, r2, core_h, acc_inter, acc_union):
    """the five per-pair arrays of a `*_from_counts` call, flat uint32; a numerator that is not given stays None"""
    arrays = [None if a is None else _u32(a).reshape(-1) for a in (r1, r2, core_h, acc_inter, acc_union)]
    if len({a.size for a in arrays if a is not None}) != 1 or arrays[0] is None or arrays[1] is None:
        raise ValueError("two indices, and one value of every numerator given, per pair")
    return arrays


def _metric(metric, core_const, acc_const):
    if metric not in ("core", "acc"):
        raise ValueError('metric must be "core" or "acc"')
    return core_const if metric == "core" else acc_const


def _timing(fn, n, handle):
    """the n device times in ms of a ps_*_timing entry"""
    t = [C.c_double() for _ in range(n)]
    check(fn(handle, *map(C.byref, t)))
    return tuple(x.value for x in t)


class _Summary:
    """What the result classes share: the fields of the C summary that FIELDS names as integer attributes, and as the head of
    `as_dict`."""
    FIELDS = ()

    def _take(self, summary):
        for name in self.FIELDS:
            setattr(self, name, int(getattr(summary, name)))

    def _head(self, *more):
        return {name: getattr(self, name) for name in self.FIELDS + more}


def site_tables(core, global_cols, mutations_vec, recombinations_vec, mutation_weights, recombination_weights=None):
    """The host tables of `Population.set_site_rates` (ps_site_tables; no device): a dict with the core plan fields
    `k`, `R`, `cshift`, `has_events`, `ranges` (True: the vectors are contiguous 0/1 masks, the set_rates path), `thresholds`
    (core: (global_cols, 7) level-2 thresholds; accessory: global_cols flip thresholds) and, accessory only, `hgt_weights`
    ((n_comp, global_cols) u16)."""
    lib = _lib.load()
    lm, lr = _f64(mutations_vec), _f64(recombinations_vec)
    cols = int(global_cols)
    wm = _weights(mutation_weights, lm.size, cols, "mutation")
    wr = _weights(recombination_weights, lm.size, cols, "recombination")
    plan = np.zeros(5, np.uint32)
    thr = np.zeros((cols, 7) if core else cols, np.uint32)
    wq = np.zeros((lm.size, cols), np.uint16)
    check(lib.ps_site_tables(int(bool(core)), cols, lm.size, lm, lr, _ptr(wm), _ptr(wr), _ptr(plan), _ptr(thr), _ptr(wq)))
    out = dict(k=int(plan[0]), R=int(plan[1]), cshift=int(plan[2]), has_events=int(plan[3]), ranges=bool(plan[4]), thresholds=thr)
    if not core:
        out["hgt_weights"] = wq
    return out


def _diversity_dict(d, spectrum):
    out = {name: int(getattr(d, name)) for name in ("pop_size", "sites", "other_cells", "segregating_sites", "pair_differences")}
    out["base_cells"] = [int(x) for x in d.base_cells]
    out["mean_pairwise_distance"] = float(d.mean_pairwise_distance)
    if spectrum is not None:
        out["spectrum"] = spectrum
    return out


def _diversity_call(fn, pop_size, spectrum, *head):
    """fn(*head, &summary, spectrum or NULL) -> the dict of Population.core_diversity"""
    d = CoreDiversity()
    spec = np.zeros(int(pop_size) + 1, np.uint64) if spectrum else None
    check(fn(*head, C.byref(d), _ptr(spec)))
    return _diversity_dict(d, spec)


def diversity_from_counts(counts, pop_size, spectrum=False):
    """The summary of `Population.core_diversity` from a (sites, 4) table of A, C, G, T counts, on the host alone
    (ps_diversity_from_counts; no device).  Cells a site's counts do not cover are its `other` class."""
    c = np.ascontiguousarray(counts, np.uint32)
    if c.ndim != 2 or c.shape[1] != 4:
        raise ValueError("counts must be (sites, 4): A, C, G, T per site")
    if int(pop_size) < 1:
        raise ValueError("pop_size must be >= 1")
    return _diversity_call(_lib.load().ps_diversity_from_counts, pop_size, spectrum, _ptr(c), c.shape[0], int(pop_size))


class DistanceHistogram(_Summary):
    """The result of `distance_histogram` (ps_pair_hist_t + the bins; docs/DISTANCE_HISTOGRAM.md): the summary fields as
    integer attributes (`core_d_sqsum` one Python integer), `mean_core_distance`, `joint` -- (core_bins, acc_bins) uint64 --
    and the two marginals `core_marginal` / `acc_marginal` (its row and column sums)."""
    FIELDS = ("pop_size", "pairs", "core_sites", "core_genes", "core_bins", "acc_bins", "core_span", "undefined_pairs",
              "core_clamped", "core_d_min", "core_d_max", "core_d_sum")

    def __init__(self, h, joint):
        self._take(h)
        self.core_d_sqsum = (int(h.core_d_sqsum_hi) << 64) | int(h.core_d_sqsum_lo)
        self.mean_core_distance = float(h.mean_core_distance)
        self.joint = joint.reshape(self.core_bins, self.acc_bins)
        self.core_marginal = self.joint.sum(axis=1, dtype=np.uint64)
        self.acc_marginal = self.joint.sum(axis=0, dtype=np.uint64)

    def core_bin_edges(self):
        """core_bins + 1 integers: bin k of the core axis holds the pairs with d in [edges[k], edges[k + 1]) -- edges[k] =
        ceil(k core_span / core_bins) -- and the last bin those with d >= core_span as well (`core_clamped` of them)"""
        return [-((-k * self.core_span) // self.core_bins) for k in range(self.core_bins + 1)]

    def as_dict(self):
        out = self._head("core_d_sqsum", "mean_core_distance")
        out.update(joint=self.joint, core_marginal=self.core_marginal, acc_marginal=self.acc_marginal)
        return out


def _hist_params(core_bins, acc_bins, core_max, core_sites, core_span=None):
    """core_max is a distance: core_span = max(1, ceil(core_max L)); None = automatic (span 0).  core_span, in units of
    d, overrides it."""
    prm = PairHistParams(int(core_bins), int(acc_bins), 0)
    if core_span is not None:
        prm.core_span = int(core_span)
    elif core_max is not None:
        if not float(core_max) > 0.0:
            raise ValueError("core_max must be > 0.0")
        prm.core_span = max(1, int(np.ceil(float(core_max) * int(core_sites))))
    return prm


def _hist_call(fn, prm, *head):
    """fn(*head, &params, &summary, joint) -> DistanceHistogram"""
    h = PairHist()
    joint = np.zeros(max(1, prm.core_bins * prm.acc_bins), np.uint64)      # (the library rejects bad bin counts itself)
    check(fn(*head, C.byref(prm), C.byref(h), _ptr(joint)))
    return DistanceHistogram(h, joint)


def histogram_from_counts(core_h, acc_inter, acc_union, core_sites, core_genes, core_bins=64, acc_bins=64, core_max=None,
                          core_span=None):
    """`Population.distance_histogram` from lists of pair numerators (`pairwise_counts` of both matrices), on the host
    alone (ps_histogram_from_counts; no device)."""
    h, i, u = _u32(core_h).reshape(-1), _u32(acc_inter).reshape(-1), _u32(acc_union).reshape(-1)
    if not h.size == i.size == u.size:
        raise ValueError("one core numerator, one intersection and one union per pair")
    prm = _hist_params(core_bins, acc_bins, core_max, core_sites, core_span)
    return _hist_call(_lib.load().ps_histogram_from_counts, prm, _ptr(h), _ptr(i), _ptr(u), h.size, int(core_sites), int(core_genes))


class StrainClusters(_Summary):
    """The result of `strain_clusters` (ps_cluster_t + the labels; docs/STRAIN_CLUSTERS.md): the summary fields as integer
    attributes and `labels` -- pop_size uint32, labels[k] the smallest row of k's cluster."""
    FIELDS = tuple(name for name, _ in Clusters._fields_)

    def __init__(self, c, labels):
        self._take(c)
        self.labels = labels

    def sizes(self):
        """the cluster sizes, descending"""
        return np.sort(np.bincount(self.labels)[np.unique(self.labels)])[::-1]

    def as_dict(self):
        out = self._head()
        out["labels"] = self.labels
        return out


def _cluster_params(core_sites, core_max=None, acc_max=None, core_max_d=None, acc_ratio=None):
    """The integer thresholds of a call.  Distances are converted once: core_max_d = floor(core_max L), acc_num / acc_den =
    floor(acc_max 2^20) / 2^20.  `core_max_d` (in units of d) and `acc_ratio` ((num, den)) give the integers themselves
    and override them; a criterion that is not given is not applied."""
    prm = ClusterParams(2**64 - 1, 0, 0)
    if core_max_d is not None:
        prm.core_max_d = int(core_max_d)
    elif core_max is not None:
        if not float(core_max) >= 0.0:
            raise ValueError("core_max must be >= 0.0")
        prm.core_max_d = min(2**64 - 2, int(np.floor(float(core_max) * int(core_sites))))
    if acc_ratio is not None:
        prm.acc_num, prm.acc_den = (int(x) for x in acc_ratio)
    elif acc_max is not None:
        if not 0.0 <= float(acc_max) <= 1.0:
            raise ValueError("acc_max must be in [0.0, 1.0]")
        prm.acc_num, prm.acc_den = int(np.floor(float(acc_max) * 2**20)), 2**20
    return prm


def _cluster_call(fn, prm, pop_size, *head):
    """fn(*head, &params, &summary, labels) -> StrainClusters"""
    c = Clusters()
    labels = np.zeros(max(1, int(pop_size)), np.uint32)
    check(fn(*head, C.byref(prm), C.byref(c), _ptr(labels)))
    return StrainClusters(c, labels[:int(pop_size)])


def clusters_from_counts(r1, r2, core_h, acc_inter, acc_union, pop_size, core_sites, core_genes, core_max=None, acc_max=None,
                         core_max_d=None, acc_ratio=None):
    """`Population.strain_clusters` from any list of pairs (r1, r2) and their numerators (`pairwise_counts` of both
    matrices), on the host alone (ps_clusters_from_counts; no device).  The numerators of a criterion that is not applied
    may be None."""
    arrays = _pair_arrays(r1, r2, core_h, acc_inter, acc_union)
    prm = _cluster_params(core_sites, core_max, acc_max, core_max_d, acc_ratio)
    return _cluster_call(_lib.load().ps_clusters_from_counts, prm, pop_size, *map(_ptr, arrays), arrays[0].size, int(pop_size),
                         int(core_sites), int(core_genes))


class LinkageTree(_Summary):
    """The result of `linkage_tree` (ps_tree_t + the edges; docs/LINKAGE_TREE.md): the summary fields as integer attributes,
    the tree's edges in ascending order of (distance, lo, hi) -- `lo`, `hi` (uint32 rows, lo < hi), `num`, `den` (uint64; the
    distance of edge k is num[k] / den[k], den 0 = undefined) -- and `distance` (float64, NaN where den is 0)."""
    FIELDS = tuple(name for name, _ in Tree._fields_)

    def __init__(self, t, lo, hi, num, den):
        self._take(t)
        n = self.edges
        self.lo, self.hi, self.num, self.den = lo[:n], hi[:n], num[:n], den[:n]
        with np.errstate(divide="ignore", invalid="ignore"):
            self.distance = np.where(self.den == 0, np.nan, self.num.astype(np.float64) / self.den.astype(np.float64))

    def _kept(self, num, den):
        """how many edges (a prefix: they ascend) have a distance <= num / den under the integer rule: defined and
        num[k] den <= num den[k] in whole numbers.  den == 0 keeps every edge, the undefined ones included."""
        num, den = int(num), int(den)
        if num < 0 or den < 0:
            raise ValueError("a threshold is num / den with num, den >= 0")
        k = 0
        while k < self.edges and (den == 0 or (int(self.den[k]) != 0 and int(self.num[k]) * den <= num * int(self.den[k]))):
            k += 1
        return k

    def cut(self, num, den):
        """labels (pop_size uint32, labels[k] the smallest row of k's cluster) after removing the edges with a distance
        above num / den: the labels of `strain_clusters` at that single threshold"""
        parent = np.arange(self.pop_size, dtype=np.uint32)

        def root(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for k in range(self._kept(num, den)):
            a, b = root(int(self.lo[k])), root(int(self.hi[k]))
            parent[max(a, b)] = min(a, b)
        return np.array([root(k) for k in range(self.pop_size)], np.uint32)

    def clusters_at(self, num, den):
        """the number of clusters of `cut(num, den)`: pop_size less the edges kept"""
        return self.pop_size - self._kept(num, den)

    def merges(self):
        """(left, right): the tree as a merge list in scipy's numbering, edge by edge (ps_merges_from_tree) -- what
        `tree_parsimony` takes"""
        from .parsimony import merges_from_tree
        return merges_from_tree(self.lo, self.hi, self.pop_size)

    def levels(self):
        """uint32 per merge: the dense rank (from 1) of its edge's distance (ps_levels_from_heights) -- the values
        `tree_compare` reads this tree with"""
        from .tree_compare import levels_from_heights
        return levels_from_heights(self.num, self.den)

    def as_dict(self):
        out = self._head()
        out.update(lo=self.lo, hi=self.hi, num=self.num, den=self.den, distance=self.distance)
        return out


def _tree_params(metric):
    return TreeParams(_metric(metric, _lib.PS_TREE_CORE, _lib.PS_TREE_ACC))


def _tree_call(fn, prm, pop_size, *head):
    """fn(*head, &params, &summary, lo, hi, num, den) -> LinkageTree"""
    t = Tree()
    n = max(1, int(pop_size))
    lo, hi, num, den = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    check(fn(*head, C.byref(prm), C.byref(t), _ptr(lo), _ptr(hi), _ptr(num), _ptr(den)))
    return LinkageTree(t, lo, hi, num, den)


def tree_from_counts(r1, r2, core_h, acc_inter, acc_union, pop_size, core_sites, core_genes, metric="core"):
    """`Population.linkage_tree` from any list of pairs (r1, r2) and their numerators (`pairwise_counts` of both matrices),
    on the host alone (ps_tree_from_counts; no device).  The numerators of the other metric may be None.  A list that does
    not connect everything gives the minimum spanning forest (`edges` < pop_size - 1)."""
    arrays = _pair_arrays(r1, r2, core_h, acc_inter, acc_union)
    return _tree_call(_lib.load().ps_tree_from_counts, _tree_params(metric), pop_size, *map(_ptr, arrays), arrays[0].size, int(pop_size),
                      int(core_sites), int(core_genes))


class _MergeCount(int):
    """`UpgmaTree.merges`: the number of merges, as before, which called gives the merge list (left, right) as
    `tree_parsimony` takes it -- `merges()` like the other two trees without renaming the summary field"""
    def __new__(cls, value, left, right):
        self = super().__new__(cls, value)
        self._lists = (left, right)
        return self

    def __call__(self):
        return self._lists


class UpgmaTree(_Summary):
    """The result of `upgma_tree` (ps_upgma_t + the merges; docs/UPGMA_TREE.md): the summary fields as integer attributes and the
    pop_size - 1 merges in the order the sequential algorithm performs them, scipy's linkage matrix with exact fractions --
    merge k creates node pop_size + k (the leaves are the rows), `left`, `right` (uint32) its children, `size` (uint32) its
    members, `num`, `den` (uint64) its distance num[k] / den[k], non-decreasing in k -- and `distance` (float64)."""
    FIELDS = tuple(name for name, _ in Upgma._fields_)

    def __init__(self, t, left, right, size, num, den):
        self._take(t)
        n = self.merges
        self.left, self.right, self.size, self.num, self.den = left[:n], right[:n], size[:n], num[:n], den[:n]
        self.merges = _MergeCount(n, self.left, self.right)
        self.distance = self.num.astype(np.float64) / self.den.astype(np.float64)

    def levels(self):
        """uint32 per merge: the dense rank (from 1) of its height (ps_levels_from_heights) -- the values `tree_compare`
        reads this tree with"""
        from .tree_compare import levels_from_heights
        return levels_from_heights(self.num, self.den)

    def _kept(self, num, den):
        """how many merges (a prefix: the heights do not descend) lie at or below num / den under the integer rule
        num[k] den <= num den[k]"""
        num, den = int(num), int(den)
        if num < 0 or den <= 0:
            raise ValueError("a threshold is num / den with num >= 0 and den > 0")
        k = 0
        while k < self.merges and int(self.num[k]) * den <= num * int(self.den[k]):
            k += 1
        return k

    def cut(self, num, den):
        """labels (pop_size uint32, labels[r] the smallest row of r's cluster) after every merge at or below num / den"""
        n = self.pop_size
        label = list(range(n)) + [0] * self.merges           # per node: the smallest row below it
        parent = list(range(n + self.merges))                # per node: the node it was merged into, among the merges kept
        for k in range(self._kept(num, den)):
            a, b = int(self.left[k]), int(self.right[k])
            parent[a] = parent[b] = n + k
            label[n + k] = min(label[a], label[b])
        for x in range(n + self.merges - 1, -1, -1):         # (a parent's number is above its children's: the roots first)
            if parent[x] != x:
                label[x] = label[parent[x]]
        return np.array(label[:n], np.uint32)

    def clusters_at(self, num, den):
        """the number of clusters of `cut(num, den)`: pop_size less the merges kept"""
        return self.pop_size - self._kept(num, den)

    def cophenetic(self, r1, r2):
        """(num, den), two uint64 arrays: the distance of the merge that first joins rows r1[k] and r2[k] -- the tree's own
        distance of the pair, the counterpart of `GenealogyResult.pairs`.  A node's number is above its children's, so the
        lower of the two climbs until they meet."""
        n = self.pop_size
        parent = [0] * (n + self.merges)
        for k in range(self.merges):
            parent[int(self.left[k])] = parent[int(self.right[k])] = n + k
        r1, r2 = _u32(r1).reshape(-1), _u32(r2).reshape(-1)
        if r1.size != r2.size:
            raise ValueError("two rows per pair")
        num, den = np.zeros(r1.size, np.uint64), np.zeros(r1.size, np.uint64)
        for k, (a, b) in enumerate(zip(r1.tolist(), r2.tolist())):
            if a >= n or b >= n or a == b:
                raise ValueError("pair %d: two different rows below pop_size" % k)
            while a != b:
                if a < b:
                    a = parent[a]
                else:
                    b = parent[b]
            num[k], den[k] = self.num[a - n], self.den[a - n]
        return num, den

    def newick(self):
        """the tree as one line of Newick text (ps_upgma_newick): leaves are rows, branch lengths half the difference of the
        two nodes' distances"""
        return upgma_newick(self.left, self.right, self.num, self.den, self.pop_size)

    def as_dict(self):
        out = self._head()
        out.update(left=self.left, right=self.right, size=self.size, num=self.num, den=self.den, distance=self.distance)
        return out


def upgma_newick(left, right, num, den, pop_size):
    """the merges of a UPGMA tree as one line of Newick text (ps_upgma_newick; host only)"""
    left, right = _u32(left).reshape(-1), _u32(right).reshape(-1)
    num, den = np.ascontiguousarray(num, np.uint64).reshape(-1), np.ascontiguousarray(den, np.uint64).reshape(-1)
    if not left.size == right.size == num.size == den.size == int(pop_size) - 1:
        raise ValueError("pop_size - 1 merges")
    lib, need = _lib.load(), C.c_uint64()
    check(lib.ps_upgma_newick(_ptr(left), _ptr(right), _ptr(num), _ptr(den), int(pop_size), None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    check(lib.ps_upgma_newick(_ptr(left), _ptr(right), _ptr(num), _ptr(den), int(pop_size), buf, need.value, C.byref(need)))
    return buf.value.decode()


def _upgma_call(fn, prm, pop_size, *head):
    """fn(*head, &params, &summary, left, right, size, num, den) -> UpgmaTree"""
    t = Upgma()
    n = max(1, int(pop_size))
    left, right, size = (np.zeros(n, np.uint32) for _ in range(3))
    num, den = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    check(fn(*head, C.byref(prm), C.byref(t), _ptr(left), _ptr(right), _ptr(size), _ptr(num), _ptr(den)))
    return UpgmaTree(t, left, right, size, num, den)


def upgma_from_counts(r1, r2, core_h, acc_inter, acc_union, pop_size, core_sites, core_genes, metric="core"):
    """`Population.upgma_tree` from the COMPLETE list of pairs (r1, r2), in any order and orientation, and their numerators
    (`pairwise_counts` of both matrices), by the sequential algorithm on the host alone (ps_upgma_from_counts; no device;
    O(pop_size^3) at worst).  The numerators of the other metric may be None."""
    arrays = _pair_arrays(r1, r2, core_h, acc_inter, acc_union)
    return _upgma_call(_lib.load().ps_upgma_from_counts, _tree_params(metric), pop_size, *map(_ptr, arrays), arrays[0].size, int(pop_size),
                       int(core_sites), int(core_genes))


class NearestNeighbours(_Summary):
    """The result of `nearest_neighbours` (ps_knn_t + the lists; docs/NEAREST_NEIGHBOURS.md): the summary fields as integer
    attributes and, as (pop_size, k) arrays, `nbr` (uint32: entry [i, r] is the r-th nearest other individual of row i in
    ascending order of (distance, row); 2^32 - 1 in a slot that a pair list left unfilled), `num`, `den` (uint64; the
    distance is num / den, den 0 = undefined) and `distance` (float64, NaN where den is 0)."""
    FIELDS = tuple(name for name, _ in Knn._fields_)

    def __init__(self, t, nbr, num, den):
        self._take(t)
        shape = (self.pop_size, self.k)
        self.nbr, self.num, self.den = nbr.reshape(shape), num.reshape(shape), den.reshape(shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.distance = np.where(self.den == 0, np.nan, self.num.astype(np.float64) / self.den.astype(np.float64))

    def lineages(self, rank=None):
        """(labels, summary) of the lineages at `rank` <= k (default k): the connected components of the graph that joins
        every individual to its first `rank` neighbours (ps_lineages_from_neighbours; host only).  labels: pop_size uint32,
        labels[i] the smallest row of i's lineage; summary: the fields of ps_lineage_t as a dict of ints."""
        out = Lineages()
        labels = np.zeros(self.pop_size, np.uint32)
        nbr = np.ascontiguousarray(self.nbr)
        check(_lib.load().ps_lineages_from_neighbours(_ptr(nbr), self.pop_size, self.k, self.k if rank is None else int(rank),
                                                      C.byref(out), _ptr(labels)))
        return labels, {name: int(getattr(out, name)) for name, _ in Lineages._fields_}

    def as_dict(self):
        out = self._head()
        out.update(nbr=self.nbr, num=self.num, den=self.den, distance=self.distance)
        return out


def _knn_params(k, metric):
    m = _metric(metric, _lib.PS_KNN_CORE, _lib.PS_KNN_ACC)
    if not 0 <= int(k) < 2**32:
        raise ValueError("k must fit 32 bits")
    return KnnParams(m, int(k))


def _knn_call(fn, prm, pop_size, *head):
    """fn(*head, &params, &summary, nbr, num, den) -> NearestNeighbours"""
    t = Knn()
    n = max(1, int(pop_size) * int(prm.k))
    nbr, num, den = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    check(fn(*head, C.byref(prm), C.byref(t), _ptr(nbr), _ptr(num), _ptr(den)))
    m = int(t.pop_size) * int(t.k)
    return NearestNeighbours(t, nbr[:m], num[:m], den[:m])


def neighbours_from_counts(r1, r2, core_h, acc_inter, acc_union, pop_size, core_sites, core_genes, k, metric="core"):
    """`Population.nearest_neighbours` from any list of pairs (r1, r2) and their numerators (`pairwise_counts` of both
    matrices), on the host alone (ps_neighbours_from_counts; no device).  The numerators of the other metric may be None.
    An individual with fewer than k listed partners has 2^32 - 1, 0, 0 in its unfilled slots."""
    arrays = _pair_arrays(r1, r2, core_h, acc_inter, acc_union)
    return _knn_call(_lib.load().ps_neighbours_from_counts, _knn_params(k, metric), pop_size, *map(_ptr, arrays), arrays[0].size,
                     int(pop_size), int(core_sites), int(core_genes))


class GroupDifferentiation(_Summary):
    """The result of `group_differentiation` (ps_diff_t + the arrays; docs/GROUP_DIFFERENTIATION.md): the integer summary
    fields as attributes, `pi_within`, `pi_between`, `fst`, and with K = `groups`: `group_of` (pop_size uint32, 2^32 - 1 =
    unassigned), `group_label`, `group_size` (K), `between`, `fixed` ((K, K) uint64); when asked for `site_within`,
    `site_total` (sites), `counts` ((sites, K, 4)) and, with an accessory matrix, `gene_counts` ((genes, K)), `acc_between`,
    `gene_fixed` ((K, K)) and `gene_private` (K).  What was not asked for is None."""
    FIELDS = tuple(name for name, kind in Diff._fields_ if kind is C.c_uint64)

    def __init__(self, d, **arrays):
        self._take(d)
        self.pi_within, self.pi_between, self.fst = float(d.pi_within), float(d.pi_between), float(d.fst)
        K = self.groups
        for name, a in arrays.items():
            if a is not None:
                if name in ("group_label", "group_size", "gene_private"):
                    a = a[:K].copy()
                elif name in ("between", "fixed", "acc_between", "gene_fixed"):
                    a = a[:K * K].reshape(K, K).copy()
                elif name == "counts":
                    a = a[:self.sites * K * 4].reshape(self.sites, K, 4).copy()
                elif name == "gene_counts":
                    a = a[:self.genes * K].reshape(self.genes, K).copy()
            setattr(self, name, a)

    ARRAYS = ("group_of", "group_label", "group_size", "between", "fixed", "site_within", "site_total", "counts", "gene_counts",
              "acc_between", "gene_fixed", "gene_private")

    def dxy(self):
        """(K, K) float64: between[g][h] / (n_g n_h sites) off the diagonal, pi() on it"""
        n = self.group_size.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = self.between.astype(np.float64) / (np.outer(n, n) * float(self.sites))
        out[np.diag_indices(self.groups)] = self.pi()
        return np.nan_to_num(out, nan=0.0, posinf=0.0)

    def pi(self):
        """K float64: the diversity of each group, between[g][g] / (n_g (n_g - 1) / 2) / sites (0.0 for a group of one)"""
        n = self.group_size.astype(np.float64)
        den = n * (n - 1.0) / 2.0 * float(self.sites)
        return np.divide(np.diag(self.between).astype(np.float64), den, out=np.zeros(self.groups), where=den > 0)

    def site_fst(self):
        """sites float64 (needs per_site): Hudson's F_ST of every site, 1 - (within / within_pairs) / (between /
        between_pairs) with between = site_total - site_within; 0.0 where a denominator is 0"""
        if self.site_within is None or self.site_total is None:
            raise ValueError("site_fst needs per_site=True")
        w = self.site_within.astype(np.float64)
        b = self.site_total.astype(np.float64) - w
        out = np.zeros(w.size)
        if self.within_pairs and self.between_pairs:
            ok = b > 0
            out[ok] = 1.0 - (w[ok] / self.within_pairs) / (b[ok] / self.between_pairs)
        return out

    def as_dict(self):
        out = self._head("pi_within", "pi_between", "fst")
        out.update({name: getattr(self, name) for name in self.ARRAYS})
        return out


def _diff_params(max_groups, min_size):
    if not 1 <= int(max_groups) <= PS_GROUPS_MAX:
        raise ValueError("max_groups must be 1 .. %d" % PS_GROUPS_MAX)
    if int(min_size) < 1:
        raise ValueError("min_size must be >= 1")
    return DiffParams(int(max_groups), int(min_size))


def _diff_call(fn, labels, pop_size, sites, genes, max_groups, min_size, per_site, counts, with_genes, *head):
    """fn(*head, labels, &params, &summary, the twelve arrays) -> GroupDifferentiation"""
    lab = _u32(labels).reshape(-1)
    if lab.size != int(pop_size):
        raise ValueError("one label per individual: %d, not %d" % (int(pop_size), lab.size))
    prm = _diff_params(max_groups, min_size)
    M, N, L, G = prm.max_groups, int(pop_size), int(sites), int(genes)
    a = dict(group_of=np.zeros(max(1, N), np.uint32), group_label=np.zeros(M, np.uint32), group_size=np.zeros(M, np.uint32),
             between=np.zeros(M * M, np.uint64), fixed=np.zeros(M * M, np.uint64),
             site_within=np.zeros(max(1, L), np.uint32) if per_site else None,
             site_total=np.zeros(max(1, L), np.uint32) if per_site else None,
             counts=np.zeros(max(1, L * M * 4), np.uint32) if counts else None,
             gene_counts=np.zeros(max(1, G * M), np.uint32) if with_genes else None,
             acc_between=np.zeros(M * M, np.uint64) if with_genes else None,
             gene_fixed=np.zeros(M * M, np.uint64) if with_genes else None,
             gene_private=np.zeros(M, np.uint64) if with_genes else None)
    d = Diff()
    check(fn(*head, _ptr(lab), C.byref(prm), C.byref(d), *[_ptr(a[name]) for name in GroupDifferentiation.ARRAYS]))
    a["group_of"] = a["group_of"][:N]
    for name in ("site_within", "site_total"):
        if a[name] is not None:
            a[name] = a[name][:L]
    return GroupDifferentiation(d, **a)


def groups_from_labels(labels, max_groups=16, min_size=1):
    """The group rules of `group_differentiation` on the host alone (ps_groups_from_labels; no device): -> (group_of,
    group_label, group_size).  A label with at least `min_size` members is a candidate; candidates are ranked by (size
    descending, label ascending) and the first `max_groups` are the groups; group_of is 2^32 - 1 for everyone else."""
    lab = _u32(labels).reshape(-1)
    prm = _diff_params(max_groups, min_size)
    group_of = np.zeros(max(1, lab.size), np.uint32)
    label, size = np.zeros(prm.max_groups, np.uint32), np.zeros(prm.max_groups, np.uint32)
    K = C.c_uint32()
    check(_lib.load().ps_groups_from_labels(_ptr(lab), lab.size, prm.max_groups, prm.min_size, _ptr(group_of), _ptr(label), _ptr(size),
                                            C.byref(K)))
    return group_of[:lab.size], label[:K.value].copy(), size[:K.value].copy()


def differentiation_from_counts(counts, group_size):
    """The core results of `group_differentiation` from a (sites, K, 4) table of per-group A, C, G, T counts and the K group
    sizes, on the host alone (ps_differentiation_from_counts; no device) -> a GroupDifferentiation with `between`, `fixed`,
    `site_within`, `site_total` and the summary.  Cells a group's counts do not cover are its `other` class."""
    n = _u32(group_size).reshape(-1)
    c = np.ascontiguousarray(counts, np.uint32)
    if c.ndim != 3 or c.shape[1] != n.size or c.shape[2] != 4:
        raise ValueError("counts must be (sites, groups, 4): A, C, G, T per site and group")
    K, L = n.size, c.shape[0]
    if not 1 <= K <= PS_GROUPS_MAX:
        raise ValueError("1 .. %d groups" % PS_GROUPS_MAX)
    between, fixed = np.zeros(K * K, np.uint64), np.zeros(K * K, np.uint64)
    within, total = np.zeros(max(1, L), np.uint32), np.zeros(max(1, L), np.uint32)
    d = Diff()
    check(_lib.load().ps_differentiation_from_counts(_ptr(c), L, K, _ptr(n), C.byref(d), _ptr(between), _ptr(fixed), _ptr(within),
                                                     _ptr(total)))
    return GroupDifferentiation(d, group_of=None, group_label=None, group_size=n.copy(), between=between, fixed=fixed,
                                site_within=within[:L], site_total=total[:L], counts=c, gene_counts=None, acc_between=None,
                                gene_fixed=None, gene_private=None)


def draw_parents(weights, seed, generation):
    """population.rs:440-443"""
    w = _f64(weights)
    idx = np.zeros(w.size, np.uint32)
    check(_lib.load().ps_draw_parents(w, w.size, int(seed), int(generation), idx))
    return idx


class Population:
    """`struct Population` (population.rs:164-170) with its HBM state.

    Population::new (population.rs:181-190) takes (size, allele_count, max_variants, core,
    avg_gene_freq, rng, core_genes, acc_sampling_vec); `rng` becomes `seed` (the build's
    seeded host stream) and `acc_sampling_vec` is accepted and ignored, as in the reference
    (population.rs:189, :216).
    """

    def __init__(self, size, allele_count, max_variants, core, avg_gene_freq, seed, core_genes,
                 acc_sampling_vec=None, *, col_offset=0, global_cols=None, device=-1, init_vec=None,
                 _handle=None, _owned=True):
        self._lib = _lib.load()
        self.core = bool(core)
        self.size = int(size)
        self.ncols = int(allele_count)
        self.core_genes = int(core_genes)
        self.seed = int(seed)
        self.global_cols = self.ncols if global_cols is None else int(global_cols)
        self._owned = _owned
        if _handle is not None:
            self._h = C.c_void_p(_handle)
            return
        if self.core and max_variants != 4:
            raise ValueError("core populations use 4 variants (main.rs:375)")
        cfg = Config(self.size, self.ncols, self.global_cols, int(col_offset), self.core_genes,
                     self.seed, int(self.core), int(device))
        if init_vec is None:
            init_vec = init_vector(seed, core, self.ncols, avg_gene_freq, col_offset)
        init_vec = np.ascontiguousarray(init_vec, np.uint8)
        if init_vec.size != self.ncols:
            raise ValueError("init_vec must have allele_count entries")
        self._h = C.c_void_p()
        check(self._lib.ps_population_create(C.byref(cfg), init_vec.ctypes.data_as(C.c_void_p),
                                             C.byref(self._h)))

    # -- lifetime ---------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and self._h.value and self._owned:
            self._lib.ps_population_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- state ------------------------------------------------------------------
    def load_matrix(self, rows):
        rows = np.ascontiguousarray(rows, np.uint8)
        if rows.shape != (self.size, self.ncols):
            raise ValueError("matrix must be (size, allele_count)")
        check(self._lib.ps_load_matrix(self._h, rows))

    def read_matrix(self):
        out = np.zeros((self.size, self.ncols), np.uint8)
        check(self._lib.ps_read_matrix(self._h, out))
        return out

    def set_rates(self, mutations_vec, recombinations_vec, comp_begin=None, comp_end=None):
        """The `mutations_vec` / `recombinations_vec` of mutate_alleles / recombine
        (population.rs:469, :546) and the gene range of each compartment's weight mask."""
        lm, lr = _f64(mutations_vec), _f64(recombinations_vec)
        if comp_begin is None:
            comp_begin, comp_end = [0], [self.global_cols]
        b = np.ascontiguousarray(comp_begin, np.uint64)
        e = np.ascontiguousarray(comp_end, np.uint64)
        check(self._lib.ps_set_rates(self._h, lm.size, lm, lr, b, e))

    def set_site_rates(self, mutations_vec, recombinations_vec, mutation_weights, recombination_weights=None):
        """The rates with the reference's weight vectors (`weighted_dist` of mutate_alleles, population.rs:467-471;
        `locus_weights` of recombine, :544-549): (n_comp, global_cols) f32 each, over the GLOBAL columns even on a site
        shard.  Core populations pass no recombination weights (:687-689 draws the site uniformly)."""
        lm, lr = _f64(mutations_vec), _f64(recombinations_vec)
        if lr.size != lm.size:
            raise ValueError("one recombination rate per mutation rate")
        wm = _weights(mutation_weights, lm.size, self.global_cols, "mutation")
        wr = _weights(recombination_weights, lm.size, self.global_cols, "recombination")
        if wm is None:
            raise ValueError("mutation weights are required")
        check(self._lib.ps_set_site_rates(self._h, lm.size, lm, lr, _ptr(wm), _ptr(wr)))

    # -- per-generation operators ---------------------------------------------------
    def next_generation(self, sample):
        """population.rs:450-465"""
        s = _u32(sample)
        if s.size != self.size:
            raise ValueError("sample must have one parent per individual")
        check(self._lib.ps_next_generation(self._h, s))

    def mutate_alleles(self, generation):
        """population.rs:467-542"""
        check(self._lib.ps_mutate_alleles(self._h, int(generation)))

    def recombine(self, generation):
        """population.rs:544-751"""
        check(self._lib.ps_recombine(self._h, int(generation)))

    def step(self, generation, sample, do_recombine=True):
        """next_generation + mutate_alleles + recombine fused (main.rs:445-464)"""
        s = _u32(sample)
        check(self._lib.ps_step(self._h, int(generation), s, int(bool(do_recombine))))

    def sample_indices(self, generation, avg_gene_num, avg_pairwise_dists, selection_coefficients,
                       verbose=False, no_control_genome_size=False, genome_size_penalty=0.99,
                       competition_strength=0.0):
        """population.rs:270-448"""
        idx = np.zeros(self.size, np.uint32)
        check(self._lib.ps_sample_indices(self._h, int(generation), int(avg_gene_num),
                                          _f64(avg_pairwise_dists), _f64(selection_coefficients),
                                          int(verbose), int(no_control_genome_size),
                                          float(genome_size_penalty), float(competition_strength), idx))
        return idx

    def fitness_terms(self, selection_coefficients):
        """population.rs:282-322 -> (num_genes, log_sum)"""
        ng = np.zeros(self.size, np.int32)
        lw = np.zeros(self.size, np.float64)
        check(self._lib.ps_fitness_terms(self._h, _f64(selection_coefficients), ng, lw))
        return ng, lw

    # -- measurements -----------------------------------------------------------------
    def average_distance(self):
        """population.rs:753-784"""
        out = np.zeros(self.size, np.float64)
        check(self._lib.ps_average_distance(self._h, out))
        return out

    def average_distance_rows(self, first, count):
        """rows [first, first + count) of average_distance (one rank's share of a row-sharded D-avg)"""
        out = np.zeros(int(count), np.float64)
        check(self._lib.ps_average_distance_rows(self._h, int(first), int(count), out))
        return out

    def pairwise_distances(self, max_distances, range1, range2):
        """population.rs:787-837"""
        r1, r2 = _u32(range1)[:max_distances], _u32(range2)[:max_distances]
        out = np.zeros(int(max_distances), np.float64)
        check(self._lib.ps_pairwise_distances(self._h, int(max_distances), np.ascontiguousarray(r1),
                                              np.ascontiguousarray(r2), out))
        return out

    def pairwise_counts(self, range1, range2):
        """integer numerators of pairwise_distances (host arrays)"""
        r1, r2 = _u32(range1), _u32(range2)
        a = np.zeros(r1.size, np.uint32)
        b = np.zeros(r1.size, np.uint32)
        check(self._lib.ps_pairwise_counts(self._h, r1.size, r1, r2, a.ctypes.data_as(C.c_void_p),
                                           b.ctypes.data_as(C.c_void_p), 0))
        return (a,) if self.core else (a, b)

    def pairwise_counts_device(self, range1, range2, out_a_ptr, out_b_ptr=0):
        """integer numerators written to caller-owned DEVICE memory (raw pointers)"""
        r1, r2 = _u32(range1), _u32(range2)
        check(self._lib.ps_pairwise_counts(self._h, r1.size, r1, r2, C.c_void_p(out_a_ptr),
                                           C.c_void_p(out_b_ptr), 1))

    def set_donor_shard(self, shard_rank, shard_count, fn=None):
        """HGT donors [N r / K, N (r + 1) / K) only (ps_set_donor_shard); `fn`: an _lib.EXCHANGE_FN object or None
        (own donors' events only).  The caller keeps `fn` alive."""
        ptr = C.cast(fn, C.c_void_p) if fn is not None else None
        self._exchange_fn = fn
        check(self._lib.ps_set_donor_shard(self._h, int(shard_rank), int(shard_count), ptr, None))

    def last_pair_form(self):
        """kernel form of the last core pair-count call (include/pansim_hip.h, PS_PAIR_FORM_*)"""
        return int(self._lib.ps_last_pair_form(self._h))

    def last_sweep_form(self):
        """kernel of the last core sweep launch (include/pansim_hip.h, PS_SWEEP_FORM_*)"""
        return int(self._lib.ps_last_sweep_form(self._h))

    def gene_frequencies(self):
        """population.rs:840-863"""
        out = np.zeros(self.ncols + self.core_genes, np.float64)
        check(self._lib.ps_gene_frequencies(self._h, out))
        return out

    def site_allele_counts(self):
        """core counterpart of gene_frequencies (the reference has none): (ncols, 4) uint32, the cells of every site of
        this handle that are A, C, G, T (bytes 1, 2, 4, 8); docs/CORE_DIVERSITY.md"""
        out = np.zeros((self.ncols, 4), np.uint32)
        check(self._lib.ps_site_allele_counts(self._h, _ptr(out)))
        return out

    def core_diversity(self, spectrum=False):
        """the diversity summary of this handle's core sites (ps_core_diversity): a dict of the fields of
        ps_core_diversity_t -- pop_size, sites, other_cells, segregating_sites, pair_differences, base_cells (A, C, G, T),
        mean_pairwise_distance -- plus, on request, `spectrum`: pop_size + 1 bins of sites by minor count"""
        return _diversity_call(self._lib.ps_core_diversity, self.size, spectrum, self._h)

    def distance_histogram(self, acc, core_bins=64, acc_bins=64, core_max=None, core_span=None):
        """the joint histogram of (core distance, accessory Jaccard distance) over ALL pairs of this core population and
        the accessory population `acc` of the same individuals (ps_distance_histogram; docs/DISTANCE_HISTOGRAM.md) -> a
        DistanceHistogram.  `core_max`: the upper end of the core axis as a distance (None: just above the largest)."""
        prm = _hist_params(core_bins, acc_bins, core_max, self.global_cols, core_span)
        return _hist_call(self._lib.ps_distance_histogram, prm, self._h, acc._h)

    def distance_histogram_timing(self):
        """device ms of (the count kernels, the binning kernel) of the last distance_histogram() on this core handle"""
        return _timing(self._lib.ps_distance_histogram_timing, 2, self._h)

    def strain_clusters(self, acc, core_max=None, acc_max=None, core_max_d=None, acc_ratio=None):
        """the single-linkage clusters of ALL individuals of this core population and the accessory population `acc` of
        the same individuals (ps_strain_clusters; docs/STRAIN_CLUSTERS.md) -> a StrainClusters.  A pair is joined when its
        core distance is at most `core_max` and its accessory distance at most `acc_max` (either may be left out)."""
        prm = _cluster_params(self.global_cols, core_max, acc_max, core_max_d, acc_ratio)
        return _cluster_call(self._lib.ps_strain_clusters, prm, self.size, self._h, acc._h)

    def linkage_tree(self, acc, metric="core"):
        """the single-linkage tree -- the minimum spanning tree over ALL pairs -- of this core population and the accessory
        population `acc` of the same individuals under the core (`"core"`) or the accessory (`"acc"`) distance
        (ps_linkage_tree; docs/LINKAGE_TREE.md) -> a LinkageTree"""
        return _tree_call(self._lib.ps_linkage_tree, _tree_params(metric), self.size, self._h, acc._h)

    def upgma_tree(self, acc, metric="core"):
        """the average-linkage (UPGMA) tree over ALL pairs of this core population and the accessory population `acc` of the
        same individuals under the core (`"core"`) or the accessory (`"acc"`) distance (ps_upgma_tree; docs/UPGMA_TREE.md) ->
        an UpgmaTree"""
        return _upgma_call(self._lib.ps_upgma_tree, _tree_params(metric), self.size, self._h, acc._h)

    def upgma_tree_timing(self):
        """device ms of (the count kernels, the store kernels, the rounds) of the last upgma_tree() on this core handle"""
        return _timing(self._lib.ps_upgma_tree_timing, 3, self._h)

    def neighbour_joining(self, acc, metric="core"):
        """the neighbour-joining tree over ALL pairs of this core population and the accessory population `acc` of the same
        individuals under the core (`"core"`) or the accessory (`"acc"`) distance (ps_neighbour_joining;
        docs/NEIGHBOUR_JOINING.md) -> a NeighbourJoiningTree"""
        from .joining import _nj_call
        return _nj_call(self._lib.ps_neighbour_joining, _tree_params(metric), self.size, self._h, acc._h)

    def neighbour_joining_timing(self):
        """device ms of (the count kernels, the store kernels and the row sums, the joins) of the last neighbour_joining() on
        this core handle"""
        return _timing(self._lib.ps_neighbour_joining_timing, 3, self._h)

    def bootstrap_support(self, acc, method="nj", replicates=100, seed=0, draws=None, sites=None):
        """Felsenstein's bootstrap of a tree of ALL pop_size individuals under the core distance (this handle the core matrix,
        one-hot; `acc` its accessory one): the tree of `method` ("linkage", "upgma" or "nj"), then `replicates` trees of
        `draws` (None: all) core sites resampled with replacement on the device -- drawn under the key `seed`, or the rows of
        `sites` ((replicates, draws) global site indices) -- and how often every merge of the first comes back
        (ps_bootstrap_support; docs/BOOTSTRAP_SUPPORT.md) -> a BootstrapSupport"""
        from .bootstrap import _boot_call
        return _boot_call(self._lib.ps_bootstrap_support, self.size, method, replicates, seed, draws, sites, self._h, acc._h)

    def bootstrap_support_timing(self):
        """device ms of (the site lists, the operands: pack + counts + store, the trees), summed over the replicates of the last
        bootstrap_support() on this (core) handle (HIP events)"""
        return _timing(self._lib.ps_bootstrap_timing, 3, self._h)

    def nearest_neighbours(self, acc, k, metric="core"):
        """the k nearest other individuals of every individual among ALL of this core population and the accessory population
        `acc` of the same individuals, under the core (`"core"`) or the accessory (`"acc"`) distance, in ascending order of
        (distance, row) (ps_nearest_neighbours; docs/NEAREST_NEIGHBOURS.md) -> a NearestNeighbours"""
        return _knn_call(self._lib.ps_nearest_neighbours, _knn_params(k, metric), self.size, self._h, acc._h)

    def nearest_neighbours_timing(self):
        """device ms of (the count kernels, the select kernels) of the last nearest_neighbours() on this core handle"""
        return _timing(self._lib.ps_nearest_neighbours_timing, 2, self._h)

    def linkage_tree_timing(self):
        """device ms of (the count kernels, the store kernels, the rounds) of the last linkage_tree() on this core handle"""
        return _timing(self._lib.ps_linkage_tree_timing, 3, self._h)

    def strain_clusters_timing(self):
        """device ms of (the count kernels, the edge kernel, the label rounds) of the last strain_clusters() on this core handle"""
        return _timing(self._lib.ps_strain_clusters_timing, 3, self._h)

    def group_differentiation(self, labels, acc=None, max_groups=16, min_size=1, per_site=False, counts=False):
        """how the groups that `labels` name (one value per individual, the reference's row order: the labels of
        strain_clusters, clusters_at, lineages ...) differ on this core population and, if given, the accessory population
        `acc` of the same individuals (ps_group_differentiation; docs/GROUP_DIFFERENTIATION.md) -> a GroupDifferentiation.
        `per_site`: site_within / site_total as well; `counts`: the (sites, K, 4) per-group allele counts as well."""
        return _diff_call(self._lib.ps_group_differentiation, labels, self.size, self.ncols, acc.ncols if acc is not None else 0,
                          max_groups, min_size, per_site, counts, acc is not None, self._h, acc._h if acc is not None else None)

    def group_differentiation_timing(self):
        """device ms of (the membership tables, the core pass, the gene pass) of the last group_differentiation() on this core handle"""
        return _timing(self._lib.ps_group_differentiation_timing, 3, self._h)

    def tree_parsimony(self, left, right, acc=None, per_site=False, branches=False, genes=False):
        """Fitch parsimony of every site of this core population and, with `genes`, every gene of the accessory population
        `acc` of the same individuals on the tree of the merge list (left, right) -- `UpgmaTree.merges()`,
        `LinkageTree.merges()`, `GenealogyResult.merges()[:2]`; leaves are rows of the reference's row order
        (ps_tree_parsimony; docs/TREE_PARSIMONY.md) -> a TreeParsimony.  `per_site`: site_changes as well; `branches`:
        branch_changes (and with `genes` branch_gains, branch_losses) as well; `genes`: gene_changes, gene_gains, gene_losses."""
        from .parsimony import _pars_call
        if genes and acc is None:
            raise ValueError("genes=True needs the accessory population")
        return _pars_call(self._lib.ps_tree_parsimony, left, right, self.size, self.ncols, acc.ncols if genes else 0, per_site, branches,
                          genes, self._h, acc._h if acc is not None else None)

    def tree_parsimony_timing(self):
        """device ms of (the schedule's upload, the core pass, the gene pass) of the last tree_parsimony() on this core handle"""
        return _timing(self._lib.ps_tree_parsimony_timing, 3, self._h)

    def tree_nni(self, left, right, max_rounds=1000, moves_per_round=0):
        """Parsimony tree search from the spanning tree of the merge list (left, right): nearest-neighbour interchanges towards
        a local optimum of the Fitch length over the sites of this core population (ps_tree_nni; docs/PARSIMONY_SEARCH.md) ->
        a ParsimonySearch.  Every round is one pass of the device over the core matrix; at most `max_rounds` rounds of at most
        `moves_per_round` interchanges (0: no cap)."""
        from .search import _nni_call
        return _nni_call(self._lib.ps_tree_nni, left, right, self.size, max_rounds, moves_per_round, self._h)

    def nni_deltas(self, left, right):
        """One pass on the merge list as given (ps_tree_nni_deltas) -> (total_changes, delta): delta[k, kind] = the change of
        the total under candidate (pop_size + k, kind), PS_NNI_NONE where there is none"""
        from .search import _deltas_call
        return _deltas_call(self._lib.ps_tree_nni_deltas, left, right, self._h)

    def tree_nni_timing(self):
        """device ms of (the uploads of the schedules, the kernels) of the last tree_nni() or nni_deltas() on this core handle,
        summed over its passes"""
        return _timing(self._lib.ps_tree_nni_timing, 2, self._h)

    def tree_likelihood(self, left, right, lengths, per_site=False, derivatives=False):
        """The Jukes-Cantor likelihood of the spanning tree of the merge list (left, right) with `lengths` (pop_size + merges
        float64: substitutions per site on the branch above every node, the root's ignored) over the sites of this core
        population, in one pass (ps_tree_likelihood; docs/TREE_LIKELIHOOD.md) -> a TreeLikelihood.  `per_site`: every site's
        likelihood; `derivatives`: the sums behind the first and second derivative with respect to every branch."""
        from .likelihood import _lik_call
        return _lik_call(self._lib.ps_tree_likelihood, left, right, lengths, self.size, self.ncols, per_site, derivatives, self._h)

    def tree_ml_lengths(self, left, right, lengths=None, max_rounds=50, eps_lnl=1e-3):
        """Maximum-likelihood branch lengths of the tree under Jukes-Cantor by damped Newton steps on all branches at once
        (ps_tree_ml_lengths; docs/TREE_LIKELIHOOD.md) -> an MlLengths.  `lengths`: the start lengths (None: the Jukes-Cantor
        correction of the parsimony changes of every branch, jc_lengths_from_changes of tree_parsimony)."""
        from .likelihood import _ml_call, _start_lengths
        if lengths is None:
            lengths = _start_lengths(self, left, right)
        return _ml_call(self._lib.ps_tree_ml_lengths, left, right, lengths, self.size, max_rounds, eps_lnl, self._h)

    def tree_likelihood_timing(self):
        """device ms of (the uploads of the schedules, the kernels, the sums of the workgroups' rows) of the last
        tree_likelihood() or tree_ml_lengths() on this core handle, summed over its passes"""
        return _timing(self._lib.ps_tree_likelihood_timing, 3, self._h)

    def tree_model_likelihood(self, left, right, lengths, model, per_site=False, derivatives=False):
        """The likelihood of the tree under `model` (a SubstModel: F81 base frequencies, a root distribution, rate categories) over
        the sites of this core population, in one pass (ps_tree_model_likelihood; docs/TREE_MODEL.md) -> a ModelLikelihood.
        `per_site`: every site's likelihood and posterior mean rate; `derivatives`: the sums behind the first and second derivative
        with respect to every branch (pop_size <= PS_MODEL_MAX_POP_DERIV).  `model.site_class`: one entry per site of this handle."""
        from .models import _model_call
        return _model_call(self._lib.ps_tree_model_likelihood, left, right, lengths, model, self.size, self.ncols, per_site, derivatives, self._h)

    def tree_model_ml_lengths(self, left, right, model, lengths=None, max_rounds=50, eps_lnl=1e-3):
        """Maximum-likelihood branch lengths of the tree under `model` by the damped Newton steps of tree_ml_lengths
        (ps_tree_model_ml_lengths; docs/TREE_MODEL.md) -> a ModelMlLengths.  `lengths`: the start lengths (None: the F81 correction
        of the parsimony changes of every branch, f81_lengths_from_changes of tree_parsimony)."""
        from .models import _model_ml_call, _model_start_lengths
        if lengths is None:
            lengths = _model_start_lengths(self, left, right, model)
        return _model_ml_call(self._lib.ps_tree_model_ml_lengths, left, right, lengths, model, self.size, max_rounds, eps_lnl, self._h)

    def model_nni_deltas(self, left, right, lengths, model):
        """One pass of the likelihood tree search on the merge list as given (ps_tree_model_nni_deltas;
        docs/LIKELIHOOD_SEARCH.md) -> a ModelNniDeltas: `lnl` of the tree under `model` over the sites of this core population and
        `delta[k, kind]`, the exact change of lnL under interchange (pop_size + k, kind), NaN where there is no candidate"""
        from .ml_search import _deltas_call
        return _deltas_call(self._lib.ps_tree_model_nni_deltas, left, right, lengths, model, self.size, self._h)

    def tree_model_nni(self, left, right, model, lengths=None, max_rounds=1000, moves_per_round=0, length_rounds=5, eps_gain=1e-3):
        """Nearest-neighbour interchanges of the spanning tree (left, right) with branch lengths towards a local optimum of its
        likelihood under `model` over the sites of this core population (ps_tree_model_nni; docs/LIKELIHOOD_SEARCH.md) -> a
        LikelihoodSearch.  `lengths`: the start lengths (None: the F81 correction of the parsimony changes); `length_rounds`: rounds
        of tree_model_ml_lengths before every pass (0: the lengths travel with their subtrees unchanged)."""
        from .ml_search import _search_call
        from .models import _model_start_lengths
        if lengths is None:
            lengths = _model_start_lengths(self, left, right, model)
        return _search_call(self._lib.ps_tree_model_nni, left, right, lengths, model, self.size, max_rounds, moves_per_round, length_rounds,
                            eps_gain, self._h)

    def tree_model_nni_timing(self):
        """device ms of (the uploads, the kernels, the products of the workgroups' rows) of the search passes of the last
        tree_model_nni() or model_nni_deltas() on this core handle, summed"""
        return _timing(self._lib.ps_tree_model_nni_timing, 3, self._h)

    def tree_model_timing(self):
        """device ms of (the uploads, the kernels, the sums of the workgroups' rows) of the last tree_model_likelihood() or
        tree_model_ml_lengths() on this core handle, summed over its passes"""
        return _timing(self._lib.ps_tree_model_timing, 3, self._h)

    def ancestral_states(self, left, right, lengths, model, min_posterior=0.0, states=True):
        """The marginal reconstruction of every inner node of the tree under `model` over the sites of this core population, in one
        pass (ps_tree_ancestral_states; docs/ANCESTRAL_STATES.md) -> an AncestralStates whose `population` holds the merges
        reconstructed genomes on the device (row k = node pop_size + k; None without `states`).  A cell whose largest posterior is
        below `min_posterior` is written 0.  `model.site_class`: one entry per site of this handle."""
        from .ancestral import _device_call
        return _device_call(self._lib.ps_tree_ancestral_states, self, self.ncols, left, right, lengths, model, self.size, min_posterior, states, self._h)

    def ancestral_states_timing(self):
        """device ms of (the uploads, the kernel with its stores, the sums of the workgroups' rows) of the last ancestral_states()
        on this core handle"""
        return _timing(self._lib.ps_ancestral_states_timing, 3, self._h)

    def tree_gene_likelihood(self, left, right, lengths, model, per_gene=False):
        """The likelihood of the genes of this ACCESSORY population on the tree under the gain / loss `model` (a GeneModel), in one
        up pass (ps_tree_gene_likelihood; docs/GENE_MODEL.md) -> a GeneLikelihood; `per_gene`: every gene's (mantissa,
        exponent), class posteriors and posterior mean rate.  `lengths` are clamped below only: generations are fine."""
        from .gene_model import _lik_call
        return _lik_call(self._lib.ps_tree_gene_likelihood, left, right, lengths, model, self.size, self.ncols, per_gene, self._h)

    def tree_gene_ancestral(self, left, right, lengths, model, states=True):
        """The marginal gene content of every inner node of the tree under `model`, with the expected gains and losses of every
        branch and gene (ps_tree_gene_ancestral) -> a GeneAncestral whose `population` is a new accessory Population of merges
        rows on the device (row k = node pop_size + k; None without `states`)."""
        from .gene_model import _anc_device_call
        return _anc_device_call(self._lib.ps_tree_gene_ancestral, self, left, right, lengths, model, self.size, states, self._h)

    def tree_gene_fit(self, left, right, lengths, model, fit_rates=True, fit_freq=True, fit_weights=True, max_rounds=50, eps_lnl=1e-3):
        """The rates, pi_1 and (a mixture) the weights of `model` fitted to the genes of this accessory population on the tree,
        derivative-free and deterministic (ps_tree_gene_fit) -> a GeneFit; equal bit for bit to gene_fit_from_rows on the same
        matrix"""
        from .gene_model import _fit_call
        return _fit_call(self._lib.ps_tree_gene_fit, left, right, lengths, model, self.size, fit_rates, fit_freq, fit_weights, max_rounds,
                         eps_lnl, self._h)

    def tree_gene_timing(self):
        """device ms of (the uploads, the kernels with their stores, the sums of the workgroups' rows) of the last tree_gene_*()
        call on this accessory handle, summed over its passes"""
        return _timing(self._lib.ps_tree_gene_timing, 3, self._h)

    def tree_compare(self, a, b, bins=(32, 32), spans=(0, 0), triplets=True, values=None):
        """How well tree `b` recovers tree `a` over the pop_size leaves of this handle (ps_tree_compare;
        docs/TREE_COMPARISON.md) -> a TreeComparison: the cophenetic agreement over all pairs, the rooted triplets both
        resolve alike (`triplets`), the shared clades.  A tree is a `(left, right)` or `(left, right, val)` tuple, a
        LinkageTree or an UpgmaTree (values: `levels()`) or a GenealogyResult (values: the coalescence times); `values`:
        a pair (val_a, val_b) that replaces them (None: keep).  Any handle will do: no matrix is read."""
        from .tree_compare import _compare_call
        return _compare_call(self._lib.ps_tree_compare, self._h, a, b, bins, spans, triplets, values)

    def tree_compare_timing(self):
        """device ms of (the uploads and the tables, the pass over all pairs) of the last tree_compare() on this handle"""
        return _timing(self._lib.ps_tree_compare_timing, 2, self._h)

    def locus_ld(self, r2_bins=64, lag_bins=1, min_minor=1, max_loci=4096, loci=None):
        """linkage disequilibrium between the columns of this handle -- core sites or accessory genes by its kind
        (ps_locus_ld; docs/LINKAGE_DISEQUILIBRIUM.md) -> a LocusLd: r^2 and the four-gamete test over all pairs of the
        selected loci, binned by r^2 and by log2 of the distance between the columns.  `loci`: an explicit strictly
        ascending list of columns (None: the columns with minor count >= min_minor, thinned evenly to max_loci)."""
        from .linkage import _ld_call, _ld_params
        return _ld_call(self._lib.ps_locus_ld, _ld_params(r2_bins, lag_bins, min_minor, max_loci), loci, self._h)

    def locus_ld_timing(self):
        """device ms of (counts and selection, packing, the contraction, the pair statistics) of the last locus_ld()"""
        return _timing(self._lib.ps_locus_ld_timing, 4, self._h)

    def gene_site_ld(self, acc, r2_bins=64, freq_bins=1, site_min_minor=1, gene_min_minor=1, max_sites=4096, max_genes=4096, strong_q=32768,
                     sites=None, genes=None):
        """gene-site association of this core handle's sites with the genes of the accessory handle `acc` of the same individuals
        (ps_gene_site_ld; docs/GENE_SITE_ASSOCIATION.md) -> a GeneSiteLd: r^2 over all (gene, site) pairs of the two selected
        lists, binned by r^2 and the gene's minor frequency, and the best tag of every gene and site; `sites` / `genes`: an
        explicit strictly ascending list of columns instead of that side's automatic selection"""
        from .association import _gs_call, _gs_params
        prm = _gs_params(r2_bins, freq_bins, site_min_minor, gene_min_minor, max_sites, max_genes, strong_q)
        return _gs_call(self._lib.ps_gene_site_ld, prm, sites, genes, self._h, acc._h)

    def gene_site_ld_timing(self):
        """device ms of (counts and selection, packing, the contraction, the pair statistics) of the last gene_site_ld()"""
        return _timing(self._lib.ps_gene_site_ld_timing, 4, self._h)

    def allele_profiles(self, n_loci, bounds=None, dist_bins=None, complex_max=0, want_profiles=True, key_seed=0, key_bits=64):
        """core allele profiles (cgMLST) of this core handle (ps_allele_profiles; docs/ALLELE_PROFILES.md) -> an AlleleProfiles:
        the sites are cut into `n_loci` loci (evenly, or at the n_loci + 1 sites of `bounds`), every distinct sequence of a locus
        is an allele, and two individuals are as far apart as they have loci with different alleles; the sequence types, the
        single-linkage complexes at `complex_max` loci and the histogram of all pairs (`dist_bins`: n_loci + 1, capped at 16384,
        when None)"""
        from .mlst import _mlst_device_call
        return _mlst_device_call(self._lib.ps_allele_profiles, self._h, self.size, n_loci, bounds, dist_bins, complex_max, want_profiles, key_seed,
                                 key_bits)

    def allele_profiles_timing(self):
        """device ms of (the fingerprints, the allele numbers, the verification, the pairs, the label rounds) of the last
        allele_profiles()"""
        return _timing(self._lib.ps_allele_profiles_timing, 5, self._h)

    def subset(self, rows=None):
        """the rows `rows` of this population (output rows as every read-out numbers them; they may repeat; None = all) as a new,
        owned Population on the device, to which every read-out applies (ps_population_subset; docs/ISOLATE_SAMPLES.md); this
        population is read, not changed"""
        from .samples import _rows, _wrap
        r, h = _rows(rows), C.c_void_p()
        n = self.size if r is None else r.size
        check(self._lib.ps_population_subset(self._h, _ptr(r), n, C.byref(h)))
        return _wrap(self, h, n)

    def subset_timing(self):
        """device ms of the gather(s) that filled this population, which subset() or pool() made"""
        return _timing(self._lib.ps_population_subset_timing, 1, self._h)[0]

    def core_diversity_timing(self):
        """device ms of the counts kernel of the last site_allele_counts() / core_diversity() call"""
        ms = C.c_double()
        check(self._lib.ps_core_diversity_timing(self._h, C.byref(ms)))
        return ms.value

    def calc_gene_freq(self):
        """population.rs:244-268"""
        v = C.c_double()
        check(self._lib.ps_calc_gene_freq(self._h, C.byref(v)))
        return v.value

    def write(self, outpref):
        """population.rs:865-897"""
        check(self._lib.ps_write(self._h, str(outpref).encode()))

    def sync(self):
        check(self._lib.ps_sync(self._h))

    def set_tuning(self, key, value):
        """launch tuning / test hooks of ps_set_tuning (no reference counterpart)"""
        check(self._lib.ps_set_tuning(self._h, key.encode(), int(value)))

    def get_tuning(self, key):
        """the value of a ps_set_tuning switch as it is now (ps_get_tuning)"""
        value = C.c_int64(0)
        check(self._lib.ps_get_tuning(self._h, key.encode(), C.byref(value)))
        return int(value.value)
