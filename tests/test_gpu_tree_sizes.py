"""The all-pairs trees and clusters on the device at the sizes they are quoted and capped at: ps_upgma_tree, ps_linkage_tree,
ps_strain_clusters and ps_bootstrap_support above N = 300, where the other device tests of these read-outs stop.

* N = 4096 and N = 16384 (the cap of the UPGMA tree) against the closed forms of tests/planted_trees.py, which
  tests/test_planted_trees.py holds to the plain-Python references at N = 8, 64 and 128: the second trip of
  upgma_merge_rows_kernel's pair loop (more than 1024 pairs in a round), 32 trips of upgma_merge_cols_kernel's lane loop, four
  trips of the store kernels' row loop (a band of more than 4096 rows), thousands of rows per component in
  tree_comp_min_kernel, long chains in tree_jump_kernel, 2048 shared edges at once in tree_link_kernel, an adjacency bit matrix
  of 64 words per row.
* The 128-bit comparator of the UPGMA rounds (ps_up_dist_cmp's device body) on a designed population whose merge list changes
  under every one of three wrong comparators, which the test checks of its own input before it calls the device.
* The cfg2 population (N = 1000, L = 130, G = 40) against the library's host forms over the numerators of ps_pairwise_counts.
* Bootstrap support at N = 1030 by its known answers.

Measured on one MI355X (pytest's call times, host work included): test_upgma_at_the_cap 0.19 s and test_linkage_at_the_cap
0.18 s (N = 16384, each with its own load of the 268 MB matrix), the five tests on the N = 4096 fixture 0.53 s together and its
set-up 0.48 s; the slowest test of the file is the comparator's, 2.1 s, nearly all of it the four runs of the sequential
algorithm in Python."""
import numpy as np
import pytest

import bootstrap_ref
import linkage_tree_ref
import planted_trees as planted
import strain_clusters_ref
import upgma_tree_ref

pytestmark = pytest.mark.gpu

BASES = np.array([1, 2, 4, 8], np.uint8)
METRICS = (("core", planted.CORE), ("acc", planted.ACC))
NO_CORE = strain_clusters_ref.NO_CORE


def _handles(pa, core_matrix, acc_matrix, cg):
    N, L = core_matrix.shape
    core = pa.Population(N, L, 4, True, 0.0, 0, cg)
    core.load_matrix(core_matrix)
    acc = pa.Population(N, acc_matrix.shape[1], 2, False, 0.5, 0, cg)
    acc.load_matrix(acc_matrix)
    return core, acc


def _device_numerators(core, acc):
    """(r1, r2, h, I, U) of every pair i < j from the sampled-pair path, which shares nothing with the all-pairs read-outs"""
    r1, r2 = upgma_tree_ref.all_pairs(core.size)
    (h,) = core.pairwise_counts(r1, r2)
    i, u = acc.pairwise_counts(r1, r2)
    return r1, r2, h, i, u


# ---- N = 4096: both metrics against the closed forms -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mid(pa):
    """K = 12, c = 2: N = 4096, L = G = 8190, core_genes 3"""
    p = planted.Planted(12, c=2, core_genes=3, seed=4096)
    core, acc = _handles(pa, p.core_matrix(), p.acc_matrix(), 3)
    yield p, core, acc
    core.close()
    acc.close()


@pytest.mark.parametrize("name,metric", METRICS)
def test_upgma_at_4096(mid, name, metric):
    """12 rounds that halve the clusters: 2048, 1024, ... 1 mutual pairs"""
    p, core, acc = mid
    want = p.upgma(metric)
    first_round = int((want["size"] == 2).sum())
    assert first_round > 1024 and first_round > 64 * 2          # a second trip of both merge kernels' pair loops
    got = core.upgma_tree(acc, metric=name)
    upgma_tree_ref.assert_equal(got, want, p.N)
    assert got.rounds == want["rounds"] == 12


@pytest.mark.parametrize("name,metric", METRICS)
def test_linkage_at_4096(mid, name, metric):
    """the unique minimum spanning tree, and its cut at every level's distance and just below"""
    p, core, acc = mid
    got = core.linkage_tree(acc, metric=name)
    linkage_tree_ref.assert_equal(got, p.mst(metric), p.N)
    assert 1 <= got.rounds <= 12
    for l in range(1, p.K + 1):
        n, d = p.distance(metric, l)
        assert np.array_equal(got.cut(n, d), p.labels(l)) and got.clusters_at(n, d) == p.N >> l
        assert np.array_equal(got.cut(n * 1000 - 1, d * 1000), p.labels(l - 1)) and got.clusters_at(n * 1000 - 1, d * 1000) == p.N >> (l - 1)


def _clusters(core, acc, want, d=None, ratio=None):
    strain_clusters_ref.assert_equal(core.strain_clusters(acc, core_max_d=d, acc_ratio=ratio), want, core.size)


def test_clusters_at_4096(mid):
    """thresholds at each level's distance and just below it: the blocks of that level and of the one below, under the core
    criterion, the accessory criterion and both (the lower level decides)"""
    p, core, acc = mid
    for l in range(1, p.K + 1):
        (dn, _), (an, ad) = p.distance(planted.CORE, l), p.distance(planted.ACC, l)
        at, below = p.clusters(l), p.clusters(l - 1)
        _clusters(core, acc, at, d=dn)
        _clusters(core, acc, below, d=dn - 1)
        _clusters(core, acc, at, ratio=(an, ad))
        _clusters(core, acc, below, ratio=(an * 1000 - 1, ad * 1000))
        _clusters(core, acc, at, d=dn, ratio=(an, ad))
        _clusters(core, acc, below, d=dn - 1, ratio=(an, ad))
        _clusters(core, acc, below, d=dn, ratio=(an * 1000 - 1, ad * 1000))
    _clusters(core, acc, p.clusters(3), d=p.distance(planted.CORE, p.K)[0], ratio=p.distance(planted.ACC, 3))
    _clusters(core, acc, p.clusters(2), d=p.distance(planted.CORE, 2)[0], ratio=p.distance(planted.ACC, 9))


# ---- N = 16384, the cap: the core metric ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cap():
    """K = 14, c = 1: N = 16384, L = 16383, a 268 MB matrix; no accessory gene is looked at"""
    p = planted.Planted(14, c=1, core_genes=3, seed=16384)
    return p, p.core_matrix(), np.zeros((p.N, 8), np.uint8)


def test_upgma_at_the_cap(pa, cap):
    """one band of 16384 rows: four trips of upgma_store_core_kernel's row loop; 14 rounds, the first of 8192 pairs.  The 2 GB of
    sums hang off the core handle and go with it.  The cross products stay below 2^57 here, and no population of this shape
    passes 2^64 (test_the_128_bit_comparator's docstring): the comparator's high words are that test's."""
    p, core_matrix, acc_matrix = cap
    core, acc = _handles(pa, core_matrix, acc_matrix, 3)
    try:
        got = core.upgma_tree(acc, metric="core")
    finally:
        core.close()
        acc.close()
    want = p.upgma(planted.CORE)
    upgma_tree_ref.assert_equal(got, want, p.N)
    assert got.rounds == 14 and int(want["num"].max()) * (int(want["den"].max()) // p.L) < 2**57


def test_linkage_at_the_cap(pa, cap):
    """four trips of tree_store_core_kernel's row loop, components of up to 8192 rows"""
    p, core_matrix, acc_matrix = cap
    core, acc = _handles(pa, core_matrix, acc_matrix, 3)
    try:
        got = core.linkage_tree(acc, metric="core")
    finally:
        core.close()
        acc.close()
    linkage_tree_ref.assert_equal(got, p.mst(planted.CORE), p.N)
    assert 1 <= got.rounds <= 14


# ---- the 128-bit comparator ----------------------------------------------------------------------------------------------------

CLADE_SIZES, SHARED_GENES, PRIVATE_GENES = (63, 72, 78, 87), 67, (645, 524, 606, 612)
WORD = 2**64


def _clades():
    """300 rows in four clades of identical rows, shuffled, rows 0 .. 3 one of each so that clade g's id is g.  Every clade
    carries the 67 shared genes and its own private ones: between clades g and h every pair has a = p_g + p_h and
    b = 67 + a + core_genes with core_genes = 2^32 - 65536 - G, so b is just below 2^32.  -> (accessory matrix, core_genes)"""
    G = SHARED_GENES + sum(PRIVATE_GENES)
    genes = np.zeros((4, G), np.uint8)
    genes[:, :SHARED_GENES] = 1
    at = SHARED_GENES
    for g, n in enumerate(PRIVATE_GENES):
        genes[g, at:at + n] = 1
        at += n
    rest = np.random.default_rng(77).permutation(np.repeat(np.arange(4), np.array(CLADE_SIZES) - 1))
    return genes[np.concatenate([np.arange(4), rest])], 2**32 - 65536 - G


# num1 / den1 < num2 / den2 as three wrong comparators see it.  The first two are one function written twice: as a u64 multiply,
# and as the device body (__umul64hi and the low product) without its line on the high words.
MUTANTS = (("products cut to 64 bits", lambda n1, d1, n2, d2: (n1 * d2) % WORD < (n2 * d1) % WORD),
           ("low words only", lambda n1, d1, n2, d2: (n1 * d2) & (WORD - 1) < (n2 * d1) & (WORD - 1)),
           ("high words only", lambda n1, d1, n2, d2: (n1 * d2) >> 64 < (n2 * d1) >> 64))


def test_the_128_bit_comparator(pa):
    """N = 300, accessory metric, G = 2454, core_genes = 2^32 - 65536 - G.  The clades collapse at distance 0; what remains is
    decided between sums over 4536 .. 6786 pairs, and over more once two clades have merged: num 2^22 .. 2^24, den 2^44 .. 2^46,
    cross products 2^66 .. 2^70.  Before the device is called the sequential algorithm runs with the exact comparator, which
    counts what it is asked, and with each of three wrong ones: every wrong one must give another merge list, and the exact
    one must have decided comparisons whose high words differ while the low words say the opposite, and comparisons whose
    high words are equal and not 0.  Then the device equals the exact list, and so does the host form.
    The same construction on the core metric does not exist at this size.  Its den is |A| |B|, and two pairs of clusters of
    N rows hold at most N^4 / 64 pairs of pairs (|A|^2 |B| |C| with A = N / 2): below 2^27 at N = 300, so a product of 2^64
    needs a pair more than 2^37 sites apart, past the 2^32 sites of the contract.  At the cap, N^4 / 64 = 2^50 against
    d <= L < 2^14 in test_upgma_at_the_cap.  The comparator is one function for both metrics (ps_up_dist_cmp; the metric
    only picks where den is read), so this test is the cover of its high words under either."""
    acc_matrix, cg = _clades()
    N, G = acc_matrix.shape
    core_matrix = BASES[np.random.default_rng(78).integers(0, 4, (N, 64))]
    nums = planted.numerators(core_matrix, acc_matrix)
    seen = dict(beyond=0, low_words_disagree=0, equal_high_words=0)

    def exact(n1, d1, n2, d2):
        x, y = n1 * d2, n2 * d1
        if x >= WORD or y >= WORD:
            (xh, xl), (yh, yl) = divmod(x, WORD), divmod(y, WORD)          # (__umul64hi and the low product)
            seen["beyond"] += 1
            seen["low_words_disagree"] += xh != yh and (xh < yh) != (xl < yl)
            seen["equal_high_words"] += xh == yh and xl != yl
        return x < y

    want = upgma_tree_ref.tree(planted.ACC, *nums, N, 64, cg, less=exact)
    assert seen["beyond"] >= 100 and seen["low_words_disagree"] >= 10 and seen["equal_high_words"] >= 10, seen
    assert int(want["num"][-1]) * int(want["den"][-2]) >= WORD and want["distinct_heights"] == 4
    arrays = ("left", "right", "size", "num", "den")
    for what, less in MUTANTS:
        wrong = upgma_tree_ref.tree(planted.ACC, *nums, N, 64, cg, less=less)
        assert any(not np.array_equal(wrong[a], want[a]) for a in arrays), what
        assert not (np.array_equal(wrong["left"], want["left"]) and np.array_equal(wrong["right"], want["right"])), what
    core, acc = _handles(pa, core_matrix, acc_matrix, cg)
    try:
        got = core.upgma_tree(acc, metric="acc")
        host = pa.upgma_from_counts(*_device_numerators(core, acc), N, 64, cg, metric="acc")
    finally:
        core.close()
        acc.close()
    upgma_tree_ref.assert_equal(got, want, N)
    upgma_tree_ref.assert_equal(host, want, N)                 # (the host body of the comparator, on the device's own numerators)


# ---- the cfg2 population against the host forms ---------------------------------------------------------------------------

def _related(rng, N, L, G, founders=5, moves=3):
    """as related() of tests/test_gpu_isolate_samples.py, with genes: founders, then copies of earlier rows that move away by
    fewer than `moves` core sites and gene flips (one copy in nine by none: exact ties), shuffled"""
    core, acc = BASES[rng.integers(0, 4, (N, L))], (rng.random((N, G)) < 0.3).astype(np.uint8)
    for k in range(founders, N):
        src = rng.integers(k)
        core[k], acc[k] = core[src], acc[src]
        sites = rng.choice(L, rng.integers(0, moves), replace=False)
        core[k, sites] = BASES[(np.log2(core[k, sites]).astype(int) + 1 + rng.integers(0, 3, sites.size)) % 4]
        acc[k, rng.choice(G, rng.integers(0, moves), replace=False)] ^= 1
    order = rng.permutation(N)
    return np.ascontiguousarray(core[order]), np.ascontiguousarray(acc[order])


@pytest.fixture(scope="module")
def cfg2(pa):
    """N = 1000, L = 130, G = 40, core_genes 3: the handles and the numerators of all 499500 pairs from ps_pairwise_counts"""
    core, acc = _handles(pa, *_related(np.random.default_rng(1000), 1000, 130, 40), 3)
    yield core, acc, _device_numerators(core, acc)
    core.close()
    acc.close()


@pytest.mark.parametrize("name,metric", METRICS)
def test_cfg2_trees_against_the_host_forms(pa, cfg2, name, metric):
    """N = 1000, not lowered: on the MI355X machine's host ps_upgma_from_counts takes 0.011 s and ps_tree_from_counts 0.025 s per
    metric at this shape.  Both are held to the Python references at small sizes by the CPU suite; the numerators share
    nothing with the all-pairs kernels; ties and near-ties throughout"""
    core, acc, nums = cfg2
    h, i, u = nums[2:]
    assert int((h == 0).sum()) > 50 and int((u == i).sum()) > 50               # exact ties at distance 0 under both metrics
    got = core.upgma_tree(acc, metric=name)
    upgma_tree_ref.assert_equal(got, pa.upgma_from_counts(*nums, 1000, 130, 3, metric=name).as_dict(), 1000)
    assert got.rounds < 999 and got.distinct_heights > 100
    tree = core.linkage_tree(acc, metric=name)
    linkage_tree_ref.assert_equal(tree, pa.tree_from_counts(*nums, 1000, 130, 3, metric=name).as_dict(), 1000)
    assert tree.edges == 999 and tree.distinct_heights > 3


def test_cfg2_clusters_against_the_host_form(pa, cfg2):
    core, acc, nums = cfg2
    counts = set()
    for d, ratio in ((0, None), (1, None), (3, None), (None, (0, 1)), (None, (1, 20)), (None, (1, 8)), (2, (1, 10)), (40, (1, 30)), (1, (1, 2))):
        got = core.strain_clusters(acc, core_max_d=d, acc_ratio=ratio)
        strain_clusters_ref.assert_equal(got, pa.clusters_from_counts(*nums, 1000, 130, 3, core_max_d=d, acc_ratio=ratio).as_dict(), 1000)
        counts.add(got.clusters)
    assert len(counts) >= 5 and min(counts) < 100 and max(counts) > 500


# ---- bootstrap support past 300 ------------------------------------------------------------------------------------------------

def test_bootstrap_at_1030(pa):
    """the planted matrices of N = 1024 (c = 1, L = 1023) and six copies of existing leaves: N = 1030 = 4 x 256 + 6 = 16 x 64 + 6.
    Two replicates.  The caller's lists equal to the identity are the matrix again, so every merge comes back in both; the
    lists reversed are the same multiset of sites; the keyed draw is a function of its seed."""
    p = planted.Planted(10, c=1, core_genes=3, seed=1030)
    copies = [0, 77, 77, 500, 1000, 1023]
    m, a = p.core_matrix(), p.acc_matrix()
    m, a = np.concatenate([m, m[copies]]), np.concatenate([a, a[copies]])
    N, L = m.shape
    assert N == 1030 and L == 1023
    core, acc = _handles(pa, m, a, 3)
    identity = np.tile(np.arange(L), (2, 1))
    try:
        for method in bootstrap_ref.METHODS:
            own = bootstrap_ref.tree_merges(pa, core, acc, method)
            got = core.bootstrap_support(acc, method=method, replicates=2, sites=identity)
            assert np.array_equal(got.left, own[0]) and np.array_equal(got.right, own[1]) and got.merges == N - 1
            assert (got.support == 2).all() and (got.shared == N - 1).all() and got.support_sum == 2 * (N - 1), method
            back = core.bootstrap_support(acc, method=method, replicates=2, sites=np.ascontiguousarray(identity[:, ::-1]))
            assert np.array_equal(back.support, got.support) and np.array_equal(back.shared, got.shared), method
            once, twice = (core.bootstrap_support(acc, method=method, replicates=2, seed=1030) for _ in range(2))
            for name in ("left", "right", "support", "shared"):
                assert np.array_equal(getattr(once, name), getattr(twice, name)), (method, name)
            assert np.array_equal(once.left, own[0]) and once.support[-1] == 2 and once.draws == L
    finally:
        core.close()
        acc.close()
