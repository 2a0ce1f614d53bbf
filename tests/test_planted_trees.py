"""The closed forms of tests/planted_trees.py against the plain-Python references of the three read-outs, without a device: the
numerators come from the planted matrices by NumPy, the references -- the sequential UPGMA algorithm, Kruskal, the union-find --
run on them, and every field of the closed form equals theirs.  This is what lets the closed forms judge the device at
N = 4096 and 16384 (tests/test_gpu_tree_sizes.py), where no reference can run.  At N = 1024 the library's host forms, which the
CPU suite holds to the same references at small sizes, take the references' place."""
import numpy as np
import pytest

import linkage_tree_ref
import planted_trees as planted
import strain_clusters_ref
import upgma_tree_ref

METRICS = (("core", planted.CORE), ("acc", planted.ACC))


def _equal(got, want, fields):
    for name in fields:
        assert got[name] == want[name], (name, got[name], want[name])
    for name, a in want.items():
        if isinstance(a, np.ndarray):
            assert got[name].dtype == a.dtype and np.array_equal(got[name], a), (name, got[name], a)


def _cuts(p, metric, l):
    """the integer thresholds (core_max_d, acc_num, acc_den) at the distance of level l, and just below that of level l + 1"""
    out = []
    for level, below in ((l, 0), (l + 1, 1)):
        if level < 1 or level > p.K:
            continue
        n, d = p.distance(metric, level)
        out.append((n - below, 0, 0) if metric == planted.CORE else (strain_clusters_ref.NO_CORE, n * 1000 - below, d * 1000))
    return out


@pytest.fixture(scope="module", params=[(3, 2), (6, 1), (7, 2)], ids=["N8", "N64", "N128"])
def population(request):
    K, c = request.param
    p = planted.Planted(K, c=c, core_genes=3, seed=40 + K)
    core, acc = p.core_matrix(), p.acc_matrix()
    assert core.shape == (p.N, p.L) and acc.shape == (p.N, p.G) and (acc.sum(1) == K).all()
    return p, planted.numerators(core, acc)


def test_the_numerators_are_those_of_the_levels(population):
    """d = c (2 l - 1), I = K - l and U = K + l for a pair of level l, and the rows are shuffled"""
    p, (r1, r2, h, i, u) = population
    l = p.level(r1, r2)
    assert l.min() == 1 and l.max() == p.K and not np.array_equal(p.leaf, np.arange(p.N))
    assert np.array_equal(h, 2 * p.c * (2 * l - 1)) and np.array_equal(i, p.K - l) and np.array_equal(u, p.K + l)


@pytest.mark.parametrize("name,metric", METRICS)
def test_upgma_closed_form(population, name, metric):
    p, nums = population
    want = upgma_tree_ref.tree(metric, *nums, p.N, p.L, 3)
    got = p.upgma(metric)
    _equal(got, want, upgma_tree_ref.INT_FIELDS)
    by_rounds, taken = upgma_tree_ref.tree_by_rounds(metric, *nums, p.N, p.L, 3)
    assert taken == got["rounds"] == p.K
    _equal(got, by_rounds, upgma_tree_ref.INT_FIELDS)


@pytest.mark.parametrize("name,metric", METRICS)
def test_mst_closed_form(population, name, metric):
    p, nums = population
    _equal(p.mst(metric), linkage_tree_ref.tree(metric, *nums, p.N, p.L, 3), linkage_tree_ref.INT_FIELDS)


@pytest.mark.parametrize("name,metric", METRICS)
def test_clusters_closed_form(population, name, metric):
    """at each level's distance and just below the next level's, under one criterion and under both"""
    p, nums = population
    for l in range(p.K + 1):
        want = p.clusters(l)
        for d, num, den in _cuts(p, metric, l):
            _equal(want, strain_clusters_ref.clusters(*nums, p.N, p.L, 3, d, num, den), strain_clusters_ref.INT_FIELDS)
    # both criteria: the smaller level decides
    for lc, la in ((2, 1), (1, 3), (p.K, p.K - 1), (0, 2)):
        d = _cuts(p, planted.CORE, lc)[0][0] if lc else 0
        _, num, den = _cuts(p, planted.ACC, la)[0]
        _equal(p.clusters(min(lc, la)), strain_clusters_ref.clusters(*nums, p.N, p.L, 3, d, num, den), strain_clusters_ref.INT_FIELDS)


@pytest.mark.parametrize("name,metric", METRICS)
def test_closed_forms_against_the_host_forms_at_1024(pa, name, metric):
    """N = 1024, c = 1: beyond the references' reach, within that of ps_upgma_from_counts, ps_tree_from_counts and
    ps_clusters_from_counts"""
    p = planted.Planted(10, c=1, core_genes=3, seed=50)
    nums = planted.numerators(p.core_matrix(), p.acc_matrix())
    upgma_tree_ref.assert_equal(pa.upgma_from_counts(*nums, p.N, p.L, 3, metric=name), p.upgma(metric), p.N)
    linkage_tree_ref.assert_equal(pa.tree_from_counts(*nums, p.N, p.L, 3, metric=name), p.mst(metric), p.N)
    for l in (0, 1, 5, 9, 10):
        for d, num, den in _cuts(p, metric, l):
            got = pa.clusters_from_counts(*nums, p.N, p.L, 3, core_max_d=None if d == strain_clusters_ref.NO_CORE else d,
                                          acc_ratio=(num, den) if den else None)
            strain_clusters_ref.assert_equal(got, p.clusters(l), p.N)
