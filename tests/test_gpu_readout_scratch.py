"""The scratch and the timings that the device read-outs keep on the core handle (pair_histogram.h .. clock_histogram.h), in the
two orders of calls that no other file exercises: a scratch buffer that grows between calls and is reused by a smaller call, and
the histogram's summary words borrowed by the clock histogram before the histogram itself has ever run.  Every comparison is an
equality against the same call on handles that have computed nothing before."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PS_ERR_STATE = -6
BASES = np.array([1, 2, 4, 8], np.uint8)
N, L, G, CG = 70, 96, 40, 3


def _handles(pa, core_matrix, acc_matrix, cg):
    n, sites = core_matrix.shape
    core = pa.Population(n, sites, 4, True, 0.0, 0, 0)
    core.load_matrix(core_matrix)
    acc = pa.Population(n, acc_matrix.shape[1], 2, False, 0.5, 0, cg)
    acc.load_matrix(acc_matrix)
    return core, acc


def _assert_same(got, want):
    """field for field and array for array"""
    got, want = got.as_dict(), want.as_dict()
    assert got.keys() == want.keys()
    for name in want:
        if isinstance(want[name], np.ndarray):
            assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
            assert np.array_equal(got[name], want[name], equal_nan=want[name].dtype.kind == "f"), name
        else:
            assert got[name] == want[name], name


def _assert_timing(values, n):
    assert len(values) == n and all(v >= 0.0 for v in values), values


def test_scratch_grows_and_is_reused_by_a_smaller_call(pa):
    """N = 70, L = 96, G = 40, cg = 3, random.  The tree: the accessory metric (u16 matrix), the core metric (u32: the buffer
    grows), the accessory metric again (the larger buffer reused).  The neighbours on the accessory metric: k = 1, k = 8 (three
    lists of N k: grows), k = 1 again.  Every result against the same call on a fresh pair of handles."""
    rng = np.random.default_rng(70)
    core_m, acc_m = BASES[rng.integers(0, 4, (N, L))], (rng.random((N, G)) < 0.4).astype(np.uint8)
    core, acc = _handles(pa, core_m, acc_m, CG)

    def fresh(call):
        c, a = _handles(pa, core_m, acc_m, CG)
        out = call(c, a)
        c.close()
        a.close()
        return out

    for metric in ("acc", "core", "acc"):
        got = core.linkage_tree(acc, metric=metric)
        _assert_timing(core.linkage_tree_timing(), 3)
        _assert_same(got, fresh(lambda c, a: c.linkage_tree(a, metric=metric)))
        assert got.edges == N - 1
    for k in (1, 8, 1):
        got = core.nearest_neighbours(acc, k, metric="acc")
        _assert_timing(core.nearest_neighbours_timing(), 2)
        _assert_same(got, fresh(lambda c, a: c.nearest_neighbours(a, k, metric="acc")))
        assert got.nbr.shape == (N, k)
    core.close()
    acc.close()


def _same_clock(a, b):
    assert all(getattr(a, name) == getattr(b, name) for name in a.FIELDS), [(name, getattr(a, name), getattr(b, name)) for name in a.FIELDS]
    assert np.array_equal(a.joint, b.joint) and np.array_equal(a.per_time, b.per_time)


def test_clock_histogram_borrows_the_histogram_words(pa):
    """Two runs of the same seed, pop_size 70, 48 core sites, 40 genes, five recorded generations.  The first: the clock histogram
    with the automatic core span (its moments pass writes the histogram's summary words), then the 16 x 16 distance histogram;
    the second: the two calls the other way round.  Equal results, and the histogram's timing is the histogram's own: none after
    the clock histogram alone."""
    prm = dict(pop_size=70, core_size=48, pan_genes=40, core_genes=4, HR_rate=0.5, HGT_rate=0.5, max_distances=50, n_gen=5, seed=11)
    sims = [pa.Simulation(pa.make_params(**prm)) for _ in range(2)]
    for sim in sims:
        sim.record_ancestry(5)
        sim.run(5)
    first, second = sims
    clock_1 = first.clock_histogram(metric="core", time_bins=8, dist_bins=16)
    _assert_timing(first.clock_histogram_timing(), 2)
    with pytest.raises(pa.PansimError) as e:
        first.core_genome.distance_histogram_timing()
    assert e.value.code == PS_ERR_STATE and "no distance histogram" in str(e.value)
    hist_1 = first.distance_histogram(16, 16)
    _assert_timing(first.core_genome.distance_histogram_timing(), 2)
    hist_2 = second.distance_histogram(16, 16)
    _assert_timing(second.core_genome.distance_histogram_timing(), 2)
    clock_2 = second.clock_histogram(metric="core", time_bins=8, dist_bins=16)
    _assert_timing(second.clock_histogram_timing(), 2)
    _same_clock(clock_1, clock_2)
    _assert_same(hist_1, hist_2)
    assert clock_1.core_span == hist_1.core_d_max + 1 == hist_1.core_span and hist_1.pairs == 70 * 69 // 2
    for sim in sims:
        sim.close()
