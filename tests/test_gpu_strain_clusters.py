"""Strain clusters on the device (ps_strain_clusters and its ps_sim / ps_multi forms, docs/STRAIN_CLUSTERS.md) against the
plain-integer union-find (tests/strain_clusters_ref.py) over the numerators that the existing ps_pairwise_counts returns for
the full i < j list -- a path that shares nothing with the new code.  Every comparison is an equality of `labels` and of
every integer field except `rounds`."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import strain_clusters_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_STATE = -1, -6
BASES = np.array([1, 2, 4, 8], np.uint8)


def _onehot(rng, N, L):
    return BASES[rng.integers(0, 4, (N, L))]


def planted(seed, N=100, L=300, G=70, founders=6):
    """`founders` unrelated individuals; every other one copies an earlier member of a founder's line and moves away by up to 3
    core sites and up to 3 gene flips: within a line neighbours are close, the lines are far apart"""
    rng = np.random.default_rng(seed)
    core, acc = _onehot(rng, N, L), (rng.random((N, G)) < 0.4).astype(np.uint8)
    line = [[f] for f in range(founders)]
    for k in range(founders, N):
        members = line[rng.integers(founders)]
        src = members[rng.integers(len(members))]
        core[k], acc[k] = core[src], acc[src]
        sites = rng.choice(L, rng.integers(0, 4), replace=False)
        core[k, sites] = BASES[(np.log2(core[k, sites]).astype(int) + 1 + rng.integers(0, 3, sites.size)) % 4]
        acc[k, rng.choice(G, rng.integers(0, 4), replace=False)] ^= 1
        members.append(k)
    return core, acc


def staircase(N=300, L=320, split=None):
    """row k differs from the base row in sites 0..k - 1: d(i, j) = |i - j|, a path under threshold 1; rows >= split differ in
    sites 300..319 as well: the path is cut there.  Rows shuffled by a fixed permutation."""
    m = np.full((N, L), 1, np.uint8)
    m[np.tril_indices(N, -1, L)] = 2
    if split is not None:
        m[split:, 300:] = 4
    return np.ascontiguousarray(m[np.random.default_rng(12).permutation(N)])


def _handles(pa, core_matrix, acc_matrix, cg):
    N, L = core_matrix.shape
    core = pa.Population(N, L, 4, True, 0.0, 0, 0)
    core.load_matrix(core_matrix)
    acc = pa.Population(N, acc_matrix.shape[1], 2, False, 0.5, 0, cg)
    acc.load_matrix(acc_matrix)
    return core, acc


def _numerators(core, acc):
    """(r1, r2, h, I, U) of every pair i < j from the existing sampled-pair path"""
    r1, r2 = ref.all_pairs(core.size)
    (h,) = core.pairwise_counts(r1, r2)
    i, u = acc.pairwise_counts(r1, r2)
    return r1, r2, h, i, u


def _check(core, acc, nums, cg, thresholds):
    """the device call at integer thresholds (core_max_d, acc_num, acc_den) against the union-find -> the result"""
    d, num, den = thresholds
    got = core.strain_clusters(acc, core_max_d=None if d == ref.NO_CORE else d, acc_ratio=(num, den) if den else None)
    ref.assert_equal(got, ref.clusters(*nums, core.size, core.global_cols, cg, d, num, den), core.size)
    assert got.pairs == core.size * (core.size - 1) // 2 and got.rounds >= 1
    return got


def test_one_chunk_one_band(pa):
    """N = 100, L = 300, G = 70, cg = 5: planted clusters under the core, the accessory and the joint criterion"""
    core_m, acc_m = planted(21)
    core, acc = _handles(pa, core_m, acc_m, 5)
    with pytest.raises(pa.PansimError) as e:
        core.strain_clusters_timing()                    # nothing to report yet
    assert e.value.code == PS_ERR_STATE
    nums = _numerators(core, acc)
    L = 300
    for core_max, acc_max in ((0.02, None), (None, 0.2), (0.02, 0.2), (0.01, 0.1)):
        got = _check(core, acc, nums, 5, ref.thresholds(L, core_max, acc_max))
        assert 1 < got.clusters < 100 and got.undefined_pairs == 0
        # the real-valued thresholds of the wrapper are the same call
        assert np.array_equal(core.strain_clusters(acc, core_max=core_max, acc_max=acc_max).labels, got.labels)
        counts_ms, edges_ms, labels_ms = core.strain_clusters_timing()
        assert counts_ms > 0.0 and edges_ms > 0.0 and labels_ms > 0.0
    # the host restatement of the library agrees as well
    host = pa.clusters_from_counts(*nums, 100, L, 5, core_max=0.02, acc_max=0.2)
    assert np.array_equal(host.labels, core.strain_clusters(acc, core_max=0.02, acc_max=0.2).labels)
    core.close()
    acc.close()


@pytest.mark.parametrize("band", [0, 256])
def test_chain_the_worst_case_for_propagation(pa, band):
    """N = 300 = 256 + 44 = 4 * 64 + 44, L = 320, G = 130: a shuffled path; band 256: two bands (256 + 44 rows)"""
    rng = np.random.default_rng(5)
    acc_m = (rng.random((300, 130)) < 0.3).astype(np.uint8)
    core, acc = _handles(pa, staircase(), acc_m, 7)
    core.set_tuning("core_davg_band", band)
    nums = _numerators(core, acc)
    one = _check(core, acc, nums, 7, (1, 0, 0))
    assert one.clusters == 1 and one.edges == 299 and one.rounds >= 2 and not one.labels.any()
    none = _check(core, acc, nums, 7, (0, 0, 0))
    assert none.clusters == none.singletons == 300 and none.edges == 0 and np.array_equal(none.labels, np.arange(300))
    # an accessory criterion that every pair meets changes nothing; one that some pairs miss cuts the path
    ref.assert_equal(_check(core, acc, nums, 7, (1, 1, 1)), ref.clusters(*nums, 300, 320, 7, 1, 0, 0), 300)
    cut = _check(core, acc, nums, 7, (1, 3, 4))
    assert 1 < cut.clusters < 300
    assert 1 < _check(core, acc, nums, 7, (ref.NO_CORE, 13, 20)).clusters < 300
    core.load_matrix(staircase(split=170))
    nums = _numerators(core, acc)
    two = _check(core, acc, nums, 7, (1, 0, 0))
    assert two.clusters == 2 and two.edges == 298 and sorted(two.sizes()) == [130, 170] and two.within_pairs == 170 * 169 // 2 + 130 * 129 // 2
    core.close()
    acc.close()


@pytest.mark.parametrize("N", [2, 63, 64, 65, 257])
def test_word_and_chunk_edges(pa, N):
    """L = 130, random one-hot, the thresholds those of the median pair: equality on the device"""
    rng = np.random.default_rng(N)
    core, acc = _handles(pa, _onehot(rng, N, 130), (rng.random((N, 40)) < 0.3).astype(np.uint8), 3)
    nums = _numerators(core, acc)
    _, _, h, i, u = nums
    d_med = int(np.sort(h // 2)[h.size // 2])
    m = np.argsort((u - i) / (u + 3.0), kind="stable")[h.size // 2]
    a_med, b_med = int(u[m] - i[m]), int(u[m] + 3)
    got = _check(core, acc, nums, 3, (d_med, 0, 0))
    assert got.edges >= (h.size + 1) // 2 and _check(core, acc, nums, 3, (d_med - 1, 0, 0)).edges < got.edges
    got = _check(core, acc, nums, 3, (ref.NO_CORE, a_med, b_med))
    assert got.edges >= (h.size + 1) // 2
    _check(core, acc, nums, 3, (d_med, a_med, b_med))
    core.close()
    acc.close()


def test_arbitrary_bytes_and_undefined_pairs(pa):
    """N = 70, L = 130: the generic count form with odd h; empty accessory rows and no core genes: undefined pairs"""
    rng = np.random.default_rng(3)
    N, L, G = 70, 130, 40
    A = (rng.random((N, G)) < 0.2).astype(np.uint8)
    empty = [3, 17, 18, 40, 69]
    A[empty] = 0
    core, acc = _handles(pa, rng.integers(0, 256, (N, L), dtype=np.uint8), A, 0)
    nums = _numerators(core, acc)
    _, _, h, i, u = nums
    assert (h & 1).any()
    d_med = int(np.sort(h // 2)[h.size // 2])
    for thresholds in ((ref.NO_CORE, 1, 1), (ref.NO_CORE, 3, 4), (d_med, 3, 4)):
        got = _check(core, acc, nums, 0, thresholds)
        assert got.undefined_pairs == int((u == 0).sum()) == 10
        # an empty individual is at distance 1 from every other and undefined against its like: on its own below 1 / 1,
        # joined through the others -- never through its like -- at 1 / 1
        assert got.clusters == 1 if thresholds == (ref.NO_CORE, 1, 1) else np.array_equal(got.labels[empty], empty)
    # ... and under the core criterion alone the same individuals are joined like any other
    got = _check(core, acc, nums, 0, (int((h // 2).max()), 0, 0))
    assert got.clusters == 1 and got.undefined_pairs == 0
    core.close()
    acc.close()


def test_handle_checks(pa):
    rng = np.random.default_rng(6)
    core, acc = _handles(pa, _onehot(rng, 20, 64), (rng.random((20, 10)) < 0.5).astype(np.uint8), 2)
    for a, b in ((core, core), (acc, acc), (acc, core)):
        with pytest.raises(pa.PansimError) as e:
            a.strain_clusters(b, core_max=0.1)
        assert e.value.code == PS_ERR_INVALID and "core handle first" in str(e.value)
    other = pa.Population(21, 10, 2, False, 0.5, 0, 2)
    with pytest.raises(pa.PansimError) as e:
        core.strain_clusters(other, core_max=0.1)
    assert e.value.code == PS_ERR_INVALID and "20 individuals" in str(e.value)
    for kw, text in ((dict(), "at least one criterion"), (dict(acc_ratio=(3, 2)), "acc_num <= acc_den"), (dict(acc_ratio=(1, 2**24 + 1)), "2^24")):
        with pytest.raises(pa.PansimError) as e:
            core.strain_clusters(acc, **kw)
        assert e.value.code == PS_ERR_INVALID and text in str(e.value)
    lone_c, lone_a = pa.Population(1, 64, 4, True, 0.0, 0, 0), pa.Population(1, 10, 2, False, 0.5, 0, 2)
    with pytest.raises(pa.PansimError) as e:
        lone_c.strain_clusters(lone_a, core_max=0.1)
    assert e.value.code == PS_ERR_INVALID and "pop_size >= 2" in str(e.value)
    # a site shard on its own
    shard = pa.Population(20, 32, 4, True, 0.0, 0, 0, col_offset=32, global_cols=64)
    with pytest.raises(pa.PansimError) as e:
        shard.strain_clusters(acc, core_max=0.1)
    assert e.value.code == PS_ERR_INVALID and "ps_multi_strain_clusters" in str(e.value)
    for p in (core, acc, other, lone_c, lone_a, shard):
        p.close()


SIM = dict(pop_size=200, core_size=2000, pan_genes=300, core_genes=20, HR_rate=0.5, HGT_rate=0.5, seed=11, n_gen=8, max_distances=100)
SIM_THRESHOLDS = ((0.2, None), (None, 0.47), (0.27, 0.52))


def host_numerators(core_m, acc_m):
    """(r1, r2, h, I, U) of every pair i < j of two matrices as read_matrix returns them (output order), in numpy"""
    r1, r2 = ref.all_pairs(core_m.shape[0])
    bits = np.array([bin(x).count("1") for x in range(256)], np.uint32)
    h = np.concatenate([bits[core_m[k] ^ core_m[k + 1:]].sum(1, dtype=np.uint32) for k in range(core_m.shape[0] - 1)])
    a = acc_m.astype(np.uint32)
    inter = (a @ a.T)[r1, r2]
    return r1, r2, h, inter.astype(np.uint32), (a.sum(1)[r1] + a.sum(1)[r2] - inter).astype(np.uint32)


@pytest.fixture(scope="module")
def sim_after_five(pa):
    """the unsharded run after 5 generations: its clusters and the union-find's over the matrices it reads back"""
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(5)
    got = [sim.strain_clusters(core_max=c, acc_max=a) for c, a in SIM_THRESHOLDS]          # no sync: ordered behind the run
    nums = host_numerators(sim.core_genome.read_matrix(), sim.pan_genome.read_matrix())
    want = [ref.clusters(*nums, 200, 2000, 20, *ref.thresholds(2000, c, a)) for c, a in SIM_THRESHOLDS]
    sim.run(3)
    state = (sim.core_genome.read_matrix(), sim.pan_genome.read_matrix(), sim.last_parents())
    sim.close()
    return got, want, state


def test_row_order_in_a_simulation(pa, sim_after_five):
    got, want, state = sim_after_five
    for g, w in zip(got, want):
        ref.assert_equal(g, w, 200)
    assert all(1 < g.clusters < 200 for g in got)
    # the call changes no state: the run that asked continues bit for bit with one that never did
    plain = pa.Simulation(pa.make_params(**SIM))
    plain.run(8)
    assert np.array_equal(plain.core_genome.read_matrix(), state[0]) and np.array_equal(plain.pan_genome.read_matrix(), state[1])
    assert np.array_equal(plain.last_parents(), state[2])
    plain.close()


def test_multi_simulation_equals_the_unsharded_run(pa, sim_after_five):
    _, want, _ = sim_after_five
    multi = pa.MultiSimulation(pa.make_params(**SIM), 2, devices=[0, 0])
    multi.run(5)
    for (c, a), w in zip(SIM_THRESHOLDS, want):
        ref.assert_equal(multi.strain_clusters(core_max=c, acc_max=a), w, 200)
    with pytest.raises(pa.PansimError) as e:             # a site shard on its own
        multi.shards[1].strain_clusters(core_max=0.2)
    assert e.value.code == PS_ERR_INVALID and "ps_multi_strain_clusters" in str(e.value)
    multi.close()


def test_multi_simulation_over_two_bands(pa):
    """N = 300 in two site shards with core_davg_band = 256 on shard 0: two bands (256 + 44 rows), each one the sum of both
    shards' counts.  Against the unsharded run (one band) and the union-find over the matrices it reads back; the core
    threshold is the lowest tenth of the host's own distances, so some pairs are edges and some are not."""
    kw = dict(SIM, pop_size=300, seed=12)
    sim = pa.Simulation(pa.make_params(**kw))
    sim.run(4)
    nums = host_numerators(sim.core_genome.read_matrix(), sim.pan_genome.read_matrix())
    d = np.sort(nums[2] // 2)
    core_max_d = int(d[d.size // 10])
    multi = pa.MultiSimulation(pa.make_params(**kw), 2, devices=[0, 0])
    multi.shards[0].core_genome.set_tuning("core_davg_band", 256)
    multi.run(4)
    for acc_max in (None, 0.5):
        crit = dict(core_max_d=core_max_d, acc_max=acc_max)
        got = multi.strain_clusters(**crit)
        _, num, den = ref.thresholds(2000, None, acc_max)
        ref.assert_equal(got, ref.clusters(*nums, 300, 2000, 20, core_max_d, num, den), 300)
        one = sim.strain_clusters(**crit)
        assert np.array_equal(got.labels, one.labels) and got.edges == one.edges
        if acc_max is None:
            assert 0 < got.edges < got.pairs == 300 * 299 // 2
    sim.close()
    multi.close()


CLI = dict(pop_size=100,core_size=300, pan_genes=600, core_genes=200, n_gen=4, seed=9, max_distances=500, HR_rate=0.5)
CLI_CORE_MAX, CLI_ACC_MAX = 0.2, 0.4
USUAL = (".tsv", "_freqs.txt", "_core_genome.csv", "_pangenome.csv", "_per_gen.tsv", "_selection.tsv")


@pytest.fixture(scope="module")
def cli_want(pa):
    """what the API gives for the command line's run, formatted as the two files"""
    sim = pa.Simulation(pa.make_params(**CLI))
    sim.run(4)
    c = sim.strain_clusters(core_max=CLI_CORE_MAX, acc_max=CLI_ACC_MAX)
    sim.close()
    assert 1 < c.clusters < 100
    names = ("pop_size", "pairs", "core_sites", "core_genes", "edges", "clusters", "singletons", "largest_cluster", "within_pairs",
             "undefined_pairs")
    d, num, den = ref.thresholds(300, CLI_CORE_MAX, CLI_ACC_MAX)
    summary = "".join("%s\t%d\n" % (n, getattr(c, n)) for n in names) + "core_max_d\t%d\nacc_num\t%d\nacc_den\t%d\n" % (d, num, den)
    return "".join("%d\t%d\n" % (k, x) for k, x in enumerate(c.labels)), summary


def _cli(*args):
    r = subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("mode", ["plain", "gpus2", "load_state"])
def test_cli_print_clusters(pa, cli_want, tmp_path, mode):
    base = [x for k, v in CLI.items() for x in ("--" + k, v)] + ["--print_dist", "--print_matrices", "--print_selection"]
    flags = ["--print_clusters", "--cluster_core_max", CLI_CORE_MAX, "--cluster_acc_max", CLI_ACC_MAX]
    if mode == "gpus2":
        base += ["--gpus", 2]
    if mode == "load_state":
        state = tmp_path / "half.state"
        _cli(*base[:8], "--n_gen", 2, *base[10:], "--outpref", tmp_path / "half", "--save_state", state)
        for f in os.listdir(tmp_path):
            if f.startswith("half_") or f == "half.tsv":
                os.remove(tmp_path / f)
        base += ["--load_state", state]
    _cli(*base, "--outpref", tmp_path / "no")
    _cli(*base, *flags, "--outpref", tmp_path / "yes")
    for suffix in USUAL:
        assert filecmp.cmp(str(tmp_path / "no") + suffix, str(tmp_path / "yes") + suffix, shallow=False), suffix
    extra = {"half.state"} if mode == "load_state" else set()
    assert set(os.listdir(tmp_path)) == {"no" + s for s in USUAL} | {"yes" + s for s in USUAL + ("_clusters.tsv", "_clusters_summary.tsv")} | extra
    assert (tmp_path / "yes_clusters.tsv").read_text() == cli_want[0]
    assert (tmp_path / "yes_clusters_summary.tsv").read_text() == cli_want[1]
