"""The single-linkage tree on the device (ps_linkage_tree and its ps_sim / ps_multi forms, docs/LINKAGE_TREE.md) against the
plain-integer Kruskal (tests/linkage_tree_ref.py) over the numerators that the existing ps_pairwise_counts returns for the full
i < j list -- a path that shares nothing with the new code.  Every comparison is an equality of the four edge arrays and of
every integer field except `rounds`, of which only 1 <= rounds <= ceil(log2 N) is asserted."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import linkage_tree_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID = -1
BASES = np.array([1, 2, 4, 8], np.uint8)
METRICS = (("core", ref.CORE), ("acc", ref.ACC))


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
    """row k differs from the base row in sites 0..k - 1: d(i, j) = |i - j|; rows >= split differ in sites 300..319 as well:
    d = |i - j| + 20 across the split.  Rows shuffled by a fixed permutation."""
    m = np.full((N, L), 1, np.uint8)
    m[np.tril_indices(N, -1, L)] = 2
    if split is not None:
        m[split:, 300:] = 4
    return np.ascontiguousarray(m[np.random.default_rng(12).permutation(N)])


def _handles(pa, core_matrix, acc_matrix, cg, G=None):
    N, L = core_matrix.shape
    core = pa.Population(N, L, 4, True, 0.0, 0, 0)
    core.load_matrix(core_matrix)
    acc = pa.Population(N, acc_matrix.shape[1] if acc_matrix is not None else G, 2, False, 0.5, 0, cg)
    if acc_matrix is not None:
        acc.load_matrix(acc_matrix)
    return core, acc


def _numerators(core, acc):
    """(r1, r2, h, I, U) of every pair i < j from the existing sampled-pair path"""
    r1, r2 = ref.all_pairs(core.size)
    (h,) = core.pairwise_counts(r1, r2)
    if acc.ncols:
        i, u = acc.pairwise_counts(r1, r2)
    else:
        i = u = np.zeros(r1.size, np.uint32)
    return r1, r2, h, i, u


def _max_rounds(N):
    return max(1, int(N - 1).bit_length())              # ceil(log2 N)


def _assert_tree(got, nums, metric, N, L, cg):
    ref.assert_equal(got, ref.tree(metric, *nums, N, L, cg), N)
    ref.assert_spanning(got, N)
    assert got.pairs == N * (N - 1) // 2 and 1 <= got.rounds <= _max_rounds(N), got.rounds


def _check(core, acc, nums, cg):
    """both metrics on the device against Kruskal -> the two results"""
    out = []
    for name, metric in METRICS:
        got = core.linkage_tree(acc, metric=name)
        _assert_tree(got, nums, metric, core.size, core.global_cols, cg)
        out.append(got)
    return out


@pytest.mark.parametrize("N", [2, 63, 64, 65, 257])
def test_wave_and_chunk_edges(pa, N):
    """L = 130, G = 40, cg = 3, random: one edge only, a row of one wave trip less one / exactly / plus one, two 256-chunks"""
    rng = np.random.default_rng(N)
    core, acc = _handles(pa, _onehot(rng, N, 130), (rng.random((N, 40)) < 0.3).astype(np.uint8), 3)
    _check(core, acc, _numerators(core, acc), 3)
    core.close()
    acc.close()


@pytest.mark.parametrize("band", [0, 256])
def test_staircase_over_two_bands(pa, band):
    """N = 300 = 256 + 44, L = 320, G = 130; band 256: two bands, and row pairs on both sides of the band boundary.  Every tree
    edge at d = 1 with ties broken by output row; the split staircase has one edge at d = 21."""
    rng = np.random.default_rng(5)
    acc_m = (rng.random((300, 130)) < 0.3).astype(np.uint8)
    core, acc = _handles(pa, staircase(), acc_m, 7)
    core.set_tuning("core_davg_band", band)
    nums = _numerators(core, acc)
    one, by_acc = _check(core, acc, nums, 7)
    assert one.distinct_heights == 1 and list(one.num) == [1] * 299 and list(one.den) == [320] * 299 and one.rounds >= 2
    assert by_acc.distinct_heights > 1 and by_acc.undefined_edges == 0
    core.load_matrix(staircase(split=170))
    nums = _numerators(core, acc)
    two, _ = _check(core, acc, nums, 7)
    assert list(two.num) == [1] * 298 + [21] and two.distinct_heights == 2
    assert two.clusters_at(1, 320) == 2 and two.clusters_at(20, 320) == 2 and two.clusters_at(21, 320) == 1
    assert sorted(np.bincount(two.cut(1, 320))[np.unique(two.cut(1, 320))]) == [130, 170]
    core.close()
    acc.close()


def test_clonal_population_is_the_star_of_row_0(pa):
    """N = 100, every pair d = 0 and a = 0: the star of row 0, found in one round"""
    N = 100
    core, acc = _handles(pa, np.full((N, 200), 4, np.uint8), np.tile((np.arange(50) % 3 == 0).astype(np.uint8), (N, 1)), 2)
    for got in _check(core, acc, _numerators(core, acc), 2):
        assert list(got.lo) == [0] * (N - 1) and list(got.hi) == list(range(1, N)) and not got.num.any()
        assert got.rounds == 1 and got.distinct_heights == 1
    core.close()
    acc.close()


@pytest.fixture(scope="module")
def planted_lines(pa):
    core_m, acc_m = planted(21)
    core, acc = _handles(pa, core_m, acc_m, 5)
    yield core, acc, _numerators(core, acc)
    core.close()
    acc.close()


@pytest.mark.parametrize("name,metric", METRICS)
def test_cut_equals_the_strain_clusters_at_every_height(pa, planted_lines, name, metric):
    """N = 100, L = 300, G = 70, 6 founders: at every distinct merge height and just below it, the tree's cut is the labels of
    the existing ps_strain_clusters with that single criterion"""
    core, acc, nums = planted_lines
    tree = core.linkage_tree(acc, metric=name)
    _assert_tree(tree, nums, metric, 100, 300, 5)
    assert tree.distinct_heights >= 4
    heights = sorted({(int(n), int(d)) for n, d in zip(tree.num, tree.den)}, key=lambda t: t[0] / t[1])
    for n, d in heights:
        below = (n - 1, d) if metric == ref.CORE else (n * 1000 - 1, d * 1000)
        for tn, td in ((n, d), below):
            if tn < 0:
                continue
            crit = dict(core_max_d=tn) if metric == ref.CORE else dict(acc_ratio=(tn, td))
            want = core.strain_clusters(acc, **crit)
            assert np.array_equal(tree.cut(tn, td), want.labels), (tn, td)
            assert tree.clusters_at(tn, td) == want.clusters
    assert tree.clusters_at(*heights[-1]) == 1
    # the host restatement of the library agrees as well
    host = pa.tree_from_counts(*nums, 100, 300, 5, metric=name)
    for a in ("lo", "hi", "num", "den"):
        assert np.array_equal(getattr(host, a), getattr(tree, a))


def test_timing(pa, planted_lines):
    core, acc, _ = planted_lines
    for name, _ in METRICS:
        core.linkage_tree(acc, metric=name)
        counts_ms, store_ms, rounds_ms = core.linkage_tree_timing()
        assert counts_ms > 0.0 and store_ms > 0.0 and rounds_ms > 0.0


@pytest.mark.parametrize("cg", [0, 3])
def test_empty_accessory_rows(pa, cg):
    """N = 70, L = 130 (arbitrary bytes: the generic count form with odd h), G = 40, five all-zero accessory rows.  Without core
    genes the ten pairs among them are undefined (0 / 0), but each of them is at the defined distance 1 / 1 from every other
    row, and an undefined distance is above every defined one: the unique tree reaches them through defined edges and holds
    no undefined edge.  (One might expect undefined_edges == 4, a path through the five; under the order that is impossible while any row
    has a gene -- the count is 0, or N - 1 when no row has one, which test_no_accessory_genes covers.)  With core genes no
    pair is undefined at all."""
    rng = np.random.default_rng(3)
    N, L, G = 70, 130, 40
    A = (rng.random((N, G)) < 0.2).astype(np.uint8)
    empty = [3, 17, 18, 40, 69]
    A[empty] = 0
    assert A.any(1).sum() == N - 5
    core, acc = _handles(pa, rng.integers(0, 256, (N, L), dtype=np.uint8), A, cg)
    nums = _numerators(core, acc)
    assert (nums[2] & 1).any() and int((nums[4] == 0).sum()) == 10
    _, got = _check(core, acc, nums, cg)
    assert got.undefined_edges == 0 and got.den.all()
    if cg == 0:
        # every empty row is a leaf on an edge at 1 / 1, the largest defined distance
        touch = [k for k in range(N - 1) if got.lo[k] in empty or got.hi[k] in empty]
        assert len(touch) == 5 and all(got.num[k] == got.den[k] for k in touch)
    core.close()
    acc.close()


@pytest.mark.parametrize("cg", [3, 0])
def test_no_accessory_genes(pa, cg):
    """G = 0 under the accessory metric: every pair 0 / cg, or undefined without core genes; either way the star of row 0"""
    rng = np.random.default_rng(8)
    N, L = 130, 200
    core, acc = _handles(pa, _onehot(rng, N, L), None, cg, G=0)
    nums = _numerators(core, acc)
    _, got = _check(core, acc, nums, cg)
    assert list(got.lo) == [0] * (N - 1) and list(got.hi) == list(range(1, N)) and not got.num.any()
    assert list(got.den) == [cg] * (N - 1) and got.undefined_edges == (0 if cg else N - 1) and got.rounds == 1
    core.close()
    acc.close()


def test_limits(pa):
    rng = np.random.default_rng(6)
    core, acc = _handles(pa, _onehot(rng, 20, 64), (rng.random((20, 10)) < 0.5).astype(np.uint8), 2)
    wide = pa.Population(20, 65536, 2, False, 0.5, 0, 2)
    for name, _ in METRICS:
        with pytest.raises(pa.PansimError) as e:
            core.linkage_tree(wide, metric=name)
        assert e.value.code == PS_ERR_INVALID and "65535 accessory genes" in str(e.value)
    huge = pa.Population(20, 10, 2, False, 0.5, 0, 2**32 - 65535)
    with pytest.raises(pa.PansimError) as e:
        core.linkage_tree(huge, metric="acc")
    assert e.value.code == PS_ERR_INVALID and "core_genes + 65535 < 2^32" in str(e.value)
    for a, b in ((core, core), (acc, acc), (acc, core)):
        with pytest.raises(pa.PansimError) as e:
            a.linkage_tree(b)
        assert e.value.code == PS_ERR_INVALID and "core handle first" in str(e.value)
    with pytest.raises(ValueError):
        core.linkage_tree(acc, metric="joint")
    # a site shard on its own
    shard = pa.Population(20, 32, 4, True, 0.0, 0, 0, col_offset=32, global_cols=64)
    with pytest.raises(pa.PansimError) as e:
        shard.linkage_tree(acc)
    assert e.value.code == PS_ERR_INVALID and "ps_multi_linkage_tree" in str(e.value)
    for p in (core, acc, wide, huge, shard):
        p.close()


SIM = dict(pop_size=200, core_size=2048, pan_genes=300, core_genes=20, HR_rate=0.5, HGT_rate=0.5, seed=11, n_gen=9, max_distances=100)


@pytest.fixture(scope="module")
def sim_after_six(pa):
    """the unsharded run after 6 generations: its trees, Kruskal's over pairwise_counts on its handles (output rows), and its
    state after 3 more generations"""
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(6)
    got = [sim.linkage_tree(metric=name) for name, _ in METRICS]          # no sync: ordered behind the run
    nums = _numerators(sim.core_genome, sim.pan_genome)
    want = [ref.tree(metric, *nums, 200, 2048, 20) for _, metric in METRICS]
    sim.run(3)
    state = (sim.core_genome.read_matrix(), sim.pan_genome.read_matrix(), sim.last_parents())
    sim.close()
    return got, want, state


def test_row_order_in_a_simulation(pa, sim_after_six):
    got, want, state = sim_after_six
    for g, w in zip(got, want):
        ref.assert_equal(g, w, 200)
        ref.assert_spanning(g, 200)
        assert 1 <= g.rounds <= 8
    assert got[0].distinct_heights > 1
    # the call changes no state: the run that asked continues bit for bit with one that never did
    plain = pa.Simulation(pa.make_params(**SIM))
    plain.run(9)
    assert np.array_equal(plain.core_genome.read_matrix(), state[0]) and np.array_equal(plain.pan_genome.read_matrix(), state[1])
    assert np.array_equal(plain.last_parents(), state[2])
    plain.close()


@pytest.mark.parametrize("shards", [2, 3])
def test_multi_simulation_equals_the_unsharded_run(pa, sim_after_six, shards):
    _, want, _ = sim_after_six
    multi = pa.MultiSimulation(pa.make_params(**SIM), shards, devices=[0] * shards)
    multi.run(6)
    for (name, _), w in zip(METRICS, want):
        got = multi.linkage_tree(metric=name)
        ref.assert_equal(got, w, 200)
        assert 1 <= got.rounds <= 8
    with pytest.raises(pa.PansimError) as e:             # a site shard on its own
        multi.shards[1].linkage_tree()
    assert e.value.code == PS_ERR_INVALID and "ps_multi_linkage_tree" in str(e.value)
    multi.close()


CLI = dict(pop_size=100, core_size=300, pan_genes=600, core_genes=200, n_gen=4, seed=9, max_distances=500, HR_rate=0.5)
USUAL = (".tsv", "_freqs.txt", "_core_genome.csv", "_pangenome.csv", "_per_gen.tsv", "_selection.tsv")
SUMMARY = ("pop_size", "pairs", "core_sites", "core_genes", "metric", "edges", "undefined_edges", "distinct_heights")


@pytest.fixture(scope="module")
def cli_want(pa):
    """what the API gives for the command line's run, formatted as the two files, per metric"""
    sim = pa.Simulation(pa.make_params(**CLI))
    sim.run(4)
    out = {}
    for name, _ in METRICS:
        t = sim.linkage_tree(metric=name)
        assert t.edges == 99
        edges = "".join("%d\t%d\t%d\t%d\t%s\n" % (a, b, n, d, pa.fmt_f64(int(n) / int(d)) if d else "NaN")
                        for a, b, n, d in zip(t.lo, t.hi, t.num, t.den))
        out[name] = edges, "".join("%s\t%d\n" % (f, getattr(t, f)) for f in SUMMARY)
    sim.close()
    return out


def _cli(*args):
    r = subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("mode,metric", [("plain", "core"), ("plain", "acc"), ("gpus2", "core"), ("gpus2", "acc"), ("load_state", "core")])
def test_cli_print_tree(pa, cli_want, tmp_path, mode, metric):
    base = [x for k, v in CLI.items() for x in ("--" + k, v)] + ["--print_dist", "--print_matrices", "--print_selection"]
    flags = ["--print_tree"] + (["--tree_metric", metric] if metric != "core" else [])
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
    assert set(os.listdir(tmp_path)) == {"no" + s for s in USUAL} | {"yes" + s for s in USUAL + ("_tree.tsv", "_tree_summary.tsv")} | extra
    assert (tmp_path / "yes_tree.tsv").read_text() == cli_want[metric][0]
    assert (tmp_path / "yes_tree_summary.tsv").read_text() == cli_want[metric][1]
