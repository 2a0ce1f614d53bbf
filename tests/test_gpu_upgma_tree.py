"""The average-linkage (UPGMA) tree on the device (ps_upgma_tree and its ps_sim / ps_multi forms, docs/UPGMA_TREE.md) against
the plain-integer sequential algorithm (tests/upgma_tree_ref.py) over the numerators that the existing ps_pairwise_counts
returns for the full i < j list -- a path that shares nothing with the new code.  Every comparison is an equality of the five
merge arrays and of every integer field except `rounds`, which is asserted where the construction fixes it."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import upgma_tree_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID = -1
BASES = np.array([1, 2, 4, 8], np.uint8)
METRICS = (("core", ref.CORE), ("acc", ref.ACC))


def _onehot(rng, N, L):
    return BASES[rng.integers(0, 4, (N, L))]


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


def _check(core, acc, nums, cg, want=None):
    """both metrics on the device against the sequential algorithm (`want`: its two results, computed before) -> the two results"""
    out = []
    N, L = core.size, core.global_cols
    for k, (name, metric) in enumerate(METRICS):
        got = core.upgma_tree(acc, metric=name)
        ref.assert_equal(got, want[k] if want else ref.tree(metric, *nums, N, L, cg), N)
        ref.assert_monotone(got)
        assert got.pairs == N * (N - 1) // 2 and 1 <= got.rounds <= N - 1, got.rounds
        out.append(got)
    return out


@pytest.mark.parametrize("N", [2, 3, 63, 64, 65, 257])
def test_wave_and_chunk_edges(pa, N):
    """L = 130, G = 40, cg = 3, random: one merge only, a row of one wave trip less one / exactly / plus one, two 256-chunks"""
    rng = np.random.default_rng(N)
    core, acc = _handles(pa, _onehot(rng, N, 130), (rng.random((N, 40)) < 0.3).astype(np.uint8), 3)
    _check(core, acc, _numerators(core, acc), 3)
    core.close()
    acc.close()


@pytest.fixture(scope="module")
def two_bands(pa):
    """N = 300 = 256 + 44, L = 320, G = 130: the matrices and, computed once, the sequential algorithm's two trees"""
    rng = np.random.default_rng(5)
    core_m, acc_m = _onehot(rng, 300, 320), (rng.random((300, 130)) < 0.3).astype(np.uint8)
    # a few close relatives, so that mutual pairs lie on both sides of row 256 and across it
    for a, b in ((3, 290), (255, 256), (10, 11), (270, 299), (100, 257)):
        core_m[b], acc_m[b] = core_m[a], acc_m[a]
        core_m[b, :3] = BASES[(np.log2(core_m[b, :3]).astype(int) + 1) % 4]
        acc_m[b, :2] ^= 1
    core, acc = _handles(pa, core_m, acc_m, 7)
    nums = _numerators(core, acc)
    want = [ref.tree(metric, *nums, 300, 320, 7) for _, metric in METRICS]
    yield core, acc, nums, want
    core.close()
    acc.close()


@pytest.mark.parametrize("band", [0, 256])
def test_two_bands(pa, two_bands, band):
    """band 256: two bands; the planted relatives are the first merges, on both sides of the band boundary and across it"""
    core, acc, nums, want = two_bands
    core.set_tuning("core_davg_band", band)
    by_core, _ = _check(core, acc, nums, 7, want)
    first = {(int(a), int(b)) for a, b in zip(by_core.left[:5], by_core.right[:5])}
    assert first == {(3, 290), (255, 256), (10, 11), (270, 299), (100, 257)} and by_core.rounds < 299
    core.set_tuning("core_davg_band", 0)


def test_arbitrary_bytes(pa):
    """N = 70, L = 130 of arbitrary bytes: the generic count form, with odd h that the store halves downwards"""
    rng = np.random.default_rng(3)
    core, acc = _handles(pa, rng.integers(0, 256, (70, 130), dtype=np.uint8), (rng.random((70, 40)) < 0.2).astype(np.uint8), 3)
    nums = _numerators(core, acc)
    assert (nums[2] & 1).any()
    _check(core, acc, nums, 3)
    core.close()
    acc.close()


def test_clonal_population_is_the_caterpillar(pa):
    """N = 100, every pair d = 0 and a = 0: only row 0's cluster and its nearest neighbour are mutual, one merge per round"""
    N = 100
    core, acc = _handles(pa, np.full((N, 200), 4, np.uint8), np.tile((np.arange(50) % 3 == 0).astype(np.uint8), (N, 1)), 2)
    for got in _check(core, acc, _numerators(core, acc), 2):
        assert list(got.left) == [0] + list(range(N, 2 * N - 2)) and list(got.right) == list(range(1, N)) and not got.num.any()
        assert got.rounds == N - 1 and got.distinct_heights == 1
    core.close()
    acc.close()


def test_planted_balanced_tree(pa):
    """N = 128 leaves of a complete binary tree; every internal node owns 4 private sites where its left leaves carry base 2,
    its right leaves base 4 and all other leaves base 1 (L = 4 x 127 = 508).  For a pair whose lowest common ancestor spans
    2^l leaves d = 8 l - 4 (4 sites at the ancestor, 4 at each of the 2 (l - 1) nodes between): an ultrametric, so every round
    merges all siblings: 7 rounds, 7 heights, every merge at num = |A| |B| (8 l - 4), and the cut at each height is the blocks."""
    N, L = 128, 508
    leaves = np.full((N, L), 1, np.uint8)
    site = 0
    for level in range(1, 8):
        span = 1 << level
        for start in range(0, N, span):
            leaves[start:start + span // 2, site:site + 4] = 2
            leaves[start + span // 2:start + span, site:site + 4] = 4
            site += 4
    assert site == L
    perm = np.random.default_rng(31).permutation(N)              # row r is leaf perm[r]
    rng = np.random.default_rng(32)
    core, acc = _handles(pa, np.ascontiguousarray(leaves[perm]), (rng.random((N, 40)) < 0.3).astype(np.uint8), 3)
    nums = _numerators(core, acc)
    got = core.upgma_tree(acc, metric="core")
    ref.assert_equal(got, ref.tree(ref.CORE, *nums, N, L, 3), N)
    assert got.rounds == 7 and got.distinct_heights == 7
    k = 0
    for level in range(1, 8):
        half, count = 1 << (level - 1), N >> level
        for _ in range(count):
            assert (int(got.num[k]), int(got.den[k]), int(got.size[k])) == (half * half * (8 * level - 4), half * half * L, 2 * half)
            k += 1
        block = perm >> level                                   # the block of 2^level leaves that holds each row
        want = np.array([np.flatnonzero(block == block[r])[0] for r in range(N)], np.uint32)
        assert np.array_equal(got.cut(8 * level - 4, L), want) and got.clusters_at(8 * level - 4, L) == count
        assert got.clusters_at(8 * level - 5, L) == 2 * count
    assert k == N - 1
    core.close()
    acc.close()


def planted(seed, N=100, L=300, G=70, founders=6):
    """`founders` unrelated individuals; every other one copies an earlier member of a founder's line and moves away by up to 3
    core sites and up to 3 gene flips: within a line neighbours are close, the lines are far apart (the shape of the
    single-linkage tree's device test, restated)"""
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


@pytest.fixture(scope="module")
def planted_lines(pa):
    core_m, acc_m = planted(21)
    core, acc = _handles(pa, core_m, acc_m, 5)
    yield core, acc, _numerators(core, acc)
    core.close()
    acc.close()


def test_planted_lines_and_the_host_form(pa, planted_lines):
    """N = 100, L = 300, G = 70, 6 founders: the device, the sequential algorithm and the library's host form agree array for
    array, in fewer than N - 1 rounds"""
    core, acc, nums = planted_lines
    for (name, _), got in zip(METRICS, _check(core, acc, nums, 5)):
        assert got.rounds < 99 and got.distinct_heights >= 4
        host = pa.upgma_from_counts(*nums, 100, 300, 5, metric=name)
        for a in ("left", "right", "size", "num", "den"):
            assert np.array_equal(getattr(host, a), getattr(got, a)), a
        assert host.rounds == 0 and all(getattr(host, f) == getattr(got, f) for f in ref.INT_FIELDS)


def test_timing(pa, planted_lines):
    core, acc, _ = planted_lines
    for name, _ in METRICS:
        core.upgma_tree(acc, metric=name)
        counts_ms, store_ms, rounds_ms = core.upgma_tree_timing()
        assert counts_ms > 0.0 and store_ms > 0.0 and rounds_ms > 0.0


def test_timing_before_any_call(pa):
    core = pa.Population(4, 16, 4, True, 0.0, 0, 0)
    with pytest.raises(pa.PansimError) as e:
        core.upgma_tree_timing()
    assert e.value.code == -6 and "no UPGMA tree" in str(e.value)
    core.close()


def test_limits(pa):
    rng = np.random.default_rng(6)
    core, acc = _handles(pa, _onehot(rng, 20, 64), (rng.random((20, 10)) < 0.5).astype(np.uint8), 2)
    wide = pa.Population(20, 65536, 2, False, 0.5, 0, 2)
    for name, _ in METRICS:
        with pytest.raises(pa.PansimError) as e:
            core.upgma_tree(wide, metric=name)
        assert e.value.code == PS_ERR_INVALID and "65535 accessory genes" in str(e.value)
    none = pa.Population(20, 10, 2, False, 0.5, 0, 0)
    with pytest.raises(pa.PansimError) as e:
        core.upgma_tree(none, metric="acc")
    assert e.value.code == PS_ERR_INVALID and "core_genes >= 1" in str(e.value)
    assert core.upgma_tree(none, metric="core").merges == 19      # (the core metric does not look at the core genes)
    huge = pa.Population(20, 10, 2, False, 0.5, 0, 2**32 - 65535)
    with pytest.raises(pa.PansimError) as e:
        core.upgma_tree(huge, metric="acc")
    assert e.value.code == PS_ERR_INVALID and "core_genes + 65535 < 2^32" in str(e.value)
    big_core, big_acc = pa.Population(16385, 8, 4, True, 0.0, 0, 0), pa.Population(16385, 4, 2, False, 0.5, 0, 2)
    for name, _ in METRICS:
        with pytest.raises(pa.PansimError) as e:
            big_core.upgma_tree(big_acc, metric=name)
        assert e.value.code == PS_ERR_INVALID and "pop_size <= 16384" in str(e.value)
    for a, b in ((core, core), (acc, acc), (acc, core)):
        with pytest.raises(pa.PansimError) as e:
            a.upgma_tree(b)
        assert e.value.code == PS_ERR_INVALID and "core handle first" in str(e.value)
    with pytest.raises(ValueError):
        core.upgma_tree(acc, metric="joint")
    # a site shard on its own
    shard = pa.Population(20, 32, 4, True, 0.0, 0, 0, col_offset=32, global_cols=64)
    with pytest.raises(pa.PansimError) as e:
        shard.upgma_tree(acc)
    assert e.value.code == PS_ERR_INVALID and "ps_multi_upgma_tree" in str(e.value)
    for p in (core, acc, wide, none, huge, big_core, big_acc, shard):
        p.close()


SIM = dict(pop_size=200, core_size=2048, pan_genes=300, core_genes=20, HR_rate=0.5, HGT_rate=0.5, seed=11, n_gen=9, max_distances=100)


@pytest.fixture(scope="module")
def sim_after_six(pa):
    """the unsharded run after 6 generations: its trees, the sequential algorithm's over pairwise_counts on its handles (output
    rows), and its state after 3 more generations"""
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(6)
    got = [sim.upgma_tree(metric=name) for name, _ in METRICS]            # no sync: ordered behind the run
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
        ref.assert_monotone(g)
        assert 1 <= g.rounds <= 199
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
        ref.assert_equal(multi.upgma_tree(metric=name), w, 200)
    with pytest.raises(pa.PansimError) as e:             # a site shard on its own
        multi.shards[1].upgma_tree()
    assert e.value.code == PS_ERR_INVALID and "ps_multi_upgma_tree" in str(e.value)
    multi.close()


CLI = dict(pop_size=100, core_size=300, pan_genes=600, core_genes=200, n_gen=4, seed=9, max_distances=500, HR_rate=0.5)
USUAL = (".tsv", "_freqs.txt", "_core_genome.csv", "_pangenome.csv", "_per_gen.tsv", "_selection.tsv")
NEW = ("_upgma.tsv", "_upgma.nwk", "_upgma_summary.tsv")
SUMMARY = ("pop_size", "pairs", "core_sites", "core_genes", "metric", "merges", "distinct_heights", "root_num", "root_den")


@pytest.fixture(scope="module")
def cli_want(pa):
    """what the API gives for the command line's run, formatted as the three files, per metric"""
    sim = pa.Simulation(pa.make_params(**CLI))
    sim.run(4)
    out = {}
    for name, _ in METRICS:
        t = sim.upgma_tree(metric=name)
        assert t.merges == 99
        merges = "".join("%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (100 + k, a, b, s, n, d, pa.fmt_f64(int(n) / int(d)))
                         for k, (a, b, s, n, d) in enumerate(zip(t.left, t.right, t.size, t.num, t.den)))
        out[name] = merges, t.newick() + "\n", "".join("%s\t%d\n" % (f, getattr(t, f)) for f in SUMMARY)
    sim.close()
    return out


def _cli(*args):
    r = subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("mode,metric", [("plain", "core"), ("plain", "acc"), ("gpus2", "core"), ("gpus2", "acc"), ("load_state", "core"),
                                         ("load_state", "acc")])
def test_cli_print_upgma(pa, cli_want, tmp_path, mode, metric):
    base = [x for k, v in CLI.items() for x in ("--" + k, v)] + ["--print_dist", "--print_matrices", "--print_selection"]
    flags = ["--print_upgma"] + (["--upgma_metric", metric] if metric != "core" else [])
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
    assert set(os.listdir(tmp_path)) == {"no" + s for s in USUAL} | {"yes" + s for s in USUAL + NEW} | extra
    for suffix, text in zip(NEW, cli_want[metric]):
        assert (tmp_path / ("yes" + suffix)).read_text() == text, suffix
