"""The recorded genealogy on the device (ps_sim_record_ancestry, ps_sim_genealogy, ps_sim_clock_histogram and their ps_multi
forms, docs/GENEALOGY.md) against a truth from an independent path: a twin run with the same seed, one generation per call,
whose ps_sim_last_parents of every generation give the all-pairs matrix of divergence times by brute force
(tests/genealogy_ref.py).  Every comparison is an equality of integers, of bytes or of text."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import genealogy_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_STATE = -1, -6
METRICS = (("core", ref.CORE), ("acc", ref.ACC))
BASE = dict(core_size=300, pan_genes=260, core_genes=20, HR_rate=0.5, HGT_rate=0.5, max_distances=50)


def params(pa, N, gens, seed=5, **kw):
    return pa.make_params(**{**BASE, "pop_size": N, "n_gen": gens, "seed": seed, **kw})


def twin_parents(pa, prm, gens):
    """the draws of every generation in output rows from a run that takes one generation per call -> (list, oldest first; the twin)"""
    twin = pa.Simulation(prm)
    out = []
    for _ in range(gens):
        twin.run(1)
        out.append(twin.last_parents())
    return out, twin


def check_comb(g, T, depth, capacity, generation):
    """the comb against the matrix of the truth: every pair, the summary, the clusters at a few look-backs"""
    N = T.shape[0]
    assert sorted(g.order.tolist()) == list(range(N)) and g.coal.size == N - 1
    r1, r2 = ref.all_pairs(N)
    assert np.array_equal(g.pairs(r1, r2), T[r1, r2])
    for i, j in ((0, N - 1), (N - 1, 0), (N // 2, N // 2), (0, 1)):
        assert g.pair(i, j) == T[i, j]
    assert {name: getattr(g, name) for name in g.FIELDS} == ref.summary(T, depth, capacity, generation)
    for t in sorted({0, 1, depth // 2, depth}):
        labels, out = g.clusters(t)
        want_labels, want = ref.clusters(T, t)
        assert np.array_equal(labels, want_labels) and out == want, t
    if N <= 65:
        assert g.newick() == ref.newick(g.order, T)


@pytest.fixture(scope="module")
def truth(pa):
    """(N, gens) -> (the matrix of the truth, the recording run after all its generations in ONE call), computed once"""
    made = {}

    def get(N, gens, **kw):
        key = (N, gens, tuple(sorted(kw.items())))
        if key not in made:
            prm = params(pa, N, gens, **kw)
            parents, twin = twin_parents(pa, prm, gens)
            state = twin.core_genome.read_matrix(), twin.pan_genome.read_matrix()
            twin.close()
            sim = pa.Simulation(params(pa, N, gens, **kw))
            sim.record_ancestry(gens)
            sim.run(gens)
            made[key] = ref.tmrca_matrix(parents, N), sim, state
        return made[key]

    yield get
    for _, sim, _ in made.values():
        sim.close()


@pytest.mark.parametrize("gens", [7, 12])
@pytest.mark.parametrize("N", [2, 5, 64, 65, 257, 1000, 1100])
def test_every_pair_equals_the_brute_force_truth(pa, truth, N, gens):
    """odd and even numbers of generations in one call: two-generation sweep launches with and without a remainder up to
    N = 1024, the window sweep above; a neutral short run leaves pairs beyond the record"""
    T, sim, state = truth(N, gens)
    g = sim.genealogy()
    check_comb(g, T, gens, gens, gens)
    if N >= 257:
        assert g.roots > 1 and (g.coal == ref.BEYOND).any() and (T == ref.BEYOND).any()
    # recording changed nothing: the run equals its twin, which recorded nothing, byte for byte -- after the read-out too
    assert np.array_equal(sim.core_genome.read_matrix(), state[0]) and np.array_equal(sim.pan_genome.read_matrix(), state[1])


@pytest.mark.parametrize("N", [65, 1000])
def test_the_device_draw(pa, monkeypatch, N):
    """the draw on the device (chosen from 4096 individuals on; forced here) fills the same ring slot by a counting sort of its own"""
    monkeypatch.setenv("PANSIM_DEVICE_DRAW", "1")
    prm = params(pa, N, 7, seed=8)
    parents, twin = twin_parents(pa, prm, 7)
    twin.close()
    sim = pa.Simulation(params(pa, N, 7, seed=8))
    sim.record_ancestry(10)
    sim.run(7)
    check_comb(sim.genealogy(), ref.tmrca_matrix(parents, N), 7, 10, 7)
    sim.close()


def test_strong_selection_coalesces_fully(pa):
    kw = dict(prop_positive=0.5, pos_lambda=2.0, competition_strength=5.0)
    N, gens = 30, 200
    parents, twin = twin_parents(pa, params(pa, N, gens, **kw), gens)
    twin.close()
    sim = pa.Simulation(params(pa, N, gens, **kw))
    sim.record_ancestry(gens)
    sim.run(gens)
    T = ref.tmrca_matrix(parents, N)
    g = sim.genealogy()
    check_comb(g, T, gens, gens, gens)
    assert g.roots == 1 and g.tmrca == int(T.max()) and 1 <= g.tmrca <= gens and g.newick().count("\n") == 1
    sim.close()


def test_the_ring_keeps_the_last_generations(pa):
    """capacity 3 with 8 generations: depth 3 and the truth over the last 3 draws only"""
    N = 130
    parents, twin = twin_parents(pa, params(pa, N, 8), 8)
    twin.close()
    sim = pa.Simulation(params(pa, N, 8))
    sim.record_ancestry(3)
    sim.run(8)
    check_comb(sim.genealogy(), ref.tmrca_matrix(parents[-3:], N), 3, 3, 8)
    sim.close()


def test_resets_of_the_record(pa, tmp_path):
    N = 65
    parents, twin = twin_parents(pa, params(pa, N, 9), 9)
    twin.close()
    sim = pa.Simulation(params(pa, N, 9))
    # nothing recorded yet: PS_ERR_STATE with the way out in the message
    for call in (sim.genealogy, sim.clock_histogram):
        with pytest.raises(pa.PansimError) as e:
            call()
        assert e.value.code == PS_ERR_STATE and "ps_sim_record_ancestry" in str(e.value)
    sim.record_ancestry(0)
    sim.run(4)
    with pytest.raises(pa.PansimError) as e:
        sim.genealogy()
    assert e.value.code == PS_ERR_STATE
    # switched on mid-run: an empty record (every individual its own root), then the generations from here on
    sim.record_ancestry(20)
    g = sim.genealogy()
    assert (g.depth, g.roots, g.tmrca, g.generation) == (0, N, 0, 4) and (g.coal == ref.BEYOND).all()
    with pytest.raises(pa.PansimError) as e:
        sim.clock_histogram()
    assert e.value.code == PS_ERR_STATE and "no generation has been recorded" in str(e.value)
    sim.run(3)
    check_comb(sim.genealogy(), ref.tmrca_matrix(parents[4:7], N), 3, 20, 7)
    # a state file carries no record: the loaded run records nothing; the saving run goes on recording
    path = str(tmp_path / "seven.state")
    sim.save(path)
    loaded = pa.Simulation.load(path)
    with pytest.raises(pa.PansimError) as e:
        loaded.genealogy()
    assert e.value.code == PS_ERR_STATE and "ps_sim_record_ancestry" in str(e.value)
    loaded.record_ancestry(5)
    loaded.run(2)
    check_comb(loaded.genealogy(), ref.tmrca_matrix(parents[7:9], N), 2, 5, 9)
    loaded.close()
    sim.run(2)
    check_comb(sim.genealogy(), ref.tmrca_matrix(parents[4:9], N), 5, 20, 9)
    # a matrix loaded into a handle: the next generation starts the record again
    sim.pan_genome.load_matrix(sim.pan_genome.read_matrix())
    sim.run(1)
    assert sim.genealogy().depth == 1
    sim.run(2)
    assert sim.genealogy().depth == 3
    # a run that does not continue the last one
    sim.run(2, first_generation=40)
    g = sim.genealogy()
    assert (g.depth, g.generation) == (2, 42)
    sim.run(1)
    assert sim.genealogy().depth == 3
    sim.record_ancestry(20)                                  # (any call starts an empty record)
    assert sim.genealogy().depth == 0
    sim.close()


def test_reset_by_a_loaded_matrix_gives_the_truth_of_the_generations_after_it(pa):
    """both matrices loaded again after 3 generations (their rows are then stored in the order of the outputs): the record restarts"""
    N = 64
    sim = pa.Simulation(params(pa, N, 6))
    sim.record_ancestry(10)
    sim.run(3)
    core_m, acc_m = sim.core_genome.read_matrix(), sim.pan_genome.read_matrix()
    sim.core_genome.load_matrix(core_m)
    sim.pan_genome.load_matrix(acc_m)
    parents = []
    for _ in range(3):
        sim.run(1)
        parents.append(sim.last_parents())
    g = sim.genealogy()
    assert g.depth == 3
    # (how the first draw after the load names its parents does not matter: of the oldest recorded draw only equality is used)
    check_comb(g, ref.tmrca_matrix(parents, N), 3, 10, 6)
    sim.close()


def counts(sim, N):
    r1, r2 = ref.all_pairs(N)
    (h,), (i, u) = sim.core_genome.pairwise_counts(r1, r2), sim.pan_genome.pairwise_counts(r1, r2)
    return r1, r2, h, i, u


def check_clock(sim, T, depth, N, cnt=None, **kw):
    r1, r2, h, i, u = cnt or counts(sim, N)
    p = sim.params
    out = []
    for name, metric in METRICS:
        got = sim.clock_histogram(metric=name, **kw)
        bt, bx = kw.get("time_bins", 32), kw.get("dist_bins", 64)
        want = ref.clock_from_counts(metric, T[r1, r2], h, i, u, depth, p.core_size, p.core_genes, bt, bx, kw.get("time_span") or 0,
                                     kw.get("core_span") or 0)
        want["pop_size"] = N
        ref.assert_clock(got, want)
        assert int(got.joint.sum()) + got.undefined_pairs == N * (N - 1) // 2 == got.pairs
        assert got.beyond_pairs == int(got.joint[-1].sum())
        if name == "core":
            assert got.beyond_pairs == int((T[r1, r2] == ref.BEYOND).sum())
        counts_ms, bin_ms = sim.clock_histogram_timing()
        assert bin_ms > 0.0 and (counts_ms > 0.0 or name == "acc")
        out.append(got)
    return out


@pytest.mark.parametrize("N,band", [(65, 0), (600, 256), (1100, 0)])
def test_clock_histogram_equals_the_restatement(pa, truth, N, band):
    """the counts of ps_pairwise_counts over all pairs in output rows and the brute-force times through the plain restatement;
    N = 600 with bands of 256 rows: three bands, the last with pad rows, and the automatic core span counts twice"""
    T, sim, state = truth(N, 12)
    sim.core_genome.set_tuning("core_davg_band", band)
    cnt = counts(sim, N)
    by_core, by_acc = check_clock(sim, T, 12, N, cnt)
    comb = sim.genealogy()
    assert by_core.beyond_pairs == int((comb.pairs(*ref.all_pairs(N)) == ref.BEYOND).sum())
    assert by_core.core_clamped == 0 and by_core.binned_pairs == by_core.pairs
    check_clock(sim, T, 12, N, cnt, time_bins=5, dist_bins=7, time_span=4, core_span=3)          # (both axes clamp)
    check_clock(sim, T, 12, N, cnt, time_bins=12, dist_bins=1, core_span=10**6)
    sim.core_genome.set_tuning("core_davg_band", 0)
    assert np.array_equal(sim.core_genome.read_matrix(), state[0]) and np.array_equal(sim.pan_genome.read_matrix(), state[1])


def test_clock_histogram_with_the_most_bins(pa, truth):
    """1023 time bins of 16 and 3 of 4096: the largest LDS footprints the limits admit"""
    T, sim, _ = truth(65, 12)
    check_clock(sim, T, 12, 65, time_bins=1023, dist_bins=16)
    check_clock(sim, T, 12, 65, time_bins=3, dist_bins=4096)
    for kw, text in ((dict(time_bins=1025, dist_bins=1), "1024 time bins"), (dict(time_bins=1023, dist_bins=17), "16384 bins"),
                     (dict(time_bins=0), ">= 1"), (dict(time_span=2**32), "2^32 - 1 generations")):
        with pytest.raises(pa.PansimError) as e:
            sim.clock_histogram(**kw)
        assert e.value.code == PS_ERR_INVALID and text in str(e.value)
    with pytest.raises(ValueError):
        sim.clock_histogram(metric="joint")


def test_clock_histogram_without_accessory_genes(pa):
    """pan_genes = core_genes: an accessory matrix of no columns, no accessory kernel launched; every pair is at 0 / core_genes
    (a run needs core_genes >= 1 there: the all-undefined case is covered on the host, tests/test_genealogy.py)"""
    N, gens, cg = 70, 7, 20
    kw = dict(pan_genes=cg, core_genes=cg)
    parents, twin = twin_parents(pa, params(pa, N, gens, **kw), gens)
    twin.close()
    sim = pa.Simulation(params(pa, N, gens, **kw))
    assert sim.pan_genome.ncols == 0
    sim.record_ancestry(gens)
    sim.run(gens)
    T = ref.tmrca_matrix(parents, N)
    check_comb(sim.genealogy(), T, gens, gens, gens)
    r1, r2 = ref.all_pairs(N)
    zero = np.zeros(r1.size, np.uint32)
    got = sim.clock_histogram(metric="acc", time_bins=4, dist_bins=3)
    want = ref.clock_from_counts(ref.ACC, T[r1, r2], None, zero, zero, gens, BASE["core_size"], cg, 4, 3)
    want["pop_size"] = N
    ref.assert_clock(got, want)
    assert got.undefined_pairs == 0 and got.num_sum == 0 and got.den_sum == cg * r1.size
    (h,) = sim.core_genome.pairwise_counts(r1, r2)
    got = sim.clock_histogram(time_bins=4, dist_bins=3)
    want = ref.clock_from_counts(ref.CORE, T[r1, r2], h, None, None, gens, BASE["core_size"], cg, 4, 3)
    want["pop_size"] = N
    ref.assert_clock(got, want)
    sim.close()


def test_two_shards_equal_the_unsharded_run(pa, truth):
    N, gens = 257, 7
    T, sim, _ = truth(N, gens)
    multi = pa.MultiSimulation(params(pa, N, gens), 2, devices=[0, 0])
    multi.record_ancestry(gens)
    multi.run(gens)
    g, want = multi.genealogy(), sim.genealogy()
    assert np.array_equal(g.order, want.order) and np.array_equal(g.coal, want.coal)
    assert all(getattr(g, name) == getattr(want, name) for name in g.FIELDS)
    check_comb(g, T, gens, gens, gens)
    for name, _ in METRICS:
        a, b = multi.clock_histogram(metric=name, time_bins=7, dist_bins=9), sim.clock_histogram(metric=name, time_bins=7, dist_bins=9)
        assert np.array_equal(a.joint, b.joint) and np.array_equal(a.per_time, b.per_time)
        assert all(getattr(a, f) == getattr(b, f) for f in a.FIELDS)
    assert multi.clock_histogram_timing()[1] > 0.0
    with pytest.raises(pa.PansimError) as e:             # a site shard on its own
        multi.shards[0].clock_histogram()
    assert e.value.code == PS_ERR_INVALID and "ps_multi_clock_histogram" in str(e.value)
    multi.close()


CLI = dict(pop_size=100, core_size=300, pan_genes=600, core_genes=200, n_gen=6, seed=9, max_distances=500, HR_rate=0.5)
USUAL = (".tsv", "_freqs.txt", "_core_genome.csv", "_pangenome.csv", "_per_gen.tsv", "_selection.tsv")
NEW = ("_genealogy.tsv", "_genealogy.nwk", "_clock.tsv", "_clock_summary.tsv")


def _cli(*args):
    r = subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def _read_csv(path, lut):
    rows = open(path, "rb").read().splitlines()
    text = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)[:, ::2]
    return lut[text]


@pytest.mark.parametrize("mode,metric", [("plain", "core"), ("plain", "acc"), ("gpus2", "core")])
def test_cli_print_genealogy(pa, tmp_path, mode, metric):
    """the four files equal the restatement's text: the times from a twin run of the library with the command line's parameters,
    the counts from the matrices the same command wrote; the usual outputs do not change"""
    base = [x for k, v in CLI.items() for x in ("--" + k, v)] + ["--print_matrices", "--print_selection"]
    flags = ["--print_genealogy", 4, "--clock_bins", "4,8"] + (["--clock_metric", metric] if metric != "core" else [])
    if mode == "gpus2":
        base += ["--gpus", 2]
    usual = tuple(s for s in USUAL if s != "_per_gen.tsv")
    _cli(*base, "--outpref", tmp_path / "no")
    _cli(*base, *flags, "--outpref", tmp_path / "yes")
    for suffix in usual:
        assert filecmp.cmp(str(tmp_path / "no") + suffix, str(tmp_path / "yes") + suffix, shallow=False), suffix
    assert set(os.listdir(tmp_path)) == {"no" + s for s in usual} | {"yes" + s for s in usual + NEW}
    N, gens, cg = CLI["pop_size"], CLI["n_gen"], CLI["core_genes"]
    parents, twin = twin_parents(pa, pa.make_params(**CLI), gens)
    twin.close()
    T = ref.tmrca_matrix(parents[-4:], N)
    lines = [l.split("\t") for l in (tmp_path / "yes_genealogy.tsv").read_text().splitlines()]
    order = np.array([int(l[1]) for l in lines], np.uint32)
    coal = np.array([ref.BEYOND if l[2] == "beyond" else int(l[2]) for l in lines[:-1]], np.uint32)
    assert [int(l[0]) for l in lines] == list(range(N)) and lines[-1][2] == ""
    assert (tmp_path / "yes_genealogy.tsv").read_text() == ref.genealogy_tsv(order, coal)
    r1, r2 = ref.all_pairs(N)
    assert np.array_equal(pa.genealogy_pairs(order, coal, r1, r2), T[r1, r2])
    assert (tmp_path / "yes_genealogy.nwk").read_text() == ref.newick(order, T)
    lut = np.zeros(256, np.uint8)
    for ch, v in zip(b"ACGT01", (1, 2, 4, 8, 0, 1)):
        lut[ch] = v
    core_m, pan = _read_csv(tmp_path / "yes_core_genome.csv", lut), _read_csv(tmp_path / "yes_pangenome.csv", lut)
    acc_m = pan[:, cg:].astype(np.int64)
    h = 2 * (core_m[r1] != core_m[r2]).sum(1)                     # (one-hot rows: every differing site counts twice)
    inter = (acc_m[r1] & acc_m[r2]).sum(1)
    union = (acc_m[r1] | acc_m[r2]).sum(1)
    want = ref.clock_from_counts(dict(METRICS)[metric], T[r1, r2], h, inter, union, 4, CLI["core_size"], cg, 4, 8)
    want["pop_size"] = N
    assert (tmp_path / "yes_clock.tsv").read_text() == ref.clock_tsv(want["joint"])
    assert (tmp_path / "yes_clock_summary.tsv").read_text() == ref.clock_summary_tsv(want, ref.summary(T, 4, 4, gens))
