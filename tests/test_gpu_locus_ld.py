"""Linkage disequilibrium between loci on the device (ps_locus_ld and its ps_sim / ps_multi forms,
docs/LINKAGE_DISEQUILIBRIUM.md) against the plain restatement (tests/ld_ref.py) over the matrices that were loaded or that
read_matrix() returns -- a path that shares nothing with the new code.  Every comparison is an equality of integers; the one
double is compared bit for bit."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import ld_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_STATE = -1, -6
BASES = np.array([1, 2, 4, 8], np.uint8)


def _onehot(rng, N, L):
    return BASES[rng.integers(0, 4, (N, L))]


def related(rng, N, L, G, founders=5, moves=3):
    """`founders` unrelated individuals; every other one copies an earlier one and moves away by a few core sites and gene
    flips (as related() of tests/test_gpu_nearest_neighbours.py): loci carry the founders' structure, r^2 is not all near 0"""
    core, acc = _onehot(rng, N, L), (rng.random((N, G)) < 0.4).astype(np.uint8)
    for k in range(min(founders, N), N):
        src = rng.integers(k)
        core[k], acc[k] = core[src], acc[src]
        sites = rng.choice(L, rng.integers(0, moves), replace=False)
        core[k, sites] = BASES[(np.log2(core[k, sites]).astype(int) + 1 + rng.integers(0, 3, sites.size)) % 4]
        if G:
            acc[k, rng.choice(G, rng.integers(0, moves), replace=False)] ^= 1
    order = rng.permutation(N)
    return np.ascontiguousarray(core[order]), np.ascontiguousarray(acc[order])


def _handles(pa, core_m, acc_m):
    N, L = core_m.shape
    core = pa.Population(N, L, 4, True, 0.0, 0, 0)
    core.load_matrix(core_m)
    acc = pa.Population(N, acc_m.shape[1], 2, False, 0.5, 0, 0)
    acc.load_matrix(acc_m)
    return core, acc


def _both(core, acc, core_m, acc_m, **kw):
    """both handles on the device against the restatement of the two matrices -> the two results"""
    out = []
    for pop, X in ((core, ref.core_indicators(core_m)), (acc, ref.acc_indicators(acc_m))):
        got = pop.locus_ld(**kw)
        ref.assert_equal(got, ref.locus_ld(X, **kw))
        assert got.pairs == got.defined_pairs + got.undefined_pairs == got.loci * (got.loci - 1) // 2
        assert all(ms >= 0.0 for ms in pop.locus_ld_timing())
        out.append(got)
    return out


@pytest.mark.parametrize("N,L,G", [(2, 8, 5), (7, 203, 40), (64, 130, 64), (65, 130, 65), (300, 1001, 500), (1000, 600, 300), (1030, 300, 100),
                                   (2049, 70, 70)])
def test_loaded_matrices(pa, N, L, G):
    """N below, at and just above a 32-, 64-, 128- and 1024-cell boundary of the pack kernels and of WP; M below and above 128
    and no multiple of it; automatic selection"""
    rng = np.random.default_rng(N)
    core_m, acc_m = related(rng, N, L, G)
    core, acc = _handles(pa, core_m, acc_m)
    by_core, by_acc = _both(core, acc, core_m, acc_m, r2_bins=64, lag_bins=4)
    if N >= 64:
        assert by_core.loci > 1 and by_acc.loci > 1 and by_core.four_gamete_pairs > 0 and (N > 300 or by_core.complete_pairs > 0)
        assert 0.0 < by_core.mean_r2 < 1.0 and np.count_nonzero(by_core.hist) > 4
    core.close()
    acc.close()


def test_the_cap_and_the_lag_bins(pa):
    """L = 1001 with more candidates than max_loci = 100 and 128 (the stride rule); lag_bins 1, 5, 32; min_minor above 1"""
    rng = np.random.default_rng(5)
    core_m, acc_m = related(rng, 90, 1001, 700, founders=8, moves=40)
    core, acc = _handles(pa, core_m, acc_m)
    for max_loci in (100, 128):
        for lag_bins in (1, 5, 32):
            by_core, by_acc = _both(core, acc, core_m, acc_m, r2_bins=16, lag_bins=lag_bins, max_loci=max_loci)
            assert by_core.candidates > max_loci == by_core.loci and by_acc.candidates > max_loci == by_acc.loci
    _both(core, acc, core_m, acc_m, r2_bins=16, lag_bins=3, min_minor=9, max_loci=4096)
    _both(core, acc, core_m, acc_m, r2_bins=1, lag_bins=1, min_minor=45, max_loci=7)
    core.close()
    acc.close()


def test_an_explicit_list_with_monomorphic_entries(pa):
    """their pairs are undefined and nothing else; the other pairs are those of the list without them"""
    rng = np.random.default_rng(8)
    N, L, G = 200, 150, 90
    core_m, acc_m = related(rng, N, L, G)
    core_m[:, [3, 77]] = 4
    acc_m[:, 10], acc_m[:, 50] = 0, 1
    core, acc = _handles(pa, core_m, acc_m)
    for pop, X, mono in ((core, ref.core_indicators(core_m), [3, 77]), (acc, ref.acc_indicators(acc_m), [10, 50])):
        loci = sorted(set(rng.choice(X.shape[0], 60, replace=False).tolist()) | set(mono))
        got = pop.locus_ld(r2_bins=32, lag_bins=6, loci=loci)
        ref.assert_equal(got, ref.locus_ld(X, r2_bins=32, lag_bins=6, loci=loci))
        M = len(loci)
        n_mono = int(((got.locus_count == 0) | (got.locus_count == N)).sum())
        assert n_mono >= 2 and got.undefined_pairs == M * (M - 1) // 2 - (M - n_mono) * (M - n_mono - 1) // 2
        rest = pop.locus_ld(r2_bins=32, lag_bins=6, loci=[s for s, c in zip(loci, got.locus_count) if 0 < c < N])
        assert np.array_equal(rest.hist, got.hist) and rest.undefined_pairs == 0 and rest.sum_q == got.sum_q
        for bad in ([5, 5], [9, 4], [0, X.shape[0]]):
            with pytest.raises(pa.PansimError) as e:
                pop.locus_ld(loci=bad)
            assert e.value.code == PS_ERR_INVALID
    core.close()
    acc.close()


def test_not_one_hot(pa):
    """arbitrary bytes in about 5 % of the cells: they are in no class, neither for the major base nor for the indicator"""
    rng = np.random.default_rng(31)
    N, L, G = 130, 300, 40
    core_m, acc_m = related(rng, N, L, G)
    cells = rng.random((N, L)) < 0.05
    core_m[cells] = rng.integers(0, 256, int(cells.sum()), dtype=np.uint8)
    core_m[:, 7] = 3                      # a site without a single base: monomorphic at c = 0
    core_m[: N // 2, 8], core_m[N // 2:, 8] = 1, 2        # a tie: the lowest byte is the major base
    core, acc = _handles(pa, core_m, acc_m)
    got = core.locus_ld(r2_bins=64, lag_bins=3)
    ref.assert_equal(got, ref.locus_ld(ref.core_indicators(core_m), r2_bins=64, lag_bins=3))
    loci = [6, 7, 8, 9]
    got = core.locus_ld(loci=loci)
    ref.assert_equal(got, ref.locus_ld(ref.core_indicators(core_m), loci=loci))
    assert got.locus_count[1] == 0 and got.locus_count[2] == int((core_m[:, 8] == 1).sum())
    core.close()
    acc.close()


def test_a_population_of_clones(pa):
    """a simulation at generation 0: no candidate, M = 0, zero pairs"""
    sim = pa.Simulation(pa.make_params(pop_size=100, core_size=2048, pan_genes=300, core_genes=20, seed=4, n_gen=3, max_distances=100))
    for metric in ("core", "acc"):
        got = sim.locus_ld(metric)
        assert got.loci == got.candidates == got.pairs == got.defined_pairs == got.undefined_pairs == got.sum_q == 0
        assert got.mean_r2 == 0.0 and not got.hist.any() and got.locus_index.size == 0
        assert got.columns == (2048 if metric == "core" else sim.pan_genome.ncols)
    with pytest.raises(ValueError):
        sim.locus_ld("joint")
    sim.close()


def test_three_bands_equal_one(pa):
    """M = 300 with ld_band = 128: three bands (128 + 128 + 44 rows) equal the unforced call"""
    rng = np.random.default_rng(7)
    core_m, acc_m = related(rng, 150, 700, 330, founders=9, moves=30)
    core, acc = _handles(pa, core_m, acc_m)
    whole = _both(core, acc, core_m, acc_m, r2_bins=32, lag_bins=8, max_loci=300)
    assert whole[0].loci == 300 and whole[1].loci == 300
    for pop, w in zip((core, acc), whole):
        pop.set_tuning("ld_band", 128)
        got = pop.locus_ld(r2_bins=32, lag_bins=8, max_loci=300)
        assert got.summary() == w.summary() and np.array_equal(got.hist, w.hist) and np.array_equal(got.lag_sum_q, w.lag_sum_q)
        pop.set_tuning("ld_band", 0)
    core.close()
    acc.close()


def test_the_u16_edge_at_65536_individuals(pa):
    """N = 65536, L = 40, explicit loci: two identical sites with c = 65535 (n11 = 65535, the largest a u16 holds), a pair with
    n11 = 0, and monomorphic sites (c = 65536: their rows are zeroed, no count leaves 16 bits)"""
    rng = np.random.default_rng(65536)
    N, L = 65536, 40
    core_m = np.ones((N, L), np.uint8)
    for s in range(10, L):
        core_m[rng.random(N) < rng.choice([0.02, 0.3, 0.5]), s] = 8
    core_m[12345, 2] = core_m[12345, 5] = 2           # two identical sites, c = 65535
    core_m[:, 6] = 1
    core_m[: N // 2, 6] = 4                            # c = 32768 twice: a tie, major base 1 = the upper half
    core_m[:, 7] = 4
    core_m[: N // 2, 7] = 1                            # ... its complement: n11 = 0
    core = pa.Population(N, L, 4, True, 0.0, 0, 0)
    core.load_matrix(core_m)
    X = ref.core_indicators(core_m)
    loci = [0, 2, 5, 6, 7] + list(range(10, L))
    got = core.locus_ld(r2_bins=128, lag_bins=6, loci=loci)
    ref.assert_equal(got, ref.locus_ld(X, r2_bins=128, lag_bins=6, loci=loci))
    assert got.locus_count[0] == N and got.locus_count[1] == got.locus_count[2] == 65535 and got.locus_count[3] == got.locus_count[4] == 32768
    pair = core.locus_ld(loci=[2, 5])
    assert pair.sum_q == 65536 and pair.complete_pairs == 1 and pair.positive_pairs == 1
    pair = core.locus_ld(loci=[6, 7])
    assert pair.sum_q == 65536 and pair.negative_pairs == 1 and int((X[6].astype(int) * X[7]).sum()) == 0
    ref.assert_equal(core.locus_ld(min_minor=1), ref.locus_ld(X, min_minor=1))
    core.close()


SIM = dict(core_size=2048, pan_genes=300, core_genes=20, HR_rate=0.5, HGT_rate=0.5, prop_positive=0.5, seed=11, n_gen=8, max_distances=100)
KW = dict(r2_bins=32, lag_bins=5, max_loci=200)


def _restated(sim, **kw):
    core_m, acc_m = sim.core_genome.read_matrix(), sim.pan_genome.read_matrix()
    return (core_m, acc_m), [ref.locus_ld(ref.core_indicators(core_m), **kw), ref.locus_ld(ref.acc_indicators(acc_m), **kw)]


@pytest.fixture(scope="module")
def sim_200_after_five(pa):
    sim = pa.Simulation(pa.make_params(pop_size=200, **SIM))
    sim.run(5)
    got = [sim.locus_ld(metric, **KW) for metric in ("core", "acc")]          # no sync: ordered behind the run
    before, want = _restated(sim, **KW)
    after, _ = _restated(sim, **KW)
    sim.run(3)
    state = (sim.core_genome.read_matrix(), sim.pan_genome.read_matrix(), sim.last_parents())
    sim.close()
    return got, want, before, after, state


def _check_sim(pa, N, fixture):
    got, want, before, after, state = fixture
    for g, w in zip(got, want):
        ref.assert_equal(g, w)
    assert got[0].loci > 1
    assert all(np.array_equal(b, a) for b, a in zip(before, after))
    # the calls changed no state: the run that asked continues bit for bit with one that never did
    plain = pa.Simulation(pa.make_params(pop_size=N, **SIM))
    plain.run(8)
    assert np.array_equal(plain.core_genome.read_matrix(), state[0]) and np.array_equal(plain.pan_genome.read_matrix(), state[1])
    assert np.array_equal(plain.last_parents(), state[2])
    plain.close()


def test_a_simulation_after_five_generations(pa, sim_200_after_five):
    """N = 200: the wave sweep (two generations per launch) precedes the call"""
    _check_sim(pa, 200, sim_200_after_five)


def test_a_wide_simulation_after_five_generations(pa):
    """N = 1500: the window sweep precedes the call; rows longer than one 1 KiB piece"""
    sim = pa.Simulation(pa.make_params(pop_size=1500, **SIM))
    sim.run(5)
    got = [sim.locus_ld(metric, **KW) for metric in ("core", "acc")]
    before, want = _restated(sim, **KW)
    after, _ = _restated(sim, **KW)
    sim.run(3)
    state = (sim.core_genome.read_matrix(), sim.pan_genome.read_matrix(), sim.last_parents())
    sim.close()
    _check_sim(pa, 1500, (got, want, before, after, state))


def test_three_shards_equal_the_unsharded_run(pa, sim_200_after_five):
    _, want, _, _, _ = sim_200_after_five
    multi = pa.MultiSimulation(pa.make_params(pop_size=200, **SIM), 3, devices=[0, 0, 0])
    multi.run(5)
    for metric, w in zip(("core", "acc"), want):
        ref.assert_equal(multi.locus_ld(metric, **KW), w)
    # fewer loci than candidates, all of them, and an explicit list across the shards
    core_m = np.concatenate([s.core_genome.read_matrix() for s in multi.shards], axis=1)
    X = ref.core_indicators(core_m)
    for kw in (dict(max_loci=37), dict(max_loci=4096, lag_bins=11), dict(loci=list(range(0, 2048, 29)), lag_bins=11)):
        ref.assert_equal(multi.locus_ld("core", **kw), ref.locus_ld(X, **kw))
    with pytest.raises(pa.PansimError) as e:             # a site shard on its own
        multi.shards[1].core_genome.locus_ld()
    assert e.value.code == PS_ERR_INVALID and "ps_multi_locus_ld" in str(e.value)
    multi.close()


def test_limits(pa):
    rng = np.random.default_rng(6)
    core, acc = _handles(pa, _onehot(rng, 20, 64), (rng.random((20, 10)) < 0.5).astype(np.uint8))
    with pytest.raises(pa.PansimError) as e:
        core.locus_ld_timing()
    assert e.value.code == PS_ERR_STATE and "no linkage disequilibrium" in str(e.value)
    for kw in (dict(r2_bins=0), dict(lag_bins=0), dict(lag_bins=33), dict(r2_bins=16385), dict(r2_bins=1024, lag_bins=32), dict(min_minor=0),
               dict(max_loci=0), dict(max_loci=65537)):
        for pop in (core, acc):
            with pytest.raises(pa.PansimError) as e:
                pop.locus_ld(**kw)
            assert e.value.code == PS_ERR_INVALID, kw
    for p in (core, acc):
        p.close()


CLI = dict(pop_size=100, core_size=300, pan_genes=600, core_genes=200, n_gen=4, seed=9, max_distances=500, HR_rate=0.5)
USUAL = (".tsv", "_freqs.txt", "_core_genome.csv", "_pangenome.csv", "_per_gen.tsv", "_selection.tsv")
NEW = ("_ld.tsv", "_ld_summary.tsv", "_ld_loci.tsv")


def _cli(*args):
    r = subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def _read_csv(path, lut):
    rows = open(path, "rb").read().splitlines()
    text = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)[:, ::2]
    return lut[text]


def _tsv_files(want, metric, fmt):
    nl, nr = want["lag_bins"], want["r2_bins"]
    hist = "".join("%d\t%d\t%d\n" % (l, r, want["hist"][l, r]) for l in range(nl) for r in range(nr) if want["hist"][l, r])
    names = ("pop_size", "metric", "columns", "candidates", "loci", "pairs", "defined_pairs", "undefined_pairs", "four_gamete_pairs",
             "complete_pairs", "positive_pairs", "negative_pairs", "sum_q", "r2_bins", "lag_bins", "min_minor", "max_loci")
    values = dict(want, metric=0 if metric == "core" else 1)
    summary = "".join("%s\t%d\n" % (n, values[n]) for n in names) + "mean_r2\t%s\n" % fmt(want["mean_r2"])
    summary += "".join("lag\t%d\t%d\t%d\n" % (l, want["hist"][l].sum(), want["lag_sum_q"][l]) for l in range(nl) if want["hist"][l].sum())
    loci = "".join("%d\t%d\n" % (s, c) for s, c in zip(want["locus_index"], want["locus_count"]))
    return hist, summary, loci


@pytest.mark.parametrize("mode,metric", [("plain", "core"), ("plain", "acc"), ("gpus2", "core"), ("gpus2", "acc"), ("load_state", "core")])
def test_cli_print_ld(pa, tmp_path, mode, metric):
    """the three files equal the restatement of the matrices the same run wrote, as text; the usual outputs do not change"""
    base = [x for k, v in CLI.items() for x in ("--" + k, v)] + ["--print_dist", "--print_matrices", "--print_selection"]
    flags = ["--print_ld", "--ld_bins", "16,4", "--ld_max_loci", 50] + (["--ld_metric", metric, "--ld_min_minor", 2] if metric != "core" else [])
    kw = dict(r2_bins=16, lag_bins=4, max_loci=50, min_minor=1 if metric == "core" else 2)
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
    lut = np.zeros(256, np.uint8)
    for ch, v in zip(b"ACGT01", (1, 2, 4, 8, 0, 1)):
        lut[ch] = v
    core_m, pan = _read_csv(tmp_path / "yes_core_genome.csv", lut), _read_csv(tmp_path / "yes_pangenome.csv", lut)
    cg = CLI["core_genes"]
    assert core_m.shape == (100, 300) and pan.shape[0] == 100 and pan[:, :cg].all()      # (the core genes lead every line as 1s)
    X = ref.core_indicators(core_m) if metric == "core" else ref.acc_indicators(pan[:, cg:])
    want = ref.locus_ld(X, **kw)
    assert want["loci"] > 1
    for suffix, text in zip(NEW, _tsv_files(want, metric, pa.fmt_f64)):
        assert (tmp_path / ("yes" + suffix)).read_text() == text, suffix
