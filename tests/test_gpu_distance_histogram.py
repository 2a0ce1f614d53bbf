"""The joint distance histogram on the device (ps_distance_histogram and its ps_sim / ps_multi forms,
docs/DISTANCE_HISTOGRAM.md) against the plain-integer restatement (tests/distance_histogram_ref.py) of the numerators
that the existing ps_pairwise_counts returns for the full i < j list -- a path that shares nothing with the new code.
Every comparison is an equality of `joint` and of every integer field."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import distance_histogram_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID = -1


def _onehot(rng, N, L):
    p = rng.dirichlet([0.25] * 4, L)
    u = rng.random((N, L))
    m = (u[:, :, None] > np.cumsum(p, 1)[None, :, :3]).sum(2)
    return (1 << m).astype(np.uint8)


def _handles(pa, N, L, G, cg, core_matrix, acc_matrix):
    core = pa.Population(N, L, 4, True, 0.0, 0, 0)
    core.load_matrix(core_matrix)
    acc = pa.Population(N, G, 2, False, 0.5, 0, cg)
    if G:
        acc.load_matrix(acc_matrix)
    return core, acc


def _numerators(core, acc):
    """(h, I, U) of every pair i < j from the existing sampled-pair path"""
    r1, r2 = ref.all_pairs(core.size)
    (h,) = core.pairwise_counts(r1, r2)
    if acc.ncols:
        i, u = acc.pairwise_counts(r1, r2)
    else:
        i = u = np.zeros(r1.size, np.uint32)
    return h, i, u


def _want(core, acc, L, cg, Bc, Ba, span=0):
    return ref.histogram(*_numerators(core, acc), L, cg, Bc, Ba, span)


@pytest.fixture(scope="module")
def shape1(pa):
    """N = 100, L = 300, G = 70, cg = 5: one tile, one band; sites no multiple of 128; the genes cross one u64 word"""
    rng = np.random.default_rng(1)
    N, L, G, cg = 100, 300, 70, 5
    core, acc = _handles(pa, N, L, G, cg, _onehot(rng, N, L), (rng.random((N, G)) < 0.4).astype(np.uint8))
    yield core, acc, _numerators(core, acc), (N, L, G, cg)
    core.close()
    acc.close()


def test_one_tile_one_band(pa, shape1):
    core, acc, (h, i, u), (N, L, G, cg) = shape1
    got = core.distance_histogram(acc, 64, 64, core_span=L)
    ref.assert_equal(got, ref.histogram(h, i, u, L, cg, 64, 64, L), pop_size=N)
    assert got.pairs == N * (N - 1) // 2 and got.undefined_pairs == 0 and got.core_clamped == 0
    assert got.core_d_sum == core.core_diversity()["pair_differences"]
    # the host restatement of the library agrees as well, and the distance form of the span is the same call
    host = pa.histogram_from_counts(h, i, u, L, cg, 64, 64, core_span=L)
    assert np.array_equal(host.joint, got.joint) and host.core_d_sqsum == got.core_d_sqsum
    assert np.array_equal(core.distance_histogram(acc, 64, 64, core_max=1.0).joint, got.joint)
    counts_ms, bin_ms = core.distance_histogram_timing()
    assert counts_ms > 0.0 and bin_ms > 0.0


@pytest.mark.parametrize("Bc,Ba", [(1, 1), (128, 128), (16384, 1), (1, 16384)])
def test_bin_limits_and_degenerate_axes(pa, shape1, Bc, Ba):
    core, acc, (h, i, u), (N, L, G, cg) = shape1
    for span in (0, 150):
        ref.assert_equal(core.distance_histogram(acc, Bc, Ba, core_span=span), ref.histogram(h, i, u, L, cg, Bc, Ba, span), pop_size=N)


def test_clamping_and_the_automatic_span(pa, shape1):
    core, acc, (h, i, u), (N, L, G, cg) = shape1
    got = core.distance_histogram(acc, 64, 64, core_span=3)
    ref.assert_equal(got, ref.histogram(h, i, u, L, cg, 64, 64, 3), pop_size=N)
    assert got.core_clamped == int(((h // 2) >= 3).sum()) > 0 and got.core_span == 3
    got = core.distance_histogram(acc, 64, 64)
    ref.assert_equal(got, ref.histogram(h, i, u, L, cg, 64, 64, 0), pop_size=N)
    assert got.core_clamped == 0 and got.core_span == got.core_d_max + 1 and got.joint[-1].any()


def test_two_bands_equal_one(pa):
    """N = 300, L = 1100, G = 130 with the band forced to 256 rows: 256 + 44 rows, the 256-individual tile and the 128-row
    accessory pad crossed (Npad = 384), three 512-site pack tiles, diagonal tiles skipped in the second band"""
    rng = np.random.default_rng(2)
    N, L, G, cg = 300, 1100, 130, 7
    core, acc = _handles(pa, N, L, G, cg, _onehot(rng, N, L), (rng.random((N, G)) < 0.3).astype(np.uint8))
    nums = _numerators(core, acc)
    one = {span: core.distance_histogram(acc, 50, 30, core_span=span) for span in (0, 700)}
    core.set_tuning("core_davg_band", 256)
    for span in (0, 700):                                # (the automatic span over two bands: the contraction runs twice)
        two = core.distance_histogram(acc, 50, 30, core_span=span)
        want = ref.histogram(*nums, L, cg, 50, 30, span)
        ref.assert_equal(two, want, pop_size=N)
        ref.assert_equal(one[span], want, pop_size=N)
    core.close()
    acc.close()


def test_arbitrary_bytes_and_undefined_pairs(pa):
    """N = 70, L = 130: the generic count form with odd h; empty accessory rows and no core genes: undefined pairs"""
    rng = np.random.default_rng(3)
    N, L, G = 70, 130, 40
    M = rng.integers(0, 256, (N, L), dtype=np.uint8)
    A = (rng.random((N, G)) < 0.2).astype(np.uint8)
    A[[3, 17, 18, 40, 69]] = 0
    core, acc = _handles(pa, N, L, G, 0, M, A)
    h, i, u = _numerators(core, acc)
    assert (h & 1).any()
    for span in (0, 200):
        got = core.distance_histogram(acc, 16, 16, core_span=span)
        ref.assert_equal(got, ref.histogram(h, i, u, L, 0, 16, 16, span), pop_size=N)
        assert got.undefined_pairs == int((u == 0).sum()) >= 10
    core.close()
    acc.close()


def test_one_pair_and_no_accessory_genes(pa):
    rng = np.random.default_rng(4)
    core, acc = _handles(pa, 2, 50, 9, 1, _onehot(rng, 2, 50), np.array([[1, 0, 1, 1, 0, 0, 0, 1, 0], [1, 1, 0, 1, 0, 0, 0, 0, 0]], np.uint8))
    got = core.distance_histogram(acc, 8, 8)
    ref.assert_equal(got, _want(core, acc, 50, 1, 8, 8), pop_size=2)
    assert got.pairs == 1 and int(got.joint.sum()) == 1
    core.close()
    acc.close()
    # G = 0 is valid: I = U = 0 for every pair -- distance 0 with core genes, undefined without
    N, L = 130, 200
    M = _onehot(rng, N, L)
    for cg in (3, 0):
        core, acc = _handles(pa, N, L, 0, cg, M, None)
        got = core.distance_histogram(acc, 10, 10)
        ref.assert_equal(got, _want(core, acc, L, cg, 10, 10), pop_size=N)
        assert got.undefined_pairs == (0 if cg else got.pairs) and int(got.joint[:, 1:].sum()) == 0
        core.close()
        acc.close()


def test_handle_checks(pa):
    rng = np.random.default_rng(6)
    core, acc = _handles(pa, 20, 64, 10, 2, _onehot(rng, 20, 64), (rng.random((20, 10)) < 0.5).astype(np.uint8))
    for a, b in ((core, core), (acc, acc), (acc, core)):
        with pytest.raises(pa.PansimError) as e:
            a.distance_histogram(b)
        assert e.value.code == PS_ERR_INVALID and "core handle first" in str(e.value)
    other = pa.Population(21, 10, 2, False, 0.5, 0, 2)
    with pytest.raises(pa.PansimError) as e:
        core.distance_histogram(other)
    assert e.value.code == PS_ERR_INVALID and "20 individuals" in str(e.value)
    for kw, text in ((dict(core_bins=0), ">= 1"), (dict(acc_bins=0), ">= 1"), (dict(core_bins=129, acc_bins=128), "16384")):
        with pytest.raises(pa.PansimError) as e:
            core.distance_histogram(acc, **kw)
        assert e.value.code == PS_ERR_INVALID and text in str(e.value)
    lone_c, lone_a = pa.Population(1, 64, 4, True, 0.0, 0, 0), pa.Population(1, 10, 2, False, 0.5, 0, 2)
    with pytest.raises(pa.PansimError) as e:
        lone_c.distance_histogram(lone_a)
    assert e.value.code == PS_ERR_INVALID and "pop_size >= 2" in str(e.value)
    shard = pa.Population(20, 32, 4, True, 0.0, 0, 0, col_offset=32, global_cols=64)
    with pytest.raises(pa.PansimError) as e:
        shard.distance_histogram(acc)
    assert e.value.code == PS_ERR_INVALID and "ps_multi_distance_histogram" in str(e.value)
    with pytest.raises(pa.PansimError):
        pa.Population(20, 64, 4, True, 0.0, 0, 0).distance_histogram_timing()      # nothing to report yet
    for p in (core, acc, other, lone_c, lone_a, shard):
        p.close()


SIM = dict(pop_size=300, core_size=1100, pan_genes=150, core_genes=20, HR_rate=0.5, HGT_rate=0.5, prop_positive=0.3, seed=11,
           n_gen=8, max_distances=100)


def _sim_want(sim, Bc, Ba, span=0):
    p = sim.params
    return ref.histogram(*_numerators(sim.core_genome, sim.pan_genome), p.core_size, p.core_genes, Bc, Ba, span)


@pytest.fixture(scope="module")
def sim_after_six(pa):
    """the unsharded run after 6 generations: its histograms (automatic and fixed span) and the reference's"""
    sim = pa.Simulation(pa.make_params(**SIM))
    gen0 = sim.distance_histogram(40, 40, core_span=1100)
    sim.run(6)                                          # (the default two-generation sweep)
    got = {span: sim.distance_histogram(40, 40, core_span=span) for span in (0, 1100)}       # no sync: ordered behind the run
    want = {span: _sim_want(sim, 40, 40, span) for span in (0, 1100)}
    diversity = sim.core_genome.core_diversity()
    sim.run(2)
    state = (sim.core_genome.read_matrix(), sim.pan_genome.read_matrix(), sim.last_parents())
    sim.close()
    return gen0, got, want, diversity, state


def test_simulation_generation_zero_is_one_bin(pa, sim_after_six):
    gen0 = sim_after_six[0]
    pairs = 300 * 299 // 2
    assert gen0.pairs == pairs and gen0.undefined_pairs == 0 and gen0.core_d_max == 0 and gen0.core_d_sqsum == 0
    assert int(gen0.joint[0, 0]) == pairs and int(gen0.joint.sum()) == pairs          # every pair in one bin


def test_simulation_after_six_generations(pa, sim_after_six):
    _, got, want, diversity, state = sim_after_six
    for span in (0, 1100):
        ref.assert_equal(got[span], want[span], pop_size=300)
    assert got[0].core_d_max > 0 and got[0].core_d_sum == diversity["pair_differences"]
    assert int(got[0].joint.sum()) == got[0].pairs - got[0].undefined_pairs
    # the call changes no state: the run that asked continues bit for bit with one that never did
    plain = pa.Simulation(pa.make_params(**SIM))
    plain.run(6)
    plain.run(2)
    assert np.array_equal(plain.core_genome.read_matrix(), state[0]) and np.array_equal(plain.pan_genome.read_matrix(), state[1])
    assert np.array_equal(plain.last_parents(), state[2])
    plain.close()


@pytest.mark.parametrize("shards,band", [(2, 0), (3, 0), (3, 256)])
def test_multi_simulation_equals_the_unsharded_run(pa, sim_after_six, shards, band):
    """L = 1100 over 3 shards: unequal widths; band 256: two bands, the shards' counts added per band"""
    _, _, want, _, _ = sim_after_six
    multi = pa.MultiSimulation(pa.make_params(**SIM), shards, devices=[0] * shards)
    multi.run(6)
    if band:
        multi.shards[0].core_genome.set_tuning("core_davg_band", band)
    for span in (0, 1100):
        ref.assert_equal(multi.distance_histogram(40, 40, core_span=span), want[span], pop_size=300)
    with pytest.raises(pa.PansimError) as e:             # a site shard on its own
        multi.shards[1].distance_histogram(40, 40)
    assert e.value.code == PS_ERR_INVALID and "ps_multi_distance_histogram" in str(e.value)
    multi.close()


CLI = dict(pop_size=100, core_size=300, pan_genes=600, core_genes=200, n_gen=4, seed=9, max_distances=500, HR_rate=0.5)
USUAL = (".tsv", "_freqs.txt", "_core_genome.csv", "_pangenome.csv", "_per_gen.tsv", "_selection.tsv")


@pytest.fixture(scope="module")
def cli_want(pa):
    """what the API gives for the command line's run, formatted as the two files"""
    sim = pa.Simulation(pa.make_params(**CLI))
    sim.run(4)
    h = sim.distance_histogram(16, 8)
    ref.assert_equal(h, _sim_want(sim, 16, 8), pop_size=100)
    sim.close()
    bins = "".join("%d\t%d\t%d\n" % (c, a, h.joint[c, a]) for c in range(16) for a in range(8) if h.joint[c, a])
    names = ("pop_size", "pairs", "core_sites", "core_genes", "core_bins", "acc_bins", "core_span", "undefined_pairs", "core_clamped",
             "core_d_min", "core_d_max", "core_d_sum", "core_d_sqsum")
    summary = "".join("%s\t%d\n" % (n, getattr(h, n)) for n in names) + "mean_core_distance\t%s\n" % pa.fmt_f64(h.mean_core_distance)
    return bins, summary


def _cli(*args):
    r = subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("mode", ["plain", "gpus2", "load_state"])
def test_cli_print_dist_hist(pa, cli_want, tmp_path, mode):
    base = [x for k, v in CLI.items() for x in ("--" + k, v)] + ["--print_dist", "--print_matrices", "--print_selection"]
    hist = ["--print_dist_hist", "--dist_hist_bins", "16,8"]
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
    _cli(*base, *hist, "--outpref", tmp_path / "yes")
    for suffix in USUAL:
        assert filecmp.cmp(str(tmp_path / "no") + suffix, str(tmp_path / "yes") + suffix, shallow=False), suffix
    extra = {"half.state"} if mode == "load_state" else set()
    assert set(os.listdir(tmp_path)) == {"no" + s for s in USUAL} | {"yes" + s for s in USUAL + ("_dist_hist.tsv", "_dist_hist_summary.tsv")} | extra
    assert (tmp_path / "yes_dist_hist.tsv").read_text() == cli_want[0]
    assert (tmp_path / "yes_dist_hist_summary.tsv").read_text() == cli_want[1]
