"""Two generations per launch of the wave sweep: ps_sim_run applies generations g and g + 1 to a
wave's rows between one load and one store of the core matrix.  Everything here holds the two-generation launches to the
results of one-generation launches: bit for bit against the CPU oracle (tests/orc_sim.py) and against the same run with
`sweep_generations` 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAVE = 1     # ps_last_sweep_form: the wave-per-row sweep


def _sim(pa, T, seed, n_gen, kw, extra=None, P=200, tune=None, **shard):
    sim = pa.Simulation(pa.make_params(seed=seed, n_gen=n_gen, max_distances=P, **kw, **(extra or {}), **shard))
    if T is not None:
        sim.core_genome.set_tuning("sweep_generations", T)
    for k, v in (tune or {}).items():
        sim.core_genome.set_tuning(k, v)
    return sim


def _launches(sim, count):
    sim.enable_timing(True)
    sim.sweep_timing(reset=True)
    sim.run(count)
    sim.sync()
    n, _ms, b = sim.sweep_timing(reset=True)
    sim.enable_timing(False)
    return n, b


LOOP_CASES = [
    # (simulation parameters, shard, oracle's site range)
    (dict(pop_size=1000, core_size=1500, pan_genes=500, core_genes=100, HR_rate=0.05, HGT_rate=0.05), {}, None),
    (dict(pop_size=1000, core_size=1203, pan_genes=500, core_genes=100, HR_rate=0.0, HGT_rate=0.05), {}, None),
    (dict(pop_size=77, core_size=3001, pan_genes=600, core_genes=200, HR_rate=0.5, HGT_rate=0.5), {}, None),       # N % 16 != 0
    (dict(pop_size=203, core_size=2999, pan_genes=600, core_genes=200, HR_rate=0.0, HGT_rate=0.0), {}, None),
    # a site shard that starts inside a group of 4 sites: sites [2001, 4003) of 6005
    (dict(pop_size=150, core_size=6005, pan_genes=600, core_genes=200, HR_rate=0.3), dict(shard_rank=1, shard_count=3), (2001, 4003)),
]


@pytest.mark.parametrize("start", [0, 1])
@pytest.mark.parametrize("kw,shard,sites", LOOP_CASES)
def test_two_generation_launches_match_oracle(pa, orc, kw, shard, sites, start):
    # runs of 1, 2, 3, 5 and 8 generations one after the other (blocks of two, and a single generation behind the odd
    # ones), the first one at an even or an odd generation: parents and both matrices after every run
    from orc_sim import OracleSim
    counts = (1, 2, 3, 5, 8)
    n_gen = start + sum(counts)
    sim = _sim(pa, 2, 3, n_gen, kw, **shard)
    ref = OracleSim(seed=3, **kw) if sites is None else OracleSim(seed=3, site_begin=sites[0], site_end=sites[1], **kw)
    if sites is not None:
        assert sim.core_genome.ncols == sites[1] - sites[0] and sites[0] % 4 != 0
    g = 0
    for _ in range(start):
        sim.run(1)
        ref.generation(g)
        g += 1
    for c in counts:
        n, nbytes = _launches(sim, c)
        assert n == (c + 1) // 2, "run(%d) took %d launches" % (c, n)
        assert nbytes == 2.0 * kw["pop_size"] * sim.core_genome.ncols
        for _ in range(c):
            ref.generation(g)
            g += 1
        assert sim.core_genome.last_sweep_form() == WAVE
        assert np.array_equal(sim.last_parents(), ref.last_idx), "parents after generation %d" % (g - 1)
        assert np.array_equal(sim.core_genome.read_matrix(), ref.core), "core matrix after generation %d" % (g - 1)
        assert np.array_equal(sim.pan_genome.read_matrix(), ref.acc), "accessory matrix after generation %d" % (g - 1)
    sim.close()


@pytest.mark.parametrize("kw", [
    dict(pop_size=1000, core_size=2000, pan_genes=500, core_genes=100, HR_rate=0.05, HGT_rate=0.05),
    dict(pop_size=333, core_size=2501, pan_genes=500, core_genes=100, HR_rate=0.4, HGT_rate=0.1),
])
def test_two_generation_launches_equal_single_ones_however_the_run_is_split(pa, kw):
    def state(T, splits):
        sim = _sim(pa, T, 8, 7, kw)
        for c in splits:
            sim.run(c)
        sim.sync()
        out = (sim.core_genome.read_matrix(), sim.pan_genome.read_matrix(), sim.last_parents())
        sim.close()
        return out
    want = state(1, (7,))
    for T, splits in ((2, (7,)), (2, (3, 4)), (2, (1,) * 7), (1, (3, 4)), (2, (2, 5)), (None, (7,))):
        got = state(T, splits)
        for a, b, name in zip(got, want, ("core matrix", "accessory matrix", "parents")):
            assert np.array_equal(a, b), "%s differs at sweep_generations %r, runs %r" % (name, T, splits)


def test_population_calls_between_two_runs(pa, orc):
    # ps_load_matrix and ps_step on the simulation's own handles between two runs: the next block starts from what they left
    from orc_sim import OracleSim
    kw = dict(pop_size=300, core_size=1801, pan_genes=400, core_genes=100, HR_rate=0.2, HGT_rate=0.05)
    N, L = kw["pop_size"], kw["core_size"]
    sim = _sim(pa, 2, 6, 12, kw)
    ref = OracleSim(seed=6, **kw)
    sim.run(3)
    for g in range(3):
        ref.generation(g)
    assert np.array_equal(sim.core_genome.read_matrix(), ref.core)
    rng = np.random.default_rng(17)
    core = (1 << rng.integers(0, 4, (N, L))).astype(np.uint8)
    acc = (rng.random(ref.acc.shape) < 0.4).astype(np.uint8)
    sim.core_genome.load_matrix(core)
    sim.pan_genome.load_matrix(acc)
    sample = rng.integers(0, N, N).astype(np.uint32)
    sim.core_genome.step(3, sample, True)            # one generation of the core matrix alone, through the Population API
    want = orc.next_generation(core, sample)
    orc.mutate_core(want, 0, 6, 3, ref.plan)
    orc.recombine_core(want, 0, 6, 3, ref.plan)
    assert np.array_equal(sim.core_genome.read_matrix(), want)
    ref.core = want
    ref.acc = acc
    for c in (4, 5):                                 # two blocks; then two blocks and a single generation
        first = sim.generation
        sim.run(c)
        for g in range(first, first + c):
            ref.generation(g)
        assert np.array_equal(sim.last_parents(), ref.last_idx)
        assert np.array_equal(sim.core_genome.read_matrix(), ref.core)
        assert np.array_equal(sim.pan_genome.read_matrix(), ref.acc)
    sim.close()


@pytest.mark.parametrize("hr", [0.0, 0.3])
def test_full_queues_in_both_generations_of_a_block(pa, orc, hr):
    # `sweep_queue_cap` 1: no batch with two residual cells fits its queue (a batch of 4 x 500 cells holds dozens at these
    # rates), so every batch is redone queue-free -- in the first and in the second generation of every launch
    from orc_sim import OracleSim
    kw = dict(pop_size=500, core_size=1600, pan_genes=400, core_genes=100, HR_rate=hr, HGT_rate=0.05)
    sim = _sim(pa, 2, 4, 6, kw, tune={"sweep_queue_cap": 1})
    ref = OracleSim(seed=4, **kw)
    n, _b = _launches(sim, 6)
    assert n == 3 and sim.core_genome.last_sweep_form() == WAVE
    for g in range(6):
        ref.generation(g)
    assert np.array_equal(sim.last_parents(), ref.last_idx)
    assert np.array_equal(sim.core_genome.read_matrix(), ref.core)
    assert np.array_equal(sim.pan_genome.read_matrix(), ref.acc)
    sim.close()


def test_competition_and_heavy_hgt_whichever_form_they_take(pa, orc, monkeypatch):
    # D-avg in the accessory chain, and an HGT that takes turns with the sweep: the library's own choice of generations
    # per launch (no tuning), against the oracle
    from orc_sim import OracleSim
    kw = dict(pop_size=400, core_size=1400, pan_genes=420, core_genes=120, HR_rate=0.1, HGT_rate=0.05)
    extra = dict(competition_strength=10.0, prop_positive=0.2)
    sim = _sim(pa, None, 12, 7, kw, extra)
    ref = OracleSim(seed=12, **kw, **extra)
    sim.run(7)
    for g in range(7):
        ref.generation(g)
    assert np.array_equal(sim.last_parents(), ref.last_idx)
    assert np.array_equal(sim.core_genome.read_matrix(), ref.core)
    assert np.array_equal(sim.pan_genome.read_matrix(), ref.acc)
    sim.close()
    monkeypatch.setenv("PANSIM_HEAVY_HGT", "1")          # the schedule of >= 7.5e6 events per generation, at a testable size
    monkeypatch.setenv("PANSIM_HGT_MODE", "2")
    kw = dict(pop_size=700, core_size=900, pan_genes=420, core_genes=120, HR_rate=0.5, HGT_rate=0.5)
    for T in (None, 2):
        sim = _sim(pa, T, 5, 7, kw)
        ref = OracleSim(seed=5, **kw)
        sim.run(7)
        for g in range(7):
            ref.generation(g)
        assert np.array_equal(sim.last_parents(), ref.last_idx)
        assert np.array_equal(sim.core_genome.read_matrix(), ref.core)
        assert np.array_equal(sim.pan_genome.read_matrix(), ref.acc)
        sim.close()


def _sim_weights(p, d):
    L, G = p.core_size, d.pan_size
    wc = (1.0 + 0.9 * np.cos(np.arange(L) / 17.0)).astype(np.float32)
    wc[::7] = 0.0
    rng = np.random.default_rng(4)
    wm = rng.random((d.n_comp, G)).astype(np.float32)
    wm[:, ::5] = 0.0
    wr = rng.random((d.n_comp, G)).astype(np.float32)
    wr[:, 1::4] = 0.0
    return wc, wm, wr


def test_per_site_weights_in_two_generation_launches(pa):
    # the reference of the per-site rates is the Population API (one generation per call, tests/test_gpu_site_weights.py
    # holds it to the model); a run at one generation per launch supplies every generation's parents
    N = 200
    kw = dict(pop_size=N, core_size=2003, pan_genes=600, core_genes=200, HR_rate=0.05, HGT_rate=0.05)
    one = _sim(pa, 1, 5, 5, kw, P=10)
    two = _sim(pa, 2, 5, 5, kw, P=10)
    p, d = one.params, one.derived
    wc, wm, wr = _sim_weights(p, d)
    one.set_site_weights(wc, wm, wr)
    two.set_site_weights(wc, wm, wr)
    core = pa.Population(N, p.core_size, 4, True, 0.0, p.seed, p.core_genes, init_vec=one.core_genome.read_matrix()[0])
    acc = pa.Population(N, d.pan_size, 2, False, 0.0, p.seed, p.core_genes, init_vec=one.pan_genome.read_matrix()[0])
    core.set_site_rates([d.n_core_mutations], [d.n_recombinations_core], wc)
    acc.set_site_rates([d.n_pan_mutations[c] for c in range(d.n_comp)], [d.n_recombinations_pan[c] for c in range(d.n_comp)], wm, wr)
    sigma = np.arange(N)                        # output row -> internal row
    for g in range(5):
        one.run(1)
        one.sync()
        draw = sigma[one.last_parents()].astype(np.uint32)      # parents by internal row
        order = np.argsort(draw, kind="stable")
        idx = np.ascontiguousarray(draw[order])
        sigma = np.empty(N, np.int64)
        sigma[order] = np.arange(N)
        core.step(g, idx, True)
        acc.step(g, idx, True)
    n, _b = _launches(two, 5)
    assert n == 3
    assert np.array_equal(two.last_parents(), one.last_parents())
    assert np.array_equal(two.core_genome.read_matrix(), core.read_matrix()[sigma])
    assert np.array_equal(two.pan_genome.read_matrix(), acc.read_matrix()[sigma])
    assert np.array_equal(one.core_genome.read_matrix(), core.read_matrix()[sigma])
    for x in (core, acc, one, two):
        x.close()


def test_sweep_timing_counts_launches(pa):
    # a launch moves the matrix once in and once out, however many generations it carries
    N, L = 1000, 4000
    kw = dict(pop_size=N, core_size=L, pan_genes=500, core_genes=100, HR_rate=0.05, HGT_rate=0.05)
    sim = _sim(pa, 2, 0, 16, kw)
    n, nbytes = _launches(sim, 8)
    assert n == 4 and nbytes == 2.0 * N * L
    n_host = sim.host_timing(reset=True)[0]
    assert n_host == 8                               # the host half is counted per generation
    sim.core_genome.set_tuning("sweep_generations", 1)
    n, nbytes = _launches(sim, 8)
    assert n == 8 and nbytes == 2.0 * N * L
    sim.close()


def test_wide_populations_keep_one_generation_per_launch(pa):
    # N > 1024: the window sweep's segments depend on each other across a generation
    kw = dict(pop_size=1500, core_size=600, pan_genes=300, core_genes=100)
    sim = _sim(pa, 2, 0, 4, kw)
    n, _b = _launches(sim, 4)
    assert n == 4 and sim.core_genome.last_sweep_form() != WAVE
    sim.close()
