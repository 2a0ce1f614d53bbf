"""The symbol-decided mutations of the queued sweeps (ps_apply_prepare / ps_apply_dword select bytes with one
v_bitop3_b32, truth table 0xCA) and their class words (ps_classes), bit for bit against the CPU oracle (tests/orc_sim.py)
at small shapes where every path can still go wrong: the last lane partly valid (N = 1000), lanes past the row and fewer
than 64 chunks per row (N = 77, 203), a shard whose first batch of 4 sites is partial, two generations per launch and the
odd remainder through one, the plan of the default workload (k = 1, R = 1: decided symbols and residual cells) and a k = 0
plan (residual cells only), HR on and off, full queues, and the window and block sweeps, which share the apply code.

(Site shards start at core_size * rank // count, so no shard of 6000 sites starts at site 2001; the shard used here is
sites [2001, 4002) of 6003 -- the same partial first batch, 2001 % 4 = 1.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAVE, WINDOW, BLOCK = 1, 3, 4     # ps_last_sweep_form
COUNTS = (1, 2, 3, 5)             # generations per run: a single one, a block of two, blocks with an odd remainder


def _sim(pa, T, seed, n_gen, kw, tune=None, **shard):
    sim = pa.Simulation(pa.make_params(seed=seed, n_gen=n_gen, max_distances=200, **kw, **shard))
    if T is not None:
        sim.core_genome.set_tuning("sweep_generations", T)
    for k, v in (tune or {}).items():
        sim.core_genome.set_tuning(k, v)
    return sim


def _kw(N, L, core_mu, hr):
    return dict(pop_size=N, core_size=L, pan_genes=500, core_genes=100, core_mu=core_mu, HR_rate=hr, HGT_rate=0.05)


def _run_against_oracle(pa, kw, plan_kr, form, T=2, tune=None, shard=None, sites=None, seed=5):
    from orc_sim import OracleSim
    sim = _sim(pa, T, seed, sum(COUNTS), kw, tune, **(shard or {}))
    ref = OracleSim(seed=seed, **kw) if sites is None else OracleSim(seed=seed, site_begin=sites[0], site_end=sites[1], **kw)
    assert (ref.plan.k, ref.plan.R) == plan_kr
    if sites is not None:
        assert sim.core_genome.ncols == sites[1] - sites[0] and sites[0] % 4 != 0
    g = 0
    for c in COUNTS:
        sim.run(c)
        sim.sync()
        for _ in range(c):
            ref.generation(g)
            g += 1
        assert sim.core_genome.last_sweep_form() == form
        assert np.array_equal(sim.last_parents(), ref.last_idx), "parents after generation %d" % (g - 1)
        assert np.array_equal(sim.core_genome.read_matrix(), ref.core), "core matrix after generation %d" % (g - 1)
        assert np.array_equal(sim.pan_genome.read_matrix(), ref.acc), "accessory matrix after generation %d" % (g - 1)
    out = sim.core_genome.read_matrix()
    sim.close()
    return out


@pytest.mark.parametrize("hr", [0.0, 0.05])
@pytest.mark.parametrize("core_mu,plan_kr", [(0.05, (1, 1)), (0.01, (0, 1))])
@pytest.mark.parametrize("N", [1000, 77, 203])
def test_wave_sweep_matches_oracle(pa, orc, N, core_mu, plan_kr, hr):
    # core_mu 0.05 at 4096 sites is the plan of the default workload: decided symbols (three of four mutations, applied in
    # registers) and one residual symbol; core_mu 0.01 has no decided symbol, only the residual cells fire
    kw = _kw(N, 4096, core_mu, hr)
    two = _run_against_oracle(pa, kw, plan_kr, WAVE, T=2)
    one = _run_against_oracle(pa, kw, plan_kr, WAVE, T=1)
    assert np.array_equal(two, one)
    assert (two != two[:1]).any()            # the clonal start has diverged: the mutations did fire


@pytest.mark.parametrize("hr", [0.0, 0.05])
@pytest.mark.parametrize("core_mu,plan_kr", [(0.05, (1, 1)), (0.01, (0, 1))])
def test_shard_with_a_partial_first_batch(pa, orc, core_mu, plan_kr, hr):
    kw = _kw(203, 6003, core_mu, hr)
    shard, sites = dict(shard_rank=1, shard_count=3), (2001, 4002)
    two = _run_against_oracle(pa, kw, plan_kr, WAVE, T=2, shard=shard, sites=sites)
    one = _run_against_oracle(pa, kw, plan_kr, WAVE, T=1, shard=shard, sites=sites)
    assert np.array_equal(two, one)


def test_two_generations_equal_single_ones_however_the_run_is_split(pa):
    kw = _kw(1000, 4096, 0.05, 0.05)

    def state(T, splits):
        sim = _sim(pa, T, 9, 11, kw)
        for c in splits:
            sim.run(c)
        sim.sync()
        out = (sim.core_genome.read_matrix(), sim.pan_genome.read_matrix(), sim.last_parents())
        sim.close()
        return out
    want = state(1, (11,))
    for T, splits in ((2, (11,)), (2, COUNTS), (2, COUNTS[::-1]), (2, (1,) * 11), (None, (4, 7))):
        for a, b, name in zip(state(T, splits), want, ("core matrix", "accessory matrix", "parents")):
            assert np.array_equal(a, b), "%s differs at sweep_generations %r, runs %r" % (name, T, splits)


def test_full_queues_redo_the_batch(pa, orc):
    # `sweep_queue_cap` 1: every batch with two residual cells is redone queue-free, on top of the child bytes the symbols
    # have already decided
    _run_against_oracle(pa, _kw(1000, 4096, 0.05, 0.05), (1, 1), WAVE, T=2, tune={"sweep_queue_cap": 1})


def test_window_sweep_shares_the_apply_code(pa, orc):
    # N > 1024: the window sweep (one generation per launch), same ps_apply_row / ps_apply_prepare
    _run_against_oracle(pa, _kw(3000, 1024, 0.05, 0.05), (1, 1), WINDOW, T=None)


def test_block_sweep_with_unsorted_parents(pa, orc):
    # a Population-level step with parents in draw order: N > 1024 and no ascending order leaves the block sweep
    N, L, LG, seed, gen = 1500, 203, 4096, 31, 4
    rng = np.random.default_rng(N + L)
    m0 = (1 << rng.integers(0, 4, (N, L))).astype(np.uint8)
    sample = rng.integers(0, N, N).astype(np.uint32)
    assert (np.diff(sample.astype(np.int64)) < 0).any()
    for hr in (0.0, 0.05):
        lm, lh = 0.05 * LG, hr * 0.05 * LG
        plan = orc.core_plan(lm, lh, LG)
        assert (plan.k, plan.R) == (1, 1)
        want = orc.next_generation(m0, sample)
        orc.mutate_core(want, 1001, seed, gen, plan)
        if hr > 0.0:
            orc.recombine_core(want, 1001, seed, gen, plan)
        pop = pa.Population(N, L, 4, True, 0.0, seed, 0, col_offset=1001, global_cols=LG)
        pop.set_rates([lm], [lh])
        pop.load_matrix(m0)
        pop.step(gen, sample, hr > 0.0)
        assert pop.last_sweep_form() == BLOCK
        assert np.array_equal(pop.read_matrix(), want)
        assert (want != m0[sample]).any()
        pop.close()
