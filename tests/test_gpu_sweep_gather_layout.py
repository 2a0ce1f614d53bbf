"""The wave sweep's transposed gather (core_kernels.h: ps_gather_child -- lane l gathers the child dwords
l + 64 m, stores them with four 4-byte LDS stores, and the chunk owner reads its 16 cells back for the symbol-decided
mutations), bit for bit against the CPU oracle (tests/orc_sim.py) at 4096 sites and the population sizes where the mapping
can go wrong: the last chunk partly valid (1000), N = pitch with no padding byte inside the row (1024), lanes without a chunk
and dwords past the row (203, 77), a row of one lane group (64) and a row inside one lane's dwords (5).  Runs of 1, 2 and 3
generations at two generations per launch and at one, HR on and off, the plan of the default workload (k = 1, R = 1) and a
k = 0 plan, a shard that starts at an odd site, parents where one has most children, unsorted parents, and full queues (the
redo path reads the rows the new stores wrote)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAVE = 1                  # ps_last_sweep_form
COUNTS = (1, 2, 3)        # generations per run
L = 4096


def _sim(pa, T, seed, n_gen, kw, tune=None, **shard):
    sim = pa.Simulation(pa.make_params(seed=seed, n_gen=n_gen, max_distances=200, **kw, **shard))
    sim.core_genome.set_tuning("sweep_generations", T)
    for k, v in (tune or {}).items():
        sim.core_genome.set_tuning(k, v)
    return sim


def _kw(N, sites, core_mu, hr):
    return dict(pop_size=N, core_size=sites, pan_genes=500, core_genes=100, core_mu=core_mu, HR_rate=hr, HGT_rate=0.05)


def _oracle_states(kw, plan_kr, sites=None, seed=5):
    # the reference, computed once per case: (parents, core, accessory) after every run of COUNTS
    from orc_sim import OracleSim
    ref = OracleSim(seed=seed, **kw) if sites is None else OracleSim(seed=seed, site_begin=sites[0], site_end=sites[1], **kw)
    assert (ref.plan.k, ref.plan.R) == plan_kr
    out, g = [], 0
    for c in COUNTS:
        for _ in range(c):
            ref.generation(g)
            g += 1
        out.append((ref.last_idx.copy(), ref.core.copy(), ref.acc.copy()))
    return out


def _check(pa, kw, want, T, tune=None, shard=None, sites=None, seed=5):
    sim = _sim(pa, T, seed, sum(COUNTS), kw, tune, **(shard or {}))
    if sites is not None:
        assert sim.core_genome.ncols == sites[1] - sites[0] and sites[0] % 2 == 1
    g = 0
    for c, (parents, core, acc) in zip(COUNTS, want):
        sim.run(c)
        sim.sync()
        g += c
        assert sim.core_genome.last_sweep_form() == WAVE
        assert np.array_equal(sim.last_parents(), parents), "parents after generation %d (T = %d)" % (g - 1, T)
        assert np.array_equal(sim.core_genome.read_matrix(), core), "core matrix after generation %d (T = %d)" % (g - 1, T)
        assert np.array_equal(sim.pan_genome.read_matrix(), acc), "accessory matrix after generation %d (T = %d)" % (g - 1, T)
    sim.close()


@pytest.mark.parametrize("hr", [0.0, 0.05])
@pytest.mark.parametrize("core_mu,plan_kr", [(0.05, (1, 1)), (0.01, (0, 1))])
@pytest.mark.parametrize("N", [1000, 1024, 203, 77, 64, 5])
def test_wave_sweep_matches_oracle(pa, orc, N, core_mu, plan_kr, hr):
    # core_mu 0.05 at 4096 sites is the plan of the default workload (decided symbols: the chunk owner's read-modify-write of
    # the gathered row); core_mu 0.01 has no decided symbol
    kw = _kw(N, L, core_mu, hr)
    want = _oracle_states(kw, plan_kr)
    _check(pa, kw, want, 2)
    _check(pa, kw, want, 1)
    if N > 5:
        assert (want[-1][1] != want[-1][1][:1]).any()            # the clonal start has diverged: the mutations did fire


@pytest.mark.parametrize("hr", [0.0, 0.05])
def test_shard_that_starts_at_an_odd_site(pa, orc, hr):
    kw = _kw(203, 6003, 0.05, hr)
    shard, sites = dict(shard_rank=1, shard_count=3), (2001, 4002)
    want = _oracle_states(kw, (1, 1), sites)
    _check(pa, kw, want, 2, shard=shard, sites=sites)
    _check(pa, kw, want, 1, shard=shard, sites=sites)


@pytest.mark.parametrize("hr", [0.0, 0.05])
def test_full_queues_redo_the_batch_on_the_new_rows(pa, orc, hr):
    # `sweep_queue_cap` 1: every batch with two residual cells is redone queue-free, reading the LDS rows as the four
    # 4-byte stores and the owner's write-back left them
    kw = _kw(1000, L, 0.05, hr)
    want = _oracle_states(kw, (1, 1))
    _check(pa, kw, want, 2, tune={"sweep_queue_cap": 1})
    _check(pa, kw, want, 1, tune={"sweep_queue_cap": 1})


def _step_against_oracle(pa, orc, N, sample, hr):
    sites, LG, seed, gen, off = 1203, L, 31, 4, 1001
    rng = np.random.default_rng(N)
    m0 = (1 << rng.integers(0, 4, (N, sites))).astype(np.uint8)
    lm, lh = 0.05 * LG, hr * 0.05 * LG
    plan = orc.core_plan(lm, lh, LG)
    assert (plan.k, plan.R) == (1, 1)
    want = orc.next_generation(m0, sample)
    orc.mutate_core(want, off, seed, gen, plan)
    if hr > 0.0:
        orc.recombine_core(want, off, seed, gen, plan)
    pop = pa.Population(N, sites, 4, True, 0.0, seed, 0, col_offset=off, global_cols=LG)
    pop.set_rates([lm], [lh])
    pop.load_matrix(m0)
    pop.step(gen, sample, hr > 0.0)
    assert pop.last_sweep_form() == WAVE
    assert np.array_equal(pop.read_matrix(), want)
    assert (want != m0[sample]).any()
    pop.close()


@pytest.mark.parametrize("hr", [0.0, 0.05])
@pytest.mark.parametrize("N", [1000, 203])
def test_one_parent_with_most_children(pa, orc, N, hr):
    # strong selection: nine children in ten are parent 7's, so the lanes of a gather instruction read one dword over long
    # stretches of the row and all of it at the row's ends
    rng = np.random.default_rng(N + 1)
    sample = np.where(rng.random(N) < 0.9, 7, rng.integers(0, N, N))
    sample = np.sort(sample).astype(np.uint32)
    assert np.bincount(sample).max() > 0.85 * N
    _step_against_oracle(pa, orc, N, sample, hr)


@pytest.mark.parametrize("hr", [0.0, 0.05])
@pytest.mark.parametrize("N", [1000, 77])
def test_unsorted_parents_change_nothing_but_speed(pa, orc, N, hr):
    sample = np.random.default_rng(N + 2).integers(0, N, N).astype(np.uint32)
    assert (np.diff(sample.astype(np.int64)) < 0).any()
    _step_against_oracle(pa, orc, N, sample, hr)
