"""Per-site rate weights on the GPU: every kernel form bit for bit against tests/site_weights_ref.py, the
0/1-mask path against ps_set_rates and the existing oracle, shards against the whole, the loop against the calls."""
import numpy as np
import pytest

import site_weights_ref as ref

pytestmark = pytest.mark.gpu

WAVE, WINDOW, BLOCK, INLINE = 1, 3, 4, 5


def _rand_core(rng, N, L):
    return (1 << rng.integers(0, 4, (N, L))).astype(np.uint8)


def _core_weights(LG, hot):
    w = (1.0 + 0.9 * np.sin(np.arange(LG) / 11.0)).astype(np.float32)
    w[::13] = 0.0
    if hot:
        w[5::97] = 400.0          # spikes: the envelope of the event mass is far above the mean
    return w


CORE_FORMS = [
    # N, L (not a multiple of 4), offset, L global, lam_mut, lam_hr, hot, tuning, form of the fused step
    (300, 203, 1001, 5000, 150.0, 60.0, False, {}, WAVE),
    (1000, 81, 0, 2000, 60.0, 0.0, False, {}, WAVE),
    (300, 203, 1001, 5000, 150.0, 60.0, True, {}, INLINE),            # R > 8: no queued sweep takes the plan
    (300, 203, 1001, 5000, 150.0, 60.0, False, {"force_block_sweep": 1}, BLOCK),
    (1500, 150, 102, 3000, 100.0, 40.0, False, {}, BLOCK),
    (1500, 150, 102, 3000, 100.0, 40.0, True, {}, INLINE),
    (5000, 61, 7, 60000, 2000.0, 900.0, False, {"force_inline_sweep": 1}, INLINE),
    (3000, 33, 11, 40000, 1500.0, 800.0, False, {"sorted": 1}, WINDOW),
    (3000, 33, 11, 40000, 1500.0, 0.0, False, {"sorted": 1, "sweep_queue_cap": 8}, WINDOW),
]


@pytest.mark.parametrize("N,L,off,LG,lm,lh,hot,tune,form", CORE_FORMS)
def test_core_sweep_forms_match_the_restatement(pa, N, L, off, LG, lm, lh, hot, tune, form):
    rng = np.random.default_rng(N + L)
    w = _core_weights(LG, hot)
    R, cshift, T = ref.core_tables([lm], [lh], w)
    assert (R > 8) == hot and R > 0
    Tl = T[off:off + L]
    seed, gen = 987654321012, 5
    m0 = _rand_core(rng, N, L)
    pop = pa.Population(N, L, 4, True, 0.0, seed, 0, col_offset=off, global_cols=LG)
    tune = dict(tune)
    ascending = tune.pop("sorted", 0)
    for k, v in tune.items():
        pop.set_tuning(k, v)
    pop.set_site_rates([lm], [lh], w)
    pop.load_matrix(m0)
    pop.mutate_alleles(gen)
    want = ref.core_mutate(m0.copy(), off, seed, gen, R, Tl)
    got = pop.read_matrix()
    assert np.array_equal(got, want)
    assert (got != m0).any() and not (got != m0)[:, w[off:off + L] == 0].any()
    pop.recombine(gen)
    ref.core_recombine(want, off, seed, gen, R, Tl)
    assert np.array_equal(pop.read_matrix(), want)
    sample = rng.integers(0, N, N).astype(np.uint32)
    if ascending:
        sample = np.sort(sample)
    for g, rec in ((gen + 1, True), (gen + 2, False)):
        pop.load_matrix(m0)
        pop.step(g, sample, rec)
        assert pop.last_sweep_form() == form
        x = np.ascontiguousarray(m0[sample])
        ref.core_mutate(x, off, seed, g, R, Tl)
        if rec and lh > 0:
            ref.core_recombine(x, off, seed, g, R, Tl)
        assert np.array_equal(pop.read_matrix(), x), "generation %d" % g
    pop.close()


def test_core_column_shards_equal_the_whole_matrix(pa):
    N, LG, lm, lh, seed = 200, 1003, 80.0, 30.0, 77
    rng = np.random.default_rng(1)
    w = np.stack([_core_weights(LG, False), rng.random(LG).astype(np.float32)])
    m0 = _rand_core(rng, N, LG)
    sample = rng.integers(0, N, N).astype(np.uint32)
    whole = pa.Population(N, LG, 4, True, 0.0, seed, 0)
    whole.set_site_rates([lm, 10.0], [lh, 5.0], w)           # two core compartments: the HR rates add
    whole.load_matrix(m0)
    whole.step(3, sample, True)
    full = whole.read_matrix()
    whole.close()
    R, _, T = ref.core_tables([lm, 10.0], [lh, 5.0], w)
    x = np.ascontiguousarray(m0[sample])
    ref.core_recombine(ref.core_mutate(x, 0, seed, 3, R, T), 0, seed, 3, R, T)
    assert np.array_equal(full, x)
    cut = 501                                                # inside a 4-site group
    for lo, hi in ((0, cut), (cut, LG)):
        sh = pa.Population(N, hi - lo, 4, True, 0.0, seed, 0, col_offset=lo, global_cols=LG)
        sh.set_site_rates([lm, 10.0], [lh, 5.0], w)
        sh.load_matrix(np.ascontiguousarray(m0[:, lo:hi]))
        sh.step(3, sample, True)
        assert np.array_equal(sh.read_matrix(), full[:, lo:hi])
        sh.close()


def test_core_cfg2_sized_case_on_sampled_columns(pa):
    # the default workload's shape; the restatement is evaluated on 3000 of the 1.2 M columns (a cell depends on its own
    # column only), the rest is checked through the columns of weight 0
    N, L, seed, gen = 1000, 1200000, 0, 9
    w = (1.0 + 0.5 * np.sin(np.arange(L) / 5000.0)).astype(np.float32)
    w[::1000] = 0.0
    lm, lh = 0.05 * L, 0.05 * L
    R, _, T = ref.core_tables([lm], [lh], w)
    rng = np.random.default_rng(2)
    cv = (1 << rng.integers(0, 4, L)).astype(np.uint8)
    pop = pa.Population(N, L, 4, True, 0.0, seed, 0, init_vec=cv)
    pop.set_site_rates([lm], [lh], w)
    sample = rng.integers(0, N, N).astype(np.uint32)
    pop.step(gen, sample, False)
    assert pop.last_sweep_form() == WAVE
    got = pop.read_matrix()
    cols = np.unique(np.concatenate([np.arange(0, 1000), np.arange(L - 1000, L), rng.integers(0, L, 1000)]))
    x = np.ascontiguousarray(np.tile(cv, (N, 1))[:, cols])
    sub = np.ascontiguousarray(x)
    rs, ri, mut, _, _ = ref._core_events(N, cols, seed, gen, R, T[cols])
    sub[ri[mut > 0], rs[mut > 0]] = mut[mut > 0]
    assert np.array_equal(got[:, cols], sub)
    assert (got[:, ::1000] == cv[::1000]).all()
    pop.close()


def _acc_case(rng, N, G):
    m0 = (rng.random((N, G)) < 0.3).astype(np.uint8)
    wm = rng.random((3, G)).astype(np.float32)
    wm[1, : G // 2] = 0.0                                    # overlapping compartments: rates add
    wr = (rng.random((3, G)) + 0.05).astype(np.float32)
    wr[0, ::3] = 0.0
    wr[2, G // 3:] = 0.0
    m0[0, :] = 0                                             # a donor with no genes at all
    m0[1, : G // 3] = 0                                      # a donor with no qualifying gene in compartment 2
    m0[2, :] = 0
    m0[2, ::3] = 1                                           # ... and one whose genes all have weight 0 in compartment 0
    return m0, wm, wr


@pytest.mark.parametrize("N,G", [(70, 129), (200, 1000)])
def test_accessory_operators_match_the_restatement(pa, orc, N, G):
    rng = np.random.default_rng(G)
    m0, wm, wr = _acc_case(rng, N, G)
    lam_mut, lam_rec = [3.0, 1.0, 0.5], [40.0, 0.0, 25.0]
    flip, wq = ref.acc_tables(lam_mut, wm, wr)
    seed, gen = 4242, 6
    pop = pa.Population(N, G, 2, False, 0.3, seed, 10)
    pop.set_site_rates(lam_mut, lam_rec, wm, wr)
    pop.load_matrix(m0)
    pop.mutate_alleles(gen)
    want = ref.acc_mutate(m0.copy(), seed, gen, flip)
    assert np.array_equal(pop.read_matrix(), want) and (want != m0).any()
    pop.recombine(gen)
    want2 = want.copy()
    assert ref.acc_hgt(want2, seed, gen, lam_rec, wq, orc.poisson_table) > 0
    assert np.array_equal(pop.read_matrix(), want2) and (want2 != want).any()
    # light and binned forms, donor lists in LDS and in global scratch, several recipient partitions
    row_bytes = 8 * ((G + 63) // 64)
    for tune in ({"hgt_mode": 1}, {"hgt_mode": 1, "hgt_list_in_global": 1}, {"hgt_mode": 2},
                 {"hgt_mode": 2, "hgt_bin_list_in_global": 1},
                 {"hgt_mode": 2, "lds_limit": min(160 * 1024, max(1024 + 21 * row_bytes, 6 * G + 8192))},
                 {"hgt_mode": 2, "hgt_bin_cap": 3}):
        alt = pa.Population(N, G, 2, False, 0.3, seed, 10)
        for k, v in tune.items():
            alt.set_tuning(k, v)
        alt.set_site_rates(lam_mut, lam_rec, wm, wr)
        alt.load_matrix(want)
        alt.recombine(gen)
        assert np.array_equal(alt.read_matrix(), want2), tune
        alt.close()
    # donor shards: every shard's own events are the restatement's for its donors, and their union is the unsharded result
    for K in (2, 3):
        union = want.copy()
        for mode in (1, 2):
            for r in range(K):
                sh = pa.Population(N, G, 2, False, 0.3, seed, 10)
                sh.set_tuning("hgt_mode", mode)
                sh.set_site_rates(lam_mut, lam_rec, wm, wr)
                sh.set_donor_shard(r, K)
                sh.load_matrix(want)
                sh.recombine(gen)
                own = want.copy()
                ref.acc_hgt(own, seed, gen, lam_rec, wq, orc.poisson_table, donors=range(N * r // K, N * (r + 1) // K))
                got = sh.read_matrix()
                assert np.array_equal(got, own), (K, mode, r)
                union |= got
                sh.close()
        assert np.array_equal(union, want2)
    # fused step = the calls in order
    sample = rng.integers(0, N, N).astype(np.uint32)
    pop.load_matrix(m0)
    pop.step(gen + 1, sample, True)
    x = ref.acc_mutate(np.ascontiguousarray(m0[sample]), seed, gen + 1, flip)
    ref.acc_hgt(x, seed, gen + 1, lam_rec, wq, orc.poisson_table)
    assert np.array_equal(pop.read_matrix(), x)
    pop.close()


def test_contiguous_masks_equal_set_rates_and_the_oracle(pa, orc):
    rng = np.random.default_rng(9)
    N, L, LG, off, lm, lh, seed, gen = 300, 200, 4000, 1000, 2000.0, 500.0, 31, 4
    m0 = _rand_core(rng, N, L)
    sample = rng.integers(0, N, N).astype(np.uint32)
    outs = []
    for weighted in (False, True):
        pop = pa.Population(N, L, 4, True, 0.0, seed, 0, col_offset=off, global_cols=LG)
        if weighted:
            pop.set_site_rates([lm], [lh], np.ones(LG, np.float32))
        else:
            pop.set_rates([lm], [lh])
        pop.load_matrix(m0)
        pop.step(gen, sample, True)
        outs.append(pop.read_matrix())
        pop.close()
    plan = orc.core_plan(lm, lh, LG)
    x = orc.next_generation(m0, sample)
    orc.recombine_core(orc.mutate_core(x, off, seed, gen, plan), off, seed, gen, plan)
    assert np.array_equal(outs[0], x) and np.array_equal(outs[1], x)
    G, cb, ce, lam_mut, lam_rec = 300, [0, 100], [100, 300], [2.0, 5.0], [30.0, 10.0]
    a0 = (rng.random((N, G)) < 0.3).astype(np.uint8)
    mask = np.zeros((2, G), np.float32)
    mask[0, :100] = 1
    mask[1, 100:] = 1
    outs = []
    for weighted in (False, True):
        pop = pa.Population(N, G, 2, False, 0.3, seed, 10)
        if weighted:
            pop.set_site_rates(lam_mut, lam_rec, mask, mask)
        else:
            pop.set_rates(lam_mut, lam_rec, cb, ce)
        pop.load_matrix(a0)
        pop.step(gen, sample, True)
        outs.append(pop.read_matrix())
        pop.close()
    x = orc.next_generation(a0, sample)
    orc.mutate_acc(x, seed, gen, cb, ce, lam_mut)
    orc.recombine_acc(x, seed, gen, cb, ce, lam_rec)
    assert np.array_equal(outs[0], x) and np.array_equal(outs[1], x)


def test_switching_back_to_set_rates_restores_the_old_bits(pa, orc):
    rng = np.random.default_rng(10)
    N, L, lm, lh, seed = 500, 300, 30.0, 10.0, 3
    m0 = _rand_core(rng, N, L)
    pop = pa.Population(N, L, 4, True, 0.0, seed, 0)
    pop.set_site_rates([lm], [lh], _core_weights(L, True))
    pop.load_matrix(m0)
    pop.mutate_alleles(1)
    pop.set_rates([lm], [lh])
    pop.load_matrix(m0)
    pop.mutate_alleles(1)
    pop.recombine(1)
    plan = orc.core_plan(lm, lh, L)
    x = orc.recombine_core(orc.mutate_core(m0.copy(), 0, seed, 1, plan), 0, seed, 1, plan)
    assert np.array_equal(pop.read_matrix(), x)
    pop.close()
    G = 200
    a0 = (rng.random((N, G)) < 0.3).astype(np.uint8)
    acc = pa.Population(N, G, 2, False, 0.3, seed, 10)
    w = rng.random((1, G)).astype(np.float32)
    acc.set_site_rates([2.0], [20.0], w, w)
    acc.load_matrix(a0)
    acc.mutate_alleles(1)
    acc.recombine(1)
    acc.set_rates([2.0], [20.0], [0], [G])
    acc.load_matrix(a0)
    acc.mutate_alleles(1)
    acc.recombine(1)
    x = orc.mutate_acc(a0.copy(), seed, 1, [0], [G], [2.0])
    orc.recombine_acc(x, seed, 1, [0], [G], [20.0])
    assert np.array_equal(acc.read_matrix(), x)
    acc.close()


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


@pytest.mark.parametrize("N", [100, 1500])
def test_sim_run_with_weights_equals_the_calls_through_population(pa, N):
    kw = dict(pop_size=N, core_size=2000, pan_genes=600, core_genes=200, HR_rate=0.05, HGT_rate=0.05)
    sim = pa.Simulation(pa.make_params(seed=5, n_gen=6, max_distances=10, device=0, **kw))
    p, d = sim.params, sim.derived
    wc, wm, wr = _sim_weights(p, d)
    sim.set_site_weights(wc, wm, wr)
    L, G = p.core_size, d.pan_size
    core = pa.Population(N, L, 4, True, 0.0, p.seed, p.core_genes, init_vec=sim.core_genome.read_matrix()[0])
    acc = pa.Population(N, G, 2, False, 0.0, p.seed, p.core_genes, init_vec=sim.pan_genome.read_matrix()[0])
    core.set_site_rates([d.n_core_mutations], [d.n_recombinations_core], wc)
    acc.set_site_rates([d.n_pan_mutations[c] for c in range(d.n_comp)], [d.n_recombinations_pan[c] for c in range(d.n_comp)], wm, wr)
    sigma = np.arange(N)                        # output row -> internal row
    for g in range(6):
        sim.run(1)
        sim.sync()
        draw = sigma[sim.last_parents()].astype(np.uint32)      # parents by internal row
        order = np.argsort(draw, kind="stable")
        idx = np.ascontiguousarray(draw[order])
        sigma = np.empty(N, np.int64)
        sigma[order] = np.arange(N)
        core.step(g, idx, True)
        acc.step(g, idx, True)
        assert np.array_equal(sim.core_genome.read_matrix(), core.read_matrix()[sigma]), g
        assert np.array_equal(sim.pan_genome.read_matrix(), acc.read_matrix()[sigma]), g
    core.close()
    acc.close()
    sim.close()


def test_columns_of_weight_zero_never_change(pa):
    kw = dict(pop_size=200, core_size=3000, pan_genes=600, core_genes=200, HGT_rate=0.05)      # no HR: a core column only mutates
    sim = pa.Simulation(pa.make_params(seed=1, n_gen=50, max_distances=10, device=0, **kw))
    p, d = sim.params, sim.derived
    wc, wm, wr = _sim_weights(p, d)
    wr[:, ::5] = 0.0                            # genes that neither flip nor transfer
    sim.set_site_weights(wc, wm, wr)
    c0, a0 = sim.core_genome.read_matrix(), sim.pan_genome.read_matrix()
    sim.run(50)
    sim.sync()
    c1, a1 = sim.core_genome.read_matrix(), sim.pan_genome.read_matrix()
    # (rows are clonal at the start, so a parent gather moves no value in a column that never changed)
    assert (c1[:, ::7] == c0[:, ::7]).all() and (c1 != c0).any()
    assert (a1[:, ::5] == a0[:, ::5]).all() and (a1 != a0).any()
    sim.close()


def test_multi_runs_say_that_weights_are_not_plumbed(pa):
    from pansim_amd import _lib
    lib = pa.load()
    assert lib.ps_multi_set_site_weights(None, None, None, None) == _lib.PS_ERR_INVALID
    assert b"ps_sim_set_site_weights" in lib.ps_last_error()
