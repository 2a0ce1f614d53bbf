"""State files on the device (ps_sim_save / ps_sim_load, docs/STATE_FORMAT.md): a run that is saved, dropped,
loaded and continued equals the run that was never interrupted -- bit for bit, every comparison here is array_equal or byte
equality of files -- and the file is what the document says (tests/state_file_ref.py reads and writes it independently)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import state_file_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_IO, PS_ERR_STATE = -1, -5, -6


def _weights(p, d):
    L, G = p.core_size, d.pan_size
    wc = (1.0 + 0.9 * np.cos(np.arange(L) / 17.0)).astype(np.float32)
    wc[::7] = 0.0
    rng = np.random.default_rng(4)
    wm = rng.random((d.n_comp, G)).astype(np.float32)
    wm[:, ::5] = 0.0
    wr = rng.random((d.n_comp, G)).astype(np.float32)
    wr[:, 1::4] = 0.0
    return wc, wm, wr


def _setup(sim, case):
    for k, v in case.get("tune_core", {}).items():
        sim.core_genome.set_tuning(k, v)
    for k, v in case.get("tune_acc", {}).items():
        sim.pan_genome.set_tuning(k, v)
    if case.get("weights"):
        sim.set_site_weights(*_weights(sim.params, sim.derived))      # (state of the handles: applied again after a load)
    return sim


def _new(pa, case, n_gen, seed=7, P=150):
    return _setup(pa.Simulation(pa.make_params(seed=seed, n_gen=n_gen, max_distances=P, **case["kw"])), case)


def _outputs(sim):
    sim.sync()
    out = dict(parents=sim.last_parents(), core=sim.core_genome.read_matrix(), acc=sim.pan_genome.read_matrix(),
               avg_acc=sim.pan_genome.average_distance(), freqs=sim.pan_genome.gene_frequencies())
    out["core_dist"], out["acc_dist"] = sim.final_distances()
    if sim.params.shard_count == 1:          # (a site shard cannot finish the core sum: ps_average_distance refuses)
        out["avg_core"] = sim.core_genome.average_distance()
    return out


def _same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), "%s: %s differs" % (what, k)


CASES = {
    "wave": dict(kw=dict(pop_size=1000, core_size=1500, pan_genes=500, core_genes=100, HR_rate=0.05, HGT_rate=0.05)),
    "no_hr": dict(kw=dict(pop_size=1000, core_size=1203, pan_genes=500, core_genes=100, HR_rate=0.0, HGT_rate=0.05)),
    "n77": dict(kw=dict(pop_size=77, core_size=3001, pan_genes=600, core_genes=200, HR_rate=0.5, HGT_rate=0.5)),          # N % 16 != 0
    "neutral": dict(kw=dict(pop_size=203, core_size=2999, pan_genes=600, core_genes=200, HR_rate=0.0, HGT_rate=0.0)),
    # a site shard that starts inside a group of 4 sites: sites [2001, 4003) of 6005
    "shard": dict(kw=dict(pop_size=150, core_size=6005, pan_genes=600, core_genes=200, HR_rate=0.3, shard_rank=1, shard_count=3)),
    "window": dict(kw=dict(pop_size=2048, core_size=700, pan_genes=400, core_genes=100, HR_rate=0.1, HGT_rate=0.05)),   # N > 1024: window sweep
    "competition": dict(kw=dict(pop_size=400, core_size=1400, pan_genes=420, core_genes=120, HR_rate=0.1, HGT_rate=0.05,
                                competition_strength=10.0, prop_positive=0.2)),
    "binned_hgt": dict(kw=dict(pop_size=700, core_size=900, pan_genes=420, core_genes=120, HR_rate=0.5, HGT_rate=0.5), tune_acc={"hgt_mode": 2}),
    "weights": dict(kw=dict(pop_size=200, core_size=2003, pan_genes=600, core_genes=200, HR_rate=0.05, HGT_rate=0.05), weights=True),
    "ref_stream": dict(kw=dict(pop_size=300, core_size=1100, pan_genes=500, core_genes=100, prop_positive=0.3, reference_seed_stream=1)),
}


@pytest.mark.parametrize("a", [3, 4])           # odd and even: two-generation launches pair up differently on the two sides
@pytest.mark.parametrize("name", list(CASES))
def test_a_saved_run_continues_bit_for_bit(pa, orc, tmp_path, name, a):
    case, b = CASES[name], 4
    path = str(tmp_path / "run.state")
    straight = _new(pa, case, a + b)
    straight.run(a + b)
    want = _outputs(straight)
    first = _new(pa, case, a + b)
    first.run(a)
    at_a = _outputs(first)
    first.save(path)
    assert first.generations_done == a
    first.close()                                # the run is gone; the file is all that is left
    sim = _setup(pa.Simulation.load(path), case)
    assert sim.generation == a and sim.generations_done == a
    for f, _ in sim.params._fields_:
        if f != "device":
            assert getattr(sim.params, f) == getattr(straight.params, f), f
    # right after the load, before any generation: every output, sigma and its predecessor included
    _same(_outputs(sim), at_a, "right after the load")
    sim.run(b)
    _same(_outputs(sim), want, "continued run")
    assert sim.generations_done == a + b
    if name == "wave":
        # ... and the pair of runs is not wrong together
        from orc_sim import OracleSim
        kw = case["kw"]
        o = OracleSim(seed=7, **kw)
        for g in range(a + b):
            o.generation(g)
        assert np.array_equal(want["parents"], o.last_idx)
        assert np.array_equal(want["core"], o.core) and np.array_equal(want["acc"], o.acc)
    # the file is what the document says: matrices in internal order, mapped through the stored sigma, are read_matrix
    st = ref.read(path)
    assert st["generations_done"] == a and st["encoding"] == ref.PACKED2 and st["has_row_maps"]
    assert np.array_equal(ref.output_rows(st, "core"), at_a["core"]) and np.array_equal(ref.output_rows(st, "acc"), at_a["acc"])
    assert np.array_equal(st["last_parents"], at_a["parents"]) and not st["padding"].any()
    straight.close()
    sim.close()


def test_saving_does_not_perturb_the_run(pa, tmp_path):
    case = CASES["wave"]
    straight = _new(pa, case, 7)
    straight.run(7)
    sim = _new(pa, case, 7)
    sim.run(3)
    sim.save(str(tmp_path / "a.state"))
    sim.run(1)
    sim.save(str(tmp_path / "b.state"), per_gen=np.arange(16.0).reshape(4, 4))
    sim.run(3)
    _same(_outputs(sim), _outputs(straight), "run with two saves inside")
    info = pa.state_info(str(tmp_path / "b.state"), per_gen=True)
    assert info["generations_done"] == 4 and np.array_equal(info["per_gen"], np.arange(16.0).reshape(4, 4))
    with pytest.raises(ValueError):
        sim.save(str(tmp_path / "c.state"), per_gen=np.zeros((2, 4)))
    straight.close()
    sim.close()


def test_a_file_written_from_the_document_loads_and_runs_against_the_oracle(pa, orc, tmp_path):
    # N not a multiple of 16, L not a multiple of 4, garbage in the padding cells: the load must leave zeros there (the
    # sweeps gather whole 16-cell pieces: a surviving byte would show up in the next generation)
    from orc_sim import OracleSim
    kw = dict(pop_size=77, core_size=1003, pan_genes=330, core_genes=100, HR_rate=0.4, HGT_rate=0.2)
    N, L, G, g0 = 77, 1003, 230, 4
    rng = np.random.default_rng(9)
    core = (1 << rng.integers(0, 4, (N, L))).astype(np.uint8)
    acc = (rng.random((N, G)) < 0.45).astype(np.uint8)
    sigma = rng.permutation(N).astype(np.uint32)
    parents = rng.integers(0, N, N).astype(np.uint32)
    path = str(tmp_path / "ref.state")
    padding = rng.integers(1, 256, (L, 128 - N)).astype(np.uint8)
    ref.write(path, dict(kw, seed=5, n_gen=8, max_distances=100), core, acc, generations_done=g0, sigma=sigma,
              last_parents=parents, padding=padding)
    assert ref.read(path)["padding"].any()
    sim = pa.Simulation.load(path)
    assert sim.generation == g0
    assert np.array_equal(sim.last_parents(), parents)
    assert np.array_equal(sim.core_genome.read_matrix(), core[sigma.astype(np.int64)])
    assert np.array_equal(sim.pan_genome.read_matrix(), acc[sigma.astype(np.int64)])
    o = OracleSim(seed=5, **kw)
    o._core, o._acc, o.sigma = core.copy(), acc.copy(), sigma.astype(np.int64)
    sim.run(3)
    for g in range(g0, g0 + 3):
        o.generation(g)
    assert np.array_equal(sim.last_parents(), o.last_idx)
    assert np.array_equal(sim.core_genome.read_matrix(), o.core) and np.array_equal(sim.pan_genome.read_matrix(), o.acc)
    # saved again, the padding is code 0
    again = str(tmp_path / "again.state")
    sim.save(again)
    st = ref.read(again)
    assert not st["padding"].any() and st["generations_done"] == g0 + 3
    assert np.array_equal(ref.output_rows(st, "core"), o.core)
    sim.close()


def test_raw8_for_matrices_that_are_not_one_hot_and_the_size_of_a_packed_file(pa, tmp_path):
    kw = dict(pop_size=120, core_size=901, pan_genes=400, core_genes=100, HR_rate=0.2, HGT_rate=0.05)
    case = dict(kw=kw)
    sim = _new(pa, case, 6)
    sim.run(2)
    packed = str(tmp_path / "packed.state")
    sim.save(packed)
    h = pa.state_info(packed)
    assert h["encoding"] == "packed2"
    assert os.path.getsize(packed) <= 0.26 * h["header"].pitch * 901 + h["header"].acc_bytes + 64 * 1024
    rows = sim.core_genome.read_matrix()
    rows[0, 0], rows[5, 17], rows[119, 900] = 3, 16, 255
    sim.core_genome.load_matrix(rows)
    raw = str(tmp_path / "raw.state")
    sim.save(raw)
    h = pa.state_info(raw)
    assert h["encoding"] == "raw8" and h["header"].core_bytes == 901 * 128 and h["header"].core_rows_overridden == 1
    st = ref.read(raw)
    assert np.array_equal(st["core"], rows)            # (the loaded order is the internal one)
    back = pa.Simulation.load(raw)
    _same(_outputs(back), _outputs(sim), "raw8 state right after the load")
    sim.run(1)
    back.run(1)
    _same(_outputs(back), _outputs(sim), "a generation on a raw8 state")
    assert back.core_genome.read_matrix().max() == 255
    sim.close()
    back.close()


@pytest.mark.parametrize("rows", [1, 3, 4097])
def test_chunking_never_shows(pa, tmp_path, monkeypatch, rows):
    case = dict(kw=dict(pop_size=100, core_size=5003, pan_genes=300, core_genes=100, HR_rate=0.1))
    sim = _new(pa, case, 4)
    sim.run(3)
    want = _outputs(sim)
    default, chunked = str(tmp_path / "default.state"), str(tmp_path / "chunked.state")
    sim.save(default)
    monkeypatch.setenv("PANSIM_STATE_CHUNK_ROWS", str(rows))
    sim.save(chunked)
    assert open(default, "rb").read() == open(chunked, "rb").read()
    back = pa.Simulation.load(default)
    _same(_outputs(back), want, "loaded in chunks of %d rows" % rows)
    back.run(1)
    sim.run(1)
    _same(_outputs(back), _outputs(sim), "a generation behind a chunked load")
    back.close()
    sim.close()


def test_a_corrupt_section_is_an_error_return_and_nothing_sticks(pa, tmp_path):
    case = dict(kw=dict(pop_size=130, core_size=2000, pan_genes=300, core_genes=100))
    sim = _new(pa, case, 4)
    sim.run(2)
    want = _outputs(sim)
    good = str(tmp_path / "good.state")
    sim.save(good)
    sim.close()
    raw = open(good, "rb").read()
    h = pa.state_info(good)["header"]
    for offset, name in ((h.core_offset + 12345, "core section"), (h.acc_offset + 77, "accessory section"), (h.maps_offset + 5, "row-map section")):
        bad = bytearray(raw)
        bad[offset] ^= 0x10
        p = str(tmp_path / "bad.state")
        open(p, "wb").write(bytes(bad))
        with pytest.raises(pa.PansimError) as e:
            pa.Simulation.load(p)
        assert e.value.code == PS_ERR_IO and name in str(e.value) and "checksum mismatch" in str(e.value)
        back = pa.Simulation.load(good)          # nothing leaked, no sticky error
        _same(_outputs(back), want, "valid load behind a refused one")
        back.close()


def test_branch_other_rates_and_seed_from_the_saved_matrices(pa, tmp_path):
    kw = dict(pop_size=160, core_size=1501, pan_genes=500, core_genes=100, prop_positive=0.3)
    N, L, G = 160, 1501, 400
    rng = np.random.default_rng(21)
    core = (1 << rng.integers(0, 4, (N, L))).astype(np.uint8)
    acc = (rng.random((N, G)) < 0.5).astype(np.uint8)
    src = pa.Simulation(pa.make_params(seed=1, n_gen=4, max_distances=100, **kw))
    src.core_genome.load_matrix(core)          # the two row orders coincide: the branch is pinned without the oracle
    src.pan_genome.load_matrix(acc)
    path = str(tmp_path / "src.state")
    src.save(path)
    h = pa.state_info(path)["header"]
    assert h.has_row_maps == 0 and h.core_rows_overridden == 1 and h.acc_rows_overridden == 1
    other = dict(kw, HR_rate=0.4, HGT_rate=0.3, core_mu=0.08, rate_genes1=2.0)
    q = pa.make_params(seed=99, n_gen=4, max_distances=100, **other)
    branch = pa.Simulation.load(path, q)
    by_hand = pa.Simulation(pa.make_params(seed=99, n_gen=4, max_distances=100, **other))
    by_hand.core_genome.load_matrix(core)
    by_hand.pan_genome.load_matrix(acc)
    assert np.array_equal(branch.selection_weights, pa.selection_coefficients(99, G, 0.3, 10.0, 10.0))
    assert not np.array_equal(branch.selection_weights, src.selection_weights)
    assert np.array_equal(branch.range1, by_hand.range1)
    _same(_outputs(branch), _outputs(by_hand), "branch right after the load")
    branch.run(3)
    by_hand.run(3, first_generation=0)
    _same(_outputs(branch), _outputs(by_hand), "branch after three generations")
    # a branch off a state with row maps runs too
    src.run(2)
    src.save(path)
    b2 = pa.Simulation.load(path, q)
    b2.run(2)
    assert b2.generations_done == 4 and np.array_equal(b2.selection_weights, branch.selection_weights)
    # the sizes and the shard are the file's
    for field, value in (("pop_size", 161), ("core_size", 1500), ("pan_genes", 501), ("core_genes", 99), ("shard_count", 2)):
        bad = pa.make_params(seed=99, n_gen=4, max_distances=100, **dict(other, **{field: value}))
        with pytest.raises(pa.PansimError) as e:
            pa.Simulation.load(path, bad)
        assert e.value.code == PS_ERR_INVALID and field in str(e.value)
    for s in (src, branch, by_hand, b2):
        s.close()


def test_a_ps_multi_run_is_saved_shard_by_shard(pa, tmp_path):
    kw = dict(pop_size=140, core_size=2001, pan_genes=400, core_genes=100, HR_rate=0.2, HGT_rate=0.1)
    m = pa.MultiSimulation(pa.make_params(seed=3, n_gen=5, max_distances=60, **kw), 2, devices=[0, 0])
    m.run(3)
    m.sync()
    for k, shard in enumerate(m.shards):
        path = str(tmp_path / ("shard%d.state" % k))
        shard.save(path)                               # reading a borrowed shard is allowed
        alone = pa.Simulation.load(path)
        assert (alone.params.shard_rank, alone.params.shard_count) == (k, 2)
        assert np.array_equal(alone.core_genome.read_matrix(), shard.core_genome.read_matrix())
        assert np.array_equal(alone.pan_genome.read_matrix(), shard.pan_genome.read_matrix())
        assert np.array_equal(alone.last_parents(), shard.last_parents())
        alone.close()
    m.run(2)                                           # and the run goes on
    m.sync()
    m.close()


FILES = (".tsv", "_freqs.txt", "_per_gen.tsv", "_selection.tsv", "_core_genome.csv", "_pangenome.csv")


def _cli(*args):
    return subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=600)


def test_cli_save_then_load_writes_the_bytes_of_the_straight_run(pa, tmp_path):
    k = 3
    common = ["--pop_size", 100, "--core_size", 1200, "--pan_genes", 600, "--core_genes", 200, "--max_distances", 300, "--seed", 4,
              "--prop_positive", 0.2]
    prints = ["--print_dist", "--print_matrices", "--print_selection"]
    state = tmp_path / "k.state"
    r = _cli(*common, *prints, "--n_gen", 2 * k, "--outpref", tmp_path / "straight")
    assert r.returncode == 0, r.stderr
    r = _cli(*common, *prints, "--n_gen", k, "--outpref", tmp_path / "first", "--save_state", state)
    assert r.returncode == 0, r.stderr
    r = _cli(*common, *prints, "--n_gen", 2 * k, "--outpref", tmp_path / "second", "--load_state", state, "--verbose")
    assert r.returncode == 0, r.stderr
    assert "Loaded 3 generations" in r.stdout and "Finished gen: 4" in r.stdout and "Finished gen: 3\n" not in r.stdout
    for suffix in FILES:
        a, b = open(str(tmp_path / "straight") + suffix, "rb").read(), open(str(tmp_path / "second") + suffix, "rb").read()
        assert len(a) > 0 and a == b, suffix
    assert pa.state_info(str(state), per_gen=True)["per_gen"].shape == (k, 4)
    # a state saved without --print_dist cannot continue under it
    r = _cli(*common, "--n_gen", k, "--outpref", tmp_path / "plain", "--save_state", tmp_path / "plain.state")
    assert r.returncode == 0, r.stderr
    r = _cli(*common, "--print_dist", "--n_gen", 2 * k, "--outpref", tmp_path / "no", "--load_state", tmp_path / "plain.state")
    assert r.returncode == 101 and "saved without --print_dist" in r.stderr
    r = _cli(*common, "--n_gen", 2 * k, "--outpref", tmp_path / "plain2", "--load_state", tmp_path / "plain.state")
    assert r.returncode == 0 and open(str(tmp_path / "plain2.tsv"), "rb").read() == open(str(tmp_path / "straight.tsv"), "rb").read()
    r = _cli(*common, "--n_gen", k - 1, "--outpref", tmp_path / "no", "--load_state", state)
    assert r.returncode == 101 and "--n_gen" in r.stderr
    r = _cli(*common, "--pop_size", 101, "--n_gen", 2 * k, "--outpref", tmp_path / "no", "--load_state", state)
    assert r.returncode == 101 and "pop_size" in r.stderr
    r = _cli(*common, "--n_gen", k, "--gpus", 2, "--outpref", tmp_path / "no", "--save_state", tmp_path / "no.state")
    assert r.returncode == 101 and "--gpus 1" in r.stderr and not os.path.exists(tmp_path / "no.state")


def test_cfg2_at_full_size(pa, tmp_path):
    # 1000 x 1.2 M: a 300 MB file.  Skipped when the temporary directory has less than 1 GiB free -- the cases above are the
    # coverage then.
    if shutil.disk_usage(str(tmp_path)).free < (1 << 30):
        pytest.skip("less than 1 GiB free in the temporary directory")
    case = dict(kw=dict(pop_size=1000, core_size=1200000, pan_genes=6000, core_genes=2000))
    path = str(tmp_path / "cfg2.state")
    straight = _new(pa, case, 5, P=1000)
    straight.run(5)
    first = _new(pa, case, 5, P=1000)
    first.run(3)
    first.save(path)
    first.close()
    h = pa.state_info(path)["header"]
    assert h.core_bytes == 1200000 * 256 and os.path.getsize(path) < 310 * 10 ** 6
    sim = pa.Simulation.load(path)
    sim.run(2)
    sim.sync()
    straight.sync()
    assert np.array_equal(sim.last_parents(), straight.last_parents())
    for x, y in zip(sim.final_distances(), straight.final_distances()):
        assert np.array_equal(x, y)
    assert np.array_equal(sim.pan_genome.read_matrix(), straight.pan_genome.read_matrix())
    assert np.array_equal(sim.core_genome.read_matrix(), straight.core_genome.read_matrix())
    sim.close()
    straight.close()
    os.remove(path)
