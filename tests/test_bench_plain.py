"""A plain `bench.py --gpus 1 --steps N --warmup W` does only what its headline figure needs; everything else waits for
`--full`.  `--dump-outputs DIR` writes what the timed path computed in its last step, the same on every run with the same
arguments.  The CPU checks run the host logic with tests/bench_stub.py standing in for the HIP engine; the GPU check runs
the real engine at a small size and compares its dump with the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONTRACT = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "scaling",
            "vs_baseline", "data", "config", "roofline"}
FULL_ONLY = {"cpu_baseline", "other_configs", "mpairs_per_s", "distance_ms", "pair_sites_per_s", "distance_roofline",
             "north_star_scaling", "north_star_generations_per_s", "north_star_distance"}


def _run(*args, env_add=None, stub=True, timeout=240):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PANSIM_BENCH_STUB", "PANSIM_BENCH_BACKEND"):
        env.pop(k, None)
    if stub:
        env.update({"PANSIM_BENCH_STUB": "bench_stub", "PANSIM_BENCH_PG_TIMEOUT": "60",
                    "PYTHONPATH": os.path.join(ROOT, "tests") + os.pathsep + env.get("PYTHONPATH", "")})
    env.update(env_add or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + [str(a) for a in args], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    return lines[0]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_plain_run_prints_only_the_headline_line():
    d = _run("--gpus", 1, "--steps", 7, "--warmup", 2)
    assert CONTRACT <= set(d), sorted(CONTRACT - set(d))
    assert not FULL_ONLY & set(d), sorted(FULL_ONLY & set(d))
    assert d["full"] is False and d["steps"] == 7 and d["warmup"] == 2 and d["line"] == "final"
    assert d["metric"] == "generations/sec" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]


def test_plain_run_with_two_ranks_skips_the_north_star_workloads():
    d = _run("--gpus", 2, "--steps", 5, "--warmup", 1)
    assert d["n_gpus"] == 2 and d["line"] == "final" and d["launcher"]["self_launched"]
    assert CONTRACT <= set(d) and not FULL_ONLY & set(d)


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode != 0 and "--steps" in p.stderr


def test_dump_outputs_are_float_bounded_and_repeatable(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    da = _run("--steps", 4, "--warmup", 1, "--dump-outputs", a)
    _run("--steps", 4, "--warmup", 1, "--dump-outputs", b)
    oa, ob = _load(a), _load(b)
    assert set(oa) == set(da["dumped_outputs"]["arrays"]) == {"parents", "pan_genome", "core_genome_sample",
                                                               "core_genome_sample_index"}
    assert sum(x.nbytes for x in oa.values()) <= 64 << 20
    for name, x in oa.items():
        assert x.dtype in (np.float32, np.float64), (name, x.dtype)
        assert np.array_equal(x, ob[name]), name
    idx = oa["core_genome_sample_index"]
    assert oa["parents"].dtype == np.float64 and oa["pan_genome"].dtype == np.float32
    assert np.all(np.diff(idx) >= 0) and idx[0] >= 0 and idx[-1] < 1000 * 5000


def test_dump_arrays_keeps_small_arrays_whole_and_samples_large_ones():
    import bench
    raw = {"p": np.arange(10, dtype=np.uint32), "m": np.arange(bench.DUMP_WHOLE_CELLS + 1, dtype=np.int64).astype(np.uint8)}
    out = bench.dump_arrays(raw)
    assert set(out) == {"p", "m_sample", "m_sample_index"}
    assert out["p"].dtype == np.float64 and np.array_equal(out["p"], np.arange(10))
    idx = out["m_sample_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE_CELLS and out["m_sample"].dtype == np.float32
    assert np.array_equal(out["m_sample"], raw["m"][idx].astype(np.float32))
    assert np.array_equal(bench.dump_arrays(raw)["m_sample_index"], out["m_sample_index"])


@pytest.mark.gpu
def test_plain_dump_is_the_oracle_state_and_full_dumps_the_same(pa, tmp_path):
    # small sizes (the matrices are written whole): SETTLE_BATCHES x 50 settle generations, then warm-up and timed steps
    import bench
    from orc_sim import OracleSim
    kw = dict(pop_size=100, core_size=12000, pan_genes=2400)
    args = ["--pop_size", 100, "--core_size", 12000, "--pan_genes", 2400, "--steps", 5, "--warmup", 2]
    d = _run(*args, "--dump-outputs", tmp_path / "plain", stub=False, timeout=600)
    assert d["steps"] == 5 and d["full"] is False and not FULL_ONLY & set(d)
    f = _run(*args, "--full", "--no-cpu-baseline", "--dump-outputs", tmp_path / "full", stub=False, timeout=600)
    assert "distance_ms" in f
    plain, full = _load(tmp_path / "plain"), _load(tmp_path / "full")
    assert set(plain) == {"parents", "pan_genome", "core_genome"}
    for name in plain:
        assert np.array_equal(plain[name], full[name]), name
    ref = OracleSim(seed=0, HR_rate=0.05, HGT_rate=0.05, **kw)
    for g in range(bench.SETTLE_BATCHES * 50 + 2 + 5):
        ref.generation(g)
    assert np.array_equal(plain["parents"], ref.last_idx.astype(np.float64))
    assert np.array_equal(plain["core_genome"], ref.core.astype(np.float32))
    assert np.array_equal(plain["pan_genome"], ref.acc.astype(np.float32))
