#!/usr/bin/env python3
"""Device time of the core counts kernel (ps_core_diversity / ps_site_allele_counts, docs/CORE_DIVERSITY.md) beside the
one-generation core sweep of the same run.  Run it under a time limit:
    timeout -k 10 900 python scripts/bench_core_diversity.py [OUT.json] [case ...]

Cases: cfg2 (N = 1000, L = 1 200 000), n8192 (N = 8192, L = 1 200 000).  Per case, in one process: a simulation runs 3 + 20
generations with one generation per sweep launch ("sweep_generations" = 1) and sweep timing on (HIP events around each
launch, Simulation.sweep_timing()); then each form of the counts pass -- summary only, counts stored -- is launched 3 + 20
times on the evolved matrix and timed by the HIP events around its kernel (Population.core_diversity_timing()).  GB/s are
over the bytes the pass has to move: N L cells read (+ 16 L bytes of counts written); the fraction is of the 8 TB/s HBM
peak.  The condition: neither form takes longer than the sweep launch, which moves twice the bytes."""
import json
import os
import sys

import numpy as np

try:                # before the library: one HIP runtime per process (tests/conftest.py)
    import torch
except ImportError:
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pansim_amd as pa  # noqa: E402

HBM_PEAK = 8.0e12
WARMUP, LAUNCHES = 3, 20
CASES = {"cfg2": (1000, 1200000), "n8192": (8192, 1200000)}


def timed(pop, call):
    ms = []
    for k in range(WARMUP + LAUNCHES):
        call()
        if k >= WARMUP:
            ms.append(pop.core_diversity_timing())
    return ms


def case(name):
    N, L = CASES[name]
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, n_gen=WARMUP + LAUNCHES, max_distances=100))
    core = sim.core_genome
    core.set_tuning("sweep_generations", 1)
    sim.run(WARMUP)
    sim.sync()
    sim.enable_timing(True)
    sim.sweep_timing(reset=True)
    sim.run(LAUNCHES)
    sim.sync()
    launches, total_ms, sweep_bytes = sim.sweep_timing(reset=True)
    sweep_ms = total_ms / launches
    row = {"case": name, "pop_size": N, "core_size": L, "sweep_form": core.last_sweep_form(), "sweep_launches": launches,
           "sweep_ms": round(sweep_ms, 4), "sweep_gb_per_s": round(sweep_bytes / sweep_ms / 1e6, 1), "forms": {}}
    ok = True
    for form, call, nbytes in (("summary", core.core_diversity, N * L), ("counts", core.site_allele_counts, N * L + 16 * L)):
        ms = timed(core, call)
        med = float(np.median(ms))
        row["forms"][form] = {"ms_median": round(med, 4), "ms_mean": round(float(np.mean(ms)), 4), "ms_max": round(max(ms), 4),
                              "bytes": nbytes, "gb_per_s": round(nbytes / med / 1e6, 1),
                              "fraction_of_8_tb_per_s": round(nbytes / (med * 1e-3) / HBM_PEAK, 4),
                              "no_longer_than_the_sweep": bool(med <= sweep_ms)}
        ok = ok and med <= sweep_ms
    d = core.core_diversity()
    row["segregating_sites"], row["mean_pairwise_distance"] = d["segregating_sites"], d["mean_pairwise_distance"]
    sim.close()
    print(json.dumps(row), flush=True)
    return row, ok


def main():
    out = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1].endswith(".json") else None
    names = [a for a in sys.argv[1:] if not a.endswith(".json")] or list(CASES)
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    rows, ok = [], True
    for n in names:
        row, good = case(n)
        rows.append(row)
        ok = ok and good
    if out:
        with open(out, "w") as f:
            json.dump({"script": "scripts/bench_core_diversity.py", "device": device, "warmup": WARMUP, "launches": LAUNCHES,
                       "hbm_peak_bytes_per_s": HBM_PEAK, "results": rows}, f, indent=1)
    if not ok:
        raise SystemExit("a form of the counts pass took longer than the one-generation sweep launch")


if __name__ == "__main__":
    main()
