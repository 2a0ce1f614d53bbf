#!/usr/bin/env python3
"""Device time of the linkage disequilibrium between loci (ps_locus_ld, docs/LINKAGE_DISEQUILIBRIUM.md) beside the
one-generation core sweep and the ps_core_diversity pass of the same process.  Run it under a time limit:
    timeout -k 10 900 python scripts/bench_site_ld.py [OUT.json]

cfg2's shape (N = 1000, L = 1 200 000, G = 6000): a simulation runs 100 generations, the last 20 with one generation per sweep
launch ("sweep_generations" = 1) and sweep timing on; then ps_core_diversity and, for max_loci 4096 and 16384 and both metrics,
ps_locus_ld are launched 3 + 20 times on the evolved matrices and timed by their own HIP events (the four phases of
Population.locus_ld_timing(): select, pack, counts, statistics).  No figure is a condition: the script reports."""
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

WARMUP, LAUNCHES = 3, 20
N, L, G, GENERATIONS = 1000, 1200000, 6000, 100
PHASES = ("select_ms", "pack_ms", "counts_ms", "stats_ms")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1].endswith(".json") else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, pan_genes=G, n_gen=GENERATIONS, max_distances=100))
    core = sim.core_genome
    sim.run(GENERATIONS - LAUNCHES)
    sim.sync()
    core.set_tuning("sweep_generations", 1)
    sim.enable_timing(True)
    sim.sweep_timing(reset=True)
    sim.run(LAUNCHES)
    sim.sync()
    launches, total_ms, _ = sim.sweep_timing(reset=True)
    div = []
    for k in range(WARMUP + LAUNCHES):
        core.core_diversity()
        if k >= WARMUP:
            div.append(core.core_diversity_timing())
    rows = {"script": "scripts/bench_site_ld.py", "device": device, "pop_size": N, "core_size": L, "pan_genes": G,
            "generations": GENERATIONS, "warmup": WARMUP, "launches": LAUNCHES, "sweep_ms": round(total_ms / launches, 4),
            "core_diversity_ms": round(float(np.median(div)), 4), "results": []}
    for metric, pop in (("core", core), ("acc", sim.pan_genome)):
        for max_loci in (4096, 16384):
            ms = []
            for k in range(WARMUP + LAUNCHES):
                r = sim.locus_ld(metric, max_loci=max_loci)
                if k >= WARMUP:
                    ms.append(pop.locus_ld_timing())
            med = np.median(np.array(ms), axis=0)
            row = {"metric": metric, "max_loci": max_loci, "candidates": r.candidates, "loci": r.loci, "pairs": r.pairs,
                   "defined_pairs": r.defined_pairs, "four_gamete_pairs": r.four_gamete_pairs, "mean_r2": r.mean_r2,
                   "total_ms": round(float(med.sum()), 4)}
            row.update({name: round(float(v), 4) for name, v in zip(PHASES, med)})
            rows["results"].append(row)
            print(json.dumps(row), flush=True)
    sim.close()
    print(json.dumps({k: v for k, v in rows.items() if k != "results"}), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
