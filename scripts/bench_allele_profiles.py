#!/usr/bin/env python3
"""Device time of the core allele profiles (ps_allele_profiles, docs/ALLELE_PROFILES.md) beside the counts pass of
ps_core_diversity of the same process on the same handle.  Run it under a time limit:
    timeout -k 10 900 python scripts/bench_allele_profiles.py [OUT.json] [OUT.md]

cfg2's shape (N = 1000, L = 1 200 000, G = 6000): a simulation runs 100 generations; then, for n_loci = 2000 with complex_max = 0
and 20 (600 sites per locus) and for n_loci = 60000 with complex_max = 600 (20 sites per locus: alleles are shared, rows are
verified, four bands of loci), ps_sim_allele_profiles and, alternating with it, ps_core_diversity on the core handle are
launched 3 + 10 times on the evolved matrix and timed by their own HIP events (the five phases of Population.allele_profiles_timing(): fingerprint, canon,
verify, pairs, labels; core_diversity_timing(): the one pass over the same bytes; medians).  The fingerprint pass over the
counts pass is recorded as a ratio, and the pairs phase as compares per second (pairs x n_loci / pairs_ms).  No figure is a
condition: the script reports."""
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

WARMUP, LAUNCHES = 3, 10
N, L, G, GENERATIONS = 1000, 1200000, 6000, 100
PHASES = ("fingerprint_ms", "canon_ms", "verify_ms", "pairs_ms", "labels_ms")
SHAPES = ((2000, 0), (2000, 20), (60000, 600))          # (n_loci, complex_max)


def _table(rows):
    head = ("n_loci", "complex_max") + PHASES + ("total_ms", "counts_ms", "fingerprint_over_counts", "compares_per_s", "sequence_types",
                                                  "complexes", "alleles_total", "mean_distance", "rounds")
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    lines += ["| " + " | ".join(str(r[h]) for h in head) + " |" for r in rows]
    return "\n".join(lines) + "\n"


def main():
    args = sys.argv[1:]
    out = next((a for a in args if a.endswith(".json")), None)
    table = next((a for a in args if a.endswith(".md")), None)
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, pan_genes=G, n_gen=GENERATIONS, max_distances=100))
    sim.run(GENERATIONS)
    sim.sync()
    doc = {"script": "scripts/bench_allele_profiles.py", "device": device, "pop_size": N, "core_size": L, "pan_genes": G,
           "generations": GENERATIONS, "warmup": WARMUP, "launches": LAUNCHES, "results": []}
    for N_LOCI, complex_max in SHAPES:
        ms, counts = [], []
        for k in range(WARMUP + LAUNCHES):          # alternating: both see the same clocks and caches
            r = sim.allele_profiles(N_LOCI, complex_max=complex_max, want_profiles=False)
            t = sim.allele_profiles_timing()
            sim.core_genome.core_diversity()
            if k >= WARMUP:
                ms.append(t)
                counts.append(sim.core_genome.core_diversity_timing())
        med = np.median(np.array(ms), axis=0)
        counts_ms = float(np.median(counts))
        row = {"n_loci": N_LOCI, "complex_max": complex_max}
        row.update({name: round(float(v), 4) for name, v in zip(PHASES, med)})
        row.update(total_ms=round(float(med.sum()), 4), counts_ms=round(counts_ms, 4), fingerprint_over_counts=round(float(med[0]) / counts_ms, 3),
                   compares_per_s=float("%.4g" % (r.pairs * N_LOCI / (float(med[3]) * 1e-3))), sequence_types=r.sequence_types,
                   complexes=r.complexes, alleles_total=r.alleles_total, monomorphic_loci=r.monomorphic_loci, max_alleles=r.max_alleles,
                   identical_pairs=r.identical_pairs, edges=r.edges, sum_d=r.sum_d, min_d=r.min_d, max_d=r.max_d,
                   mean_distance=r.mean_distance, rounds=r.rounds)
        doc["results"].append(row)
        print(json.dumps(row), flush=True)
    if table:
        with open(table, "w") as f:
            f.write(_table(doc["results"]))
    sim.close()
    print(json.dumps({k: v for k, v in doc.items() if k != "results"}), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
