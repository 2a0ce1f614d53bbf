#!/usr/bin/env python3
"""Device time of the core pass of the group differentiation (ps_group_differentiation, docs/GROUP_DIFFERENTIATION.md)
beside the per-site counts pass (ps_site_allele_counts), which reads the same N L bytes of the same handle.  Run it under a
time limit:
    timeout -k 10 900 python scripts/bench_group_differentiation.py [OUT.json]

cfg2 (N = 1000, L = 1 200 000, G = 6000) after 100 generations.  The labels are those of strain_clusters at the largest core
threshold of a halving ladder that still gives 16 clusters; K = 2, 8, 16 takes the K largest (max_groups = K, min_size = 1),
without counts or per-site output.  Per K: 3 warm-up calls, then 20 calls alternating call for call with
ps_site_allele_counts; core_ms of group_differentiation_timing() against core_diversity_timing(), HIP events around each
kernel.  The medians, their ratio and GB/s over the N L bytes read are printed; no ratio is a condition."""
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

WARMUP, CALLS = 3, 20
N, L, GENERATIONS = 1000, 1200000, 100


def labels_with(sim, wanted):
    """strain_clusters labels with at least `wanted` clusters: the largest threshold of L / 2, L / 4 ... 0 that gives them"""
    d = L // 2
    while True:
        c = sim.strain_clusters(core_max_d=d)
        if c.clusters >= wanted or d == 0:
            return c, d
        d //= 2


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, n_gen=GENERATIONS, max_distances=100))
    sim.run(GENERATIONS)
    sim.sync()
    core = sim.core_genome
    clusters, core_max_d = labels_with(sim, 16)
    rows = []
    for K in (2, 8, 16):
        diff_ms, counts_ms = [], []
        for k in range(WARMUP + CALLS):
            d = core.group_differentiation(clusters.labels, max_groups=K, min_size=1)
            t = core.group_differentiation_timing()
            core.site_allele_counts()
            c = core.core_diversity_timing()
            if k >= WARMUP:
                diff_ms.append(t[1])
                counts_ms.append(c)
        dm, cm = float(np.median(diff_ms)), float(np.median(counts_ms))
        row = {"max_groups": K, "groups": d.groups, "group_size": [int(x) for x in d.group_size], "assigned": d.assigned,
               "core_ms_median": round(dm, 4), "core_ms_min": round(min(diff_ms), 4), "core_ms_max": round(max(diff_ms), 4),
               "members_ms": round(t[0], 4), "site_allele_counts_ms_median": round(cm, 4), "ratio": round(dm / cm, 3),
               "gb_per_s": round(N * L / dm / 1e6, 1), "site_allele_counts_gb_per_s": round(N * L / cm / 1e6, 1), "fst": d.fst}
        rows.append(row)
        print(json.dumps(row), flush=True)
    sim.close()
    if out:
        with open(out, "w") as f:
            json.dump({"script": "scripts/bench_group_differentiation.py", "device": device, "pop_size": N, "core_size": L,
                       "generations": GENERATIONS, "warmup": WARMUP, "calls": CALLS, "clusters": clusters.clusters,
                       "core_max_d": core_max_d, "results": rows}, f, indent=1)


if __name__ == "__main__":
    main()
