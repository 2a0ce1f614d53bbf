#!/usr/bin/env python3
"""Device time of the strain clusters (ps_sim_strain_clusters, docs/STRAIN_CLUSTERS.md) at the cfg5 population: N = 8192,
L = 1 200 000, G = 6000, a joint threshold.  Run it under a time limit:
    timeout -k 10 900 python scripts/bench_strain_clusters.py [OUT.json]

Two rows, in one process: generation 0 (every pair an edge: the densest bit matrix, one cluster) and the population after
100 generations (core threshold a quarter of the way from the smallest to the largest d found, accessory distance 0.25).
Per row 3 warm-up calls, then 10 calls read through ps_strain_clusters_timing (HIP events): the count kernels of both
matrices, the edge kernel, the label rounds.  The yardstick is the joint distance histogram with an explicit span and 64 x 64
bins on the same handles, alternating call for call and read through ps_distance_histogram_timing: the edge kernel reads
the bytes the binning kernel reads and does less per pair, so the condition is median edges_ms <= 1.10 x median binning_ms
(10 % for the jitter of event timing on sub-millisecond kernels)."""
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

WARMUP, CALLS, MARGIN = 3, 10, 1.10
N, L, PAN, CG, BINS, GENERATIONS = 8192, 1200000, 8000, 2000, 64, 100
ACC_MAX = 0.25


def row(sim, name):
    span = sim.distance_histogram(BINS, BINS).core_span           # (also gives the state's range of d)
    h = sim.distance_histogram(BINS, BINS, core_span=span)
    core_max_d = h.core_d_min + (h.core_d_max - h.core_d_min) // 4
    t = {"counts": [], "edges": [], "labels": [], "binning": []}
    for k in range(WARMUP + CALLS):
        c = sim.strain_clusters(core_max_d=core_max_d, acc_max=ACC_MAX)
        mine = sim.core_genome.strain_clusters_timing()
        sim.distance_histogram(BINS, BINS, core_span=span)
        yard = sim.core_genome.distance_histogram_timing()
        if k >= WARMUP:
            for key, v in zip(("counts", "edges", "labels"), mine):
                t[key].append(v)
            t["binning"].append(yard[1])
    med = {key: float(np.median(v)) for key, v in t.items()}
    out = {"state": name, "core_max_d": core_max_d, "acc_max": ACC_MAX, "counts_ms": round(med["counts"], 4),
           "edges_ms": round(med["edges"], 4), "edges_ms_max": round(max(t["edges"]), 4), "labels_ms": round(med["labels"], 4),
           "yardstick_binning_ms": round(med["binning"], 4), "edges_over_binning": round(med["edges"] / med["binning"], 4),
           "rounds": c.rounds, "edges": c.edges, "clusters": c.clusters, "largest_cluster": c.largest_cluster,
           "adjacency_bytes_per_round": N * ((N + 63) // 64) * 8, "within_margin": bool(med["edges"] <= MARGIN * med["binning"])}
    print(json.dumps(out), flush=True)
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, pan_genes=PAN, core_genes=CG, n_gen=GENERATIONS, max_distances=100))
    rows = [row(sim, "generation 0")]
    sim.run(GENERATIONS)
    sim.sync()
    rows.append(row(sim, "generation %d" % GENERATIONS))
    sim.close()
    ok = all(r["within_margin"] for r in rows)
    result = {"device": device, "pop_size": N, "core_size": L, "accessory_genes": PAN - CG, "yardstick_bins": [BINS, BINS],
              "warmup": WARMUP, "calls": CALLS, "margin": MARGIN, "rows": rows, "ok": ok}
    if out:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
