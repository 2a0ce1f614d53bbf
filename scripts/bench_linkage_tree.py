#!/usr/bin/env python3
"""Device time of the single-linkage tree (ps_sim_linkage_tree, docs/LINKAGE_TREE.md) at the cfg5 population: N = 8192,
L = 1 200 000, G = 6000, both metrics.  Run it under a time limit:
    timeout -k 10 900 python scripts/bench_linkage_tree.py [OUT.json]

Two states in one process: generation 0 (every pair a tie: the star of row 0 in one round) and the population after 100
generations.  Per state and metric 3 warm-up calls, then 10 calls read through ps_linkage_tree_timing (HIP events): the count
kernels of the metric, the store kernels, the rounds (host round trips included).  The yardstick is the existing
ps_strain_clusters with the matching single criterion (the threshold: the tree's median merge height) on the same handles,
alternating call for call and read through ps_strain_clusters_timing -- code the tree shares only its count phase with.
Both calls are dominated by that phase; the tree adds the store (N^2 x 4 or 2 bytes written) and its rounds (the same bytes
read per round).  The condition is median total device time of the tree call <= 1.25 x that of the cluster call: a few per
cent for the added traffic, the rest for the 8 % spread between boxes that README records."""
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

WARMUP, CALLS, MARGIN = 3, 10, 1.25
N, L, PAN, CG, GENERATIONS = 8192, 1200000, 8000, 2000, 100


def row(sim, state, metric):
    first = sim.linkage_tree(metric=metric)
    mid = first.edges // 2
    num, den = int(first.num[mid]), int(first.den[mid])
    crit = dict(core_max_d=num) if metric == "core" else dict(acc_ratio=(num, den))
    t = {"counts": [], "store": [], "rounds": [], "yard_counts": [], "yard_edges": [], "yard_labels": []}
    for k in range(WARMUP + CALLS):
        tree = sim.linkage_tree(metric=metric)
        mine = sim.core_genome.linkage_tree_timing()
        c = sim.strain_clusters(**crit)
        yard = sim.core_genome.strain_clusters_timing()
        if k >= WARMUP:
            for key, v in zip(("counts", "store", "rounds"), mine):
                t[key].append(v)
            for key, v in zip(("yard_counts", "yard_edges", "yard_labels"), yard):
                t[key].append(v)
    assert tree.clusters_at(num, den) == c.clusters, (tree.clusters_at(num, den), c.clusters)
    total = [a + b + c_ for a, b, c_ in zip(t["counts"], t["store"], t["rounds"])]
    yard_total = [a + b + c_ for a, b, c_ in zip(t["yard_counts"], t["yard_edges"], t["yard_labels"])]
    med = {key: float(np.median(v)) for key, v in t.items()}
    m_tree, m_yard = float(np.median(total)), float(np.median(yard_total))
    out = {"state": state, "metric": metric, "counts_ms": round(med["counts"], 4), "store_ms": round(med["store"], 4),
           "rounds_ms": round(med["rounds"], 4), "total_ms": round(m_tree, 4), "total_ms_max": round(max(total), 4),
           "yardstick_counts_ms": round(med["yard_counts"], 4), "yardstick_edges_ms": round(med["yard_edges"], 4),
           "yardstick_labels_ms": round(med["yard_labels"], 4), "yardstick_total_ms": round(m_yard, 4),
           "tree_over_clusters": round(m_tree / m_yard, 4), "rounds": tree.rounds, "distinct_heights": tree.distinct_heights,
           "undefined_edges": tree.undefined_edges, "threshold": [num, den], "clusters_at_threshold": c.clusters,
           "matrix_bytes": N * ((N + 63) // 64 * 64) * (4 if metric == "core" else 2), "within_margin": bool(m_tree <= MARGIN * m_yard)}
    print(json.dumps(out), flush=True)
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, pan_genes=PAN, core_genes=CG, n_gen=GENERATIONS, max_distances=100))
    rows = [row(sim, "generation 0", m) for m in ("core", "acc")]
    sim.run(GENERATIONS)
    sim.sync()
    rows += [row(sim, "generation %d" % GENERATIONS, m) for m in ("core", "acc")]
    sim.close()
    ok = all(r["within_margin"] for r in rows)
    result = {"device": device, "pop_size": N, "core_size": L, "accessory_genes": PAN - CG, "warmup": WARMUP, "calls": CALLS,
              "margin": MARGIN, "rows": rows, "ok": ok}
    if out:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
