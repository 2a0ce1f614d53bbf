#!/usr/bin/env python3
"""Device time of the nearest neighbours (ps_sim_nearest_neighbours, docs/NEAREST_NEIGHBOURS.md) at the cfg5 population:
N = 8192, L = 1 200 000, G = 6000, both metrics, k = 10 and k = 128.  Run it under a time limit:
    timeout -k 10 900 python scripts/bench_nearest_neighbours.py [OUT.json]

Two states in one process: generation 0 (every pair a tie: every pass of the selection moves on by one row) and the population
after 100 generations.  Per state, metric and k 3 warm-up calls, then 10 calls read through ps_nearest_neighbours_timing (HIP
events): the count kernels of the metric, the select kernels.  The yardstick is the existing ps_linkage_tree with the same
metric on the same handles, alternating call for call and read through ps_linkage_tree_timing -- code the neighbours share
only their count phase with.  The one condition: core metric, k = 10, median total device time <= 1.10 x the tree call's.  By
arithmetic the k passes read k N^2 x 4 bytes = 2.7 GB, mostly from L2, beside a count phase of about 90 ms; the margin leaves
about three times that estimate for the spread between boxes.  k = 128 and the accessory metric (a 0.2 ms contraction, to which
a ratio says nothing) report select_ms in absolute terms, with no condition."""
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
N, L, PAN, CG, GENERATIONS = 8192, 1200000, 8000, 2000, 100


def row(sim, state, metric, k):
    t = {"counts": [], "select": [], "yard": []}
    for call in range(WARMUP + CALLS):
        knn = sim.nearest_neighbours(k, metric=metric)
        mine = sim.core_genome.nearest_neighbours_timing()
        tree = sim.linkage_tree(metric=metric)
        yard = sim.core_genome.linkage_tree_timing()
        if call >= WARMUP:
            t["counts"].append(mine[0])
            t["select"].append(mine[1])
            t["yard"].append(sum(yard))
    # every (i, nbr[i][0]) is an edge of the tree
    edges = set(zip(tree.lo.tolist(), tree.hi.tolist()))
    first = knn.nbr[:, 0].astype(np.int64)
    rows = np.arange(N)
    assert all(e in edges for e in zip(np.minimum(rows, first).tolist(), np.maximum(rows, first).tolist()))
    total = [a + b for a, b in zip(t["counts"], t["select"])]
    m_knn, m_yard = float(np.median(total)), float(np.median(t["yard"]))
    conditional = metric == "core" and k == 10
    out = {"state": state, "metric": metric, "k": k, "counts_ms": round(float(np.median(t["counts"])), 4),
           "select_ms": round(float(np.median(t["select"])), 4), "select_ms_max": round(max(t["select"]), 4), "total_ms": round(m_knn, 4),
           "total_ms_max": round(max(total), 4), "yardstick_total_ms": round(m_yard, 4), "knn_over_tree": round(m_knn / m_yard, 4),
           "graph_edges": knn.graph_edges, "mutual_edges": knn.mutual_edges, "undefined_neighbours": knn.undefined_neighbours,
           "lineages_at_k": knn.lineages()[1]["lineages"], "condition": conditional,
           "within_margin": bool(m_knn <= MARGIN * m_yard) if conditional else None}
    print(json.dumps(out), flush=True)
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, pan_genes=PAN, core_genes=CG, n_gen=GENERATIONS, max_distances=100))
    cases = [(m, k) for m in ("core", "acc") for k in (10, 128)]
    rows = [row(sim, "generation 0", m, k) for m, k in cases]
    sim.run(GENERATIONS)
    sim.sync()
    rows += [row(sim, "generation %d" % GENERATIONS, m, k) for m, k in cases]
    sim.close()
    ok = all(r["within_margin"] for r in rows if r["condition"])
    result = {"device": device, "pop_size": N, "core_size": L, "accessory_genes": PAN - CG, "warmup": WARMUP, "calls": CALLS,
              "margin": MARGIN, "rows": rows, "ok": ok}
    if out:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
