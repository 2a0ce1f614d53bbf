#!/usr/bin/env python3
"""Device time of the neighbour-joining tree (ps_sim_neighbour_joining, docs/NEIGHBOUR_JOINING.md) at the cfg5 population (N = 8192,
L = 1 200 000, G = 6000) and the cfg2 population (N = 1000, same L and G), both metrics.  Run it under a time limit:
    timeout -k 10 900 python scripts/bench_neighbour_joining.py [OUT.json] [cfg2 cfg5]
(the populations named, both by default).

Per population two states in one process: generation 0 (every pair a tie: the caterpillar) and the population after 100
generations.  Per state and metric an untimed first call, 3 warm-up calls, then 10 calls (where the first call takes more than
4 s it is the only warm-up and 3 calls are timed, 1 above 40 s; the row says so) read through ps_neighbour_joining_timing (HIP
events): the count kernels of the metric, the store kernels and the row sums, the N - 1 joins.  The yardstick is the existing
ps_upgma_tree with the same metric on the same handles, alternating call for call and read through ps_upgma_tree_timing; the two
share their count phase and nothing else.  Bytes by arithmetic: the scan of the join among n active nodes loads n (n - 1) / 2
distances of 8 bytes (every pair once), n = N, N - 1, ..., 2 whatever the state: about N^3 / 6 words per call.  One expectation, reported and not
enforced: the cost of a join, joins_ms / (N - 2), stays below the cost of a round of the UPGMA tree measured in the same run
(its rounds_ms / rounds)."""
import json
import os
import sys
import time

import numpy as np

try:                # before the library: one HIP runtime per process (tests/conftest.py)
    import torch
except ImportError:
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pansim_amd as pa  # noqa: E402

WARMUP, CALLS, SLOW_CALL_S, VERY_SLOW_CALL_S = 3, 10, 4.0, 40.0
L, PAN, CG, GENERATIONS = 1200000, 8000, 2000, 100


def row(sim, config, N, state, metric, warmup, calls):
    t0 = time.time()
    sim.neighbour_joining(metric=metric)
    first_s = time.time() - t0
    if first_s > SLOW_CALL_S:                       # (the untimed first call is the warm-up then)
        warmup, calls = 0, 3 if first_s < VERY_SLOW_CALL_S else 1
    t = {"counts": [], "store": [], "joins": [], "yard_counts": [], "yard_store": [], "yard_rounds": []}
    for k in range(warmup + calls):
        tree = sim.neighbour_joining(metric=metric)
        mine = sim.neighbour_joining_timing()
        upgma = sim.upgma_tree(metric=metric)
        yard = sim.core_genome.upgma_tree_timing()
        if k >= warmup:
            for key, v in zip(("counts", "store", "joins"), mine):
                t[key].append(v)
            for key, v in zip(("yard_counts", "yard_store", "yard_rounds"), yard):
                t[key].append(v)
    total = [a + b + c for a, b, c in zip(t["counts"], t["store"], t["joins"])]
    yard_total = [a + b + c for a, b, c in zip(t["yard_counts"], t["yard_store"], t["yard_rounds"])]
    med = {key: float(np.median(v)) for key, v in t.items()}
    scan_bytes = 8 * sum(n * (n - 1) // 2 for n in range(2, N + 1))
    per_join, per_round = med["joins"] / (N - 2), med["yard_rounds"] / upgma.rounds
    out = {"config": config, "pop_size": N, "state": state, "metric": metric, "counts_ms": round(med["counts"], 4),
           "store_ms": round(med["store"], 4), "joins_ms": round(med["joins"], 4), "joins_ms_max": round(max(t["joins"]), 4),
           "total_ms": round(float(np.median(total)), 4), "ms_per_join": round(per_join, 5), "negative_branches": tree.negative_branches,
           "tree_length": tree.tree_length, "matrix_bytes": N * ((N + 63) // 64 * 64) * 8, "scan_bytes": scan_bytes,
           "scan_GBps": round(scan_bytes / med["joins"] / 1e6, 1), "yardstick_counts_ms": round(med["yard_counts"], 4),
           "yardstick_store_ms": round(med["yard_store"], 4), "yardstick_rounds_ms": round(med["yard_rounds"], 4),
           "yardstick_total_ms": round(float(np.median(yard_total)), 4), "yardstick_rounds": upgma.rounds,
           "yardstick_ms_per_round": round(per_round, 5), "join_below_round": bool(per_join < per_round), "first_call_s": round(first_s, 3),
           "warmup": warmup, "timed_calls": calls}
    print(json.dumps(out), flush=True)
    return out


def population(config, N):
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, pan_genes=PAN, core_genes=CG, n_gen=GENERATIONS, max_distances=100))
    rows = [row(sim, config, N, "generation 0", m, WARMUP, CALLS) for m in ("core", "acc")]
    sim.run(GENERATIONS)
    sim.sync()
    rows += [row(sim, config, N, "generation %d" % GENERATIONS, m, WARMUP, CALLS) for m in ("core", "acc")]
    sim.close()
    return rows


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sizes = {"cfg2": 1000, "cfg5": 8192}
    names = sys.argv[2:] or list(sizes)
    if any(name not in sizes for name in names):
        sys.exit("populations: cfg2 cfg5")
    rows = [r for name in names for r in population(name, sizes[name])]
    result = {"device": device, "core_size": L, "accessory_genes": PAN - CG, "warmup": WARMUP, "calls": CALLS, "rows": rows,
              "expectation_met": all(r["join_below_round"] for r in rows)}
    if out:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
