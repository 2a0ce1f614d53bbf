#!/usr/bin/env python3
"""Device time of the average-linkage (UPGMA) tree (ps_sim_upgma_tree, docs/UPGMA_TREE.md) at the cfg5 population: N = 8192,
L = 1 200 000, G = 6000, both metrics.  Run it under a time limit (the whole script took under a minute on one MI355X, a clonal
call about 1.1 s: profiles/upgma_tree.md):
    timeout -k 10 600 python scripts/bench_upgma_tree.py [OUT.json]

Two states in one process: generation 0 (every pair a tie: the caterpillar, N - 1 rounds of one merge each, the worst case)
and the population after 100 generations.  Per state and metric an untimed first call, 3 warm-up calls, then 10 calls (where the
first call takes more than 4 s it is the only warm-up and 3 calls are timed, 1 above 40 s; the row says so) read through
ps_upgma_tree_timing (HIP events): the count kernels of the metric, the store kernels, the rounds (host round trips
included).  The yardstick is the existing ps_linkage_tree with the same metric on the same handles, alternating call for call
and read through ps_linkage_tree_timing; the two share their count phase and nothing else.  Bytes by arithmetic: the scan of a
round with m active clusters loads m (m - 1) sums of 8 bytes (twice that under the accessory metric; an inactive column is
skipped before its load, and the lines it shares with active columns are not counted); the clonal state has m = N, N - 1,
..., 2, for the other state the first round (m = N) and the bound rounds x N (N - 1) x 8 are given.  One expectation, reported and not
enforced: core metric after 100 generations, rounds_ms <= counts_ms of the same call."""
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
N, L, PAN, CG, GENERATIONS = 8192, 1200000, 8000, 2000, 100


def row(sim, state, metric, warmup, calls):
    # a state whose call takes seconds (the clonal one) is timed over fewer calls, which the row says (warmup, timed_calls)
    t0 = time.time()
    sim.upgma_tree(metric=metric)
    first_s = time.time() - t0
    if first_s > SLOW_CALL_S:                       # (the untimed first call is the warm-up then)
        warmup, calls = 0, 3 if first_s < VERY_SLOW_CALL_S else 1
    t = {"counts": [], "store": [], "rounds": [], "yard_counts": [], "yard_store": [], "yard_rounds": []}
    for k in range(warmup + calls):
        tree = sim.upgma_tree(metric=metric)
        mine = sim.core_genome.upgma_tree_timing()
        single = sim.linkage_tree(metric=metric)
        yard = sim.core_genome.linkage_tree_timing()
        if k >= warmup:
            for key, v in zip(("counts", "store", "rounds"), mine):
                t[key].append(v)
            for key, v in zip(("yard_counts", "yard_store", "yard_rounds"), yard):
                t[key].append(v)
    total = [a + b + c for a, b, c in zip(t["counts"], t["store"], t["rounds"])]
    yard_total = [a + b + c for a, b, c in zip(t["yard_counts"], t["yard_store"], t["yard_rounds"])]
    med = {key: float(np.median(v)) for key, v in t.items()}
    word = 8 * (2 if metric == "acc" else 1)
    clonal = tree.rounds == N - 1
    scan_bytes = word * sum(m * (m - 1) for m in range(2, N + 1)) if clonal else None     # the loads of the sums: about N^3 / 3 words
    out = {"state": state, "metric": metric, "counts_ms": round(med["counts"], 4), "store_ms": round(med["store"], 4),
           "rounds_ms": round(med["rounds"], 4), "rounds_ms_max": round(max(t["rounds"]), 4), "total_ms": round(float(np.median(total)), 4),
           "yardstick_counts_ms": round(med["yard_counts"], 4), "yardstick_store_ms": round(med["yard_store"], 4),
           "yardstick_rounds_ms": round(med["yard_rounds"], 4), "yardstick_total_ms": round(float(np.median(yard_total)), 4),
           "rounds": tree.rounds, "ms_per_round": round(med["rounds"] / tree.rounds, 5), "distinct_heights": tree.distinct_heights,
           "root": [tree.root_num, tree.root_den], "yardstick_rounds": single.rounds, "matrix_bytes": N * ((N + 63) // 64 * 64) * word,
           "first_round_scan_bytes": word * N * (N - 1), "scan_bytes_bound": word * N * (N - 1) * tree.rounds, "scan_bytes": scan_bytes,
           "scan_GBps": round(scan_bytes / med["rounds"] / 1e6, 1) if clonal else None,
           "rounds_within_counts": bool(med["rounds"] <= med["counts"]), "first_call_s": round(first_s, 3), "warmup": warmup, "timed_calls": calls}
    print(json.dumps(out), flush=True)
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, pan_genes=PAN, core_genes=CG, n_gen=GENERATIONS, max_distances=100))
    rows = [row(sim, "generation 0", m, WARMUP, CALLS) for m in ("core", "acc")]
    sim.run(GENERATIONS)
    sim.sync()
    rows += [row(sim, "generation %d" % GENERATIONS, m, WARMUP, CALLS) for m in ("core", "acc")]
    sim.close()
    met = next(r["rounds_within_counts"] for r in rows if r["state"] != "generation 0" and r["metric"] == "core")
    result = {"device": device, "pop_size": N, "core_size": L, "accessory_genes": PAN - CG, "warmup": WARMUP, "calls": CALLS,
              "rows": rows, "expectation_met": met}
    if out:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
