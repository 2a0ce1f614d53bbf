#!/usr/bin/env python3
"""Device time of one pass of the parsimony tree search (ps_tree_nni_deltas, docs/PARSIMONY_SEARCH.md) beside the up + down pass
of the tree parsimony on the same tree (ps_tree_parsimony with branch_changes), and what the search does to the UPGMA and the
neighbour-joining tree.  Run it under a time limit:
    timeout -k 10 900 python scripts/bench_parsimony_search.py [OUT.json]

cfg2 (N = 1000, L = 1 200 000, G = 6000) after 100 generations with the ancestry recorded.  Per start tree, in its canonical
form: 3 warm-up calls, then 20 calls of nni_deltas() alternating call for call with tree_parsimony(branches=True); pass_ms of
tree_nni_timing() against core_ms of tree_parsimony_timing(), HIP events around each kernel.  Then one tree_nni() with its
rounds, passes, rollbacks, total changes and pass_ms per pass, and tree_compare() of the start and the end tree against the
recorded genealogy (values: the merge ranks of the canonical lists).  The medians and their ratio are printed; no ratio is a
condition."""
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
COMPARE = ("shared_clades", "clades_a", "clades_b", "rf_distance", "clade_recall", "clade_precision", "triplet_recall", "triplet_precision",
           "cophenetic_r")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, n_gen=GENERATIONS, max_distances=100))
    sim.record_ancestry(GENERATIONS)
    sim.run(GENERATIONS)
    sim.sync()
    core, genealogy = sim.core_genome, sim.genealogy()
    trees = {"upgma": sim.upgma_tree().merges(), "nj": sim.neighbour_joining().merges()}
    rows = []
    for name, (left, right) in trees.items():
        left, right = pa.merges_canonical(left, right, N)
        level_of, levels = pa.parsimony_schedule(left, right, N)
        nni_ms, pars_ms, sched_ms = [], [], []
        for k in range(WARMUP + CALLS):
            total, delta = core.nni_deltas(left, right)
            t = core.tree_nni_timing()
            sim.tree_parsimony(left, right, branches=True)
            p = sim.tree_parsimony_timing()
            if k >= WARMUP:
                nni_ms.append(t[1])
                sched_ms.append(t[0])
                pars_ms.append(p[1])
        nm, pm = float(np.median(nni_ms)), float(np.median(pars_ms))
        row = {"tree": name, "form": "pass", "merges": int(left.size), "levels": levels, "widest_level": int(np.bincount(level_of).max()),
               "total_changes": total, "improving_candidates": int((delta < 0).sum()), "pass_ms_median": round(nm, 4),
               "pass_ms_min": round(min(nni_ms), 4), "pass_ms_max": round(max(nni_ms), 4), "schedule_ms_median": round(float(np.median(sched_ms)), 4),
               "tree_parsimony_up_down_ms_median": round(pm, 4), "ratio": round(nm / pm, 3), "gb_per_s": round(N * L / nm / 1e6, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        got = sim.tree_nni(left, right)
        t = sim.tree_nni_timing()
        row = {"tree": name, "form": "search", "rounds": got.rounds, "passes": got.passes, "rollbacks": got.rollbacks, "moves": got.n_moves,
               "local_optimum": got.local_optimum, "start_changes": got.start_changes, "total_changes": got.total_changes,
               "min_changes": got.min_changes, "pass_ms_sum": round(t[1], 3), "pass_ms_per_pass": round(t[1] / got.passes, 4),
               "schedule_ms_sum": round(t[0], 3)}
        for which, tree in (("start", (left, right)), ("end", got.merges())):
            c = sim.tree_compare(genealogy, tree)
            row[which] = {f: (round(getattr(c, f), 6) if isinstance(getattr(c, f), float) else getattr(c, f)) for f in COMPARE}
        rows.append(row)
        print(json.dumps(row), flush=True)
    sim.close()
    if out:
        with open(out, "w") as f:
            json.dump({"script": "scripts/bench_parsimony_search.py", "device": device, "pop_size": N, "core_size": L, "generations": GENERATIONS,
                       "warmup": WARMUP, "calls": CALLS, "results": rows}, f, indent=1)


if __name__ == "__main__":
    main()
