#!/usr/bin/env python3
"""Device time of the bootstrap support of the three trees (ps_sim_bootstrap_support, docs/BOOTSTRAP_SUPPORT.md) at the cfg2
shape: N = 1000, L = 1 200 000, after 20 generations.  Run it under a time limit (profiles/bootstrap_support.md has what it
took on one MI355X):
    timeout -k 10 600 python scripts/bench_bootstrap_support.py [OUT.json]

Per method an untimed first call of both entries, then ROUNDS rounds that alternate one bootstrap_support(replicates=REPLICATES)
with one call of the method's own tree on the same handles.  The bootstrap's three groups come from ps_bootstrap_timing (HIP
events, summed over the replicates; divided by REPLICATES here), the yardstick's three from the method's own *_timing entry.
What is reported per method, medians over the rounds: the lists, the operands (pack + counts + store) and the trees per replicate;
the yardstick's counts, store and tree; `operands_ratio` = the operands of a replicate over the yardstick's counts + store.  The
tree's own entry does not time the pack of the unresampled strings, so the ratio holds the whole resampled pack against no pack
at all: it is an upper bound of the ratio to "unresampled pack + counts".  Last, the operands of one UPGMA replicate whose list
is every site once (the matrix's own strings, gathered through the list) beside those of a drawn replicate."""
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

N, L, PAN, CG, GENERATIONS = 1000, 1200000, 6000, 2000, 20
REPLICATES, ROUNDS = 10, 5


def row(sim, method):
    own = {"linkage": sim.linkage_tree, "upgma": sim.upgma_tree, "nj": sim.neighbour_joining}[method]
    own_timing = getattr(sim.core_genome, {"linkage": "linkage_tree_timing", "upgma": "upgma_tree_timing", "nj": "neighbour_joining_timing"}[method])
    sim.bootstrap_support(method=method, replicates=2, seed=1)
    own()
    t = {k: [] for k in ("lists", "operands", "trees", "yard_counts", "yard_store", "yard_tree")}
    for r in range(ROUNDS):
        res = sim.bootstrap_support(method=method, replicates=REPLICATES, seed=100 + r)
        for key, v in zip(("lists", "operands", "trees"), sim.bootstrap_support_timing()):
            t[key].append(v / REPLICATES)
        own()
        for key, v in zip(("yard_counts", "yard_store", "yard_tree"), own_timing()):
            t[key].append(v)
    med = {k: float(np.median(v)) for k, v in t.items()}
    yard_operands = med["yard_counts"] + med["yard_store"]
    out = {"method": method, "replicates": REPLICATES, "rounds": ROUNDS,
           "lists_ms_per_replicate": round(med["lists"], 4), "operands_ms_per_replicate": round(med["operands"], 4),
           "trees_ms_per_replicate": round(med["trees"], 4),
           "replicate_ms": round(med["lists"] + med["operands"] + med["trees"], 4),
           "yardstick_counts_ms": round(med["yard_counts"], 4), "yardstick_store_ms": round(med["yard_store"], 4),
           "yardstick_tree_ms": round(med["yard_tree"], 4), "yardstick_total_ms": round(yard_operands + med["yard_tree"], 4),
           "operands_ratio": round(med["operands"] / yard_operands, 3),
           "replicate_over_yardstick": round((med["lists"] + med["operands"] + med["trees"]) / (yard_operands + med["yard_tree"]), 3),
           "support_sum": res.support_sum, "supported_70": res.supported_70}
    print(json.dumps(out), flush=True)
    return out


def identity_list(sim):
    """the resampled pack against itself without repeats: one replicate whose list is every site once, i.e. the matrix's own
    strings through the list, against the drawn replicate; UPGMA, operands group only"""
    sites = np.arange(L, dtype=np.uint32).reshape(1, L)
    t = {"identity": [], "drawn": []}
    for r in range(ROUNDS):
        sim.bootstrap_support(method="upgma", replicates=1, sites=sites)
        t["identity"].append(sim.bootstrap_support_timing()[1])
        sim.bootstrap_support(method="upgma", replicates=1, seed=r)
        t["drawn"].append(sim.bootstrap_support_timing()[1])
    out = {"operands_ms_identity_list": round(float(np.median(t["identity"])), 4), "operands_ms_drawn_list": round(float(np.median(t["drawn"])), 4)}
    print(json.dumps(out), flush=True)
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, pan_genes=PAN, core_genes=CG, n_gen=GENERATIONS, max_distances=100))
    sim.run(GENERATIONS)
    sim.sync()
    rows = [row(sim, m) for m in ("linkage", "upgma", "nj")]
    ident = identity_list(sim)
    sim.close()
    result = {"device": device, "pop_size": N, "core_size": L, "generations": GENERATIONS, "rows": rows, "pack": ident}
    if out:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
