#!/usr/bin/env python3
"""Device time of the core pass of the tree parsimony (ps_tree_parsimony, docs/TREE_PARSIMONY.md) beside the per-site counts
pass (ps_site_allele_counts), which reads the same N L bytes of the same handle.  Run it under a time limit:
    timeout -k 10 900 python scripts/bench_tree_parsimony.py [OUT.json]

cfg2 (N = 1000, L = 1 200 000, G = 6000) after 100 generations with the ancestry recorded.  Trees: the merges of the recorded
genealogy and the UPGMA tree of the core distance.  Per tree and form -- the up pass alone (no optional output) and up + down
(branch_changes) -- 3 warm-up calls, then 20 calls alternating call for call with ps_site_allele_counts; core_ms of
tree_parsimony_timing() against core_diversity_timing(), HIP events around each kernel.  One more call per tree with the gene
outputs gives gene_ms.  The medians, their ratio and GB/s over the N L bytes read are printed; no ratio is a condition."""
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


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, n_gen=GENERATIONS, max_distances=100))
    sim.record_ancestry(GENERATIONS)
    sim.run(GENERATIONS)
    sim.sync()
    core = sim.core_genome
    trees = {"genealogy": sim.genealogy().merges()[:2], "upgma": sim.upgma_tree().merges()}
    rows = []
    for name, (left, right) in trees.items():
        level_of, levels = pa.parsimony_schedule(left, right, N)
        widest = int(np.bincount(level_of).max())
        for form, kw in (("up", dict()), ("up+down", dict(branches=True))):
            pars_ms, counts_ms, sched_ms = [], [], []
            for k in range(WARMUP + CALLS):
                r = sim.tree_parsimony(left, right, **kw)
                t = sim.tree_parsimony_timing()
                core.site_allele_counts()
                c = core.core_diversity_timing()
                if k >= WARMUP:
                    pars_ms.append(t[1])
                    sched_ms.append(t[0])
                    counts_ms.append(c)
            pm, cm = float(np.median(pars_ms)), float(np.median(counts_ms))
            row = {"tree": name, "form": form, "merges": int(left.size), "levels": levels, "widest_level": widest, "trees": r.trees,
                   "total_changes": r.total_changes, "changed_sites": r.changed_sites, "homoplasic_sites": r.homoplasic_sites, "ci": r.ci,
                   "core_ms_median": round(pm, 4), "core_ms_min": round(min(pars_ms), 4), "core_ms_max": round(max(pars_ms), 4),
                   "schedule_ms_median": round(float(np.median(sched_ms)), 4), "site_allele_counts_ms_median": round(cm, 4),
                   "ratio": round(pm / cm, 3), "gb_per_s": round(N * L / pm / 1e6, 1), "site_allele_counts_gb_per_s": round(N * L / cm / 1e6, 1)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        g = sim.tree_parsimony(left, right, branches=True, genes=True)
        t = sim.tree_parsimony_timing()
        row = {"tree": name, "form": "genes", "genes": g.genes, "gene_total_gains": g.gene_total_gains, "gene_total_losses": g.gene_total_losses,
               "gene_ms": round(t[2], 4), "core_ms": round(t[1], 4), "schedule_ms": round(t[0], 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    sim.close()
    if out:
        with open(out, "w") as f:
            json.dump({"script": "scripts/bench_tree_parsimony.py", "device": device, "pop_size": N, "core_size": L, "generations": GENERATIONS,
                       "warmup": WARMUP, "calls": CALLS, "results": rows}, f, indent=1)


if __name__ == "__main__":
    main()
