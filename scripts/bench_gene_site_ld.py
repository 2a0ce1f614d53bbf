#!/usr/bin/env python3
"""Device time of the gene-site association (ps_gene_site_ld, docs/GENE_SITE_ASSOCIATION.md) beside ps_locus_ld of the same
process at the same operand size.  Run it under a time limit:
    timeout -k 10 900 python scripts/bench_gene_site_ld.py [OUT.json] [OUT.md]
    timeout -k 10 900 python scripts/bench_gene_site_ld.py [OUT.json] --locus-ld 8192,22000

cfg2's shape (N = 1000, L = 1 200 000, G = 6000): a simulation runs 100 generations; then for (max_sites, max_genes) = (4096,
4096) and (16384, all polymorphic genes) ps_gene_site_ld and, alternating with it, ps_locus_ld on the core handle with max_loci =
Ms + Mg are launched 3 + 10 times on the evolved matrices and timed by their own HIP events (the four phases of
Population.gene_site_ld_timing() / locus_ld_timing(): select, pack, counts, statistics; medians).  --locus-ld runs ps_locus_ld
alone at the given max_loci and needs nothing but that entry: the figure of a library built before ps_gene_site_ld existed.  No
figure is a condition: the script reports."""
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
PHASES = ("select_ms", "pack_ms", "counts_ms", "stats_ms")
SHAPES = ((4096, 4096), (16384, 65536 - 16384))


def _phases(prefix, ms):
    med = np.median(np.array(ms), axis=0)
    row = {prefix + name: round(float(v), 4) for name, v in zip(PHASES, med)}
    row[prefix + "total_ms"] = round(float(med.sum()), 4)
    return row


def _locus_ld(sim, max_loci):
    ms = []
    for k in range(WARMUP + LAUNCHES):
        r = sim.locus_ld("core", max_loci=max_loci)
        if k >= WARMUP:
            ms.append(sim.core_genome.locus_ld_timing())
    return dict(_phases("ld_", ms), ld_loci=r.loci, ld_pairs=r.pairs)


def _table(rows):
    head = ("max_sites", "max_genes", "sites", "genes", "pairs", "select_ms", "pack_ms", "counts_ms", "stats_ms", "total_ms", "ld_loci",
            "ld_pairs", "ld_select_ms", "ld_pack_ms", "ld_counts_ms", "ld_stats_ms", "ld_total_ms")
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    lines += ["| " + " | ".join(str(r[h]) for h in head) + " |" for r in rows]
    return "\n".join(lines) + "\n"


def main():
    args = sys.argv[1:]
    only = [int(x) for x in args[args.index("--locus-ld") + 1].split(",")] if "--locus-ld" in args else None
    out = next((a for a in args if a.endswith(".json")), None)
    table = next((a for a in args if a.endswith(".md")), None)
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, pan_genes=G, n_gen=GENERATIONS, max_distances=100))
    sim.run(GENERATIONS)
    sim.sync()
    doc = {"script": "scripts/bench_gene_site_ld.py", "device": device, "pop_size": N, "core_size": L, "pan_genes": G,
           "generations": GENERATIONS, "warmup": WARMUP, "launches": LAUNCHES, "results": []}
    if only is not None:
        for max_loci in only:
            row = dict(max_loci=max_loci, **_locus_ld(sim, max_loci))
            doc["results"].append(row)
            print(json.dumps(row), flush=True)
    else:
        for max_sites, max_genes in SHAPES:
            r = sim.gene_site_ld(max_sites=max_sites, max_genes=max_genes)
            gs, ld = [], []
            for k in range(WARMUP + LAUNCHES):          # alternating: both see the same clocks and caches
                r = sim.gene_site_ld(max_sites=max_sites, max_genes=max_genes)
                t = sim.gene_site_ld_timing()
                sim.locus_ld("core", max_loci=r.sites + r.genes)
                if k >= WARMUP:
                    gs.append(t)
                    ld.append(sim.core_genome.locus_ld_timing())
            one = sim.locus_ld("core", max_loci=r.sites + r.genes)
            row = {"max_sites": max_sites, "max_genes": max_genes, "site_candidates": r.site_candidates, "gene_candidates": r.gene_candidates,
                   "sites": r.sites, "genes": r.genes, "pairs": r.pairs, "defined_pairs": r.defined_pairs, "strong_pairs": r.strong_pairs,
                   "genes_tagged": r.genes_tagged, "sites_tagging": r.sites_tagging, "mean_r2": r.mean_r2, "ld_loci": one.loci,
                   "ld_pairs": one.pairs}
            row.update(_phases("", gs))
            row.update(_phases("ld_", ld))
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
