#!/usr/bin/env python3
"""What per-site weights cost: python scripts/site_weights_cost.py [OUT.json]

cfg2 (N = 1000, L = 1.2 M): the fused sweep by HIP events (ps_sim_sweep_timing) with uniform rates and with a smooth
non-uniform core weight vector of the same mean rate; cfg3 (HR = HGT = 0.5): generations/s with uniform and non-uniform gene
weights (the HGT chain decides that loop).  Yardstick: the uniform run of the same build in the same process; the variants
alternate, three rounds each."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pansim_amd as pa  # noqa: E402

STEPS, WARM = 1000, 200


def run(sim):
    sim.run(WARM)
    sim.sync()
    sim.enable_timing(True)
    sim.sweep_timing(True)
    t0 = time.perf_counter()
    sim.run(STEPS)
    sim.sync()
    dt = time.perf_counter() - t0
    n, total_ms, _ = sim.sweep_timing(True)
    sim.enable_timing(False)
    return {"generations_per_s": round(STEPS / dt, 1), "sweep_ms": round(total_ms / max(n, 1), 4), "sweep_form": sim.core_genome.last_sweep_form()}


def variants(label, kw, what):
    sims = {}
    for name in ("uniform", "weighted"):
        sim = pa.Simulation(pa.make_params(seed=0, n_gen=10 ** 6, max_distances=100, device=0, **kw))
        p, d = sim.params, sim.derived
        if name == "weighted" and what == "core":
            sim.set_site_weights((1.0 + 0.5 * np.sin(np.arange(p.core_size) / 3000.0)).astype(np.float32))
        if name == "weighted" and what == "genes":
            rng = np.random.default_rng(1)
            w = np.zeros((d.n_comp, d.pan_size), np.float32)
            for c in range(d.n_comp):          # the compartments' own ranges, non-uniform inside
                w[c, d.comp_begin[c]:d.comp_end[c]] = 0.25 + rng.random(d.comp_end[c] - d.comp_begin[c])
            sim.set_site_weights(None, w, w)
        sims[name] = sim
    rows = []
    for rnd in range(3):
        for name, sim in sims.items():
            rows.append(dict(run(sim), workload=label, variant=name, round=rnd))
            print(json.dumps(rows[-1]), flush=True)
    for sim in sims.values():
        sim.close()
    return rows


def main():
    rows = variants("cfg2", dict(pop_size=1000, core_size=1200000, pan_genes=6000, core_genes=2000), "core")
    rows += variants("cfg3", dict(pop_size=1000, core_size=1200000, pan_genes=6000, core_genes=2000, HR_rate=0.5, HGT_rate=0.5), "genes")
    if len(sys.argv) > 1:
        json.dump(rows, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
