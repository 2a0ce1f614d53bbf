#!/usr/bin/env python3
"""Device time of the joint distance histogram (ps_sim_distance_histogram, docs/DISTANCE_HISTOGRAM.md) at the cfg5
population: N = 8192, L = 1 200 000, G = 6000, 64 x 64 bins.  Run it under a time limit:
    timeout -k 10 900 python scripts/bench_distance_histogram.py [OUT.json]

Three rows, in one process: generation 0 with an explicit span (every pair in one bin: the worst case of the LDS
atomics), the population after 100 generations with an explicit span, and the same state with the automatic span (one
band here, so one more pass over the counts and no second contraction).  Per row 3 warm-up calls, then 10 calls read
through ps_distance_histogram_timing (HIP events): the count kernels of both matrices, and the binning kernel.  The
binning kernel reads 6 bytes per pair of the rectangles it touches (whole 256-column chunks from the diagonal's on); the
fraction is of the 8 TB/s HBM peak.  The condition: binning takes at most 5 % of the call's device time."""
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

HBM_PEAK = 8.0e12
WARMUP, CALLS = 3, 10
N, L, PAN, CG, BINS, GENERATIONS = 8192, 1200000, 8000, 2000, 64, 100


def bytes_read(n):
    chunks = (n + 255) // 256
    return sum((chunks - (i + 1) // 256) * 256 * 6 for i in range(n - 1))


def row(sim, name, span):
    counts, binning = [], []
    for k in range(WARMUP + CALLS):
        h = sim.distance_histogram(BINS, BINS, core_span=span)
        if k >= WARMUP:
            c, b = sim.core_genome.distance_histogram_timing()
            counts.append(c)
            binning.append(b)
    c, b = float(np.median(counts)), float(np.median(binning))
    nbytes = bytes_read(N) * (2 if span == 0 else 1)
    out = {"state": name, "core_span": h.core_span, "automatic": span == 0, "counts_ms": round(c, 4), "binning_ms": round(b, 4),
           "binning_ms_max": round(max(binning), 4), "binning_share": round(b / (b + c), 5), "bytes_read": nbytes,
           "fraction_of_8_tb_per_s": round(nbytes / (b * 1e-3) / HBM_PEAK, 4), "non_empty_bins": int((h.joint != 0).sum()),
           "core_d_max": h.core_d_max, "within_5_percent": bool(b <= 0.05 * (b + c))}
    print(json.dumps(out), flush=True)
    return out, h


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, pan_genes=PAN, core_genes=CG, n_gen=GENERATIONS, max_distances=100))
    rows = [row(sim, "generation 0", L // 100)[0]]
    sim.run(GENERATIONS)
    sim.sync()
    auto, h = row(sim, "generation %d" % GENERATIONS, 0)
    rows += [row(sim, "generation %d" % GENERATIONS, h.core_span)[0], auto]
    sim.close()
    ok = all(r["within_5_percent"] for r in rows)
    result = {"device": device, "pop_size": N, "core_size": L, "accessory_genes": PAN - CG, "bins": [BINS, BINS], "warmup": WARMUP,
              "calls": CALLS, "rows": rows, "ok": ok}
    if out:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
