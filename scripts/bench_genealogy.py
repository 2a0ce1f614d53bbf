#!/usr/bin/env python3
"""Device time of the clock histogram and the cost of recording the ancestry (docs/GENEALOGY.md).  Run it under a time limit:
    timeout -k 10 900 python scripts/bench_genealogy.py [OUT.json]

(a) The cfg5 population (N = 8192, L = 1 200 000, G = 6000) with 100 recorded generations, core metric: 3 warm-up calls, then
10 calls read through ps_clock_histogram_timing (HIP events), alternating call for call with ps_distance_histogram on the same
handles.  The condition, the sibling's own: group 1 (comb + table + binning) is at most 5 % of the call's device time.
(b) cfg2 (N = 1000, L = 1 200 000, G = 6000), 1000 generations per run, generations/s with recording off and on (capacity
1000), alternating, five runs each, every run a fresh simulation of the same seed.  The yardstick is the off runs; the margin
is their spread (max - min); the on median should lie within it below the off median.  Both medians and the spread are
reported whatever the outcome."""
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

WARMUP, CALLS, SHARE = 3, 10, 0.05
N, L, PAN, CG, GENERATIONS = 8192, 1200000, 8000, 2000, 100
RUNS, RUN_GENERATIONS = 5, 1000


def clock():
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, pan_genes=PAN, core_genes=CG, n_gen=GENERATIONS, max_distances=100))
    sim.record_ancestry(GENERATIONS)
    sim.run(GENERATIONS)
    sim.sync()
    t = {"counts": [], "bin": [], "yard_counts": [], "yard_bin": []}
    for call in range(WARMUP + CALLS):
        got = sim.clock_histogram()
        mine = sim.clock_histogram_timing()
        hist = sim.distance_histogram()
        yard = sim.core_genome.distance_histogram_timing()
        if call >= WARMUP:
            for key, value in zip(("counts", "bin", "yard_counts", "yard_bin"), mine + yard):
                t[key].append(value)
    g = sim.genealogy()
    sim.close()
    # the two read-outs saw the same pairs: the core sums agree, and every pair is in a bin
    assert got.num_sum == hist.core_d_sum and got.binned_pairs == got.pairs == hist.pairs and int(got.joint.sum()) == got.pairs
    med = {key: float(np.median(v)) for key, v in t.items()}
    share = med["bin"] / (med["counts"] + med["bin"])
    out = {"part": "clock_histogram", "pop_size": N, "depth": g.depth, "roots": g.roots, "tmrca": g.tmrca, "beyond_pairs": got.beyond_pairs,
           "counts_ms": round(med["counts"], 4), "comb_table_binning_ms": round(med["bin"], 4), "comb_table_binning_ms_max": round(max(t["bin"]), 4),
           "share_of_call": round(share, 5), "histogram_counts_ms": round(med["yard_counts"], 4),
           "histogram_binning_ms": round(med["yard_bin"], 4), "limit": SHARE, "within_limit": bool(share <= SHARE)}
    print(json.dumps(out), flush=True)
    return out


def recording():
    rate = {False: [], True: []}
    for run in range(2 * RUNS + 2):                      # (one unrecorded pair of warm-up runs first)
        on = run % 2 == 1
        sim = pa.Simulation(pa.make_params(pop_size=1000, core_size=L, pan_genes=PAN, core_genes=CG, n_gen=RUN_GENERATIONS, max_distances=100))
        if on:
            sim.record_ancestry(RUN_GENERATIONS)
        sim.sync()
        t0 = time.perf_counter()
        sim.run(RUN_GENERATIONS)
        sim.sync()
        dt = time.perf_counter() - t0
        if on:
            assert sim.genealogy().depth == RUN_GENERATIONS
        sim.close()
        if run >= 2:
            rate[on].append(RUN_GENERATIONS / dt)
    off, on = float(np.median(rate[False])), float(np.median(rate[True]))
    spread = max(rate[False]) - min(rate[False])
    out = {"part": "recording", "pop_size": 1000, "generations": RUN_GENERATIONS, "runs": RUNS,
           "off_generations_per_s": [round(x, 1) for x in rate[False]], "on_generations_per_s": [round(x, 1) for x in rate[True]],
           "off_median": round(off, 1), "on_median": round(on, 1), "off_spread": round(spread, 1), "on_minus_off": round(on - off, 1),
           "within_spread": bool(on >= off - spread)}
    print(json.dumps(out), flush=True)
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    rows = [clock(), recording()]
    ok = rows[0]["within_limit"] and rows[1]["within_spread"]
    result = {"device": device, "warmup": WARMUP, "calls": CALLS, "rows": rows, "ok": ok}
    if out:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
