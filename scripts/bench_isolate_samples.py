#!/usr/bin/env python3
"""Isolate samples (ps_sim_subset, docs/ISOLATE_SAMPLES.md) beside the counts pass of ps_core_diversity on the same source handle
and beside the host route they replace (read_matrix()[rows] into a fresh Population with load_matrix).  Run it under a time limit:
    timeout -k 10 1100 python scripts/bench_isolate_samples.py [OUT.json] [OUT.md] [--shapes cfg2,cfg5] [--host-calls-large K]

Two shapes: cfg2 (N = 1000, L = 1 200 000, G = 6000) after 100 generations and the cfg5 population (N = 8192, the same L and G)
after 4.  For n in {100, 500, N} rows drawn with repeats, 3 + 10 calls of Simulation.subset(rows), each alternating with
ps_core_diversity on the core handle and with the host route; medians.  Reported: the device time of the core gather
(Population.subset_timing() of the core sample), its bytes/s from L x (bytes read + pitch_out) -- bytes read = the source pitch in
the LDS form, min(32 n, pitch) in the direct form (n sectors of 32 bytes) --, the bytes/s of the counts pass over L x pitch, the wall time of the whole
subset call and of the host route.  The host route of the large shape moves 2 x 9.8 GB per call: it is run --host-calls-large
times (default 2) per sample size instead of 13, and the table says so.  A second table scans the form switch: the device time
of the gather with the tuning key "gather_form" forced to 1 (LDS) and 2 (direct) over small n.

One figure is a condition: the whole subset call must be faster than the host route of the same run; the script exits with
status 1 if it is not."""
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

WARMUP, LAUNCHES = 3, 10
L, G = 1200000, 6000
SHAPES = {"cfg2": dict(pop_size=1000, generations=100), "cfg5": dict(pop_size=8192, generations=4)}
SCAN = (4, 8, 16, 32, 48, 64, 96, 128, 192, 256, 512)
HEAD = ("shape", "n", "form", "gather_ms", "gather_TBps", "counts_ms", "counts_TBps", "gather_over_counts", "acc_gather_ms", "subset_wall_ms",
        "host_route_ms", "host_calls", "speedup")
SCAN_HEAD = ("shape", "n", "chosen", "lds_ms", "direct_ms")


def _table(head, rows):
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    lines += ["| " + " | ".join(str(r[h]) for h in head) + " |" for r in rows]
    return "\n".join(lines) + "\n"


def _pitch(n):
    return (n + 127) // 128 * 128


def _direct(pitch, n):
    """the library's choice (core_gather_direct of pansim_amd/csrc/sample_plan.h)"""
    return pitch > 65536 or 48 * n < pitch


def _host_route(sim, rows):
    """what the call replaces: both matrices to the host, indexed there, loaded into fresh handles"""
    t0 = time.perf_counter()
    p = sim.params
    cm, am = sim.core_genome.read_matrix()[rows], sim.pan_genome.read_matrix()[rows]
    core = pa.Population(rows.size, cm.shape[1], 4, True, 0.0, p.seed, p.core_genes)
    core.load_matrix(cm)
    acc = pa.Population(rows.size, am.shape[1], 2, False, 0.5, p.seed, p.core_genes)
    acc.load_matrix(am)
    ms = (time.perf_counter() - t0) * 1e3
    core.close()
    acc.close()
    return ms


def _subset(sim, rows):
    t0 = time.perf_counter()
    core, acc = sim.subset(rows)
    wall = (time.perf_counter() - t0) * 1e3
    out = wall, core.subset_timing(), acc.subset_timing()
    core.close()
    acc.close()
    return out


def main():
    args = sys.argv[1:]
    out = next((a for a in args if a.endswith(".json")), None)
    table = next((a for a in args if a.endswith(".md")), None)
    shapes = args[args.index("--shapes") + 1].split(",") if "--shapes" in args else list(SHAPES)
    host_large = int(args[args.index("--host-calls-large") + 1]) if "--host-calls-large" in args else 2
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    doc = {"script": "scripts/bench_isolate_samples.py", "device": device, "core_size": L, "pan_genes": G, "warmup": WARMUP, "launches": LAUNCHES,
           "results": [], "form_scan": []}
    slower = []
    for shape in shapes:
        N, gens = SHAPES[shape]["pop_size"], SHAPES[shape]["generations"]
        sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, pan_genes=G, n_gen=gens, max_distances=100))
        sim.run(gens)
        sim.sync()
        pitch = _pitch(N)
        rng = np.random.default_rng(N)
        for n in (100, 500, N):
            rows = rng.integers(0, N, n).astype(np.uint32)
            host_calls = WARMUP + LAUNCHES if N <= 1000 else host_large
            wall, gather, acc_ms, counts, host = [], [], [], [], []
            for k in range(WARMUP + LAUNCHES):          # alternating: all three see the same clocks and caches
                w, g, a = _subset(sim, rows)
                sim.core_genome.core_diversity()
                c = sim.core_genome.core_diversity_timing()
                if k < host_calls:
                    h = _host_route(sim, rows)
                    if k >= WARMUP or host_calls < WARMUP + LAUNCHES:
                        host.append(h)
                if k >= WARMUP:
                    wall.append(w)
                    gather.append(g)
                    acc_ms.append(a)
                    counts.append(c)
            g_ms, c_ms, w_ms, h_ms = (float(np.median(x)) for x in (gather, counts, wall, host))
            direct = _direct(pitch, n)
            read = min(32 * n, pitch) if direct else pitch
            g_bytes, c_bytes = L * (read + _pitch(n)), L * pitch
            row = dict(shape=shape, n=n, form="direct" if direct else "lds", gather_ms=round(g_ms, 4), gather_TBps=round(g_bytes / g_ms / 1e9, 3),
                       counts_ms=round(c_ms, 4), counts_TBps=round(c_bytes / c_ms / 1e9, 3),
                       gather_over_counts=round((g_bytes / g_ms) / (c_bytes / c_ms), 3), acc_gather_ms=round(float(np.median(acc_ms)), 4),
                       subset_wall_ms=round(w_ms, 3), host_route_ms=round(h_ms, 1), host_calls=len(host), speedup=round(h_ms / w_ms, 1))
            doc["results"].append(row)
            print(json.dumps(row), flush=True)
            if not w_ms < h_ms:
                slower.append(row)
        for n in SCAN:
            rows = rng.integers(0, N, n).astype(np.uint32)
            ms = {}
            for form in (1, 2):
                sim.core_genome.set_tuning("gather_form", form)
                t = []
                for k in range(2 + 5):
                    core, _ = sim.subset(rows)
                    if k >= 2:
                        t.append(core.subset_timing())
                    core.close()
                    _.close()
                ms[form] = float(np.median(t))
            sim.core_genome.set_tuning("gather_form", 0)
            row = dict(shape=shape, n=n, chosen="direct" if _direct(pitch, n) else "lds", lds_ms=round(ms[1], 4), direct_ms=round(ms[2], 4))
            doc["form_scan"].append(row)
            print(json.dumps(row), flush=True)
        sim.close()
    if table:
        with open(table, "w") as f:
            f.write(_table(HEAD, doc["results"]) + "\n" + _table(SCAN_HEAD, doc["form_scan"]))
    print(json.dumps({k: v for k, v in doc.items() if k not in ("results", "form_scan")}), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
    if slower:
        print("the subset call is not faster than the host route: %s" % json.dumps(slower), flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
