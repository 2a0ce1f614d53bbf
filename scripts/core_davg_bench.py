#!/usr/bin/env python3
"""Core D-avg (average_distance of the core matrix, population.rs:753-784) per form:
python scripts/core_davg_bench.py [OUT.json] [case ...]

Cases: n1000 / n8192 (L = 1.2 M: whole matrix against banded), n65536 (L = 150 000: banded; the whole matrix does not fit
its cap), multi4 (ps_multi, four site shards of N = 8192, L = 1.2 M on device 0).  Times are the median wall time of the
synchronous call after one warm-up call (device work + one copy of N doubles to the host), like scripts/davg_bench.py.
The contraction's time does not depend on the values, so the matrices are the initial clonal ones (nothing to upload)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pansim_amd as pa  # noqa: E402

# plan_core_pairs' rate of the FP4 contraction over whole 256-tiles (pair-sites/s): the issue's estimates
RATE = 5.5e14


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 3) for t in ts]


def estimate_ms(N, L, whole):
    t = -(-N // 256)
    tiles = t * (t + 1) / 2 if whole else t * t
    return tiles * 65536.0 * L / RATE * 1e3


def single(N, L, forms, reps):
    pop = pa.Population(N, L, 4, True, 0.0, 0, 0)
    rows = []
    ref = None
    for name, form in forms:
        pop.set_tuning("core_davg_form", form)
        ms, all_ms = timed(pop.average_distance, reps)
        got = pop.average_distance()
        ref = got if ref is None else ref
        rows.append({"case": "N%d_L%d" % (N, L), "form": name, "ms": round(ms, 3), "runs_ms": all_ms,
                     "estimate_ms": round(estimate_ms(N, L, name == "whole"), 2), "equal_to_first_form": bool(np.array_equal(got, ref))})
        print(json.dumps(rows[-1]), flush=True)
    pop.close()
    return rows


def multi(N, L, K, reps):
    params = pa.make_params(pop_size=N, core_size=L, pan_genes=200, core_genes=20, n_gen=1, max_distances=100)
    ms_ = pa.MultiSimulation(params, K, devices=[0] * K)
    ms, all_ms = timed(lambda: ms_.average_distance(True), reps)
    row = {"case": "multi%d_N%d_L%d" % (K, N, L), "form": "banded, %d shards on one GPU" % K, "ms": round(ms, 3), "runs_ms": all_ms,
           "estimate_ms": round(estimate_ms(N, L, False), 2)}
    print(json.dumps(row), flush=True)
    ms_.close()
    return [row]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1].endswith(".json") else None
    cases = [a for a in sys.argv[1:] if not a.endswith(".json")] or ["n1000", "n8192", "n65536", "multi4"]
    both = (("whole", 1), ("banded", 2))
    rows = []
    for c in cases:
        if c == "n1000":
            rows += single(1000, 1200000, both, 5)
        elif c == "n8192":
            rows += single(8192, 1200000, both, 3)
        elif c == "n65536":
            rows += single(65536, 150000, (("banded", 2),), 2)
        elif c == "multi4":
            rows += multi(8192, 1200000, 4, 3)
        else:
            raise SystemExit("unknown case %s" % c)
    if out:
        with open(out, "w") as f:
            json.dump({"script": "scripts/core_davg_bench.py", "rate_for_estimates": RATE, "results": rows}, f, indent=1)


if __name__ == "__main__":
    main()
