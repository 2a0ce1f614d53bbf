#!/usr/bin/env python3
"""Device time of the tree comparison (docs/TREE_COMPARISON.md).  Run it under a time limit:
    timeout -k 10 900 python scripts/bench_tree_compare.py [OUT.json]

(a) The cfg5 population (N = 8192, L = 1 200 000, G = 6000) with 100 recorded generations: the genealogy against the UPGMA tree
of the core distance.  3 warm-up calls, then 10 calls read through ps_tree_compare_timing (HIP events), alternating call for
call with ps_sim_clock_histogram on the same simulation.  The yardstick is the clock histogram's group 1 (comb + table +
binning), which walks the same pairs with 2 table loads per pair where tree_pair_kernel issues about 12: both medians and their
ratio are reported, there is no target.
(b) N = 16384 (2^27 pairs, a 512 MB rank table outside the L2) on a bare handle, a random tree against a random tree, with and
without triplets: 2 warm-up calls, then 5."""
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

WARMUP, CALLS = 3, 10
N, L, PAN, CG, GENERATIONS = 8192, 1200000, 8000, 2000, 100
BIG, BIG_WARMUP, BIG_CALLS = 16384, 2, 5


def med(v):
    return round(float(np.median(v)), 4)


def cfg5():
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, pan_genes=PAN, core_genes=CG, n_gen=GENERATIONS, max_distances=100))
    sim.record_ancestry(GENERATIONS)
    sim.run(GENERATIONS)
    g, u = sim.genealogy(), sim.upgma_tree()
    a, b = g.merges(), (*u.merges(), u.levels())
    t = {"tables": [], "pairs": [], "yard_counts": [], "yard_bin": []}
    for call in range(WARMUP + CALLS):
        got = sim.tree_compare(a, b)
        mine = sim.tree_compare_timing()
        clock = sim.clock_histogram()
        yard = sim.clock_histogram_timing()
        if call >= WARMUP:
            for key, value in zip(t, mine + yard):
                t[key].append(value)
    sim.close()
    # the two read-outs saw the same pairs: those beyond the record are the ones the genealogy does not join
    assert got.pairs == clock.pairs and got.joined_b_only + got.joined_neither == clock.beyond_pairs and int(got.joint.sum()) == got.pairs
    out = {"part": "cfg5", "pop_size": N, "merges_a": got.merges_a, "merges_b": got.merges_b, "joined_both": got.joined_both,
           "cophenetic_r": got.cophenetic_r, "triplet_recall": got.triplet_recall, "clade_recall": got.clade_recall,
           "tables_ms": med(t["tables"]), "pairs_ms": med(t["pairs"]), "pairs_ms_max": round(max(t["pairs"]), 4),
           "clock_counts_ms": med(t["yard_counts"]), "clock_comb_table_binning_ms": med(t["yard_bin"]),
           "ratio_pairs": round(float(np.median(t["pairs"]) / np.median(t["yard_bin"])), 3),
           "ratio_call": round(float((np.median(t["pairs"]) + np.median(t["tables"])) / np.median(t["yard_bin"])), 3)}
    print(json.dumps(out), flush=True)
    return out


def random_tree(rng, n):
    """n - 1 merges of two random roots each"""
    roots, left, right = list(range(n)), [], []
    for k in range(n - 1):
        i, j = (int(x) for x in rng.choice(len(roots), 2, replace=False))
        left.append(roots[i])
        right.append(roots[j])
        roots[i] = n + k
        roots[j] = roots[-1]
        roots.pop()
    return np.array(left, np.uint32), np.array(right, np.uint32)


def largest():
    rng = np.random.default_rng(1)
    a, b = random_tree(rng, BIG), random_tree(rng, BIG)
    h = pa.Population(BIG, 16, 4, True, 0.0, 0, 0)
    rows = []
    for triplets in (True, False):
        t = {"tables": [], "pairs": []}
        for call in range(BIG_WARMUP + BIG_CALLS):
            got = h.tree_compare(a, b, triplets=triplets)
            if call >= BIG_WARMUP:
                for key, value in zip(t, h.tree_compare_timing()):
                    t[key].append(value)
        assert got.joined_both == got.pairs == BIG * (BIG - 1) // 2
        rows.append({"part": "largest", "pop_size": BIG, "triplets": triplets, "pairs": got.pairs, "tables_ms": med(t["tables"]),
                     "pairs_ms": med(t["pairs"]), "pairs_ms_max": round(max(t["pairs"]), 4)})
        print(json.dumps(rows[-1]), flush=True)
    h.close()
    return rows


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    result = {"device": device, "warmup": WARMUP, "calls": CALLS, "rows": [cfg5()] + largest()}
    if out:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
