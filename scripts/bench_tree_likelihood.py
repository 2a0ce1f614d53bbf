#!/usr/bin/env python3
"""Device time of one pass of the Jukes-Cantor likelihood of a tree (ps_tree_likelihood, docs/TREE_LIKELIHOOD.md), the up pass
alone and with the down pass, beside the up + down pass of the tree parsimony on the same tree (ps_tree_parsimony with
branch_changes: one level-scheduled pass over the same bytes), and what the maximum-likelihood branch lengths do to the UPGMA and
the neighbour-joining tree.  Run it under a time limit:
    timeout -k 10 1100 python scripts/bench_tree_likelihood.py [OUT.json]

cfg2 (N = 1000, L = 1 200 000, G = 6000) after 100 generations with the ancestry recorded.  Per tree, in its canonical form, with
the Jukes-Cantor correction of its parsimony changes as lengths: 3 warm-up calls, then 20 calls of tree_likelihood() and 20 of
tree_likelihood(derivatives=True), each alternating call for call with tree_parsimony(branches=True); pass_ms of
tree_likelihood_timing() against core_ms of tree_parsimony_timing(), HIP events around each kernel.  Then one tree_ml_lengths() with
its rounds, passes, rollbacks and lnL, and tree_compare() of the cophenetic heights of the maximum-likelihood phylogram and of the
parsimony phylogram against the recorded genealogy (values: the height of every merge above its furthest leaf, scaled to the
values tree_compare takes).  The medians and their ratios are printed; no ratio is a condition."""
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
COMPARE = ("shared_clades", "clade_recall", "triplet_recall", "triplet_precision", "cophenetic_r")


def heights(left, right, length, n):
    """uint32 per merge, as tree_compare takes values: the largest sum of branch lengths down to a leaf (so a parent is at least as
    high as its children), scaled to 1 .. 2^18 - 1 of the root's"""
    h = np.zeros(n + left.size)
    for k in range(left.size):
        a, b = int(left[k]), int(right[k])
        h[n + k] = max(h[a] + length[a], h[b] + length[b])
    return (1 + np.round(h[n:] / max(h[-1], 1e-300) * 262142.0)).astype(np.uint32)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, n_gen=GENERATIONS, max_distances=100))
    sim.record_ancestry(GENERATIONS)
    sim.run(GENERATIONS)
    sim.sync()
    genealogy = sim.genealogy()
    trees = {"upgma": sim.upgma_tree().merges(), "nj": sim.neighbour_joining().merges()[:2]}
    rows = []
    for name, (left, right) in trees.items():
        left, right = pa.merges_canonical(left, right, N)
        level_of, levels = pa.parsimony_schedule(left, right, N)
        pars = sim.tree_parsimony(left, right, branches=True)
        start = pa.jc_lengths_from_changes(pars.branch_changes, L)
        for form, kw in (("up", {}), ("up_down", dict(derivatives=True))):
            lik_ms, pars_ms, sched_ms, red_ms = [], [], [], []
            for k in range(WARMUP + CALLS):
                got = sim.tree_likelihood(left, right, start, **kw)
                t = sim.tree_likelihood_timing()
                sim.tree_parsimony(left, right, branches=True)
                p = sim.tree_parsimony_timing()
                if k >= WARMUP:
                    lik_ms.append(t[1])
                    sched_ms.append(t[0])
                    red_ms.append(t[2])
                    pars_ms.append(p[1])
            lm, pm = float(np.median(lik_ms)), float(np.median(pars_ms))
            row = {"tree": name, "form": form, "merges": int(left.size), "levels": levels, "widest_level": int(np.bincount(level_of).max()),
                   "lnl": got.lnl, "pass_ms_median": round(lm, 3), "pass_ms_min": round(min(lik_ms), 3), "pass_ms_max": round(max(lik_ms), 3),
                   "schedule_ms_median": round(float(np.median(sched_ms)), 4), "reduce_ms_median": round(float(np.median(red_ms)), 4),
                   "tree_parsimony_up_down_ms_median": round(pm, 3), "ratio": round(lm / pm, 2), "sites_per_us": round(L / lm / 1e3, 2)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        ml = sim.tree_ml_lengths(left, right, start)
        t = sim.tree_likelihood_timing()
        row = {"tree": name, "form": "ml_lengths", "rounds": ml.rounds, "passes": ml.passes, "rollbacks": ml.rollbacks, "converged": ml.converged,
               "start_lnl": ml.start_lnl, "lnl": ml.lnl, "tree_length_start": float(np.clip(start[:-1], 1e-8, 10.0).sum()),
               "tree_length": ml.tree_length, "pass_ms_sum": round(t[1], 2), "pass_ms_per_pass": round(t[1] / ml.passes, 3)}
        for which, length in (("parsimony_phylogram", pars.branch_length()), ("ml_phylogram", ml.lengths)):
            c = sim.tree_compare(genealogy, (left, right, heights(left, right, length, N)))
            row[which] = {f: (round(getattr(c, f), 6) if isinstance(getattr(c, f), float) else getattr(c, f)) for f in COMPARE}
        rows.append(row)
        print(json.dumps(row), flush=True)
    sim.close()
    if out:
        with open(out, "w") as f:
            json.dump({"script": "scripts/bench_tree_likelihood.py", "device": device, "pop_size": N, "core_size": L, "generations": GENERATIONS,
                       "warmup": WARMUP, "calls": CALLS, "results": rows}, f, indent=1)


if __name__ == "__main__":
    main()
