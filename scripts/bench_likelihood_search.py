#!/usr/bin/env python3
"""Device time of one pass of the likelihood tree search (ps_tree_model_nni_deltas, docs/LIKELIHOOD_SEARCH.md) beside the
likelihood pass with derivatives (ps_tree_model_likelihood) on the same tree and handle, and what the search does to the UPGMA
and the neighbour-joining tree against the recorded genealogy.  Run it under a time limit:
    timeout -k 10 1100 python scripts/bench_likelihood_search.py [OUT.json [OUT.md [MAX_ROUNDS]]]

cfg2 (N = 1000, L = 1 200 000, G = 6000) after 100 generations with the ancestry recorded, SubstModel.simulator().  Per tree, in
its canonical form, with the F81 correction of its parsimony changes as lengths: 3 warm-up calls, then 20 calls of
model_nni_deltas() alternating call for call with tree_model_likelihood(derivatives=True); pass_ms of tree_model_nni_timing()
against pass_ms of tree_model_timing(), HIP events around each kernel.  Then one tree_model_nni() (MAX_ROUNDS rounds at the most,
default 30; 2 length rounds per pass): rounds, passes, moves, lnL start -> end, and tree_compare() of the tree before and after
against the genealogy (the phylogram's cophenetic heights from tree_model_ml_lengths before, from the search's lengths after).
The medians and their ratio are printed; no ratio is a condition."""
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

WARMUP, CALLS = 3, 20
N, L, GENERATIONS = 1000, 1200000, 100
COMPARE = ("shared_clades", "rf_distance", "triplet_recall", "cophenetic_r")


def heights(left, right, length, n):
    """uint32 per merge, as tree_compare takes values: the largest sum of branch lengths down to a leaf, scaled to 1 .. 2^18 - 1
    of the root's"""
    h = np.zeros(n + left.size)
    for k in range(left.size):
        a, b = int(left[k]), int(right[k])
        h[n + k] = max(h[a] + length[a], h[b] + length[b])
    return (1 + np.round(h[n:] / max(h[-1], 1e-300) * 262142.0)).astype(np.uint32)


def spread(ms):
    return {"median": round(float(np.median(ms)), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def compared(sim, genealogy, left, right, lengths):
    c = sim.tree_compare(genealogy, (left, right, heights(left, right, lengths, N)))
    return {f: (round(getattr(c, f), 6) if isinstance(getattr(c, f), float) else getattr(c, f)) for f in COMPARE}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    out_md = sys.argv[2] if len(sys.argv) > 2 else None
    max_rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 30
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, n_gen=GENERATIONS, max_distances=100))
    sim.record_ancestry(GENERATIONS)
    sim.run(GENERATIONS)
    sim.sync()
    genealogy = sim.genealogy()
    trees = {"upgma": sim.upgma_tree().merges(), "nj": sim.neighbour_joining().merges()[:2]}
    model = pa.SubstModel.simulator()
    rows, lines, found = [], [], []
    for name, (left, right) in trees.items():
        left, right = pa.merges_canonical(left, right, N)
        pars = sim.tree_parsimony(left, right, branches=True)
        start = pa.f81_lengths_from_changes(pars.branch_changes, L, model.freq)
        nni_ms, lik_ms = [], []
        for k in range(WARMUP + CALLS):
            d = sim.model_nni_deltas(left, right, start, model)
            t = sim.tree_model_nni_timing()
            sim.tree_model_likelihood(left, right, start, model, derivatives=True)
            j = sim.tree_model_timing()
            if k >= WARMUP:
                nni_ms.append(t[1])
                lik_ms.append(j[1])
        m, j = spread(nni_ms), spread(lik_ms)
        some = ~np.isnan(d.delta)
        row = {"tree": name, "lnl": d.lnl, "candidates": int(some.sum()), "improving": int((d.delta[some] > 1e-3).sum()),
               "best_gain": float(d.delta[some].max()), "nni_pass_ms": m, "likelihood_pass_ms": j, "ratio": round(m["median"] / j["median"], 3),
               "reduce_ms": round(t[2], 3)}
        rows.append(row)
        lines.append("| %s | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.2f |" % (name, m["median"], m["min"], m["max"], j["median"], j["min"],
                                                                                 j["max"], row["ratio"]))
        print(json.dumps(row), flush=True)
        before = sim.tree_model_ml_lengths(left, right, model, start, max_rounds=5)
        t0 = time.time()
        s = sim.tree_model_nni(left, right, model, start, max_rounds=max_rounds, length_rounds=2)
        wall = time.time() - t0
        row = {"tree": name, "form": "search", "max_rounds": max_rounds, "rounds": s.rounds, "passes": s.passes, "length_passes": s.length_passes,
               "rollbacks": s.rollbacks, "moves": s.n_moves, "local_optimum": s.local_optimum, "candidates_last": s.candidates_last,
               "start_lnl": s.start_lnl, "lnl_before_with_ml_lengths": before.lnl, "lnl": s.lnl, "wall_s": round(wall, 1),
               "before": compared(sim, genealogy, left, right, before.lengths), "after": compared(sim, genealogy, s.left, s.right, s.lengths)}
        rows.append(row)
        found.append("| %s | %d | %d + %d | %d | %d | %.1f -> %.1f | %s | %s |" % (
            name, s.rounds, s.passes, s.length_passes, s.n_moves, s.rollbacks, s.start_lnl, s.lnl,
            " / ".join("%s -> %s" % (row["before"][f], row["after"][f]) for f in COMPARE), "yes" if s.local_optimum else "no (%d left)" % s.candidates_last))
        print(json.dumps(row), flush=True)
    sim.close()
    if out:
        with open(out, "w") as f:
            json.dump({"script": "scripts/bench_likelihood_search.py", "device": device, "pop_size": N, "core_size": L, "generations": GENERATIONS,
                       "warmup": WARMUP, "calls": CALLS, "results": rows}, f, indent=1)
    if out_md:
        with open(out_md, "w") as f:
            f.write("| tree | search pass ms (min .. max) | `ps_tree_model_likelihood` up + down pass ms (min .. max) | ratio |\n|---|---|---|---|\n")
            f.write("\n".join(lines) + "\n\n")
            f.write("| tree | rounds | passes (search + likelihood) | moves | rollbacks | lnL start -> end | %s (before -> after) | local optimum |\n"
                    "|---|---|---|---|---|---|---|---|\n" % " / ".join(COMPARE))
            f.write("\n".join(found) + "\n")


if __name__ == "__main__":
    main()
