#!/usr/bin/env python3
"""Device time of one pass of the tree likelihood under F81 with rate categories (ps_tree_model_likelihood, docs/TREE_MODEL.md)
beside the Jukes-Cantor pass (ps_tree_likelihood) on the same tree, and what the simulator's own model does to the
maximum-likelihood branch lengths of the UPGMA and the neighbour-joining tree.  Run it under a time limit:
    timeout -k 10 1100 python scripts/bench_tree_model.py [OUT.json [OUT.md]]

cfg2 (N = 1000, L = 1 200 000, G = 6000) after 100 generations with the ancestry recorded.  Per tree, in its canonical form, with
the F81 correction of its parsimony changes as lengths, four forms of the model pass: K = 1 (SubstModel.simulator()), a K = 4
mixture (discrete gamma, alpha = 0.5), K = 2 assigned classes up only, and the same up + down.  Each: 3 warm-up calls, then 20
calls alternating call for call with ps_tree_likelihood on the same tree (with derivatives where the model pass has them);
pass_ms of tree_model_timing() against pass_ms of tree_likelihood_timing(), HIP events around each kernel.  Then one
tree_ml_lengths() (JC69) and one tree_model_ml_lengths(SubstModel.simulator()): lnL, tree length in substitutions and in events,
and tree_compare() of the cophenetic heights of each phylogram against the recorded genealogy.  The medians and their ratios are
printed; no ratio is a condition."""
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
    """uint32 per merge, as tree_compare takes values: the largest sum of branch lengths down to a leaf, scaled to 1 .. 2^18 - 1
    of the root's"""
    h = np.zeros(n + left.size)
    for k in range(left.size):
        a, b = int(left[k]), int(right[k])
        h[n + k] = max(h[a] + length[a], h[b] + length[b])
    return (1 + np.round(h[n:] / max(h[-1], 1e-300) * 262142.0)).astype(np.uint32)


def spread(ms):
    return {"median": round(float(np.median(ms)), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    out_md = sys.argv[2] if len(sys.argv) > 2 else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, n_gen=GENERATIONS, max_distances=100))
    sim.record_ancestry(GENERATIONS)
    sim.run(GENERATIONS)
    sim.sync()
    genealogy = sim.genealogy()
    trees = {"upgma": sim.upgma_tree().merges(), "nj": sim.neighbour_joining().merges()[:2]}
    one = pa.SubstModel.simulator()
    classes = np.random.default_rng(0).integers(0, 2, L).astype(np.uint8)
    forms = (("K=1", one, {}), ("K=4 mixture", pa.SubstModel.gamma(0.5, 4, freq=one.freq, root=one.root), {}),
             ("K=2 assigned up", pa.SubstModel.simulator(rates=(0.5, 2.0), site_class=classes), {}),
             ("K=2 assigned up+down", pa.SubstModel.simulator(rates=(0.5, 2.0), site_class=classes), dict(derivatives=True)))
    rows, lines = [], []
    for name, (left, right) in trees.items():
        left, right = pa.merges_canonical(left, right, N)
        pars = sim.tree_parsimony(left, right, branches=True)
        start = pa.f81_lengths_from_changes(pars.branch_changes, L, one.freq)
        for form, model, kw in forms:
            model_ms, jc_ms = [], []
            for k in range(WARMUP + CALLS):
                got = sim.tree_model_likelihood(left, right, start, model, **kw)
                t = sim.tree_model_timing()
                sim.tree_likelihood(left, right, start, **kw)
                j = sim.tree_likelihood_timing()
                if k >= WARMUP:
                    model_ms.append(t[1])
                    jc_ms.append(j[1])
            m, j = spread(model_ms), spread(jc_ms)
            row = {"tree": name, "form": form, "lnl": got.lnl, "model_pass_ms": m, "jc_pass_ms": j, "ratio": round(m["median"] / j["median"], 3)}
            rows.append(row)
            lines.append("| %s | %s | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.2f |" % (name, form, m["median"], m["min"], m["max"], j["median"],
                                                                                          j["min"], j["max"], row["ratio"]))
            print(json.dumps(row), flush=True)
        jc = sim.tree_ml_lengths(left, right, pa.jc_lengths_from_changes(pars.branch_changes, L))
        ml = sim.tree_model_ml_lengths(left, right, one, start)
        t = sim.tree_model_timing()
        row = {"tree": name, "form": "ml_lengths", "pass_ms_per_pass": round(t[1] / ml.passes, 3)}
        for which, r, beta in (("jc69", jc, 0.75), ("simulator", ml, ml.beta)):
            c = sim.tree_compare(genealogy, (left, right, heights(left, right, r.lengths, N)))
            row[which] = {"rounds": r.rounds, "passes": r.passes, "rollbacks": r.rollbacks, "converged": r.converged, "start_lnl": r.start_lnl,
                          "lnl": r.lnl, "tree_length_substitutions": r.tree_length, "tree_length_events": r.tree_length / beta,
                          "root_branches": [float(r.lengths[int(left[-1])]), float(r.lengths[int(right[-1])])],
                          **{f: (round(getattr(c, f), 6) if isinstance(getattr(c, f), float) else getattr(c, f)) for f in COMPARE}}
        rows.append(row)
        print(json.dumps(row), flush=True)
    sim.close()
    if out:
        with open(out, "w") as f:
            json.dump({"script": "scripts/bench_tree_model.py", "device": device, "pop_size": N, "core_size": L, "generations": GENERATIONS,
                       "warmup": WARMUP, "calls": CALLS, "results": rows}, f, indent=1)
    if out_md:
        with open(out_md, "w") as f:
            f.write("| tree | form | model pass ms (min .. max) | `ps_tree_likelihood` pass ms (min .. max) | ratio |\n|---|---|---|---|---|\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
