#!/usr/bin/env python3
"""Device time of one pass of the marginal ancestral states (ps_tree_ancestral_states, docs/ANCESTRAL_STATES.md) beside the
likelihood pass with derivatives (ps_tree_model_likelihood) on the same tree and handle, and what the reconstruction says about
the UPGMA and the neighbour-joining tree.  Run it under a time limit:
    timeout -k 10 1100 python scripts/bench_ancestral.py [OUT.json [OUT.md]]

cfg2 (N = 1000, L = 1 200 000, G = 6000) after 100 generations.  Per tree, in its canonical form, with the lengths of
tree_model_ml_lengths under SubstModel.simulator(), three forms of the pass: K = 1 with the new matrix stored, K = 1 without it
(states=False: what the 1.2 GB of stores cost is the difference), and a K = 4 mixture (discrete gamma, alpha = 0.5) with the matrix.
Each: 3 warm-up calls, then 20 calls alternating call for call with ps_tree_model_likelihood with derivatives under the same model;
pass_ms of ancestral_states_timing() against pass_ms of tree_model_timing(), HIP events around each kernel.  Then, per tree:
mean_conf and total_diff beside the total changes of tree_parsimony, and node_accuracy() against the node's height (the longest
path down to a leaf, in events per site), in five bins of equal count.  The medians and their ratios are printed; no ratio is a
condition."""
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
BINS = 5


def spread(ms):
    return {"median": round(float(np.median(ms)), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def heights(left, right, length, n):
    """per merge: the longest path down to a leaf"""
    h = np.zeros(n + left.size)
    for k in range(left.size):
        a, b = int(left[k]), int(right[k])
        h[n + k] = max(h[a] + length[a], h[b] + length[b])
    return h[n:]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    out_md = sys.argv[2] if len(sys.argv) > 2 else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, n_gen=GENERATIONS, max_distances=100))
    sim.run(GENERATIONS)
    sim.sync()
    trees = {"upgma": sim.upgma_tree().merges(), "nj": sim.neighbour_joining().merges()[:2]}
    one = pa.SubstModel.simulator()
    forms = (("K=1", one, True), ("K=1, no matrix", one, False), ("K=4 mixture", pa.SubstModel.gamma(0.5, 4, freq=one.freq, root=one.root), True))
    rows, lines, tables = [], [], []
    for name, (left, right) in trees.items():
        left, right = pa.merges_canonical(left, right, N)
        pars = sim.tree_parsimony(left, right, branches=True)
        ml = sim.tree_model_ml_lengths(left, right, one, pa.f81_lengths_from_changes(pars.branch_changes, L, one.freq))
        lengths = ml.lengths
        medians = {}
        for form, model, states in forms:
            anc_ms, lik_ms = [], []
            for k in range(WARMUP + CALLS):
                got = sim.ancestral_states(left, right, lengths, model, states=states)
                a = sim.ancestral_states_timing()
                got.close()
                sim.tree_model_likelihood(left, right, lengths, model, derivatives=True)
                t = sim.tree_model_timing()
                if k >= WARMUP:
                    anc_ms.append(a[1])
                    lik_ms.append(t[1])
            a, t = spread(anc_ms), spread(lik_ms)
            medians[form] = a["median"]
            row = {"tree": name, "form": form, "lnl": got.lnl, "anc_pass_ms": a, "likelihood_deriv_pass_ms": t, "ratio": round(a["median"] / t["median"], 3)}
            rows.append(row)
            lines.append("| %s | %s | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.2f |" % (name, form, a["median"], a["min"], a["max"], t["median"],
                                                                                          t["min"], t["max"], row["ratio"]))
            print(json.dumps(row), flush=True)
        stores = medians["K=1"] - medians["K=1, no matrix"]
        got = sim.ancestral_states(left, right, lengths, one, states=False)
        acc, h = got.node_accuracy(), heights(left, right, ml.events(), N)
        order = np.argsort(h, kind="stable")
        bins = [{"nodes": int(part.size), "height_events": [round(float(h[part].min()), 4), round(float(h[part].max()), 4)],
                 "mean_accuracy": round(float(acc[part].mean()), 4), "min_accuracy": round(float(acc[part].min()), 4)}
                for part in np.array_split(order, BINS)]
        row = {"tree": name, "form": "reconstruction", "ml_lnl": ml.lnl, "ml_passes": ml.passes, "tree_length_events": ml.tree_length / ml.beta,
               "mean_conf": got.mean_conf, "total_diff": got.total_diff, "parsimony_total_changes": pars.total_changes,
               "root_accuracy": float(acc[-1]), "stores_ms": round(stores, 3), "stores_share_of_pass": round(stores / medians["K=1"], 3),
               "matrix_bytes": (N - 1 + 127) // 128 * 128 * L, "accuracy_by_height": bins}
        rows.append(row)
        tables.append((name, row))
        print(json.dumps(row), flush=True)
    sim.close()
    if out:
        with open(out, "w") as f:
            json.dump({"script": "scripts/bench_ancestral.py", "device": device, "pop_size": N, "core_size": L, "generations": GENERATIONS,
                       "warmup": WARMUP, "calls": CALLS, "results": rows}, f, indent=1)
    if out_md:
        with open(out_md, "w") as f:
            f.write("| tree | form | ancestral pass ms (min .. max) | `ps_tree_model_likelihood` with derivatives, pass ms (min .. max) | ratio |\n"
                    "|---|---|---|---|---|\n")
            f.write("\n".join(lines) + "\n\n")
            f.write("| tree | mean_conf | total_diff | parsimony changes | tree length (events) | stores ms | stores / pass |\n|---|---|---|---|---|---|---|\n")
            for name, r in tables:
                f.write("| %s | %.4f | %.0f | %d | %.1f | %.3f | %.3f |\n" % (name, r["mean_conf"], r["total_diff"], r["parsimony_total_changes"],
                                                                           r["tree_length_events"], r["stores_ms"], r["stores_share_of_pass"]))
            f.write("\n| tree | nodes | height (events per site) | mean node_accuracy | lowest |\n|---|---|---|---|---|\n")
            for name, r in tables:
                for b in r["accuracy_by_height"]:
                    f.write("| %s | %d | %.4f .. %.4f | %.4f | %.4f |\n" % (name, b["nodes"], b["height_events"][0], b["height_events"][1],
                                                                          b["mean_accuracy"], b["min_accuracy"]))


if __name__ == "__main__":
    main()
