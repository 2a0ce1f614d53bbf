#!/usr/bin/env python3
"""Hardware counters of the ancestral-states kernel beside the likelihood kernel with derivatives (docs/ANCESTRAL_STATES.md), in a
run of their own -- no tracing beside the counters, one counter set per run:
    timeout -k 10 300 rocprofv3 --pmc MeanOccupancyPerCU --output-format csv -d OUT/occupancy -- python scripts/pmc_ancestral.py
    timeout -k 10 300 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_BUSY_CU_CYCLES --output-format csv -d OUT/valu -- python scripts/pmc_ancestral.py
    python scripts/pmc_ancestral.py --summarise OUT [OUT.json]

The workload: cfg2 (N = 1000, L = 1 200 000) after 100 generations, the canonical UPGMA tree with the F81 correction of its
parsimony changes as lengths; two calls each of ancestral_states() and of tree_model_likelihood(derivatives=True) under
SubstModel.simulator() and under a K = 4 mixture (discrete gamma, alpha = 0.5).  The summary lists every counter of every launch
of tree_anc_kernel and tree_model_kernel in dispatch order.  With single-wave workgroups (N <= 1024)
MeanOccupancyPerCU -- the waves resident on a CU, averaged over the kernel's time -- is the workgroups resident per CU."""
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, L, GENERATIONS = 1000, 1200000, 100


def summarise(top, out):
    """per kernel and counter the values of its launches in dispatch order: the first two under K = 1, the last two under K = 4"""
    rows = {}
    for path in sorted(glob.glob(os.path.join(top, "**", "*counter_collection.csv"), recursive=True)):
        with open(path, newline="") as f:
            found = [r for r in csv.DictReader(f) if re.search(r"tree_(anc|model)_kernel<", r["Kernel_Name"])]
        for r in sorted(found, key=lambda r: int(r["Dispatch_Id"])):
            key = re.search(r"tree_(?:anc|model)_kernel<[^>]*>", r["Kernel_Name"]).group(0)
            k = rows.setdefault(key, {"workgroups": int(r["Grid_Size"]) // int(r["Workgroup_Size"]), "workgroup_size": int(r["Workgroup_Size"])})
            k.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    print(json.dumps(rows, indent=1))
    if out:
        with open(out, "w") as f:
            json.dump({"script": "scripts/pmc_ancestral.py", "pop_size": N, "core_size": L, "generations": GENERATIONS,
                       "launch_order": "K = 1 twice, then the K = 4 mixture twice", "kernels": rows}, f, indent=1)


def workload():
    try:                # before the library: one HIP runtime per process (tests/conftest.py)
        import torch  # noqa: F401
    except ImportError:
        pass
    sys.path.insert(0, ROOT)
    import pansim_amd as pa
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, n_gen=GENERATIONS, max_distances=100))
    sim.run(GENERATIONS)
    sim.sync()
    left, right = pa.merges_canonical(*sim.upgma_tree().merges(), N)
    one = pa.SubstModel.simulator()
    pars = sim.tree_parsimony(left, right, branches=True)
    lengths = pa.f81_lengths_from_changes(pars.branch_changes, L, one.freq)
    for model in (one, pa.SubstModel.gamma(0.5, 4, freq=one.freq, root=one.root)):
        for _ in range(2):
            sim.ancestral_states(left, right, lengths, model).close()
            sim.tree_model_likelihood(left, right, lengths, model, derivatives=True)
    sim.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        workload()
