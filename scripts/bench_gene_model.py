#!/usr/bin/env python3
"""Device time of the gene gain / loss pass (ps_tree_gene_ancestral, docs/GENE_MODEL.md) beside its yardstick, and what the fit
says about a run's own gain / loss rates.  Run it under a time limit:
    timeout -k 10 1100 python scripts/bench_gene_model.py [OUT.json [OUT.md]]

cfg2 (N = 1000, L = 1 200 000, G = 6000) after 100 generations, the canonical UPGMA tree with the lengths of tree_model_ml_lengths
under SubstModel.simulator(), in events per site.
  timing   per row 3 warm-up and 20 timed calls of pass_ms (HIP events around the kernels), each alternating call for call with the
           yardstick: ps_tree_ancestral_states (K = 1, no matrix) on a core handle of the same tree whose L = G columns are the
           expanded gene bytes, re-measured in the same run.  Rows: the up + down pass without and with the new matrix, under both
           teams of the tuning key "gene_team" (one wave, 256 threads), the up pass alone, a two-class mixture.  Repeated on a
           pangenome ten times as large (--pan_genes 60000; the core cut to 200 000 sites there: only the tree comes from it).
  fit      assigned compartments and the mixture, from GeneModel.simulator(run) with every rate doubled and pi_1 = 0.4 as the start:
           the fitted rates times the core's events per site and generation beside lambda_c / |c|, pi_1, lnL, the share of genes whose
           largest posterior class is their compartment, sum branch_gains / branch_losses beside tree_parsimony's gene totals; once
           at the default --HGT_rate and once at 0.  The wall time of one round of tree_gene_fit on the device beside
           gene_fit_from_rows on the host, on the same data.
Everything is printed and written as measured; the acceptance line compares the two medians with the two rows' own spread."""
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


def spread(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def fmt(s):
    return "%.3f (%.3f .. %.3f)" % (s["median"], s["min"], s["max"])


def tree_of(sim, core_size):
    """the canonical UPGMA tree with its ML lengths in events per site, and the core's events per site and generation"""
    one = pa.SubstModel.simulator()
    left, right = pa.merges_canonical(*sim.upgma_tree().merges(), N)
    pars = sim.tree_parsimony(left, right, branches=True)
    ml = sim.tree_model_ml_lengths(left, right, one, pa.f81_lengths_from_changes(pars.branch_changes, core_size, one.freq))
    return left, right, ml.events(), float(sim.derived.n_core_mutations) / core_size


def timing(sim, left, right, lengths, tag, rows, lines):
    acc = sim.pan_genome
    genes = acc.read_matrix()
    G = genes.shape[1]
    yard = pa.Population(N, G, 4, True, 0.0, 0, 0)
    yard.load_matrix((genes + 1).astype(np.uint8))                 # the expanded gene bytes 1 / 2 as core cells
    jc = pa.SubstModel.jc69()
    t_yard = np.minimum(lengths, 10.0)
    sim_model = pa.GeneModel.simulator(sim)
    one = pa.GeneModel((0.5, 0.5), root=sim_model.root, rates=(float(np.dot(sim_model.rates, sim_model.mixture().weights)),))
    forms = (("up + down, no matrix", one, 0, "anc0"), ("up + down, no matrix, team 64", one, 64, "anc0"),
             ("up + down, no matrix, team 256", one, 256, "anc0"), ("up + down, new matrix", one, 0, "anc1"),
             ("up pass alone", one, 0, "lik"), ("up + down, 2-class mixture, no matrix", sim_model.mixture(), 0, "anc0"),
             ("up + down, assigned compartments, no matrix", sim_model, 0, "anc0"))
    for form, model, team, kind in forms:
        acc.set_tuning("gene_team", team)
        g_ms, y_ms = [], []
        for k in range(WARMUP + CALLS):
            if kind == "lik":
                acc.tree_gene_likelihood(left, right, lengths, model)
            else:
                acc.tree_gene_ancestral(left, right, lengths, model, states=kind == "anc1").close()
            g = acc.tree_gene_timing()
            yard.ancestral_states(left, right, t_yard, jc, states=False)
            y = yard.ancestral_states_timing()
            if k >= WARMUP:
                g_ms.append(g[1])
                y_ms.append(y[1])
        a, b = spread(g_ms), spread(y_ms)
        slack = (a["max"] - a["min"]) + (b["max"] - b["min"])
        row = {"run": tag, "genes": G, "form": form, "gene_pass_ms": a, "yardstick_pass_ms": b, "ratio": round(a["median"] / b["median"], 3),
               "within_spread": bool(a["median"] <= b["median"] + slack)}
        rows.append(row)
        lines.append("| %s | %d | %s | %s | %s | %.2f | %s |" % (tag, G, form, fmt(a), fmt(b), row["ratio"], "yes" if row["within_spread"] else "no"))
        print(json.dumps(row), flush=True)
    acc.set_tuning("gene_team", 0)
    yard.close()


def fits(sim, left, right, lengths, events_per_gen, tag, rows, host_wall):
    acc = sim.pan_genome
    truth = pa.GeneModel.simulator(sim)
    comp = truth.gene_class
    pars = sim.tree_parsimony(left, right, genes=True, branches=True)
    for name, base in (("assigned", truth), ("mixture", truth.mixture())):
        start = pa.GeneModel((0.6, 0.4), base.root, base.rates * 2.0, base.weights, base.gene_class)
        t0 = time.perf_counter()
        fit = acc.tree_gene_fit(left, right, lengths, start, max_rounds=30, eps_lnl=1e-3)
        wall = time.perf_counter() - t0
        lik = acc.tree_gene_likelihood(left, right, lengths, fit.model, per_gene=True)
        anc = acc.tree_gene_ancestral(left, right, lengths, fit.model, states=False)
        row = {"run": tag, "fit": name, "rounds": fit.rounds, "passes": fit.passes, "converged": fit.converged, "device_wall_s": round(wall, 3),
               "start_lnl": fit.start_lnl, "lnl": fit.lnl, "pi1": float(fit.model.freq[1]), "rates_per_event": [float(v) for v in fit.model.rates],
               "rates_per_generation": [float(v * events_per_gen) for v in fit.model.rates], "lambda_over_size": [float(v) for v in truth.rates],
               "weights": [float(v) for v in fit.model.weights], "compartment_shares": [float(v) for v in truth.mixture().weights],
               "largest_posterior_is_compartment": float(np.mean(lik.gene_best_class() == comp)),
               "sum_branch_gains": anc.total_gains, "sum_branch_losses": anc.total_losses, "parsimony_gene_gains": int(pars.gene_total_gains),
               "parsimony_gene_losses": int(pars.gene_total_losses), "mean_conf": anc.mean_conf}
        if host_wall and name == "assigned":
            genes = acc.read_matrix()
            t0 = time.perf_counter()
            dev = acc.tree_gene_fit(left, right, lengths, start, max_rounds=1, eps_lnl=1e-3)
            row["device_one_round_wall_s"] = round(time.perf_counter() - t0, 3)
            t0 = time.perf_counter()
            host = pa.gene_fit_from_rows(genes, left, right, lengths, start, max_rounds=1, eps_lnl=1e-3)
            row["host_one_round_wall_s"] = round(time.perf_counter() - t0, 3)
            row["one_round_passes"] = host.passes
            row["one_round_same_bits"] = bool(np.array_equal(dev.round_lnl, host.round_lnl) and np.array_equal(dev.model.rates, host.model.rates))
        rows.append(row)
        print(json.dumps(row), flush=True)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    out_md = sys.argv[2] if len(sys.argv) > 2 else None
    device = torch.cuda.get_device_name(0) if torch is not None and torch.cuda.is_available() else "unknown"
    rows, lines, fit_rows = [], [], []
    for tag, kw, do_timing, do_fit in (("cfg2", {}, True, True), ("cfg2, HGT_rate 0", dict(HGT_rate=0.0), False, True),
                                       ("G = 60 000", dict(pan_genes=60000, core_size=200000), True, False)):
        core_size = kw.get("core_size", L)
        sim = pa.Simulation(pa.make_params(**{**dict(pop_size=N, core_size=L, n_gen=GENERATIONS, max_distances=100), **kw}))
        sim.run(GENERATIONS)
        sim.sync()
        left, right, lengths, per_gen = tree_of(sim, core_size)
        if do_timing:
            timing(sim, left, right, lengths, tag, rows, lines)
        if do_fit:
            fits(sim, left, right, lengths, per_gen, tag, fit_rows, host_wall=tag == "cfg2")
        sim.close()
    if out:
        with open(out, "w") as f:
            json.dump({"script": "scripts/bench_gene_model.py", "device": device, "pop_size": N, "core_size": L, "generations": GENERATIONS,
                       "warmup": WARMUP, "calls": CALLS, "timing": rows, "fits": fit_rows}, f, indent=1)
    if out_md:
        with open(out_md, "w") as f:
            f.write("| run | G | form | gene pass ms (min .. max) | yardstick `ps_tree_ancestral_states` pass ms (min .. max) | ratio | median within the two spreads |\n"
                    "|---|---|---|---|---|---|---|\n" + "\n".join(lines) + "\n\n")
            f.write("| run | fit | rounds | passes | device wall s | lnL start | lnL | pi_1 | rates per generation | lambda_c / size | weights | compartment shares "
                    "| largest posterior = compartment | sum gains / losses | parsimony gains / losses |\n" + "|---" * 15 + "|\n")
            for r in fit_rows:
                f.write("| %s | %s | %d | %d | %.2f | %.1f | %.1f | %.4f | %s | %s | %s | %s | %.4f | %.0f / %.0f | %d / %d |\n" % (
                    r["run"], r["fit"], r["rounds"], r["passes"], r["device_wall_s"], r["start_lnl"], r["lnl"], r["pi1"],
                    ", ".join("%.3g" % v for v in r["rates_per_generation"]), ", ".join("%.3g" % v for v in r["lambda_over_size"]),
                    ", ".join("%.3f" % v for v in r["weights"]), ", ".join("%.3f" % v for v in r["compartment_shares"]),
                    r["largest_posterior_is_compartment"], r["sum_branch_gains"], r["sum_branch_losses"], r["parsimony_gene_gains"],
                    r["parsimony_gene_losses"]))
            for r in fit_rows:
                if "host_one_round_wall_s" in r:
                    f.write("\nOne round of the assigned fit on the same data (%d passes): %.2f s on the device, %.2f s on the host; the same bits: %s.\n" % (
                        r["one_round_passes"], r["device_one_round_wall_s"], r["host_one_round_wall_s"], r["one_round_same_bits"]))


if __name__ == "__main__":
    main()
