#!/usr/bin/env python3
"""Record what the `pansim` executable answers to command lines that end before any device work: exit status, stdout
and stderr of every case of CASES, written to tests/golden/cli_messages.json -- data (expected outputs), which
tests/test_cli_messages.py compares in full with the built executable.  The fixture pins the texts, the statuses and,
through the cases with two faulty flags, the order in which the flags are checked; it is recorded from the executable of
the commit BEFORE a change of the command line's code, built in a scratch checkout:
    python tests/golden/make_cli_messages.py /path/to/that/checkout/pansim_amd/pansim
A case whose stderr mentions a HIP device reached the library's device check: it is refused, because its result would
depend on the machine."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [
    # the command line itself (clap's answers: status 2) and the texts that need no run
    # (--help is compared with the reference's own text by tests/test_cli.py)
    ["--help-extensions"], ["--version"], ["-V"],
    ["stray"], ["-x"], ["--bogus"], ["--bogus=1"], ["--print_dist=1"], ["--seed"], ["--pop_size", "-x"], ["--outpref"],
    # values that do not parse (the reference's unwrap() panics: status 101)
    ["--pop_size", "abc"], ["--pop_size="], ["--max_distances", "1.5"], ["--max_distances="], ["--seed", "-3"], ["--seed", "1.0"],
    ["--threads", "x"], ["--genome_size_penalty", "1,0"], ["--n_gen", "ten"], ["--gpus", "x"],
    # validation: message on stdout, status 0
    ["--pop_size", "0"], ["--pop_size", "100", "--core_size", "12000", "--pan_genes", "600", "--n_gen", "50", "--seed", "0"],
    ["--core_mu", "1.5"], ["--HGT_rate", "-1"], ["--prop_genes2", "1.01"],
    # the shards and the state files
    ["--gpus", "0"], ["--gpus", "2000"], ["--gpus", "2", "--save_state", "s.bin"], ["--gpus", "3", "--load_state", "s.bin"],
    # --print_dist_hist
    ["--dist_hist_bins", "3"], ["--dist_hist_bins", "0,4"], ["--dist_hist_bins", "4,0"], ["--dist_hist_bins", "200,200"],
    ["--dist_hist_bins", "+3,4"], ["--dist_hist_bins", "3,4 "], ["--dist_hist_bins", "20000,1"], ["--dist_hist_bins="],
    ["--dist_hist_core_max", "0"], ["--dist_hist_core_max", "abc"], ["--dist_hist_core_max", "inf"],
    # --print_clusters
    ["--cluster_core_max", "-1"], ["--cluster_core_max", "nan"], ["--cluster_core_max", "x"], ["--cluster_acc_max", "1.5"],
    ["--cluster_acc_max", "-0.5"], ["--print_clusters"],
    # --print_differentiation
    ["--diff_max_groups", "17"], ["--diff_max_groups", "0"], ["--diff_max_groups", "x"], ["--diff_min_size", "0"],
    ["--diff_min_size", "4294967296"], ["--diff_min_size", "-2"], ["--print_differentiation"],
    ["--print_differentiation", "--cluster_core_max", "0.1", "--pop_size", "70000"],
    # --print_tree, --print_upgma
    ["--tree_metric", "x"], ["--upgma_metric", "core "], ["--print_upgma", "--pop_size", "20000"], ["--print_upgma", "--pop_size", "1"],
    ["--print_upgma", "--upgma_metric", "acc", "--core_genes", "0"],
    # --print_knn
    ["--knn_metric", "x"], ["--print_knn", "x"], ["--print_knn", "0"], ["--print_knn", "3 "], ["--print_knn", "200"],
    ["--print_knn", "5", "--pop_size", "4"], ["--print_knn", "5", "--pop_size", "5"],
    # --print_genealogy and its clock histogram
    ["--clock_metric", "x"], ["--clock_bins", "9"], ["--clock_bins", "0,4"], ["--clock_bins", "2000,1"], ["--clock_bins", "1024,16"],
    ["--clock_bins", "4,20000"], ["--print_genealogy", "x"], ["--print_genealogy", "0"], ["--print_genealogy", "5000000000"],
    ["--print_genealogy", "-4"],
    # --print_ld
    ["--ld_metric", "x"], ["--ld_bins", "9"], ["--ld_bins", "0,1"], ["--ld_bins", "64,33"], ["--ld_bins", "20000,1"], ["--ld_bins", "1024,32"],
    ["--ld_max_loci", "70000"], ["--ld_max_loci", "x"], ["--ld_max_loci", "0"], ["--ld_max_loci", "5000000000"], ["--ld_min_minor", "0"],
    ["--ld_min_minor", "x"], ["--ld_min_minor", "+1"],
    # --print_parsimony
    ["--print_parsimony", "x"], ["--print_parsimony", "genealogy"], ["--print_parsimony", "upgma", "--pop_size", "20000"],
    ["--print_parsimony", "tree", "--pop_size", "1"], ["--print_parsimony", "upgma", "--upgma_metric", "acc", "--core_genes", "0"],
    # --print_tree_compare
    ["--print_tree_compare", "upgma"], ["--print_tree_compare", "upgma,x"], ["--print_tree_compare", "tree,tree"],
    ["--print_tree_compare", "genealogy,upgma"], ["--print_tree_compare", "upgma,genealogy"],
    ["--print_tree_compare", "upgma,tree", "--pop_size", "20000"],
    ["--print_tree_compare", "tree,upgma", "--upgma_metric", "acc", "--core_genes", "0"],
    ["--print_tree_compare", "upgma,tree", "--tree_compare_bins", "9"], ["--print_tree_compare", "upgma,tree", "--tree_compare_bins", "0,1"],
    ["--print_tree_compare", "upgma,tree", "--tree_compare_bins", "2000,1"], ["--print_tree_compare", "upgma,tree", "--tree_compare_bins", "200,200"],
    ["--print_tree_compare", "genealogy,tree", "--print_genealogy", "300000"],
    # two faulty flags of different read-outs: the one checked first answers
    ["--clock_bins", "0,4", "--ld_bins", "9"],
    ["--print_knn", "5", "--pop_size", "4", "--knn_metric", "x"],
    ["--print_parsimony", "upgma", "--pop_size", "20000", "--print_upgma"],
    ["--ld_bins", "9", "--dist_hist_bins", "3"],
    ["--print_clusters", "--dist_hist_core_max", "0"],
    ["--print_differentiation", "--print_clusters"],
    ["--diff_max_groups", "17", "--print_clusters"],
    ["--tree_metric", "x", "--diff_min_size", "0"],
    ["--upgma_metric", "x", "--tree_metric", "y"],
    ["--print_knn", "x", "--print_upgma", "--pop_size", "20000"],
    ["--clock_metric", "x", "--print_knn", "0"],
    ["--ld_metric", "x", "--clock_bins", "9"],
    ["--ld_max_loci", "70000", "--ld_min_minor", "0"],
    ["--ld_max_loci", "70000", "--ld_bins", "0,1"],
    ["--print_parsimony", "x", "--ld_min_minor", "0"],
    ["--print_tree_compare", "upgma", "--print_parsimony", "genealogy"],
    ["--print_genealogy", "x", "--print_tree_compare", "tree,tree"],
    ["--print_genealogy", "x", "--print_parsimony", "genealogy"],
    ["--print_genealogy", "0", "--tree_compare_bins", "9"],
    ["--print_tree_compare", "upgma,tree", "--tree_compare_bins", "9", "--pop_size", "20000"],
    ["--gpus", "0", "--dist_hist_bins", "3"],
    ["--dist_hist_bins", "3", "--pop_size", "0"],
    ["--cluster_acc_max", "2", "--cluster_core_max", "-1"],
    ["--print_genealogy", "4", "--print_knn", "0", "--bogus"],
]


def record(exe, args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60, cwd=HERE)
    if "HIP device" in r.stderr:
        sys.exit("refused: %r reached the library's device check (%s)" % (args, r.stderr.strip()))
    return dict(args=args, returncode=r.returncode, stdout=r.stdout, stderr=r.stderr)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    cases = [record(sys.argv[1], args) for args in CASES]
    with open(os.path.join(HERE, "cli_messages.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in cases) + "\n]\n")      # one case per line
    print("wrote %d cases, statuses %s" % (len(cases), sorted({c["returncode"] for c in cases})))
