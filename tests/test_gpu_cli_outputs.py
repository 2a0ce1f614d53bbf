"""Every file the `pansim` executable writes with ALL its read-outs switched on, byte for byte against
tests/golden/cli_outputs.json ({run: {suffix: text}}; "(stdout)" and "(stderr)" are the two streams; a text of 1500 bytes
or more is kept as {"xz": base64 of its xz form}, see pack / unpack): one shard, two shards, and a run saved after 3 of its 6
generations and resumed.  The golden was recorded on an MI355X by
tests/golden/make_cli_outputs.py from the executable and library of the commit before the read-outs moved to
cli_readouts.h -- twice, with equal results, and with equal results for one and two shards ("full" serves both).  Every
read-out is exact integers formatted by the library, so nothing here has a tolerance."""
import base64
import json
import lzma
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "pansim_amd", "pansim")
GOLDEN = os.path.join(HERE, "golden", "cli_outputs.json")

# the smallest shape every read-out accepts.  --cluster_core_max 0.15 joins the closest relatives only: the recorded run has 47
# clusters, of which --print_differentiation takes the 16 largest, of 5 to 2 individuals (the golden's _diff_groups.tsv)
FLAGS = ["--pop_size", "96", "--core_size", "512", "--pan_genes", "120", "--core_genes", "20", "--max_distances", "200", "--seed", "7",
         "--print_dist", "--print_selection", "--print_matrices", "--print_core_freqs", "--print_dist_hist",
         "--print_clusters", "--cluster_core_max", "0.15", "--print_differentiation", "--print_tree", "--print_upgma", "--print_knn", "3",
         "--print_ld", "--print_genealogy", "6", "--print_parsimony", "upgma", "--print_tree_compare", "genealogy,upgma", "--outpref", "out"]
# after --load_state the record of --print_genealogy starts at the loaded generation: the resumed run has its own golden
# for the files that depend on it, every other file is the uninterrupted run's (tests/golden/make_cli_outputs.py checks that)
RECORD_DEPENDENT = {"_genealogy.tsv", "_genealogy.nwk", "_clock.tsv", "_clock_summary.tsv", "_tree_compare.tsv", "_tree_compare_clades.tsv",
                    "_tree_compare_summary.tsv"}


def pack(text):
    return text if len(text) < 1500 else {"xz": base64.b64encode(lzma.compress(text.encode())).decode()}


def unpack(kept):
    return kept if isinstance(kept, str) else lzma.decompress(base64.b64decode(kept["xz"])).decode()


def pansim(exe, cwd, *args):
    """one run in its own process and directory -> {suffix: text} of every file it wrote, and its two streams"""
    os.makedirs(cwd)
    r = subprocess.run([exe, *FLAGS, *args], capture_output=True, text=True, cwd=cwd, timeout=300)
    assert r.returncode == 0, r.stderr
    out = {"(stdout)": r.stdout, "(stderr)": r.stderr}
    for name in sorted(os.listdir(cwd)):
        if name.startswith("out"):
            out[name[3:]] = open(os.path.join(cwd, name)).read()
    return out


def run_form(exe, form, tmp):
    tmp = str(tmp)
    if form == "gpus1":
        return pansim(exe, tmp + "/one", "--n_gen", "6", "--gpus", "1")
    if form == "gpus2":
        return pansim(exe, tmp + "/two", "--n_gen", "6", "--gpus", "2")
    # (the genealogy record is not saved: the first half writes its own files, of which only the state is used)
    pansim(exe, tmp + "/half", "--n_gen", "3", "--save_state", "half.state")
    return pansim(exe, tmp + "/resumed", "--n_gen", "6", "--load_state", "../half/half.state")


@pytest.fixture(scope="module")
def golden():
    g = {run: {suffix: unpack(kept) for suffix, kept in files.items()} for run, files in json.load(open(GOLDEN)).items()}
    return {"gpus1": g["full"], "gpus2": g["full"], "resume": {**g["full"], **g["resume"]}}


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["gpus1", "gpus2", "resume"])
def test_every_output_file_is_the_recorded_one(pa, golden, tmp_path, form):
    got, want = run_form(EXE, form, tmp_path), golden[form]
    assert sorted(got) == sorted(want)
    for suffix in want:
        assert got[suffix] == want[suffix], "out%s of %s differs from the recorded file" % (suffix, form)
