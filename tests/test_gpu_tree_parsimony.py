"""Tree parsimony on the device (ps_tree_parsimony and its ps_sim / ps_multi forms, docs/TREE_PARSIMONY.md) against the numpy
restatement over the matrix bytes and the merge list (tests/tree_parsimony_ref.py), which shares nothing with the library.
Every comparison is an equality.  The shapes are the smallest at which each thing can still go wrong: one merge, the lane
boundary, the single-wave team against the shared tile (1024 / 1025), LDS counters against global ones (4096 / 16384); the
caterpillar has one merge per level and catches a missing level fence, the balanced tree many lane trips per level."""
import ctypes as C
import filecmp
import os
import subprocess

import numpy as np
import pytest

import tree_parsimony_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_STATE = -1, -6
SHAPES = [(2, 5), (7, 203), (64, 16), (65, 17), (1000, 4099), (1024, 64), (1025, 301), (4096, 130), (16384, 33)]
TREES = ("random", "caterpillar", "balanced", "forest", "permuted")


def core_handle(pa, m, **kw):
    p = pa.Population(m.shape[0], m.shape[1], 4, True, 0.0, 0, 0, **kw)
    p.load_matrix(m)
    return p


def acc_handle(pa, a, cg=3):
    p = pa.Population(a.shape[0], a.shape[1], 2, False, 0.5, 0, cg)
    p.load_matrix(a)
    return p


def check_core(core, m, left, right):
    """every output of the call against the restatement, with and without the optional outputs"""
    want = ref.parsimony(m, left, right)
    full = core.tree_parsimony(left, right, per_site=True, branches=True)
    ref.assert_equal(full, want)
    bare = core.tree_parsimony(left, right)
    ref.assert_equal(bare, want, skip=("site_changes", "branch_changes"))
    assert bare.site_changes is None and bare.branch_changes is None
    up = core.tree_parsimony(left, right, per_site=True)          # the up pass alone, storing
    ref.assert_equal(up, want, skip=("branch_changes",))
    return full


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("N,L", SHAPES)
def test_loaded_matrices(pa, N, L, tree):
    rng = np.random.default_rng(N * 131 + L + len(tree))
    all_trees = ref.trees(rng, N)
    if tree not in all_trees:
        assert N < 4 and tree == "forest"                           # (two leaves have no forest)
        return
    left, right = all_trees[tree]
    # arbitrary bytes, a column of zeros and one of 0x03 on three of the trees, clean one-hot data (the fast load) on two
    m = ref.evolved(rng, N, L, left, right, junk=tree in ("random", "forest", "permuted"))
    if L >= 8:
        m[:, 4:8] = 2                                               # a fully monomorphic tile: the skip path
    core = core_handle(pa, m)
    got = check_core(core, m, left, right)
    core.close()
    assert got.spanning == (tree != "forest")
    if L >= 8:
        assert not got.site_changes[4:8].any()
    if tree == "forest":
        assert got.covered_leaves < N and got.trees > 1
    elif N >= 64:
        assert got.homoplasic_sites > 0 and got.site_changes.min() == 0 and got.max_changes >= 3
    if tree == "random" and N == 1000:
        assert 10 <= pa.parsimony_schedule(left, right, N)[1] <= 40  # depth about 20


@pytest.mark.parametrize("N,G", [(7, 40), (300, 65), (1025, 131), (5000, 70)])
def test_genes(pa, N, G):
    rng = np.random.default_rng(G)
    L = 37
    for name, (left, right) in ref.trees(rng, N).items():
        if N > 300 and name in ("caterpillar", "permuted"):
            continue
        m = ref.evolved(rng, N, L, left, right)
        a = ref.evolved_genes(rng, N, G, left, right)
        want = ref.parsimony(m, left, right, a)
        core, acc = core_handle(pa, m), acc_handle(pa, a)
        full = core.tree_parsimony(left, right, acc=acc, per_site=True, branches=True, genes=True)
        ref.assert_equal(full, want)
        assert full.gene_total_gains > 0 and full.gene_total_losses > 0 and full.genes == G
        # other sets of optional outputs on the same handles agree on what they share
        part = core.tree_parsimony(left, right, acc=acc, genes=True)
        ref.assert_equal(part, want, skip=("site_changes", "branch_changes", "branch_gains", "branch_losses"))
        assert part.branch_gains is None
        none = core.tree_parsimony(left, right, acc=acc, branches=True)
        ref.assert_equal(none, dict(want, genes=0, gene_total_changes=0, gene_total_gains=0, gene_total_losses=0),
                         skip=("site_changes", "gene_changes", "gene_gains", "gene_losses", "branch_gains", "branch_losses"))
        lib, out, buf = pa.load(), pa._lib.Parsimony(), np.zeros(G, np.uint32)
        args = (left.ctypes.data, right.ctypes.data, left.size, C.byref(out), None, None, None, buf.ctypes.data, None, None, None, None)
        assert lib.ps_tree_parsimony(core._h, acc._h, *args) == 0                     # gene_changes alone: the up pass of the genes
        assert np.array_equal(buf, want["gene_changes"]) and out.gene_total_gains == 0 and out.gene_total_changes == want["gene_total_changes"]
        assert lib.ps_tree_parsimony(core._h, None, *args) == PS_ERR_INVALID and "accessory handle" in lib.ps_last_error().decode()
        core.close()
        acc.close()


SIM = dict(pop_size=100, core_size=2001, pan_genes=300, core_genes=20, HR_rate=0.5, HGT_rate=0.5, seed=11, n_gen=8, max_distances=100)


def test_the_three_trees_of_a_simulation(pa):
    """upgma, linkage tree and recorded genealogy of a short run, end to end: leaves are rows of the reference's row order
    while the matrices are stored in another"""
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.record_ancestry(16)
    sim.run(6)
    sources = dict(upgma=sim.upgma_tree().merges(), tree=sim.linkage_tree().merges(), genealogy=sim.genealogy().merges()[:2])
    parents = sim.last_parents()
    assert (np.diff(parents.astype(np.int64)) < 0).any()                             # the internal order is not the output order
    m, a = sim.core_genome.read_matrix(), sim.pan_genome.read_matrix()
    for name, (left, right) in sources.items():
        assert 1 <= left.size <= 99, name
        want = ref.parsimony(m, left, right, a)
        got = sim.tree_parsimony(left, right, per_site=True, branches=True, genes=True)
        ref.assert_equal(got, want)
        assert got.genes == 280 and got.total_changes > 0, name
        # the leaves taken in internal order would be another answer
        other = ref.parsimony(m[np.argsort(parents, kind="stable")], left, right)
        assert other["total_changes"] != want["total_changes"] or not np.array_equal(other["branch_changes"], want["branch_changes"]), name
        host = pa.parsimony_from_rows(m, left, right)
        assert np.array_equal(host.branch_changes, got.branch_changes) and got.newick().count(";") == got.trees
    assert sources["upgma"][0].size == 99 and len(sim.tree_parsimony_timing()) == 3
    # the calls changed no state
    sim.run(2)
    plain = pa.Simulation(pa.make_params(**SIM))
    plain.run(8)
    assert np.array_equal(plain.core_genome.read_matrix(), sim.core_genome.read_matrix())
    assert np.array_equal(plain.pan_genome.read_matrix(), sim.pan_genome.read_matrix())
    plain.close()
    sim.close()


def test_multi_simulation_equals_the_unsharded_run(pa):
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(5)
    left, right = sim.upgma_tree().merges()
    want = ref.parsimony(sim.core_genome.read_matrix(), left, right, sim.pan_genome.read_matrix())
    sim.close()
    multi = pa.MultiSimulation(pa.make_params(**SIM), 2, devices=[0, 0])
    multi.run(5)
    ref.assert_equal(multi.tree_parsimony(left, right, per_site=True, branches=True, genes=True), want)
    ref.assert_equal(multi.tree_parsimony(left, right), dict(want, genes=0, gene_total_changes=0, gene_total_gains=0, gene_total_losses=0),
                     skip=ref.ARRAYS[:1] + ref.ARRAYS[2:])
    # a site shard answers for its own sites, and not with an accessory matrix
    lo = multi.shards[0].core_genome.ncols
    part = multi.shards[1].core_genome.tree_parsimony(left, right, per_site=True)
    assert 0 < part.sites < 2001 and lo + part.sites == 2001 and lo != part.sites
    assert np.array_equal(part.site_changes, want["site_changes"][lo:])
    with pytest.raises(pa.PansimError) as e:
        multi.shards[1].tree_parsimony(left, right)
    assert e.value.code == PS_ERR_INVALID and "ps_multi_tree_parsimony" in str(e.value)
    multi.close()


def test_three_site_shards_add_to_the_whole(pa):
    rng = np.random.default_rng(4)
    N, L = 130, 1000
    left, right = ref.random_joining(rng, N)
    m = ref.evolved(rng, N, L, left, right)
    want = ref.parsimony(m, left, right)
    cuts = [0, 333, 700, L]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        shard = core_handle(pa, np.ascontiguousarray(m[:, lo:hi]), col_offset=lo, global_cols=L)
        parts.append(shard.tree_parsimony(left, right, per_site=True, branches=True))
        shard.close()
    assert [p.sites for p in parts] == [333, 367, 300]
    for name in ("site_hist", "branch_changes"):
        assert np.array_equal(sum(getattr(p, name) for p in parts), want[name]), name
    assert np.array_equal(np.concatenate([p.site_changes for p in parts]), want["site_changes"])
    for name in ("total_changes", "changed_sites", "min_changes", "homoplasic_sites"):
        assert sum(getattr(p, name) for p in parts) == want[name], name
    assert max(p.max_changes for p in parts) == want["max_changes"]


def test_the_scratch_grows_and_timing(pa):
    rng = np.random.default_rng(8)
    N, L = 500, 700
    big, small = ref.random_joining(rng, N), ref.random_joining(rng, N, 20)
    m = ref.evolved(rng, N, L, *big)
    core = core_handle(pa, m)
    with pytest.raises(pa.PansimError) as e:
        core.tree_parsimony_timing()                          # nothing to report yet
    assert e.value.code == PS_ERR_STATE
    for (left, right), kw in ((small, dict()), (big, dict(per_site=True, branches=True)), (small, dict(branches=True))):
        got = core.tree_parsimony(left, right, **kw)
        skip = tuple(n for n, on in (("site_changes", "per_site" in kw), ("branch_changes", "branches" in kw)) if not on)
        ref.assert_equal(got, ref.parsimony(m, left, right), skip=skip)
        ms = core.tree_parsimony_timing()
        assert len(ms) == 3 and all(x >= 0.0 for x in ms) and ms[1] > 0.0 and ms[2] == 0.0
    core.close()


def test_handle_checks(pa):
    rng = np.random.default_rng(6)
    core, acc = core_handle(pa, ref.onehot(rng, (20, 64))), acc_handle(pa, (rng.random((20, 10)) < 0.5).astype(np.uint8))
    left, right = ref.caterpillar(20)
    with pytest.raises(pa.PansimError) as e:
        acc.tree_parsimony(left, right)
    assert e.value.code == PS_ERR_INVALID and "core handle first" in str(e.value)
    with pytest.raises(pa.PansimError) as e:
        core.tree_parsimony(left, right, acc=core)
    assert e.value.code == PS_ERR_INVALID and "accessory handle" in str(e.value)
    other = pa.Population(21, 10, 2, False, 0.5, 0, 2)
    with pytest.raises(pa.PansimError) as e:
        core.tree_parsimony(left, right, acc=other)
    assert e.value.code == PS_ERR_INVALID and "20 individuals" in str(e.value)
    with pytest.raises(ValueError):
        core.tree_parsimony(left, right, genes=True)
    for bad_left, bad_right in (([0, 0], [1, 2]), ([0, 21], [1, 2]), ([3], [3]), ([], []), (list(range(20)), list(range(1, 21)))):
        with pytest.raises(pa.PansimError) as e:
            core.tree_parsimony(bad_left, bad_right)
        assert e.value.code == PS_ERR_INVALID
    shard = pa.Population(20, 32, 4, True, 0.0, 0, 0, col_offset=32, global_cols=64)
    with pytest.raises(pa.PansimError) as e:
        shard.tree_parsimony(left, right, acc=acc)
    assert e.value.code == PS_ERR_INVALID and "ps_multi_tree_parsimony" in str(e.value)
    big = pa.Population(16385, 16, 4, True, 0.0, 0, 0)
    with pytest.raises(pa.PansimError) as e:
        big.tree_parsimony(*ref.caterpillar(16385))
    assert e.value.code == PS_ERR_INVALID and "16384" in str(e.value)
    for p in (core, acc, other, shard, big):
        p.close()


CLI = dict(pop_size=100, core_size=301, pan_genes=600, core_genes=200, n_gen=5, seed=9, max_distances=500, HR_rate=0.5, HGT_rate=0.5)
USUAL = (".tsv", "_freqs.txt", "_core_genome.csv", "_pangenome.csv", "_per_gen.tsv", "_selection.tsv")
PARS = ("_parsimony_sites.tsv", "_parsimony_genes.tsv", "_parsimony_branches.tsv", "_parsimony.nwk", "_parsimony_summary.tsv")
SOURCE = dict(upgma=(("--print_upgma",), ("_upgma.tsv", "_upgma.nwk", "_upgma_summary.tsv")),
              tree=(("--print_tree",), ("_tree.tsv", "_tree_summary.tsv")),
              genealogy=(("--print_genealogy", 3), ("_genealogy.tsv", "_genealogy.nwk", "_clock.tsv", "_clock_summary.tsv")))


def _cli(*args):
    r = subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("source,gpus", [("upgma", 1), ("tree", 2), ("genealogy", 1), ("genealogy", 2)])
def test_cli_print_parsimony(pa, tmp_path, source, gpus):
    """the five files against the Python API over _core_genome.csv, _pangenome.csv and the tree's own file of the same run;
    every other output byte-identical to the run without the flag"""
    flags, files = SOURCE[source]
    base = [x for k, v in CLI.items() for x in ("--" + k, v)] + ["--print_dist", "--print_matrices", "--print_selection", "--gpus", gpus, *flags]
    _cli(*base, "--outpref", tmp_path / "no")
    _cli(*base, "--print_parsimony", source, "--outpref", tmp_path / "yes")
    for suffix in USUAL + files:
        assert filecmp.cmp(str(tmp_path / "no") + suffix, str(tmp_path / "yes") + suffix, shallow=False), suffix
    assert set(os.listdir(tmp_path)) == {"no" + s for s in USUAL + files} | {"yes" + s for s in USUAL + files + PARS}
    code = {pa.int_to_base(int(b)): b for b in ref.BASES}
    m = np.array([[code.get(x, 0) for x in line.split(",")] for line in (tmp_path / "yes_core_genome.csv").read_text().splitlines()], np.uint8)
    a = np.loadtxt(tmp_path / "yes_pangenome.csv", delimiter=",", dtype=np.uint8)[:, CLI["core_genes"]:]
    assert m.shape == (100, 301) and a.shape == (100, 400)
    if source == "upgma":
        t = np.loadtxt(tmp_path / "yes_upgma.tsv", usecols=(1, 2), dtype=np.int64)
        left, right = t[:, 0].astype(np.uint32), t[:, 1].astype(np.uint32)
    elif source == "tree":
        t = np.loadtxt(tmp_path / "yes_tree.tsv", usecols=(0, 1), dtype=np.int64)
        left, right = pa.merges_from_tree(t[:, 0], t[:, 1], 100)
    else:
        rows = [line.split("\t") for line in (tmp_path / "yes_genealogy.tsv").read_text().splitlines()]
        order = [int(r[1]) for r in rows]
        coal = [ref.BEYOND if r[2] == "beyond" else int(r[2]) for r in rows[:-1]]
        left, right, _ = pa.merges_from_genealogy(order, coal)
    want = ref.parsimony(m, left, right, a)
    api = pa.parsimony_from_rows(m, left, right)
    par = ref.parents(left, right, 100)
    text = {s: (tmp_path / ("yes" + s)).read_text() for s in PARS}
    assert text["_parsimony_sites.tsv"] == "".join("%d\n" % x for x in want["site_changes"])
    assert text["_parsimony_genes.tsv"] == "".join("%d\t%d\t%d\n" % x for x in zip(want["gene_changes"], want["gene_gains"], want["gene_losses"]))
    assert text["_parsimony_branches.tsv"] == "".join("%d\t%d\t%d\t%d\t%d\n" % (x, par[x], want["branch_changes"][x], want["branch_gains"][x],
                                                                              want["branch_losses"][x]) for x in range(par.size))
    assert text["_parsimony.nwk"] == api.newick() and text["_parsimony.nwk"].count(";\n") == want["trees"]
    summary = "".join("%s\t%d\n" % (k, want[k]) for k in ref.INTEGERS) + "ci\t%s\ntree\t%s\n" % (pa.fmt_f64(want["ci"]), source)
    assert text["_parsimony_summary.tsv"] == summary
    assert want["total_changes"] > 0 and want["gene_total_changes"] > 0
