"""Group differentiation on the device (ps_group_differentiation and its ps_sim / ps_multi forms,
docs/GROUP_DIFFERENTIATION.md) against the numpy restatement over the matrix bytes and the labels
(tests/group_differentiation_ref.py), which shares nothing with the library.  Every comparison is an equality.  The group sizes
are skewed and pairwise different and the members scattered over the rows, so a transposed or permuted membership fragment
cannot pass."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import group_differentiation_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_STATE = -1, -6
BASES = np.array([1, 2, 4, 8], np.uint8)


def onehot(rng, N, L):
    return BASES[rng.integers(0, 4, (N, L))]


def structured(rng, N, L, labels):
    """one-hot rows that follow their label's own random sequence except at a quarter of their cells: groups differ, with fixed
    differences between the small ones"""
    values, inverse = np.unique(labels, return_inverse=True)
    m = onehot(rng, values.size, L)[inverse]
    noise = rng.random((N, L)) < 0.25
    m[noise] = onehot(rng, N, L)[noise]
    return np.ascontiguousarray(m)


def skewed_labels(rng, N, distinct):
    """up to `distinct` label values (arbitrary u32) of pairwise different sizes 1, 2, 3 ... with the rest of the N rows in the
    largest, scattered over the rows"""
    D = distinct
    while D * (D + 1) // 2 > N:
        D -= 1
    sizes = np.arange(1, D + 1)
    sizes[-1] += N - sizes.sum()
    values = rng.choice(2**32 - 1, D, replace=False).astype(np.uint32)
    return np.repeat(values, sizes)[rng.permutation(N)]


# (distinct labels, max_groups, min_size): 16 groups out of 20 labels with some below min_size, one group, a few groups
RUNS = ((20, 16, 3), (20, 1, 1), (5, 16, 1))
SHAPES = [(7, 203), (64, 16), (65, 17), (100, 12000), (1000, 4099), (1024, 64), (1025, 301), (3000, 1000), (8192, 257), (65536, 48)]


def core_handle(pa, m, **kw):
    p = pa.Population(m.shape[0], m.shape[1], 4, True, 0.0, 0, 0, **kw)
    p.load_matrix(m)
    return p


def acc_handle(pa, a, cg=3):
    p = pa.Population(a.shape[0], a.shape[1], 2, False, 0.5, 0, cg)
    p.load_matrix(a)
    return p


def check_core(pa, core, m, labels, max_groups, min_size):
    """every output of the call against the restatement, with and without the optional outputs, and the host form"""
    want = ref.differentiation(m, labels, None, max_groups, min_size)
    full = core.group_differentiation(labels, max_groups=max_groups, min_size=min_size, per_site=True, counts=True)
    ref.assert_equal(full, want)
    assert full.gene_counts is None and full.genes == 0
    bare = core.group_differentiation(labels, max_groups=max_groups, min_size=min_size)
    ref.assert_equal(bare, want, skip=("site_within", "site_total", "counts"))
    assert bare.site_within is None and bare.site_total is None and bare.counts is None
    host = pa.differentiation_from_counts(full.counts, full.group_size)
    for name in ("between", "fixed", "site_within", "site_total"):
        assert np.array_equal(getattr(host, name), getattr(full, name)), name
    for name in ("other_cells", "within_differences", "between_differences", "within_pairs", "between_pairs", "pi_within", "pi_between", "fst"):
        assert getattr(host, name) == getattr(full, name), name
    return full


@pytest.mark.parametrize("N,L", SHAPES)
def test_loaded_matrices(pa, N, L):
    rng = np.random.default_rng(N * 131 + L)
    labels = skewed_labels(rng, N, 20)
    m = structured(rng, N, L, labels)
    core = core_handle(pa, m)
    for distinct, max_groups, min_size in RUNS:
        lab = labels if distinct == 20 else skewed_labels(rng, N, distinct)
        got = check_core(pa, core, m, lab, max_groups, min_size)
        sizes = list(got.group_size)
        assert len(set(sizes)) == len(sizes) and sizes == sorted(sizes, reverse=True) and got.other_cells == 0
        if N >= 210 and max_groups == 16 and distinct == 20:
            assert got.groups == 16 and got.unassigned == 1 + 2 + 3 + 4 and int(np.triu(got.fixed, 1).sum()) > 0
    core.close()


def test_arbitrary_bytes_are_other(pa):
    """3 % random bytes, a site of zeros and a site of 0x03: none of them counts in a plane"""
    rng = np.random.default_rng(77)
    N, L = 1025, 301
    labels = skewed_labels(rng, N, 9)
    m = structured(rng, N, L, labels)
    junk = rng.random((N, L)) < 0.03
    m[junk] = rng.integers(0, 256, int(junk.sum()), dtype=np.uint8)
    m[:, 5], m[:, 17] = 0, 3
    core = core_handle(pa, m)
    got = check_core(pa, core, m, labels, 16, 1)
    assert got.other_cells >= 2 * N and got.site_total[5] == got.site_total[17] == 0 and not got.counts[5].any() and not got.counts[17].any()
    core.close()


def test_identity_against_the_distance_kernels(pa):
    """N = 100, L = 3001, three groups: between[g][h] = the sum over i in g, j in h of the pair's differing sites, from the
    existing ps_pairwise_counts over all 4950 pairs"""
    rng = np.random.default_rng(9)
    N, L = 100, 3001
    labels = skewed_labels(rng, N, 3)
    m = structured(rng, N, L, labels)
    core = core_handle(pa, m)
    got = core.group_differentiation(labels)
    r1, r2 = np.triu_indices(N, 1)
    (h,) = core.pairwise_counts(r1.astype(np.uint32), r2.astype(np.uint32))
    assert h.size == 4950 and not (h & 1).any()
    g1, g2 = got.group_of[r1], got.group_of[r2]
    for g in range(3):
        for k in range(g, 3):
            pairs = ((g1 == g) & (g2 == k)) | ((g1 == k) & (g2 == g))
            assert int(got.between[g, k]) == int((h[pairs] // 2).sum(dtype=np.uint64)), (g, k)
    assert got.groups == 3 and got.within_differences + got.between_differences == int((h // 2).sum(dtype=np.uint64))
    core.close()


@pytest.mark.parametrize("G", [40, 64, 65, 6000])
def test_genes(pa, G):
    rng = np.random.default_rng(G)
    N, L = 300, 130
    labels = skewed_labels(rng, N, 20)
    m = structured(rng, N, L, labels)
    values, inverse = np.unique(labels, return_inverse=True)
    a = (rng.random((values.size, G)) < 0.4)[inverse]
    flip = rng.random((N, G)) < 0.1
    a = np.ascontiguousarray((a ^ flip).astype(np.uint8))
    core, acc = core_handle(pa, m), acc_handle(pa, a)
    for max_groups, min_size in ((16, 3), (1, 1), (4, 1)):
        want = ref.differentiation(m, labels, a, max_groups, min_size)
        got = core.group_differentiation(labels, acc=acc, max_groups=max_groups, min_size=min_size, per_site=True, counts=True)
        ref.assert_equal(got, want)
        assert got.genes == G
    core.close()
    acc.close()


def sim_labels(N):
    """a function of the OUTPUT row: k % 3 in the upper half, one large group below"""
    k = np.arange(N)
    return np.where(k < N // 2, 7, 100 + k % 3).astype(np.uint32)


@pytest.mark.parametrize("N", [100, 1000])
def test_row_order_in_a_simulation(pa, N, tmp_path):
    kw = dict(pop_size=N, core_size=2000, pan_genes=300, core_genes=20, HR_rate=0.5, HGT_rate=0.5, seed=11, n_gen=8, max_distances=100)
    sim = pa.Simulation(pa.make_params(**kw))
    sim.run(5)
    labels = sim_labels(N)
    got = sim.group_differentiation(labels, per_site=True, counts=True)             # no sync: ordered behind the run
    parents = sim.last_parents()
    assert (np.diff(parents.astype(np.int64)) < 0).any()                            # the internal order is not the output order
    m, a = sim.core_genome.read_matrix(), sim.pan_genome.read_matrix()
    want = ref.differentiation(m, labels, a)
    ref.assert_equal(got, want)
    assert got.groups == 4 and got.genes == 280 and got.between_differences > 0
    # labels applied in internal order would be another answer
    assert not np.array_equal(ref.differentiation(m[np.argsort(parents, kind="stable")], labels)["between"], want["between"])
    # the same after save and load
    sim.save(str(tmp_path / "s.state"))
    again = pa.Simulation.load(str(tmp_path / "s.state"))
    ref.assert_equal(again.group_differentiation(labels, per_site=True, counts=True), want)
    again.close()
    # the call changed no state
    sim.run(3)
    plain = pa.Simulation(pa.make_params(**kw))
    plain.run(8)
    assert np.array_equal(plain.core_genome.read_matrix(), sim.core_genome.read_matrix())
    assert np.array_equal(plain.pan_genome.read_matrix(), sim.pan_genome.read_matrix())
    plain.close()
    sim.close()


def test_multi_simulation_equals_the_unsharded_run(pa):
    kw = dict(pop_size=100, core_size=2000, pan_genes=300, core_genes=20, HR_rate=0.5, HGT_rate=0.5, seed=11, n_gen=8, max_distances=100)
    sim = pa.Simulation(pa.make_params(**kw))
    sim.run(5)
    labels = sim_labels(100)
    want = ref.differentiation(sim.core_genome.read_matrix(), labels, sim.pan_genome.read_matrix())
    sim.close()
    multi = pa.MultiSimulation(pa.make_params(**kw), 3, devices=[0, 0, 0])
    multi.run(5)
    ref.assert_equal(multi.group_differentiation(labels, per_site=True, counts=True), want)
    ref.assert_equal(multi.group_differentiation(labels), want, skip=("site_within", "site_total", "counts"))
    # a site shard answers for its own sites, and not with an accessory matrix
    part = multi.shards[1].core_genome.group_differentiation(labels, per_site=True)
    lo = multi.shards[0].core_genome.ncols
    assert np.array_equal(part.site_total, want["site_total"][lo:lo + part.sites]) and 0 < part.sites < 2000
    with pytest.raises(pa.PansimError) as e:
        multi.shards[1].group_differentiation(labels)
    assert e.value.code == PS_ERR_INVALID and "ps_multi_group_differentiation" in str(e.value)
    multi.close()


def test_three_site_shards_add_to_the_whole(pa):
    rng = np.random.default_rng(4)
    N, L = 130, 1000
    labels = skewed_labels(rng, N, 6)
    m = structured(rng, N, L, labels)
    want = ref.differentiation(m, labels)
    cuts = [0, 333, 700, L]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        shard = core_handle(pa, np.ascontiguousarray(m[:, lo:hi]), col_offset=lo, global_cols=L)
        parts.append(shard.group_differentiation(labels, per_site=True, counts=True))
        shard.close()
    assert [p.sites for p in parts] == [333, 367, 300]
    for name in ("between", "fixed"):
        assert np.array_equal(sum(getattr(p, name) for p in parts), want[name]), name
    for name in ("site_within", "site_total", "counts"):
        assert np.array_equal(np.concatenate([getattr(p, name) for p in parts]), want[name]), name
    assert sum(p.within_differences for p in parts) == want["within_differences"]
    assert sum(p.between_differences for p in parts) == want["between_differences"]


def test_the_scratch_grows_and_timing(pa):
    rng = np.random.default_rng(8)
    N, L = 500, 700
    labels = skewed_labels(rng, N, 20)
    two = skewed_labels(rng, N, 2)
    m = structured(rng, N, L, labels)
    core = core_handle(pa, m)
    with pytest.raises(pa.PansimError) as e:
        core.group_differentiation_timing()                  # nothing to report yet
    assert e.value.code == PS_ERR_STATE
    calls = ((two, dict()), (labels, dict(counts=True, per_site=True)), (two, dict()))
    for lab, kw in calls:
        got = core.group_differentiation(lab, **kw)
        fresh = core_handle(pa, m)
        want = fresh.group_differentiation(lab, **kw)
        fresh.close()
        for name in ("between", "fixed", "group_of", "site_within", "counts"):
            assert np.array_equal(getattr(got, name), getattr(want, name)), name
        ref.assert_equal(got, ref.differentiation(m, lab), skip=() if kw else ("site_within", "site_total", "counts"))
        ms = core.group_differentiation_timing()
        assert len(ms) == 3 and all(x >= 0.0 for x in ms) and ms[1] > 0.0 and ms[2] == 0.0
    core.close()


def test_handle_checks(pa):
    rng = np.random.default_rng(6)
    core, acc = core_handle(pa, onehot(rng, 20, 64)), acc_handle(pa, (rng.random((20, 10)) < 0.5).astype(np.uint8))
    labels = np.arange(20, dtype=np.uint32) % 3
    with pytest.raises(pa.PansimError) as e:
        acc.group_differentiation(labels)
    assert e.value.code == PS_ERR_INVALID and "core handle first" in str(e.value)
    with pytest.raises(pa.PansimError) as e:
        core.group_differentiation(labels, acc=core)
    assert e.value.code == PS_ERR_INVALID and "accessory handle" in str(e.value)
    other = pa.Population(21, 10, 2, False, 0.5, 0, 2)
    with pytest.raises(pa.PansimError) as e:
        core.group_differentiation(labels, acc=other)
    assert e.value.code == PS_ERR_INVALID and "20 individuals" in str(e.value)
    with pytest.raises(pa.PansimError) as e:
        core.group_differentiation(np.arange(20, dtype=np.uint32), min_size=2)
    assert e.value.code == PS_ERR_INVALID and "no groups" in str(e.value)
    with pytest.raises(ValueError):
        core.group_differentiation(labels[:-1])
    for bad in (dict(max_groups=0), dict(max_groups=17), dict(min_size=0)):
        with pytest.raises(ValueError):
            core.group_differentiation(labels, **bad)
    shard = pa.Population(20, 32, 4, True, 0.0, 0, 0, col_offset=32, global_cols=64)
    with pytest.raises(pa.PansimError) as e:
        shard.group_differentiation(labels, acc=acc)
    assert e.value.code == PS_ERR_INVALID and "ps_multi_group_differentiation" in str(e.value)
    big = pa.Population(65537, 16, 4, True, 0.0, 0, 0)
    with pytest.raises(pa.PansimError) as e:
        big.group_differentiation(np.zeros(65537, np.uint32))
    assert e.value.code == PS_ERR_INVALID and "65536" in str(e.value)
    for p in (core, acc, other, shard, big):
        p.close()


CLI = dict(pop_size=100, core_size=300, pan_genes=600, core_genes=200, n_gen=4, seed=9, max_distances=500, HR_rate=0.5)
CLI_CORE_MAX, CLI_ACC_MAX = 0.2, 0.4
USUAL = (".tsv", "_freqs.txt", "_core_genome.csv", "_pangenome.csv", "_per_gen.tsv", "_selection.tsv", "_clusters.tsv", "_clusters_summary.tsv")
DIFF = ("_diff_groups.tsv", "_diff_between.tsv", "_diff_sites.tsv", "_diff_genes.tsv", "_diff_summary.tsv")


def _cli(*args):
    r = subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def _rows(rows):
    return "".join("\t".join(str(int(x)) for x in row) + "\n" for row in rows)


@pytest.mark.parametrize("gpus", [1, 2])
def test_cli_print_differentiation(pa, tmp_path, gpus):
    """the five files recomputed from _core_genome.csv, _pangenome.csv and _clusters.tsv of the same run; every other output
    byte-identical to the run without the flag"""
    base = [x for k, v in CLI.items() for x in ("--" + k, v)] + ["--print_dist", "--print_matrices", "--print_selection", "--gpus", gpus,
                                                                 "--print_clusters", "--cluster_core_max", CLI_CORE_MAX, "--cluster_acc_max", CLI_ACC_MAX]
    _cli(*base, "--outpref", tmp_path / "no")
    _cli(*base, "--print_differentiation", "--diff_max_groups", 5, "--outpref", tmp_path / "yes")
    for suffix in USUAL:
        assert filecmp.cmp(str(tmp_path / "no") + suffix, str(tmp_path / "yes") + suffix, shallow=False), suffix
    assert set(os.listdir(tmp_path)) == {"no" + s for s in USUAL} | {"yes" + s for s in USUAL + DIFF}
    code = {pa.int_to_base(int(b)): b for b in BASES}
    m = np.array([[code.get(x, 0) for x in line.split(",")] for line in (tmp_path / "yes_core_genome.csv").read_text().splitlines()], np.uint8)
    a = np.loadtxt(tmp_path / "yes_pangenome.csv", delimiter=",", dtype=np.uint8)[:, CLI["core_genes"]:]
    labels = np.loadtxt(tmp_path / "yes_clusters.tsv", dtype=np.int64)[:, 1].astype(np.uint32)
    assert m.shape == (100, 300) and a.shape == (100, 400)
    want = ref.differentiation(m, labels, a, max_groups=5, min_size=2)
    K, n = want["groups"], want["group_size"]
    assert K >= 2 and (n >= 2).all()
    b, f, ab, gf = want["between"], want["fixed"], want["acc_between"], want["gene_fixed"]
    text = {s: (tmp_path / ("yes" + s)).read_text() for s in DIFF}
    assert text["_diff_groups.tsv"] == _rows((g, want["group_label"][g], n[g], b[g, g], f[g, g], want["gene_private"][g]) for g in range(K))
    assert text["_diff_between.tsv"] == _rows((g, h, int(n[g]) * int(n[h]), b[g, h], f[g, h], ab[g, h], gf[g, h], gf[h, g])
                                              for g in range(K) for h in range(g + 1, K))
    assert text["_diff_sites.tsv"] == _rows(zip(want["site_within"], want["site_total"]))
    assert text["_diff_genes.tsv"] == _rows(want["gene_counts"])
    names = ("pop_size", "sites", "genes", "groups", "assigned", "unassigned", "other_cells", "within_pairs", "between_pairs", "within_differences",
             "between_differences")
    summary = "".join("%s\t%d\n" % (k, want[k]) for k in names) + "".join("%s\t%s\n" % (k, pa.fmt_f64(want[k])) for k in ref.DOUBLES)
    assert text["_diff_summary.tsv"] == summary + "diff_max_groups\t5\ndiff_min_size\t2\n"
