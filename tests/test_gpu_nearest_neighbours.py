"""Nearest neighbours on the device (ps_nearest_neighbours and its ps_sim / ps_multi forms, docs/NEAREST_NEIGHBOURS.md) against the
plain restatement (tests/nearest_neighbours_ref.py) over the matrices that read_matrix() returns -- a path that shares nothing
with the new code.  Every comparison is an equality of the three (N, k) arrays and of every integer field; the doubles are
compared bit for bit with (double)num / (double)den."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import nearest_neighbours_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_STATE = -1, -6
BASES = np.array([1, 2, 4, 8], np.uint8)
METRICS = (("core", ref.CORE), ("acc", ref.ACC))


def _onehot(rng, N, L):
    return BASES[rng.integers(0, 4, (N, L))]


def related(rng, N, L, G, founders=5):
    """`founders` unrelated individuals; every other one copies an earlier one and moves away by up to 2 core sites and up to 2
    gene flips: near neighbours at few distinct small distances, so ties at the head of every list"""
    core, acc = _onehot(rng, N, L), (rng.random((N, G)) < 0.4).astype(np.uint8)
    for k in range(min(founders, N), N):
        src = rng.integers(k)
        core[k], acc[k] = core[src], acc[src]
        sites = rng.choice(L, rng.integers(0, 3), replace=False)
        core[k, sites] = BASES[(np.log2(core[k, sites]).astype(int) + 1 + rng.integers(0, 3, sites.size)) % 4]
        if G:
            acc[k, rng.choice(G, rng.integers(0, 3), replace=False)] ^= 1
    order = rng.permutation(N)
    return np.ascontiguousarray(core[order]), np.ascontiguousarray(acc[order])


def _handles(pa, core_matrix, acc_matrix, cg, G=None):
    N, L = core_matrix.shape
    core = pa.Population(N, L, 4, True, 0.0, 0, 0)
    core.load_matrix(core_matrix)
    acc = pa.Population(N, acc_matrix.shape[1] if acc_matrix is not None else G, 2, False, 0.5, 0, cg)
    if acc_matrix is not None:
        acc.load_matrix(acc_matrix)
    return core, acc


def _check(core, acc, core_m, acc_m, cg, k, ranks=None):
    """both metrics on the device against the restatement of the two matrices -> the two results"""
    nums = ref.numerators(core_m, acc_m)
    out = []
    for name, metric in METRICS:
        got = core.nearest_neighbours(acc, k, metric=name)
        want = ref.neighbours(metric, core_m, acc_m, cg, k, nums)
        ref.assert_equal(got, want)
        N = core_m.shape[0]
        assert got.pairs == N * (N - 1) // 2 and got.graph_edges + got.mutual_edges == N * k
        for rank in ranks or sorted({1, k}):
            ref.assert_lineages(got.lineages(rank), want["nbr"], rank)
        counts_ms, select_ms = core.nearest_neighbours_timing()
        assert select_ms > 0.0 and (counts_ms > 0.0 or (name == "acc" and acc.ncols == 0))
        out.append(got)
    return out


@pytest.mark.parametrize("N,L,G,k", [(2, 8, 5, 1), (7, 203, 40, 6), (64, 130, 64, 5), (65, 130, 65, 64), (300, 1001, 500, 5),
                                     (1000, 4099, 600, 10), (1025, 301, 130, 3), (2500, 130, 300, 128)])
def test_loaded_matrices(pa, N, L, G, k):
    """one-hot matrices of related individuals, cg = 3: lane tails, the 256-tile edge, the 1024 edge, k at both ends of its range,
    a row longer than one trip"""
    rng = np.random.default_rng(N)
    core_m, acc_m = related(rng, N, L, G)
    core, acc = _handles(pa, core_m, acc_m, 3)
    by_core, by_acc = _check(core, acc, core_m, acc_m, 3, k)
    assert by_core.undefined_neighbours == 0 and by_acc.undefined_neighbours == 0
    if N >= 64:
        assert len(np.unique(by_core.num)) > 1 and (by_core.num[:, 0] <= 2).sum() > N // 2      # (a copy is near its source)
    core.close()
    acc.close()


def test_identical_individuals_list_the_lowest_rows(pa):
    """a simulation at generation 0 is clonal: every list is the k lowest rows other than i, all at distance 0"""
    N, k = 100, 5
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=2048, pan_genes=300, core_genes=20, seed=4, n_gen=3, max_distances=100))
    core_m, acc_m = sim.core_genome.read_matrix(), sim.pan_genome.read_matrix()
    assert (core_m == core_m[0]).all() and (acc_m == acc_m[0]).all()
    for name, metric in METRICS:
        got = sim.nearest_neighbours(k, metric=name)
        ref.assert_equal(got, ref.neighbours(metric, core_m, acc_m, 20, k))
        for i in range(N):
            assert list(got.nbr[i]) == [j for j in range(N) if j != i][:k]
        assert not got.num.any() and got.den.all() and not got.distance.any()
        assert got.mutual_edges == k * (k + 1) // 2 and got.lineages(1)[1]["lineages"] == 1
    sim.close()


def test_not_one_hot(pa):
    """arbitrary bytes in about 3 % of the cells: the generic count form, odd h among the numerators"""
    rng = np.random.default_rng(31)
    N, L, G = 130, 300, 40
    core_m, acc_m = related(rng, N, L, G)
    cells = rng.random((N, L)) < 0.03
    core_m[cells] = rng.integers(0, 256, int(cells.sum()), dtype=np.uint8)
    assert (ref.numerators(core_m, acc_m)[0] & 1).any()
    core, acc = _handles(pa, core_m, acc_m, 2)
    _check(core, acc, core_m, acc_m, 2, 7)
    core.close()
    acc.close()


def test_empty_accessory_rows(pa):
    """N = 70, G = 40, five all-zero accessory rows and no core genes: their mutual pairs are 0 / 0, sort last by row and are
    counted; with every row empty, and with G = 0, every entry is undefined (or 0 / cg with core genes)"""
    rng = np.random.default_rng(3)
    N, L, G = 70, 130, 40
    core_m = _onehot(rng, N, L)
    A = (rng.random((N, G)) < 0.2).astype(np.uint8)
    A[0, 0] = 1
    empty = [3, 17, 18, 40, 69]
    A[A.sum(1) == 0, 1] = 1
    A[empty] = 0
    core, acc = _handles(pa, core_m, A, 0)
    _, got = _check(core, acc, core_m, A, 0, N - 1)
    assert got.undefined_neighbours == 20
    for e in empty:
        assert list(got.nbr[e, -4:]) == [j for j in empty if j != e] and not got.den[e, -4:].any() and got.den[e, :-4].all()
        assert (got.num[e, :-4] == got.den[e, :-4]).all()                 # (an empty row is at 1 / 1 from every other)
    _, got = _check(core, acc, core_m, A, 0, 3)
    assert got.undefined_neighbours == 0                                  # (65 defined distances come first)
    # all individuals empty
    Z = np.zeros_like(A)
    acc.load_matrix(Z)
    _, got = _check(core, acc, core_m, Z, 0, 4)
    assert got.undefined_neighbours == N * 4 and np.isnan(got.distance).all() and list(got.nbr[2]) == [0, 1, 3, 4]
    core.close()
    acc.close()
    # G = 0
    for cg in (0, 3):
        core, acc = _handles(pa, core_m, None, cg, G=0)
        _, got = _check(core, acc, core_m, np.zeros((N, 0), np.uint8), cg, 4)
        assert got.undefined_neighbours == (0 if cg else N * 4) and not got.num.any() and (got.den == cg).all()
        assert list(got.nbr[2]) == [0, 1, 3, 4]
        core.close()
        acc.close()


def test_three_bands_equal_one(pa):
    """N = 700 with bands of 256 rows (three bands, the last of 188) equals the unforced call"""
    rng = np.random.default_rng(7)
    N, L, G, k = 700, 260, 130, 6
    core_m, acc_m = related(rng, N, L, G)
    core, acc = _handles(pa, core_m, acc_m, 1)
    whole = _check(core, acc, core_m, acc_m, 1, k)
    core.set_tuning("core_davg_band", 256)
    for (name, _), w in zip(METRICS, whole):
        got = core.nearest_neighbours(acc, k, metric=name)
        for a in ("nbr", "num", "den"):
            assert np.array_equal(getattr(got, a), getattr(w, a)), (name, a)
        assert all(getattr(got, f) == getattr(w, f) for f in ref.INT_FIELDS)
    core.close()
    acc.close()


def test_limits(pa):
    rng = np.random.default_rng(6)
    core, acc = _handles(pa, _onehot(rng, 20, 64), (rng.random((20, 10)) < 0.5).astype(np.uint8), 2)
    with pytest.raises(pa.PansimError) as e:
        core.nearest_neighbours_timing()
    assert e.value.code == PS_ERR_STATE and "no nearest neighbours" in str(e.value)
    for name, _ in METRICS:
        for k in (0, 20, 129):
            with pytest.raises(pa.PansimError) as e:
                core.nearest_neighbours(acc, k, metric=name)
            assert e.value.code == PS_ERR_INVALID and "1 <= k <= min(pop_size - 1, 128)" in str(e.value)
        assert core.nearest_neighbours(acc, 19, metric=name).nbr.shape == (20, 19)
    wide = pa.Population(20, 65536, 2, False, 0.5, 0, 2)
    for name, _ in METRICS:
        with pytest.raises(pa.PansimError) as e:
            core.nearest_neighbours(wide, 3, metric=name)
        assert e.value.code == PS_ERR_INVALID and "65535 accessory genes" in str(e.value)
    huge = pa.Population(20, 10, 2, False, 0.5, 0, 2**32 - 65535)
    with pytest.raises(pa.PansimError) as e:
        core.nearest_neighbours(huge, 3, metric="acc")
    assert e.value.code == PS_ERR_INVALID and "core_genes + 65535 < 2^32" in str(e.value)
    for a, b in ((core, core), (acc, acc), (acc, core)):
        with pytest.raises(pa.PansimError) as e:
            a.nearest_neighbours(b, 3)
        assert e.value.code == PS_ERR_INVALID and "core handle first" in str(e.value)
    with pytest.raises(ValueError):
        core.nearest_neighbours(acc, 3, metric="joint")
    # a site shard on its own
    shard = pa.Population(20, 32, 4, True, 0.0, 0, 0, col_offset=32, global_cols=64)
    with pytest.raises(pa.PansimError) as e:
        shard.nearest_neighbours(acc, 3)
    assert e.value.code == PS_ERR_INVALID and "ps_multi_nearest_neighbours" in str(e.value)
    for p in (core, acc, wide, huge, shard):
        p.close()


SIM = dict(pop_size=200, core_size=2048, pan_genes=300, core_genes=20, HR_rate=0.5, HGT_rate=0.5, prop_positive=0.5, seed=11, n_gen=9,
           max_distances=100)
K = 6


def _restated(sim):
    core_m, acc_m = sim.core_genome.read_matrix(), sim.pan_genome.read_matrix()
    nums = ref.numerators(core_m, acc_m)
    return [ref.neighbours(metric, core_m, acc_m, SIM["core_genes"], K, nums) for _, metric in METRICS]


@pytest.fixture(scope="module")
def sim_after_five(pa, tmp_path_factory):
    """the unsharded run with selection and HR on: neighbours asked for after generation 3 (not compared) and after generation 5
    without a sync, the restatement of its matrices there, the sibling read-outs there, the same from a state file saved there,
    and its state after 9 generations"""
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.run(3)
    sim.nearest_neighbours(K)
    sim.run(2)
    got = [sim.nearest_neighbours(K, metric=name) for name, _ in METRICS]          # no sync: ordered behind the run
    want = _restated(sim)
    trees = [sim.linkage_tree(metric=name) for name, _ in METRICS]
    d_max = int(np.median(got[0].num[:, -1]))
    a_num, a_den = int(np.median(got[1].num[:, -1])), int(np.median(got[1].den[:, -1]))
    clusters = (d_max, sim.strain_clusters(core_max_d=d_max).labels), ((a_num, a_den), sim.strain_clusters(acc_ratio=(a_num, a_den)).labels)
    path = str(tmp_path_factory.mktemp("knn") / "five.state")
    sim.save(path)
    sim.run(4)
    state = (sim.core_genome.read_matrix(), sim.pan_genome.read_matrix(), sim.last_parents())
    sim.close()
    loaded = pa.Simulation.load(path)
    again = [loaded.nearest_neighbours(K, metric=name) for name, _ in METRICS], _restated(loaded)
    loaded.close()
    return got, want, trees, clusters, again, state


def test_row_order_in_a_simulation(pa, sim_after_five):
    got, want, _, _, (again, again_want), state = sim_after_five
    for g, w, a, aw in zip(got, want, again, again_want):
        ref.assert_equal(g, w)
        ref.assert_equal(a, aw)
        ref.assert_equal(a, w)                              # (the loaded run holds the same individuals in the same rows)
    assert len(np.unique(got[0].num)) > 1 and (np.sort(got[0].nbr, 1) != np.arange(K)).any()
    # the calls changed no state: the run that asked continues bit for bit with one that never did
    plain = pa.Simulation(pa.make_params(**SIM))
    plain.run(9)
    assert np.array_equal(plain.core_genome.read_matrix(), state[0]) and np.array_equal(plain.pan_genome.read_matrix(), state[1])
    assert np.array_equal(plain.last_parents(), state[2])
    plain.close()


def test_the_siblings_agree(pa, sim_after_five):
    """every pair (i, nbr[i, 0]) is an edge of the linkage tree of the same metric, at the same distance; every listed neighbour at
    a distance within a threshold carries i's strain-clusters label at that threshold"""
    got, _, trees, clusters, _, _ = sim_after_five
    for g, tree in zip(got, trees):
        edges = {(int(a), int(b)): (int(n), int(d)) for a, b, n, d in zip(tree.lo, tree.hi, tree.num, tree.den)}
        for i in range(g.pop_size):
            j = int(g.nbr[i, 0])
            assert edges.get((min(i, j), max(i, j))) == (int(g.num[i, 0]), int(g.den[i, 0])), i
    (d_max, labels), ((a_num, a_den), a_labels) = clusters
    within = got[0].num <= d_max
    assert within.any()
    assert (labels[got[0].nbr][within] == np.broadcast_to(labels[:, None], within.shape)[within]).all()
    num, den = got[1].num, got[1].den                                      # (a <= 65535, b < 2^32: the products fit u64)
    within = (den != 0) & (num * np.uint64(a_den) <= np.uint64(a_num) * den)
    assert within.any()
    assert (a_labels[got[1].nbr][within] == np.broadcast_to(a_labels[:, None], within.shape)[within]).all()


def test_three_shards_equal_the_unsharded_run(pa, sim_after_five):
    _, want, _, _, _, _ = sim_after_five
    multi = pa.MultiSimulation(pa.make_params(**SIM), 3, devices=[0, 0, 0])
    multi.run(5)
    for (name, _), w in zip(METRICS, want):
        ref.assert_equal(multi.nearest_neighbours(K, metric=name), w)
    with pytest.raises(pa.PansimError) as e:             # a site shard on its own
        multi.shards[1].nearest_neighbours(K)
    assert e.value.code == PS_ERR_INVALID and "ps_multi_nearest_neighbours" in str(e.value)
    multi.close()


CLI = dict(pop_size=100, core_size=300, pan_genes=600, core_genes=200, n_gen=4, seed=9, max_distances=500, HR_rate=0.5)
USUAL = (".tsv", "_freqs.txt", "_core_genome.csv", "_pangenome.csv", "_per_gen.tsv", "_selection.tsv")
NEW = ("_knn.tsv", "_lineages.tsv", "_knn_summary.tsv")


def _cli(*args):
    r = subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def _read_csv(path, lut):
    rows = open(path, "rb").read().splitlines()
    text = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)[:, ::2]
    return lut[text]


@pytest.mark.parametrize("mode,metric", [("plain", "core"), ("plain", "acc"), ("gpus2", "core"), ("gpus2", "acc"), ("load_state", "core")])
def test_cli_print_knn(pa, tmp_path, mode, metric):
    """the three files equal the restatement of the matrices the same run wrote, as text; the usual outputs do not change"""
    base = [x for k, v in CLI.items() for x in ("--" + k, v)] + ["--print_dist", "--print_matrices", "--print_selection"]
    flags = ["--print_knn", 4] + (["--knn_metric", metric] if metric != "core" else [])
    if mode == "gpus2":
        base += ["--gpus", 2]
    if mode == "load_state":
        state = tmp_path / "half.state"
        _cli(*base[:8], "--n_gen", 2, *base[10:], "--outpref", tmp_path / "half", "--save_state", state)
        for f in os.listdir(tmp_path):
            if f.startswith("half_") or f == "half.tsv":
                os.remove(tmp_path / f)
        base += ["--load_state", state]
    _cli(*base, "--outpref", tmp_path / "no")
    _cli(*base, *flags, "--outpref", tmp_path / "yes")
    for suffix in USUAL:
        assert filecmp.cmp(str(tmp_path / "no") + suffix, str(tmp_path / "yes") + suffix, shallow=False), suffix
    extra = {"half.state"} if mode == "load_state" else set()
    assert set(os.listdir(tmp_path)) == {"no" + s for s in USUAL} | {"yes" + s for s in USUAL + NEW} | extra
    lut = np.zeros(256, np.uint8)
    for ch, v in zip(b"ACGT01", (1, 2, 4, 8, 0, 1)):
        lut[ch] = v
    core_m, pan = _read_csv(tmp_path / "yes_core_genome.csv", lut), _read_csv(tmp_path / "yes_pangenome.csv", lut)
    cg = CLI["core_genes"]
    assert core_m.shape == (100, 300) and pan.shape[0] == 100 and pan[:, :cg].all()      # (the core genes lead every line as 1s)
    want = ref.neighbours(dict(METRICS)[metric], core_m, pan[:, cg:], cg, 4)
    for suffix, text in zip(NEW, ref.tsv_files(want, pa.fmt_f64)):
        assert (tmp_path / ("yes" + suffix)).read_text() == text, suffix
