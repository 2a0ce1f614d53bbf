"""Tree comparison on the device (ps_tree_compare and its ps_sim / ps_multi forms, docs/TREE_COMPARISON.md) against the numpy
restatement over the two merge lists (tests/tree_compare_ref.py), which shares nothing with the library.  Integers and arrays
are compared by equality, the doubles within 1e-12 (tests/test_tree_compare.py says why).  The shapes are the smallest at which
each thing can still go wrong: one pair, one triple, the lane boundary (64 / 65), the four-column lane and the chunk boundary
(255 / 256 / 257), more than one chunk per wave (1000 / 1025), several row groups of the rank table (4096); N = 16384 -- the
u16 table's largest entry, hi = 16384 in the packed interval, 2^27 pairs and the 512 MB of scratch -- against the closed forms."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import tree_compare_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_STATE = -1, -6
SIZES = (2, 3, 64, 65, 255, 256, 257, 1000, 1025, 4096)
PAIRS = (("random", "random"), ("caterpillar", "balanced"), ("forest", "random"), ("permuted", "permuted"))
TRIPLET_FIELDS = ("triples", "resolved_a", "resolved_b", "shared_triplets", "triplet_recall", "triplet_precision")


def handle(pa, N):
    """any handle of N individuals: no matrix is read"""
    return pa.Population(N, 16, 4, True, 0.0, 0, 0)


def tree_pair(rng, N, x, y):
    ts = ref.trees(rng, N)
    if x not in ts:
        assert N < 4 and x == "forest"                          # (three leaves have no forest: a lone merge is one)
        x = "caterpillar"
        ts[x] = (ts[x][0][:1], ts[x][1][:1])
    return ts[x], ref.random_joining(rng, N) if (x, y) == ("random", "random") else ts[y]


def without_triplets(want):
    out = dict(want)
    out.update({name: 0 for name in TRIPLET_FIELDS})
    return out


@pytest.mark.parametrize("x,y", PAIRS)
@pytest.mark.parametrize("N", SIZES)
def test_device_equals_the_restatement(pa, N, x, y):
    rng = np.random.default_rng(N * 31 + len(x) + len(y))
    a, b = tree_pair(rng, N, x, y)
    h = handle(pa, N)
    tied = (*a, ref.tied_values(len(a[0]), 3)), (*b, ref.tied_values(len(b[0]), 2))
    for ta, tb in (tied, (a, b)):
        want = ref.compare(N, ta, tb)
        ref.assert_equal(h.tree_compare(ta, tb), want)
        ref.assert_equal(h.tree_compare(ta, tb, triplets=False), without_triplets(want))
    h.close()
    if (x, y) == ("permuted", "permuted"):
        assert want["rf_distance"] == 0 and want["shared_triplets"] == want["resolved_a"]
    if x == "forest" and N >= 4:
        assert want["joined_b_only"] > 0 and want["joined_a_only"] == 0


@pytest.mark.parametrize("bins,spans", [((1, 1), (0, 0)), ((127, 127), (0, 0)), ((32, 32), (100, 5000)), ((1023, 15), (0, 7))])
def test_bins_and_spans(pa, bins, spans):
    rng = np.random.default_rng(4)
    N = 1000
    a, b = ref.genealogy_tree(rng, N, depth=40, beyond=0.01), (*ref.random_joining(rng, N), ref.tied_values(N - 1, 4))
    h = handle(pa, N)
    got = h.tree_compare(a, b, bins=bins, spans=spans)
    h.close()
    ref.assert_equal(got, ref.compare(N, a, b, bins=bins, spans=spans))
    assert int(got.joint.sum()) == got.pairs and got.joined_b_only > 0


def test_device_equals_the_host_form_and_reuses_the_slot(pa):
    """a larger call, then a smaller one on the same handle's slot, both against ps_tree_compare_from_merges on the same
    input; the timing entry before and after"""
    rng = np.random.default_rng(9)
    N = 2000
    h = handle(pa, N)
    with pytest.raises(pa.PansimError) as e:
        h.tree_compare_timing()
    assert e.value.code == PS_ERR_STATE and "no tree comparison" in str(e.value)
    big = ref.random_joining(rng, N), ref.genealogy_tree(rng, N, depth=30, beyond=0.02)
    small = ref.random_joining(rng, N, 40), ref.random_joining(rng, N, 700)
    for (a, b), kw in ((big, dict(bins=(64, 64))), (small, dict(bins=(3, 3), triplets=False)), (small, dict()), (big, dict(spans=(7, 9)))):
        got, host = h.tree_compare(a, b, **kw), pa.tree_compare_from_merges(N, a, b, **kw)
        ref.assert_equal(got, host.as_dict())
        ms = h.tree_compare_timing()
        assert len(ms) == 2 and all(np.isfinite(x) and x > 0.0 for x in ms)
    h.close()


def test_the_largest_population(pa):
    """N = 16384 without an O(N^2) restatement: the marginals and the row and column sums of joint against the closed forms, a
    tree against itself, and the (A, B) / (B, A) symmetry"""
    rng = np.random.default_rng(16384)
    N = 16384
    a = (*ref.random_joining(rng, N), ref.tied_values(N - 1, 3))
    b = ref.caterpillar(N, rng.permutation(N))
    h = handle(pa, N)
    ab, ba, aa = h.tree_compare(a, b), h.tree_compare(b, a), h.tree_compare(a, a, bins=(64, 64))
    bare = h.tree_compare(a, b, triplets=False)
    h.close()
    for got, (ja, ra, s1, s2), (jb, rb, t1, t2) in ((ab, ref.closed_forms(N, a), ref.closed_forms(N, b)), (ba, ref.closed_forms(N, b), ref.closed_forms(N, a))):
        assert ja == jb == got.pairs == got.joined_both == N * (N - 1) // 2
        assert (got.resolved_a, got.sum_a, got.sum_aa, got.resolved_b, got.sum_b, got.sum_bb) == (ra, s1, s2, rb, t1, t2)
        assert got.triples == N * (N - 1) * (N - 2) // 6 and 0 < got.shared_triplets <= min(ra, rb)
    # the marginals of joint: the pairs of every merge of a tree fall into its value's bin
    for got, t, axis in ((ab, a, 1), (ab, b, 0)):
        T_val = np.arange(1, N, dtype=np.int64) if len(t) == 2 else t[2].astype(np.int64)
        size = np.ones(2 * N - 1, np.int64)
        for k in range(N - 1):
            size[N + k] = size[t[0][k]] + size[t[1][k]]
        w = size[t[0].astype(np.int64)] * size[t[1].astype(np.int64)]
        want = np.bincount(ref.value_bin(T_val, 32, int(T_val.max())), weights=w, minlength=33).astype(np.uint64)
        np.testing.assert_array_equal(got.joint.sum(axis=axis), want)
    np.testing.assert_array_equal(ab.joint, ba.joint.T)
    assert (ab.sum_ab, ab.shared_triplets, ab.shared_clades, ab.cophenetic_r) == (ba.sum_ab, ba.shared_triplets, ba.shared_clades, ba.cophenetic_r)
    np.testing.assert_array_equal(ab.in_b, ba.in_a)
    assert aa.shared_triplets == aa.resolved_a == aa.resolved_b == ab.resolved_a and aa.rf_distance == 0 and aa.cophenetic_r == 1.0
    assert not (aa.joint - np.diag(np.diag(aa.joint))).any() and aa.sum_ab == aa.sum_aa == ab.sum_aa
    np.testing.assert_array_equal(bare.joint, ab.joint)
    assert (bare.sum_ab, bare.shared_triplets, bare.resolved_a) == (ab.sum_ab, 0, 0)


def test_pop_size_comes_from_the_handle(pa):
    h = handle(pa, 20)
    with pytest.raises(pa.PansimError) as e:
        h.tree_compare(ref.caterpillar(21), ref.caterpillar(20))
    assert e.value.code == PS_ERR_INVALID and "1 .. 19 merges" in str(e.value)
    with pytest.raises(pa.PansimError) as e:
        h.tree_compare(ref.caterpillar(20), ref.caterpillar(20), bins=(0, 1))
    assert e.value.code == PS_ERR_INVALID
    h.close()
    big = handle(pa, 16385)
    with pytest.raises(pa.PansimError) as e:
        big.tree_compare(ref.caterpillar(16385), ref.caterpillar(16385))
    assert e.value.code == PS_ERR_INVALID and "16384" in str(e.value)
    big.close()


SIM = dict(pop_size=200, core_size=2000, pan_genes=600, core_genes=200, n_gen=50, seed=7, max_distances=100, HR_rate=0.5, HGT_rate=0.5)


def test_simulation_and_shards(pa):
    """the target use on a run and on two shards with the same seed"""
    sim = pa.Simulation(pa.make_params(**SIM))
    sim.record_ancestry(30)
    sim.run(50)
    g, u, t = sim.genealogy(), sim.upgma_tree(), sim.linkage_tree()
    got = sim.tree_compare(g, u)
    a, b = g.merges(), (*u.merges(), u.levels())
    ref.assert_equal(got, ref.compare(200, a, b))
    assert got.merges_b == 199 and got.joined_b_only == got.pairs - got.joined_both and got.clades_b <= 199
    ref.assert_equal(sim.tree_compare(u, t, bins=(8, 8)), ref.compare(200, b, (*t.merges(), t.levels()), bins=(8, 8)))
    ref.assert_equal(sim.tree_compare(g, u, values=(None, np.arange(1, 200))), ref.compare(200, a, u.merges()))
    assert all(x > 0.0 for x in sim.tree_compare_timing())
    sim.close()
    multi = pa.MultiSimulation(pa.make_params(**SIM), 2, devices=[0, 0])
    multi.record_ancestry(30)
    multi.run(50)
    ref.assert_equal(multi.tree_compare(multi.genealogy(), multi.upgma_tree()), got.as_dict())
    assert len(multi.tree_compare_timing()) == 2
    multi.close()


CLI = dict(pop_size=200, core_size=2000, pan_genes=600, core_genes=200, n_gen=50, seed=7, max_distances=100, HR_rate=0.5, HGT_rate=0.5)
FILES = ("_tree_compare.tsv", "_tree_compare_clades.tsv", "_tree_compare_summary.tsv")


def _cli(*args):
    r = subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_print_tree_compare(pa, tmp_path):
    """the three files against the Python API on the run's own tree files; --gpus 2 byte-identical to one GPU; every other
    output byte-identical to the run without the flag"""
    base = [x for k, v in CLI.items() for x in ("--" + k, v)] + ["--print_genealogy", 30, "--print_upgma"]
    _cli(*base, "--outpref", tmp_path / "no")
    _cli(*base, "--print_tree_compare", "genealogy,upgma", "--tree_compare_bins", "16,8", "--outpref", tmp_path / "one")
    _cli(*base, "--print_tree_compare", "genealogy,upgma", "--tree_compare_bins", "16,8", "--gpus", 2, "--outpref", tmp_path / "two")
    names = sorted(os.listdir(tmp_path))
    usual = [n[2:] for n in names if n.startswith("no")]
    assert [n[3:] for n in names if n.startswith("one")] == sorted(usual + list(FILES))
    for suffix in usual:
        assert filecmp.cmp(str(tmp_path / "no") + suffix, str(tmp_path / "one") + suffix, shallow=False), suffix
    for suffix in usual + list(FILES):
        assert filecmp.cmp(str(tmp_path / "one") + suffix, str(tmp_path / "two") + suffix, shallow=False), suffix
    rows = [line.split("\t") for line in (tmp_path / "one_genealogy.tsv").read_text().splitlines()]
    order = [int(r[1]) for r in rows]
    coal = [0xFFFFFFFF if r[2] == "beyond" else int(r[2]) for r in rows[:-1]]
    a = pa.merges_from_genealogy(order, coal)
    t = np.loadtxt(tmp_path / "one_upgma.tsv", usecols=(1, 2, 4, 5), dtype=np.uint64)
    b = (t[:, 0].astype(np.uint32), t[:, 1].astype(np.uint32), pa.levels_from_heights(t[:, 2], t[:, 3]))
    want = pa.tree_compare_from_merges(200, a, b, bins=(16, 8))
    ref.assert_equal(want, ref.compare(200, a, b, bins=(16, 8)))
    text = {s: (tmp_path / ("one" + s)).read_text() for s in FILES}
    assert text["_tree_compare.tsv"] == "".join("%d\t%d\t%d\n" % (i, j, want.joint[i, j]) for i in range(17) for j in range(9) if want.joint[i, j])
    clades = ""
    for name, (left, right, val), shared in (("genealogy", a, want.in_b), ("upgma", b, want.in_a)):
        T = ref.Tree(200, left, right, val)
        clades += "".join("%s\t%d\t%d\t%d\t%d\n" % (name, 200 + k, T.size[k], T.val[k], shared[k]) for k in range(T.M) if T.is_top[k])
    assert text["_tree_compare_clades.tsv"] == clades
    summary = "".join("%s\t%d\n" % (k, getattr(want, k)) for k in ref.INT_FIELDS) + \
        "".join("%s\t%s\n" % (k, pa.fmt_f64(getattr(want, k))) for k in ref.DOUBLES) + "a\tgenealogy\nb\tupgma\n"
    assert text["_tree_compare_summary.tsv"] == summary
    assert want.joined_both > 0 and want.shared_clades > 0
