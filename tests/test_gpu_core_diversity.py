"""Core allele counts and diversity on the device (ps_site_allele_counts / ps_core_diversity, docs/CORE_DIVERSITY.md)
against the numpy restatement (tests/core_diversity_ref.py) of the matrix the library itself reads back, against the
existing distance kernels through the identity sum_{i<j} d(i, j) = sum_s (N^2 - sum_c n_c^2) / 2, on running
simulations, across site shards and through the command line.  Every comparison of integers is an equality."""
import filecmp
import itertools
import os
import subprocess

import numpy as np
import pytest

import core_diversity_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID = -1


def _onehot(rng, N, L):
    """random one-hot cells, sites of every skew among them (fixed, nearly fixed, even)"""
    p = rng.dirichlet([0.25] * 4, L)
    u = rng.random((N, L))
    m = (u[:, :, None] > np.cumsum(p, 1)[None, :, :3]).sum(2)
    m[:, 0] = 2                      # a monomorphic site
    return (1 << m).astype(np.uint8)


def _core(pa, N, L, **kw):
    return pa.Population(N, L, 4, True, 0.0, 0, 0, **kw)


def _check(pa, pop, M=None):
    """counts and summary of the handle against the restatement of the matrix it reads back (or of M)"""
    M = pop.read_matrix() if M is None else M
    counts = pop.site_allele_counts()
    assert counts.dtype == np.uint32 and counts.shape == (M.shape[1], 4)
    want_counts = ref.site_counts(M)
    assert np.array_equal(counts, want_counts)
    got = pop.core_diversity(spectrum=True)
    want = ref.summary(want_counts, M.shape[0])
    assert ref.same(got, want) is None, ref.same(got, want)
    # the device summary is the host's summary of the device counts
    host = pa.diversity_from_counts(counts, M.shape[0], spectrum=True)
    assert ref.same(got, host) is None, ref.same(got, host)
    assert ref.same(pop.core_diversity(), want) is None and "spectrum" not in pop.core_diversity()
    return got


SHAPES = [(7, 203), (100, 12000), (1000, 4099), (1024, 64), (1025, 301), (3000, 1000), (8192, 257), (65536, 48)]


@pytest.mark.parametrize("N,L", SHAPES)
def test_counts_and_summary_of_loaded_matrices(pa, N, L):
    rng = np.random.default_rng(N * 31 + L)
    M = _onehot(rng, N, L)
    pop = _core(pa, N, L)
    pop.load_matrix(M)
    got = _check(pa, pop, M)
    assert got["other_cells"] == 0 and sum(got["base_cells"]) == N * L and got["sites"] == L
    assert pop.core_diversity_timing() > 0.0
    pop.close()


@pytest.mark.parametrize("N,L", [(100, 517), (1000, 300), (2500, 130)])
def test_arbitrary_bytes_are_the_other_class(pa, N, L):
    rng = np.random.default_rng(N + L)
    M = _onehot(rng, N, L)
    hit = rng.random((N, L)) < 0.03
    M[hit] = rng.integers(0, 256, int(hit.sum()), dtype=np.uint8)     # zeros, two-bit nibbles, high bits
    M[:, 3] = 0                                                        # a site of `other` cells only
    M[:, 4] = 3
    M[:5, 5] = (0x11, 0x80, 0x0F, 0x21, 0xFF)
    pop = _core(pa, N, L)
    pop.load_matrix(M)
    got = _check(pa, pop, M)
    assert got["other_cells"] == int((~np.isin(M, (1, 2, 4, 8))).sum()) > 2 * N
    pop.close()


def test_the_spectrum_without_an_lds_histogram(pa):
    """the same results when the bins do not fit the LDS the handle may use (every row adds to the global spectrum)"""
    rng = np.random.default_rng(12)
    N, L = 1000, 2000
    M = _onehot(rng, N, L)
    pop = _core(pa, N, L)
    pop.load_matrix(M)
    pop.set_tuning("lds_limit", 2048)
    _check(pa, pop, M)
    pop.close()


def test_accessory_handles_are_refused(pa):
    acc = pa.Population(50, 64, 2, False, 0.5, 0, 0)
    for call in (acc.site_allele_counts, acc.core_diversity):
        with pytest.raises(pa.PansimError) as e:
            call()
        assert e.value.code == PS_ERR_INVALID and "ps_gene_frequencies" in str(e.value)
    acc.close()


def test_identity_against_the_distance_kernels(pa, orc):
    N, L = 100, 3001
    rng = np.random.default_rng(77)
    M = _onehot(rng, N, L)
    pop = _core(pa, N, L)
    pop.load_matrix(M)
    pairs = np.array(list(itertools.combinations(range(N), 2)), np.uint32)
    assert len(pairs) == 4950
    got = pop.core_diversity()
    (cnt,) = pop.pairwise_counts(pairs[:, 0], pairs[:, 1])
    assert int(cnt.astype(np.uint64).sum()) == 2 * got["pair_differences"]
    brute = sum(int((M[i] != M[j]).sum()) for i, j in pairs.tolist())
    assert brute == got["pair_differences"]
    d = orc.pairwise_distances(M, True, 0, pairs[:, 0], pairs[:, 1])
    mean = float(np.mean(d))
    print("mean_pairwise_distance %r, mean of the oracle's distances %r" % (got["mean_pairwise_distance"], mean))
    assert abs(got["mean_pairwise_distance"] - mean) <= 4950 * 2.0 ** -52 * mean
    pop.close()


@pytest.mark.parametrize("N,L", [(100, 3001), (1000, 1500)])
def test_on_a_running_simulation_and_across_save_and_load(pa, tmp_path, N, L):
    sim = pa.Simulation(pa.make_params(pop_size=N, core_size=L, pan_genes=500, core_genes=100, HR_rate=0.5, seed=3, n_gen=5,
                                       max_distances=100))
    sim.run(5)                                   # an odd count: a two-generation launch, then a remainder
    got = sim.core_genome.core_diversity(spectrum=True)          # (no sync: the call is ordered behind the queued sweeps)
    counts = sim.core_genome.site_allele_counts()
    M = sim.core_genome.read_matrix()
    assert np.array_equal(counts, ref.site_counts(M))
    assert ref.same(got, ref.of_matrix(M)) is None
    assert got["segregating_sites"] > 0 and got["other_cells"] == 0
    path = str(tmp_path / "run.state")
    sim.save(path)
    assert ref.same(sim.core_genome.core_diversity(spectrum=True), got) is None
    sim.close()
    back = pa.Simulation.load(path)
    assert ref.same(back.core_genome.core_diversity(spectrum=True), got) is None
    assert np.array_equal(back.core_genome.site_allele_counts(), counts)
    back.close()


def test_site_shards_add_to_the_whole(pa):
    N, L = 300, 1001
    rng = np.random.default_rng(8)
    M = _onehot(rng, N, L)
    M[rng.random((N, L)) < 0.01] = 0
    whole = _core(pa, N, L)
    whole.load_matrix(M)
    want = _check(pa, whole, M)
    whole.close()
    parts, counts = [], []
    for k in range(3):
        b, e = L * k // 3, L * (k + 1) // 3
        shard = _core(pa, N, e - b, col_offset=b, global_cols=L)
        shard.load_matrix(np.ascontiguousarray(M[:, b:e]))
        parts.append(_check(pa, shard, M[:, b:e]))
        assert parts[-1]["sites"] == e - b
        counts.append(shard.site_allele_counts())
        shard.close()
    assert ref.same(ref.add(parts), want) is None
    assert np.array_equal(np.concatenate(counts), ref.site_counts(M))


def test_multi_simulation_equals_the_unsharded_run(pa):
    kw = dict(pop_size=200, core_size=3001, pan_genes=500, core_genes=100, HR_rate=0.3, seed=5, n_gen=5, max_distances=100)
    one = pa.Simulation(pa.make_params(**kw))
    one.run(5)
    want_counts = one.core_genome.site_allele_counts()
    want = one.core_genome.core_diversity(spectrum=True)
    assert ref.same(want, ref.of_matrix(one.core_genome.read_matrix())) is None
    one.close()
    multi = pa.MultiSimulation(pa.make_params(**kw), 3, devices=[0, 0, 0])
    multi.run(5)
    assert np.array_equal(multi.site_allele_counts(), want_counts)
    got = multi.core_diversity(spectrum=True)
    assert ref.same(got, want) is None, ref.same(got, want)
    assert got["sites"] == 3001 and "spectrum" not in multi.core_diversity()
    multi.close()


def _read_core_csv(path, N, L):
    text = np.frombuffer(open(path, "rb").read(), np.uint8).reshape(N, 2 * L)[:, ::2]
    lut = np.zeros(256, np.uint8)
    for ch, v in zip(b"ACGT", (1, 2, 4, 8)):
        lut[ch] = v
    return lut[text]


@pytest.mark.parametrize("gpus", [1, 2])
def test_cli_print_core_freqs(pa, tmp_path, gpus):
    N, L = 100, 12000
    base = ["--pop_size", N, "--core_size", L, "--pan_genes", 600, "--core_genes", 200, "--n_gen", 4, "--seed", 9,
            "--max_distances", 500, "--HR_rate", 0.5, "--print_matrices", "--gpus", gpus]
    for pref, extra in (("plain", []), ("freqs", ["--print_core_freqs"])):
        r = subprocess.run([EXE, *map(str, base), *extra, "--outpref", str(tmp_path / pref)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    for suffix in (".tsv", "_freqs.txt", "_core_genome.csv", "_pangenome.csv"):
        assert filecmp.cmp(str(tmp_path / "plain") + suffix, str(tmp_path / "freqs") + suffix, shallow=False), suffix
    assert sorted(os.listdir(tmp_path)) == sorted(["plain" + s for s in (".tsv", "_freqs.txt", "_core_genome.csv", "_pangenome.csv")]
                                                  + ["freqs" + s for s in (".tsv", "_freqs.txt", "_core_genome.csv", "_pangenome.csv",
                                                                            "_core_freqs.tsv", "_core_diversity.tsv")])
    M = _read_core_csv(tmp_path / "freqs_core_genome.csv", N, L)
    counts = ref.site_counts(M)
    want = ref.summary(counts, N)
    assert want["segregating_sites"] > 0
    text = "".join("%d\t%d\t%d\t%d\n" % tuple(row) for row in counts.tolist())
    assert (tmp_path / "freqs_core_freqs.tsv").read_text() == text
    lines = ["%s\t%d" % (k, want[k]) for k in ref.INT_FIELDS]
    lines += ["base_cells_%s\t%d" % (b, v) for b, v in zip("ACGT", want["base_cells"])]
    lines += ["mean_pairwise_distance\t%s" % pa.fmt_f64(want["mean_pairwise_distance"])]
    lines += ["spectrum\t%d\t%d" % (m, c) for m, c in enumerate(want["spectrum"].tolist()) if c]
    assert (tmp_path / "freqs_core_diversity.tsv").read_text() == "\n".join(lines) + "\n"
