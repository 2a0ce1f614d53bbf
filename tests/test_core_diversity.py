"""Core allele counts and diversity without a device (docs/CORE_DIVERSITY.md): ps_diversity_from_counts against the numpy
restatement (tests/core_diversity_ref.py), shard addition, the no-device errors of the device entries, the wrappers'
argument checks and the CLI's help texts.  The device half is tests/test_gpu_core_diversity.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import core_diversity_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_NO_DEVICE = -1, -2


def random_table(rng, N, sites, other=True):
    """(sites, 4) counts of N cells split at random over A, C, G, T (and `other`), with skewed sites among them"""
    p = rng.dirichlet([0.3] * (5 if other else 4), sites)
    t = np.stack([rng.multinomial(N, q) for q in p])
    return np.ascontiguousarray(t[:, :4], np.uint32)


@pytest.mark.parametrize("N", [1, 2, 7, 1000, 65536])
def test_from_counts_equals_the_restatement(pa, N):
    rng = np.random.default_rng(N)
    t = random_table(rng, N, 300)
    t[5] = 0                          # a site of `other` cells only
    t[6] = [N, 0, 0, 0]               # monomorphic sites
    t[7] = [0, 0, 0, N]
    assert (t.sum(1) < N).any() or N == 1
    got = pa.diversity_from_counts(t, N, spectrum=True)
    want = ref.summary(t, N)
    assert ref.same(got, want) is None, ref.same(got, want)
    assert got["spectrum"].dtype == np.uint64 and got["spectrum"].shape == (N + 1,) and int(got["spectrum"].sum()) == 300
    assert "spectrum" not in pa.diversity_from_counts(t, N)


@pytest.mark.parametrize("N", [1, 2, 7, 1000, 65536])
def test_monomorphic_and_all_other_tables(pa, N):
    mono = np.zeros((40, 4), np.uint32)
    mono[:, 2] = N
    got = pa.diversity_from_counts(mono, N, spectrum=True)
    assert ref.same(got, ref.summary(mono, N)) is None
    assert got["pair_differences"] == 0 and got["segregating_sites"] == 0 and got["other_cells"] == 0
    assert got["mean_pairwise_distance"] == 0.0 and got["spectrum"][0] == 40 and got["base_cells"] == [0, 0, 40 * N, 0]
    none = np.zeros((40, 4), np.uint32)
    got = pa.diversity_from_counts(none, N, spectrum=True)
    assert ref.same(got, ref.summary(none, N)) is None
    assert got["other_cells"] == 40 * N and got["segregating_sites"] == 0 and got["pair_differences"] == 0


def test_a_table_of_no_sites(pa):
    got = pa.diversity_from_counts(np.zeros((0, 4), np.uint32), 9, spectrum=True)
    assert ref.same(got, ref.summary(np.zeros((0, 4), np.uint32), 9)) is None
    assert got["sites"] == 0 and got["mean_pairwise_distance"] == 0.0 and not got["spectrum"].any()


@pytest.mark.parametrize("N", [2, 7, 1000, 65536])
def test_column_parts_add_to_the_whole(pa, N):
    rng = np.random.default_rng(100 + N)
    t = random_table(rng, N, 257)
    whole = pa.diversity_from_counts(t, N, spectrum=True)
    parts = [pa.diversity_from_counts(t[a:b], N, spectrum=True) for a, b in ((0, 85), (85, 86), (86, 257))]
    assert ref.same(ref.add(parts), whole) is None, ref.same(ref.add(parts), whole)
    assert ref.same(whole, ref.summary(t, N)) is None


def test_wrapper_shape_and_argument_errors(pa):
    with pytest.raises(ValueError):
        pa.diversity_from_counts(np.zeros((5, 3), np.uint32), 10)
    with pytest.raises(ValueError):
        pa.diversity_from_counts(np.zeros(8, np.uint32), 10)
    with pytest.raises(ValueError):
        pa.diversity_from_counts(np.zeros((5, 4), np.uint32), 0)
    with pytest.raises(pa.PansimError) as e:       # a site that holds more cells than the population
        pa.diversity_from_counts(np.array([[1, 1, 1, 1], [3, 3, 3, 2]], np.uint32), 10)
    assert e.value.code == PS_ERR_INVALID and "site 1" in str(e.value)
    with pytest.raises(pa.PansimError) as e:
        pa.diversity_from_counts(np.zeros((1, 4), np.uint32), 1 << 32)
    assert e.value.code == PS_ERR_INVALID
    lib = pa.load()
    out = pa._lib.CoreDiversity()
    assert lib.ps_diversity_from_counts(None, 3, 10, C.byref(out), None) == PS_ERR_INVALID
    assert lib.ps_diversity_from_counts(None, 0, 10, None, None) == PS_ERR_INVALID
    assert lib.ps_diversity_from_counts(None, 0, 10, C.byref(out), None) == 0 and out.pop_size == 10 and out.sites == 0


def test_the_device_entries_need_a_device(pa):
    """without a device every device entry fails with PS_ERR_NO_DEVICE before it looks at its arguments, as every compute
    call; with one, the same calls refuse their null arguments"""
    lib = pa.load()
    out = pa._lib.CoreDiversity()
    buf = np.zeros(4, np.uint32)
    want = PS_ERR_NO_DEVICE if lib.ps_device_count() <= 0 else PS_ERR_INVALID
    assert lib.ps_site_allele_counts(None, buf.ctypes.data) == want
    assert lib.ps_core_diversity(None, C.byref(out), None) == want
    assert lib.ps_multi_site_allele_counts(None, buf.ctypes.data) == want
    assert lib.ps_multi_core_diversity(None, C.byref(out), None) == want
    if want == PS_ERR_NO_DEVICE:
        assert "no HIP device" in lib.ps_last_error().decode()
        with pytest.raises(pa.PansimError) as e:
            pa.Population(10, 20, 4, True, 0.0, 0, 0).site_allele_counts()
        assert e.value.code == PS_ERR_NO_DEVICE
    # the timing getter touches no device before it has something to report
    assert lib.ps_core_diversity_timing(None, None) == PS_ERR_INVALID


def test_help_extensions_lists_print_core_freqs(pa):
    r = subprocess.run([EXE, "--help-extensions"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--print_core_freqs\n" in r.stdout and "_core_diversity.tsv" in r.stdout
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "print_core_freqs" not in r.stdout
    assert r.stdout[r.stdout.index("USAGE:"):] == open(os.path.join(ROOT, "tests", "golden", "help_usage.txt")).read()
