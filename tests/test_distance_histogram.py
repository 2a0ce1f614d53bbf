"""The joint distance histogram without a device (docs/DISTANCE_HISTOGRAM.md): ps_histogram_from_counts against the
plain-integer restatement (tests/distance_histogram_ref.py), its error paths, the no-device errors of the device entries
and the CLI's flag checks and help texts.  The device half -- the handle checks and pop_size < 2 included, which need a
handle -- is tests/test_gpu_distance_histogram.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import distance_histogram_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_NO_DEVICE = -1, -2


def random_counts(rng, P, L, G):
    """numerators of P pairs: h of either parity up to 2 L, intersections below unions up to 2 G"""
    h = rng.integers(0, 2 * L + 2, P, dtype=np.uint32)
    u = rng.integers(0, 2 * G + 1, P, dtype=np.uint32)
    i = (rng.random(P) * (u + 1)).astype(np.uint32)
    return h, np.minimum(i, u), u


def check(pa, h, i, u, L, cg, Bc, Ba, span=0):
    got = pa.histogram_from_counts(h, i, u, L, cg, core_bins=Bc, acc_bins=Ba, core_span=span)
    ref.assert_equal(got, ref.histogram(h, i, u, L, cg, Bc, Ba, span), pop_size=0)
    return got


@pytest.mark.parametrize("Bc,Ba", [(64, 64), (1, 1), (128, 128), (16384, 1), (1, 16384), (7, 13)])
@pytest.mark.parametrize("span", [0, 37, 300, 100000])
def test_from_counts_equals_the_restatement(pa, Bc, Ba, span):
    rng = np.random.default_rng(Bc * 31 + Ba + span)
    h, i, u = random_counts(rng, 3000, 300, 70)
    u[:40] = 0                      # empty unions: undefined when there are no core genes
    i[:40] = 0
    i[40:80] = 0                    # a == b when cg == 0: distance exactly 1, the last bin
    h[80:120] |= 1                  # odd numerators
    assert (h & 1).any() and not (h & 1).all()
    for cg in (0, 5):
        got = check(pa, h, i, u, 300, cg, Bc, Ba, span)
        assert got.undefined_pairs == (40 + int((u[40:] == 0).sum()) if cg == 0 else 0)
        assert got.core_clamped == (int(((h // 2) >= span).sum()) if span else 0)
        if not span:
            # nothing clamps, and the largest d has the last bin whenever there are at most as many bins as values of d
            assert got.core_span == got.core_d_max + 1 and (cg == 0 or Bc > got.core_span or got.joint[-1].any())
        if cg == 0:
            assert int(got.joint[:, -1].sum()) >= 40 - int((u[40:80] == 0).sum())


def test_core_distances_on_the_bin_edges_and_past_the_span(pa):
    """d on every integer edge ceil(k S / Bc), one below, one above; d == S - 1, S, S + 1 and far past"""
    for Bc, S in ((10, 100), (7, 100), (64, 1000), (3, 2), (5, 1), (16384, 16385), (100, 2**40)):
        edges = ref.core_edges(Bc, S)
        d = sorted(x for x in {x for e in edges for x in (e - 1, e, e + 1)} | {S - 1, S, S + 1, 2**31 - 1} if 0 <= x < 2**31)
        h = np.array([2 * x for x in d] + [2 * x + 1 for x in d], np.uint32)
        z = np.ones(h.size, np.uint32)
        got = check(pa, h, z, z, 1000, 3, Bc, 4 if Bc <= 4096 else 1, S)
        assert got.core_bin_edges() == edges
        # every pair below the span sits in the bin its d belongs to by the edges
        for x, row in ((x, min(Bc - 1, x * Bc // S)) for x in d if x < S):
            assert edges[row] <= x and (x < edges[row + 1] or row == Bc - 1)
        assert got.core_clamped == 2 * sum(1 for x in d if x >= S)


def test_accessory_quotients_on_the_bin_edges(pa):
    """every (a, b) with b up to 40 against bins that divide some b and not others: floor(a Ba / b), a == b clamped"""
    pairs = [(u - i, i, u) for cg in (0,) for u in range(0, 41) for i in range(0, u + 1)]
    i = np.array([p[1] for p in pairs], np.uint32)
    u = np.array([p[2] for p in pairs], np.uint32)
    h = np.zeros(i.size, np.uint32)
    for cg in (0, 1, 8, 2000, 2**31 - 1, 2**40):
        for Ba in (1, 2, 3, 10, 64, 16384):
            check(pa, h, i, u, 50, cg, 1, Ba, 1)


def test_the_square_sum_passes_64_bits(pa):
    h = np.array([2**32 - 1, 2**32 - 2, 2**32 - 3, 2**32 - 1, 2**32 - 1, 7], np.uint32)      # d near 2^31
    z = np.ones(h.size, np.uint32)
    got = check(pa, h, z, z, 2**31, 2, 8, 2)
    assert got.core_d_sqsum >= 2**64 and got.core_d_sqsum == sum((int(x) // 2) ** 2 for x in h)
    assert got.core_d_min == 3 and got.core_d_max == 2**31 - 1 and got.core_span == 2**31
    check(pa, h, z, z, 2**31, 2, 8, 2, span=2**33)


def test_wrapper_marginals_and_edges(pa):
    rng = np.random.default_rng(5)
    h, i, u = random_counts(rng, 500, 300, 70)
    got = pa.histogram_from_counts(h, i, u, 300, 5, core_bins=10, acc_bins=4, core_max=0.25)
    assert got.core_span == 75 and got.joint.shape == (10, 4)
    assert got.core_bin_edges() == [0, 8, 15, 23, 30, 38, 45, 53, 60, 68, 75]
    assert np.array_equal(got.core_marginal, got.joint.sum(1)) and np.array_equal(got.acc_marginal, got.joint.sum(0))
    assert pa.histogram_from_counts(h, i, u, 300, 5, core_max=1e-9).core_span == 1
    d = got.as_dict()
    assert d["pairs"] == 500 and d["joint"] is got.joint and d["core_d_sqsum"] == got.core_d_sqsum
    with pytest.raises(ValueError):
        pa.histogram_from_counts(h, i[:-1], u, 300, 5)
    with pytest.raises(ValueError):
        pa.histogram_from_counts(h, i, u, 300, 5, core_max=0.0)


def test_error_paths(pa):
    lib = pa.load()
    P, H = pa._lib.PairHistParams, pa._lib.PairHist
    h = np.array([4, 6], np.uint32)
    i = np.array([1, 2], np.uint32)
    u = np.array([3, 2], np.uint32)
    joint = np.zeros(16385, np.uint64)
    out = H()

    def call(prm, hh=h, ii=i, uu=u, n=2, o=out, j=joint):
        ptr = lambda a: None if a is None else a.ctypes.data
        return lib.ps_histogram_from_counts(ptr(hh), ptr(ii), ptr(uu), n, 10, 1, C.byref(prm) if prm is not None else None,
                                            C.byref(o) if o is not None else None, ptr(j))

    assert call(P(2, 2, 0)) == 0
    for prm in (P(0, 4, 0), P(4, 0, 0), P(0, 0, 0)):
        assert call(prm) == PS_ERR_INVALID and ">= 1" in lib.ps_last_error().decode()
    for prm in (P(16385, 1, 0), P(1, 16385, 0), P(129, 128, 0), P(2**31, 2**31, 0)):
        assert call(prm) == PS_ERR_INVALID and "16384" in lib.ps_last_error().decode()
    assert call(P(16384, 1, 0)) == 0 and call(P(128, 128, 0)) == 0
    # no pair at all: the counterpart of pop_size < 2
    assert call(P(2, 2, 0), n=0) == PS_ERR_INVALID and "pop_size >= 2" in lib.ps_last_error().decode()
    for kw in (dict(hh=None), dict(ii=None), dict(uu=None), dict(o=None), dict(j=None)):
        assert call(P(2, 2, 0), **kw) == PS_ERR_INVALID and "null" in lib.ps_last_error().decode()
    assert call(None) == PS_ERR_INVALID
    # an intersection above its union
    assert call(P(2, 2, 0), ii=np.array([1, 3], np.uint32)) == PS_ERR_INVALID and "pair 1" in lib.ps_last_error().decode()
    with pytest.raises(pa.PansimError) as e:
        pa.histogram_from_counts(h, i, u, 10, 1, core_bins=0)
    assert e.value.code == PS_ERR_INVALID
    with pytest.raises(pa.PansimError) as e:
        pa.histogram_from_counts(h, i, u, 10, 1, core_bins=4097, acc_bins=4)
    assert e.value.code == PS_ERR_INVALID and "16384" in str(e.value)


def test_the_device_entries_need_a_device(pa):
    """without a device the three device entries fail with PS_ERR_NO_DEVICE before they look at their arguments; with
    one, the same calls refuse their null arguments"""
    lib = pa.load()
    out, prm = pa._lib.PairHist(), pa._lib.PairHistParams(4, 4, 0)
    joint = np.zeros(16, np.uint64)
    want = PS_ERR_NO_DEVICE if lib.ps_device_count() <= 0 else PS_ERR_INVALID
    assert lib.ps_distance_histogram(None, None, C.byref(prm), C.byref(out), joint.ctypes.data) == want
    assert lib.ps_sim_distance_histogram(None, C.byref(prm), C.byref(out), joint.ctypes.data) == want
    assert lib.ps_multi_distance_histogram(None, C.byref(prm), C.byref(out), joint.ctypes.data) == want
    if want == PS_ERR_NO_DEVICE:
        assert "no HIP device" in lib.ps_last_error().decode()
        # ... and before the parameters: bins that no call accepts
        bad = pa._lib.PairHistParams(0, 0, 0)
        assert lib.ps_distance_histogram(None, None, C.byref(bad), C.byref(out), joint.ctypes.data) == PS_ERR_NO_DEVICE
    # the timing getter touches no device before it has something to report
    assert lib.ps_distance_histogram_timing(None, None, None) == PS_ERR_INVALID


def cli(*args):
    return subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value,text", [
    ("64", "<core>,<accessory>"), ("64,", "<core>,<accessory>"), ("a,b", "<core>,<accessory>"), ("8,8,8", "<core>,<accessory>"),
    ("-4,4", "<core>,<accessory>"), ("4.5,4", "<core>,<accessory>"), ("0,4", "at least 1"), ("4,0", "at least 1"),
    ("16385,1", "at most 16384"), ("129,128", "at most 16384"), ("4294967297,1", "at most 16384")])
def test_cli_rejects_bad_bins(pa, value, text):
    """the optional flags are checked before any device work, whether or not --print_dist_hist is given"""
    for extra in ((), ("--print_dist_hist",)):
        r = cli("--dist_hist_bins=" + value, "--pan_genes", 3000, *extra)
        assert r.returncode == 101 and r.stdout == "" and "--dist_hist_bins" in r.stderr and text in r.stderr, (r.returncode, r.stderr)


@pytest.mark.parametrize("value,text", [("0", "must be > 0.0"), ("-0.5", "must be > 0.0"), ("nan", "must be > 0.0"),
                                        ("inf", "must be > 0.0"), ("x", "invalid float literal")])
def test_cli_rejects_a_bad_core_max(pa, value, text):
    r = cli("--print_dist_hist", "--dist_hist_core_max=" + value, "--pan_genes", 3000)
    assert r.returncode == 101 and r.stdout == "" and "--dist_hist_core_max" in r.stderr and text in r.stderr, (r.returncode, r.stderr)


def test_cli_flag_shapes(pa):
    r = cli("--print_dist_hist=1")
    assert r.returncode == 2 and "takes no value" in r.stderr
    r = cli("--dist_hist_bins")
    assert r.returncode == 2 and "requires a value" in r.stderr


def test_help_extensions_lists_the_histogram_flags(pa):
    r = cli("--help-extensions")
    assert r.returncode == 0
    assert "--print_dist_hist\n" in r.stdout and "_dist_hist.tsv" in r.stdout and "_dist_hist_summary.tsv" in r.stdout
    assert "--dist_hist_bins <dist_hist_bins>\n" in r.stdout and "[default: 64,64]" in r.stdout
    assert "--dist_hist_core_max <dist_hist_core_max>\n" in r.stdout
    r = cli("--help")
    assert r.returncode == 0 and "dist_hist" not in r.stdout
