"""Linkage disequilibrium between loci without a device (docs/LINKAGE_DISEQUILIBRIUM.md): the host-only ps_ld_select_loci and
ps_ld_from_counts against the plain restatement (tests/ld_ref.py) on random tables, the hand cases of the document, the
rounding traps of the f64 estimate of q at N = 65536, every PS_ERR_INVALID limit, the no-device error of the device entries and
the CLI's flag checks.  The device half is tests/test_gpu_locus_ld.py.  Every comparison is an equality of integers; the one
double is compared bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ld_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_NO_DEVICE, PS_ERR_STATE = -1, -2, -6
NEW_SYMBOLS = ("ps_locus_ld", "ps_sim_locus_ld", "ps_multi_locus_ld", "ps_ld_select_loci", "ps_ld_from_counts", "ps_locus_ld_timing")


def _bits(s):
    return np.array([int(c) for c in s], np.uint8)


def _from_rows(pa, rows, index=None, r2_bins=64, lag_bins=1):
    """ps_ld_from_counts on explicit indicator rows -> (result, reference)"""
    X = np.array([_bits(r) if isinstance(r, str) else r for r in rows], np.uint8)
    M, N = X.shape
    index = list(range(M)) if index is None else index
    count = X.sum(1, dtype=np.int64)
    Xi = X.astype(np.int64)
    n11 = [int(Xi[a] @ Xi[b]) for a in range(M) for b in range(a + 1, M)]
    got = pa.ld_from_counts(index, count, n11, N, r2_bins, lag_bins)
    want = ref.from_counts(index, count, lambda a, b: int(Xi[a] @ Xi[b]), N, r2_bins, lag_bins)
    want["locus_index"], want["locus_count"] = np.array(index, np.uint32), count.astype(np.uint32)
    return got, want


@pytest.mark.parametrize("C_,max_loci", [(10, 50), (50, 50), (51, 50), (200, 7), (1000, 999), (1, 1), (0, 5)])
def test_select_loci_equals_the_restatement(pa, C_, max_loci):
    """C below, at and above max_loci; the min_minor edges of both tails; every column monomorphic when C_ == 0"""
    rng = np.random.default_rng(100 + C_)
    N, L = 37, 1500
    for min_minor in (1, 2, 5, 18):
        ones = rng.choice([0, N, min_minor - 1, N - min_minor + 1], L).astype(np.uint32)        # (none a candidate)
        cand = rng.choice(L, C_, replace=False)
        ones[cand] = rng.choice([min_minor, N - min_minor, N // 2], C_)
        want, C_want = ref.select(ones, N, min_minor, max_loci)
        got, C_got = pa.ld_select_loci(ones, N, min_minor, max_loci)
        assert C_got == C_want == C_ and got.tolist() == want
        assert len(want) == min(C_, max_loci)


def test_select_loci_of_a_monomorphic_table(pa):
    got, C_ = pa.ld_select_loci(np.array([0, 9, 9, 0], np.uint32), 9, 1, 4)
    assert got.size == 0 and C_ == 0
    got, C_ = pa.ld_select_loci(np.zeros(0, np.uint32), 9, 1, 4)
    assert got.size == 0 and C_ == 0


@pytest.mark.parametrize("N,M,r2_bins,lag_bins", [(2, 5, 1, 1), (9, 30, 64, 1), (64, 40, 7, 5), (301, 25, 512, 32), (1000, 12, 16384, 1)])
def test_from_counts_equals_the_restatement(pa, N, M, r2_bins, lag_bins):
    rng = np.random.default_rng(N + M)
    base = rng.random((4, N)) < 0.5
    X = np.array([base[rng.integers(4)] ^ (rng.random(N) < rng.choice([0.0, 0.02, 0.3])) for _ in range(M)], np.uint8)
    X[rng.integers(M)] = 0                      # monomorphic rows of both kinds
    X[rng.integers(M)] = 1
    index = np.sort(rng.choice(1 << 20, M, replace=False)).tolist()
    got, want = _from_rows(pa, X, index, r2_bins, lag_bins)
    ref.assert_equal(got, want)
    assert got.pairs == got.defined_pairs + got.undefined_pairs == M * (M - 1) // 2
    assert got.undefined_pairs > 0


def test_hand_cases(pa):
    got, want = _from_rows(pa, ["1100", "1010"])
    ref.assert_equal(got, want)
    assert got.sum_q == 0 and got.four_gamete_pairs == 1 and got.positive_pairs == got.negative_pairs == 0
    got, want = _from_rows(pa, ["1100", "1110"])
    ref.assert_equal(got, want)
    assert got.sum_q == 21845 and got.four_gamete_pairs == 0 and got.positive_pairs == 1
    assert got.hist[0, (21845 * 64) >> 16] == 1
    got, want = _from_rows(pa, ["1100", "1100"])
    ref.assert_equal(got, want)
    assert got.sum_q == 65536 and got.complete_pairs == 1 and got.positive_pairs == 1 and got.hist[0, 63] == 1
    assert got.mean_r2 == 1.0
    got, want = _from_rows(pa, ["1100", "0011"])
    ref.assert_equal(got, want)
    assert got.sum_q == 65536 and got.complete_pairs == 1 and got.negative_pairs == 1
    # fewer than two loci: no pairs, everything zero
    for rows in ([], ["1100"]):
        got = pa.ld_from_counts(list(range(len(rows))), [2] * len(rows), [], 4)
        assert got.loci == len(rows) and got.pairs == got.defined_pairs == got.undefined_pairs == got.sum_q == 0 and got.mean_r2 == 0.0
        assert not got.hist.any()


def test_lag_bins_are_the_floor_of_log2_of_the_column_distance(pa):
    index = [0, 1, 3, 7, 1000, 1 << 31, (1 << 32) - 1]
    rows = ["1100", "1010", "1001", "0110", "0101", "0011", "1110"]
    for lag_bins in (1, 5, 32):
        got, want = _from_rows(pa, rows, index, 8, lag_bins)
        ref.assert_equal(got, want)
    # (2^31 from column 0 and 2^32 - 1 from the five columns below 2^31 are distances of 2^31 and more; one distance is 1)
    assert got.hist[31].sum() == 6 and got.hist[0].sum() == 1


def _near_integers(limit):
    """(ca, cb, n11, side) at N = 65536 with 2^16 D^2 / den within 2^-20 of an integer: cb = N / 2 makes the quotient
    2^16 t^2 / m with t = 2 n11 - ca and m = ca (N - ca), which a vectorised search can walk; every hit is checked again in
    Python integers"""
    N, cb = 65536, 32768
    below, above = [], []
    for ca in range(16001, 32768, 3):
        m = ca * (N - ca)
        n11 = np.arange(max(0, ca + cb - N), min(ca, cb) + 1, dtype=np.int64)
        t = 2 * n11 - ca
        rem = ((t * t).astype(np.uint64) << np.uint64(16)) % np.uint64(m)
        eps = np.uint64(m >> 20)
        for k in np.nonzero((rem > 0) & (rem < eps))[0]:
            above.append((ca, cb, int(n11[k])))
        for k in np.nonzero((rem > 0) & (np.uint64(m) - rem < eps))[0]:
            below.append((ca, cb, int(n11[k])))
        if len(below) >= limit and len(above) >= limit:
            break
    return below, above


def test_rounding_traps_of_the_f64_estimate(pa):
    """quotients just below and just above an integer at N = 65536, and the corners c = 65535"""
    N = 65536
    below, above = _near_integers(150)
    assert len(below) >= 100 and len(above) >= 100
    scale = 1 << 20
    for side, cases in (("below", below), ("above", above)):
        for ca, cb, n in cases:
            D, q = ref.pair_q(N, ca, cb, n)
            den = ca * (N - ca) * cb * (N - cb)
            rem = (D * D << 16) - q * den
            assert 0 < (den - rem if side == "below" else rem) * scale < den          # (within 2^-20 of an integer, not on it)
            got = pa.ld_from_counts([0, 1], [ca, cb], [n], N)
            assert got.sum_q == q, (ca, cb, n, got.sum_q, q)
    for n in (65535, 65534):
        got = pa.ld_from_counts([0, 1], [65535, 65535], [n], N)
        D, q = ref.pair_q(N, 65535, 65535, n)
        assert got.sum_q == q and got.complete_pairs == (q == 65536) and got.positive_pairs == (D > 0) and got.negative_pairs == (D < 0)
    # two loci of 65535 ones share at least 65534 individuals: n11 = 0 is no table of counts (its "q" would be 2^16 65535^2, and
    # D^2 all but fills 64 bits) and is refused
    idx, cnt, n0 = np.array([0, 1], np.uint32), np.array([65535, 65535], np.uint32), np.array([0], np.uint32)
    o, prm, hist, lag = pa._lib.Ld(), pa._lib.LdParams(64, 1, 1, 1), np.zeros(64, np.uint64), np.zeros(1, np.uint64)
    rc = pa.load().ps_ld_from_counts(idx.ctypes.data, cnt.ctypes.data, n0.ctypes.data, 2, N, C.byref(prm), C.byref(o), hist.ctypes.data,
                                     lag.ctypes.data)
    assert rc == PS_ERR_INVALID and "does not fit" in pa.load().ps_last_error().decode()
    # n11 = 0 beside a locus of 65535 ones: the other locus is the one individual it lacks
    got = pa.ld_from_counts([0, 1], [65535, 1], [0], N)
    assert got.sum_q == 65536 and got.negative_pairs == 1 and got.four_gamete_pairs == 0
    # exact integers over every n11 of a small table, where an estimate just below the integer would lose one
    for ca, cb in ((32768, 32768), (16384, 49152), (1, 65535), (4096, 61440)):
        for n in sorted({max(0, ca + cb - N), min(ca, cb), (max(0, ca + cb - N) + min(ca, cb)) // 2}):
            got = pa.ld_from_counts([0, 1], [ca, cb], [n], N)
            assert got.sum_q == ref.pair_q(N, ca, cb, n)[1]


def _call(pa, fn, *args):
    rc = fn(*args)
    return rc, pa.load().ps_last_error().decode()


def test_invalid_arguments(pa):
    lib = pa.load()
    o = pa._lib.Ld()
    hist, lag = np.zeros(16384, np.uint64), np.zeros(32, np.uint64)
    idx, cnt, n11 = np.array([0, 3, 9], np.uint32), np.array([2, 2, 2], np.uint32), np.array([1, 1, 1], np.uint32)

    def from_counts(prm, idx=idx, cnt=cnt, n11=n11, N=4):
        return _call(pa, lib.ps_ld_from_counts, idx.ctypes.data, cnt.ctypes.data, n11.ctypes.data, idx.size, N, C.byref(prm), C.byref(o),
                     hist.ctypes.data, lag.ctypes.data)

    assert from_counts(pa._lib.LdParams(64, 1, 1, 1))[0] == 0
    for r2, lg, word in ((0, 1, "r2_bins"), (4, 0, "lag_bins"), (4, 33, "lag_bins"), (16385, 1, "exceeds"), (1024, 32, "exceeds")):
        rc, msg = from_counts(pa._lib.LdParams(r2, lg, 1, 1))
        assert rc == PS_ERR_INVALID and word in msg, (r2, lg, msg)
    prm = pa._lib.LdParams(8, 2, 1, 1)
    rc, msg = from_counts(prm, idx=np.array([0, 3, 3], np.uint32))
    assert rc == PS_ERR_INVALID and "strictly ascending" in msg
    rc, msg = from_counts(prm, idx=np.array([5, 3, 9], np.uint32))
    assert rc == PS_ERR_INVALID and "strictly ascending" in msg
    rc, msg = from_counts(prm, cnt=np.array([2, 5, 2], np.uint32))
    assert rc == PS_ERR_INVALID and "ones among" in msg
    rc, msg = from_counts(prm, n11=np.array([3, 1, 1], np.uint32))
    assert rc == PS_ERR_INVALID and "does not fit" in msg
    rc, msg = from_counts(prm, cnt=np.array([3, 3, 2], np.uint32), n11=np.array([1, 1, 1], np.uint32))      # 3 + 3 - 1 > 4
    assert rc == PS_ERR_INVALID and "does not fit" in msg
    rc, msg = from_counts(prm, N=65537)
    assert rc == PS_ERR_INVALID and "pop_size" in msg
    ones, index, n, c = np.array([1, 2, 3], np.uint32), np.zeros(8, np.uint32), C.c_uint64(), C.c_uint64()
    for N, mm, ml, word in ((4, 0, 4, "min_minor"), (4, 1, 0, "max_loci"), (4, 1, 65537, "max_loci"), (65537, 1, 4, "pop_size"), (2, 1, 4, "ones among")):
        rc, msg = _call(pa, lib.ps_ld_select_loci, ones.ctypes.data, 3, N, mm, ml, index.ctypes.data, C.byref(n), C.byref(c))
        assert rc == PS_ERR_INVALID and word in msg, (N, mm, ml, msg)
    assert lib.ps_locus_ld_timing(None, None, None, None, None) == PS_ERR_INVALID


def test_the_device_entries_need_a_device(pa):
    """without a device the device entries fail with PS_ERR_NO_DEVICE before they look at their arguments; with one, the same
    calls refuse their null arguments"""
    lib = pa.load()
    o, prm = pa._lib.Ld(), pa._lib.LdParams(64, 1, 1, 4096)
    a, b = np.zeros(4096, np.uint32), np.zeros(64, np.uint64)
    want = PS_ERR_NO_DEVICE if lib.ps_device_count() <= 0 else PS_ERR_INVALID
    tail = (C.byref(prm), None, 0, C.byref(o), a.ctypes.data, a.ctypes.data, b.ctypes.data, b.ctypes.data)
    assert lib.ps_locus_ld(None, *tail) == want
    assert lib.ps_sim_locus_ld(None, 0, *tail) == want
    assert lib.ps_multi_locus_ld(None, 1, *tail) == want
    if want == PS_ERR_NO_DEVICE:
        assert "no HIP device" in lib.ps_last_error().decode()
        bad = pa._lib.LdParams(0, 99, 0, 0)                        # ... and before the parameters
        assert lib.ps_locus_ld(None, C.byref(bad), None, 0, C.byref(o), None, None, None, None) == PS_ERR_NO_DEVICE
        assert lib.ps_sim_locus_ld(None, 7, C.byref(bad), None, 0, C.byref(o), None, None, None, None) == PS_ERR_NO_DEVICE


def test_abi_header_and_bindings_agree(pa):
    lib = pa.load()
    hdr = open(os.path.join(ROOT, "include", "pansim_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in pa._lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
    assert lib.ps_abi_version() == 3
    for struct, cls in (("ps_ld_params", pa._lib.LdParams), ("ps_ld_t", pa._lib.Ld)):
        fields = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1)
        assert re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields)) == [n for n, _ in cls._fields_]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert "fn %s(" % name in integration, name
    assert os.path.exists(os.path.join(ROOT, "docs", "LINKAGE_DISEQUILIBRIUM.md"))


def cli(*args):
    return subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=60)


def test_cli_rejects_bad_values(pa):
    """checked before any device work, whether or not --print_ld is given"""
    for extra in ((), ("--print_ld",)):
        r = cli("--ld_metric", "bogus", "--pan_genes", 3000, *extra)
        assert r.returncode == 101 and r.stdout == "" and "--ld_metric" in r.stderr and "core or acc" in r.stderr, (r.returncode, r.stderr)
        for value in ("0,4", "4,0", "4", "4,4,4", "x,4", "-1,4", "2.5,4", "4,33", "1024,32", "4, 4"):
            r = cli("--pan_genes", 3000, "--ld_bins=" + value, *extra)
            assert r.returncode == 101 and r.stdout == "" and "--ld_bins" in r.stderr, (value, r.returncode, r.stderr)
        for value in ("0", "-1", "x", "2.5", "65537"):
            r = cli("--pan_genes", 3000, "--ld_max_loci=" + value, *extra)
            assert r.returncode == 101 and r.stdout == "" and "--ld_max_loci" in r.stderr, (value, r.returncode, r.stderr)
        for value in ("0", "-1", "x", "4294967296"):
            r = cli("--pan_genes", 3000, "--ld_min_minor=" + value, *extra)
            assert r.returncode == 101 and r.stdout == "" and "--ld_min_minor" in r.stderr, (value, r.returncode, r.stderr)


def test_help_extensions_lists_the_ld_flags(pa):
    r = cli("--help-extensions")
    assert r.returncode == 0
    for flag in ("--print_ld", "--ld_metric", "--ld_max_loci", "--ld_min_minor", "--ld_bins"):
        assert flag in r.stdout, flag
    assert "--print_ld" not in cli("--help").stdout
