"""The recorded genealogy without a device (docs/GENEALOGY.md): the host-only read-outs of a comb (pair, pairs, clusters,
Newick) and ps_clock_from_counts against the plain restatement (tests/genealogy_ref.py) on hand-made combs with ties
(multifurcations), entries beyond the record and N = 2; every PS_ERR_INVALID limit with its message, the no-device errors of
the device entries, the CLI's flag checks and help texts.  The device half is tests/test_gpu_genealogy.py.  Every comparison is
an equality of integers or of text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import genealogy_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_NO_DEVICE, PS_ERR_STATE = -1, -2, -6
B = ref.BEYOND
NEW_SYMBOLS = ("ps_sim_record_ancestry", "ps_multi_record_ancestry", "ps_sim_genealogy", "ps_multi_genealogy", "ps_genealogy_pair",
               "ps_genealogy_pairs", "ps_genealogy_clusters", "ps_genealogy_newick", "ps_sim_clock_histogram", "ps_multi_clock_histogram",
               "ps_clock_from_counts", "ps_clock_histogram_timing")

# (order, coal, depth): ties, entries beyond the record, N = 2 and N = 1
COMBS = {
    "ties": ([2, 0, 1, 3, 4], [1, 3, 3, B], 5),
    "pair": ([1, 0], [2], 2),
    "pair_beyond": ([0, 1], [B], 3),
    "one": ([0], [], 4),
    "caterpillar": ([5, 4, 3, 2, 1, 0], [1, 2, 3, 4, 5], 5),
    "star": ([0, 3, 1, 2], [2, 2, 2], 2),
    "forest": ([3, 1, 0, 2, 5, 4, 6], [1, B, 2, 2, B, 1], 2),
    "nested_ties": ([0, 1, 2, 3, 4, 5, 6, 7], [1, 2, 1, 4, 1, 2, 2], 6),
}
NEWICK = {
    "ties": "((2:1,0:1):2,1:3,3:3);\n4;\n",
    "pair": "(1:2,0:2);\n",
    "pair_beyond": "0;\n1;\n",
    "one": "0;\n",
    "caterpillar": "(((((5:1,4:1):1,3:2):1,2:3):1,1:4):1,0:5);\n",
    "star": "(0:2,3:2,1:2,2:2);\n",
    "forest": "(3:1,1:1);\n(0:2,2:2,5:2);\n(4:1,6:1);\n",
    "nested_ties": "(((0:1,1:1):1,(2:1,3:1):1):2,((4:1,5:1):1,6:2,7:2):2);\n",
}


def comb(name):
    order, coal, depth = COMBS[name]
    return np.array(order, np.uint32), np.array(coal, np.uint32), depth


def random_comb(rng, N, depth, p_beyond=0.1):
    coal = rng.integers(1, depth + 1, N - 1).astype(np.uint32)
    coal[rng.random(N - 1) < p_beyond] = B
    return rng.permutation(N).astype(np.uint32), coal, depth


@pytest.mark.parametrize("name", sorted(COMBS))
def test_hand_made_combs_equal_the_restatement(pa, name):
    order, coal, depth = comb(name)
    N = order.size
    T = ref.matrix_of_comb(order, coal)
    r1, r2 = np.divmod(np.arange(N * N, dtype=np.uint32), np.uint32(N))
    assert np.array_equal(pa.genealogy_pairs(order, coal, r1, r2).reshape(N, N), T)
    for i in range(N):
        for j in range(N):
            assert pa.genealogy_pair(order, coal, i, j) == T[i, j]
    for t in range(depth + 1):
        labels, out = pa.genealogy_clusters(order, coal, depth, t)
        want_labels, want = ref.clusters(T, t)
        assert np.array_equal(labels, want_labels) and out == want, (t, labels, want_labels, out, want)
    text = pa.genealogy_newick(order, coal)
    assert text == NEWICK[name] == ref.newick(order, T)


@pytest.mark.parametrize("N,depth", [(2, 1), (3, 2), (17, 3), (64, 4), (65, 200), (300, 6)])
def test_random_combs_equal_the_restatement(pa, N, depth):
    rng = np.random.default_rng(N * 1000 + depth)
    order, coal, depth = random_comb(rng, N, depth)
    T = ref.matrix_of_comb(order, coal)
    r1, r2 = ref.all_pairs(N)
    assert np.array_equal(pa.genealogy_pairs(order, coal, r1, r2), T[r1, r2])
    assert np.array_equal(pa.genealogy_pairs(order, coal, r2, r1), T[r1, r2])
    for t in sorted({0, 1, depth // 2, depth}):
        labels, out = pa.genealogy_clusters(order, coal, depth, t)
        want_labels, want = ref.clusters(T, t)
        assert np.array_equal(labels, want_labels) and out == want
    if N <= 65:
        assert pa.genealogy_newick(order, coal) == ref.newick(order, T)


def test_a_deep_caterpillar_needs_no_deep_recursion(pa):
    N = 200000
    order, coal = np.arange(N, dtype=np.uint32), np.arange(1, N, dtype=np.uint32)
    text = pa.genealogy_newick(order, coal)
    assert text.startswith("(" * (N - 1) + "0:1,1:1):1,2:2):1,") and text.endswith(",%d:%d);\n" % (N - 1, N - 1))


def test_host_entries_reject_bad_arguments(pa):
    lib = pa.load()
    order, coal, depth = comb("ties")
    t, lab, out, need = C.c_uint32(), np.zeros(5, np.uint32), pa._lib.GenClusters(), C.c_uint64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def err():
        return lib.ps_last_error().decode()

    assert lib.ps_genealogy_pair(p(order), p(coal), 5, 5, 0, C.byref(t)) == PS_ERR_INVALID and "index 5 is not below pop_size 5" in err()
    assert lib.ps_genealogy_pair(None, p(coal), 5, 0, 1, C.byref(t)) == PS_ERR_INVALID and "null" in err()
    assert lib.ps_genealogy_pair(p(order), p(coal), 0, 0, 0, C.byref(t)) == PS_ERR_INVALID and "1 <= pop_size < 2^32" in err()
    twice = np.array([0, 1, 1, 3, 4], np.uint32)
    assert lib.ps_genealogy_pair(p(twice), p(coal), 5, 0, 1, C.byref(t)) == PS_ERR_INVALID and "permutation" in err()
    high = np.array([0, 1, 9, 3, 4], np.uint32)
    assert lib.ps_genealogy_newick(p(high), p(coal), 5, None, 0, C.byref(need)) == PS_ERR_INVALID and "order[2] = 9 is not below pop_size 5" in err()
    # a look-back above the depth
    assert lib.ps_genealogy_clusters(p(order), p(coal), 5, depth, depth + 1, p(lab), C.byref(out)) == PS_ERR_INVALID
    assert "0 .. depth = 5 generations, not 6" in err()
    with pytest.raises(pa.PansimError) as e:
        pa.genealogy_clusters(order, coal, 2, 3)
    assert e.value.code == PS_ERR_INVALID
    # the Newick buffer: the size alone, a buffer that is too small, a time of 0
    assert lib.ps_genealogy_newick(p(order), p(coal), 5, None, 0, C.byref(need)) == 0 and need.value == len(NEWICK["ties"]) + 1
    buf = C.create_string_buffer(8)
    assert lib.ps_genealogy_newick(p(order), p(coal), 5, buf, 8, C.byref(need)) == PS_ERR_INVALID and "needs 27 bytes" in err()
    zero = np.array([1, 0, 3, B], np.uint32)
    assert lib.ps_genealogy_newick(p(order), p(zero), 5, None, 0, C.byref(need)) == PS_ERR_INVALID and "coal[1] = 0" in err()


def clock_case(rng, P, depth, L, G, cg):
    t = rng.integers(1, depth + 1, P).astype(np.uint32)
    t[rng.random(P) < 0.2] = B
    h = rng.integers(0, 2 * L + 2, P, dtype=np.uint32)
    u = rng.integers(0, G + 1, P, dtype=np.uint32)
    i = np.minimum((rng.random(P) * (u + 1)).astype(np.uint32), u)
    return t, h, i, u


@pytest.mark.parametrize("P,depth,L,G,cg,Bt,Bx,time_span,core_span", [
    (1, 1, 10, 4, 0, 1, 1, 0, 0), (500, 7, 40, 6, 0, 4, 8, 0, 0), (500, 12, 300, 50, 3, 32, 64, 0, 0), (400, 100, 300, 50, 0, 7, 5, 30, 100),
    (300, 9, 50, 10, 1, 1023, 16, 0, 0), (300, 9, 50, 10, 1, 3, 4096, 5, 17)])
def test_clock_from_counts_equals_the_restatement(pa, P, depth, L, G, cg, Bt, Bx, time_span, core_span):
    """both metrics; cg = 0 with small G: pairs with b = 0; a fifth of the pairs beyond the record; a span below the depth clamps"""
    rng = np.random.default_rng(P + depth + Bt)
    t, h, i, u = clock_case(rng, P, depth, L, G, cg)
    for name, metric in (("core", ref.CORE), ("acc", ref.ACC)):
        got = pa.clock_from_counts(t, h, i, u, depth, L, cg, metric=name, time_bins=Bt, dist_bins=Bx, time_span=time_span, core_span=core_span or None)
        ref.assert_clock(got, ref.clock_from_counts(metric, t, h, i, u, depth, L, cg, Bt, Bx, time_span, core_span))
        assert got.pop_size == 0 and int(got.joint.sum()) + got.undefined_pairs == P
    # the numerators of the other metric may be missing
    got = pa.clock_from_counts(t, h, None, None, depth, L, cg, time_bins=Bt, dist_bins=Bx, time_span=time_span, core_span=core_span or None)
    ref.assert_clock(got, ref.clock_from_counts(ref.CORE, t, h, i, u, depth, L, cg, Bt, Bx, time_span, core_span))
    got = pa.clock_from_counts(t, None, i, u, depth, L, cg, metric="acc", time_bins=Bt, dist_bins=Bx, time_span=time_span)
    ref.assert_clock(got, ref.clock_from_counts(ref.ACC, t, h, i, u, depth, L, cg, Bt, Bx, time_span, 0))


def test_clock_bin_edges_undefined_pairs_and_the_beyond_row(pa):
    """times on both sides of every edge of the time axis, distances on both sides of an edge of either distance axis, a pair with
    b = 0 and pairs beyond the record, written out by hand"""
    # depth 8, 4 time bins: t = 1, 2 | 3, 4 | 5, 6 | 7, 8; beyond: row 4
    t = np.array([1, 2, 3, 4, 5, 6, 7, 8, B, B], np.uint32)
    # S = 10, 5 bins: d = 0, 1 | 2, 3 | ... ; h = 2 d + 1 halves to d
    h = np.array([0, 3, 4, 7, 8, 11, 12, 19, 3, 5], np.uint32)
    got = pa.clock_from_counts(t, h, None, None, 8, 100, 0, time_bins=4, dist_bins=5, core_span=10)
    want = np.zeros((5, 5), np.uint64)
    for row, col in ((0, 0), (0, 0), (1, 1), (1, 1), (2, 2), (2, 2), (3, 3), (3, 4), (4, 0), (4, 1)):
        want[row, col] += 1
    assert np.array_equal(got.joint, want)
    assert got.per_time.tolist() == [[2, 1, 200], [2, 5, 200], [2, 9, 200], [2, 15, 200], [2, 3, 200]]
    assert (got.beyond_pairs, got.binned_pairs, got.num_sum, got.den_sum, got.core_clamped) == (2, 10, 33, 1000, 0)
    # a span of 3 generations: t = 1 | 2 | 3 | 4 and later (clamped into the last bin); d >= 4 clamped
    got = pa.clock_from_counts(t, h, None, None, 8, 100, 0, time_bins=3, dist_bins=2, time_span=3, core_span=4)
    assert got.joint.tolist() == [[1, 0], [1, 0], [0, 6], [1, 1]]
    assert got.per_time[:, 0].tolist() == [1, 1, 6, 2] and got.core_clamped == 4 and got.time_span == 3
    # accessory: a = U - I, b = U + cg; (0, 0) with cg = 0 is undefined; a / b = 1 / 2 on the edge of 2 bins goes up
    i = np.array([0, 1, 2, 0, 3], np.uint32)
    u = np.array([0, 2, 2, 4, 4], np.uint32)
    ta = np.array([1, 1, 2, B, 2], np.uint32)
    got = pa.clock_from_counts(ta, None, i, u, 2, 100, 0, metric="acc", time_bins=2, dist_bins=2)
    assert got.undefined_pairs == 1 and got.joint.tolist() == [[0, 1], [2, 0], [0, 1]]
    assert got.per_time.tolist() == [[1, 1, 2], [2, 1, 6], [1, 4, 4]] and got.core_span == 0
    ref.assert_clock(got, ref.clock_from_counts(ref.ACC, ta, None, i, u, 2, 100, 0, 2, 2))


def test_clock_limits_and_their_messages(pa):
    lib = pa.load()
    t, h = np.array([1, 2], np.uint32), np.array([2, 4], np.uint32)
    one = np.array([1, 1], np.uint32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(metric=0, Bt=4, Bx=4, time_span=0, core_span=0, tm=t, hh=h, i=None, u=None, n=2, depth=2, cg=0, out=True):
        prm, o = pa._lib.ClockParams(metric, Bt, Bx, time_span, core_span), pa._lib.Clock()
        joint, pt = np.zeros((Bt + 1) * max(Bx, 1) + 1, np.uint64), np.zeros(3 * (Bt + 1), np.uint64)
        rc = lib.ps_clock_from_counts(p(tm), p(hh), p(i), p(u), n, depth, 10, cg, C.byref(prm), C.byref(o) if out else None, p(joint), p(pt))
        return rc, lib.ps_last_error().decode()

    assert call()[0] == 0
    for kw, text in ((dict(metric=2), "PS_KNN_CORE (0) or PS_KNN_ACC (1), not 2"), (dict(Bt=0), "time_bins and dist_bins must be >= 1"),
                     (dict(Bx=0), "time_bins and dist_bins must be >= 1"), (dict(Bt=1025, Bx=1), "exceeds the limit of 1024 time bins"),
                     (dict(Bt=1023, Bx=17), "= 17408 exceeds the limit of 16384 bins"), (dict(time_span=2**32), "exceeds the limit of 2^32 - 1 generations"),
                     (dict(n=0), "at least one pair"), (dict(depth=0), "1 <= depth < 2^32 - 1"), (dict(depth=2**32 - 1), "1 <= depth < 2^32 - 1"),
                     (dict(tm=np.array([1, 3], np.uint32)), "pair 1: a divergence time is 1 .. depth = 2 or PS_GEN_BEYOND, not 3"),
                     (dict(tm=np.array([0, 1], np.uint32)), "pair 0: a divergence time"), (dict(hh=None), "the metric needs its numerators"),
                     (dict(metric=1, i=one, u=None), "the metric needs its numerators"),
                     (dict(metric=1, i=np.array([1, 3], np.uint32), u=np.array([1, 2], np.uint32)), "pair 1: intersection 3 above union 2"),
                     (dict(metric=1, i=one, u=np.array([1, 65536], np.uint32)), "pair 1: union 65536 above the limit of 65535"),
                     (dict(metric=1, i=one, u=one, cg=2**32 - 65535), "core_genes + 65535 < 2^32"), (dict(out=False), "null"), (dict(tm=None), "null")):
        rc, msg = call(**kw)
        assert rc == PS_ERR_INVALID and text in msg, (kw, rc, msg)
    assert call(Bt=1024, Bx=15)[0] == 0 and call(Bt=1, Bx=8192)[0] == 0 and call(time_span=2**32 - 1)[0] == 0
    with pytest.raises(ValueError):
        pa.clock_from_counts(t, h, None, None, 2, 10, 0, metric="bogus")


def test_every_new_symbol_is_exported_and_declared(pa):
    lib = C.CDLL(pa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pansim_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in pa._lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
    assert lib.ps_abi_version() == 3
    for struct, cls in (("ps_genealogy_t", pa._lib.Genealogy), ("ps_gen_clusters_t", pa._lib.GenClusters), ("ps_clock_params", pa._lib.ClockParams),
                        ("ps_clock_t", pa._lib.Clock)):
        fields = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1)
        assert re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields)) == [n for n, _ in cls._fields_]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert "fn %s(" % name in integration, name
    assert os.path.exists(os.path.join(ROOT, "docs", "GENEALOGY.md"))


def test_the_device_entries_need_a_device(pa):
    """without a device the device entries fail with PS_ERR_NO_DEVICE before they look at their arguments; with one, the same
    calls refuse their null arguments"""
    lib = pa.load()
    g, c, prm = pa._lib.Genealogy(), pa._lib.Clock(), pa._lib.ClockParams(0, 4, 4, 0, 0)
    a, b = np.zeros(16, np.uint32), np.zeros(64, np.uint64)
    want = PS_ERR_NO_DEVICE if lib.ps_device_count() <= 0 else PS_ERR_INVALID
    assert lib.ps_sim_record_ancestry(None, 4) == want
    assert lib.ps_multi_record_ancestry(None, 4) == want
    assert lib.ps_sim_genealogy(None, C.byref(g), a.ctypes.data, a.ctypes.data) == want
    assert lib.ps_multi_genealogy(None, C.byref(g), a.ctypes.data, a.ctypes.data) == want
    assert lib.ps_sim_clock_histogram(None, C.byref(prm), C.byref(c), b.ctypes.data, b.ctypes.data) == want
    assert lib.ps_multi_clock_histogram(None, C.byref(prm), C.byref(c), b.ctypes.data, b.ctypes.data) == want
    if want == PS_ERR_NO_DEVICE:
        assert "no HIP device" in lib.ps_last_error().decode()
        bad = pa._lib.ClockParams(9, 0, 0, 0, 0)                   # ... and before the parameters
        assert lib.ps_sim_clock_histogram(None, C.byref(bad), C.byref(c), b.ctypes.data, b.ctypes.data) == PS_ERR_NO_DEVICE
    assert lib.ps_clock_histogram_timing(None, None, None) == PS_ERR_INVALID


def cli(*args):
    return subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=60)


def test_cli_rejects_bad_values(pa):
    """checked before any device work; the bins and the metric whether or not --print_genealogy is given"""
    for extra in ((), ("--print_genealogy", 3)):
        r = cli("--clock_metric", "bogus", "--pan_genes", 3000, *extra)
        assert r.returncode == 101 and r.stdout == "" and "--clock_metric" in r.stderr and "core or acc" in r.stderr, (r.returncode, r.stderr)
        for value in ("0,4", "4,0", "4", "4,4,4", "x,4", "-1,4", "2.5,4", "1025,1", "1023,17", "4, 4"):
            r = cli("--pan_genes", 3000, "--clock_bins=" + value, *extra)
            assert r.returncode == 101 and r.stdout == "" and "--clock_bins" in r.stderr, (value, r.returncode, r.stderr)
    for value in ("0", "-1", "x", "2.5", "4294967296"):
        r = cli("--pan_genes", 3000, "--print_genealogy=" + value)
        assert r.returncode == 101 and r.stdout == "" and "--print_genealogy" in r.stderr, (value, r.returncode, r.stderr)
    r = cli("--print_genealogy")
    assert r.returncode == 2 and "requires a value" in r.stderr


def test_help_extensions_lists_the_genealogy_flags(pa):
    r = cli("--help-extensions")
    assert r.returncode == 0
    for flag in ("print_genealogy", "clock_bins", "clock_metric"):
        assert "--%s <%s>\n" % (flag, flag) in r.stdout
    for name in ("_genealogy.tsv", "_genealogy.nwk", "_clock.tsv", "_clock_summary.tsv"):
        assert name in r.stdout
    r = cli("--help")
    assert r.returncode == 0 and "genealogy" not in r.stdout and "clock" not in r.stdout
    assert r.stdout[r.stdout.index("USAGE:"):] == open(os.path.join(ROOT, "tests", "golden", "help_usage.txt")).read()
