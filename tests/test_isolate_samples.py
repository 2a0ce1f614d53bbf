"""Isolate samples without a device (docs/ISOLATE_SAMPLES.md): the six symbols are declared, exported and bound, `subset` is
written once beside _Readouts and asks for the entry of its class, null and empty arguments are refused before a device is looked
for, nothing falls back without one, the host-only ps_genealogy_restrict against brute force over combs built by hand, and the
launch arithmetic of the core gather (pansim_amd/csrc/sample_plan.h) in a host program of its own under the address and
undefined-behaviour sanitizers.  The device half is tests/test_gpu_isolate_samples.py.  Every comparison is an equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS_ERR_INVALID, PS_ERR_NO_DEVICE = -1, -2
NEW_SYMBOLS = ("ps_population_pool", "ps_population_subset", "ps_sim_subset", "ps_multi_subset", "ps_population_subset_timing",
               "ps_genealogy_restrict")
BEYOND = 0xFFFFFFFF


def test_abi_header_and_bindings_agree(pa):
    lib = pa.load()
    hdr = open(os.path.join(ROOT, "include", "pansim_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in pa._lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
        assert "fn %s(" % name in integration, name
        comment = hdr[:hdr.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert "reference has no such function" in comment, name
    assert lib.ps_abi_version() == 3
    assert os.path.exists(os.path.join(ROOT, "docs", "ISOLATE_SAMPLES.md"))
    assert pa.pool is pa.samples.pool and pa.genealogy_restrict is pa.samples.genealogy_restrict
    for method in ("subset", "subset_timing"):
        assert callable(getattr(pa.Population, method))
    assert callable(pa.GenealogyResult.restrict)
    # the tuning key of the form switch is documented where the others are: in the header
    assert b"gather_form" in [lib.ps_tuning_key(k) for k in range(64)] and '"gather_form"' in hdr


def test_both_run_classes_ask_for_their_own_entry(pa):
    """written once in _Samples, not in _Readouts or the two classes; no device: the library is an object that notes the first
    symbol asked for"""
    from pansim_amd import _lib, simulation

    class Asked(Exception):
        pass

    class Library:
        def __getattr__(self, name):
            raise Asked(name)

    assert "subset" in vars(simulation._Samples)
    for other in (simulation._Readouts, simulation._Associations, simulation._Profiles):
        assert "subset" not in vars(other)
    for cls, symbol in ((pa.Simulation, "ps_sim_subset"), (pa.MultiSimulation, "ps_multi_subset")):
        assert hasattr(cls, "subset") and "subset" not in vars(cls)
        run = object.__new__(cls)
        run._lib, run._h, run.generation = Library(), None, 0
        run.params = _lib.SimParams(pop_size=8, core_size=100, pan_genes=60, core_genes=20, max_distances=10)
        for rows in (None, [1, 2, 2]):
            with pytest.raises(Asked) as e:
                run.subset(rows)
            assert str(e.value) == symbol and symbol in _lib.SIGNATURES


def _call(pa, fn, *args):
    rc = fn(*args)
    return rc, pa.load().ps_last_error().decode()


def test_null_and_empty_arguments_are_refused_without_a_device(pa):
    lib = pa.load()
    out, out2 = C.c_void_p(123), C.c_void_p(456)
    fake = (C.c_void_p * 1)(None)
    n = np.array([3], np.uint64)
    rows = np.zeros(3, np.uint32)
    rc, msg = _call(pa, lib.ps_population_pool, None, None, n.ctypes.data, 1, C.byref(out))
    assert rc == PS_ERR_INVALID and "null" in msg and not out.value
    rc, msg = _call(pa, lib.ps_population_pool, fake, None, None, 1, C.byref(out))
    assert rc == PS_ERR_INVALID and "null" in msg
    rc, msg = _call(pa, lib.ps_population_pool, fake, None, n.ctypes.data, 1, None)
    assert rc == PS_ERR_INVALID and "null" in msg
    rc, msg = _call(pa, lib.ps_population_pool, fake, None, n.ctypes.data, 1, C.byref(out))
    assert rc == PS_ERR_INVALID and "parts[0]" in msg
    rc, msg = _call(pa, lib.ps_population_pool, fake, None, n.ctypes.data, 0, C.byref(out))
    assert rc == PS_ERR_INVALID and "n_parts" in msg
    out = C.c_void_p(123)
    rc, msg = _call(pa, lib.ps_population_subset, None, rows.ctypes.data, 3, C.byref(out))
    assert rc == PS_ERR_INVALID and "null" in msg and not out.value
    for fn in (lib.ps_sim_subset, lib.ps_multi_subset):
        out, out2 = C.c_void_p(123), C.c_void_p(456)
        rc, msg = _call(pa, fn, None, rows.ctypes.data, 3, C.byref(out), C.byref(out2))
        assert rc == PS_ERR_INVALID and "null" in msg and not out.value and not out2.value
    assert lib.ps_population_subset_timing(None, None) == PS_ERR_INVALID
    with pytest.raises(pa.PansimError) as e:
        pa.pool([])
    assert e.value.code == PS_ERR_INVALID and "n_parts" in str(e.value)
    with pytest.raises(TypeError):
        pa.pool([object()])


def test_nothing_falls_back_without_a_device(pa):
    """a non-null handle and rows, no device: the entries fail with PS_ERR_NO_DEVICE before they look at the handle (with a
    device the handle would have to be real: tests/test_gpu_isolate_samples.py)"""
    lib = pa.load()
    if lib.ps_device_count() > 0:
        pytest.skip("a GPU is present")
    block = np.zeros(4096, np.uint8)                     # (never read: the device check comes first)
    handle = C.c_void_p(block.ctypes.data)
    parts = (C.c_void_p * 1)(handle)
    n, rows = np.array([3], np.uint64), np.zeros(3, np.uint32)
    out, out2 = C.c_void_p(), C.c_void_p()
    assert lib.ps_population_pool(parts, None, n.ctypes.data, 1, C.byref(out)) == PS_ERR_NO_DEVICE and not out.value
    assert "no HIP device" in lib.ps_last_error().decode()
    assert lib.ps_population_subset(handle, rows.ctypes.data, 3, C.byref(out)) == PS_ERR_NO_DEVICE and not out.value
    for fn in (lib.ps_sim_subset, lib.ps_multi_subset):
        assert fn(handle, rows.ctypes.data, 3, C.byref(out), C.byref(out2)) == PS_ERR_NO_DEVICE and not out.value and not out2.value
    with pytest.raises(pa.PansimError) as e:
        pa.Population(10, 20, 4, True, 0.0, 0, 0).subset([1])
    assert e.value.code == PS_ERR_NO_DEVICE


# -- ps_genealogy_restrict against brute force ---------------------------------------------------------------------------------

def _comb(rng, N, beyond):
    """a comb built by hand: a random permutation of the rows over the internal positions, random coalescence times with ties,
    a few of them beyond the record"""
    order = rng.permutation(N).astype(np.uint32)
    coal = rng.integers(1, max(2, N // 2), max(0, N - 1)).astype(np.uint32)
    if beyond and N > 1:
        coal[rng.choice(N - 1, max(1, (N - 1) // 5), replace=False)] = BEYOND
    return order, coal


def _pair_table(order, coal):
    """tmrca of every pair of ROWS under a comb: 0 on the diagonal, else the maximum of coal between the two positions"""
    N = order.size
    pos = np.empty(N, np.int64)
    pos[order] = np.arange(N)
    T = np.zeros((N, N), np.uint32)
    for i in range(N):
        run = 0
        for j in range(i + 1, N):
            run = max(run, int(coal[j - 1]))
            T[order[i], order[j]] = T[order[j], order[i]] = run
    return T


def _subsets(rng, N):
    yield np.array([rng.integers(N)], np.uint32)
    yield rng.integers(0, N, 2).astype(np.uint32)
    yield np.array([N - 1, N - 1], np.uint32)                     # one row twice
    yield rng.permutation(N).astype(np.uint32)                   # all rows, shuffled
    yield rng.integers(0, N, N).astype(np.uint32)                # N rows with repeats
    yield rng.integers(0, N, min(N + 5, 40)).astype(np.uint32)


@pytest.mark.parametrize("N", [2, 5, 64, 257])
@pytest.mark.parametrize("beyond", [False, True])
def test_genealogy_restrict_against_brute_force(pa, N, beyond):
    rng = np.random.default_rng(1000 * N + beyond)
    order, coal = _comb(rng, N, beyond)
    full = _pair_table(order, coal)
    g = pa._lib.Genealogy(pop_size=N, generation=9, capacity=16, depth=7, roots=1 + int((coal == BEYOND).sum()),
                          tmrca=0 if (coal == BEYOND).any() else int(coal.max()))
    whole = pa.GenealogyResult(g, order, coal)
    assert whole.pair(int(order[0]), int(order[-1])) == full[order[0], order[-1]]          # (the table is the library's pair)
    for rows in _subsets(rng, N):
        n = rows.size
        o, c = pa.genealogy_restrict(order, coal, rows)
        assert o.dtype == np.uint32 and o.size == n and c.size == n - 1
        assert np.array_equal(np.sort(o), np.arange(n))                          # indices into rows, each once
        got = _pair_table(o, c)
        assert np.array_equal(got, full[np.ix_(rows, rows)])                     # ALL a, b
        # repeats stay in the order of their indices, with time 0 between them
        pos = np.empty(N, np.int64)
        pos[order] = np.arange(N)
        keys = list(zip(pos[rows[o]].tolist(), o.tolist()))
        assert keys == sorted(keys)
        res = whole.restrict(rows)
        assert np.array_equal(res.order, o) and np.array_equal(res.coal, c)
        assert res.pop_size == n and res.roots == 1 + int((c == BEYOND).sum())
        assert res.tmrca == (0 if (c == BEYOND).any() or not c.size else int(c.max()))
        assert (res.generation, res.capacity, res.depth) == (9, 16, 7)
        if n >= 2:
            assert res.pair(0, n - 1) == got[0, n - 1]
            r1, r2 = np.triu_indices(n, 1)
            assert np.array_equal(res.pairs(r1, r2), got[r1, r2])
            left, right, height = res.merges()
            assert len(left) == len(right) == len(height) == n - 1 - int((c == BEYOND).sum())
        if np.unique(rows).size == n:
            text = res.newick()
            assert len(text.splitlines()) == text.count(";") == res.roots
            assert sorted(int(x) for x in re.findall(r"(?<![:\d])(\d+)(?=[:;])", text)) == list(range(n))      # every leaf once
        else:
            # (a repeated row sits at time 0 from its copy, and ps_genealogy_newick keeps refusing a time of 0: tests/test_genealogy.py)
            assert (c == 0).any()
            with pytest.raises(pa.PansimError) as e:
                res.newick()
            assert e.value.code == PS_ERR_INVALID and "= 0" in str(e.value)


def test_genealogy_restrict_refuses_bad_arguments(pa):
    lib = pa.load()
    order, coal = np.array([2, 0, 1], np.uint32), np.array([1, 2], np.uint32)
    out = np.zeros(8, np.uint32)
    p = lambda a: a.ctypes.data                                                  # noqa: E731
    rows = np.array([0, 3], np.uint32)
    rc, msg = _call(pa, lib.ps_genealogy_restrict, p(order), p(coal), 3, p(rows), 2, p(out), p(out))
    assert rc == PS_ERR_INVALID and "rows[1]" in msg
    rc, msg = _call(pa, lib.ps_genealogy_restrict, p(order), p(coal), 3, p(rows), 0, p(out), p(out))
    assert rc == PS_ERR_INVALID and "n_rows" in msg
    rc, msg = _call(pa, lib.ps_genealogy_restrict, p(order), p(coal), 3, None, 2, p(out), p(out))
    assert rc == PS_ERR_INVALID and "null" in msg
    bad = np.array([0, 0, 1], np.uint32)
    rc, msg = _call(pa, lib.ps_genealogy_restrict, p(bad), p(coal), 3, p(rows[:1]), 1, p(out), p(out))
    assert rc == PS_ERR_INVALID and "permutation" in msg


def test_gather_plans_hold_their_invariants(tmp_path):
    """tests/sample_plan_check.cpp: every launch the host arithmetic can choose covers its bytes once, stays inside the LDS, the
    block and the grid limits; built with the sanitizers, nothing loaded into Python"""
    exe = str(tmp_path / "sample_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "sample_plan_check.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1].startswith("every plan holds") and not any("BAD" in line for line in lines)
