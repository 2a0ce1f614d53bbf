"""The tuning switches on real handles: what every key accepts and refuses, word for word; what every PANSIM_* variable does to
a new handle, in range and out of it; the two "was the variable given" decisions of a Simulation.  The literals are those of the
if / else-if chain and of the environment block that the table of pansim_amd/csrc/tuning.h replaced."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "tuning_env_worker.py")

# key -> (accepted values, one refused value, what ps_last_error then says); the listed-set keys refuse a value inside their span
KEYS = {
    "sweep_blocks_per_cu": ([1, 5, 8], 9, "sweep_blocks_per_cu must be 1..8"),
    "sweep_rows": ([2, 3, 4], 5, "sweep_rows must be 2..4"),
    "sweep_out_of_place": ([-1, 0, 1, 2], 3, "sweep_out_of_place must be -1 (choose), 0 (in place), 1 (out of place) or 2 (out of place, nontemporal loads and stores)"),
    "hgt_apply_threads": ([256, 512, 1024], 768, "hgt_apply_threads must be 256, 512 or 1024"),
    "window_blocks_per_cu": ([0, 3, 8], 9, "window_blocks_per_cu must be 0 (choose) or 1..8"),
    "davg_form": ([0, 1, 2, 3], 4, "davg_form must be 0 (choose), 1 (LDS-tile popcount kernels), 2 (matrix cores, one kernel) or 3 (matrix cores, two phases)"),
    "core_davg_form": ([0, 1, 2, 3], -1, "core_davg_form must be 0 (choose), 1 (whole matrix), 2 (banded) or 3 (generic)"),
    "ld_band": ([0, 64, 65536], 65537, "ld_band must be 0 (choose)..65536 rows of loci"),
    "mlst_band": ([0, 7, 65535], 65536, "mlst_band must be 0 (choose)..65535 loci"),
    "gene_team": ([0, 64, 256], 128, "gene_team must be 0 (choose), 64 or 256 threads"),
    "gather_form": ([0, 1, 2], 3, "gather_form must be 0 (choose), 1 (source rows staged in LDS) or 2 (bytes loaded from global memory)"),
    "core_davg_band": ([0, 256, 2**31], 2**31 + 1, "core_davg_band must be 0 (choose)..2^31 rows"),
    "davg_plain_division": ([0, 1], None, None),
    "davg_ib": ([0, 16, 32], 24, "davg_ib must be 0 (choose), 16 or 32"),
    "davg_nb": ([0, 1, 2, 4], 3, "davg_nb must be 0 (choose), 1, 2 or (two-phase form only) 4"),
    "hgt_mode": ([0, 1, 2], 3, "hgt_mode must be 0 (auto), 1 (one atomic per event) or 2 (binned by recipient partition, two passes)"),
    "pair_mode": ([0, 1, 2, 3, 4, 5, 6, 7], 8, "pair_mode must be 0 (auto), 1 (sampled), 2 (all pairs), 3 (sampled, nibble form even for one-hot matrices), 4 (transposed bit strings, streamed per pair), 5 (all pairs, xor + popcount tiles even for one-hot matrices), 6 (all pairs, i8 matrix cores when the matrix is one-hot; mode 2 takes the FP4 form) or 7 (the FP4 form on three +-1 features per site)"),
    "pair_ranges": ([0, 3, 65535], 65536, "pair_ranges must be 0 (choose)..65535"),
    "force_block_sweep": ([0, 1], None, None),
    "force_inline_sweep": ([0, 1], None, None),
    "hgt_slices": ([0, 5, 4096], 4097, "hgt_slices must be 0..4096"),
    "block_batch": ([0, 2, 4], 3, "block_batch must be 0 (choose), 2 or 4"),
    "hgt_bin_cap": ([0, 17, 2**30], 2**30 + 1, "hgt_bin_cap must be 0 (sized by the rates)..2^30"),
    "hgt_events_per_thread": ([0, 175, 100000], 100001, "hgt_events_per_thread must be 0 (whole chip)..100000"),
    "window_sweep": ([-1, 0, 1], 2, "window_sweep must be -1 (choose), 0 (block sweep) or 1 (window sweep where the parents are sorted)"),
    "sweep_generations": ([0, 1, 2], 3, "sweep_generations must be 0 (choose), 1 or 2"),
    "sweep_queue_cap": ([0, 9, 65536], 65537, "sweep_queue_cap must be 0 (real size)..65536"),
    "hgt_list_in_global": ([0, 1], None, None),
    "hgt_bin_list_in_global": ([0, 1], None, None),
    "no_block_preload": ([0, 1], None, None),
    "block_waves": ([0, 4, 8, 16], 12, "block_waves must be 0 (auto), 4, 8 or 16"),
    "lds_limit": ([1024, 65536, 160 * 1024], 1023, "lds_limit must be 1 KiB..160 KiB"),
}
# the two switches that only the environment sets: ps_get_tuning reads them, ps_set_tuning never knew their names
ENV_ONLY = ["free_cus_per_xcd", "hgt_bin_prio"]

# variable -> (key, value in range, what the handles then read, value out of range, what they read then): an out-of-range
# value is ignored (the default stays), clamped to the nearest end, or taken as it is, as the environment block had it
ENV = {
    "PANSIM_SWEEP_BLOCKS_PER_CU": ("sweep_blocks_per_cu", "3", 3, "9", 8),         # ignored
    "PANSIM_SWEEP_ROWS": ("sweep_rows", "2", 4, "9", 4),                           # (accepted and ignored: always 4)
    "PANSIM_SWEEP_OOP": ("sweep_out_of_place", "1", 1, "7", 2),                    # clamped
    "PANSIM_SWEEP_GENERATIONS": ("sweep_generations", "1", 1, "5", 0),             # ignored
    "PANSIM_WINDOW_SWEEP": ("window_sweep", "0", 0, "-5", -1),                     # clamped
    "PANSIM_WINDOW_BPC": ("window_blocks_per_cu", "3", 3, "12", 8),                # clamped
    "PANSIM_BLOCK_BATCH": ("block_batch", "2", 2, "3", 3),                         # taken
    "PANSIM_BLOCK_WAVES": ("block_waves", "8", 8, "5", 5),                         # taken
    "PANSIM_HGT_MODE": ("hgt_mode", "2", 2, "7", 7),                               # taken
    "PANSIM_HGT_SLICES": ("hgt_slices", "16", 16, "5000", 5000),                   # taken
    "PANSIM_HGT_APPLY_THREADS": ("hgt_apply_threads", "512", 512, "768", 1024),    # ignored
    "PANSIM_HGT_BIN_LIST_GLOBAL": ("hgt_bin_list_in_global", "1", 1, "7", 1),      # (0/1: any non-zero number is 1)
    "PANSIM_HGT_BIN_PRIO": ("hgt_bin_prio", "2", 2, "9", 3),                       # clamped
    "PANSIM_ACC_LDS_LIMIT": ("lds_limit", "65536", 65536, "100", 160 * 1024),      # ignored; accessory handles only
    "PANSIM_SWEEP_FREE_CUS": ("free_cus_per_xcd", "2", None, "11", None),          # clamped; core handles only (see the test)
}


@pytest.fixture
def pops(pa):
    core = pa.Population(64, 8, 4, True, 0.0, 1, 4, device=0)
    acc = pa.Population(64, 8, 2, False, 0.5, 1, 4, device=0)
    yield core, acc
    core.close()
    acc.close()


def test_the_literal_tables_cover_the_table(pa):
    lib, keys = pa.load(), []
    while lib.ps_tuning_key(len(keys)) is not None:
        keys.append(lib.ps_tuning_key(len(keys)).decode())
    assert sorted(keys) == sorted(list(KEYS) + ENV_ONLY)
    assert {key for key, *_ in ENV.values()} <= set(keys)


@pytest.mark.parametrize("key", list(KEYS))
def test_key_accepts_reads_back_and_refuses(pa, pops, key):
    accepted, refused, message = KEYS[key]
    for pop in pops:
        for value in accepted:
            pop.set_tuning(key, value)
            # ("sweep_rows" is accepted and ignored: it reads as the 4 that the sweep does)
            assert pop.get_tuning(key) == (4 if key == "sweep_rows" else value)
        if refused is None:         # a 0/1 switch: every non-zero value is 1
            pop.set_tuning(key, 5)
            assert pop.get_tuning(key) == 1
            pop.set_tuning(key, 0)
            assert pop.get_tuning(key) == 0
            continue
        before = pop.get_tuning(key)
        with pytest.raises(pa.PansimError) as e:
            pop.set_tuning(key, refused)
        assert e.value.code == -1                                   # PS_ERR_INVALID
        assert pa.load().ps_last_error().decode() == message
        assert pop.get_tuning(key) == before


def test_unknown_and_null_keys(pa, pops):
    lib = pa.load()
    for pop in pops:
        for key in ["no_such_key", ""] + ENV_ONLY:
            with pytest.raises(pa.PansimError) as e:
                pop.set_tuning(key, 1)
            assert e.value.code == -1 and lib.ps_last_error().decode() == "unknown tuning key %s" % key
        with pytest.raises(pa.PansimError) as e:
            pop.get_tuning("no_such_key")
        assert e.value.code == -1 and lib.ps_last_error().decode() == "unknown tuning key no_such_key"
        assert lib.ps_set_tuning(pop._h, None, 1) == -1 and lib.ps_last_error().decode() == "null argument"
        assert lib.ps_get_tuning(pop._h, None, None) == -1 and lib.ps_last_error().decode() == "null argument"
        for key in ENV_ONLY:
            assert pop.get_tuning(key) == 0
    assert lib.ps_set_tuning(None, b"lds_limit", 1024) == -1 and lib.ps_last_error().decode() == "null argument"


def test_lds_limit_drops_the_cached_pair_list(pa, pops):
    # The device copy of a pair list is sorted and has a thread table only when a tile of the matrix fits "lds_limit": the same
    # list around a change of the limit gives the same counts, by the kernel form that a handle which never cached it takes.
    core, _ = pops
    rng = np.random.default_rng(5)
    rows = (1 << rng.integers(0, 4, (64, 8))).astype(np.uint8)
    r1, r2 = rng.integers(0, 64, 300).astype(np.uint32), rng.integers(0, 64, 300).astype(np.uint32)
    want = np.unpackbits(rows[r1] ^ rows[r2], axis=1).sum(1).astype(np.uint32)      # (distances.rs:22-52: differing bits of the one-hot bytes)
    fresh = pa.Population(64, 8, 4, True, 0.0, 1, 4, device=0)
    forms = []
    for pop in (core, fresh):
        pop.load_matrix(rows)
    for limit in (160 * 1024, 1024, 160 * 1024):
        core.set_tuning("lds_limit", limit)
        (got,) = core.pairwise_counts(r1, r2)
        assert np.array_equal(got, want)
        forms.append(core.last_pair_form())
    fresh.set_tuning("lds_limit", 1024)
    (got,) = fresh.pairwise_counts(r1, r2)
    assert np.array_equal(got, want)
    assert forms[1] == fresh.last_pair_form() and forms[0] == forms[2]
    fresh.close()


def child(mode, key, extra=(), **env):
    full = {k: v for k, v in os.environ.items() if k not in ENV}
    full.update(env)
    r = subprocess.run([sys.executable, WORKER, mode, key, *extra], env=full, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("name", list(ENV))
def test_environment_value_in_and_out_of_range(name):
    key, inside, want_in, outside, want_out = ENV[name]
    for value, want in ((inside, want_in), (outside, want_out)):
        got = child("pop", key, **{name: value})
        if name == "PANSIM_SWEEP_FREE_CUS":     # (a box may refuse the CU-masked stream: the handle then has an ordinary one and reads 0)
            assert 0 <= got["core"] <= 8 and got["acc"] == 0
        elif name == "PANSIM_ACC_LDS_LIMIT":
            assert got == dict(core=160 * 1024, acc=want)
        else:
            assert got == dict(core=want, acc=want)


@pytest.mark.parametrize("given,want", [(None, 4), ("3", 3), ("8", 8), ("99", 8)])
def test_sim_chooses_sweep_blocks_per_cu_unless_the_variable_is_given(given, want):
    # ps_sim_create puts 4 workgroups of the wave sweep on a CU unless PANSIM_SWEEP_BLOCKS_PER_CU is PRESENT: then the handle
    # keeps what its creation made of the variable (a refused value: the default, 8)
    env = {} if given is None else dict(PANSIM_SWEEP_BLOCKS_PER_CU=given)
    assert child("sim", "sweep_blocks_per_cu", **env)["core"] == want


@pytest.mark.parametrize("given,exchange,want", [(None, True, 5), ("0", True, 0), ("3", True, 3), (None, False, 0)])
def test_sim_with_an_exchange_chooses_window_bpc_unless_the_variable_is_given(given, exchange, want):
    # ps_sim_set_exchange makes a window_blocks_per_cu of 0 (choose) 5 unless PANSIM_WINDOW_BPC is PRESENT, a 0 included
    env = {} if given is None else dict(PANSIM_WINDOW_BPC=given)
    assert child("sim", "window_blocks_per_cu", ("exchange",) if exchange else (), **env)["core"] == want
