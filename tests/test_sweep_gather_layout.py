"""The transposed lane mapping of the wave sweep's gather (pansim_amd/csrc/core_kernels.h: ps_gather_dword,
ps_gather_child, ps_gather_source) and the LDS bank model that motivates it (scripts/lds_gather_banks.py).
The probe is the header's host side (no kernel is instantiated or run)."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pansim_amd", "csrc")

PROBE = """
#include "core_kernels.h"
// child[64 * 4 * 4], dword[64 * 4]: the whole mapping of a wave
extern "C" void probe_mapping(uint32_t *child, uint32_t *dword)
{
    for (uint32_t lane = 0; lane < 64; lane++)
        for (uint32_t m = 0; m < 4; m++) {
            dword[4 * lane + m] = ps_gather_dword(lane, m);
            for (uint32_t b = 0; b < 4; b++) child[16 * lane + 4 * m + b] = ps_gather_child(lane, m, b);
        }
}
extern "C" uint32_t probe_source(uint32_t child, uint32_t parent, uint32_t N, uint32_t pitch) { return ps_gather_source(child, parent, N, pitch); }
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("gather_probe")
    src, so = d / "probe.hip", d / "libprobe.so"
    src.write_text(PROBE)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-shared", "-Wno-unused-function", "-I", CSRC,
                    "-o", str(so), str(src)], check=True, capture_output=True, text=True, timeout=300)
    lib = ctypes.CDLL(str(so))
    lib.probe_mapping.restype = None
    lib.probe_mapping.argtypes = [ctypes.c_void_p] * 2
    lib.probe_source.restype = ctypes.c_uint32
    lib.probe_source.argtypes = [ctypes.c_uint32] * 4
    return lib


@pytest.fixture(scope="module")
def mapping(probe):
    child = np.zeros((64, 4, 4), np.uint32)
    dword = np.zeros((64, 4), np.uint32)
    probe.probe_mapping(child.ctypes.data, dword.ctypes.data)
    return child, dword


@pytest.fixture(scope="module")
def banks():
    spec = importlib.util.spec_from_file_location("lds_gather_banks", os.path.join(ROOT, "scripts", "lds_gather_banks.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_mapping_is_a_permutation_of_the_lds_row(mapping):
    child, dword = mapping
    assert np.array_equal(np.sort(dword.ravel()), np.arange(256))           # the 256 dwords of a 1024-byte LDS row, once each
    assert np.array_equal(np.sort(child.ravel()), np.arange(1024))
    assert np.array_equal(child, 4 * dword[:, :, None] + np.arange(4))      # byte b of the dword a lane stores
    assert np.array_equal(dword, np.arange(64)[:, None] + 64 * np.arange(4))     # the 64 lanes of a store: 64 neighbouring dwords


@pytest.mark.parametrize("pitch", range(16, 1025, 16))
def test_every_child_dword_of_a_row_is_gathered_exactly_once(mapping, pitch):
    child, dword = mapping
    inside = dword < pitch // 4
    assert np.array_equal(np.sort(dword[inside]), np.arange(pitch // 4))
    assert np.array_equal(np.sort(child[inside].ravel()), np.arange(pitch))
    # the lanes that gather a dword of the row are a prefix of the wave for every m (no holes for the redo path to meet)
    for m in range(4):
        lanes = np.flatnonzero(inside[:, m])
        assert np.array_equal(lanes, np.arange(lanes.size))
    assert (child[~inside] >= pitch).all()


@pytest.mark.parametrize("pitch", range(16, 1025, 16))
def test_padding_cells_gather_the_zero_byte(probe, mapping, pitch):
    child, _ = mapping
    rng = np.random.default_rng(pitch)
    for N in sorted({1, pitch - 15, pitch - 1, pitch, max(1, pitch - 127), int(rng.integers(1, pitch + 1))}):
        if N < 1:
            continue
        parents = np.sort(rng.integers(0, N, N))
        for c in child.ravel():
            c = int(c)
            got = probe.probe_source(c, int(parents[c]) if c < N else 0, N, pitch)
            if c < N:
                assert got == parents[c]
            elif c < pitch:
                # a cell of the row that holds no individual: its source is a padding byte (>= N: zero in every state the
                # library keeps, and its own source), inside the row
                assert N <= got < pitch and probe.probe_source(got, 0, N, pitch) == got
            else:
                assert got < pitch                  # past the row: any byte of the row will do, nothing of it is stored


def test_bank_model_uses_the_header_mapping(mapping, banks):
    child, _ = mapping
    for i in range(banks.INSTRUCTIONS):
        assert np.array_equal(banks.children("transposed", i), child[:, i // 4, i % 4])
        assert np.array_equal(banks.children("chunk", i), 16 * np.arange(64) + i)


def test_bank_model_figures(banks):
    draws = 200
    w = np.ones(banks.N)
    chunk, n_chunk = banks.model(w, draws, "chunk")
    transposed, n_tr = banks.model(w, draws, "transposed")
    # no instruction hidden: all 16 of every draw are in the mean
    assert n_chunk == n_tr == 16 * draws
    assert abs(chunk - 5.9) <= 0.3
    assert abs(transposed - 2.7) <= 0.3
    assert transposed >= 2.0            # two lane groups: the conflict-free floor


def test_bank_model_counts_a_known_pattern(banks):
    lanes = np.arange(64)
    assert banks.instruction_cycles(4 * lanes) == 2                   # 32 neighbouring dwords per group
    assert banks.instruction_cycles(np.zeros(64, np.int64)) == 2      # one dword: broadcast
    assert banks.instruction_cycles(4 * lanes + 3) == 2               # bytes of neighbouring dwords
    assert banks.instruction_cycles(128 * lanes) == 64                # every lane another dword of bank 0
    assert banks.instruction_cycles(16 * lanes) == 8                  # 16 bytes apart: 8 banks, 4 dwords each, per group
