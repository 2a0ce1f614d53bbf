"""ps_bfi (pansim_amd/csrc/core_kernels.h), the byte select of the symbol-decided mutations: the host form against the
defining expression on random words, and the truth table the device form hands to v_bitop3_b32 (0xCA in the order mask,
allele, child) against the eight input combinations.  The probe is the header's host side (no kernel is instantiated or run)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pansim_amd", "csrc")

PROBE = """
#include "core_kernels.h"
extern "C" void probe_bfi(const uint32_t *m, const uint32_t *a, const uint32_t *b, uint32_t *out, uint64_t n)
{
    for (uint64_t i = 0; i < n; i++) out[i] = ps_bfi(m[i], a[i], b[i]);
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("bfi_probe")
    src, so = d / "probe.hip", d / "libprobe.so"
    src.write_text(PROBE)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-shared", "-Wno-unused-function", "-I", CSRC,
                    "-o", str(so), str(src)], check=True, capture_output=True, text=True, timeout=300)
    lib = ctypes.CDLL(str(so))
    lib.probe_bfi.restype = None
    lib.probe_bfi.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_uint64]

    def bfi(m, a, b):
        m, a, b = (np.ascontiguousarray(x, np.uint32) for x in (m, a, b))
        out = np.zeros_like(m)
        lib.probe_bfi(m.ctypes.data, a.ctypes.data, b.ctypes.data, out.ctypes.data, m.size)
        return out
    return bfi


def test_host_select_equals_its_definition(probe):
    rng = np.random.default_rng(0xCA)
    m, a, b = (rng.integers(0, 1 << 32, 100000, dtype=np.uint64).astype(np.uint32) for _ in range(3))
    m[:4] = (0, 0xFFFFFFFF, 0x00FF00FF, 0x24242424)
    assert np.array_equal(probe(m, a, b), (a & m) | (b & ~m))


def _device_table():
    # the immediate of the device form, read from the source
    txt = open(os.path.join(CSRC, "core_kernels.h")).read()
    body = txt[txt.index("uint32_t ps_bfi("):]
    body = body[:body.index("\n}")]
    (imm,) = re.findall(r"__builtin_amdgcn_bitop3_b32\(m, a, b, (0x[0-9A-Fa-f]+)\)", body)
    return int(imm, 16)


def test_truth_table_is_a_bit_field_insert(probe):
    table = _device_table()
    assert table == 0xCA
    # v_bitop3_b32: bit (m << 2 | a << 1 | b) of the immediate is the result for the input bits (m, a, b)
    for m in (0, 1):
        for a in (0, 1):
            for b in (0, 1):
                want = (a & m) | (b & ~m & 1)
                assert (table >> (m << 2 | a << 1 | b)) & 1 == want
                got = probe([0xFFFFFFFF * m], [0xFFFFFFFF * a], [0xFFFFFFFF * b])[0]
                assert got == 0xFFFFFFFF * want
    assert [i for i in range(8) if table >> i & 1] == [1, 3, 6, 7]
