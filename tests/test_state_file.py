"""State files without a device (docs/STATE_FORMAT.md): ps_state_info against files written by the independent numpy
restatement of the format (tests/state_file_ref.py), the refusals of damaged files, and the no-device errors of
ps_sim_save / ps_sim_load.  The device half is tests/test_gpu_state.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

import state_file_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pansim_amd", "pansim")
PS_ERR_INVALID, PS_ERR_NO_DEVICE, PS_ERR_IO = -1, -2, -5


def _random_state(tmp_path, name="s.state", encoding=ref.PACKED2, per_gen=True, g0=5, **over):
    params = dict(pop_size=77, core_size=203, pan_genes=330, core_genes=100, seed=11, HR_rate=0.25, n_gen=9, max_distances=50)
    params.update(over)
    geo = ref.geometry(dict(ref.PARAM_DEFAULTS, **params))
    rng = np.random.default_rng(5)
    N, L, G = geo["N"], geo["L"], geo["G"]
    core = (1 << rng.integers(0, 4, (N, L))).astype(np.uint8)
    if encoding == ref.RAW8:
        core[3, 7], core[5, 0] = 255, 16
    acc = (rng.random((N, G)) < 0.4).astype(np.uint8)
    sigma = rng.permutation(N).astype(np.uint32)
    parents = rng.integers(0, N, N).astype(np.uint32)
    rows = rng.random((g0, 4)) if per_gen else None
    path = str(tmp_path / name)
    ref.write(path, params, core, acc, generations_done=g0, sigma=sigma, last_parents=parents, encoding=encoding, per_gen=rows)
    return path, params, geo, rows


@pytest.mark.parametrize("encoding", [ref.PACKED2, ref.RAW8])
@pytest.mark.parametrize("shard", [{}, dict(shard_rank=1, shard_count=3)])
def test_state_info_reads_a_file_written_from_the_document(pa, tmp_path, encoding, shard):
    path, params, geo, rows = _random_state(tmp_path, encoding=encoding, **shard)
    info = pa.state_info(path, per_gen=True)
    for k, v in params.items():
        assert getattr(info["params"], k) == v, k
    assert info["params"].core_mu == 0.05 and info["params"].device == -1
    h = info["header"]
    assert info["generations_done"] == 5 and info["encoding"] == ("packed2" if encoding == ref.PACKED2 else "raw8")
    assert (h.pan_size, h.site_begin, h.site_end, h.pitch) == (geo["G"], geo["site_begin"], geo["site_end"], geo["pitch"])
    N, L, GW, pitch = geo["N"], geo["L"], geo["GW"], geo["pitch"]
    assert h.core_bytes == (L * pitch // 4 if encoding == ref.PACKED2 else L * pitch)
    assert (h.acc_bytes, h.maps_bytes, h.per_gen_bytes) == (N * GW * 8, 8 * N, 32 * 5)
    assert h.core_offset == 4096 and h.acc_offset % 4096 == 0 and h.maps_offset % 4096 == 0 and h.per_gen_offset % 4096 == 0
    assert h.has_row_maps == 1 and h.has_per_gen == 1 and h.core_rows_overridden == 0 and h.acc_rows_overridden == 0
    assert np.array_equal(info["per_gen"], rows)
    assert os.path.getsize(path) == h.per_gen_offset + h.per_gen_bytes
    # the reference reads its own file back, checksums and gaps included
    assert ref.read(path)["generations_done"] == 5


def test_state_info_without_a_per_generation_section(pa, tmp_path):
    path, _params, _geo, _rows = _random_state(tmp_path, per_gen=False)
    info = pa.state_info(path, per_gen=True)
    assert info["per_gen"] is None and info["header"].has_per_gen == 0 and info["header"].per_gen_bytes == 0
    buf = np.zeros(64)
    rc = pa.load().ps_state_info(path.encode(), None, None, buf.ctypes.data, 64)
    assert rc == PS_ERR_INVALID and b"per-generation" in pa.load().ps_last_error()


def _info_error(pa, path):
    with pytest.raises(pa.PansimError) as e:
        pa.state_info(path, per_gen=True)
    return e.value.code, str(e.value)


def test_damaged_files_are_refused_with_a_message_that_names_what(pa, tmp_path):
    path, _params, _geo, _rows = _random_state(tmp_path)
    raw = open(path, "rb").read()

    def variant(name, data):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        return p
    code, msg = _info_error(pa, str(tmp_path / "missing.state"))
    assert code == PS_ERR_IO and "cannot open" in msg
    code, msg = _info_error(pa, variant("short_header", raw[:1000]))
    assert code == PS_ERR_IO and "truncated header" in msg
    code, msg = _info_error(pa, variant("short", raw[:len(raw) - 8]))
    assert code == PS_ERR_IO and "truncated" in msg and "per-generation section" in msg
    code, msg = _info_error(pa, variant("short_core", raw[:4096 + 100]))
    assert code == PS_ERR_IO and "truncated" in msg and "core section" in msg
    code, msg = _info_error(pa, variant("magic", b"PANSIMXX" + raw[8:]))
    assert code == PS_ERR_IO and "bad magic" in msg
    future = bytearray(raw)
    struct.pack_into("<I", future, 8, 2)
    code, msg = _info_error(pa, variant("future", bytes(future)))
    assert code == PS_ERR_IO and "version 2" in msg
    for at in (33, 200, 300, 3000):          # generations_done, a parameter, the seed's neighbourhood, an unused byte
        flipped = bytearray(raw)
        flipped[at] ^= 0x40
        code, msg = _info_error(pa, variant("flip%d" % at, bytes(flipped)))
        assert code == PS_ERR_IO and "header: checksum mismatch" in msg, at
    # a flipped byte inside the per-generation section is found when the rows are asked for
    h = pa.state_info(path)["header"]
    flipped = bytearray(raw)
    flipped[h.per_gen_offset + 9] ^= 1
    code, msg = _info_error(pa, variant("flip_rows", bytes(flipped)))
    assert code == PS_ERR_IO and "per-generation section: checksum mismatch" in msg
    assert pa.state_info(path, per_gen=True)["generations_done"] == 5      # and nothing sticks


def test_a_header_whose_geometry_does_not_follow_from_its_parameters_is_refused(pa, tmp_path):
    path, _params, _geo, _rows = _random_state(tmp_path)
    raw = bytearray(open(path, "rb").read())
    struct.pack_into("<Q", raw, 64, 256)           # pitch
    struct.pack_into("<Q", raw, 16, 0)
    struct.pack_into("<Q", raw, 16, ref.checksum(raw[:4096]))
    p = str(tmp_path / "pitch.state")
    open(p, "wb").write(bytes(raw))
    code, msg = _info_error(pa, p)
    assert code == PS_ERR_IO and "pitch" in msg


def test_the_checksum_detects_any_single_changed_byte():
    # (of the reference's restatement; the library's is held to it by the files above and by tests/test_gpu_state.py)
    rng = np.random.default_rng(2)
    data = bytearray(rng.integers(0, 256, 4096, dtype=np.uint8).tobytes())
    base = ref.checksum(data)
    for at in rng.integers(0, 4096, 64):
        for bit in (0, 3, 7):
            d = bytearray(data)
            d[at] ^= 1 << bit
            assert ref.checksum(d) != base
    # two words that change places are a different section
    d = bytearray(data)
    d[0:4], d[400:404] = data[400:404], data[0:4]
    assert ref.checksum(d) != base


def test_save_and_load_need_a_device(pa, tmp_path):
    if pa.load().ps_device_count() > 0:
        pytest.skip("a GPU is present")
    path, _params, _geo, _rows = _random_state(tmp_path)
    with pytest.raises(pa.PansimError) as e:
        pa.Simulation.load(path)
    assert e.value.code == PS_ERR_NO_DEVICE
    with pytest.raises(pa.PansimError) as e:
        pa.Simulation.load(path, pa.make_params(pop_size=77, core_size=203, pan_genes=330, core_genes=100))
    assert e.value.code == PS_ERR_NO_DEVICE
    # there is no ps_sim without a device, so ps_sim_save can only be handed nothing
    assert pa.load().ps_sim_save(None, path.encode(), None) == PS_ERR_INVALID
    assert pa.load().ps_sim_generations_done(None) == 0


def test_help_extensions_lists_the_state_flags(pa):
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()
    r = subprocess.run([EXE, "--help-extensions"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--save_state <save_state>" in r.stdout and "--load_state <load_state>" in r.stdout
    assert "[default: ]" not in r.stdout
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert "save_state" not in r.stdout and "load_state" not in r.stdout


def test_cli_refuses_state_files_on_several_shards_before_it_touches_a_device(pa, tmp_path):
    r = subprocess.run([EXE, "--pan_genes", "600", "--core_genes", "200", "--gpus", "2", "--save_state", str(tmp_path / "x.state")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 101 and "--gpus 1" in r.stderr and not os.path.exists(tmp_path / "x.state")
