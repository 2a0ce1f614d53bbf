"""A plain numpy reader AND writer of the simulation state file, written from docs/STATE_FORMAT.md alone: it shares no code
with the library, so that "round trip" in tests/test_state_file.py and tests/test_gpu_state.py cannot mean the same bug twice.

Matrices cross this module in INTERNAL row order and in the library's boundary layout: core (N, L) u8 (individual-major,
like read_matrix), accessory (N, G) u8 of 0 / 1."""
import struct

import numpy as np

MAGIC = b"PANSIMST"
HEADER = 4096
PACKED2, RAW8 = 1, 2
M32 = np.uint64(0xFFFFFFFF)

# (name, kind) in the order of ps_sim_params: u = u64, i = i64, d = double
PARAM_SLOTS = [("pop_size", "u"), ("core_size", "u"), ("pan_genes", "u"), ("core_genes", "u"), ("avg_gene_freq", "d"),
               ("HR_rate", "d"), ("HGT_rate", "d"), ("n_gen", "i"), ("max_distances", "u"), ("core_mu", "d"),
               ("rate_genes1", "d"), ("rate_genes2", "d"), ("prop_genes2", "d"), ("prop_positive", "d"), ("pos_lambda", "d"),
               ("neg_lambda", "d"), ("seed", "u"), ("print_dist", "i"), ("print_matrices", "i"), ("print_selection", "i"),
               ("verbose", "i"), ("no_control_genome_size", "i"), ("genome_size_penalty", "d"), ("competition_strength", "d"),
               ("shard_rank", "i"), ("shard_count", "i"), ("device", "i"), ("reference_seed_stream", "i")]
PARAM_DEFAULTS = dict(pop_size=1000, core_size=1200000, pan_genes=6000, core_genes=2000, avg_gene_freq=0.5, HR_rate=0.05,
                      HGT_rate=0.05, n_gen=100, max_distances=100000, core_mu=0.05, rate_genes1=1.0, rate_genes2=1000.0,
                      prop_genes2=0.1, prop_positive=-0.1, pos_lambda=10.0, neg_lambda=10.0, seed=0, print_dist=0,
                      print_matrices=0, print_selection=0, verbose=0, no_control_genome_size=0, genome_size_penalty=0.99,
                      competition_strength=0.0, shard_rank=0, shard_count=1, device=-1, reference_seed_stream=0)


def checksum(data):
    """sum over the little-endian u32 words w_j of mix(w_j, j), modulo 2^64"""
    w = np.frombuffer(bytes(data), "<u4").astype(np.uint64)
    j = np.arange(w.size, dtype=np.uint64)
    jl, jh = j & M32, j >> np.uint64(32)
    with np.errstate(over="ignore"):
        a = (w + jl * np.uint64(0x9E3779B1) + jh * np.uint64(0x85EBCA77)) & M32
        a ^= a >> np.uint64(16)
        a = (a * np.uint64(0x7FEB352D)) & M32
        a ^= a >> np.uint64(15)
        a = (a * np.uint64(0x846CA68B)) & M32
        a ^= a >> np.uint64(16)
        b = (w * np.uint64(0xC2B2AE3D) + jl) & M32
        return int(np.sum((a << np.uint64(32)) | b, dtype=np.uint64))


def _align(x):
    return (x + 4095) // 4096 * 4096


def geometry(params):
    N, L = params["pop_size"], params["core_size"]
    sb = L * params["shard_rank"] // params["shard_count"]
    se = L * (params["shard_rank"] + 1) // params["shard_count"]
    G = params["pan_genes"] - params["core_genes"]
    return dict(N=N, site_begin=sb, site_end=se, L=se - sb, G=G, GW=(G + 63) // 64, pitch=(N + 127) // 128 * 128)


def pack_core(core, pitch, encoding, padding=None):
    """(N, L) u8 -> the bytes of section 0; `padding`: (L, pitch - N) u8 put into the padding cells (codes 0..3 / any byte)"""
    N, L = core.shape
    rows = np.zeros((L, pitch), np.uint8)
    rows[:, :N] = core.T
    if encoding == RAW8:
        if padding is not None:
            rows[:, N:] = padding
        return rows.tobytes()
    code = np.zeros((L, pitch), np.uint8)
    for allele, c in ((1, 0), (2, 1), (4, 2), (8, 3)):
        code[rows == allele] = c
    assert np.isin(rows[:, :N], (1, 2, 4, 8)).all(), "packed2 holds one-hot cells only"
    if padding is not None:
        code[:, N:] = padding & 3
    q = code.reshape(L, pitch // 4, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8).tobytes()


def unpack_core(data, N, L, pitch, encoding):
    """the bytes of section 0 -> ((N, L) u8 in internal row order, the (L, pitch - N) padding cells as stored)"""
    if encoding == RAW8:
        rows = np.frombuffer(data, np.uint8).reshape(L, pitch)
        return np.ascontiguousarray(rows[:, :N].T), rows[:, N:].copy()
    b = np.frombuffer(data, np.uint8).reshape(L, pitch // 4)
    code = np.stack([(b >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(L, pitch)
    rows = (1 << code).astype(np.uint8)
    return np.ascontiguousarray(rows[:, :N].T), code[:, N:].copy()


def pack_acc(acc, GW):
    N, G = acc.shape
    bits = np.zeros((N, GW * 64), np.uint8)
    bits[:, :G] = acc
    return np.packbits(bits.reshape(N, GW, 8, 8), axis=3, bitorder="little").reshape(N, GW * 8).tobytes()


def unpack_acc(data, N, G, GW):
    b = np.frombuffer(data, np.uint8).reshape(N, GW * 8)
    return np.ascontiguousarray(np.unpackbits(b, axis=1, bitorder="little")[:, :G])


def write(path, params, core, acc, generations_done=0, sigma=None, last_parents=None, encoding=PACKED2, per_gen=None,
          core_overridden=False, acc_overridden=False, padding=None, version=1):
    """write a state file: core (N, L_local) and acc (N, G) in internal row order; sigma / last_parents: the row maps"""
    p = dict(PARAM_DEFAULTS)
    p.update(params)
    g = geometry(p)
    N = g["N"]
    assert core.shape == (N, g["L"]) and acc.shape == (N, g["G"])
    sections = [pack_core(core, g["pitch"], encoding, padding), pack_acc(acc, g["GW"])]
    maps = np.zeros(2 * N, "<u4")
    if sigma is not None:
        maps[:N] = sigma
        maps[N:] = last_parents
    sections.append(maps.tobytes())
    sections.append(b"" if per_gen is None else np.ascontiguousarray(per_gen, "<f8").tobytes())
    if per_gen is not None:
        assert len(sections[3]) == 32 * generations_done
    hdr = bytearray(HEADER)
    hdr[0:8] = MAGIC
    struct.pack_into("<II", hdr, 8, version, HEADER)
    flags = (1 if sigma is not None else 0) | (2 if core_overridden else 0) | (4 if acc_overridden else 0) | (8 if per_gen is not None else 0)
    struct.pack_into("<II", hdr, 24, encoding, flags)
    struct.pack_into("<QQQQQQ", hdr, 32, generations_done, g["G"], g["site_begin"], g["site_end"], g["pitch"], g["GW"])
    body = bytearray()
    offset = HEADER
    for k, s in enumerate(sections):
        body += bytes(offset - HEADER - len(body))          # zeros up to the section's aligned start
        struct.pack_into("<QQQ", hdr, 80 + 24 * k, offset, len(s), checksum(s))
        body += s
        offset = _align(offset + len(s))
    for i, (name, kind) in enumerate(PARAM_SLOTS):
        struct.pack_into({"u": "<Q", "i": "<q", "d": "<d"}[kind], hdr, 192 + 8 * i, p[name])
    struct.pack_into("<Q", hdr, 16, checksum(hdr))
    with open(path, "wb") as f:
        f.write(hdr)
        f.write(body)
    return p


def read(path, verify=True):
    """-> dict: params, header fields, core / acc (internal row order), sigma, last_parents, per_gen, checks"""
    raw = open(path, "rb").read()
    hdr = bytearray(raw[:HEADER])
    assert len(hdr) == HEADER and bytes(hdr[0:8]) == MAGIC
    version, hsize = struct.unpack_from("<II", hdr, 8)
    assert version == 1 and hsize == HEADER
    stored, = struct.unpack_from("<Q", hdr, 16)
    encoding, flags = struct.unpack_from("<II", hdr, 24)
    g0, G, sb, se, pitch, GW = struct.unpack_from("<QQQQQQ", hdr, 32)
    table = [struct.unpack_from("<QQQ", hdr, 80 + 24 * k) for k in range(4)]
    params = {name: struct.unpack_from({"u": "<Q", "i": "<q", "d": "<d"}[kind], hdr, 192 + 8 * i)[0]
              for i, (name, kind) in enumerate(PARAM_SLOTS)}
    geo = geometry(params)
    out = dict(params=params, encoding=encoding, generations_done=g0, pan_size=G, site_begin=sb, site_end=se, pitch=pitch,
               GW=GW, table=table, has_row_maps=bool(flags & 1), core_overridden=bool(flags & 2), acc_overridden=bool(flags & 4),
               has_per_gen=bool(flags & 8), file_bytes=len(raw))
    if verify:
        struct.pack_into("<Q", hdr, 16, 0)
        assert checksum(hdr) == stored, "header checksum"
        assert (G, sb, se, pitch, GW) == (geo["G"], geo["site_begin"], geo["site_end"], geo["pitch"], geo["GW"])
        N, L = geo["N"], geo["L"]
        sizes = [L * pitch // 4 if encoding == PACKED2 else L * pitch, N * GW * 8, 8 * N, 32 * g0 if flags & 8 else 0]
        offset = HEADER
        for k in range(4):
            assert table[k][0] == offset and table[k][1] == sizes[k], "section %d is not where the geometry puts it" % k
            assert checksum(raw[offset:offset + sizes[k]]) == table[k][2], "checksum of section %d" % k
            assert not any(raw[offset + sizes[k]:min(_align(offset + sizes[k]), len(raw))]), "gap behind section %d is not zero" % k
            offset = _align(offset + sizes[k])
        assert len(raw) == table[3][0] + table[3][1], "the file ends with the per-generation section"
    N, L = geo["N"], geo["L"]
    sec = [raw[o:o + n] for o, n, _ in table]
    out["core"], out["padding"] = unpack_core(sec[0], N, L, pitch, encoding)
    out["acc"] = unpack_acc(sec[1], N, G, GW)
    maps = np.frombuffer(sec[2], "<u4")
    out["sigma"], out["last_parents"] = maps[:N].copy(), maps[N:].copy()
    out["per_gen"] = np.frombuffer(sec[3], "<f8").reshape(-1, 4).copy() if flags & 8 else None
    return out


def output_rows(state, which):
    """the matrix as read_matrix returns it: output row k = internal row sigma[k], unless the handle's orders coincide"""
    m = state[which]
    over = state["core_overridden" if which == "core" else "acc_overridden"]
    if over or not state["has_row_maps"]:
        return m
    return np.ascontiguousarray(m[state["sigma"].astype(np.int64)])
