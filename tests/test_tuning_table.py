"""The table of the tuning switches (pansim_amd/csrc/tuning.h) against what is written about it elsewhere: the key list of
include/pansim_hip.h, the keys that the tests and scripts set, the chain of keys it replaced, and the one place that reads
the environment.  No device: ps_tuning_key takes no handle."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pansim_amd", "csrc")

# the keys of the if / else-if chain of ps_set_tuning that the table replaced, in its order
CHAIN_KEYS = ["sweep_blocks_per_cu", "sweep_rows", "sweep_out_of_place", "hgt_apply_threads", "window_blocks_per_cu", "davg_form",
              "core_davg_form", "ld_band", "mlst_band", "gene_team", "gather_form", "core_davg_band", "davg_plain_division", "davg_ib",
              "davg_nb", "hgt_mode", "pair_mode", "pair_ranges", "force_block_sweep", "force_inline_sweep", "hgt_slices", "block_batch",
              "hgt_bin_cap", "hgt_events_per_thread", "window_sweep", "sweep_generations", "sweep_queue_cap", "hgt_list_in_global",
              "hgt_bin_list_in_global", "no_block_preload", "block_waves", "lds_limit"]


def walk(pa):
    lib, keys = pa.load(), []
    while lib.ps_tuning_key(len(keys)) is not None:
        keys.append(lib.ps_tuning_key(len(keys)).decode())
    return keys


def test_keys_are_unique_and_listed_in_the_header_in_table_order(pa):
    keys = walk(pa)
    assert len(set(keys)) == len(keys)
    assert pa.load().ps_tuning_key(len(keys) + 1) is None and pa.load().ps_tuning_key(2**32 - 1) is None
    hdr = open(os.path.join(ROOT, "include", "pansim_hip.h")).read()
    comment = hdr[hdr.index("/* Launch tuning / test hooks"):hdr.index("int ps_set_tuning(")]
    listed = re.findall(r'^ \*   "([a-z_]+)"', comment, flags=re.M)
    assert listed == keys


def test_the_walk_has_every_key_of_the_chain_it_replaced(pa):
    keys = walk(pa)
    assert len(CHAIN_KEYS) == len(set(CHAIN_KEYS)) == 32
    assert set(CHAIN_KEYS) <= set(keys), set(CHAIN_KEYS) - set(keys)
    assert len(keys) >= 33


def test_every_key_that_tests_and_scripts_set_is_in_the_walk(pa):
    keys = set(walk(pa))
    used = {}
    for path in glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True) + glob.glob(os.path.join(ROOT, "scripts", "**", "*.py"), recursive=True):
        for key in re.findall(r"""set_tuning\(\s*["']([A-Za-z0-9_]+)["']""", open(path).read()):
            used.setdefault(key, path)
    assert len(used) >= 20
    assert "test_gpu_parity.py" in used.pop("no_such_key")      # (set there to see it refused)
    assert set(used) <= keys, {k: used[k] for k in set(used) - keys}


def test_the_environment_is_read_in_one_place_and_every_name_is_listed():
    sources = {p: open(p).read() for ext in ("*.h", "*.hip", "*.cpp") for p in glob.glob(os.path.join(CSRC, ext))}
    assert [os.path.basename(p) for p, text in sources.items() if "getenv(" in text] == ["tuning.h"]
    tuning = sources[os.path.join(CSRC, "tuning.h")]
    closing = tuning[tuning.index("// Every PANSIM_* name the library reads"):]
    listed = set(re.findall(r"^//   (PANSIM_[A-Z0-9_]+)(?:, (PANSIM_[A-Z0-9_]+))?", closing, flags=re.M))
    listed = {n for pair in listed for n in pair if n}
    read = {n for text in sources.values() for n in re.findall(r'"(PANSIM_[A-Z0-9_]+)"', text)}
    assert len(read) >= 30      # (the regular expression still finds them)
    assert read == listed, read ^ listed
