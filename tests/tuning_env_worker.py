"""What a fresh process sees of the PANSIM_* variables that set a tuning switch at creation -- test infrastructure, started as
a subprocess by tests/test_gpu_tuning.py with the variable in the child's environment only.

    python tests/tuning_env_worker.py pop KEY            a core and an accessory population of N = 64 with 8 columns
    python tests/tuning_env_worker.py sim KEY [exchange] a Simulation of N = 64 (shard 0 of 2 with an exchange function installed)
Prints one JSON line: get_tuning(KEY) of the core and of the accessory handle."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pansim_amd as pa  # noqa: E402
from pansim_amd import _lib  # noqa: E402


def main():
    mode, key = sys.argv[1], sys.argv[2]
    if mode == "pop":
        core = pa.Population(64, 8, 4, True, 0.0, 1, 4, device=0)
        acc = pa.Population(64, 8, 2, False, 0.5, 1, 4, device=0)
        owner = None
    else:
        shard = dict(shard_rank=0, shard_count=2) if sys.argv[3:] == ["exchange"] else {}
        owner = pa.Simulation(pa.make_params(seed=1, n_gen=1, max_distances=10, pop_size=64, core_size=200, pan_genes=60, core_genes=20, device=0, **shard))
        if shard:
            owner.set_exchange(_lib.EXCHANGE_FN(lambda ctx, words, n_words, stream: 0))
        core, acc = owner.core_genome, owner.pan_genome
    print(json.dumps(dict(core=core.get_tuning(key), acc=acc.get_tuning(key))))
    for h in filter(None, (owner, core, acc)):
        h.close()


if __name__ == "__main__":
    main()
