#!/usr/bin/env python3
"""LDS bank model of the wave sweep's byte gather (profiles/sweep_transposed_gather.md): LDS-array cycles
per gather instruction (one ds_read_u8 of a wave) for the two lane mappings, over sorted multinomial parents.

The model is ds_read_b32's banking: a wave's access is served in two groups of 32 lanes, the bank of byte address a is
(a / 4) mod 32, lanes that read the same dword share one access (broadcast), and a group takes as many cycles as its busiest
bank has distinct dwords.  That ds_read_u8 banks the same way is an ASSUMPTION of the model; the counters of
scripts/ubench/sweep_skeleton.hip (`gens`) are its check.

  chunk:       lane l gathers the 16 children of its own chunk, 16 l + k (instruction k)
  transposed:  lane l gathers children 4 (l + 64 m) + b (instruction (m, b)): ps_gather_child of core_kernels.h

python3 scripts/lds_gather_banks.py [draws = 200]"""
import sys

import numpy as np

N, PITCH, LANES, GROUP, BANKS = 1000, 1024, 64, 32, 32
INSTRUCTIONS = 16      # gather instructions per row and generation: 16 children per lane


def gather_child(lane, m, b):
    """ps_gather_child (pansim_amd/csrc/core_kernels.h)"""
    return 4 * (lane + 64 * m) + b


def sorted_parents(rng, weights, n=N):
    """One generation's parents as ps_sim hands them to the sweep: n multinomial draws in ascending order; the cells of the
    row past n gather its first padding byte."""
    p = np.sort(rng.choice(n, size=n, p=weights / weights.sum()))
    return np.concatenate([p, np.full(PITCH - n, min(n, PITCH - 1))])


def instruction_cycles(addr):
    """LDS-array cycles of one wave instruction whose lane l reads byte address addr[l]."""
    cycles = 0
    for g in range(0, LANES, GROUP):
        dwords = np.unique(addr[g:g + GROUP] // 4)
        cycles += int(np.bincount(dwords % BANKS, minlength=BANKS).max())
    return cycles


def children(mapping, i):
    """The child each lane gathers in instruction i (0 .. 15) of a row."""
    lane = np.arange(LANES)
    if mapping == "chunk":
        return 16 * lane + i
    return gather_child(lane, i // 4, i % 4)


def model(weights, draws, mapping, seed=0):
    """(mean cycles per gather instruction, instructions counted) over `draws` generations"""
    rng = np.random.default_rng(seed)
    total = count = 0
    for _ in range(draws):
        parents = sorted_parents(rng, weights)
        for i in range(INSTRUCTIONS):
            total += instruction_cycles(parents[children(mapping, i)])
            count += 1
    return total / count, count


def weight_sets(seed=1):
    rng = np.random.default_rng(seed)
    out = [("uniform", np.ones(N))]
    for sigma in (0.5, 1.0, 2.0):
        out.append(("log-normal, sigma = %.1f" % sigma, np.exp(sigma * rng.standard_normal(N))))
    return out


def main():
    draws = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    print("| parents' weights | chunk (before) | transposed | conflict-free |")
    print("|---|---|---|---|")
    for name, w in weight_sets():
        print("| %s | %.1f | %.1f | %d |" % (name, model(w, draws, "chunk")[0], model(w, draws, "transposed")[0], LANES // GROUP))


if __name__ == "__main__":
    main()
