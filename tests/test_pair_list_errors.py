"""The pair-list checks that the host restatements share (pansim_amd/csrc/pair_readout.h), without a device: one table of bad
lists of 3 pairs of 3 individuals through ps_clusters_from_counts, ps_tree_from_counts, ps_upgma_from_counts and
ps_neighbours_from_counts, and through ps_histogram_from_counts where a case applies to it.  Every message is the literal text
the library gave before the checks were shared."""
import ctypes as C

import numpy as np
import pytest

PS_ERR_INVALID = -1
ACC, BAD_METRIC = 1, 7
OK = None                       # (the list is accepted)
ENTRIES = ("clusters", "tree", "upgma", "neighbours", "histogram")
NOUN = {"tree": "a linkage tree is PS_TREE_CORE (0) or PS_TREE_ACC (1)", "upgma": "a UPGMA tree is PS_TREE_CORE (0) or PS_TREE_ACC (1)",
        "neighbours": "nearest neighbours is PS_KNN_CORE (0) or PS_KNN_ACC (1)"}


def arr(*v):
    return np.array(v, np.uint32)


BASE = dict(r1=arr(0, 1, 0), r2=arr(1, 2, 2), h=arr(4, 6, 2), i=arr(1, 2, 0), u=arr(3, 2, 5), metric=ACC)
NEEDS = "null argument: the metric needs its numerators"
# (name, what differs from BASE, the message per entry: one text for all that have indices, or a dict; an entry left out of a
# dict does not have the case)
CASES = [
    ("index equal to pop_size", dict(r2=arr(1, 3, 2)), "pair 1: index 3 is not below pop_size 3"),
    ("equal indices", dict(r2=arr(1, 1, 2)), "pair 1: both indices are 1"),
    ("intersection above union", dict(i=arr(1, 3, 0)), dict.fromkeys(ENTRIES, "pair 1: intersection 3 above union 2")),
    ("union 65536", dict(u=arr(3, 65536, 5)),
     dict(dict.fromkeys(("tree", "upgma", "neighbours"), "pair 1: union 65536 above the limit of 65535 accessory genes"), clusters=OK, histogram=OK)),
    ("missing numerators", dict(i=None),
     dict(dict.fromkeys(("tree", "upgma", "neighbours"), NEEDS), clusters="null argument: an active criterion needs its numerators",
          histogram="null argument")),
    ("bad metric", dict(metric=BAD_METRIC), {e: "the metric of %s, not 7" % NOUN[e] for e in NOUN}),
    # two faults in one list: the earlier pair's is the one reported, whichever check it fails
    ("an index behind an intersection", dict(i=arr(4, 2, 0), r2=arr(1, 2, 3)),
     dict.fromkeys(ENTRIES[:4], "pair 0: intersection 4 above union 3")),
    ("an intersection behind equal indices", dict(r1=arr(1, 1, 0), i=arr(1, 3, 0)), "pair 0: both indices are 1"),
    ("a union behind an index", dict(r1=arr(0, 5, 0), u=arr(3, 2, 70000)), "pair 1: index 5 is not below pop_size 3"),
    # ... and of two kinds of fault the parameters win over the numerators, the numerators over the pairs
    ("bad metric, missing numerators and a bad index", dict(metric=BAD_METRIC, i=None, r2=arr(1, 3, 2)),
     {e: "the metric of %s, not 7" % NOUN[e] for e in NOUN}),
    ("missing numerators and a bad index", dict(u=None, r2=arr(1, 3, 2)),
     dict(dict.fromkeys(("tree", "upgma", "neighbours"), NEEDS), clusters="null argument: an active criterion needs its numerators")),
]


def call(pa, entry, a):
    """the entry over the list `a` -> its return code"""
    lib, L = pa.load(), pa._lib
    ptr = lambda x: None if x is None else x.ctypes.data
    u32, u64 = (lambda n: np.zeros(n, np.uint32)), (lambda n: np.zeros(n, np.uint64))
    nums = [ptr(a[k]) for k in ("h", "i", "u")]
    head = [ptr(a["r1"]), ptr(a["r2"])] + nums + [3, 3, 10, 1]
    keep = []                   # (the output arrays stay alive across the call)

    def outs(*arrays):
        keep.extend(arrays)
        return [ptr(x) for x in arrays]

    if entry == "histogram":
        prm, out = L.PairHistParams(4, 4, 0), L.PairHist()
        return lib.ps_histogram_from_counts(*nums, 3, 10, 1, C.byref(prm), C.byref(out), *outs(u64(16)))
    if entry == "clusters":      # (both criteria active: the counterpart of a metric that reads the accessory numerators)
        prm, out = L.ClusterParams(5, 1, 2), L.Clusters()
        return lib.ps_clusters_from_counts(*head, C.byref(prm), C.byref(out), *outs(u32(3)))
    if entry == "tree":
        prm, out = L.TreeParams(a["metric"]), L.Tree()
        return lib.ps_tree_from_counts(*head, C.byref(prm), C.byref(out), *outs(u32(3), u32(3), u64(3), u64(3)))
    if entry == "upgma":
        prm, out = L.TreeParams(a["metric"]), L.Upgma()
        return lib.ps_upgma_from_counts(*head, C.byref(prm), C.byref(out), *outs(u32(3), u32(3), u32(3), u64(3), u64(3)))
    prm, out = L.KnnParams(a["metric"], 1), L.Knn()
    return lib.ps_neighbours_from_counts(*head, C.byref(prm), C.byref(out), *outs(u32(3), u64(3), u64(3)))


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_base_list_is_accepted(pa, entry):
    assert call(pa, entry, BASE) == 0, pa.load().ps_last_error().decode()


@pytest.mark.parametrize("name,change,want", CASES, ids=[c[0] for c in CASES])
def test_bad_lists(pa, name, change, want):
    lib = pa.load()
    if not isinstance(want, dict):
        want = dict.fromkeys(ENTRIES[:4], want)
    assert want, name
    for entry, text in want.items():
        rc = call(pa, entry, dict(BASE, **change))
        if text is OK:
            assert rc == 0, (entry, lib.ps_last_error().decode())
        else:
            assert rc == PS_ERR_INVALID, (entry, rc)
            assert lib.ps_last_error().decode() == text, entry
