"""The core average_distance surface of the C ABI, without a GPU: the new entry point is declared, bound and wrapped, and the
tuning keys that select its forms are documented."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "pansim_hip.h")).read()


def test_multi_average_distance_is_declared_and_bound():
    from pansim_amd import _lib
    assert re.search(r"int ps_multi_average_distance\(ps_multi \*m, int core, double \*out\);", header())
    restype, argtypes = _lib.SIGNATURES["ps_multi_average_distance"]
    assert len(argtypes) == 3
    from pansim_amd.simulation import MultiSimulation
    assert callable(getattr(MultiSimulation, "average_distance", None))


def test_core_davg_tuning_keys_are_documented(pa):
    h = header()
    for key in ("core_davg_form", "core_davg_band"):
        assert '"%s"' % key in h
    known = [pa.load().ps_tuning_key(k) for k in range(64)]
    for key in ("core_davg_form", "core_davg_band"):
        assert key.encode() in known
