"""Isolate samples over the C ABI (docs/ISOLATE_SAMPLES.md): some rows of one or more populations as a new Population on the
device, to which every read-out applies unchanged, and the recorded genealogy restricted to a sample.

All computation happens in the HIP library; this module only marshals buffers.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .population import Population, _ptr, _u32


def _rows(rows):
    """a row list as flat uint32, None = all rows"""
    return None if rows is None else _u32(rows).reshape(-1)


def _wrap(like, handle, size, ncols=None, global_cols=None):
    """the owned Population around a handle a ps_*_subset / ps_population_pool call made: `size` rows, the other attributes those
    of `like`"""
    ncols = like.ncols if ncols is None else int(ncols)
    return Population(int(size), ncols, 4 if like.core else 2, like.core, 0.0, like.seed, like.core_genes,
                      global_cols=like.global_cols if global_cols is None else int(global_cols), _handle=handle.value, _owned=True)


def pool(parts, rows=None):
    """the rows `rows[k]` of every Population `parts[k]` (None, or a None entry: all of them), stacked in this order into a new
    Population on the device (ps_population_pool): rows are numbered as every read-out of the part numbers them and may repeat;
    the parts are all core or all accessory matrices of the same columns on one device, and may repeat too"""
    parts = list(parts)
    if rows is None:
        rows = [None] * len(parts)
    lists = [_rows(r) for r in rows]
    if len(lists) != len(parts):
        raise ValueError("one row list (or None) per part")
    if any(not isinstance(p, Population) for p in parts):
        raise TypeError("the parts of a pool are Population objects")
    K = len(parts)
    handles = (C.c_void_p * max(1, K))(*[p._h.value for p in parts])
    ptrs = (C.c_void_p * max(1, K))(*[None if r is None else r.ctypes.data for r in lists])
    n = np.array([p.size if r is None else r.size for p, r in zip(parts, lists)] + [0] * (K == 0), np.uint64)
    h = C.c_void_p()
    check(_lib.load().ps_population_pool(handles, ptrs, _ptr(n), K, C.byref(h)))
    return _wrap(parts[0], h, int(n.sum()))


def _run_subset(fn, run, rows):
    """fn(handle, rows, n, &core, &acc) -> (core, acc), the two samples of a run as owned Populations"""
    r = _rows(rows)
    n = run.params.pop_size if r is None else r.size
    core, acc = C.c_void_p(), C.c_void_p()
    check(fn(run._h, _ptr(r), n, C.byref(core), C.byref(acc)))
    first = run._timed                      # (the Simulation whose two Populations the samples are shaped like)
    return (_wrap(first.core_genome, core, n, ncols=run._core_width), _wrap(first.pan_genome, acc, n))


def genealogy_restrict(order, coal, rows):
    """the comb (order, coal) restricted to `rows` (ps_genealogy_restrict; host only) -> (order, coal) of the sample:
    order[q] is an INDEX into `rows`, the row of the sample handle `subset(rows)` makes"""
    order, coal, rows = _u32(order), _u32(coal), _u32(rows).reshape(-1)
    order_out, coal_out = np.zeros(max(1, rows.size), np.uint32), np.zeros(max(1, rows.size), np.uint32)
    check(_lib.load().ps_genealogy_restrict(_ptr(order), _ptr(coal), order.size, _ptr(rows), rows.size, _ptr(order_out), _ptr(coal_out)))
    return order_out[:rows.size], coal_out[:max(0, rows.size - 1)]


__all__ = ["genealogy_restrict", "pool"]
