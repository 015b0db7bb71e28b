"""The filtered wide-input flagstat (fsk_launch_wide_filter, csrc/flagstat_wide_filter.hip) in numpy: what a call over a column
of 4-byte or 8-byte integers must report.

Expected values never come from the code under test: the counters are filter_oracle.want_counters (oracle.flagstat_c of
``values[mask]``, superset slots from oracle.samtools_counts and the definition) of the low 16 bits of the column, ``selected`` is
``int(mask.sum())`` and ``high`` is the OR of ``element & ~0xFFFF`` over ALL elements, whatever the predicate says about them."""
import numpy as np

import filter_oracle

UNSIGNED = {2: np.uint16, 4: np.uint32, 8: np.uint64}
ALL_HIGH = {2: 0, 4: 0xFFFF0000, 8: 0xFFFFFFFFFFFF0000}


def low16(values) -> np.ndarray:
    v = np.ascontiguousarray(values)
    return (v.view(UNSIGNED[v.dtype.itemsize]) & UNSIGNED[v.dtype.itemsize](0xFFFF)).astype(np.uint16)


def want_high(values) -> int:
    v = np.ascontiguousarray(values)
    if v.size == 0:
        return 0
    W = v.dtype.itemsize
    return int(np.bitwise_or.reduce(v.view(UNSIGNED[W]) & UNSIGNED[W](ALL_HIGH[W])))


def want(oracle_mod, values, require: int, exclude: int, mapq=None, min_mapq: int = 0, superset: bool = False):
    """(uint64[32] of the low 16 bits of the elements that pass, how many pass, the mask of all elements)"""
    counters, selected = filter_oracle.want_counters(oracle_mod, low16(values), require, exclude, mapq, min_mapq, superset)
    return counters, selected, want_high(values)
