"""The filtered flagstat under samtools' whole FLAG predicate (fsk_launch_filter_rf, csrc/flagstat_filter_rf.hip) in numpy: the
mask that ``samtools view -f require -F exclude --rf include_any -G exclude_all -q min_mapq`` selects, and the expected counters
of the values under it.

Expected counters never come from the code under test: ``want_counters`` is where_oracle.want_counters (oracle.flagstat_c of
``values[mask]``, superset slots from oracle.samtools_counts and the definition) under ``view_mask``; ``selected`` is
``int(mask.sum())``."""
import numpy as np

import where_oracle


def view_mask(values, require: int = 0, exclude: int = 0, include_any: int = 0, exclude_all: int = 0, mapq=None,
              min_mapq: int = 0) -> np.ndarray:
    """bool[n]: values[i] has every bit of `require`, no bit of `exclude`, at least one bit of `include_any` (unless that is 0),
    not all bits of `exclude_all` (unless that is 0) and (min_mapq > 0) mapq[i] >= min_mapq"""
    v = np.asarray(values, dtype=np.uint16)
    for m in (require, exclude, include_any, exclude_all):
        assert 0 <= m <= 0xFFFF
    assert 0 <= min_mapq <= 255
    mask = ((v & np.uint16(require)) == np.uint16(require)) & ((v & np.uint16(exclude)) == 0)
    if include_any:
        mask = mask & ((v & np.uint16(include_any)) != 0)
    if exclude_all:
        mask = mask & ((v & np.uint16(exclude_all)) != np.uint16(exclude_all))
    if min_mapq > 0:
        q = np.asarray(mapq, dtype=np.uint8)
        assert q.shape == v.shape
        mask = mask & (q >= min_mapq)
    return mask


def want_counters(oracle_mod, values, require: int = 0, exclude: int = 0, include_any: int = 0, exclude_all: int = 0, mapq=None,
                  min_mapq: int = 0, superset: bool = False):
    """(uint64[32] of the values that pass, how many pass)"""
    mask = view_mask(values, require, exclude, include_any, exclude_all, mapq, min_mapq)
    return where_oracle.want_counters(oracle_mod, values, mask, superset), int(mask.sum())
