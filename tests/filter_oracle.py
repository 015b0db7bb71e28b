"""The filtered flagstat (fsk_launch_filter, csrc/flagstat_filter.hip) in numpy: the mask samtools' view filter -f require
-F exclude -q min_mapq selects, and the expected counters of the values under it.

Expected counters never come from the code under test: ``want_counters`` is where_oracle.want_counters (oracle.flagstat_c of
``values[mask]``, superset slots from oracle.samtools_counts and the definition) under ``filter_mask``; ``selected`` is
``int(mask.sum())``."""
import numpy as np

import where_oracle


def filter_mask(values, require: int, exclude: int, mapq=None, min_mapq: int = 0) -> np.ndarray:
    """bool[n]: values[i] has every bit of `require`, no bit of `exclude` and (min_mapq > 0) mapq[i] >= min_mapq"""
    v = np.asarray(values, dtype=np.uint16)
    assert 0 <= require <= 0xFFFF and 0 <= exclude <= 0xFFFF and 0 <= min_mapq <= 255
    mask = ((v & np.uint16(require)) == np.uint16(require)) & ((v & np.uint16(exclude)) == 0)
    if min_mapq > 0:
        q = np.asarray(mapq, dtype=np.uint8)
        assert q.shape == v.shape
        mask = mask & (q >= min_mapq)
    return mask


def want_counters(oracle_mod, values, require: int, exclude: int, mapq=None, min_mapq: int = 0, superset: bool = False):
    """(uint64[32] of the values that pass, how many pass)"""
    mask = filter_mask(values, require, exclude, mapq, min_mapq)
    return where_oracle.want_counters(oracle_mod, values, mask, superset), int(mask.sum())
