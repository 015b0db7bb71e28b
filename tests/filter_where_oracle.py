"""The filtered flagstat under a selection (fsk_launch_filter_where, csrc/flagstat_filter_where.hip) in numpy: the elements
counted are those that samtools' view filter -f require -F exclude -q min_mapq passes AND that the mask selects.

Expected counters never come from the code under test: ``want_counters`` is where_oracle.want_counters (oracle.flagstat_c of
``values[mask]``, superset slots from oracle.samtools_counts and the definition) under ``filter_mask(...) & mask``; ``selected``
is that mask's sum."""
import numpy as np

import where_oracle
from filter_oracle import filter_mask


def combined_mask(values, mask, require: int, exclude: int, mapq=None, min_mapq: int = 0) -> np.ndarray:
    """bool[n]: values[i] passes the filter and mask[i] is set"""
    m = np.asarray(mask, dtype=bool)
    assert m.shape == np.asarray(values).shape
    return filter_mask(values, require, exclude, mapq, min_mapq) & m


def want_counters(oracle_mod, values, mask, require: int, exclude: int, mapq=None, min_mapq: int = 0, superset: bool = False):
    """(uint64[32] of the values counted, how many are counted)"""
    m = combined_mask(values, mask, require, exclude, mapq, min_mapq)
    return where_oracle.want_counters(oracle_mod, values, m, superset), int(m.sum())
