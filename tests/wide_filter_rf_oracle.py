"""The filtered wide-input flagstat under samtools' whole FLAG predicate (fsk_launch_wide_filter_rf,
csrc/flagstat_wide_filter_rf.hip) in numpy: what a call over a column of 4-byte or 8-byte integers must report.

Expected values never come from the code under test: the counters and ``selected`` are filter_rf_oracle.want_counters
(oracle.flagstat_c of ``values[mask]``, superset slots from oracle.samtools_counts and the definition) of the low 16 bits of the
column.  ``high`` is the OR of ``element & ~0xFFFF`` over ALL elements, whatever the predicate says about them -- unless no FLAG
value at all satisfies the FLAG part of the predicate: such a call reads no element and its ``high`` is 0.  Whether one does is
found by trying all 65,536 values, not by the library's reduction of the masks."""
import numpy as np

import filter_rf_oracle
from wide_filter_oracle import ALL_HIGH, UNSIGNED, low16, want_high  # noqa: F401  (re-exported for the tests)

_EVERY_FLAG = np.arange(65536, dtype=np.uint32).astype(np.uint16)
_SATISFIABLE = {}


def satisfiable(require: int, exclude: int, include_any: int, exclude_all: int) -> bool:
    """some 16-bit value passes the FLAG part of the predicate: brute force over all of them"""
    key = (require, exclude, include_any, exclude_all)
    if key not in _SATISFIABLE:
        _SATISFIABLE[key] = bool(filter_rf_oracle.view_mask(_EVERY_FLAG, require, exclude, include_any, exclude_all).any())
    return _SATISFIABLE[key]


def want(oracle_mod, values, require: int = 0, exclude: int = 0, include_any: int = 0, exclude_all: int = 0, mapq=None,
         min_mapq: int = 0, superset: bool = False):
    """(uint64[32] of the low 16 bits of the elements that pass, how many pass, the mask of all elements -- 0 when the FLAG part
    can pass nothing)"""
    counters, selected = filter_rf_oracle.want_counters(oracle_mod, low16(values), require, exclude, include_any, exclude_all, mapq,
                                                        min_mapq, superset)
    high = want_high(values) if satisfiable(require, exclude, include_any, exclude_all) else 0
    return counters, selected, high
