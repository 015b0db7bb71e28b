"""The filtered segmented flagstat over 4-byte and 8-byte elements (fsk_launch_segments_wide_filter,
csrc/flagstat_segments_wide_filter.hip) in numpy, composed of the oracles of its parents.

Expected values never come from the code under test.  Rows and ``selected`` are ``segments_filter_oracle.want`` of the low 16 bits
of the column (the failing elements zeroed, superset slot 9 replaced by the passing count minus slot 25; ``selected`` the
per-segment sum of the pass vector); ``high`` is ``segments_wide_oracle.segmented_high`` of the UNFILTERED column: the mask covers
every element of a segment, passing or not.  An overlapping require / exclude pair reads no element: its masks are 0.

``periodic_want`` is the same for x[i] = pattern[(i + phase) % P], mapq[i] = mq_pattern[(i + phase) % Q] of any length: the two are
brought to one joint period lcm(P, Q) (coprime prime periods give P * Q) and handed to the parents' periodic forms."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_filter_oracle as sfo  # noqa: E402
import segments_wide_oracle as swo  # noqa: E402
from filter_oracle import filter_mask  # noqa: E402
from segments_wide_oracle import UNIT_BYTES, SEG_EPOCH, WideWriterSplit, low16, unsigned, writer_ranges  # noqa: E402,F401


def pass_vector(x, require: int, exclude: int, mapq=None, min_mapq: int = 0) -> np.ndarray:
    """bool[n]: which elements of x pass (the predicate sees the low 16 bits)"""
    return filter_mask(low16(x), require, exclude, mapq, min_mapq)


def want(x, offsets, require: int, exclude: int, mapq=None, min_mapq: int = 0, superset: bool = False):
    """(uint64[nseg, 32] rows, uint64[nseg] selected, uint64[nseg] high) of the column x under the predicate, per segment"""
    rows, selected = sfo.want(low16(x), offsets, require, exclude, mapq, min_mapq, superset)
    high = swo.segmented_high(x, offsets)
    if require & exclude:
        high = np.zeros_like(high)   # nothing is launched, no element is read
    return rows, selected, high


def periodic_want(pattern, offsets, require: int, exclude: int, mq_pattern=None, min_mapq: int = 0, superset: bool = False,
                  phase: int = 0):
    """`want` of the periodic column and MAPQ column, exact at any length, in O(lcm(P, Q) + nseg)"""
    p = np.ascontiguousarray(pattern)
    if mq_pattern is None:
        joint, mq = p, None
    else:
        q = np.ascontiguousarray(mq_pattern, dtype=np.uint8)
        period = int(np.lcm(p.size, q.size))
        joint, mq = np.resize(p, period), np.resize(q, period)
    rows, selected = sfo.periodic_want(low16(joint), offsets, require, exclude, mq, min_mapq, superset, phase)
    _, high = swo.periodic_want(joint, offsets, False, phase)
    if require & exclude:
        high = np.zeros_like(high)
    return rows, selected, high
