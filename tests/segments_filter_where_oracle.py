"""The filtered and selected segmented flagstat (fsk_launch_segments_filter_where, csrc/flagstat_segments_filter_where.hip) in
numpy: per segment, the elements counted are those that samtools' view filter -f require -F exclude -q min_mapq passes AND that
the mask (one bool per ELEMENT of the array) selects.

Expected rows never come from the code under test: ``want`` is segments_where_oracle.want (segments_oracle.segmented_counters of
the array with the uncounted flags zeroed, slot 9 from the definition, ``selected`` the per-segment sum of the mask) under
``filter_where_oracle.combined_mask``.  (test_segments_filter_where_host.py checks it against a per-element, per-segment Python
loop and against compacting: oracle.flagstat_c of ``values[b:e][m[b:e]]`` segment by segment.)

``periodic_want`` is the same for arrays x[i] = pattern[(i + phase) % P] with MAPQ bytes q[i] = mapq_pattern[i % R] under masks
m[i] = mask_pattern[i % Q] of any length: the combined mask has the period lcm(P, Q, R) and the array's period divides it, so
segments_where_oracle.periodic_want over that one period gives the rows in O(nseg)."""
import math

import numpy as np

import segments_where_oracle
from filter_where_oracle import combined_mask

MAX_PERIOD = segments_where_oracle.MAX_PERIOD


def want(values, offsets, mask, require: int, exclude: int, mapq=None, min_mapq: int = 0, superset: bool = False):
    """(uint64[nseg, 32] rows, uint64[nseg] counted) of the values that pass the filter and that the mask selects, per segment"""
    return segments_where_oracle.want(values, offsets, combined_mask(values, mask, require, exclude, mapq, min_mapq), superset)


def periodic_want(pattern, offsets, mask_pattern, require: int, exclude: int, mapq_pattern=None, min_mapq: int = 0,
                  superset: bool = False, phase: int = 0):
    """`want` of x[i] = pattern[(i + phase) % P], q[i] = mapq_pattern[i % R] under m[i] = mask_pattern[i % Q], exact at any length"""
    p = np.roll(np.ascontiguousarray(pattern, dtype=np.uint16).ravel(), -int(phase))
    m = np.asarray(mask_pattern, dtype=bool).ravel()
    sizes = [p.size, m.size]
    q = None
    if min_mapq > 0:
        q = np.ascontiguousarray(mapq_pattern, dtype=np.uint8).ravel()
        sizes.append(q.size)
    period = math.lcm(*sizes)
    o = np.asarray(offsets, dtype=np.int64).ravel()
    span = int(o.max()) if o.size else 0
    length = min(period, span)      # co-prime periods multiply: where the joint period is longer than the array, the array itself
    assert length <= MAX_PERIOD, "the joint period of flags, mask and MAPQ (or the array, if shorter) is materialised"
    x = np.resize(p, max(length, 1))
    c = combined_mask(x, np.resize(m, x.size), require, exclude, None if q is None else np.resize(q, x.size), min_mapq)
    if period > span:
        return segments_where_oracle.want(x[:span], o, c[:span], superset)
    return segments_where_oracle.periodic_want(x, o, c, superset)
