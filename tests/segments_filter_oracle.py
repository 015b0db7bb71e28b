"""The filtered segmented flagstat (fsk_launch_segments_filter, csrc/flagstat_segments_filter.hip) in numpy.

Expected rows never come from the code under test.  A zero flag counts in no slot, so the rows of the flags that pass are
``segments_oracle.segmented_counters`` of the array with the failing flags zeroed (``filter_oracle.filter_mask`` says which fail);
only the superset slot 9, which counts every flag that is not QC-fail -- zeroed ones too --, is then replaced by the definition:
per segment, the number that pass minus slot 25.  ``selected`` is the per-segment sum of the mask.

``periodic_want`` is the same for arrays x[i] = pattern[(i + phase) % P], mapq[i] = mq_pattern[(i + phase) % P] of any length, in
O(P + nseg): ``segments_oracle.periodic_counters`` of the masked pattern, and a prefix count of the pass pattern."""
import numpy as np

from filter_oracle import filter_mask
from segments_oracle import periodic_counters, segmented_counters


def segment_sums(mask, offsets) -> np.ndarray:
    """uint64[nseg]: how many of mask[offsets[i]:offsets[i+1]] are set"""
    o = np.asarray(offsets, dtype=np.int64).ravel()
    pre = np.concatenate([[0], np.cumsum(np.asarray(mask, dtype=bool), dtype=np.int64)])
    return np.where(o[1:] > o[:-1], pre[o[1:]] - pre[o[:-1]], 0).astype(np.uint64)


def _slot9(rows, selected, superset):
    if superset:
        assert (selected >= rows[:, 25]).all()
        rows[:, 9] = selected - rows[:, 25]
    return rows


def want(values, offsets, require: int, exclude: int, mapq=None, min_mapq: int = 0, superset: bool = False):
    """(uint64[nseg, 32] rows, uint64[nseg] selected) of values under the predicate, per segment"""
    v = np.ascontiguousarray(values, dtype=np.uint16).ravel()
    mask = filter_mask(v, require, exclude, mapq, min_mapq)
    selected = segment_sums(mask, offsets)
    rows = segmented_counters(np.where(mask, v, np.uint16(0)), offsets, superset)
    return _slot9(rows, selected, superset), selected


def periodic_want(pattern, offsets, require: int, exclude: int, mq_pattern=None, min_mapq: int = 0, superset: bool = False,
                  phase: int = 0):
    """`want` of the periodic array and column (one period P for both), exact at any length"""
    p = np.ascontiguousarray(pattern, dtype=np.uint16).ravel()
    if mq_pattern is not None:
        assert np.asarray(mq_pattern).size == p.size
    mask = filter_mask(p, require, exclude, mq_pattern, min_mapq)
    rows = periodic_counters(np.where(mask, p, np.uint16(0)), offsets, superset, phase)
    period = p.size
    pre = np.concatenate([[0], np.cumsum(np.roll(mask, -int(phase)), dtype=np.int64)])
    o = np.asarray(offsets, dtype=np.int64).ravel()

    def upto(t):
        return (t // period) * pre[-1] + pre[t % period]

    selected = np.where(o[1:] > o[:-1], upto(o[1:]) - upto(o[:-1]), 0).astype(np.uint64)
    return _slot9(rows, selected, superset), selected
