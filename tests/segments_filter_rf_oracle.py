"""The filtered segmented flagstat under samtools' whole FLAG predicate (fsk_launch_segments_filter_rf,
csrc/flagstat_segments_filter_rf.hip) in numpy.

Expected rows never come from the code under test.  A zero flag counts in no slot, so the rows of the flags that pass are
``segments_oracle.segmented_counters`` of the array with the failing flags zeroed (``filter_rf_oracle.view_mask`` says which fail:
-f require, -F exclude, --rf include_any, -G exclude_all, -q min_mapq); only the superset slot 9, which counts every flag that is
not QC-fail -- zeroed ones too --, is then replaced by the definition: per segment, the number that pass minus slot 25.
``selected`` is the per-segment sum of the mask (``segments_filter_oracle.segment_sums``).

``periodic_want`` is the same for arrays x[i] = pattern[(i + phase) % P], mapq[i] = mq_pattern[(i + phase) % P] of any length, in
O(P + nseg): ``segments_oracle.periodic_counters`` of the masked pattern, and a prefix count of the pass pattern."""
import numpy as np

from filter_rf_oracle import view_mask
from segments_filter_oracle import segment_sums
from segments_oracle import periodic_counters, segmented_counters


# The predicates of the tests, as (require, exclude, include_any, exclude_all).  TABLE: what the reduction makes of each -- its
# answer (0 nothing passes, 1 a plain pair, 2 a residue) and, for a plain pair, the pair -- worked out by hand from the rules at
# the reduction's declaration; tests/test_segments_filter_rf_host.py pins them against the library.
TABLE = (
    ((0, 0x904, 0x50, 0), 2, None),
    ((0, 0x904, 0, 0x420), 2, None),
    ((0, 0x904, 0x210, 0x480), 2, None),
    ((0x1, 0x804, 0x110, 0x2200), 2, None),
    ((0, 0, 0x0101, 0x8080), 2, None),
    ((0, 0, 0xFFFF, 0xFFFF), 2, None),
    ((0, 0x904, 0x40, 0), 1, (0x40, 0x904)),
    ((0, 0x904, 0, 0xC), 1, (0, 0x904)),
    ((0, 0x904, 0x900, 0), 0, None),
    ((0x3, 0, 0, 0x3), 0, None),
    ((0x40, 0x40, 0x50, 0), 0, None),
)
# every mask of two bits: both in the low byte plane, both in the high one, one in each
TWO_BITS = tuple((1 << i) | (1 << j) for i in range(16) for j in range(i + 1, 16))
PREDICATES = (tuple((0, 0, m, 0) for m in TWO_BITS) + tuple((0, 0, 0, m) for m in TWO_BITS) + tuple(p for p, _, _ in TABLE))
RESIDUES = tuple((0, 0, m, 0) for m in TWO_BITS) + tuple((0, 0, 0, m) for m in TWO_BITS) + tuple(p for p, kind, _ in TABLE if kind == 2)


def every_value_input():
    """(values, offsets): 0..65535 once each, shuffled (16 units of the kernel), cut into segments of lengths without a common
    factor with the vector, the row or the unit, some of them empty, with a gap in front and behind"""
    n = 65536
    values = np.random.RandomState(2027).permutation(n).astype(np.uint16)
    lengths = (7, 11, 13, 0, 4099, 1, 509, 8191, 17, 0, 0, 3, 1021, 64, 4096, 19)
    o = [2]
    i = 0
    while o[-1] < n - 5:
        o.append(min(o[-1] + lengths[i % len(lengths)], n - 5))
        i += 1
    return values, np.array(o, dtype=np.int64)


def _slot9(rows, selected, superset):
    if superset:
        assert (selected >= rows[:, 25]).all()
        rows[:, 9] = selected - rows[:, 25]
    return rows


def want(values, offsets, require: int = 0, exclude: int = 0, include_any: int = 0, exclude_all: int = 0, mapq=None,
         min_mapq: int = 0, superset: bool = False):
    """(uint64[nseg, 32] rows, uint64[nseg] selected) of values under the predicate, per segment"""
    v = np.ascontiguousarray(values, dtype=np.uint16).ravel()
    mask = view_mask(v, require, exclude, include_any, exclude_all, mapq, min_mapq)
    selected = segment_sums(mask, offsets)
    rows = segmented_counters(np.where(mask, v, np.uint16(0)), offsets, superset)
    return _slot9(rows, selected, superset), selected


def periodic_want(pattern, offsets, require: int = 0, exclude: int = 0, include_any: int = 0, exclude_all: int = 0, mq_pattern=None,
                  min_mapq: int = 0, superset: bool = False, phase: int = 0):
    """`want` of the periodic array and column (one period P for both), exact at any length"""
    p = np.ascontiguousarray(pattern, dtype=np.uint16).ravel()
    if mq_pattern is not None:
        assert np.asarray(mq_pattern).size == p.size
    mask = view_mask(p, require, exclude, include_any, exclude_all, mq_pattern, min_mapq)
    rows = periodic_counters(np.where(mask, p, np.uint16(0)), offsets, superset, phase)
    period = p.size
    pre = np.concatenate([[0], np.cumsum(np.roll(mask, -int(phase)), dtype=np.int64)])
    o = np.asarray(offsets, dtype=np.int64).ravel()

    def upto(t):
        return (t // period) * pre[-1] + pre[t % period]

    selected = np.where(o[1:] > o[:-1], upto(o[1:]) - upto(o[:-1]), 0).astype(np.uint64)
    return _slot9(rows, selected, superset), selected
