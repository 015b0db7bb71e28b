"""The selected-elements segmented flagstat (fsk_launch_segments_where, csrc/flagstat_segments_where.hip) in numpy.

Expected rows never come from the code under test.  A zero flag counts in no slot, so the rows of the selected flags are
``segments_oracle.segmented_counters`` of the array with the unselected flags set to 0; only the superset slot 9, which counts
every flag that is not QC-fail -- zeroed ones too --, is then replaced by the definition: per segment, the number selected minus
slot 25.  ``selected`` is the per-segment sum of the mask.  (test_segments_where_host.py checks this zeroing against compacting:
oracle.flagstat_c of ``values[b:e][mask[b:e]]`` segment by segment.)

``periodic_want`` is the same for arrays x[i] = pattern[(i + phase) % P] under masks m[i] = mask_pattern[(i + mask_phase) % Q] of
any length: flags and mask together have the period lcm(P, Q), which is materialised once, and the rows follow in O(nseg) from
``segments_oracle.periodic_counters``.

``segments_where_geometry`` mirrors fsk_segments_where_geometry, ``selection_bytes`` (where_oracle's) is the exact set of
selection bytes that a launch over n elements may read."""
import math

import numpy as np

from segments_filter_oracle import segment_sums
from segments_oracle import WriterSplit, periodic_counters, segmented_counters
from where_oracle import BITMAP, BYTES, pack, selection_bytes  # noqa: F401  (re-exported for the tests)

MAX_PERIOD = 1 << 24


def _slot9(rows, selected, superset):
    if superset:
        assert (selected >= rows[:, 25]).all()
        rows[:, 9] = selected - rows[:, 25]
    return rows


def want(values, offsets, mask, superset: bool = False):
    """(uint64[nseg, 32] rows, uint64[nseg] selected) of values under the mask (one bool per ELEMENT of values), per segment"""
    v = np.ascontiguousarray(values, dtype=np.uint16).ravel()
    m = np.asarray(mask, dtype=bool).ravel()
    assert m.size == v.size
    selected = segment_sums(m, offsets)
    rows = segmented_counters(np.where(m, v, np.uint16(0)), offsets, superset)
    return _slot9(rows, selected, superset), selected


def periodic_want(pattern, offsets, mask_pattern, superset: bool = False, phase: int = 0, mask_phase: int = 0):
    """`want` of x[i] = pattern[(i + phase) % P] under m[i] = mask_pattern[(i + mask_phase) % Q], exact at any length"""
    p = np.roll(np.ascontiguousarray(pattern, dtype=np.uint16).ravel(), -int(phase))
    q = np.roll(np.asarray(mask_pattern, dtype=bool).ravel(), -int(mask_phase))
    period = math.lcm(p.size, q.size)
    assert period <= MAX_PERIOD, "the joint period of flags and mask is materialised"
    x, m = np.resize(p, period), np.resize(q, period)
    rows = periodic_counters(np.where(m, x, np.uint16(0)), offsets, superset)
    pre = np.concatenate([[0], np.cumsum(m, dtype=np.int64)])
    o = np.asarray(offsets, dtype=np.int64).ravel()

    def upto(t):
        return (t // period) * pre[-1] + pre[t % period]

    selected = np.where(o[1:] > o[:-1], upto(o[1:]) - upto(o[:-1]), 0).astype(np.uint64)
    return _slot9(rows, selected, superset), selected


def segments_where_geometry(address: int, m: int, sel_offset: int, sel_bits: int, grid: int) -> list:
    """what fsk_segments_where_geometry returns in geo[0..7) for m > 0: the segmented launch shape (lo0, units, workgroups), the
    selection base the kernel is handed as an offset from the selection pointer (mod 2^64: it may be -1) with the bit at which a
    grid vector's 8 bits start in its byte, then the first selection byte that holds an element's bit or byte and one past the
    last"""
    assert sel_bits in (BITMAP, BYTES) and m > 0
    w = WriterSplit(address % 16, m, grid)
    if sel_bits == BITMAP:
        bit0 = sel_offset + 8 - w.lo0                     # grid position q is bit q + bit0 - 8
        adjust, shift = (bit0 >> 3) - 1, bit0 & 7
        first, end = sel_offset // 8, (sel_offset + m - 1) // 8 + 1
    else:
        adjust, shift = sel_offset - w.lo0, 0             # grid position q is byte q + sel_offset - lo0
        first, end = sel_offset, sel_offset + m
    return [w.lo0, w.nunits, w.grid, adjust % (1 << 64), shift, first, end]
