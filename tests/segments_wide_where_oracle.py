"""The selected-elements segmented flagstat of int32 / int64 columns (fsk_launch_segments_wide_where,
csrc/flagstat_segments_wide_where.hip) mirrored in numpy: the expected results, the launcher's geometry, and every selection
address that the kernel's unguarded paths form.

Expected values never come from the code under test.  Rows and ``selected`` are ``segments_where_oracle.want`` of the elements'
low 16 bits; ``high[i]`` is the OR of ``values[b:e][mask[b:e]]`` with the low 16 bits cleared -- of the SELECTED elements of
segment ``i`` only.  (test_segments_wide_where_host.py checks this against compaction: oracle.flagstat_c of
``values[b:e][mask[b:e]] & 0xFFFF`` segment by segment.)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_where_oracle  # noqa: E402
import wide_where_oracle  # noqa: E402
from segments_wide_oracle import UNIT_BYTES, WideWriterSplit  # noqa: E402,F401
from wide_where_oracle import BITMAP, BYTES, UNSIGNED, pack, poison  # noqa: E402,F401  (re-exported for the tests)

UNIT_VECS, ROW_VECS, ROWS, LANES = 512, 64, 8, 64   # kSegUnitVecs, kSegRowVecs, kUnroll, lanes of a wave


def unit_elems(W: int) -> int:
    """U: elements of an 8 KiB unit"""
    return UNIT_BYTES // W


def row_elems(W: int) -> int:
    """R: elements of one row of 64 vectors"""
    return ROW_VECS * 16 // W


def want(values, offsets, mask, superset: bool = False):
    """(uint64[nseg, 32] rows, uint64[nseg] selected, uint64[nseg] high) of ``values`` (a 4-byte or 8-byte integer array) under
    the boolean ``mask`` (one bool per ELEMENT of values), per segment"""
    v = np.ascontiguousarray(values)
    m = np.asarray(mask, dtype=bool).ravel()
    assert v.ndim == 1 and m.size == v.size
    rows, selected = segments_where_oracle.want(wide_where_oracle.low16(v), offsets, m, superset)
    u = v.view(UNSIGNED[v.dtype.itemsize])
    o = np.asarray(offsets, dtype=np.int64).ravel()
    high = np.zeros(max(o.size - 1, 0), dtype=np.uint64)
    low = u.dtype.type(0xFFFF)
    for i in range(o.size - 1):
        b, e = int(o[i]), int(o[i + 1])
        if e > b:
            picked = u[b:e][m[b:e]]
            if picked.size:
                high[i] = np.uint64(np.bitwise_or.reduce(picked & ~low))
    return rows, selected, high


def segments_wide_where_geometry(address: int, m: int, W: int, sel_offset: int, sel_bits: int, grid: int) -> list:
    """what fsk_segments_wide_where_geometry returns in geo[0..8) for m > 0: the segmented launch shape at 8192 / W elements a
    unit (lo0, units, workgroups), the selection base the kernel is handed as an offset from the selection pointer (mod 2^64: it
    may be negative) with the shift (bit q + shift of the base belongs to grid position q), whether the launch is funnelled, then
    the first selection byte that holds an element's bit or byte and one past the last"""
    assert W in (4, 8) and sel_bits in (BITMAP, BYTES) and m > 0
    w = WideWriterSplit(address % 16, m, grid, W)
    if sel_bits == BITMAP:
        bit0 = sel_offset + 8 - w.lo0                     # grid position q is bit q + bit0 - 8
        adjust, shift = (bit0 >> 3) - 1, bit0 & 7
        first, end = sel_offset // 8, (sel_offset + m - 1) // 8 + 1
    else:
        adjust, shift = sel_offset - w.lo0, 0             # grid position q is byte q + sel_offset - lo0
        first, end = sel_offset, sel_offset + m
    return [w.lo0, w.nunits, w.grid, adjust % (1 << 64), shift, int(shift != 0), first, end]


def unguarded_units(geo, m: int, W: int) -> np.ndarray:
    """The grid units that the kernel may load through its unguarded loaders, in the chain regime or as a per-piece unit: those
    that lie wholly inside [lo0, hi0) -- every position of such a unit is an element -- except, in a funnelled launch, GRID UNIT 0,
    which is never chained and always loaded through the guarded loaders."""
    U = unit_elems(W)
    lo0, nunits, funnel = geo[0], geo[1], bool(geo[5])
    hi0 = lo0 + m
    u = np.arange(nunits, dtype=np.int64)
    ok = (u * U >= lo0) & ((u + 1) * U <= hi0)
    if funnel:
        ok &= u != 0
    return u[ok]


def _signed(adjust: int) -> int:
    return adjust - (1 << 64) if adjust >= 1 << 63 else adjust


def unguarded_selection_model(geo, m: int, W: int, sel_bits: int):
    """Every selection address the unguarded paths form, derived from the geometry as the kernel derives it (the header of
    flagstat_segments_wide_where.hip): unit, row, lane -> byte, d, sh.  Returns (q, first, count, d, sh): arrays over every
    (unit, row, lane) of the unguarded units -- q the vector's first grid position, `first` the offset from the selection pointer
    of the first byte the lane loads and `count` how many it loads there (bitmap: 1, or 2 funnelled; bytes: 16 / W), d whether
    the lane's bits straddle two bytes, sh the bit of the loaded word at which its 16 / W bits start."""
    EPV = 16 // W
    base, shift, funnel = _signed(geo[3]), geo[4], bool(geo[5])
    units = unguarded_units(geo, m, W)
    u = np.repeat(units, ROWS * LANES)
    r = np.tile(np.repeat(np.arange(ROWS, dtype=np.int64), LANES), units.size)
    lane = np.tile(np.arange(LANES, dtype=np.int64), units.size * ROWS)
    q = (u * UNIT_VECS + r * ROW_VECS + lane) * EPV
    if sel_bits == BYTES:
        zero = np.zeros_like(q)
        return q, base + q, EPV, zero, zero
    lane_bit = lane * EPV + shift
    d = (((lane_bit & 7) + EPV > 8) & funnel).astype(np.int64)
    k = base + u * (UNIT_VECS * EPV // 8) + r * (ROW_VECS * EPV // 8) + (lane_bit >> 3)
    if funnel:
        return q, k + d - 1, 2, d, (lane_bit & 7) + 8 * (1 - d)
    return q, k, 1, d, lane_bit & 7
