"""numpy oracle of the segmented flagstat over 4-byte and 8-byte elements (libflagstats_amd/segments_wide.py,
csrc/flagstat_segments_wide.hip): per CSR segment the rows of the elements' low 16 bits (segments_oracle.segmented_counters) and
the OR of the bits above bit 15, a periodic form of both in O(P + nseg), and the kernel's writer split at 8192 / W elements a
unit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from segments_oracle import SEG_EPOCH, SEG_WAVES_PER_BLOCK, periodic_counters, segmented_counters  # noqa: E402,F401

UNIT_BYTES = 8192         # kSegWideUnitBytes
HIGH = ~np.uint64(0xFFFF)


def unsigned(x) -> np.ndarray:
    """the elements as unsigned integers of their own width, widened to uint64"""
    x = np.ascontiguousarray(x)
    assert x.dtype.kind in "iu" and x.dtype.itemsize in (4, 8), x.dtype
    return x.view(np.uint32 if x.dtype.itemsize == 4 else np.uint64).astype(np.uint64)


def low16(x) -> np.ndarray:
    return (unsigned(x) & np.uint64(0xFFFF)).astype(np.uint16)


def segmented_high(x, offsets) -> np.ndarray:
    """uint64[nseg]: high[i] = OR of (element & ~0xFFFF), as unsigned, over x[offsets[i]:offsets[i+1]]; 0 for an empty segment"""
    u = unsigned(x) & HIGH
    o = np.asarray(offsets, dtype=np.int64).ravel()
    out = np.zeros(max(o.size - 1, 0), dtype=np.uint64)
    for i in range(o.size - 1):
        if o[i + 1] > o[i]:
            out[i] = np.bitwise_or.reduce(u[o[i]:o[i + 1]])
    return out


def want(x, offsets, superset: bool = False):
    """(uint64[nseg, 32] rows, uint64[nseg] high) of the array x"""
    return segmented_counters(low16(x), offsets, superset), segmented_high(x, offsets)


def periodic_want(pattern, offsets, superset: bool = False, phase: int = 0):
    """rows and masks of x[i] = pattern[(i + phase) % P] for any offsets in O(64 * P + nseg): per bit above bit 15, the number of
    elements that carry it over [0, t) is (t // P) * (count over one period) + (count over the period's first t % P)"""
    rows = periodic_counters(low16(pattern), offsets, superset, phase)
    p = np.roll(unsigned(pattern), -int(phase))
    period = p.size
    o = np.asarray(offsets, dtype=np.int64).ravel()
    high = np.zeros(max(o.size - 1, 0), dtype=np.uint64)
    if o.size < 2:
        return rows, high
    nonempty = o[1:] > o[:-1]
    for bit in range(16, 64):
        m = (p >> np.uint64(bit)) & np.uint64(1)
        if not m.any():
            continue
        pre = np.concatenate([[0], np.cumsum(m, dtype=np.int64)])

        def upto(t):
            return (t // period) * pre[-1] + pre[t % period]

        has = nonempty & (upto(o[1:]) - upto(o[:-1]) > 0)
        high |= np.where(has, np.uint64(1) << np.uint64(bit), np.uint64(0)).astype(np.uint64)
    return rows, high


class WideWriterSplit:
    """The writers (waves) of one fsk_launch_segments_wide over ``n`` elements of ``W`` bytes whose first element lies
    ``addr_mod_16`` bytes past a 16-byte boundary: segments_oracle.WriterSplit at ``unit`` = 8192 / W elements.  ``begin[w]``,
    ``end[w]``: writer w's elements as indices into the launched array; unit boundaries lie at indices ``k * unit - lo0``."""

    def __init__(self, addr_mod_16: int, n: int, grid_blocks: int, W: int):
        assert W in (4, 8) and addr_mod_16 % W == 0 and n > 0 and grid_blocks > 0
        self.W = W
        self.unit = UNIT_BYTES // W
        self.lo0 = (addr_mod_16 % 16) // W
        hi0 = self.lo0 + n
        self.n = n
        self.nunits = (hi0 + self.unit - 1) // self.unit
        want_blocks = (self.nunits + 3) // 4                    # one unit per wave at least
        self.grid = min(want_blocks, grid_blocks)
        self.waves = SEG_WAVES_PER_BLOCK * self.grid
        gw = np.arange(self.waves, dtype=np.int64)
        self.u_begin = gw * self.nunits // self.waves
        self.u_end = (gw + 1) * self.nunits // self.waves
        p0 = np.maximum(self.u_begin * self.unit, self.lo0)
        e = np.maximum(np.minimum(self.u_end * self.unit, hi0), self.lo0)
        self.begin = np.minimum(p0, e) - self.lo0
        self.end = e - self.lo0

    def seams(self) -> np.ndarray:
        live = self.end > self.begin
        return self.end[live][:-1]

    def pieces(self, offsets, min_units: int = 2) -> dict:
        """every (writer, segment) piece: writer, seg, b, e, chain (whole units through the chain, 0: counted per piece only),
        plain (the store form stores row and mask plainly), head, tail (elements counted per piece around the chain run)"""
        U = self.unit
        o = np.clip(np.asarray(offsets, dtype=np.int64).ravel(), 0, self.n)
        sb, se = o[:-1], o[1:]
        cols = {k: [] for k in ("writer", "seg", "b", "e", "chain", "plain", "head", "tail")}
        for w in range(self.waves):
            p0, E = int(self.begin[w]), int(self.end[w])
            if p0 >= E:
                continue
            s = np.nonzero((se > sb) & (se > p0) & (sb < E))[0]
            b, e = np.maximum(sb[s], p0), np.minimum(se[s], E)
            g0 = -(-(b + self.lo0) // U) * U                    # first unit boundary in the piece (grid position)
            k = np.maximum((e + self.lo0 - g0) // U, 0)
            k = np.where((k >= min_units) & (k > 0), k, 0)
            cols["writer"].append(np.full(s.size, w))
            cols["seg"].append(s)
            cols["b"].append(b)
            cols["e"].append(e)
            cols["chain"].append(k)
            cols["plain"].append((sb[s] >= p0) & (se[s] <= E))
            cols["head"].append(np.where(k > 0, g0 - self.lo0 - b, e - b))
            cols["tail"].append(np.where(k > 0, e - (g0 - self.lo0 + k * U), 0))
        return {k: (np.concatenate(v) if v else np.zeros(0, dtype=np.int64)) for k, v in cols.items()}


def writer_ranges(addr_mod_16: int, n: int, grid_blocks: int, W: int) -> WideWriterSplit:
    return WideWriterSplit(addr_mod_16, n, grid_blocks, W)
