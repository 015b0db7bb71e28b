"""Segmented counterpart of ``oracle.flagstat_numpy`` for the segmented-flagstat tests: the same per-flag rule
(libflagstats.h:118-142), summed per CSR segment with ``np.add.reduceat``."""
import numpy as np


def slot_indicators(x: np.ndarray, superset: bool = False):
    """{slot: bool[n]} -- which flags add 1 to which slot."""
    bit = lambda m: (x & np.uint16(m)) != 0  # noqa: E731
    qc = bit(512)
    sec = bit(256)
    sup = bit(2048) & ~sec
    pp = bit(1) & ~sec & ~bit(2048)
    unm, mun = bit(4), bit(8)
    per_class = {2: unm, 6: pp & bit(64), 7: pp & bit(128), 8: sec, 10: bit(1024), 11: sup,
                 12: pp & bit(2) & ~unm, 13: pp & mun & ~unm, 14: pp & ~mun & ~unm}
    if superset:
        per_class[0] = pp
    ind = {}
    for slot, m in per_class.items():
        ind[slot] = m & ~qc
        ind[16 + slot] = m & qc
    ind[25] = qc
    if superset:
        ind[9] = ~qc     # pass-QC reads = length - slot 25
    return ind


def segmented_counters(values, offsets, superset: bool = False) -> np.ndarray:
    """uint64[nseg, 32]: row i = counters of values[offsets[i]:offsets[i+1]]."""
    x = np.ascontiguousarray(values, dtype=np.uint16).ravel()
    o = np.asarray(offsets, dtype=np.int64).ravel()
    nseg = o.size - 1
    out = np.zeros((nseg, 32), dtype=np.uint64)
    nonempty = o[1:] > o[:-1]
    if nseg <= 0 or not nonempty.any():
        return out
    # reduceat gives the element itself (not 0) for an empty index range and rejects an index equal to len(x): sum only the
    # non-empty segments (consecutive in memory: the empty ones between them have no flags), and close the last one with a
    # sentinel index unless it ends at the array's end
    idx = o[:-1][nonempty]
    end = int(o[-1])
    if end < x.size:
        idx = np.append(idx, end)
    for slot, m in slot_indicators(x, superset).items():
        sums = np.add.reduceat(m.astype(np.uint64), idx)
        out[nonempty, slot] = sums[:nonempty.sum()]
    return out


def segmented_counters_many(values, offsets_list, superset: bool = False) -> list:
    """``segmented_counters`` of one array for several offset vectors at once: one prefix sum per slot over the array, read at
    every layout's offsets (the array's slot indicators are built once, not once per layout)."""
    x = np.ascontiguousarray(values, dtype=np.uint16).ravel()
    idx = [np.asarray(o, dtype=np.int64).ravel() for o in offsets_list]
    outs = [np.zeros((max(o.size - 1, 0), 32), dtype=np.uint64) for o in idx]
    pre = np.zeros(x.size + 1, dtype=np.int64)
    for slot, m in slot_indicators(x, superset).items():
        np.cumsum(m, dtype=np.int64, out=pre[1:])
        for o, out in zip(idx, outs):
            if o.size > 1:
                out[:, slot] = np.where(o[1:] > o[:-1], pre[o[1:]] - pre[o[:-1]], 0).astype(np.uint64)
    return outs


def periodic_counters(pattern, offsets, superset: bool = False, phase: int = 0) -> np.ndarray:
    """uint64[nseg, 32]: exact rows of the array x[i] = pattern[(i + phase) % P] (P = len(pattern)) for any offsets, in
    O(P + nseg): per slot, the count over [0, t) is (t // P) * (count over one period) + (count over the period's first t % P)."""
    p = np.roll(np.ascontiguousarray(pattern, dtype=np.uint16).ravel(), -int(phase))
    period = p.size
    o = np.asarray(offsets, dtype=np.int64).ravel()
    nseg = o.size - 1
    out = np.zeros((max(nseg, 0), 32), dtype=np.uint64)
    if nseg <= 0:
        return out
    nonempty = o[1:] > o[:-1]
    for slot, m in slot_indicators(p, superset).items():
        pre = np.concatenate([[0], np.cumsum(m, dtype=np.int64)])

        def upto(t):
            return (t // period) * pre[-1] + pre[t % period]

        out[:, slot] = np.where(nonempty, upto(o[1:]) - upto(o[:-1]), 0).astype(np.uint64)
    return out


# ------------------------------------------------------------------ the segmented kernel's work split, mirrored
# (fsk_launch_segments and the prologue of fsk::flagstat_segments in libflagstats_amd/csrc/flagstat_segments.hip; the CPU test
# test_segments_host.py::test_writer_mirror_matches_the_sources reads these values and rules back out of the sources)
SEG_UNIT = 4096           # kSegWaveFlags: flags per wave unit
SEG_WAVES_PER_BLOCK = 4   # kThreads / 64
SEG_EPOCH = 255           # (1 << kSegDepth) - 1: chain steps (units) between epoch flushes
SEG_MIN_UNITS = 2         # the default policy: shortest run of whole units that goes through the chain


class WriterSplit:
    """The writers (waves) of one launch over ``n`` flags whose first flag lies ``addr_mod_16`` bytes past a 16-byte boundary.

    ``begin[w], end[w]``: writer w's flags [p0, E) as indices into the launched array (grid position - lo0); writers whose
    range is empty have begin == end.  Unit boundaries lie at array indices ``k * SEG_UNIT - lo0``."""

    def __init__(self, addr_mod_16: int, n: int, grid_blocks: int):
        assert addr_mod_16 % 2 == 0 and n > 0 and grid_blocks > 0
        self.lo0 = (addr_mod_16 % 16) // 2
        hi0 = self.lo0 + n
        self.n = n
        self.nunits = (hi0 + SEG_UNIT - 1) // SEG_UNIT
        want = (self.nunits + 3) // 4                      # one unit per wave at least
        self.grid = min(want, grid_blocks)
        self.waves = SEG_WAVES_PER_BLOCK * self.grid
        gw = np.arange(self.waves, dtype=np.int64)
        self.u_begin = gw * self.nunits // self.waves
        self.u_end = (gw + 1) * self.nunits // self.waves
        p0 = np.maximum(self.u_begin * SEG_UNIT, self.lo0)
        e = np.maximum(np.minimum(self.u_end * SEG_UNIT, hi0), self.lo0)   # (empty writers: begin == end)
        self.begin = np.minimum(p0, e) - self.lo0
        self.end = e - self.lo0

    def seams(self) -> np.ndarray:
        """array indices where one non-empty writer's range ends and the next one's begins"""
        live = self.end > self.begin
        return self.end[live][:-1]

    def pieces(self, offsets, min_units: int = SEG_MIN_UNITS) -> dict:
        """Every (writer, segment) piece of a launch with these offsets (array indices, non-decreasing, clamped to [0, n] as
        the kernel clamps them).  Arrays, one entry per non-empty piece:
          writer, seg, b, e   the piece [b, e) (array indices)
          chain               whole units the chain counts in it (0: the piece is counted per flag only)
          plain               the store form writes the row with plain stores (the segment lies inside this writer)
          head, tail          flags of the piece counted per flag before / after its chain run"""
        o = np.clip(np.asarray(offsets, dtype=np.int64).ravel(), 0, self.n)
        sb, se = o[:-1], o[1:]
        cols = {k: [] for k in ("writer", "seg", "b", "e", "chain", "plain", "head", "tail")}
        for w in range(self.waves):
            p0, E = int(self.begin[w]), int(self.end[w])
            if p0 >= E:
                continue
            s = np.nonzero((se > sb) & (se > p0) & (sb < E))[0]
            b, e = np.maximum(sb[s], p0), np.minimum(se[s], E)
            g0 = -(-(np.maximum(b + self.lo0, self.lo0)) // SEG_UNIT) * SEG_UNIT   # first unit boundary in the piece (grid)
            k = np.maximum((e + self.lo0 - g0) // SEG_UNIT, 0)
            k = np.where((k >= min_units) & (k > 0), k, 0)
            cols["writer"].append(np.full(s.size, w))
            cols["seg"].append(s)
            cols["b"].append(b)
            cols["e"].append(e)
            cols["chain"].append(k)
            cols["plain"].append((sb[s] >= p0) & (se[s] <= E))
            cols["head"].append(np.where(k > 0, g0 - self.lo0 - b, e - b))
            cols["tail"].append(np.where(k > 0, e - (g0 - self.lo0 + k * SEG_UNIT), 0))
        return {k: (np.concatenate(v) if v else np.zeros(0, dtype=np.int64)) for k, v in cols.items()}


def writer_ranges(addr_mod_16: int, n: int, grid_blocks: int) -> WriterSplit:
    """The writers of ``fsk_launch_segments(d_chunk, base, n, ..., grid_blocks)`` with ``d_chunk % 16 == addr_mod_16``."""
    return WriterSplit(addr_mod_16, n, grid_blocks)
