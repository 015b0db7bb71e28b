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
