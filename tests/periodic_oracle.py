"""An exact reference for columns too large to hold on the host: what every derived kernel (filter, where, wide, segments and
their combinations) must report for a periodic column with a few explicit elements -- needles -- laid over it.  It generalises
``segments_oracle.periodic_counters`` to the whole grid of counts; tests/test_periodic_oracle_host.py checks it against the
brute-force oracles of the family on arrays of a few million elements, tests/test_gpu_derived_limits.py uses it past 2^32.

The background of element ``j`` of an array of W-byte elements:
    flag       F[(j + phase) % 977]
    high bits  H[j % 13]                     (bits 16 and up; none when W == 2)
    selection  S[(sel_offset + j) % 61]      (the selection is indexed by bit or byte ``sel_offset + j``)
    MAPQ       Q[j % 13]
977, 61 and 13 are odd and pairwise coprime, so no power of two is a period of any column and the joint period is 774,761.  The
slot indicators of the kept elements, ``selected`` and the high bits are built once over the joint period and summed; any
``[b, e)`` then reads as ``(t // L) * pre[L] + pre[t % L]`` at both ends.  No flag of F has bit 0x400 or 0x200, so the background
leaves slot 10, slot 25 and every slot 16..31 at zero; a needle sets one of the two and carries a high bit that no H entry has,
so every needle shows exactly.  The expectation is the background, minus the background at every needle's index, plus the needle.
The predicate is samtools' whole one: ``include_any`` / ``exclude_all`` (--rf / -G) are off at 0, which every unit but the three
rf units passes.

``expect`` also takes index maps -- where an element, a selection bit or byte and a MAPQ byte are really read from.  ``wrapped``
makes the maps of an index held in 32 bits; they model a kernel that is subtly wrong, so that a CPU test can show that the GPU
tests' assertions would fail for one (see ``detects``)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from segments_oracle import slot_indicators  # noqa: E402

LEN_F, LEN_S, LEN_Q = 977, 61, 13
LEN_H = LEN_Q                      # the high bits turn with the MAPQ period: the joint period stays 977 * 61 * 13
JOINT = LEN_F * LEN_S * LEN_Q      # 774,761
INF = 1 << 62
IDENTITY = ((0, INF, 0),)
UNSIGNED = {2: np.uint16, 4: np.uint32, 8: np.uint64}
SELECTED = 32                      # row of a table that holds `selected`; rows 0..31 are the slots, the high bits follow
MODELS = (31, 32, "sext")


def wrapped(model, unit: int = 1):
    """The pieces ``(lo, hi, delta)`` of an index map: index j in [lo, hi) is read at j + delta.  ``unit``: bytes per index.
    31, 32: a byte at offset B >= 2^k is read at B - 2^k (an offset held modulo 2^k); "sext": a byte at 2^31 <= B < 2^32 is read
    at B - 2^32 (a 32-bit offset that was sign-extended); None: the identity."""
    if model is None:
        return IDENTITY
    if model == "sext":
        return ((0, (1 << 31) // unit, 0), ((1 << 31) // unit, (1 << 32) // unit, -((1 << 32) // unit)), ((1 << 32) // unit, INF, 0))
    t = (1 << model) // unit
    return ((0, t, 0), (t, INF, -t))


def delta_at(pieces, i: int) -> int:
    for lo, hi, d in pieces:
        if lo <= i < hi:
            return d
    raise AssertionError(i)


def map_indices(pieces, idx) -> np.ndarray:
    """the map applied to an int64 array of indices"""
    idx = np.asarray(idx, dtype=np.int64)
    out = idx.copy()
    for lo, hi, d in pieces:
        out = np.where((idx >= lo) & (idx < hi), idx + d, out)
    return out


_SATISFIABLE = {}


def flag_pass(flag, require, exclude, include_any=0, exclude_all=0):
    """bool[m]: -f / -F / --rf / -G on uint16 flags; the last two are off at 0"""
    ok = ((flag & np.uint16(require)) == np.uint16(require)) & ((flag & np.uint16(exclude)) == 0)
    if include_any:
        ok &= (flag & np.uint16(include_any)) != 0
    if exclude_all:
        ok &= (flag & np.uint16(exclude_all)) != np.uint16(exclude_all)
    return ok


def satisfiable(require, exclude, include_any=0, exclude_all=0) -> bool:
    """does any of the 65,536 FLAG values pass the four masks?  By trying them all, not by reducing the masks."""
    key = (require, exclude, include_any, exclude_all)
    if key not in _SATISFIABLE:
        _SATISFIABLE[key] = bool(flag_pass(np.arange(65536, dtype=np.uint32).astype(np.uint16), *key).any())
    return _SATISFIABLE[key]


class Result:
    """rows uint64[nseg, 32], selected uint64[nseg], and ``high`` under both rules: ``high_read`` is the OR of the bits above 15
    over every element of the segment (the plain and the filtered entries), ``high_selected`` over the selected ones, passing or
    not (the masked and the combined entries).  All are zero when no FLAG value can pass (``require & exclude != 0``, or --rf / -G
    masks that leave none)."""

    def __init__(self, rows, selected, high_read, high_selected):
        self.rows, self.selected, self.high_read, self.high_selected = rows, selected, high_read, high_selected

    def high(self, masked: bool) -> np.ndarray:
        return self.high_selected if masked else self.high_read

    def same(self, other, masked: bool, wide: bool) -> bool:
        """do the quantities that a test of this call compares agree?"""
        return (np.array_equal(self.rows, other.rows) and np.array_equal(self.selected, other.selected)
                and (not wide or np.array_equal(self.high(masked), other.high(masked))))


class Column:
    """``n`` elements of ``W`` bytes: the periodic background above with ``needles``, ``{index: (flag, high bits, selection bit,
    MAPQ)}``, laid over it.  ``high bits`` is the element's value with its low 16 bits cleared."""

    def __init__(self, W: int, n: int, F, H, S, Q, phase: int = 0, needles=None):
        self.W, self.n, self.phase = W, int(n), int(phase)
        self.F = np.ascontiguousarray(F, dtype=np.uint16)
        self.H = np.ascontiguousarray(H, dtype=np.uint64)
        self.S = np.ascontiguousarray(S, dtype=bool)
        self.Q = np.ascontiguousarray(Q, dtype=np.uint8)
        assert (self.F.size, self.H.size, self.S.size, self.Q.size) == (LEN_F, LEN_H, LEN_S, LEN_Q)
        assert not (self.F & np.uint16(0x600)).any(), "a background flag must leave slot 10 and slot 25 to the needles"
        top = (1 << (8 * W)) - (1 << 16)
        assert all(int(h) & ~top == 0 for h in self.H), "high bits lie above bit 15 and inside the element"
        self.needles = {int(k): (int(f), int(h), bool(s), int(q)) for k, (f, h, s, q) in (needles or {}).items()}
        bg_mask = int(np.bitwise_or.reduce(self.H))
        for k, (f, h, s, q) in self.needles.items():
            assert 0 <= k < self.n and f & 0x600 and 0 <= f < 65536 and h & ~top == 0 and 0 <= q < 256, (k, f, h, q)
            assert W == 2 or (h & ~bg_mask and h < 1 << 63), "a needle carries a high bit (16..62) that no H entry has"
        self.bits = [b for b in range(16, 64) if bg_mask >> b & 1]      # the background's high bits: rows of a table
        self.rows = SELECTED + 1 + 2 * len(self.bits)
        self._tables = {}

    # ------------------------------------------------------------------ single elements
    def _indicators(self, flag, hb, sel, q, require, exclude, min_mapq, masked, include_any=0, exclude_all=0):
        """(row, bool[m]) pairs: which of m elements add 1 to which row of a table (rows without a pair stay 0)"""
        flag = np.ascontiguousarray(flag, dtype=np.uint16)
        ok = flag_pass(flag, require, exclude, include_any, exclude_all)
        if min_mapq > 0:
            ok &= np.asarray(q) >= min_mapq
        pick = np.asarray(sel, dtype=bool) if masked else np.ones(flag.shape, dtype=bool)
        keep = ok & pick
        for slot, m in slot_indicators(flag, True).items():
            yield slot, m & keep
        yield SELECTED, keep
        for i, bit in enumerate(self.bits):
            has = (np.asarray(hb, dtype=np.uint64) >> np.uint64(bit)) & np.uint64(1) != 0
            yield SELECTED + 1 + i, has
            yield SELECTED + 1 + len(self.bits) + i, has & pick

    def _contrib(self, *args):
        """int32[rows, m]: what each of m elements adds to the slots (superset form), to ``selected`` and to the count of
        elements that carry each background high bit (over all elements, then over the selected ones)"""
        out = np.zeros((self.rows, np.asarray(args[0]).size), dtype=np.int32)
        for row, m in self._indicators(*args):
            out[row] = m
        return out

    def _table(self, pf, ph, ps, pq, require, exclude, min_mapq, masked, include_any=0, exclude_all=0):
        """int32[rows, JOINT + 1]: prefix sums of ``_contrib`` over one joint period of the background whose element t has flag
        F[(t + pf) % 977], high bits H[(t + ph) % 13], selection S[(t + ps) % 61] and MAPQ Q[(t + pq) % 13]"""
        if not masked:
            ps = 0
        if min_mapq == 0:
            pq = 0
        key = (pf, ph, ps, pq, require, exclude, min_mapq, masked, include_any, exclude_all)
        if key in self._tables:
            self._tables[key] = self._tables.pop(key)         # most recently used: last
        else:
            if len(self._tables) >= 8:
                self._tables.pop(next(iter(self._tables)))
            tile = lambda p, shift: np.tile(np.roll(p, -shift), JOINT // p.size)  # noqa: E731
            tab = np.zeros((self.rows, JOINT + 1), dtype=np.int32)
            for row, m in self._indicators(tile(self.F, pf), tile(self.H, ph), tile(self.S, ps), tile(self.Q, pq), require, exclude, min_mapq, masked,
                                           include_any, exclude_all):
                np.cumsum(m, dtype=np.int32, out=tab[row, 1:])
            self._tables[key] = tab
        return self._tables[key]

    @staticmethod
    def _upto(tab, t):
        """int64[rows, m]: the sums over [0, t) for every t of an int64 array"""
        return (t // JOINT)[None, :] * tab[:, -1].astype(np.int64)[:, None] + tab[:, t % JOINT]

    def background(self, ja, js, jq):
        """(flag, high bits, selection, MAPQ) of the background at element indices ``ja``, selection indices ``js`` (bit or byte
        numbers, the offset included) and MAPQ indices ``jq``; negative indices continue the pattern"""
        ja, js, jq = (np.asarray(x, dtype=np.int64) for x in (ja, js, jq))
        return self.F[(ja + self.phase) % LEN_F], self.H[ja % LEN_H], self.S[js % LEN_S], self.Q[jq % LEN_Q]

    def read(self, ja, je, jq, sel_offset: int = 0):
        """the same with the needles: the selection is read at the bit or byte of ELEMENT ``je``"""
        flag, hb, sel, q = (x.copy() for x in self.background(ja, np.asarray(je, dtype=np.int64) + sel_offset, jq))
        for k, (f, h, s, m) in self.needles.items():
            flag[np.asarray(ja) == k], hb[np.asarray(ja) == k] = f, h
            sel[np.asarray(je) == k] = s
            q[np.asarray(jq) == k] = m
        return flag, hb, sel, q

    def materialize(self, b: int, e: int, sel_offset: int = 0):
        """(values uint of W bytes, mask bool, mapq uint8) of elements [b, e), needles included: for the brute-force oracles"""
        j = np.arange(b, e, dtype=np.int64)
        flag, hb, sel, q = self.read(j, j, j, sel_offset)
        return (flag.astype(np.uint64) | hb).astype(UNSIGNED[self.W]), sel, q

    # ------------------------------------------------------------------ the expectation
    def expect(self, offsets, require: int = 0, exclude: int = 0, min_mapq: int = 0, masked: bool = False, sel_offset: int = 0,
               superset: bool = False, array_map=IDENTITY, sel_map=IDENTITY, mapq_map=IDENTITY, include_any: int = 0,
               exclude_all: int = 0) -> Result:
        """What a call over the segments ``offsets`` (element indices into this column, clamped to [0, n] as the kernels clamp
        them; a segment whose end lies before its begin is empty) must report.  ``masked``: the call takes a selection, element j
        being bit or byte ``sel_offset + j``.  The maps say where element j's value (``array_map``, in elements), its selection
        bit or byte (``sel_map``, applied to ``sel_offset + j``) and its MAPQ (``mapq_map``) are read from.  ``include_any`` /
        ``exclude_all``: samtools' --rf / -G, off at 0; FLAG masks that no 16-bit value satisfies read nothing, like an
        overlapping pair."""
        o = np.clip(np.asarray(offsets, dtype=np.int64).ravel(), 0, self.n)
        b, e = o[:-1], np.maximum(o[1:], o[:-1])
        nseg = b.size
        zero = lambda: np.zeros(nseg, dtype=np.uint64)  # noqa: E731
        if not satisfiable(require, exclude, include_any, exclude_all) or nseg == 0:
            return Result(np.zeros((nseg, 32), dtype=np.uint64), zero(), zero(), zero())
        pred = (require, exclude, min_mapq, masked, include_any, exclude_all)
        acc = np.zeros((self.rows, nseg), dtype=np.int64)
        cuts = sorted({0, INF} | {lo for lo, _, _ in array_map} | {lo for lo, _, _ in mapq_map}
                      | {max(lo - sel_offset, 0) for lo, _, _ in sel_map})
        for p, q in zip(cuts[:-1], cuts[1:]):
            x, y = np.clip(b, p, q), np.clip(e, p, q)
            live = y > x
            if not live.any():
                continue
            da, ds, dq = delta_at(array_map, p), delta_at(sel_map, p + sel_offset), delta_at(mapq_map, p)
            tab = self._table((self.phase + da) % LEN_F, da % LEN_H, (sel_offset + ds) % LEN_S, dq % LEN_Q, *pred)
            acc[:, live] += self._upto(tab, y[live]) - self._upto(tab, x[live])
        # the needles: every element that reads a needle's value, selection bit or MAPQ gives back what the background put there
        # and adds what it really reads
        hit = set()
        for k in self.needles:
            for pieces, shift in ((array_map, 0), (mapq_map, 0), (sel_map, sel_offset)):
                hit |= {k - d for lo, hi, d in pieces if lo <= k - d + shift < hi and k - d >= 0}
        extra_read, extra_sel = zero(), zero()
        if hit:
            J = np.array(sorted(hit), dtype=np.int64)
            ja, jq = map_indices(array_map, J), map_indices(mapq_map, J)
            je = map_indices(sel_map, J + sel_offset) - sel_offset
            was = self._contrib(*self.background(ja, je + sel_offset, jq), *pred)
            flag, hb, sel, mq = self.read(ja, je, jq, sel_offset)
            now = self._contrib(flag, hb, sel, mq, *pred)
            own = hb & ~np.uint64(sum(1 << bit for bit in self.bits))       # bits that the tables do not follow
            for i, j in enumerate(J):
                inside = (b <= j) & (j < e)
                acc[:, inside] += (now[:, i] - was[:, i])[:, None].astype(np.int64)
                extra_read[inside] |= own[i]
                if sel[i] or not masked:
                    extra_sel[inside] |= own[i]
        assert (acc >= 0).all()
        rows = np.ascontiguousarray(acc[:32].T).astype(np.uint64)
        if not superset:
            rows[:, [0, 9, 16]] = 0
        nb = len(self.bits)
        high_read, high_sel = extra_read, extra_sel
        for i, bit in enumerate(self.bits):
            high_read = high_read | np.where(acc[SELECTED + 1 + i] > 0, np.uint64(1 << bit), np.uint64(0))
            high_sel = high_sel | np.where(acc[SELECTED + 1 + nb + i] > 0, np.uint64(1 << bit), np.uint64(0))
        return Result(rows, acc[SELECTED].astype(np.uint64), high_read, high_sel)

    def detects(self, offsets, wide=None, **call):
        """The wrapped models of one call: ``{(what, model): bool}`` -- does the quantity that a test of this call compares
        (rows, selected, and high when ``wide``) differ from the truth when the array's byte offset, the selection index, the
        MAPQ index or the segment offsets are held in 32 bits?  Only what the call reads is listed: no selection index without
        a selection, no MAPQ index with ``min_mapq == 0``; None where the model moves no index that the call reads (a selection
        offset of 2^32 + 13 leaves no index in [2^31, 2^32) to sign-extend)."""
        wide = self.W > 2 if wide is None else wide
        masked = call.get("masked", False)
        truth = self.expect(offsets, **call)
        o = np.clip(np.asarray(offsets, dtype=np.int64), 0, self.n)
        first, last = int(o.min()), int(o.max())

        def moves(pieces, lo, hi):
            """does the map move an index of [lo, hi)?"""
            return any(d and max(a, lo) < min(b, hi) for a, b, d in pieces)

        out = {}
        for model in MODELS:
            so = call.get("sel_offset", 0)
            tries = {"array": ("array_map", wrapped(model, self.W), first, last), "offsets": (None, wrapped(model), first, last + 1)}
            if masked:
                tries["selection"] = ("sel_map", wrapped(model), so + first, so + last)
            if call.get("min_mapq", 0) > 0:
                tries["mapq"] = ("mapq_map", wrapped(model), first, last)
            for what, (name, pieces, lo, hi) in tries.items():
                if not moves(pieces, lo, hi):
                    out[(what, model)] = None
                elif name is None:
                    out[(what, model)] = not truth.same(self.expect(map_indices(pieces, offsets), **call), masked, wide)
                else:
                    out[(what, model)] = not truth.same(self.expect(offsets, **call, **{name: pieces}), masked, wide)
        return out


# ------------------------------------------------------------------ the columns and calls of tests/test_gpu_derived_limits.py
# (stated here so that tests/test_periodic_oracle_host.py can show, on the CPU, that every one of them tells a wrapped index)
MARK = {2: 1 << 32, 4: 1 << 32, 8: 1 << 31}          # int64: 2^32 elements would be 32 GiB; 2^31 are past 2^32 bytes four times
NEEDLE_AT = (1 << 28, 1 << 29, 1 << 30, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1)
NEEDLE_FLAGS = (0x443, 0x283, 0x409, 0x661, 0x410, 0x2A3, 0x481, 0x603, 0x4C1, 0x223, 0x643)   # all pass -F 0x904, six also -f 2
NEEDLE_BITS = {2: (), 4: (16, 18, 19, 20, 21, 23, 24, 25, 26, 27, 28), 8: (33, 36, 39, 44, 48, 52, 57, 62, 31, 45, 50)}
H_BITS = {2: (), 4: (17, 22, 30), 8: (17, 40, 61)}
NEEDLE_MAPQ = 60                                      # every background MAPQ is 1..59
PREDICATES = ((0, 0x904, 0), (2, 0x904, 30), (0, 0, 0))     # -F 0x904; -f 0x2 -F 0x904 -q 30; the empty predicate
BIG_OFFSET = (1 << 32) + 13
HOST_N = (1 << 32) + 3 * 65536 + 5
HOST_WIDE_N = (1 << 29) + 65541


def slab_n(W: int) -> int:
    return MARK[W] + 3 * (1 << 20) + 5


def needle_positions(n: int) -> dict:
    """``{element: place in the list}`` of the needles of a column of n elements, whatever its width: elements 2^31 - 1, 2^31,
    2^32 - 1, 2^32, 2^32 + 1, the elements at byte offsets 2^31 and 2^32 of an int32 and an int64 column (2^28, 2^29, 2^30), the
    last element of either slab, and n - 1; what the column does not have is left out.  One list for every width, so that the
    MAPQ column and the selections, which the widths share, carry the same needles."""
    out = {}
    for i, p in enumerate(NEEDLE_AT + (slab_n(8) - 1, slab_n(2) - 1, n - 1)):
        if 0 <= p < n and p not in out:
            out[p] = i
    return out


def patterns(W: int):
    """(F, H, S, Q) of the background"""
    rng = np.random.RandomState(977)                 # F, S and Q are those of every width: the widths share MAPQ and selections
    F = (rng.randint(0, 65536, LEN_F) & ~0x600).astype(np.uint16)
    F[::5] &= np.uint16(0xFFFF & ~0x904)             # a fifth passes -F 0x904 for sure, and
    F[::10] |= np.uint16(0x3)                        # a tenth -f 2 as a primary paired read
    S = rng.randint(0, 2, LEN_S).astype(bool)
    S[:2] = (True, False)
    Q = np.array([1, 7, 29, 30, 31, 59, 12, 45, 3, 30, 58, 22, 37], dtype=np.uint8)
    H = np.zeros(LEN_H, dtype=np.uint64)
    for i, bit in enumerate(H_BITS[W]):
        H[2 + 3 * i] = H[3 + 3 * i] = np.uint64(1 << bit)
    if W > 2:
        H[12] = np.uint64((1 << H_BITS[W][0]) | (1 << H_BITS[W][2]))
    return F, H, S, Q


def column(W: int, n=None, dense: bool = False) -> Column:
    """The column of width W.  ``dense``: the selection is all ones but for the needles at even places in the list, and the
    needles at odd places have MAPQ 0 -- under ``-q 1`` no needle counts and every background element does, so that
    ``selected`` and slot 9 pass 2^32 in one workgroup, and an element that reads another's selection bit or MAPQ shows."""
    n = slab_n(W) if n is None else n
    F, H, S, Q = patterns(W)
    needles = {}
    for p, i in needle_positions(n).items():
        high = 0 if W == 2 else 1 << NEEDLE_BITS[W][i]
        needles[p] = (NEEDLE_FLAGS[i], high, i % 2 == 1, NEEDLE_MAPQ if i % 2 == 0 else 0) if dense else (NEEDLE_FLAGS[i], high, True, NEEDLE_MAPQ)
    if dense:
        S = np.ones(LEN_S, dtype=bool)
    return Column(W, n, F, H, S, Q, phase=W, needles=needles)


def layouts(W: int, n: int) -> dict:
    """the three segment layouts: 512,000-element blocks, one segment [7, n - 3), and "around the mark" -- a long segment up to
    mark - 700,001, then 3,000 segments of 1..2,000 elements that cross the mark, and one segment to n - 3.  Element n - 1, a
    needle, lies in no segment of the last two and must count nowhere."""
    mark = MARK[W]
    rng = np.random.RandomState(3000 + W)
    small = mark - 700_001 + np.concatenate([[0], np.cumsum(rng.randint(1, 2001, 3000))])
    assert small[0] < mark < small[-1] < n - 3 and np.searchsorted(small, mark + 1) < small.size
    return {"blocks": np.append(np.arange(0, n, 512_000), n).astype(np.int64),
            "one": np.array([7, n - 3], dtype=np.int64),
            "around": np.concatenate([[3], small, [n - 3]]).astype(np.int64)}


def window(W: int):
    """(start, length) of the window that begins past the mark, at an address that is no multiple of 16: a few steps of 32 KiB
    and a ragged end"""
    return MARK[W] + 1, 5 * (32768 // W) + 77


def union_expect(col: Column, ranges, superset=False, **call) -> Result:
    """the flat result over the union of disjoint element ranges: what a mask that selects exactly these elements gives"""
    o = np.array(sorted(ranges), dtype=np.int64)
    nseg = len(ranges)
    r = col.expect(o.ravel(), superset=superset, **call)
    pick = np.arange(0, 2 * nseg - 1, 2)              # the ranges themselves, not what lies between them
    return Result(r.rows[pick].sum(axis=0, keepdims=True), r.selected[pick].sum(keepdims=True),
                  np.bitwise_or.reduce(r.high_read[pick], keepdims=True), np.bitwise_or.reduce(r.high_selected[pick], keepdims=True))


BLOCK_AT, BLOCK_LEN = 100_003, 4000          # the background elements that the one-needle masks select beside the needle


def one_needle_ranges(k: int, sel_pieces=IDENTITY):
    """the element ranges that the mask of needle k selects, as a kernel sees them whose selection index goes through the map"""
    out = []
    for b, e in ((BLOCK_AT, BLOCK_AT + BLOCK_LEN), (k, k + 1)):
        for lo, hi, d in sel_pieces:                  # element j reads bit j + d: selected when j + d lies in [b, e)
            x, y = max(b - d, lo, 0), min(e - d, hi)
            if y > x:
                out.append((x, y))
    return out


def slab_calls(W: int) -> list:
    """The calls over the resident slab of width W, each a dict: ``case`` (its name), ``layout`` (the name of its offsets),
    ``offsets`` (absolute element indices; flat
    kernels get the one segment as their array), ``pred`` (require, exclude, min_mapq), ``form`` and ``sel_offset`` (the selection:
    "bytes" or "bitmap", and the bit or byte of ELEMENT 0 of the slab), ``local`` (the call is handed pointers to the segment's
    first element, so only its selection index passes 2^32).  A kernel without a filter or without a selection takes the call
    without it (``reduced``)."""
    n = slab_n(W)
    lay = layouts(W, n)
    start, m = window(W)
    whole, win = np.array([0, n], dtype=np.int64), np.array([start, start + m], dtype=np.int64)
    p0, p1, p2 = PREDICATES
    forms = (("bytes", "bytes", 0), ("bitmap", "bitmap", 0), ("bitmap-big", "bitmap", BIG_OFFSET))   # byte mask; byte boundary; funnelled
    flat = [dict(case="whole-%s-p%d" % (name, i), layout="whole", offsets=whole, pred=pred, form=form, sel_offset=so, local=False)
            for i, pred in enumerate(PREDICATES) for name, form, so in forms]                        # every predicate under every mask form
    return flat + [dict(case="window-bitmap", layout="window", offsets=win, pred=p1, form="bitmap", sel_offset=5, local=True),
                   dict(case="window-bytes", layout="window", offsets=win, pred=p0, form="bytes", sel_offset=0, local=True),
                   dict(case="blocks", layout="blocks", offsets=lay["blocks"], pred=p0, form="bytes", sel_offset=0, local=False),
                   dict(case="one", layout="one", offsets=lay["one"], pred=p1, form="bitmap", sel_offset=BIG_OFFSET, local=False),
                   dict(case="around", layout="around", offsets=lay["around"], pred=p2, form="bitmap", sel_offset=5, local=False)]


def call_key(call: dict, filt: bool, mask: bool) -> tuple:
    """what the expectation of a call depends on: calls that differ only in what a kernel does not take share it"""
    return (call["layout"],) + tuple(sorted(reduced(call, filt, mask).items()))


def reduced(call: dict, filt: bool, mask: bool) -> dict:
    """the keyword arguments of ``Column.expect`` for a kernel with / without a filter and a selection"""
    require, exclude, min_mapq = call["pred"] if filt else (0, 0, 0)
    include_any, exclude_all = call.get("rf", (0, 0)) if filt else (0, 0)
    return dict(require=require, exclude=exclude, min_mapq=min_mapq, masked=mask, sel_offset=call["sel_offset"] if mask else 0,
                include_any=include_any, exclude_all=exclude_all)


HOST_OFFSETS = {2: (5, 1000, (1 << 31) + 7, (1 << 32) - 3, (1 << 32) + 2, HOST_N - 2), 8: (0, HOST_WIDE_N)}
HOST_CALL = dict(pred=(0, 0, 30), form="bitmap", sel_offset=3, local=False)      # a bitmap at an odd offset, -q 30
DENSE_CALL = dict(pred=(0, 0, 1), form="bitmap", sel_offset=0, local=False)      # one workgroup: everything passes -q 1


# ------------------------------------------------------------------ the two units of the whole predicate (--rf / -G)
# (require, exclude, include_any, exclude_all, min_mapq): -F 0x904 --rf 0x60 -G 0x3 leaves both tests to the kernel (0x60 and 0x3
# share no bit with 0x904); the second has -q 30 on top.  Of the eleven NEEDLE_FLAGS six have bit 5 or 6 and five neither; six
# have bits 0 and 1 both and five do not.
RF_PREDICATES = ((0, 0x904, 0x60, 0x3, 0), (0, 0x904, 0x60, 0x3, 30))
# one workgroup: --rf of every bit a background flag can have, -G of the same -- all but a few background flags pass -- and -q 1
RF_DENSE = (0, 0, 0xF9FF, 0xF9FF, 1)


def rf_call(pred, offsets, case, layout) -> dict:
    """a call of the rf units in the form of slab_calls, no selection: over [offsets[0], offsets[1]) for the flat ones, over the
    segments `offsets` for the segmented one"""
    require, exclude, include_any, exclude_all, min_mapq = pred
    return dict(case=case, layout=layout, offsets=np.asarray(offsets, dtype=np.int64), pred=(require, exclude, min_mapq),
                rf=(include_any, exclude_all), form="bytes", sel_offset=0, local=False)


def rf_slab_calls(W: int) -> list:
    """the calls of u16_filter_rf / wide_filter_rf over the resident slab of width W: the whole slab and the window that begins
    past the mark, under both RF_PREDICATES"""
    n = slab_n(W)
    start, m = window(W)
    return ([rf_call(p, (0, n), "rf-whole-p%d" % i, "whole") for i, p in enumerate(RF_PREDICATES)]
            + [rf_call(p, (start, start + m), "rf-window-p%d" % i, "window") for i, p in enumerate(RF_PREDICATES)])


# ------------------------------------------------------------------ the segmented unit of the whole predicate
# The `one` and `around` layouts leave elements [0, 7) or [0, 3) in front and [n - 3, n) behind to no segment, so that a kernel
# that ignored offsets[0] or offsets[nseg] counts them -- if they pass.  Under RF_PREDICATES none of them does (-F 0x904 and -G 0x3
# keep all of them out), so these two layouts run under predicates of their own: -F 0x4 --rf 0x60 -G 0x11, a residue of both
# tests, without and with -q 30.  Element 0 (flag 0xA9E9, MAPQ 1) passes the first, element 4 (0x6128, MAPQ 31) both, and so does
# the needle at n - 1 (0x223 or 0x643, MAPQ 60).  The MAPQ of elements 0, 1 and 2 is 1, 7 and 29: under -q 30 the three elements
# in front of `around` cannot count, and that one bound is tested by the call without -q alone
# (tests/test_periodic_oracle_host.py asserts all of this).
RF_BOUNDS_PREDICATES = ((0, 0x4, 0x60, 0x11, 0), (0, 0x4, 0x60, 0x11, 30))
RF_SEGMENTED_UNIT = (False, True, True, False, "rf")      # u16_segments_filter_rf: uint16 only


def rf_segments_slab_calls() -> list:
    """the calls of u16_segments_filter_rf over the resident uint16 slab: the three layouts -- `blocks` under RF_PREDICATES, `one`
    and `around` under RF_BOUNDS_PREDICATES -- and the window that begins past the mark under RF_PREDICATES (``local``: it is
    handed pointers to its first element)"""
    n = slab_n(2)
    lay = layouts(2, n)
    start, m = window(2)
    calls = []
    for i in (0, 1):
        calls.append(rf_call(RF_PREDICATES[i], lay["blocks"], "rf-blocks-p%d" % i, "blocks"))
        calls.append(rf_call(RF_BOUNDS_PREDICATES[i], lay["one"], "rf-one-b%d" % i, "one"))
        calls.append(rf_call(RF_BOUNDS_PREDICATES[i], lay["around"], "rf-around-b%d" % i, "around"))
        calls.append(dict(rf_call(RF_PREDICATES[i], (start, start + m), "rf-segments-window-p%d" % i, "window"), local=True))
    return calls


def rf_needle_calls(col: Column, offsets) -> list:
    """(needle, call) for every needle of the column that lies inside the layout `offsets`: the layout under the residue predicate
    that this needle alone passes"""
    o = np.asarray(offsets, dtype=np.int64)
    return [(k, rf_call(needle_rf_predicate(flag), o, "rf-around-needle-%d" % k, "around"))
            for k, (flag, _, _, _) in sorted(col.needles.items()) if o[0] <= k < o[-1]]


def needle_rf_predicate(flag: int) -> tuple:
    """a residue predicate with -q 60 (NEEDLE_MAPQ: no background element passes) that, of the NEEDLE_FLAGS, only `flag` passes:
    -f / -F fix bits 0..8 and 11 to the needle's; 0x443 and 0x643 differ in bit 9 alone, which --rf and -G tell: a needle with
    one of bits 9 and 10 passes --rf 0x600 -G 0x600, one with both --rf 0x1200 -G 0x5000"""
    low = flag & 0x9FF
    one = bin(flag & 0x600).count("1") == 1
    return (low, 0x9FF & ~low, 0x600 if one else 0x1200, 0x600 if one else 0x5000, NEEDLE_MAPQ)
