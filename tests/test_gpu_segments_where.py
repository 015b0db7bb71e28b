"""The selected-elements segmented flagstat on the MI355X: fsk::flagstat_segments_where (bitmap, at a byte boundary of the array's
grid or funnelled), the byte form through fsk::flagstat_segments_filter<true>, the three C entries and
libflagstats_amd/segments_where.py.  Every comparison is exact.

Expected rows never come from the code under test: segments_where_oracle.want is segments_oracle.segmented_counters of the array
with the unselected flags zeroed, slot 9 from the definition; the expected `selected` is the per-segment sum of the mask.  The
selection is indexed by array element; poison flags (0xFFFF, which count in most slots) whose bits or bytes are SET lie around the
arrays, in front of the first segment and behind the last, and the unused bits of a bitmap's first and last byte are set too, so
that anything counted from outside its segment shows.  Layouts are placed with segments_oracle.WriterSplit, the launcher's work
split mirrored, and checked to contain the runs they are for."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_where_oracle as swo  # noqa: E402
from segments_oracle import SEG_EPOCH, SEG_UNIT, segmented_counters, writer_ranges  # noqa: E402
from segments_where_oracle import BITMAP, BYTES, pack  # noqa: E402

pytestmark = pytest.mark.gpu

U = SEG_UNIT
P = 65_521                                    # prime: no unit, row or writer seam is a multiple of the period
STORE, SUPERSET = 1, 2
MODES = (1, 0, 3, 2)                          # store, +=, store + superset, += + superset
GARBAGE, BIAS, SEL_BIAS = 0x5EED_0000_0BAD, 3, 1_000_003
BYTE_ALIGNMENTS = (0, 1, 3, 8, 15)
EVERY_MIN_UNITS = (0, 1, 2, 3, 255, 256, 0xFFFFFFFF)   # tests/test_gpu_segments_regimes.py's list
POISON = 0xFFFF


def dev16(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint16).view(np.int16)).cuda()


def dev8(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint8)).cuda()


def dev64(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.int64)).cuda()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def err(hip):
    return hip.FLAGSTATS_hip_last_error().decode(errors="replace")


def expect(want_sup, want_sel, mode):
    """what a launch in `mode` must leave in rows prefilled with GARBAGE (store) or BIAS (+=) and counts prefilled with GARBAGE
    or SEL_BIAS"""
    w = want_sup.copy()
    if not mode & SUPERSET:
        w[:, [0, 9, 16]] = 0
    if mode & STORE:
        return w, want_sel.copy()
    return w + np.uint64(BIAS), want_sel + np.uint64(SEL_BIAS)


class Batch:
    """device words for many launches -- per launch nseg rows of 32, then nseg counts -- prefilled in one copy and read back in
    one copy after every launch has been queued (tests/test_gpu_segments_filter.py's)"""

    def __init__(self):
        self.items, self.words, self.t = [], 0, None

    def add(self, mode, want_sup, want_sel, note, with_selected=True):
        nseg = want_sup.shape[0]
        self.items.append((self.words, nseg, mode, want_sup, want_sel, note, with_selected))
        self.words += nseg * 33
        return len(self.items) - 1

    def upload(self):
        import torch
        host = np.empty(max(self.words, 1), dtype=np.uint64)
        for at, nseg, mode, _, _, _, _ in self.items:
            host[at:at + nseg * 32] = GARBAGE if mode & STORE else BIAS
            host[at + nseg * 32:at + nseg * 33] = GARBAGE if mode & STORE else SEL_BIAS
        self.host = host
        self.t = torch.from_numpy(host.view(np.int64)).cuda()
        torch.cuda.synchronize()

    def mode(self, k):
        return self.items[k][2]

    def out(self, k):
        return self.t.data_ptr() + 8 * self.items[k][0]

    def selected(self, k):
        at, nseg = self.items[k][:2]
        return self.t.data_ptr() + 8 * (at + nseg * 32) if self.items[k][6] else None

    def check(self):
        import torch
        torch.cuda.synchronize()
        got = self.t.cpu().numpy().view(np.uint64)
        for at, nseg, mode, want_sup, want_sel, note, with_selected in self.items:
            rows, sel = expect(want_sup, want_sel, mode)
            g = got[at:at + nseg * 32].reshape(nseg, 32)
            bad = np.nonzero((g != rows).any(axis=1))[0]
            assert bad.size == 0, (note, "mode", mode, "rows", bad[:8], g[bad[:2]], rows[bad[:2]])
            gs = got[at + nseg * 32:at + nseg * 33]
            if not with_selected:
                sel = self.host[at + nseg * 32:at + nseg * 33]      # NULL d_selected: the words behind the rows stay
            bad = np.nonzero(gs != sel)[0]
            assert bad.size == 0, (note, "mode", mode, "selected", bad[:8], gs[bad[:8]], sel[bad[:8]])


class Arena:
    """many host arrays in one device allocation, each at a chosen phase (in elements) of a 16-byte line and with `pad` elements
    of `fill` around it; uploaded in one copy"""

    def __init__(self, dtype, fill, pad=64):
        self.dtype, self.fill, self.pad = np.dtype(dtype), fill, pad
        self.per = 16 // self.dtype.itemsize
        self.parts, self.size, self.t = [], 0, None

    def add(self, x, phase=0):
        x = np.ascontiguousarray(x, dtype=self.dtype)
        start = (self.size + self.pad + self.per - 1) // self.per * self.per + phase
        self.parts.append((start, x))
        self.size = start + x.size + self.pad
        return start

    def upload(self):
        import torch
        host = np.full((self.size + self.per) // self.per * self.per, self.fill, dtype=self.dtype)
        for start, x in self.parts:
            host[start:start + x.size] = x
        signed = {1: np.uint8, 2: np.int16, 8: np.int64}[self.dtype.itemsize]
        self.t = torch.from_numpy(host.view(signed)).cuda()
        assert self.t.data_ptr() % 16 == 0
        return self

    def ptr(self, start):
        return self.t.data_ptr() + start * self.dtype.itemsize


def encode(mask, sel_bits, where, value=1):
    """the bytes of a mask for the selection arena and the phase to place them at: a bitmap that starts `where` bits into its
    first byte (every unused bit set), or bytes of `value` per selected element at byte alignment `where`.  Returns
    (bytes, arena phase, sel_offset)"""
    m = np.asarray(mask, dtype=bool)
    if sel_bits == BITMAP:
        return pack(m, where, fill=1), 0, where
    return m.astype(np.uint8) * np.uint8(value), where, 0


def get_policy(hip):
    mu, bpc = ctypes.c_uint32(), ctypes.c_uint32()
    hip.fsk_segments_policy(ctypes.byref(mu), ctypes.byref(bpc))
    return mu.value, bpc.value


@pytest.fixture(scope="module")
def launcher(hip):
    hip.fsk_segments_policy.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    hip.fsk_segments_policy.restype = None
    hip.fsk_set_segments_policy.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    hip.fsk_set_segments_policy.restype = None
    return hip.fsk_launch_segments_where


@contextlib.contextmanager
def policy(hip, min_units, blocks_per_cu=1):
    saved = get_policy(hip)
    try:
        hip.fsk_set_segments_policy(min_units, blocks_per_cu)
        yield
    finally:
        hip.fsk_set_segments_policy(*saved)
    assert get_policy(hip) == saved


def coprime_offsets(n, start=0, lengths=(7, 11, 13, 0, 4099, 1, 509, 8191, 17, 0, 0, 3, 1021, 64, 4096, 19)):
    """segments of lengths without a common factor with the vector, the row or the unit (and some empty ones), end to end"""
    o = [start]
    i = 0
    while o[-1] < n:
        o.append(min(o[-1] + lengths[i % len(lengths)], n))
        i += 1
    return np.array(o, dtype=np.int64)


def device_entry(hip, arr, n, d_off, nseg, sel, sel_offset, sel_bits, batch, k, stream=None):
    rc = hip.FLAGSTATS_hip_device_u16_segments_where(arr, n, d_off, nseg, sel, sel_offset, sel_bits, batch.out(k), batch.selected(k),
                                                     batch.mode(k), stream)
    assert rc == 0, (batch.items[k][5], err(hip))


# ------------------------------------------------------------------ 1. every value
def test_every_value(hip, launcher):
    """0..65535 once each among as many 0xFFFF poison flags (32 units), cut into segments of coprime lengths; the mask selects the
    real ones.  Both encodings (the bitmap 5 bits into its first byte, the bytes at alignment 3), all four modes, the device
    entry, the _sync form and the host form, and the four Python functions"""
    import torch
    from libflagstats_amd import segments_where as sw
    n = 2 * 65536
    rng = np.random.RandomState(2026)
    mask = np.zeros(n, dtype=bool)
    mask[rng.permutation(n)[:65536]] = True
    values = np.full(n, POISON, dtype=np.uint16)
    values[mask] = rng.permutation(65536).astype(np.uint16)
    o = coprime_offsets(n - 5, start=2)
    nseg = o.size - 1
    want_rows, want_sel = swo.want(values, o, mask, superset=True)
    assert int(want_sel.sum()) == int(mask[2:n - 5].sum()) and (want_sel < np.diff(o).astype(np.uint64)).any()
    t, d_off = dev16(values), dev64(o)
    bits, _, bit_off = encode(mask, BITMAP, 5)
    host_sel = {BITMAP: bits, BYTES: np.concatenate([[0xFF] * 3, mask.astype(np.uint8) * 0x40]).astype(np.uint8)}
    sel = {BITMAP: (dev8(bits), bit_off), BYTES: (dev8(host_sel[BYTES]), 3)}     # (device bytes, sel_offset)
    batch = Batch()
    plan = [(sb, batch.add(mode, want_rows, want_sel, ("device", sb, mode))) for sb in (BITMAP, BYTES) for mode in MODES]
    batch.upload()
    for sb, k in plan:
        device_entry(hip, t.data_ptr(), n, d_off.data_ptr(), nseg, sel[sb][0].data_ptr(), sel[sb][1], sb, batch, k)
    batch.check()
    for name, entry, src in (("sync", hip.FLAGSTATS_hip_device_u16_segments_where_sync, t.data_ptr()),
                             ("host", hip.FLAGSTATS_hip_u16_x64_segments_where, values.ctypes.data)):
        for sb in (BITMAP, BYTES):
            s_src = sel[sb][0].data_ptr() if name == "sync" else host_sel[sb].ctypes.data
            for mode in MODES:
                rows = np.full((nseg, 32), GARBAGE if mode & STORE else BIAS, dtype=np.uint64)
                cnt = np.full(nseg, GARBAGE if mode & STORE else SEL_BIAS, dtype=np.uint64)
                rc = entry(src, n, o.ctypes.data, nseg, s_src, sel[sb][1], sb, rows.ctypes.data, cnt.ctypes.data, mode)
                assert rc == 0, (name, sb, mode, err(hip))
                w_rows, w_sel = expect(want_rows, want_sel, mode)
                assert np.array_equal(rows, w_rows) and np.array_equal(cnt, w_sel), (name, sb, mode)
    # the Python layer
    plain_rows, plain_sel = swo.want(values, o, mask)
    for sup, (w_rows, w_sel) in ((False, (plain_rows, plain_sel)), (True, (want_rows, want_sel))):
        for got in (sw.counters_segments_where(values, o, mask, superset=sup),
                    sw.counters_segments_where(values, o, bits, packed=True, bit_offset=5, superset=sup),
                    sw.count_segments_device_ptr_where(t.data_ptr(), n, o, sel[BITMAP][0].data_ptr(), 1, sel_offset=5, superset=sup),
                    sw.count_segments_device_ptr_where(t.data_ptr(), n, o, sel[BYTES][0].data_ptr(), 8, sel_offset=3, superset=sup)):
            assert got[0].dtype == np.uint64 and got[1].dtype == np.uint64
            assert np.array_equal(got[0], w_rows) and np.array_equal(got[1], w_sel), sup
    d_mask = torch.from_numpy(mask).cuda()
    for kw in ({"where": d_mask}, {"where": sel[BITMAP][0], "packed": True, "bit_offset": 5}):
        rows_t, sel_t = sw.count_segments_torch_where(t, d_off, superset=True, **kw)
        torch.cuda.synchronize()
        assert rows_t.dtype == torch.int64 and tuple(rows_t.shape) == (nseg, 32) and tuple(sel_t.shape) == (nseg,) and rows_t.device == t.device
        assert np.array_equal(u64(rows_t), want_rows) and np.array_equal(u64(sel_t), want_sel)
    dicts = sw.flagstats_segments_where(values, o, mask)
    assert [d["n_values"] for d in dicts] == [int(x) for x in plain_sel]
    i = int(np.argmax(plain_sel))
    assert int(dicts[i]["passed"]["mapped"]) == int(plain_sel[i]) - int(plain_rows[i, 2]) - int(plain_rows[i, 18])


# ------------------------------------------------------------------ 2. which bit belongs to which flag
ONE_HOT_VALUES = (0x0041, 0x0081, 0x0403)


def one_hot_layout(lo0):
    """4 units and a bit at grid 1 under min_units 1: per-flag pieces in units 0 and 1, a segment from just before unit 2 to the
    end whose whole units 2 and 3 go through the chain (one run of one unit in each of two writers) and whose ragged rest is
    counted per flag; a gap in front of and behind the segments"""
    n = 4 * U + 77
    g = lambda k: k * U - lo0                                  # array index of unit boundary k  # noqa: E731
    o = np.array([2, 9, 9, 520, g(1) + 1, g(2) - 5, n - 3], dtype=np.int64)
    positions = {0, n - 1}
    for k in range(5):
        for d in (-1, 0, 1, 7, 8, 9, 511, 512, 513):
            positions.add(g(k) + d)
    for s in o.tolist():
        positions.update((s - 1, s))
    return n, o, sorted(p for p in positions if 0 <= p < n)


def one_hot_case(hip, launcher, combos):
    """combos: (phase, sel_bits, bit offset or byte alignment).  The array is poison everywhere but at one position p, the mask
    selects p alone: exactly one row has exactly the counts of that one flag and `selected` 1 (none when p lies outside every
    segment), everything else is 0"""
    import torch
    ones = {v: swo.want(np.array([v], dtype=np.uint16), [0, 1], [True], superset=True)[0][0] for v in ONE_HOT_VALUES}
    arrays, sels, offs = Arena(np.uint16, POISON), Arena(np.uint8, 0xFF, pad=16), Arena(np.int64, 0, pad=0)
    batch, calls = Batch(), []
    i = 0
    for phase, sel_bits, where in combos:
        n, o, positions = one_hot_layout(phase)
        w = writer_ranges(2 * phase, n, 1)
        assert w.lo0 == phase
        pieces = w.pieces(o, 1)
        assert (pieces["chain"] > 0).sum() >= 2 and (pieces["chain"] == 0).any() and ((pieces["chain"] > 0) & (pieces["tail"] > 0)).any()
        a_at = arrays.add(np.full(n, POISON, dtype=np.uint16), phase)
        o_at = offs.add(o)
        nseg = o.size - 1
        for p in positions:
            mask = np.zeros(n, dtype=bool)
            mask[p] = True
            data, sel_phase, sel_offset = encode(mask, sel_bits, where, value=(0x01, 0x80, 0xFF)[i % 3])
            s_at = sels.add(data, sel_phase)
            v = ONE_HOT_VALUES[i % 3]
            want_rows, want_sel = np.zeros((nseg, 32), dtype=np.uint64), np.zeros(nseg, dtype=np.uint64)
            seg = int(np.searchsorted(o, p, side="right")) - 1
            if 0 <= seg < nseg and o[seg] <= p < o[seg + 1]:
                want_rows[seg], want_sel[seg] = ones[v], 1
            k = batch.add(MODES[i % 4], want_rows, want_sel, (phase, sel_bits, where, p))
            calls.append((k, a_at, n, p, v, o_at, nseg, s_at, sel_offset, sel_bits))
            i += 1
    arrays.upload(), sels.upload(), offs.upload()
    batch.upload()
    flat = arrays.t
    with policy(hip, 1):
        for k, a_at, n, p, v, o_at, nseg, s_at, sel_offset, sel_bits in calls:
            flat[a_at + p] = v                       # (stream-ordered with the launch on the null stream)
            rc = launcher(arrays.ptr(a_at), sels.ptr(s_at), sel_offset, sel_bits, 0, n, offs.ptr(o_at), nseg, batch.out(k),
                          batch.selected(k), batch.mode(k), 1, None)
            assert rc == 0, (batch.items[k][5], rc)
            flat[a_at + p] = np.int16(-1).item()     # poison again
    torch.cuda.synchronize()
    batch.check()


@pytest.mark.parametrize("phases", [(0, 1, 2, 3), (4, 5, 6, 7)])
def test_which_bit_belongs_to_which_flag(hip, launcher, phases):
    """array phase x bit offset 0..7: the bitmap at a byte boundary of the array's grid (shift 0) and funnelled at every shift"""
    combos = [(phase, BITMAP, off) for phase in phases for off in range(8)]
    shifts = {(off + 8 - phase) & 7 for phase, _, off in combos}
    assert shifts == set(range(8))
    one_hot_case(hip, launcher, combos)


def test_which_byte_belongs_to_which_flag(hip, launcher):
    """byte alignments 0, 1, 3, 8, 15 x array phases 0, 3 and 6, selecting bytes 0x01, 0x80 and 0xFF in turn"""
    one_hot_case(hip, launcher, [(phase, BYTES, align) for phase in (0, 3, 6) for align in BYTE_ALIGNMENTS])


# ------------------------------------------------------------------ 3. seams smaller than the selection's granularity
def tiny_offsets(start, end):
    """segments of lengths 1, 2, 3, 5 and 0 in turn from `start` up to `end`: a selection byte's 8 bits belong to up to four"""
    o, i = [start], 0
    while o[-1] < end:
        o.append(min(o[-1] + (1, 2, 3, 5, 0)[i % 5], end))
        i += 1
    return np.array(o, dtype=np.int64)


def test_seams_inside_a_vector_and_a_selection_byte(hip, launcher):
    """segment boundaries inside one vector and inside one selection byte, with empty segments among them; layouts that start
    behind offsets[0] > 0 and end before n, and two layouts of one array whose ranges leave a gap between them (CSR offsets have
    no inner gaps: each launch sees the other's range, selected, as flags of no segment).  In front of the first segment and
    behind the last the flags are poison and selected.  Array phases 0, 3, 5; bit offsets 0, 1, 7; byte alignment 1; grids 1, 3
    and the device entry"""
    n = 3 * U + 41
    rng = np.random.RandomState(303)
    values = rng.randint(0, 65536, n).astype(np.uint16)
    mask = rng.randint(0, 2, n).astype(bool)
    layouts = [tiny_offsets(3, n - 5), tiny_offsets(U - 3, 2 * U + 5), tiny_offsets(7, U - 40), tiny_offsets(U + 17, n - 1)]
    values[:3], values[n - 5:], mask[:3], mask[n - 5:] = POISON, POISON, True, True
    wants = [swo.want(values, o, mask, superset=True) for o in layouts]
    for o, (rows, sel) in zip(layouts, wants):
        assert (np.diff(o) <= 5).all() and (np.diff(o) == 0).any() and int(sel.sum()) == int(mask[o[0]:o[-1]].sum())
    arrays, sels, offs = Arena(np.uint16, POISON), Arena(np.uint8, 0xFF, pad=16), Arena(np.int64, 0, pad=0)
    o_at = [offs.add(o) for o in layouts]
    batch, calls = Batch(), []
    i = 0
    for phase in (0, 3, 5):
        a_at = arrays.add(values, phase)
        for sel_bits, where in ((BITMAP, 0), (BITMAP, 1), (BITMAP, 7), (BYTES, 1)):
            data, sel_phase, sel_offset = encode(mask, sel_bits, where, value=0x02)
            s_at = sels.add(data, sel_phase)
            for li, o in enumerate(layouts):
                for grid in (1, 3, None):
                    k = batch.add(MODES[i % 4], wants[li][0], wants[li][1], (phase, sel_bits, where, li, grid), with_selected=bool(i % 5))
                    calls.append((k, a_at, s_at, sel_offset, sel_bits, li, grid))
                    i += 1
    arrays.upload(), sels.upload(), offs.upload()
    batch.upload()
    for k, a_at, s_at, sel_offset, sel_bits, li, grid in calls:
        nseg = layouts[li].size - 1
        if grid is None:
            device_entry(hip, arrays.ptr(a_at), n, offs.ptr(o_at[li]), nseg, sels.ptr(s_at), sel_offset, sel_bits, batch, k)
        else:
            rc = launcher(arrays.ptr(a_at), sels.ptr(s_at), sel_offset, sel_bits, 0, n, offs.ptr(o_at[li]), nseg, batch.out(k),
                          batch.selected(k), batch.mode(k), grid, None)
            assert rc == 0, (batch.items[k][5], rc)
    batch.check()


# ------------------------------------------------------------------ 4. chain, epochs and regime changes
N_CHAIN = 1200 * U + 77           # grid 1: four writers of 300 units each


def chain_layout(w, n):
    """writer 0: three units that belong to no segment (skipped unread), a segment that starts mid-unit, runs the chain for 257
    units and ends mid-unit (per flag -> chain -> per flag), short segments (per flag, one of them a whole unit and a bit: below
    min_units 2), a second chain run of 20 units, short segments again; then one segment across the seams of writers 0 | 1 | 2
    (a writer enters the chain straight from its first unit) and a rest"""
    g = lambda k: k * U - w.lo0                                # array index of unit boundary k  # noqa: E731
    o = [g(3) + 5, g(261) + 100, g(261) + 103, g(262) + 7, g(262) + 7, g(264) - 1, g(284) + 9, g(284) + 12, g(285) + 500,
         g(700) - 9, n - 1]
    o = np.array(o, dtype=np.int64)
    assert (np.diff(o) >= 0).all() and o[-1] <= n
    return o


@pytest.mark.parametrize("sel_offset", [3, 0])
def test_chain_epochs_and_regime_changes(hip, launcher, sel_offset):
    """grid 1 over 1200 units of flags of period 65,521 under a mask of period 8,191, array phase 3: bit offset 3 puts the bitmap on
    a byte boundary of the grid (shift 0), bit offset 0 funnels it (shift 5).  All four modes over garbage / bias"""
    import torch
    n = N_CHAIN
    pattern = np.random.RandomState(405).randint(0, 65536, P).astype(np.uint16)
    mask_pattern = np.random.RandomState(406).randint(0, 2, 8191).astype(bool)
    values, mask = np.resize(pattern, n), np.resize(mask_pattern, n)
    slab = torch.full((n + 16,), -1, dtype=torch.int16, device="cuda")
    slab[3:3 + n] = dev16(values)
    ptr = slab.data_ptr() + 2 * 3
    w = writer_ranges(ptr % 16, n, 1)
    assert w.waves == 4 and w.lo0 == 3 and ((sel_offset + 8 - w.lo0) & 7 == 0) == (sel_offset == 3)
    o = chain_layout(w, n)
    pieces = w.pieces(o)
    w0 = pieces["writer"] == 0
    chains0 = pieces["chain"][w0]
    run = [int(c) for c in chains0]
    assert 257 in run and 20 in run and run.index(257) < run.index(20) and 0 in run[run.index(257) + 1:run.index(20)], run
    big = (pieces["chain"] == 257) & w0
    assert (pieces["head"][big] > 0).all() and (pieces["tail"][big] > 0).all() and pieces["plain"][big].all() and 257 > SEG_EPOCH
    assert ((pieces["chain"] > SEG_EPOCH) & ~pieces["plain"]).any() and ((pieces["chain"] > 0) & (pieces["head"] == 0)).any()
    assert (w0 & (pieces["chain"] == 0) & (pieces["e"] - pieces["b"] > U + 7)).any()     # a whole unit below min_units: per flag
    assert o[0] >= 3 * U                                          # units 0-2 are skipped unread
    want_rows, want_sel = swo.want(values, o, mask, superset=True)
    assert (want_sel[np.diff(o) > 50] > 0).all() and (want_sel < np.diff(o).astype(np.uint64)).any()
    d_sel = torch.full((16 + (n + 7) // 8 + 1 + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    bits = pack(mask, sel_offset, fill=1)
    d_sel[16:16 + bits.size] = dev8(bits)
    d_off = dev64(o)
    batch = Batch()
    ks = [batch.add(mode, want_rows, want_sel, (sel_offset, mode)) for mode in MODES]
    batch.upload()
    with policy(hip, 2):
        for k in ks:
            rc = launcher(ptr, d_sel.data_ptr() + 16, sel_offset, BITMAP, 0, n, d_off.data_ptr(), o.size - 1, batch.out(k),
                          batch.selected(k), batch.mode(k), 1, None)
            assert rc == 0, rc
        batch.check()
    del slab, d_sel


# ------------------------------------------------------------------ 5. every min_units through the public entries
def test_every_min_units_through_the_public_entries(hip, launcher):
    """the segments policy's chain threshold 0, 1, 2, 3, 255, 256 and 0xFFFFFFFF (per flag everywhere) under the device entry, the
    _sync form and the host form, bitmap (bit offset 5) and bytes in turn: the same rows and counts under every one"""
    import torch
    from libflagstats_amd import segments_where as sw
    n = (1 << 24) + 4099          # four units per writer at one workgroup per CU of 256 CUs
    pattern = np.random.RandomState(407).randint(0, 65536, P).astype(np.uint16)
    mask_pattern = np.random.RandomState(408).randint(0, 3, 13) > 0
    x, m = np.resize(pattern, n), np.resize(mask_pattern, n)
    t = dev16(x)
    bits = pack(m, 5, fill=1)
    d_bits, d_mask = dev8(bits), torch.from_numpy(m).cuda()
    rng = np.random.RandomState(19)
    lengths = rng.choice([3, 100, 4095, 4097, 2 * U + 5, 3 * U, 17 * U - 1, 300_007, 1_000_003], 40)
    o = np.concatenate([[13], 13 + np.cumsum(lengths)])
    o = np.append(o[o < n - 7], n - 7).astype(np.int64)
    d_off = dev64(o)
    cus = hip.FLAGSTATS_hip_compute_units()
    for i, mu in enumerate(EVERY_MIN_UNITS):
        sup = bool(i % 2)
        packed = i % 3 != 1
        want_rows, want_sel = swo.periodic_want(pattern, o, mask_pattern, superset=sup)
        chain = writer_ranges(t.data_ptr() % 16, n, cus).pieces(o, mu)["chain"]
        assert (chain.max() > 0) == (mu <= 3), (mu, chain.max())
        kw = {"where": d_bits, "packed": True, "bit_offset": 5} if packed else {"where": d_mask}
        with policy(hip, mu):
            for store in (True, False):
                rows = torch.full((o.size - 1, 32), GARBAGE if store else BIAS, dtype=torch.int64, device="cuda")
                sel = torch.full((o.size - 1,), GARBAGE if store else SEL_BIAS, dtype=torch.int64, device="cuda")
                sw.count_segments_torch_where(t, d_off, out=rows, selected=sel, store=store, superset=sup, **kw)
                torch.cuda.synchronize()
                w_rows, w_sel = expect(want_rows, want_sel, (STORE if store else 0) | SUPERSET)   # (want_rows has no superset slots unless sup)
                assert np.array_equal(u64(rows), w_rows), ("device", mu, store)
                assert np.array_equal(u64(sel), w_sel), ("device", mu, store)
            got = sw.count_segments_device_ptr_where(t.data_ptr(), n, o, d_bits.data_ptr() if packed else d_mask.data_ptr(),
                                                     1 if packed else 8, sel_offset=5 if packed else 0, superset=sup)
            assert np.array_equal(got[0], want_rows) and np.array_equal(got[1], want_sel), ("sync", mu)
            got = sw.counters_segments_where(x, o, bits if packed else m, packed=packed, bit_offset=5 if packed else 0, superset=sup)
            assert np.array_equal(got[0], want_rows) and np.array_equal(got[1], want_sel), ("host", mu)


# ------------------------------------------------------------------ 6. densities and byte values
def test_densities_and_byte_values(hip, launcher):
    """an all-zero mask (store: rows and counts read 0; +=: untouched), an all-ones mask (the plain segmented rows, the lengths
    as counts), and the byte form with bytes 0x01, 0x02, 0x80 and 0xFF (select) against 0x00, in per-flag pieces and chain runs"""
    n = 7 * U + 100
    rng = np.random.RandomState(61)
    values = rng.randint(0, 65536, n).astype(np.uint16)
    o = np.array([1, 600, 2 * U - 1 + 5, 6 * U, n - 256, n - 2], dtype=np.int64)
    nseg = o.size - 1
    w = writer_ranges(2, n, 1)
    pieces = w.pieces(o)
    assert (pieces["chain"] > 0).any() and (pieces["chain"] == 0).any()
    byte_vals = np.array([0x00, 0x01, 0x02, 0x80, 0xFF, 0x00], dtype=np.uint8)[rng.randint(0, 6, n)]
    for k in np.nonzero(pieces["chain"] > 0)[0]:                 # every chain run sees every byte value
        b = int(pieces["b"][k] + pieces["head"][k])
        assert set(byte_vals[b:b + int(pieces["chain"][k]) * U].tolist()) == {0x00, 0x01, 0x02, 0x80, 0xFF}
    assert set(byte_vals[1:600].tolist()) == {0x00, 0x01, 0x02, 0x80, 0xFF}
    none, every = np.zeros(n, dtype=bool), np.ones(n, dtype=bool)
    want_none = swo.want(values, o, none, superset=True)
    want_all = swo.want(values, o, every, superset=True)
    want_vals = swo.want(values, o, byte_vals != 0, superset=True)
    assert not want_none[0].any() and not want_none[1].any()
    assert np.array_equal(want_all[0], segmented_counters(values, o, superset=True)) and np.array_equal(want_all[1], np.diff(o).astype(np.uint64))
    assert int(want_vals[1].sum()) == int((byte_vals[1:n - 2] != 0).sum())
    arrays, sels = Arena(np.uint16, POISON), Arena(np.uint8, 0xFF, pad=16)
    a_at = arrays.add(values, 1)
    cases = []
    for mask, want, name in ((none, want_none, "none"), (every, want_all, "all")):
        for sel_bits, where in ((BITMAP, 0), (BITMAP, 6), (BYTES, 3)):
            data, sel_phase, sel_offset = encode(mask, sel_bits, where, value=0xFF)
            if name == "none" and sel_bits == BITMAP:
                assert not np.unpackbits(data, bitorder="little")[where:where + n].any()
            cases.append((sels.add(data, sel_phase), sel_offset, sel_bits, want, name))
    cases.append((sels.add(byte_vals, 5), 0, BYTES, want_vals, "byte values"))
    d_off = dev64(o)
    batch, calls = Batch(), []
    for s_at, sel_offset, sel_bits, want, name in cases:
        for mode in MODES:
            for grid in (1, None):
                calls.append((batch.add(mode, want[0], want[1], (name, sel_bits, sel_offset, mode, grid)), s_at, sel_offset, sel_bits, grid))
    arrays.upload(), sels.upload()
    batch.upload()
    assert arrays.ptr(a_at) % 16 == 2
    for k, s_at, sel_offset, sel_bits, grid in calls:
        if grid is None:
            device_entry(hip, arrays.ptr(a_at), n, d_off.data_ptr(), nseg, sels.ptr(s_at), sel_offset, sel_bits, batch, k)
        else:
            assert launcher(arrays.ptr(a_at), sels.ptr(s_at), sel_offset, sel_bits, 0, n, d_off.data_ptr(), nseg, batch.out(k),
                            batch.selected(k), batch.mode(k), grid, None) == 0
    batch.check()


# ------------------------------------------------------------------ 7. equivalences
def test_equivalences(hip, launcher):
    """nseg == 1 over the whole array is FLAGSTATS_hip_device_u16_where; an all-ones mask is FLAGSTATS_hip_device_u16_segments, bit
    for bit; the byte form is FLAGSTATS_hip_device_u16_segments_filter with min_mapq 1 and the mask as its column; the bitmap form
    is the byte form of the unpacked mask.  nseg == 0 touches nothing"""
    import torch
    n = 5 * U + 77
    rng = np.random.RandomState(53)
    values = rng.randint(0, 65536, n).astype(np.uint16)
    mask = rng.randint(0, 3, n) > 0
    byte_vals = (mask * rng.randint(1, 256, n)).astype(np.uint8)
    assert np.array_equal(byte_vals != 0, mask)
    t, d_bytes, d_ones = dev16(values), dev8(byte_vals), dev8(np.ones(n, dtype=np.uint8))
    bits = pack(mask, 3, fill=1)
    d_bits, d_ones_bits = dev8(bits), dev8(np.full((n + 7) // 8 + 1, 0xFF, dtype=np.uint8))
    o = np.array([5, 5, 300, U + 1, 4 * U, n + 1000, n + 5000], dtype=np.int64)     # the last two run past the array
    d_off = dev64(o)
    nseg = o.size - 1
    whole = dev64(np.array([0, n]))
    sw_entry = hip.FLAGSTATS_hip_device_u16_segments_where

    def fresh(words):
        return torch.full((words,), BIAS, dtype=torch.int64, device="cuda")

    for mode in MODES:
        # one segment [0, n): the where entry, both encodings
        for sel, off, sb in ((d_bits, 3, BITMAP), (d_bytes, 0, BYTES)):
            a, b = fresh(33), fresh(33)
            assert hip.FLAGSTATS_hip_device_u16_where(t.data_ptr(), n, sel.data_ptr(), off, sb, a.data_ptr(), a.data_ptr() + 256, mode, None) == 0, err(hip)
            assert sw_entry(t.data_ptr(), n, whole.data_ptr(), 1, sel.data_ptr(), off, sb, b.data_ptr(), b.data_ptr() + 256, mode, None) == 0, err(hip)
            torch.cuda.synchronize()
            assert torch.equal(a, b) and int(b[32]) not in (0, BIAS), (mode, sb)
        # an all-ones mask: the plain segmented entry, and the clamped lengths as counts
        plain = fresh(nseg * 32)
        assert hip.FLAGSTATS_hip_device_u16_segments(t.data_ptr(), n, d_off.data_ptr(), nseg, plain.data_ptr(), mode, None) == 0, err(hip)
        lengths = np.diff(np.clip(o, 0, n)).astype(np.uint64) + np.uint64(0 if mode & 1 else BIAS)
        for sel, sb in ((d_ones_bits, BITMAP), (d_ones, BYTES)):
            rows = fresh(nseg * 33)
            assert sw_entry(t.data_ptr(), n, d_off.data_ptr(), nseg, sel.data_ptr(), 0, sb, rows.data_ptr(), rows.data_ptr() + nseg * 256, mode, None) == 0, err(hip)
            torch.cuda.synchronize()
            assert torch.equal(rows[:nseg * 32], plain), (mode, sb)
            assert np.array_equal(u64(rows[nseg * 32:]), lengths), (mode, sb)
        # the byte form: the filtered segmented entry with the mask as its MAPQ column; the bitmap form: the byte form
        f, by, bi = fresh(nseg * 33), fresh(nseg * 33), fresh(nseg * 33)
        assert hip.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), n, d_off.data_ptr(), nseg, 0, 0, d_bytes.data_ptr(), 1, f.data_ptr(),
                                                            f.data_ptr() + nseg * 256, mode, None) == 0, err(hip)
        assert sw_entry(t.data_ptr(), n, d_off.data_ptr(), nseg, d_bytes.data_ptr(), 0, BYTES, by.data_ptr(), by.data_ptr() + nseg * 256, mode, None) == 0, err(hip)
        assert sw_entry(t.data_ptr(), n, d_off.data_ptr(), nseg, d_bits.data_ptr(), 3, BITMAP, bi.data_ptr(), bi.data_ptr() + nseg * 256, mode, None) == 0, err(hip)
        torch.cuda.synchronize()
        assert torch.equal(f, by) and torch.equal(by, bi), mode
    # the rows themselves against the oracle (all the kernels could be wrong alike)
    want_rows, want_sel = swo.want(values, np.clip(o, 0, n), mask, superset=True)
    w = expect(want_rows, want_sel, MODES[-1])
    assert np.array_equal(u64(bi[:nseg * 32]).reshape(nseg, 32), w[0]) and np.array_equal(u64(bi[nseg * 32:]), w[1] - np.uint64(SEL_BIAS - BIAS))
    # nseg == 0 touches nothing; NULL selected in the synchronous forms
    assert sw_entry(t.data_ptr(), n, None, 0, d_bits.data_ptr(), 3, BITMAP, None, None, STORE, None) == 0
    assert hip.FLAGSTATS_hip_u16_x64_segments_where(values.ctypes.data, n, None, 0, bits.ctypes.data, 3, BITMAP, None, None, STORE) == 0
    o2 = np.array([0, 100, 2 * U + 3, n], dtype=np.uint64)
    want_rows, want_sel = swo.want(values, o2, mask, superset=True)
    for entry, src, s_src in ((hip.FLAGSTATS_hip_device_u16_segments_where_sync, t.data_ptr(), d_bits.data_ptr()),
                              (hip.FLAGSTATS_hip_u16_x64_segments_where, values.ctypes.data, bits.ctypes.data)):
        for mode in MODES:
            rows = np.full((3, 32), GARBAGE if mode & 1 else BIAS, dtype=np.uint64)
            assert entry(src, n, o2.ctypes.data, 3, s_src, 3, BITMAP, rows.ctypes.data, None, mode) == 0, err(hip)
            assert np.array_equal(rows, expect(want_rows, want_sel, mode)[0]), mode


# ------------------------------------------------------------------ 8. atomics
def test_three_streams_add_into_one_set_of_rows(hip):
    import torch
    from libflagstats_amd import segments_where as sw
    rng = np.random.RandomState(73)
    o = np.array([0, 50, 3 * U + 1, 3 * U + 1, 20 * U - 7, 36 * U], dtype=np.int64)
    nseg = o.size - 1
    d_off = dev64(o)
    rows = torch.zeros((nseg, 32), dtype=torch.int64, device="cuda")
    sel = torch.zeros(nseg, dtype=torch.int64, device="cuda")
    total_rows, total_sel = np.zeros((nseg, 32), dtype=np.uint64), np.zeros(nseg, dtype=np.uint64)
    inputs = []
    for n, packed, bit_offset, density in ((36 * U + 11, True, 0, 50), (30 * U + 5, True, 5, 90), (40 * U - 3, False, 0, 10)):
        values = rng.randint(0, 65536, n).astype(np.uint16)
        mask = rng.randint(0, 100, n) < density
        w_rows, w_sel = swo.want(values, np.clip(o, 0, n), mask, superset=True)
        assert w_sel.any()
        total_rows += w_rows
        total_sel += w_sel
        where = dev8(pack(mask, bit_offset, fill=1)) if packed else torch.from_numpy(mask).cuda()
        inputs.append((dev16(values), where, packed, bit_offset))
    streams = [torch.cuda.Stream() for _ in inputs]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    for st, (t, where, packed, bit_offset) in zip(streams, inputs):
        with torch.cuda.stream(st):
            sw.count_segments_torch_where(t, d_off, where, packed=packed, bit_offset=bit_offset, out=rows, selected=sel, store=False,
                                          superset=True)
    for st in streams:
        st.synchronize()
    assert np.array_equal(u64(rows), total_rows) and np.array_equal(u64(sel), total_sel)


# ------------------------------------------------------------------ 9. host form across chunks
def test_host_form_across_chunks(hip):
    """chunks of 8,193 flags from offsets[0] = 3 on: with bit offset 6 the seven chunks begin 1, 2, .. 7 bits into a selection byte
    (with bit offset 0: at 3, 4, .. 7, 0 and 1), the byte form's slices begin at odd and even bytes; segments span several chunks;
    flags in front of offsets[0] and behind offsets[nseg] are poison whose bits and bytes are set and never cross the bus"""
    from libflagstats_amd import _lib
    from libflagstats_amd import segments_where as sw
    n = 6 * 8193 + 77
    rng = np.random.RandomState(89)
    values = rng.randint(0, 65536, n + 1).astype(np.uint16)[1:]
    mask = rng.randint(0, 2, n).astype(bool)
    o = np.array([3, 10, 10, 8193 + 2, 3 * 8193 + 500, 3 * 8193 + 501, 5 * 8193 + 3, n - 20], dtype=np.int64)
    values[:3], values[n - 20:], mask[:3], mask[n - 20:] = POISON, POISON, True, True
    assert {(6 + 3 + k * 8193) & 7 for k in range(7)} == set(range(1, 8)) and (n - 20 - 3) // 8193 == 6
    byte_mask = np.concatenate([[0xFF], mask.astype(np.uint8) * 0x80]).astype(np.uint8)[1:]      # one byte into its buffer
    encodings = [(pack(mask, 6, fill=1), True, 6), (pack(mask, 0, fill=1), True, 0), (mask, False, 0)]
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", 8193), "chunk_flags")
        for where, packed, bit_offset in encodings:
            for sup in (False, True):
                want_rows, want_sel = swo.want(values, o, mask, superset=sup)
                assert want_sel.any() and (want_sel < np.diff(o).astype(np.uint64)).any()
                got = sw.counters_segments_where(values, o, where, packed=packed, bit_offset=bit_offset, superset=sup)
                assert np.array_equal(got[0], want_rows) and np.array_equal(got[1], want_sel), (packed, bit_offset, sup)
            want_rows, want_sel = swo.want(values, o, mask, superset=True)
            src = where if packed else byte_mask
            o64 = o.astype(np.uint64)
            for flags in (0, SUPERSET):                  # += over bias words
                rows = np.full((o.size - 1, 32), BIAS, dtype=np.uint64)
                sel = np.full(o.size - 1, SEL_BIAS, dtype=np.uint64)
                rc = hip.FLAGSTATS_hip_u16_x64_segments_where(values.ctypes.data, n, o64.ctypes.data, o.size - 1, src.ctypes.data,
                                                              bit_offset, 1 if packed else 8, rows.ctypes.data, sel.ctypes.data, flags)
                assert rc == 0, err(hip)
                w = expect(want_rows, want_sel, flags)
                assert np.array_equal(rows, w[0]) and np.array_equal(sel, w[1]), (packed, bit_offset, flags)
            # one chunk only (a single staging slot), and segments that cover nothing
            for oo in (np.array([1, 50, 99]), np.array([7, 7, 7]), np.array([n, n])):
                got = sw.counters_segments_where(values, oo, where, packed=packed, bit_offset=bit_offset)
                want = swo.want(values, oo, mask)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), oo
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old
    got = sw.counters_segments_where(values[:0], [0, 0], mask[:0])
    assert got[0].shape == (1, 32) and not got[0].any() and not got[1].any()
    got = sw.count_segments_device_ptr_where(0, 0, [0, 0, 0], 0, 1)
    assert got[0].shape == (2, 32) and not got[0].any() and not got[1].any()


# ------------------------------------------------------------------ 10. refusals
def test_refusals(hip, launcher):
    """every refusal of the C entries, the launcher and what the Python layer can refuse only with a device at hand: each is an
    argument check that returns before anything is launched, and rows and counts stay as they were.  Nothing here reads past an
    allocation: the short allocations are refused by the extent check"""
    import torch
    from libflagstats_amd import segments_where as sw
    n, nseg = 4096, 3
    t = torch.zeros(n + 8, dtype=torch.int16, device="cuda")
    m8 = torch.ones(n + 8, dtype=torch.uint8, device="cuda")
    o = np.array([0, 10, 2000, n], dtype=np.uint64)
    d_off = dev64(o)
    out = torch.full((nseg, 32), BIAS, dtype=torch.int64, device="cuda")
    sel = torch.full((nseg,), SEL_BIAS, dtype=torch.int64, device="cuda")
    h_out = np.full((nseg, 32), BIAS, dtype=np.uint64)
    h_sel = np.full(nseg, SEL_BIAS, dtype=np.uint64)
    host16 = np.zeros(n + 8, dtype=np.uint16)
    host8 = np.ones(n + 8, dtype=np.uint8)
    dev_entry = hip.FLAGSTATS_hip_device_u16_segments_where
    sync_entry = hip.FLAGSTATS_hip_device_u16_segments_where_sync
    host_entry = hip.FLAGSTATS_hip_u16_x64_segments_where

    def untouched(what):
        torch.cuda.synchronize()
        assert (out == BIAS).all() and (sel == SEL_BIAS).all(), what
        assert (h_out == BIAS).all() and (h_sel == SEL_BIAS).all(), what

    def refused(what, text, d_array=t.data_ptr(), n_=n, offsets=o, nseg_=nseg, d_sel=m8.data_ptr(), sel_offset=0, sel_bits=(1, 8), flags=0,
                rows=True, forms=("device", "sync", "host")):
        d_o = None if offsets is None else dev64(offsets.astype(np.int64))
        for sb in sel_bits:
            for form in forms:
                if form == "device":
                    rc = dev_entry(d_array, n_, None if d_o is None else d_o.data_ptr(), nseg_, d_sel, sel_offset, sb,
                                   out.data_ptr() if rows else None, sel.data_ptr(), flags, None)
                elif form == "sync":
                    rc = sync_entry(d_array, n_, None if offsets is None else offsets.ctypes.data, nseg_, d_sel, sel_offset, sb,
                                    h_out.ctypes.data if rows else None, h_sel.ctypes.data, flags)
                else:
                    src = host16.ctypes.data + (d_array - t.data_ptr()) if d_array else None
                    rc = host_entry(src, n_, None if offsets is None else offsets.ctypes.data, nseg_, host8.ctypes.data if d_sel else None,
                                    sel_offset, sb, h_out.ctypes.data if rows else None, h_sel.ctypes.data, flags)
                assert rc != 0, (what, form, sb)
                assert text in err(hip), (what, form, sb, err(hip))
        untouched(what)

    refused("sel_bits", "sel_bits must be 1 (an LSB-first bitmap) or 8 (one byte per element)", sel_bits=(0, 2, 4, 16, -1))
    refused("an extra flag bit", "no other bits", flags=4)
    refused("NULL rows", "with nseg > 0", rows=False)
    refused("NULL offsets", "with nseg > 0", offsets=None)
    refused("NULL array", "NULL array with n > 0", d_array=None)
    refused("NULL selection", "NULL selection with n > 0", d_sel=None)
    refused("an odd array address", "2-byte aligned", d_array=t.data_ptr() + 1)
    refused("n * 2 is no size", "n * 2 is not a size", n_=1 << 63)
    refused("sel_offset + n is no index", "sel_offset + n is not an index", sel_offset=(1 << 64) - 5)
    refused("too many segments", "nseg is too large", nseg_=1 << 60)
    refused("decreasing offsets", "offsets must be non-decreasing", offsets=np.array([0, 20, 10, n], dtype=np.uint64), forms=("sync", "host"))
    refused("offsets past the array", "exceeds the array's", offsets=np.array([0, 10, 20, n + 1], dtype=np.uint64), forms=("sync", "host"))
    # the selection somewhere else than the array: in host memory, a CPU tensor in Python
    rc = dev_entry(t.data_ptr(), n, d_off.data_ptr(), nseg, host8.ctypes.data, 0, 8, out.data_ptr(), sel.data_ptr(), 0, None)
    assert rc != 0 and "d_sel" in err(hip), err(hip)
    rc = sync_entry(t.data_ptr(), n, o.ctypes.data, nseg, host8.ctypes.data, 0, 8, h_out.ctypes.data, h_sel.ctypes.data, 0)
    assert rc != 0 and "d_sel" in err(hip), err(hip)
    tt = t[:n]
    cpu = {"offsets": torch.zeros(4, dtype=torch.int64), "where": torch.zeros(n, dtype=torch.bool),
           "out": torch.zeros((3, 32), dtype=torch.int64), "selected": torch.zeros(3, dtype=torch.int64)}
    for name, x in cpu.items():
        args, kw = [tt, d_off, m8[:n].bool()], {}
        if name == "offsets":
            args[1] = x
        elif name == "where":
            args[2] = x
        else:
            kw[name] = x
        with pytest.raises(ValueError, match=r"%s must live on t's device \(cuda:0\), not on cpu" % name):
            sw.count_segments_torch_where(*args, **kw)
    untouched("selection elsewhere")
    # host pointers (pageable, then page-locked) as d_out, d_selected, d_offsets
    rc = dev_entry(t.data_ptr(), n, d_off.data_ptr(), nseg, m8.data_ptr(), 0, 8, h_out.ctypes.data, sel.data_ptr(), 0, None)
    assert rc != 0 and "d_out" in err(hip), err(hip)
    rc = dev_entry(t.data_ptr(), n, d_off.data_ptr(), nseg, m8.data_ptr(), 0, 8, out.data_ptr(), h_sel.ctypes.data, 0, None)
    assert rc != 0 and "d_selected" in err(hip), err(hip)
    rc = dev_entry(t.data_ptr(), n, o.ctypes.data, nseg, m8.data_ptr(), 0, 8, out.data_ptr(), sel.data_ptr(), 0, None)
    assert rc != 0 and "d_offsets" in err(hip), err(hip)
    pinned = hip.FLAGSTATS_hip_host_alloc(1024)
    assert pinned
    try:
        ctypes.memset(pinned, 0, 1024)
        rc = dev_entry(t.data_ptr(), n, d_off.data_ptr(), nseg, m8.data_ptr(), 0, 1, pinned, sel.data_ptr(), STORE, None)
        assert rc != 0 and "d_out must be device memory" in err(hip), err(hip)
        rc = dev_entry(t.data_ptr(), n, d_off.data_ptr(), nseg, m8.data_ptr(), 0, 1, out.data_ptr(), pinned, STORE, None)
        assert rc != 0 and "d_selected must be device memory" in err(hip), err(hip)
        assert not any(ctypes.string_at(pinned, 1024))
    finally:
        hip.FLAGSTATS_hip_host_free(pinned)
    untouched("host pointers")
    # a stream of another device cannot be made on a one-GPU box; extents: the selection one byte short of the last byte that
    # holds an element's bit or byte (both encodings, also behind a sel_offset), the array one flag short, rows, counts and offsets
    # 8 bytes short
    nbytes = 2 << 20
    raw = hip.FLAGSTATS_hip_device_alloc(nbytes)
    big = torch.zeros(8 * nbytes + 8, dtype=torch.int16, device="cuda")
    assert raw
    try:
        assert hip.FLAGSTATS_hip_memcpy_h2d(raw, np.zeros(nbytes, dtype=np.uint8).ctypes.data, nbytes) == 0
        big_off = dev64(np.array([0, 5, 100, 1000]))
        h_big_off = np.array([0, 5, 100, 1000], dtype=np.uint64)
        for sb, n_, off in ((8, nbytes + 1, 0), (8, nbytes - 6, 7), (1, 8 * nbytes + 1, 0), (1, 8 * nbytes - 2, 3)):
            rc = dev_entry(big.data_ptr(), n_, big_off.data_ptr(), nseg, raw, off, sb, out.data_ptr(), sel.data_ptr(), STORE, None)
            assert rc != 0 and "d_sel" in err(hip) and "1 bytes short" in err(hip), (sb, n_, off, err(hip))
            rc = sync_entry(big.data_ptr(), n_, h_big_off.ctypes.data, nseg, raw, off, sb, h_out.ctypes.data, h_sel.ctypes.data, STORE)
            assert rc != 0 and "d_sel" in err(hip) and "1 bytes short" in err(hip), (sb, n_, off, err(hip))
        rc = dev_entry(raw, nbytes // 2 + 1, big_off.data_ptr(), nseg, m8.data_ptr(), 0, 1, out.data_ptr(), sel.data_ptr(), STORE, None)
        assert rc != 0 and "d_array" in err(hip) and "2 bytes short" in err(hip), err(hip)
        end = raw + nbytes
        for name, kw in (("d_out", {"rows": end - nseg * 256 + 8}), ("d_selected", {"counts": end - nseg * 8 + 8}),
                         ("d_offsets", {"offsets": end - (nseg + 1) * 8 + 8})):
            rc = dev_entry(t.data_ptr(), n, kw.get("offsets", d_off.data_ptr()), nseg, m8.data_ptr(), 0, 8, kw.get("rows", out.data_ptr()),
                           kw.get("counts", sel.data_ptr()), 0, None)
            assert rc != 0 and name in err(hip) and "8 bytes short" in err(hip), (name, err(hip))
        back = np.ones(nbytes, dtype=np.uint8)
        assert hip.FLAGSTATS_hip_memcpy_d2h(back.ctypes.data, raw, nbytes) == 0 and not back.any()
    finally:
        hip.FLAGSTATS_hip_device_free(raw)
    untouched("extents")
    # the launcher itself: other mode bits, no workgroups, a wave's uint32 totals, other encodings, NULLs -- nothing queued
    words = torch.full((nseg * 33,), BIAS, dtype=torch.int64, device="cuda")
    p, ps = words.data_ptr(), words.data_ptr() + nseg * 256
    a, c, f = t.data_ptr(), m8.data_ptr(), d_off.data_ptr()
    for sb in (1, 8):
        assert launcher(a, c, 0, sb, 0, 8, f, nseg, p, ps, 4, 1, None) != 0
        assert launcher(a, c, 0, sb, 0, 8, f, nseg, p, ps, STORE, 0, None) != 0
        assert launcher(a, c, 0, sb, 0, 1 << 35, f, nseg, p, ps, STORE, 1, None) != 0       # 2^33 flags per wave
        assert launcher(a, c, (1 << 64) - 5, sb, 0, 8, f, nseg, p, ps, STORE, 1, None) != 0
        assert launcher(a, None, 0, sb, 0, 8, f, nseg, p, ps, STORE, 1, None) != 0
        assert launcher(None, c, 0, sb, 0, 8, f, nseg, p, ps, STORE, 1, None) != 0
        assert launcher(a + 1, c, 0, sb, 0, 8, f, nseg, p, ps, STORE, 1, None) != 0
        assert launcher(a, c, 0, sb, 0, 8, None, nseg, p, ps, STORE, 1, None) != 0
        assert launcher(a, c, 0, sb, 0, 8, f, nseg, None, ps, STORE, 1, None) != 0
    assert launcher(a, c, 0, 2, 0, 8, f, nseg, p, ps, STORE, 1, None) != 0
    torch.cuda.synchronize()
    assert (words == BIAS).all()


# ------------------------------------------------------------------ 11. graph capture and replay
@pytest.mark.parametrize("error_mode", ["global", "thread_local"])
@pytest.mark.parametrize("layer", ["entry", "torch"])
def test_graph_capture_and_replay(hip, layer, error_mode):
    """one plain call, then the device entry (or count_segments_torch_where) captured with torch.cuda.graph -- its zeroes and its
    kernel, bitmap and byte form in one graph --, replayed, array / selection / offsets rewritten in place, replayed again: a
    replay counts what the buffers hold then"""
    import torch
    from libflagstats_amd import segments_where as sw
    rng = np.random.RandomState(71)
    n = 30 * U + 7
    nseg = 6
    sets = []
    for k in range(2):
        x = rng.randint(0, 65536, n).astype(np.uint16)
        m = rng.randint(0, 100, n) < 30 + 40 * k
        o = np.sort(np.concatenate([[3 + k], rng.randint(4, n - 5, nseg - 1), [n - 2 - k]])).astype(np.int64)
        sets.append((x, m, o, swo.want(x, o, m, superset=True)))
    assert not np.array_equal(sets[0][3][1], sets[1][3][1])
    t, d_off = dev16(sets[0][0]), dev64(sets[0][2])
    d_bits, d_mask = dev8(pack(sets[0][1], 3, fill=1)), torch.from_numpy(sets[0][1]).cuda()
    rows = torch.full((2, nseg, 32), GARBAGE, dtype=torch.int64, device="cuda")
    cnt = torch.full((2, nseg), GARBAGE, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    stream = ctypes.c_void_p(s.cuda_stream)

    def call():
        if layer == "torch":
            sw.count_segments_torch_where(t, d_off, d_bits, packed=True, bit_offset=3, out=rows[0], selected=cnt[0], store=True, superset=True)
            sw.count_segments_torch_where(t, d_off, d_mask, out=rows[1], selected=cnt[1], store=True, superset=True)
            return 0
        rc = hip.FLAGSTATS_hip_device_u16_segments_where(t.data_ptr(), n, d_off.data_ptr(), nseg, d_bits.data_ptr(), 3, BITMAP,
                                                         rows[0].data_ptr(), cnt[0].data_ptr(), STORE | SUPERSET, stream)
        return rc or hip.FLAGSTATS_hip_device_u16_segments_where(t.data_ptr(), n, d_off.data_ptr(), nseg, d_mask.data_ptr(), 0, BYTES,
                                                                 rows[1].data_ptr(), cnt[1].data_ptr(), STORE | SUPERSET, stream)

    def same(want, what):
        for enc in range(2):
            assert np.array_equal(u64(rows[enc]), want[0]) and np.array_equal(u64(cnt[enc]), want[1]), (layer, error_mode, what, enc)

    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert call() == 0, err(hip)
    torch.cuda.synchronize()
    same(sets[0][3], "plain")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode=error_mode):
        rc = call()
    assert rc == 0, err(hip)
    torch.cuda.synchronize()
    for x, m, o, want in (sets[0], sets[1], sets[0]):
        t.copy_(dev16(x))
        d_bits.copy_(dev8(pack(m, 3, fill=1)))
        d_mask.copy_(torch.from_numpy(m).cuda())
        d_off.copy_(dev64(o))
        rows.fill_(GARBAGE)
        cnt.fill_(GARBAGE)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        same(want, "replay")
    del g


# ------------------------------------------------------------------ 12. a seeded randomised sweep
def test_seeded_randomised_sweep(hip, launcher):
    """300 cases: n up to 3 units, random array phase, offsets (gaps in front and behind, empty segments), encoding, bit offset or
    byte alignment, byte values, density, mode, grid, presence of `selected`, and the chain threshold (0, 1 or 2, applied to a
    third of the cases each); all launched into one batch and read back once"""
    rng = np.random.RandomState(20261)
    arrays, sels, offs = Arena(np.uint16, POISON), Arena(np.uint8, 0xFF, pad=16), Arena(np.int64, 0, pad=0)
    batch, calls = Batch(), []
    for i in range(300):
        n = int(rng.choice([rng.randint(1, 64), rng.randint(64, U + 64), rng.randint(U, 3 * U + 1)]))
        phase = int(rng.randint(0, 8))
        values = rng.randint(0, 65536, n).astype(np.uint16)
        density = int(rng.choice([0, 1, 10, 50, 90, 99, 100]))
        mask = rng.randint(0, 100, n) < density
        nseg = int(rng.randint(1, 12))
        cuts = np.sort(rng.randint(0, n + 1, nseg + 1))
        if rng.randint(0, 3) == 0:
            cuts[rng.randint(0, nseg + 1)] = cuts[rng.randint(0, nseg + 1)]           # an empty segment (sorted again below)
        o = np.sort(cuts).astype(np.int64)
        values[:o[0]], values[o[-1]:] = POISON, POISON
        mask[:o[0]], mask[o[-1]:] = True, True
        sel_bits = BITMAP if rng.randint(0, 3) else BYTES
        where = int(rng.randint(0, 8) if sel_bits == BITMAP else rng.randint(0, 16))
        data, sel_phase, sel_offset = encode(mask, sel_bits, where, value=int(rng.randint(1, 256)))
        want_rows, want_sel = swo.want(values, o, mask, superset=True)
        mode = int(rng.randint(0, 4))
        k = batch.add(mode, want_rows, want_sel, (i, n, phase, o.tolist(), sel_bits, where, density), with_selected=bool(rng.randint(0, 4)))
        calls.append((k, arrays.add(values, phase), n, sels.add(data, sel_phase), sel_offset, sel_bits, offs.add(o), nseg, int(rng.randint(1, 4)), i % 3))
    arrays.upload(), sels.upload(), offs.upload()
    batch.upload()
    for mu in (0, 1, 2):
        with policy(hip, mu):
            for k, a_at, n, s_at, sel_offset, sel_bits, o_at, nseg, grid, which in calls:
                if which != mu:
                    continue
                rc = launcher(arrays.ptr(a_at), sels.ptr(s_at), sel_offset, sel_bits, 0, n, offs.ptr(o_at), nseg, batch.out(k),
                              batch.selected(k), batch.mode(k), grid, None)
                assert rc == 0, (batch.items[k][5], rc)
    batch.check()
