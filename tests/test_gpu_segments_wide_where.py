"""Selected-elements segmented flagstat of int32 / int64 columns on the MI355X (csrc/flagstat_segments_wide_where.hip and the layers
above it): rows, the number of selected elements and one high-bit mask of the SELECTED elements per segment, against
tests/segments_wide_where_oracle.py; every comparison is exact.

Expected values never come from the code under test.  Poison elements (low bits 0xFFFF, every high bit set) lie in every
unselected slot, around the array, in front of offsets[0] and behind offsets[nseg]; their bits or bytes are SET where they lie
outside every segment and CLEAR where they are unselected slots; unused bits of a bitmap's first and last byte are set.  Direct
launches (fsk_launch_segments_wide_where with a small grid) are placed with segments_wide_oracle.WideWriterSplit, and every case
asserts from the oracle that its input holds what it is there for."""
import contextlib
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_wide_oracle as swo  # noqa: E402
import segments_wide_where_oracle as swwo  # noqa: E402
from segments_wide_where_oracle import BITMAP, BYTES, pack, poison  # noqa: E402

pytestmark = pytest.mark.gpu

STORE, SUPERSET = 1, 2
MODES = (1, 0, 3, 2)             # store, +=, store + superset, += + superset
GARBAGE, BIAS, SEL_BIAS, MASK_BIAS = 0x5EED_0000_0BAD, 3, 5, (1 << 48) | (1 << 17)
EVERY_MIN_UNITS = (0, 1, 2, 3, 255, 256, 0xFFFFFFFF)   # tests/test_gpu_segments_regimes.py's list
NEVER = 0xFFFFFFFF               # min_units: no chain
P = 65_521                       # prime: no vector, row, unit or writer seam is a multiple of the period
SIGNED = {4: np.int32, 8: np.int64}
UNSIGNED = {4: np.uint32, 8: np.uint64}
WIDTHS = (4, 8)


def err(hip):
    return hip.FLAGSTATS_hip_last_error().decode(errors="replace")


def dev(x):
    """the array on the device (torch has signed tensors of every width: the bytes are what counts)"""
    import torch
    x = np.ascontiguousarray(x)
    if x.dtype == bool:
        return torch.from_numpy(x).cuda()
    return torch.from_numpy(x.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[x.dtype.itemsize])).cuda()


def dev64(o):
    import torch
    return torch.from_numpy(np.ascontiguousarray(o, dtype=np.int64)).cuda()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def expect(want, mode):
    """what a call in `mode` must leave in rows / counts / masks prefilled with GARBAGE (store) or BIAS / SEL_BIAS / MASK_BIAS
    (+=), given the oracle's superset triple"""
    w = want[0].copy()
    if not mode & SUPERSET:
        w[:, [0, 9, 16]] = 0
    if mode & STORE:
        return w, want[1].copy(), want[2].copy()
    return w + np.uint64(BIAS), want[1] + np.uint64(SEL_BIAS), want[2] | np.uint64(MASK_BIAS)


def same(got, want, what):
    rows, sel, high = got
    bad = np.nonzero((rows != want[0]).any(axis=1))[0]
    assert bad.size == 0, (what, "rows", bad[:8], rows[bad[:2]], want[0][bad[:2]])
    bad = np.nonzero(sel != want[1])[0]
    assert bad.size == 0, (what, "selected", bad[:8], sel[bad[:8]], want[1][bad[:8]])
    bad = np.nonzero(high != want[2])[0]
    assert bad.size == 0, (what, "masks", bad[:8], [hex(int(v)) for v in high[bad[:4]]], [hex(int(v)) for v in want[2][bad[:4]]])


class Batch:
    """device words for many launches -- per launch nseg rows of 32, then nseg counts, then nseg masks -- prefilled in one copy
    (GARBAGE for store, BIAS / SEL_BIAS / MASK_BIAS for +=) and read back in one copy after every launch has been queued"""

    def __init__(self):
        self.items, self.words, self.t = [], 0, None

    def add(self, mode, want, note, with_selected=True, with_high=True):
        nseg = want[0].shape[0]
        self.items.append((self.words, nseg, mode, want, note, with_selected, with_high))
        self.words += nseg * 34
        return len(self.items) - 1

    def upload(self):
        import torch
        host = np.empty(max(self.words, 1), dtype=np.uint64)
        for at, nseg, mode, _, _, _, _ in self.items:
            store = bool(mode & STORE)
            host[at:at + nseg * 32] = GARBAGE if store else BIAS
            host[at + nseg * 32:at + nseg * 33] = GARBAGE if store else SEL_BIAS
            host[at + nseg * 33:at + nseg * 34] = GARBAGE if store else MASK_BIAS
        self.host = host
        self.t = torch.from_numpy(host.view(np.int64)).cuda()
        torch.cuda.synchronize()

    def mode(self, k):
        return self.items[k][2]

    def nseg(self, k):
        return self.items[k][1]

    def out(self, k):
        return self.t.data_ptr() + 8 * self.items[k][0]

    def selected(self, k):
        at, nseg = self.items[k][:2]
        return self.t.data_ptr() + 8 * (at + nseg * 32) if self.items[k][5] else None

    def high(self, k):
        at, nseg = self.items[k][:2]
        return self.t.data_ptr() + 8 * (at + nseg * 33) if self.items[k][6] else None

    def check(self):
        import torch
        torch.cuda.synchronize()
        got = self.t.cpu().numpy().view(np.uint64)
        for at, nseg, mode, want, note, with_selected, with_high in self.items:
            rows, sel, high = expect(want, mode)
            if not with_selected:
                sel = self.host[at + nseg * 32:at + nseg * 33]      # NULL d_selected: the words behind the rows stay
            if not with_high:
                high = self.host[at + nseg * 33:at + nseg * 34]     # NULL d_high: so do these
            same((got[at:at + nseg * 32].reshape(nseg, 32), got[at + nseg * 32:at + nseg * 33], got[at + nseg * 33:at + nseg * 34]),
                 (rows, sel, high), (note, "mode", mode))


class Arena:
    """many host arrays in one device allocation, each at a chosen phase (in elements) of a 16-byte line and with `pad` elements
    of `fill` around it; uploaded in one copy"""

    def __init__(self, dtype, fill, pad=64):
        self.dtype, self.fill, self.pad = np.dtype(dtype), fill, pad
        self.per = 16 // self.dtype.itemsize
        self.parts, self.size, self.t = [], 0, None

    def add(self, x, phase=0):
        x = np.ascontiguousarray(x).view(self.dtype) if np.asarray(x).dtype.itemsize == self.dtype.itemsize else np.ascontiguousarray(x, dtype=self.dtype)
        start = (self.size + self.pad + self.per - 1) // self.per * self.per + phase
        self.parts.append((start, x))
        self.size = start + x.size + self.pad
        return start

    def upload(self):
        host = np.full((self.size + self.per) // self.per * self.per, self.fill, dtype=self.dtype)
        for start, x in self.parts:
            host[start:start + x.size] = x
        self.t = dev(host)
        assert self.t.data_ptr() % 16 == 0
        return self

    def ptr(self, start):
        return self.t.data_ptr() + start * self.dtype.itemsize


def encode(sel_set, sel_bits, where, value=1):
    """the bytes of a selection for the arena and the phase to place them at: a bitmap that starts `where` bits into its first
    byte (every unused bit set), or bytes of `value` per selected element at byte alignment `where & 15` behind `where - (where &
    15)` bytes of 0xFF.  Returns (bytes, arena phase, sel_offset)"""
    m = np.asarray(sel_set, dtype=bool)
    if sel_bits == BITMAP:
        return pack(m, where, fill=1), 0, where
    front = where - (where & 15)
    return np.concatenate([np.full(front, 0xFF, dtype=np.uint8), m.astype(np.uint8) * np.uint8(value)]), where & 15, front


def poisoned(clean, mask, offsets, W):
    """the column and the selection as the kernel gets them: poison in every unselected slot and outside every segment; the
    selection SET outside every segment, clear in the unselected slots of a segment.  Returns (x, sel_set); the oracle takes
    (x, mask)"""
    x = np.ascontiguousarray(clean).view(UNSIGNED[W]).copy()
    mask = np.asarray(mask, dtype=bool)
    o = np.asarray(offsets, dtype=np.int64)
    inside = np.zeros(x.size, dtype=bool)
    inside[int(o[0]):int(o[-1])] = True
    x[~mask | ~inside] = poison(W)
    return x, np.where(inside, mask, True)


def column(rng, n, W, pattern=None):
    """n elements without bits above bit 15: random, or a pattern of prime period"""
    low = rng.randint(0, 65536, n) if pattern is None else np.resize(pattern, n)
    return low.astype(UNSIGNED[W])


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
    return hip.fsk_launch_segments_wide_where   # prototype attached by _lib.lib()


@contextlib.contextmanager
def policy(hip, min_units, blocks_per_cu=1):
    saved = get_policy(hip)
    try:
        hip.fsk_set_segments_policy(min_units, blocks_per_cu)
        assert get_policy(hip) == (min_units, blocks_per_cu)
        yield
    finally:
        hip.fsk_set_segments_policy(*saved)
    assert get_policy(hip) == saved


def direct(launcher, batch, k, aptr, W, sptr, sel_offset, sel_bits, base, m, d_off, grid, stream=None):
    """one fsk_launch_segments_wide_where into the batch's words of launch k"""
    rc = launcher(aptr, W, sptr, sel_offset, sel_bits, base, m, d_off.data_ptr(), batch.nseg(k), batch.out(k), batch.selected(k),
                  batch.high(k), batch.mode(k), grid, stream)
    assert rc == 0, (batch.items[k][4], rc)


def device_entry(hip, batch, k, aptr, n, W, sptr, sel_offset, sel_bits, d_off, stream=None):
    rc = hip.FLAGSTATS_hip_device_wide_segments_where(aptr, n, W, d_off.data_ptr(), batch.nseg(k), sptr, sel_offset, sel_bits,
                                                      batch.out(k), batch.selected(k), batch.high(k), batch.mode(k), stream)
    assert rc == 0, (batch.items[k][4], err(hip))


def host_words(nseg, mode):
    store = bool(mode & STORE)
    return (np.full((nseg, 32), GARBAGE if store else BIAS, dtype=np.uint64), np.full(nseg, GARBAGE if store else SEL_BIAS, dtype=np.uint64),
            np.full(nseg, GARBAGE if store else MASK_BIAS, dtype=np.uint64))


def sync_form(hip, ptr, n, W, offsets, sptr, sel_offset, sel_bits, mode):
    o = np.ascontiguousarray(offsets, dtype=np.uint64)
    rows, sel, high = host_words(o.size - 1, mode)
    rc = hip.FLAGSTATS_hip_device_wide_segments_where_sync(ptr, n, W, o.ctypes.data, o.size - 1, sptr, sel_offset, sel_bits, rows.ctypes.data,
                                                           sel.ctypes.data, high.ctypes.data, mode)
    assert rc == 0, err(hip)
    return rows, sel, high


def host_form(hip, x, offsets, s, sel_offset, sel_bits, mode):
    o = np.ascontiguousarray(offsets, dtype=np.uint64)
    rows, sel, high = host_words(o.size - 1, mode)
    rc = hip.FLAGSTATS_hip_wide_x64_segments_where(x.ctypes.data, x.size, x.dtype.itemsize, o.ctypes.data, o.size - 1, s.ctypes.data,
                                                   sel_offset, sel_bits, rows.ctypes.data, sel.ctypes.data, high.ctypes.data, mode)
    assert rc == 0, err(hip)
    return rows, sel, high


# ------------------------------------------------------------------ 1. which bit or byte belongs to which element
def one_hot_positions(W):
    EPV, R, U = 16 // W, 1024 // W, 8192 // W
    n = 3 * U + 5
    return sorted({0, 1, EPV - 1, EPV, 7, 8, R - 1, R, U - 1, U, 2 * U - 1, 2 * U, n - 1})


@functools.lru_cache(maxsize=None)
def one_hot_cases(W):
    """(n, the two layouts, [(x, sel_set, wants per layout)] over one-hot masks and their complements): computed once per W and
    shared between the forms"""
    U = 8192 // W
    n = 3 * U + 5
    pattern = np.random.RandomState(101).randint(0, 65536, 251)
    clean = column(None, n, W, pattern)
    layouts = (np.array([0, n], dtype=np.int64), np.array([0, U - 3, 2 * U + 1, n], dtype=np.int64))
    cases = []
    for pos in one_hot_positions(W):
        for complement in (False, True):
            mask = np.zeros(n, dtype=bool)
            mask[pos] = True
            if complement:
                mask = ~mask
            x, sel_set = poisoned(clean, mask, layouts[0], W)
            wants = [swwo.want(x, o, mask, True) for o in layouts]
            assert all(int(w[1].sum()) == int(mask.sum()) and not w[2].any() for w in wants)
            cases.append((x, sel_set, wants))
    return n, layouts, cases


@pytest.mark.parametrize("sel_bits", [BITMAP, BYTES])
@pytest.mark.parametrize("W", WIDTHS)
def test_which_bit_or_byte_belongs_to_which_element(hip, launcher, W, sel_bits):
    """n = 3 U + 5; every array phase x sel_offset & 7 in 0-7 and one offset above 8,000; one-hot masks and their complements at
    the vector, byte, row and unit edges over values of prime period; one segment and the same cut into three; under min_units 1
    (chain) and 0xFFFFFFFF (per-piece only).  A selection bit applied to the wrong element selects a poison element: 0xFFFF in
    every counter's way and every high bit in the mask"""
    EPV = 16 // W
    n, layouts, cases = one_hot_cases(W)
    sel_offsets = list(range(8)) + [8013]
    arrays, sels = Arena(UNSIGNED[W], poison(W)), Arena(np.uint8, 0xFF, pad=16)
    a_at = [[arrays.add(x, phase) for x, _, _ in cases] for phase in range(EPV)]
    s_at = [[(sels.add(data, ph), off) for data, ph, off in (encode(sel_set, sel_bits, so) for so in sel_offsets)] for _, sel_set, _ in cases]
    arrays.upload(), sels.upload()
    d_offs = [dev64(o) for o in layouts]
    batch, calls = Batch(), []
    i = 0
    for mu in (1, NEVER):
        for phase in range(EPV):
            for c, (_, _, wants) in enumerate(cases):
                for s, (at, off) in enumerate(s_at[c]):
                    for lay in range(2):
                        mode = MODES[i % 4]
                        i += 1
                        k = batch.add(mode, wants[lay], (W, sel_bits, mu, phase, c, sel_offsets[s], lay))
                        calls.append((mu, k, arrays.ptr(a_at[phase][c]), sels.ptr(at), off, lay))
    batch.upload()
    for mu in (1, NEVER):
        with policy(hip, mu):
            for m, k, aptr, sptr, off, lay in calls:
                if m == mu:
                    direct(launcher, batch, k, aptr, W, sptr, off, sel_bits, 0, n, d_offs[lay], 2)
    batch.check()


# ------------------------------------------------------------------ 2. seams inside a vector and inside a selection byte
def seam_layouts(W, n):
    R, U = 1024 // W, 8192 // W
    ranges = [(0, 10), (R - 10, R + 10), (U - 10, U + 10), (n - 10, n)]
    every = np.concatenate([np.arange(a, b + 1) for a, b in ranges])
    dense = np.sort(np.concatenate([every, every[::5]]))                   # every boundary position; every fifth twice: empty segments
    steps = np.resize([2, 3, 0, 1], every.size * 2)
    sparse = [np.concatenate([[a], a + np.cumsum(steps)])for a, _ in ranges]
    sparse = np.concatenate([s[s <= b] for s, (_, b) in zip(sparse, ranges)])       # lengths 2, 3, 0, 1 inside every range
    late = dense[dense >= 2 * U + 0] if (dense >= 2 * U).any() else dense
    return [dense.astype(np.int64), sparse.astype(np.int64), np.concatenate([[3], dense[dense > 10]]).astype(np.int64), late.astype(np.int64)]


@pytest.mark.parametrize("W", WIDTHS)
def test_seams_inside_a_vector_and_a_selection_byte(hip, launcher, W):
    """segments of length 0, 1, 2, ... with every boundary position in [U - 10, U + 10], [R - 10, R + 10], [0, 10] and
    [n - 10, n]; masks 0101..., 0011... and all-set; neighbours and gaps poisoned AND selected; offsets[0] > 0, empty segments, and
    a layout whose first segment begins beyond whole units, which are skipped unread"""
    EPV, R, U = 16 // W, 1024 // W, 8192 // W
    n = 4 * U + 21
    rng = np.random.RandomState(7)
    clean = column(rng, n, W)
    layouts = seam_layouts(W, n)
    assert layouts[2][0] == 3 and layouts[3][0] >= 2 * U and (np.diff(layouts[0]) == 0).any() and set(np.diff(layouts[1])) >= {0, 1, 2, 3}
    assert all((np.diff(o) >= 0).all() and o[-1] <= n for o in layouts)
    idx = np.arange(n)
    masks = (idx % 2 == 1, idx % 4 >= 2, np.ones(n, dtype=bool))
    arrays, sels = Arena(UNSIGNED[W], poison(W)), Arena(np.uint8, 0xFF, pad=16)
    todo = []
    for li, o in enumerate(layouts):
        for mi, mask in enumerate(masks):
            # the neighbours of every piece are elements of other segments, selected like them: what keeps them out is the
            # piece's own mask; the gaps (in front of offsets[0], behind offsets[nseg]) are poison, selected
            x, sel_set = poisoned(clean, mask, o, W)
            if mi < 2:
                assert (x[int(o[0]):int(o[-1])] == poison(W)).any() and sel_set[:int(o[0])].all() and sel_set[int(o[-1]):].all()
            want = swwo.want(x, o, mask, True)
            assert not want[2].any() and int(want[1].sum()) == int(mask[int(o[0]):int(o[-1])].sum())
            for phase in range(EPV):
                at = arrays.add(x, phase)
                for sel_bits, where in ((BITMAP, 0), (BITMAP, 5), (BYTES, 3)):
                    data, ph, off = encode(sel_set, sel_bits, where, value=0x80)
                    todo.append((li, want, at, sels.add(data, ph), off, sel_bits, (W, li, mi, phase, sel_bits, where)))
    arrays.upload(), sels.upload()
    d_offs = [dev64(o) for o in layouts]
    batch, calls = Batch(), []
    i = 0
    for mu in (1, NEVER):
        for li, want, at, s_at, off, sel_bits, note in todo:
            k = batch.add(MODES[i % 4], want, note + (mu,))
            i += 1
            calls.append((mu, k, arrays.ptr(at), sels.ptr(s_at), off, sel_bits, li))
    batch.upload()
    for mu in (1, NEVER):
        with policy(hip, mu):
            for m, k, aptr, sptr, off, sel_bits, li in calls:
                if m == mu:
                    direct(launcher, batch, k, aptr, W, sptr, off, sel_bits, 0, n, d_offs[li], 1)
    batch.check()


# ------------------------------------------------------------------ 3. `high` per segment
def marked_column(rng, n, W, o, mask):
    """selected elements of segment i carry bit 16 + i % 16; at W = 8 also bit 32 + i % 32 and, in every third segment, the sign
    bit; poison in the unselected slots and outside the segments"""
    clean = column(rng, n, W)
    for i in range(o.size - 1):
        b, e = int(o[i]), int(o[i + 1])
        bits = 1 << (16 + i % 16)
        if W == 8:
            bits |= 1 << (32 + i % 32)
            if i % 3 == 0:
                bits |= 1 << 63
        clean[b:e] |= UNSIGNED[W](bits)
    return poisoned(clean, mask, o, W)


@pytest.mark.parametrize("W", WIDTHS)
def test_high_per_segment(hip, launcher, W):
    """high[i] holds exactly the bits its selected elements carry: poison in unselected slots of the same vector, in neighbouring
    segments and in the gaps reaches no mask; the strict form names the right segment and does not raise for garbage in null slots"""
    from libflagstats_amd import segments_wide_where as sww
    U = 8192 // W
    rng = np.random.RandomState(13)
    lengths = np.concatenate([[1, 2, 3, 0, 5, 3 * U + 7, 1, U, 2 * U + 1, 0, 9], rng.randint(1, 300, 30)])
    o = 6 + np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(o[-1]) + 9
    nseg = o.size - 1
    mask = rng.randint(0, 2, n).astype(bool)
    mask[o[:-1][lengths > 0]] = True                      # every non-empty segment selects something
    x, sel_set = marked_column(rng, n, W, o, mask)
    want = swwo.want(x, o, mask, True)
    for i in range(nseg):
        bits = 0 if lengths[i] == 0 else (1 << (16 + i % 16)) | ((1 << (32 + i % 32)) | ((1 << 63) if i % 3 == 0 else 0) if W == 8 else 0)
        assert int(want[2][i]) == bits, i
    w = swo.writer_ranges(W, n, 1, W)                     # the array lies one element past a 16-byte boundary
    assert (w.pieces(o, 1)["chain"] > 0).any()
    arrays, sels = Arena(UNSIGNED[W], poison(W)), Arena(np.uint8, 0xFF, pad=16)
    a_at = arrays.add(x, 1)
    encs = [encode(sel_set, BITMAP, 0), encode(sel_set, BITMAP, 3), encode(sel_set, BYTES, 5, value=7)]
    s_at = [(sels.add(d, ph), off, BITMAP if j < 2 else BYTES) for j, (d, ph, off) in enumerate(encs)]
    arrays.upload(), sels.upload()
    d_off = dev64(o)
    batch, calls = Batch(), []
    for mu in (1, NEVER):
        for at, off, sb in s_at:
            for mode in MODES:
                calls.append((mu, batch.add(mode, want, (W, mu, off, sb, mode)), sels.ptr(at), off, sb))
    batch.upload()
    for mu in (1, NEVER):
        with policy(hip, mu):
            for m, k, sptr, off, sb in calls:
                if m == mu:
                    direct(launcher, batch, k, arrays.ptr(a_at), W, sptr, off, sb, 0, n, d_off, 1)
    batch.check()
    # the Python strict form: the first segment whose selected elements carry high bits, its range and its bits
    xs = x.view(SIGNED[W])
    first = int(np.flatnonzero(want[2])[0])
    text = r"segment %d \(offsets %d\.\.%d\): values outside 0\.\.65535: bits 0x%X set above bit 15" % (first, o[first], o[first + 1],
                                                                                                     int(want[2][first]))
    with pytest.raises(ValueError, match=text):
        sww.flagstats_segments_ints_where(xs, o, mask)
    dicts = sww.flagstats_segments_ints_where(xs, o, mask, strict=False)
    assert [d["n_values"] for d in dicts] == [int(v) for v in want[1]] and [d["high_bits"] for d in dicts] == [int(v) for v in want[2]]
    # garbage in null slots only: no raise
    clean_x, _ = poisoned(column(rng, n, W), mask, o, W)
    assert (clean_x == poison(W)).any()
    dicts = sww.flagstats_segments_ints_where(clean_x.view(SIGNED[W]), o, pack(mask, 5), packed=True, bit_offset=5)
    assert [d["n_values"] for d in dicts] == [int(v) for v in want[1]]


# ------------------------------------------------------------------ 4. chain, epochs and regime changes
def chain_layout(w, n, first):
    """offsets over the four writers of a grid-1 launch: in writer k a segment of 3 ragged elements, K whole units and 5 ragged
    elements for K = 254, 255 (this one ends exactly with its 255th unit: at the epoch), 256 and 2 * 255 + 3, then a short
    per-piece segment and a chain segment of 20 units (chain -> per-piece -> chain) where the writer has room.  `first`: the first
    offset (0: the first segment begins with element 0 of the array; beyond whole units: a skipped stretch, then a chain)"""
    U = w.unit
    cuts = [first]
    for k, K in enumerate((254, 255, 256, 513)):
        g0 = first + 6 * U if k == 0 else int(w.begin[k]) + 2 * U
        if k == 0:
            cuts += [first + 3 * U, g0 - 3]                         # a segment of three whole units at the very beginning
        else:
            cuts += [int(w.begin[k]) + 7, g0 - 3]
        end = g0 + K * U + (0 if K == 255 else 5)
        cuts.append(end)
        if K != 513:
            cuts += [end + 11, end + 11 + 21 * U + U // 2]
    cuts.append(n - 3)
    o = np.array(cuts, dtype=np.int64)
    assert (np.diff(o) > 0).all()
    return o


@pytest.mark.parametrize("W", WIDTHS)
def test_chain_epochs_and_regime_changes(hip, launcher, W):
    """launcher grid 1 (four writers) over ~16 MiB of an aligned array: chains of 254, 255, 256 and 2 * 255 + 3 units inside one
    segment, a segment ending exactly at an epoch, chain -> per-piece -> chain, a skipped stretch -> chain; a plain and a funnelled
    bit offset and the byte form.  The first segment of one layout begins with element 0: grid unit 0 of the funnelled launch is a
    per-piece unit through the guarded loaders (the addresses: tests/test_segments_wide_where_host.py; the values: here)"""
    U = 8192 // W
    n = 4 * 516 * U - 9
    rng = np.random.RandomState(17)
    pattern = rng.randint(0, 65536, P)
    clean = column(None, n, W, pattern)
    hot = np.resize(rng.randint(0, 97, 8191) == 0, n)
    clean[hot] |= UNSIGNED[W](1 << (8 * W - 2))
    mask = np.resize(rng.randint(0, 2, 8191).astype(bool), n)
    w = swo.writer_ranges(0, n, 1, W)
    assert w.waves == 4 and w.lo0 == 0 and all(int(e - b) >= 515 * U for b, e in zip(w.begin, w.end))
    layouts = [chain_layout(w, n, 0), chain_layout(w, n, 3 * U)]
    for o in layouts:
        pieces = w.pieces(o, 2)
        runs = {int(c): (int(h), int(t)) for c, h, t in zip(pieces["chain"], pieces["head"], pieces["tail"]) if c in (254, 255, 256, 513)}
        assert runs == {254: (3, 5), 255: (3, 0), 256: (3, 5), 513: (3, 5)}, runs
        assert (pieces["chain"] == 20).sum() == 3 and (pieces["chain"] == 0).any() and pieces["plain"].any() and (~pieces["plain"]).any()
        assert int(pieces["chain"][0]) == 3 and int(pieces["head"][0]) == 0      # the first segment: whole units from its first element on
    assert layouts[0][0] == 0 and layouts[1][0] == 3 * U
    arrays, sels = Arena(UNSIGNED[W], poison(W)), Arena(np.uint8, 0xFF, pad=16)
    todo = []
    for li, o in enumerate(layouts):
        x, sel_set = poisoned(clean, mask, o, W)
        want = swwo.want(x, o, mask, True)
        assert want[2].any() and (want[1][np.diff(o) > 50] > 0).all() and (want[1] < np.diff(o).astype(np.uint64)).all()
        at = arrays.add(x, 0)
        for sel_bits, where in ((BITMAP, 0), (BITMAP, 5), (BYTES, 1)):
            data, ph, off = encode(sel_set, sel_bits, where)
            todo.append((li, want, at, sels.add(data, ph), off, sel_bits, where))
    arrays.upload(), sels.upload()
    assert arrays.ptr(todo[0][2]) % 16 == 0
    d_offs = [dev64(o) for o in layouts]
    batch, calls = Batch(), []
    for li, want, at, s_at, off, sel_bits, where in todo:
        for mode in (3, 0):
            calls.append((batch.add(mode, want, (W, li, sel_bits, where, mode)), arrays.ptr(at), sels.ptr(s_at), off, sel_bits, li))
    batch.upload()
    with policy(hip, 2):
        for k, aptr, sptr, off, sel_bits, li in calls:
            direct(launcher, batch, k, aptr, W, sptr, off, sel_bits, 0, n, d_offs[li], 1)
        batch.check()
    del arrays, sels


# ------------------------------------------------------------------ 5. every min_units through the three public entries
@pytest.mark.parametrize("W", WIDTHS)
def test_every_min_units_through_the_public_entries(hip, W):
    import torch
    U = 8192 // W
    rng = np.random.RandomState(29)
    n = 384 * U + 77
    o = np.array([9, 40, 40, U + 1, 2 * U + 5, 5 * U + 5, 8 * U + 7, 100 * U + 3, 100 * U + 9, 100 * U + 9 + 255 * U, n - 5], dtype=np.int64)
    mask = rng.randint(0, 3, n) > 0
    clean = column(rng, n, W)
    clean[rng.randint(0, n, 200)] |= UNSIGNED[W](1 << 21)
    x, sel_set = poisoned(clean, mask, o, W)
    want = swwo.want(x, o, mask, True)
    assert want[2].any() and (want[1] > 0).sum() >= 8
    t = dev(x)
    bits, byts = pack(sel_set, 5, fill=1), sel_set.astype(np.uint8)
    d_bits, d_bytes = dev(bits), dev(byts)
    w = swo.writer_ranges(t.data_ptr() % 16, n, hip.FLAGSTATS_hip_compute_units(), W)
    longest = {mu: int(w.pieces(o, mu)["chain"].max()) for mu in EVERY_MIN_UNITS}
    assert longest[0] >= 1 and longest[1] >= 1 and longest[NEVER] == 0, longest
    d_off = dev64(o)
    for i, mu in enumerate(EVERY_MIN_UNITS):
        sel_bits = BITMAP if i % 3 != 1 else BYTES
        d_s, h_s, off = (d_bits, bits, 5) if sel_bits == BITMAP else (d_bytes, byts, 0)
        with policy(hip, mu):
            batch = Batch()
            k = batch.add(3, want, (W, mu, "device"))
            batch.upload()
            device_entry(hip, batch, k, t.data_ptr(), n, W, d_s.data_ptr(), off, sel_bits, d_off)
            batch.check()
            same(sync_form(hip, t.data_ptr(), n, W, o, d_s.data_ptr(), off, sel_bits, 2), expect(want, 2), (W, mu, "sync"))
            same(host_form(hip, x, o, h_s, off, sel_bits, 1), expect(want, 1), (W, mu, "host"))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 6. all four modes, NULL d_selected and / or d_high
@pytest.mark.parametrize("W", WIDTHS)
def test_modes_and_null_outputs(hip, launcher, W):
    """store and += with and without superset over garbage / bias words, through the launcher and the device entry; with
    d_selected and / or d_high NULL the words behind the rows stay untouched"""
    U = 8192 // W
    rng = np.random.RandomState(33)
    n = 36 * U + 11
    o = np.array([0, 50, 3 * U + 1, 3 * U + 1, 20 * U - 7, 36 * U], dtype=np.int64)
    mask = rng.randint(0, 2, n).astype(bool)
    clean = column(rng, n, W)
    clean[rng.randint(0, n, 300)] |= UNSIGNED[W](1 << 19)
    x, sel_set = poisoned(clean, mask, o, W)
    want = swwo.want(x, o, mask, True)
    assert want[2].any() and want[1][2] == 0
    arrays, sels = Arena(UNSIGNED[W], poison(W)), Arena(np.uint8, 0xFF, pad=16)
    a_at = arrays.add(x, 16 // W - 1)
    encs = [encode(sel_set, BITMAP, 6), encode(sel_set, BYTES, 2)]
    s_at = [(sels.add(d, ph), off, sb) for (d, ph, off), sb in zip(encs, (BITMAP, BYTES))]
    arrays.upload(), sels.upload()
    d_off = dev64(o)
    batch, calls = Batch(), []
    for at, off, sb in s_at:
        for mode in MODES:
            for with_sel, with_high in ((True, True), (False, True), (True, False), (False, False)):
                for how in ("launcher", "entry"):
                    k = batch.add(mode, want, (W, sb, mode, with_sel, with_high, how), with_sel, with_high)
                    calls.append((k, sels.ptr(at), off, sb, how))
    batch.upload()
    for k, sptr, off, sb, how in calls:
        if how == "launcher":
            direct(launcher, batch, k, arrays.ptr(a_at), W, sptr, off, sb, 0, n, d_off, 64)
        else:
            device_entry(hip, batch, k, arrays.ptr(a_at), n, W, sptr, off, sb, d_off)
    batch.check()


# ------------------------------------------------------------------ 7. densities and byte values
@pytest.mark.parametrize("W", WIDTHS)
def test_densities_and_byte_values(hip, launcher, W):
    """densities 0, 0.01, 0.5, 0.99 and 1 in both forms, and in the byte form every non-zero byte value selects"""
    U = 8192 // W
    rng = np.random.RandomState(61)
    n = 9 * U + 100
    o = np.array([1, 600, 2 * U - 1 + 5, 6 * U, n - 256, n - 2], dtype=np.int64)
    clean = column(rng, n, W)
    clean[rng.randint(0, n, 500)] |= UNSIGNED[W](1 << 16)
    w = swo.writer_ranges(W, n, 1, W)
    pieces = w.pieces(o, 2)
    assert (pieces["chain"] > 0).any() and (pieces["chain"] == 0).any()
    arrays, sels = Arena(UNSIGNED[W], poison(W)), Arena(np.uint8, 0xFF, pad=16)
    todo = []
    for density in (0.0, 0.01, 0.5, 0.99, 1.0):
        mask = rng.random_sample(n) < density
        x, sel_set = poisoned(clean, mask, o, W)
        want = swwo.want(x, o, mask, True)
        if density == 0.0:
            assert not want[0].any() and not want[1].any() and not want[2].any()
        if density == 1.0:
            assert np.array_equal(want[1], np.diff(o).astype(np.uint64)) and np.array_equal(want[0], swo.want(clean.view(SIGNED[W]), o, True)[0])
        at = arrays.add(x, 1)
        for sel_bits, where in ((BITMAP, 0), (BITMAP, 6), (BYTES, 3)):
            data, ph, off = encode(sel_set, sel_bits, where, value=0xFF)
            todo.append((want, at, sels.add(data, ph), off, sel_bits, ("density", density, sel_bits, where)))
    mask = rng.randint(0, 2, n).astype(bool)
    x, sel_set = poisoned(clean, mask, o, W)
    byte_vals = np.where(sel_set, 1 + np.arange(n) % 255, 0).astype(np.uint8)
    assert set(byte_vals[mask & (np.arange(n) >= o[0]) & (np.arange(n) < o[-1])].tolist()) == set(range(1, 256))
    k = int(np.argmax(pieces["chain"]))                          # the chain run sees selected and unselected bytes of many values
    b = int(pieces["b"][k] + pieces["head"][k])
    assert len(set(byte_vals[b:b + int(pieces["chain"][k]) * U].tolist())) > 128 and 0 in byte_vals[b:b + U]
    todo.append((swwo.want(x, o, mask, True), arrays.add(x, 1), sels.add(byte_vals, 5), 0, BYTES, ("byte values",)))
    arrays.upload(), sels.upload()
    d_off = dev64(o)
    batch, calls = Batch(), []
    for want, at, s_at, off, sel_bits, note in todo:
        for mode in MODES:
            for grid in (1, None):
                calls.append((batch.add(mode, want, (W,) + note + (mode, grid)), arrays.ptr(at), sels.ptr(s_at), off, sel_bits, grid))
    batch.upload()
    assert arrays.ptr(todo[0][1]) % 16 == W
    for k, aptr, sptr, off, sel_bits, grid in calls:
        if grid is None:
            device_entry(hip, batch, k, aptr, n, W, sptr, off, sel_bits, d_off)
        else:
            direct(launcher, batch, k, aptr, W, sptr, off, sel_bits, 0, n, d_off, grid)
    batch.check()


# ------------------------------------------------------------------ 8. equivalences
@pytest.mark.parametrize("W", WIDTHS)
def test_equivalences(hip, W):
    """one segment [0, n) is FLAGSTATS_hip_device_wide_where_sync; an all-ones mask is FLAGSTATS_hip_device_wide_segments_sync, high
    included; int16 / uint16 input is the u16 segments_where entries with high zero; the bitmap form and the byte form of the same
    mask agree -- and the oracle says the same (all the kernels could be wrong alike)"""
    import torch
    from libflagstats_amd import segments_where as sw
    from libflagstats_amd import segments_wide_where as sww
    U = 8192 // W
    rng = np.random.RandomState(41)
    n = 50 * U + 3
    clean = column(rng, n, W)
    clean[rng.randint(0, n, 400)] |= UNSIGNED[W](1 << (8 * W - 1))
    mask = rng.randint(0, 3, n) > 0
    o = np.unique(np.concatenate([[7], rng.randint(7, n - 9, 30), [12 * U, 30 * U + 1, n - 9]])).astype(np.int64)
    nseg = o.size - 1
    x = clean.copy()
    x[~mask] = poison(W)
    t = dev(x)
    bits, byts = pack(mask, 3, fill=1), (mask * rng.randint(1, 256, n)).astype(np.uint8)
    d_bits, d_bytes = dev(bits), dev(byts)
    # one segment [0, n): the whole-column entry
    one = np.array([0, n], dtype=np.uint64)
    for d_s, off, sb in ((d_bits, 3, BITMAP), (d_bytes, 0, BYTES)):
        for mode in (1, 3):
            got = sync_form(hip, t.data_ptr(), n, W, one, d_s.data_ptr(), off, sb, mode)
            ref = np.zeros(34, dtype=np.uint64)
            rc = hip.FLAGSTATS_hip_device_wide_where_sync(t.data_ptr(), n, W, d_s.data_ptr(), off, sb, ref.ctypes.data, ref[32:].ctypes.data,
                                                          ref[33:].ctypes.data, mode)
            assert rc == 0, err(hip)
            assert np.array_equal(got[0][0], ref[:32]) and got[1][0] == ref[32] and got[2][0] == ref[33] and 0 < int(ref[32]) < n and ref[33]
    # an all-ones mask: the unmasked wide segmented entry, high included (the column as it is: no poison)
    tc = dev(clean)
    ones_bits, ones_bytes = dev(np.full((n + 7) // 8 + 1, 0xFF, dtype=np.uint8)), dev(np.full(n, 1, dtype=np.uint8))
    for mode in (1, 3):
        ref_rows, ref_high = np.zeros((nseg, 32), dtype=np.uint64), np.zeros(nseg, dtype=np.uint64)
        o64 = o.astype(np.uint64)
        rc = hip.FLAGSTATS_hip_device_wide_segments_sync(tc.data_ptr(), n, W, o64.ctypes.data, nseg, ref_rows.ctypes.data, ref_high.ctypes.data, mode)
        assert rc == 0, err(hip)
        assert ref_high.any()
        for d_s, off, sb in ((ones_bits, 2, BITMAP), (ones_bytes, 0, BYTES)):
            got = sync_form(hip, tc.data_ptr(), n, W, o, d_s.data_ptr(), off, sb, mode)
            same(got, (ref_rows, np.diff(o).astype(np.uint64), ref_high), (W, "all ones", sb, mode))
    # the bitmap form and the byte form of the same mask agree, and with the oracle
    want = swwo.want(x, o, mask, True)
    a = sync_form(hip, t.data_ptr(), n, W, o, d_bits.data_ptr(), 3, BITMAP, 3)
    b = sync_form(hip, t.data_ptr(), n, W, o, d_bytes.data_ptr(), 0, BYTES, 3)
    same(a, b, (W, "bitmap against bytes"))
    same(a, want, (W, "oracle"))
    # 16-bit input: the u16 segments_where entries, high zero
    for dt in (np.int16, np.uint16):
        v16 = rng.randint(0, 65536, n).astype(np.uint16).view(dt)
        got = sww.counters_segments_ints_where(v16, o, bits, packed=True, bit_offset=3, superset=True)
        ref = sw.counters_segments_where(v16.view(np.uint16), o, bits, packed=True, bit_offset=3, superset=True)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and not got[2].any() and got[2].shape == (nseg,)
        t16 = dev(v16)
        d_off = dev64(o)
        high = torch.full((nseg,), 5, dtype=torch.int64, device="cuda")
        rows, sel, h = sww.count_segments_torch_ints_where(t16, d_off, d_bits, packed=True, bit_offset=3, high=high, superset=True)
        torch.cuda.synchronize()
        assert np.array_equal(u64(rows), ref[0]) and np.array_equal(u64(sel), ref[1]) and h is high and not high.any()
    # nseg == 0 touches nothing
    assert hip.FLAGSTATS_hip_device_wide_segments_where(t.data_ptr(), n, W, None, 0, d_bits.data_ptr(), 3, BITMAP, None, None, None, STORE, None) == 0
    assert hip.FLAGSTATS_hip_wide_x64_segments_where(x.ctypes.data, n, W, None, 0, bits.ctypes.data, 3, BITMAP, None, None, None, STORE) == 0


# ------------------------------------------------------------------ 9. host form across chunks
@pytest.mark.parametrize("W", WIDTHS)
def test_host_form_across_chunks(hip, W):
    """chunks of 8,193 int32 or 4,097 int64 elements from offsets[0] = 3 on: chunk seams fall inside a bitmap byte and
    inside a segment; every chunk's staged array is aligned, so every chunk with (sel_offset + pos) & 7 != 0 is a funnelled launch
    whose unit 0 goes through the guarded loaders; elements in front of offsets[0] and behind offsets[nseg] are poison whose bits
    and bytes are set and never cross the bus"""
    from libflagstats_amd import _lib
    from libflagstats_amd import segments_wide_where as sww
    rng = np.random.RandomState(53)
    chunk_flags = 16_386 if W == 4 else 16_388             # 8,193 int32 or 4,097 int64 a chunk: odd, so seams move through a byte
    c = chunk_flags * 2 // W
    assert c % 8 == 1
    n = 7 * c + 77
    first = 3
    o = np.array([first, 10, 10, first + c + 7, first + c + c // 2, first + 3 * c + c // 2 + 5, first + 4 * c, n - 20], dtype=np.int64)
    assert (o[5] - first) // c - (o[4] - first) // c == 2 and (o[6] - first) % c == 0
    assert {(6 + first + k * c) & 7 for k in range(8)} == set(range(8))
    clean = column(rng, n + 1, W)[1:]
    clean[first + c + c // 2 + 1] |= UNSIGNED[W](1 << 16)
    clean[first + 2 * c + 9] |= UNSIGNED[W](1 << 20)
    clean[first + 3 * c + c // 2 + 4] |= UNSIGNED[W](1 << (8 * W - 1))
    clean[first + 4 * c] |= UNSIGNED[W](1 << 17)
    mask = rng.randint(0, 2, n).astype(bool)
    mask[[first + c + c // 2 + 1, first + 2 * c + 9, first + 3 * c + c // 2 + 4, first + 4 * c]] = True
    x, sel_set = poisoned(clean, mask, o, W)
    xs = x.view(SIGNED[W])
    want = swwo.want(x, o, mask, True)
    assert [hex(int(v)) for v in want[2]] == [hex(v) for v in (0, 0, 0, 0, (1 << 16) | (1 << 20) | (1 << (8 * W - 1)), 0, 1 << 17)]
    byte_sel = np.concatenate([[0xFF], sel_set.astype(np.uint8) * 0x80]).astype(np.uint8)[1:]      # one byte into its buffer
    encodings = [(pack(sel_set, 6, fill=1), 6, BITMAP), (pack(sel_set, 0, fill=1), 0, BITMAP), (byte_sel, 0, BYTES)]
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", chunk_flags), "chunk_flags")
        for s, off, sb in encodings:
            for mode in MODES:
                same(host_form(hip, xs, o, s, off, sb, mode), expect(want, mode), (W, "chunks", off, sb, mode))
        same(sww.counters_segments_ints_where(xs, o, encodings[0][0], packed=True, bit_offset=6, superset=True), want, (W, "python, packed"))
        same(sww.counters_segments_ints_where(xs, o, sel_set, superset=True), want, (W, "python, bool"))
        for oo in (np.array([1, 50, 99]), np.array([7, 7, 7]), np.array([n, n])):        # one chunk only; nothing covered
            same(sww.counters_segments_ints_where(xs, oo, mask), swwo.want(x, oo, mask), (W, oo))
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old
    got = sww.counters_segments_ints_where(xs[:0], [0, 0], mask[:0])
    assert got[0].shape == (1, 32) and not got[0].any() and not got[1].any() and not got[2].any()
    got = sww.count_segments_device_ptr_ints_where(0, 0, W, [0, 0, 0], 0, 1)
    assert got[0].shape == (2, 32) and not got[0].any() and not got[1].any() and not got[2].any()


# ------------------------------------------------------------------ 10. atomics
@pytest.mark.parametrize("W", WIDTHS)
def test_three_streams_add_into_one_set_of_rows(hip, W):
    import torch
    from libflagstats_amd import segments_wide_where as sww
    U = 8192 // W
    rng = np.random.RandomState(73)
    o = np.array([0, 50, 3 * U + 1, 3 * U + 1, 20 * U - 7, 36 * U], dtype=np.int64)
    nseg = o.size - 1
    d_off = dev64(o)
    rows = torch.zeros((nseg, 32), dtype=torch.int64, device="cuda")
    sel = torch.zeros(nseg, dtype=torch.int64, device="cuda")
    high = torch.zeros(nseg, dtype=torch.int64, device="cuda")
    total = [np.zeros((nseg, 32), dtype=np.uint64), np.zeros(nseg, dtype=np.uint64), np.zeros(nseg, dtype=np.uint64)]
    inputs = []
    for j, (n, packed, bit_offset, density) in enumerate(((36 * U + 11, True, 0, 50), (30 * U + 5, True, 5, 90), (40 * U - 3, False, 0, 10))):
        clean = column(rng, n, W)
        clean[rng.randint(0, n, 100)] |= UNSIGNED[W](1 << (18 + j))
        mask = rng.randint(0, 100, n) < density
        x = clean.copy()
        x[~mask] = poison(W)
        w = swwo.want(x, np.clip(o, 0, n), mask, True)
        assert w[1].any() and w[2].any()
        total[0] += w[0]
        total[1] += w[1]
        total[2] |= w[2]
        where = dev(pack(mask, bit_offset, fill=1)) if packed else dev(mask)
        inputs.append((dev(x), where, packed, bit_offset))
    streams = [torch.cuda.Stream() for _ in inputs]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    for st, (t, where, packed, bit_offset) in zip(streams, inputs):
        with torch.cuda.stream(st):
            sww.count_segments_torch_ints_where(t, d_off, where, packed=packed, bit_offset=bit_offset, out=rows, selected=sel, high=high,
                                                store=False, superset=True)
    for st in streams:
        st.synchronize()
    same((u64(rows), u64(sel), u64(high)), total, (W, "three streams"))


# ------------------------------------------------------------------ 11. refusals
@pytest.mark.parametrize("W", WIDTHS)
def test_refusals(hip, launcher, W):
    """every refusal of the C entries (the FLAGSTATS_hip_last_error texts), of the launcher and of the geometry: each is an argument
    check that returns before anything is launched, and rows, counts and masks stay as they were.  Nothing here reads past an
    allocation: the short allocations are refused by the extent check"""
    import torch
    n, nseg = 4096, 3
    t = torch.zeros(n + 8, dtype={4: torch.int32, 8: torch.int64}[W], device="cuda")
    ts = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    host, hosts = np.zeros(n + 8, dtype=SIGNED[W]), np.zeros(n + 8, dtype=np.uint8)
    o = np.array([0, 10, 2000, n], dtype=np.uint64)
    d_off = dev64(o)
    out = torch.full((nseg, 32), BIAS, dtype=torch.int64, device="cuda")
    sel = torch.full((nseg,), SEL_BIAS, dtype=torch.int64, device="cuda")
    high = torch.full((nseg,), MASK_BIAS, dtype=torch.int64, device="cuda")
    h_out = np.full((nseg, 32), BIAS, dtype=np.uint64)
    h_sel = np.full(nseg, SEL_BIAS, dtype=np.uint64)
    h_high = np.full(nseg, MASK_BIAS, dtype=np.uint64)

    def untouched(what):
        torch.cuda.synchronize()
        assert (out == BIAS).all() and (sel == SEL_BIAS).all() and (high == MASK_BIAS).all(), what
        assert (h_out == BIAS).all() and (h_sel == SEL_BIAS).all() and (h_high == MASK_BIAS).all(), what

    def refused(what, text, d_array=t.data_ptr(), n_=n, eb=W, offsets=o, nseg_=nseg, selection=True, so=0, sb=8, flags=0, rows=True,
                forms=("device", "sync", "host")):
        d_o = None if offsets is None else dev64(offsets.astype(np.int64))
        for form in forms:
            if form == "device":
                rc = hip.FLAGSTATS_hip_device_wide_segments_where(d_array, n_, eb, None if d_o is None else d_o.data_ptr(), nseg_,
                                                                  ts.data_ptr() if selection else None, so, sb, out.data_ptr() if rows else None,
                                                                  sel.data_ptr(), high.data_ptr(), flags, None)
            elif form == "sync":
                rc = hip.FLAGSTATS_hip_device_wide_segments_where_sync(d_array, n_, eb, None if offsets is None else offsets.ctypes.data, nseg_,
                                                                       ts.data_ptr() if selection else None, so, sb,
                                                                       h_out.ctypes.data if rows else None, h_sel.ctypes.data, h_high.ctypes.data,
                                                                       flags)
            else:
                src = host.ctypes.data + (d_array - t.data_ptr()) if d_array else None
                rc = hip.FLAGSTATS_hip_wide_x64_segments_where(src, n_, eb, None if offsets is None else offsets.ctypes.data, nseg_,
                                                               hosts.ctypes.data if selection else None, so, sb,
                                                               h_out.ctypes.data if rows else None, h_sel.ctypes.data, h_high.ctypes.data, flags)
            assert rc != 0, (what, form)
            assert err(hip) and text in err(hip), (what, form, err(hip))
        untouched(what)

    refused("elem_bytes 2", "16-bit arrays go to the u16 segments_where entries (FLAGSTATS_hip_u16_x64_segments_where, "
                            "FLAGSTATS_hip_device_u16_segments_where)", eb=2)
    for eb in (0, 1, 3, 16, -4):
        refused("elem_bytes %d" % eb, "elem_bytes must be 4 or 8", eb=eb)
    for sb in (0, 2, 4, 16, -1):
        refused("sel_bits %d" % sb, "sel_bits must be 1 (an LSB-first bitmap) or 8 (one byte per element)", sb=sb)
    refused("an extra flag bit", "flags: bit 0 store, bit 1 superset; no other bits", flags=4)
    refused("NULL offsets", "with nseg > 0", offsets=None)
    refused("NULL rows", "with nseg > 0", rows=False)
    refused("too many segments", "nseg is too large", nseg_=1 << 60)
    refused("NULL array", "NULL array with n > 0", d_array=None)
    refused("NULL selection", "NULL selection with n > 0", selection=False)
    refused("a misaligned array", "array must be %d-byte aligned (elem_bytes %d)" % (W, W), d_array=t.data_ptr() + W // 2)
    refused("n * elem_bytes is no size", "n * elem_bytes is not a size", n_=1 << 63)
    refused("sel_offset + n is no index", "sel_offset + n is not an index", so=(1 << 64) - 100)
    refused("decreasing offsets", "offsets must be non-decreasing", offsets=np.array([0, 20, 10, n], dtype=np.uint64), forms=("sync", "host"))
    refused("offsets past the array", "exceeds the array's", offsets=np.array([0, 10, 20, n + 1], dtype=np.uint64), forms=("sync", "host"))
    # host pointers where device memory is needed
    a, f, sd = t.data_ptr(), d_off.data_ptr(), ts.data_ptr()
    good = dict(d_array=a, d_offsets=f, d_sel=sd, d_out=out.data_ptr(), d_selected=sel.data_ptr(), d_high=high.data_ptr())
    for name, bad in (("d_out", h_out.ctypes.data), ("d_selected", h_sel.ctypes.data), ("d_high", h_high.ctypes.data),
                      ("d_offsets", o.ctypes.data), ("d_array", host.ctypes.data), ("d_sel", hosts.ctypes.data)):
        k = {**good, name: bad}
        rc = hip.FLAGSTATS_hip_device_wide_segments_where(k["d_array"], n, W, k["d_offsets"], nseg, k["d_sel"], 0, 8, k["d_out"],
                                                          k["d_selected"], k["d_high"], 0, None)
        assert rc != 0 and name in err(hip), (name, err(hip))
    for name, args in (("d_array", (host.ctypes.data, sd)), ("d_sel", (a, hosts.ctypes.data))):
        rc = hip.FLAGSTATS_hip_device_wide_segments_where_sync(args[0], n, W, o.ctypes.data, nseg, args[1], 0, 8, h_out.ctypes.data,
                                                               h_sel.ctypes.data, h_high.ctypes.data, 0)
        assert rc != 0 and name in err(hip), (name, err(hip))
    untouched("host pointers")
    # extents: the array one element short, the selection one byte short, rows, counts, masks and offsets 8 bytes short
    nbytes = 2 << 20
    raw = hip.FLAGSTATS_hip_device_alloc(nbytes)
    assert raw
    try:
        assert hip.FLAGSTATS_hip_memcpy_h2d(raw, np.zeros(nbytes, dtype=np.uint8).ctypes.data, nbytes) == 0
        big = np.array([0, 5, 100, nbytes // W], dtype=np.uint64)
        big_off = dev64(big)
        bigs = torch.zeros(nbytes // W + 8, dtype=torch.uint8, device="cuda")
        rc = hip.FLAGSTATS_hip_device_wide_segments_where(raw, nbytes // W + 1, W, big_off.data_ptr(), nseg, bigs.data_ptr(), 0, 8,
                                                          out.data_ptr(), sel.data_ptr(), high.data_ptr(), STORE, None)
        assert rc != 0 and "d_array" in err(hip) and "%d bytes short" % W in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_segments_where_sync(raw, nbytes // W + 1, W, big.ctypes.data, nseg, bigs.data_ptr(), 0, 8,
                                                               h_out.ctypes.data, h_sel.ctypes.data, h_high.ctypes.data, STORE)
        assert rc != 0 and "d_array" in err(hip) and "%d bytes short" % W in err(hip), err(hip)
        end = raw + nbytes
        for so, sb, sel_ptr in ((0, 8, end - n + 1), (3, 1, end - (3 + n + 7) // 8 + 1)):
            rc = hip.FLAGSTATS_hip_device_wide_segments_where(a, n, W, f, nseg, sel_ptr, so, sb, out.data_ptr(), sel.data_ptr(), high.data_ptr(),
                                                              0, None)
            assert rc != 0 and "d_sel" in err(hip) and "1 bytes short" in err(hip), (sb, err(hip))
        for name, kw in (("d_out", {"d_out": end - nseg * 256 + 8}), ("d_selected", {"d_selected": end - nseg * 8 + 8}),
                         ("d_high", {"d_high": end - nseg * 8 + 8}), ("d_offsets", {"d_offsets": end - (nseg + 1) * 8 + 8})):
            k = {**good, **kw}
            rc = hip.FLAGSTATS_hip_device_wide_segments_where(a, n, W, k["d_offsets"], nseg, sd, 0, 8, k["d_out"], k["d_selected"], k["d_high"],
                                                              0, None)
            assert rc != 0 and name in err(hip) and "8 bytes short" in err(hip), (name, err(hip))
        back = np.ones(nbytes, dtype=np.uint8)
        assert hip.FLAGSTATS_hip_memcpy_d2h(back.ctypes.data, raw, nbytes) == 0 and not back.any()
    finally:
        hip.FLAGSTATS_hip_device_free(raw)
    untouched("extents")
    # the launcher itself -- nothing queued: (d_chunk, W, d_sel, sel_offset, sel_bits, base, m, d_offsets, nseg, out, sel, high, mode, grid)
    p, ps, ph = out.data_ptr(), sel.data_ptr(), high.data_ptr()
    ok = [a, W, sd, 0, 8, 0, 8, f, nseg, p, ps, ph, 0, 1]
    for i, bad in ((1, 2), (1, 16), (4, 0), (4, 4), (12, 4), (13, 0), (9, None), (7, None), (0, None), (2, None), (0, a + W // 2),
                   (6, 1 << 34), (6, (1 << 64) // W), (3, (1 << 64) - 5)):
        args = list(ok)
        args[i] = bad
        assert launcher(*args, None) != 0, (i, bad)
    assert launcher(a, W, None, 0, 8, 0, 8, f, 0, None, None, None, STORE, 1, None) == 0     # nseg == 0
    assert launcher(None, W, None, 0, 1, 0, 0, f, nseg, p, ps, ph, 0, 1, None) == 0          # m == 0 in the += form: nothing queued
    torch.cuda.synchronize()
    untouched("launcher")


# ------------------------------------------------------------------ 12. seeded randomised sweep
def random_layout(rng, n, kind, U):
    if kind == "long":
        cuts = np.sort(rng.randint(0, n + 1, rng.randint(1, 6)))
    elif kind == "short":
        cuts = np.sort(rng.randint(0, n + 1, min(n, 400)))
    elif kind == "empty":
        cuts = np.sort(np.repeat(rng.randint(0, n + 1, 12), rng.randint(1, 4, 12)))
    else:                                                   # gapped: begins and ends well inside the array
        lo, hi = sorted(rng.randint(0, n + 1, 2))
        cuts = np.sort(rng.randint(lo, hi + 1, 20))
    return cuts.astype(np.int64)


def test_seeded_randomised_sweep(hip, launcher):
    """random W, phase, sel_offset, form, mode, layout (long, short, empty, gapped) and density over arrays of at most a few hundred
    thousand elements, through the launcher at a random grid and chain threshold, against the oracle"""
    rng = np.random.RandomState(20_261_020)
    arenas = {W: Arena(UNSIGNED[W], poison(W)) for W in WIDTHS}
    sels = Arena(np.uint8, 0xFF, pad=16)
    todo = []
    kinds = ("long", "short", "empty", "gapped")
    for case in range(48):
        W = WIDTHS[rng.randint(0, 2)]
        U = 8192 // W
        n = int(rng.choice([1, 5, U - 1, U + 3, 7 * U + 11, 40 * U - 5, rng.randint(1, 300_000)]))
        kind = kinds[case % 4]
        o = random_layout(rng, n, kind, U)
        if o.size < 2:
            o = np.array([0, n], dtype=np.int64)
        density = float(rng.choice([0.0, 0.02, 0.5, 0.97, 1.0]))
        mask = rng.random_sample(n) < density
        clean = column(rng, n, W)
        clean[rng.randint(0, n, max(1, n // 50))] |= UNSIGNED[W](1) << UNSIGNED[W](rng.randint(16, 8 * W))
        x, sel_set = poisoned(clean, mask, o, W)
        want = swwo.want(x, o, mask, True)
        sel_bits = BITMAP if rng.randint(0, 3) else BYTES
        where = int(rng.choice([0, rng.randint(0, 8), rng.randint(8, 100_000)]))
        data, ph, off = encode(sel_set, sel_bits, where, value=int(rng.randint(1, 256)))
        phase = int(rng.randint(0, 16 // W))
        todo.append((W, n, o, want, arenas[W].add(x, phase), sels.add(data, ph), off, sel_bits, MODES[rng.randint(0, 4)],
                     int(rng.choice([1, 2, 7, 256])), int(rng.choice([0, 1, 2, 3, NEVER])), (case, W, n, kind, density, sel_bits, where, phase)))
    for a in arenas.values():
        a.upload()
    sels.upload()
    batch, calls = Batch(), []
    for W, n, o, want, a_at, s_at, off, sel_bits, mode, grid, mu, note in todo:
        calls.append((batch.add(mode, want, note + (mode, grid, mu)), W, n, dev64(o), arenas[W].ptr(a_at), sels.ptr(s_at), off, sel_bits, grid, mu))
    batch.upload()
    for k, W, n, d_off, aptr, sptr, off, sel_bits, grid, mu in calls:
        with policy(hip, mu):
            direct(launcher, batch, k, aptr, W, sptr, off, sel_bits, 0, n, d_off, grid)
    batch.check()
    assert sum(int(t[3][1].sum()) for t in todo) > 100_000 and any(t[3][2].any() for t in todo)
