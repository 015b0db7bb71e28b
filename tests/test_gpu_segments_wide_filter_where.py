"""Segmented flagstat of int32 / int64 columns under samtools' filter and a selection together on the MI355X
(csrc/flagstat_segments_wide_filter_where.hip and the layers above it): rows, the number of counted elements and one high-bit mask
of the SELECTED elements per segment, against tests/segments_wide_filter_where_oracle.py; every comparison is exact.

Expected values never come from the code under test.  Decoys are placed so that a wrong AND shows: every unselected slot, every
element in front of offsets[0] and behind offsets[nseg] holds flags that PASS the predicate, every bit above bit 15 and a MAPQ of
255; the selection is SET outside every segment and clear in the unselected slots; the bytes around the array are all-ones (they
pass every predicate without `exclude` bits); unused bits of a bitmap's first and last byte are set.  Selected elements that fail
the predicate carry high bits that must reach high[i] and no counter.  The plumbing (device words prefilled with garbage or
biases, arenas of arrays at chosen phases, the selection encodings, the policy switch) is tests/test_gpu_segments_wide_where.py's."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_wide_filter_oracle as swfo  # noqa: E402
import segments_wide_filter_where_oracle as swfwo  # noqa: E402
import segments_wide_oracle as swo  # noqa: E402
import segments_wide_where_oracle as swwo  # noqa: E402
import test_gpu_segments_wide_where as base  # noqa: E402  (helpers only: its tests are collected from its own file)
from segments_wide_where_oracle import BITMAP, BYTES, pack, poison  # noqa: E402
from test_gpu_segments_wide_where import (EVERY_MIN_UNITS, MODES, NEVER, SIGNED, STORE, UNSIGNED, WIDTHS, Arena, Batch, dev, dev64,  # noqa: E402
                                          encode, err, expect, host_words, policy, same, u64)

pytestmark = pytest.mark.gpu

F904Q30 = (0, 0x904, 30)        # samtools view -F 0x904 -q 30
PREDICATES = (F904Q30, (0x1, 0x4, 0), (0, 0, 0), (0x40, 0x100, 1))
FORMS = ((BITMAP, 0), (BITMAP, 5), (BYTES, 3))


@pytest.fixture(scope="module")
def launcher(hip):
    hip.fsk_segments_policy.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    hip.fsk_segments_policy.restype = None
    hip.fsk_set_segments_policy.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    hip.fsk_set_segments_policy.restype = None
    return hip.fsk_launch_segments_wide_masked_filter   # prototype attached by _lib.lib()


def all_high(W):
    return UNSIGNED[W](int(poison(W)) & ~0xFFFF)


def scene(rng, n, W, o, mask, pred, low=None, mapq=None, hot_every=11):
    """The three columns as the kernel gets them and as the oracle gets them.  Returns (x, sel_set, mapq): x holds, in the selected
    slots of the segments, flags of which some are all-zero and every `hot_every`-th or so carries bits above bit 15 whether it
    passes or not; every other slot holds a decoy: flags that pass, all high bits, MAPQ 255.  sel_set is what the selection
    encodes: the mask inside the segments, SET outside them.  The oracle takes (x, mask, mapq)."""
    require, exclude, _ = pred
    UT = UNSIGNED[W]
    idx = np.arange(n)
    low = (rng.randint(0, 65536, n) if low is None else np.resize(low, n)).astype(UT)
    low[rng.randint(0, n, n // 40 + 1)] = 0
    x = low.copy()
    hot = rng.randint(0, hot_every, n) == 0
    x[hot] |= (UT(1) << (16 + idx[hot] % 13).astype(UT))
    if W == 8:
        x[hot] |= (UT(1) << (40 + idx[hot] % 24).astype(UT))
    mask = np.asarray(mask, dtype=bool)
    inside = np.zeros(n, dtype=bool)
    inside[int(o[0]):int(o[-1])] = True
    decoy = ~mask | ~inside
    passing = (low & UT(0xFFFF & ~exclude)) | UT(require)
    x[decoy] = passing[decoy] | all_high(W)
    q = (rng.randint(0, 61, n) if mapq is None else np.resize(mapq, n)).astype(np.uint8)
    q[decoy] = 255
    return x, np.where(inside, mask, True), q


def want_of(x, o, mask, q, pred):
    return swfwo.want(x, o, mask, pred[0], pred[1], q if pred[2] else None, pred[2], True)


def shows_what_it_is_there_for(x, o, mask, q, pred, want):
    """the input holds selected elements that fail and carry high bits (they reach `high` and no counter), and unselected ones
    that would pass"""
    if pred[0] & pred[1]:
        return
    counted = swfwo.counted_mask(x, mask, pred[0], pred[1], q if pred[2] else None, pred[2])
    inside = np.zeros(x.size, dtype=bool)
    inside[int(o[0]):int(o[-1])] = True
    if any(pred):
        failing = mask & ~counted & inside
        assert failing.any() and (x[failing] >> 16).any()
    would = swfwo.counted_mask(x, ~mask & inside, pred[0], pred[1], q if pred[2] else None, pred[2])
    assert would.sum() == (~mask & inside).sum()
    assert int(want[1].sum()) == int((counted & inside).sum())


def direct(launcher, batch, k, aptr, W, qptr, sptr, sel_offset, sel_bits, base_, m, d_off, pred, grid, stream=None):
    """one launch of the internal launcher into the batch's words of launch k"""
    rc = launcher(aptr, W, qptr if pred[2] else None, sptr, sel_offset, sel_bits, base_, m, d_off.data_ptr(), batch.nseg(k), pred[0], pred[1],
                  pred[2], batch.out(k), batch.selected(k), batch.high(k), batch.mode(k), grid, stream)
    assert rc == 0, (batch.items[k][4], rc)


def device_entry(hip, batch, k, aptr, n, W, qptr, sptr, sel_offset, sel_bits, d_off, pred, stream=None):
    rc = hip.FLAGSTATS_hip_device_wide_segments_filter_where(aptr, n, W, d_off.data_ptr(), batch.nseg(k), pred[0], pred[1],
                                                             qptr if pred[2] else None, pred[2], sptr, sel_offset, sel_bits, batch.out(k),
                                                             batch.selected(k), batch.high(k), batch.mode(k), stream)
    assert rc == 0, (batch.items[k][4], err(hip))


def sync_form(hip, ptr, n, W, offsets, qptr, sptr, sel_offset, sel_bits, pred, mode):
    o = np.ascontiguousarray(offsets, dtype=np.uint64)
    rows, sel, high = host_words(o.size - 1, mode)
    rc = hip.FLAGSTATS_hip_device_wide_segments_filter_where_sync(ptr, n, W, o.ctypes.data, o.size - 1, pred[0], pred[1],
                                                                  qptr if pred[2] else None, pred[2], sptr, sel_offset, sel_bits,
                                                                  rows.ctypes.data, sel.ctypes.data, high.ctypes.data, mode)
    assert rc == 0, err(hip)
    return rows, sel, high


def host_form(hip, x, offsets, q, s, sel_offset, sel_bits, pred, mode):
    o = np.ascontiguousarray(offsets, dtype=np.uint64)
    rows, sel, high = host_words(o.size - 1, mode)
    rc = hip.FLAGSTATS_hip_wide_x64_segments_filter_where(x.ctypes.data, x.size, x.dtype.itemsize, o.ctypes.data, o.size - 1, pred[0], pred[1],
                                                          q.ctypes.data if pred[2] else None, pred[2], s.ctypes.data, sel_offset, sel_bits,
                                                          rows.ctypes.data, sel.ctypes.data, high.ctypes.data, mode)
    assert rc == 0, err(hip)
    return rows, sel, high


def phases(W):
    """the array 0, W and 12 bytes behind a 16-byte boundary, in elements (12 bytes: 4-byte elements only)"""
    return sorted({0, 1} | ({12 // W} if 12 % W == 0 else set()))


# ------------------------------------------------------------------ 1. which bit or byte and which MAPQ byte belongs to which element
@functools.lru_cache(maxsize=None)
def mapping_cases(W):
    """one marked element moved through the vector, row and unit seams: marked by the selection (every MAPQ passes), or by its
    MAPQ byte (every element selected); computed once per W"""
    EPV, R, U = 16 // W, 1024 // W, 8192 // W
    n = 3 * U + 5
    rng = np.random.RandomState(101)
    layouts = (np.array([0, n], dtype=np.int64), np.array([0, U - 3, 2 * U + 1, n], dtype=np.int64))
    cases = []
    for pos in sorted({0, EPV - 1, EPV, 7, 8, R - 1, R, U - 2, U - 1, U, U + 1, 2 * U - 1, 2 * U, n - 1}):
        for by_mapq in (False, True):
            mask = np.ones(n, dtype=bool) if by_mapq else np.arange(n) == pos
            q = np.where(np.arange(n) == pos, 41, 0) if by_mapq else np.full(n, 200)
            for pred in ((0, 0, 30),) if by_mapq else ((0, 0, 30), (0, 0, 0)):
                x, sel_set, qq = scene(rng, n, W, layouts[0], mask, pred, mapq=q, hot_every=1)
                wants = [want_of(x, o, mask, qq, pred) for o in layouts]
                assert all(int(w[1].sum()) == 1 and int(w[2].sum()) for w in wants)
                cases.append((x, sel_set, qq, pred, wants))
    return n, layouts, cases


@pytest.mark.parametrize("sel_bits", [BITMAP, BYTES])
@pytest.mark.parametrize("W", WIDTHS)
def test_which_bit_byte_and_mapq_byte_belongs_to_which_element(hip, launcher, W, sel_bits):
    """n = 3 U + 5; the array 0, W and 12 bytes behind a 16-byte boundary x every sel_offset & 7 and one offset above 8,000 (the
    MAPQ column at the byte alignment its arena gives it, which differs per case); exactly one element counts -- the selected one,
    or the one whose MAPQ passes -- and it carries high bits; every other slot is a decoy or a selected element whose MAPQ fails;
    one segment and the same cut into three; min_units 1 (chain) and 0xFFFFFFFF (per-piece only)"""
    n, layouts, cases = mapping_cases(W)
    sel_offsets = list(range(8)) + [8013]
    arrays, sels, mapqs = Arena(UNSIGNED[W], poison(W)), Arena(np.uint8, 0xFF, pad=16), Arena(np.uint8, 0xFF, pad=16)
    a_at = [[arrays.add(x, phase) for x, _, _, _, _ in cases] for phase in phases(W)]
    q_at = [mapqs.add(q, c % 5) for c, (_, _, q, _, _) in enumerate(cases)]
    s_at = [[(sels.add(data, ph), off) for data, ph, off in (encode(sel_set, sel_bits, so) for so in sel_offsets)] for _, sel_set, _, _, _ in cases]
    arrays.upload(), sels.upload(), mapqs.upload()
    d_offs = [dev64(o) for o in layouts]
    batch, calls = Batch(), []
    i = 0
    for mu in (1, NEVER):
        for pi in range(len(phases(W))):
            for c, (_, _, _, pred, wants) in enumerate(cases):
                for s, (at, off) in enumerate(s_at[c]):
                    for lay in range(2):
                        mode = MODES[i % 4]
                        i += 1
                        k = batch.add(mode, wants[lay], (W, sel_bits, mu, pi, c, sel_offsets[s], lay))
                        calls.append((mu, k, arrays.ptr(a_at[pi][c]), mapqs.ptr(q_at[c]), sels.ptr(at), off, lay, pred))
    batch.upload()
    for mu in (1, NEVER):
        with policy(hip, mu):
            for m, k, aptr, qptr, sptr, off, lay, pred in calls:
                if m == mu:
                    direct(launcher, batch, k, aptr, W, qptr, sptr, off, sel_bits, 0, n, d_offs[lay], pred, 2)
    batch.check()


# ------------------------------------------------------------------ 2. seams inside a vector, a selection byte and a MAPQ dword
@pytest.mark.parametrize("W", WIDTHS)
def test_seams_inside_a_vector_a_selection_byte_and_a_mapq_dword(hip, launcher, W):
    """segments of length 0, 1, 2, ... with every boundary position in [U - 10, U + 10], [R - 10, R + 10], [0, 10] and
    [n - 10, n] (segments that begin at lo0 and end at hi0 among them); masks 0101..., 0011... and all-set; a MAPQ column that
    changes sides every third element; neighbours are elements of other segments, gaps are decoys, selected; offsets[0] > 0, empty
    segments, and a layout whose first segment begins beyond whole units, which are skipped unread"""
    EPV, U = 16 // W, 8192 // W
    n = 4 * U + 21
    rng = np.random.RandomState(7)
    layouts = base.seam_layouts(W, n)
    assert layouts[0][0] == 0 and layouts[0][-1] == n and layouts[2][0] == 3 and layouts[3][0] >= 2 * U and (np.diff(layouts[0]) == 0).any()
    idx = np.arange(n)
    masks = (idx % 2 == 1, idx % 4 >= 2, np.ones(n, dtype=bool))
    arrays, sels, mapqs = Arena(UNSIGNED[W], poison(W)), Arena(np.uint8, 0xFF, pad=16), Arena(np.uint8, 0xFF, pad=16)
    todo = []
    for li, o in enumerate(layouts):
        for mi, mask in enumerate(masks):
            pred = (F904Q30, (0, 0, 0), (0x1, 0x4, 0))[(li + mi) % 3]
            x, sel_set, q = scene(rng, n, W, o, mask, pred, mapq=np.where(idx % 3 == 0, 10, 50))
            want = want_of(x, o, mask, q, pred)
            shows_what_it_is_there_for(x, o, mask, q, pred, want) if mi < 2 else None
            q_at = mapqs.add(q, (li + mi) % 4)
            for phase in range(EPV):
                at = arrays.add(x, phase)
                for sel_bits, where in FORMS:
                    data, ph, off = encode(sel_set, sel_bits, where, value=0x80)
                    todo.append((li, want, at, q_at, sels.add(data, ph), off, sel_bits, pred, (W, li, mi, phase, sel_bits, where)))
    arrays.upload(), sels.upload(), mapqs.upload()
    d_offs = [dev64(o) for o in layouts]
    batch, calls = Batch(), []
    i = 0
    for mu in (1, NEVER):
        for li, want, at, q_at, s_at, off, sel_bits, pred, note in todo:
            k = batch.add(MODES[i % 4], want, note + (mu,))
            i += 1
            calls.append((mu, k, arrays.ptr(at), mapqs.ptr(q_at), sels.ptr(s_at), off, sel_bits, li, pred))
    batch.upload()
    for mu in (1, NEVER):
        with policy(hip, mu):
            for m, k, aptr, qptr, sptr, off, sel_bits, li, pred in calls:
                if m == mu:
                    direct(launcher, batch, k, aptr, W, qptr, sptr, off, sel_bits, 0, n, d_offs[li], pred, 1)
    batch.check()


# ------------------------------------------------------------------ 3. the decoys: `high` and the counters per segment
@pytest.mark.parametrize("W", WIDTHS)
def test_decoys_reach_no_counter_and_only_selected_elements_reach_high(hip, launcher, W):
    """per segment: unselected elements with passing flags and every high bit, selected elements that fail and carry the
    segment's own bit (in high[i], in no counter), decoys in the gaps and in the neighbours, MAPQ 255 under every decoy, all-zero
    selected elements under a predicate with require == 0 (counted) and with require != 0 (not counted)"""
    U = 8192 // W
    rng = np.random.RandomState(13)
    lengths = np.concatenate([[1, 2, 3, 0, 5, 3 * U + 7, 1, U, 2 * U + 1, 0, 9], rng.randint(1, 300, 30)])
    o = 6 + np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(o[-1]) + 9
    nseg = o.size - 1
    mask = rng.randint(0, 2, n).astype(bool)
    mask[o[:-1][lengths > 0]] = True
    w = swo.writer_ranges(W, n, 1, W)                     # the array lies one element past a 16-byte boundary
    assert (w.pieces(o, 1)["chain"] > 0).any()
    arrays, sels, mapqs = Arena(UNSIGNED[W], poison(W)), Arena(np.uint8, 0xFF, pad=16), Arena(np.uint8, 0xFF, pad=16)
    todo = []
    for pred in PREDICATES:
        UT = UNSIGNED[W]
        x, sel_set, q = scene(rng, n, W, o, mask, pred, hot_every=10 ** 9)     # no random high bits: the segment's own bit below
        inside_sel = mask.copy()
        inside_sel[:int(o[0])] = inside_sel[int(o[-1]):] = False
        zero = inside_sel & (rng.randint(0, 5, n) == 0)
        x[zero] = 0                                                              # all-zero selected elements
        counted = swfwo.counted_mask(x, mask, pred[0], pred[1], q if pred[2] else None, pred[2])
        for i in range(nseg):                                                    # the selected elements that FAIL carry the segment's bit
            b, e = int(o[i]), int(o[i + 1])
            fails = np.flatnonzero(mask[b:e] & ~counted[b:e]) + b
            x[fails] |= UT(1 << (16 + i % 16)) | (UT(1 << (32 + i % 32)) if W == 8 else UT(0))
        want = want_of(x, o, mask, q, pred)
        assert np.array_equal(swfwo.counted_mask(x, mask, pred[0], pred[1], q if pred[2] else None, pred[2]), counted)
        z = int((zero & counted).sum())
        assert (z > 0) == (pred[0] == 0) and zero.any(), (pred, z)               # zeros count exactly when nothing is required
        if any(pred):
            for i in np.flatnonzero(want[2]).tolist():
                assert int(want[2][i]) == (1 << (16 + i % 16)) | ((1 << (32 + i % 32)) if W == 8 else 0), i
            assert want[2].any()
        a_at, q_at = arrays.add(x, 1), mapqs.add(q, 3)
        for sel_bits, where in FORMS:
            data, ph, off = encode(sel_set, sel_bits, where, value=7)
            todo.append((want, a_at, q_at, sels.add(data, ph), off, sel_bits, pred))
    arrays.upload(), sels.upload(), mapqs.upload()
    d_off = dev64(o)
    batch, calls = Batch(), []
    for mu in (1, NEVER):
        for want, a_at, q_at, s_at, off, sb, pred in todo:
            for mode in MODES:
                calls.append((mu, batch.add(mode, want, (W, mu, off, sb, mode, pred)), arrays.ptr(a_at), mapqs.ptr(q_at), sels.ptr(s_at), off, sb, pred))
    batch.upload()
    for mu in (1, NEVER):
        with policy(hip, mu):
            for m, k, aptr, qptr, sptr, off, sb, pred in calls:
                if m == mu:
                    direct(launcher, batch, k, aptr, W, qptr, sptr, off, sb, 0, n, d_off, pred, 1)
    batch.check()


# ------------------------------------------------------------------ 4. chain, epochs and regime changes
@pytest.mark.parametrize("W", WIDTHS)
def test_chain_epochs_and_regime_changes(hip, launcher, W):
    """launcher grid 1 (four writers) over ~16 MiB of an aligned array: chains of 254, 255, 256 and 2 * 255 + 3 units inside one
    segment, a segment ending exactly at an epoch, chain -> per-piece -> chain, a skipped stretch -> chain; a plain and a funnelled
    bit offset and the byte form, with and without the MAPQ column.  The first segment of one layout begins with element 0 and is
    three whole units long: grid unit 0 of the funnelled launch is a per-piece unit through the guarded loaders inside a segment
    whose other units are chained"""
    U = 8192 // W
    n = 4 * 516 * U - 9
    rng = np.random.RandomState(17)
    pattern = rng.randint(0, 65536, base.P)
    mask = np.resize(rng.randint(0, 2, 8191).astype(bool), n)
    mq = rng.randint(0, 61, 8179)
    w = swo.writer_ranges(0, n, 1, W)
    assert w.waves == 4 and w.lo0 == 0 and all(int(e - b) >= 515 * U for b, e in zip(w.begin, w.end))
    layouts = [base.chain_layout(w, n, 0), base.chain_layout(w, n, 3 * U)]
    preds = (F904Q30, (0x1, 0x4, 0))
    for o in layouts:
        pieces = w.pieces(o, 2)
        runs = {int(c): (int(h), int(t)) for c, h, t in zip(pieces["chain"], pieces["head"], pieces["tail"]) if c in (254, 255, 256, 513)}
        assert runs == {254: (3, 5), 255: (3, 0), 256: (3, 5), 513: (3, 5)}, runs
        assert int(pieces["chain"][0]) == 3 and int(pieces["head"][0]) == 0
    arrays, sels, mapqs = Arena(UNSIGNED[W], poison(W)), Arena(np.uint8, 0xFF, pad=16), Arena(np.uint8, 0xFF, pad=16)
    todo = []
    for li, (o, pred) in enumerate(zip(layouts, preds)):
        x, sel_set, q = scene(rng, n, W, o, mask, pred, low=pattern, mapq=mq, hot_every=97)
        want = want_of(x, o, mask, q, pred)
        assert want[2].any() and (want[1][np.diff(o) > 5000] > 0).all() and (want[1] < np.diff(o).astype(np.uint64)).all()
        at, q_at = arrays.add(x, 0), mapqs.add(q, 1)
        for sel_bits, where in ((BITMAP, 0), (BITMAP, 5), (BYTES, 1)):
            data, ph, off = encode(sel_set, sel_bits, where)
            todo.append((li, want, at, q_at, sels.add(data, ph), off, sel_bits, where, pred))
    arrays.upload(), sels.upload(), mapqs.upload()
    assert arrays.ptr(todo[0][2]) % 16 == 0
    d_offs = [dev64(o) for o in layouts]
    batch, calls = Batch(), []
    for li, want, at, q_at, s_at, off, sel_bits, where, pred in todo:
        for mode in (3, 0):
            calls.append((batch.add(mode, want, (W, li, sel_bits, where, mode)), arrays.ptr(at), mapqs.ptr(q_at), sels.ptr(s_at), off, sel_bits, li,
                          pred))
    batch.upload()
    with policy(hip, 2):
        for k, aptr, qptr, sptr, off, sel_bits, li, pred in calls:
            direct(launcher, batch, k, aptr, W, qptr, sptr, off, sel_bits, 0, n, d_offs[li], pred, 1)
        batch.check()
    del arrays, sels, mapqs


# ------------------------------------------------------------------ 5. every min_units through the three public entries
@pytest.mark.parametrize("W", WIDTHS)
def test_every_min_units_through_the_public_entries(hip, W):
    import torch
    U = 8192 // W
    rng = np.random.RandomState(29)
    n = 384 * U + 77
    o = np.array([9, 40, 40, U + 1, 2 * U + 5, 5 * U + 5, 8 * U + 7, 100 * U + 3, 100 * U + 9, 100 * U + 9 + 255 * U, n - 5], dtype=np.int64)
    mask = rng.randint(0, 3, n) > 0
    inputs = {}
    for pred in (F904Q30, (0x1, 0x4, 0)):
        x, sel_set, q = scene(rng, n, W, o, mask, pred)
        want = want_of(x, o, mask, q, pred)
        shows_what_it_is_there_for(x, o, mask, q, pred, want)
        assert want[2].any() and (want[1] > 0).sum() >= 8
        bits, byts = pack(sel_set, 5, fill=1), sel_set.astype(np.uint8)
        inputs[pred] = (x, q, want, bits, byts, dev(x), dev(q), dev(bits), dev(byts))
    t0 = inputs[F904Q30][5]
    w = swo.writer_ranges(t0.data_ptr() % 16, n, hip.FLAGSTATS_hip_compute_units(), W)
    longest = {mu: int(w.pieces(o, mu)["chain"].max()) for mu in EVERY_MIN_UNITS}
    assert longest[0] >= 1 and longest[1] >= 1 and longest[NEVER] == 0, longest
    d_off = dev64(o)
    for i, mu in enumerate(EVERY_MIN_UNITS):
        pred = (F904Q30, (0x1, 0x4, 0))[i % 2]
        x, q, want, bits, byts, t, d_q, d_bits, d_bytes = inputs[pred]
        sel_bits = BITMAP if i % 3 != 1 else BYTES
        d_s, h_s, off = (d_bits, bits, 5) if sel_bits == BITMAP else (d_bytes, byts, 0)
        with policy(hip, mu):
            batch = Batch()
            k = batch.add(3, want, (W, mu, "device"))
            batch.upload()
            device_entry(hip, batch, k, t.data_ptr(), n, W, d_q.data_ptr(), d_s.data_ptr(), off, sel_bits, d_off, pred)
            batch.check()
            same(sync_form(hip, t.data_ptr(), n, W, o, d_q.data_ptr(), d_s.data_ptr(), off, sel_bits, pred, 2), expect(want, 2), (W, mu, "sync"))
            same(host_form(hip, x, o, q, h_s, off, sel_bits, pred, 1), expect(want, 1), (W, mu, "host"))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 6. modes, NULL outputs, the overlapping pair, no MAPQ column, nothing to do
@pytest.mark.parametrize("W", WIDTHS)
def test_modes_null_outputs_and_the_calls_that_read_nothing(hip, launcher, W):
    """store and += (which ORs into high) with and without superset over garbage / bias words, through the launcher and the device
    entry; with d_selected and / or d_high NULL the words behind the rows stay untouched; require & exclude != 0 zeroes rows,
    counts and masks in the store form and leaves them alone in the += form; min_mapq == 0 runs with a NULL MAPQ column;
    nseg == 0 and n == 0"""
    U = 8192 // W
    rng = np.random.RandomState(33)
    n = 36 * U + 11
    o = np.array([0, 50, 3 * U + 1, 3 * U + 1, 20 * U - 7, 36 * U], dtype=np.int64)
    mask = rng.randint(0, 2, n).astype(bool)
    preds = (F904Q30, (0x1, 0x4, 0), (0x10, 0x30, 0), (0x4, 0x4, 30))          # the last two: a bit both required and excluded
    arrays, sels, mapqs = Arena(UNSIGNED[W], poison(W)), Arena(np.uint8, 0xFF, pad=16), Arena(np.uint8, 0xFF, pad=16)
    todo = []
    for pred in preds:
        x, sel_set, q = scene(rng, n, W, o, mask, pred)
        want = want_of(x, o, mask, q, pred)
        if pred[0] & pred[1]:
            assert not want[0].any() and not want[1].any() and not want[2].any()
        else:
            assert want[2].any() and want[1][2] == 0 and want[1].any()
        a_at, q_at = arrays.add(x, 16 // W - 1), mapqs.add(q, 2)
        for (data, ph, off), sb in zip((encode(sel_set, BITMAP, 6), encode(sel_set, BYTES, 2)), (BITMAP, BYTES)):
            todo.append((want, a_at, q_at, sels.add(data, ph), off, sb, pred))
    arrays.upload(), sels.upload(), mapqs.upload()
    d_off = dev64(o)
    batch, calls = Batch(), []
    for want, a_at, q_at, s_at, off, sb, pred in todo:
        for mode in MODES:
            for with_sel, with_high in ((True, True), (False, True), (True, False), (False, False)):
                for how in ("launcher", "entry"):
                    k = batch.add(mode, want, (W, sb, mode, with_sel, with_high, how, pred), with_sel, with_high)
                    # min_mapq == 0: the MAPQ column is NULL (direct / device_entry pass None)
                    calls.append((k, arrays.ptr(a_at), mapqs.ptr(q_at), sels.ptr(s_at), off, sb, how, pred))
    batch.upload()
    for k, aptr, qptr, sptr, off, sb, how, pred in calls:
        if how == "launcher":
            direct(launcher, batch, k, aptr, W, qptr, sptr, off, sb, 0, n, d_off, pred, 64)
        else:
            device_entry(hip, batch, k, aptr, n, W, qptr, sptr, off, sb, d_off, pred)
    batch.check()
    # nothing to do: nseg == 0 touches nothing; n == 0 zeroes in the store form and leaves the += words alone
    aptr, sptr = arrays.ptr(todo[0][1]), sels.ptr(todo[0][3])
    assert hip.FLAGSTATS_hip_device_wide_segments_filter_where(aptr, n, W, None, 0, 0, 0x904, None, 0, sptr, 6, BITMAP, None, None, None, STORE,
                                                               None) == 0
    assert hip.FLAGSTATS_hip_wide_x64_segments_filter_where(None, 0, W, None, 0, 0, 0, None, 0, None, 0, BITMAP, None, None, None, STORE) == 0
    empty = tuple(np.zeros(s, dtype=np.uint64) for s in ((2, 32), (2,), (2,)))
    d_zero = dev64(np.zeros(3, dtype=np.int64))
    batch = Batch()
    ks = [batch.add(mode, empty, (W, "n == 0", mode)) for mode in MODES]
    batch.upload()
    for k in ks:
        device_entry(hip, batch, k, None, 0, W, None, None, 0, BITMAP, d_zero, (0, 0x904, 0))
    batch.check()
    for mode in MODES:
        same(sync_form(hip, None, 0, W, [0, 0, 0], None, None, 0, BYTES, (0, 0, 0), mode), expect(empty, mode), (W, "sync n == 0", mode))


# ------------------------------------------------------------------ 7. equivalences
@pytest.mark.parametrize("W", WIDTHS)
def test_equivalences(hip, W):
    """an all-ones selection is the filtered segmented entry's triple; the empty predicate is the selected segmented entry's; one
    segment [0, n] is the whole-column filter_where entry's; values below 2^16 give the u16 segments_filter_where pair of the
    narrowed copy with high zero; the bitmap form and the byte form of the same mask agree -- each bit-exact, and the oracle says
    the same (all the kernels could be wrong alike)"""
    from libflagstats_amd import segments_filter_where as sfw
    from libflagstats_amd import segments_wide_filter_where as swfw
    U = 8192 // W
    rng = np.random.RandomState(41)
    n = 50 * U + 3
    mask = rng.randint(0, 3, n) > 0
    o = np.unique(np.concatenate([[7], rng.randint(7, n - 9, 30), [12 * U, 30 * U + 1, n - 9]])).astype(np.int64)
    nseg = o.size - 1
    o64 = o.astype(np.uint64)
    pred = F904Q30
    x, _, q = scene(rng, n, W, np.array([0, n]), mask, pred)        # decoys in the unselected slots; the gaps hold selected elements
    t, d_q = dev(x), dev(q)
    bits, byts = pack(mask, 3, fill=1), (mask * rng.randint(1, 256, n)).astype(np.uint8)
    d_bits, d_bytes = dev(bits), dev(byts)
    ones_bits, ones_bytes = dev(np.full((n + 7) // 8 + 1, 0xFF, dtype=np.uint8)), dev(np.full(n, 1, dtype=np.uint8))
    for mode in (1, 3):
        # all-ones selection: the filtered wide segmented entry
        ref = host_words(nseg, 1)
        rc = hip.FLAGSTATS_hip_device_wide_segments_filter_sync(t.data_ptr(), n, W, o64.ctypes.data, nseg, pred[0], pred[1], d_q.data_ptr(), pred[2],
                                                                ref[0].ctypes.data, ref[1].ctypes.data, ref[2].ctypes.data, mode)
        assert rc == 0, err(hip)
        assert ref[2].any() and ref[1].any()
        for d_s, off, sb in ((ones_bits, 2, BITMAP), (ones_bytes, 0, BYTES)):
            same(sync_form(hip, t.data_ptr(), n, W, o, d_q.data_ptr(), d_s.data_ptr(), off, sb, pred, mode), ref, (W, "all ones", sb, mode))
        same(ref, expect(swfo.want(x, o, pred[0], pred[1], q, pred[2], True), mode), (W, "all ones, oracle", mode))
        # empty predicate: the selected wide segmented entry
        ref = host_words(nseg, 1)
        rc = hip.FLAGSTATS_hip_device_wide_segments_where_sync(t.data_ptr(), n, W, o64.ctypes.data, nseg, d_bits.data_ptr(), 3, BITMAP,
                                                               ref[0].ctypes.data, ref[1].ctypes.data, ref[2].ctypes.data, mode)
        assert rc == 0, err(hip)
        for d_s, off, sb in ((d_bits, 3, BITMAP), (d_bytes, 0, BYTES)):
            same(sync_form(hip, t.data_ptr(), n, W, o, None, d_s.data_ptr(), off, sb, (0, 0, 0), mode), ref, (W, "empty predicate", sb, mode))
        same(ref, expect(swwo.want(x, o, mask, True), mode), (W, "empty predicate, oracle", mode))
        # one segment [0, n]: the whole-column entry
        for d_s, off, sb in ((d_bits, 3, BITMAP), (d_bytes, 0, BYTES)):
            got = sync_form(hip, t.data_ptr(), n, W, [0, n], d_q.data_ptr(), d_s.data_ptr(), off, sb, pred, mode)
            one = np.zeros(34, dtype=np.uint64)
            rc = hip.FLAGSTATS_hip_device_wide_filter_where_sync(t.data_ptr(), n, W, pred[0], pred[1], d_q.data_ptr(), pred[2], d_s.data_ptr(), off,
                                                                 sb, one.ctypes.data, one[32:].ctypes.data, one[33:].ctypes.data, mode)
            assert rc == 0, err(hip)
            assert np.array_equal(got[0][0], one[:32]) and got[1][0] == one[32] and got[2][0] == one[33] and 0 < int(one[32]) < n and one[33]
    # the bitmap form and the byte form of the same mask agree, and with the oracle
    want = want_of(x, o, mask, q, pred)
    a = sync_form(hip, t.data_ptr(), n, W, o, d_q.data_ptr(), d_bits.data_ptr(), 3, BITMAP, pred, 3)
    b = sync_form(hip, t.data_ptr(), n, W, o, d_q.data_ptr(), d_bytes.data_ptr(), 0, BYTES, pred, 3)
    same(a, b, (W, "bitmap against bytes"))
    same(a, want, (W, "oracle"))
    # values below 2^16: the u16 segments_filter_where pair of the narrowed copy, high zero
    low = (x & UNSIGNED[W](0xFFFF))
    narrow = low.astype(np.uint16)
    got = swfw.counters_segments_ints_filter_where(low.view(SIGNED[W]), o, bits, require=pred[0], exclude=pred[1], mapq=q, min_mapq=pred[2],
                                                   packed=True, bit_offset=3, superset=True)
    ref = sfw.counters_segments_filter_where(narrow, o, bits, require=pred[0], exclude=pred[1], mapq=q, min_mapq=pred[2], packed=True,
                                             bit_offset=3, superset=True)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and not got[2].any() and ref[1].any()
    # 16-bit input goes to those functions, high zero
    for dt in (np.int16, np.uint16):
        got = swfw.counters_segments_ints_filter_where(narrow.view(dt), o, bits, require=pred[0], exclude=pred[1], mapq=q, min_mapq=pred[2],
                                                       packed=True, bit_offset=3, superset=True)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and not got[2].any() and got[2].shape == (nseg,)


# ------------------------------------------------------------------ 8. host form across chunks
@pytest.mark.parametrize("W", WIDTHS)
def test_host_form_across_chunks(hip, W):
    """chunks of 8,193 int32 or 4,097 int64 elements from offsets[0] = 3 on: chunk seams fall inside a bitmap byte, inside a MAPQ
    dword and inside a segment; every chunk's staged array is aligned, so every chunk with (sel_offset + pos) & 7 != 0 is a
    funnelled launch whose unit 0 goes through the guarded loaders; elements in front of offsets[0] and behind offsets[nseg] are
    decoys whose bits and bytes are set and never cross the bus"""
    from libflagstats_amd import _lib
    from libflagstats_amd import segments_wide_filter_where as swfw
    rng = np.random.RandomState(53)
    chunk_flags = 16_386 if W == 4 else 16_388             # 8,193 int32 or 4,097 int64 a chunk: odd, so seams move through a byte
    c = chunk_flags * 2 // W
    assert c % 8 == 1
    n = 7 * c + 77
    first = 3
    o = np.array([first, 10, 10, first + c + 7, first + c + c // 2, first + 3 * c + c // 2 + 5, first + 4 * c, n - 20], dtype=np.int64)
    assert {(6 + first + k * c) & 7 for k in range(8)} == set(range(8))
    mask = rng.randint(0, 2, n).astype(bool)
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", chunk_flags), "chunk_flags")
        for pred in (F904Q30, (0x1, 0x4, 0), (0x4, 0x4, 0)):
            x, sel_set, q = scene(rng, n, W, o, mask, pred)
            xs = x.view(SIGNED[W])
            want = want_of(x, o, mask, q, pred)
            shows_what_it_is_there_for(x, o, mask, q, pred, want)
            assert bool(want[2][4]) == (not pred[0] & pred[1])                   # the segment that spans three chunks
            byte_sel = np.concatenate([[0xFF], sel_set.astype(np.uint8) * 0x80]).astype(np.uint8)[1:]      # one byte into its buffer
            q1 = np.concatenate([[0xFF], q]).astype(np.uint8)[1:]                                          # and so is the MAPQ column
            for s, off, sb in ((pack(sel_set, 6, fill=1), 6, BITMAP), (pack(sel_set, 0, fill=1), 0, BITMAP), (byte_sel, 0, BYTES)):
                for mode in MODES:
                    same(host_form(hip, xs, o, q1, s, off, sb, pred, mode), expect(want, mode), (W, "chunks", off, sb, mode, pred))
            kw = dict(require=pred[0], exclude=pred[1], mapq=q if pred[2] else None, min_mapq=pred[2], superset=True)
            same(swfw.counters_segments_ints_filter_where(xs, o, pack(sel_set, 6, fill=1), packed=True, bit_offset=6, **kw), want, (W, "packed"))
            same(swfw.counters_segments_ints_filter_where(xs, o, sel_set, **kw), want, (W, "python, bool"))
            for oo in (np.array([1, 50, 99]), np.array([7, 7, 7]), np.array([n, n])):        # one chunk only; nothing covered
                same(swfw.counters_segments_ints_filter_where(xs, oo, mask, **kw), want_of(x, oo, mask, q, pred), (W, oo))
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old
    got = swfw.counters_segments_ints_filter_where(xs[:0], [0, 0], mask[:0])
    assert got[0].shape == (1, 32) and not got[0].any() and not got[1].any() and not got[2].any()
    got = swfw.count_segments_device_ptr_ints_filter_where(0, 0, W, [0, 0, 0], 0, 1)
    assert got[0].shape == (2, 32) and not got[0].any() and not got[1].any() and not got[2].any()


# ------------------------------------------------------------------ 9. atomics
@pytest.mark.parametrize("W", WIDTHS)
def test_three_streams_add_into_one_set_of_rows(hip, W):
    import torch
    from libflagstats_amd import segments_wide_filter_where as swfw
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
    for j, (n, packed, bit_offset, density, pred) in enumerate(((36 * U + 11, True, 0, 50, F904Q30), (30 * U + 5, True, 5, 90, (0x1, 0x4, 0)),
                                                                (40 * U - 3, False, 0, 10, (0, 0x904, 0)))):
        mask = rng.randint(0, 100, n) < density
        oc = np.clip(o, 0, n)
        x, sel_set, q = scene(rng, n, W, oc, mask, pred)
        w = want_of(x, oc, mask, q, pred)
        assert w[1].any() and w[2].any()
        total[0] += w[0]
        total[1] += w[1]
        total[2] |= w[2]
        where = dev(pack(sel_set, bit_offset, fill=1)) if packed else dev(sel_set)
        inputs.append((dev(x), where, dev(q), packed, bit_offset, pred))
    streams = [torch.cuda.Stream() for _ in inputs]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    for st, (t, where, d_q, packed, bit_offset, pred) in zip(streams, inputs):
        with torch.cuda.stream(st):
            swfw.count_segments_torch_ints_filter_where(t, d_off, where, require=pred[0], exclude=pred[1], mapq=d_q if pred[2] else None,
                                                        min_mapq=pred[2], packed=packed, bit_offset=bit_offset, out=rows, selected=sel,
                                                        high=high, store=False, superset=True)
    for st in streams:
        st.synchronize()
    same((u64(rows), u64(sel), u64(high)), total, (W, "three streams"))


# ------------------------------------------------------------------ 10. the four Python functions
@pytest.mark.parametrize("W", WIDTHS)
def test_the_four_python_functions(hip, W):
    """counters_, flagstats_, count_segments_device_ptr_ and count_segments_torch_ (on a non-default current stream) against the
    oracle; strict raises on a selected value with high bits that FAILS the filter and names its segment, and does not raise for
    high bits in unselected slots"""
    import torch
    from libflagstats_amd import segments_filter, segments_wide_filter_where as swfw
    U = 8192 // W
    rng = np.random.RandomState(83)
    n = 9 * U + 100
    o = np.array([1, 600, 2 * U + 4, 2 * U + 4, 6 * U, n - 2], dtype=np.int64)
    mask = rng.randint(0, 3, n) > 0
    pred = F904Q30
    x, sel_set, q = scene(rng, n, W, o, mask, pred, hot_every=10 ** 9)          # high bits in the decoys only
    xs = x.view(SIGNED[W])
    kw = dict(require=pred[0], exclude=pred[1], mapq=q, min_mapq=pred[2])
    want = want_of(x, o, mask, q, pred)
    assert not want[2].any() and want[1].any()
    bits = pack(sel_set, 5, fill=1)
    same(swfw.counters_segments_ints_filter_where(xs, o, bits, packed=True, bit_offset=5, superset=True, **kw), want, (W, "counters"))
    dicts = swfw.flagstats_segments_ints_filter_where(xs, o, sel_set, **kw)       # garbage with high bits in unselected slots: no raise
    plain = swfwo.want(x, o, mask, pred[0], pred[1], q, pred[2], False)
    assert dicts == segments_filter.segment_filter_dicts(plain[0], plain[1]) and [d["n_values"] for d in dicts] == [int(v) for v in want[1]]
    # one selected element of segment 3 that fails (an excluded flag) carries a high bit: strict raises and names the segment
    j = int(np.flatnonzero(mask[2 * U + 4:6 * U])[0]) + 2 * U + 4
    y = x.copy()
    y[j] = UNSIGNED[W](0x904 | (1 << (8 * W - 1)))
    w2 = want_of(y, o, mask, q, pred)
    assert not swfwo.counted_mask(y, mask, pred[0], pred[1], q, pred[2])[j] and [int(v) for v in w2[2]] == [0, 0, 0, 1 << (8 * W - 1), 0]
    text = r"segment 3 \(offsets %d\.\.%d\): values outside 0\.\.65535: bits 0x%X set above bit 15" % (o[3], o[4], 1 << (8 * W - 1))
    with pytest.raises(ValueError, match=text):
        swfw.flagstats_segments_ints_filter_where(y.view(SIGNED[W]), o, sel_set, **kw)
    dicts = swfw.flagstats_segments_ints_filter_where(y.view(SIGNED[W]), o, sel_set, strict=False, **kw)
    assert [d["high_bits"] for d in dicts] == [int(v) for v in w2[2]] and [d["n_values"] for d in dicts] == [int(v) for v in w2[1]]
    # raw device pointers, synchronous
    t, d_q, d_bits, d_bytes = dev(y), dev(q), dev(bits), dev(sel_set)
    got = swfw.count_segments_device_ptr_ints_filter_where(t.data_ptr(), n, W, o, d_bits.data_ptr(), 1, sel_offset=5, require=pred[0],
                                                           exclude=pred[1], mapq_ptr=d_q.data_ptr(), min_mapq=pred[2], superset=True)
    same(got, w2, (W, "device pointers"))
    # torch tensors on a non-default current stream, store and then += into the same words
    d_off = dev64(o)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        rows, sel, high = swfw.count_segments_torch_ints_filter_where(t, d_off, d_bytes, require=pred[0], exclude=pred[1], mapq=d_q,
                                                                      min_mapq=pred[2], superset=True)
        swfw.count_segments_torch_ints_filter_where(t, d_off, d_bits, require=pred[0], exclude=pred[1], mapq=d_q, min_mapq=pred[2], packed=True,
                                                    bit_offset=5, out=rows, selected=sel, high=high, store=False, superset=True)
    st.synchronize()
    same((u64(rows), u64(sel), u64(high)), (w2[0] * np.uint64(2), w2[1] * np.uint64(2), w2[2]), (W, "torch, store then +="))


# ------------------------------------------------------------------ 11. seeded random sweep
SWEEP_SEED = 20261020


@pytest.mark.parametrize("W", WIDTHS)
def test_seeded_random_sweep(hip, launcher, W):
    """random offsets (empty and gapped segments included), densities, predicates, bit offsets, array phases and min_units
    against the oracle, through the launcher at small grids and the device entry"""
    print("segments_wide_filter_where sweep: seed", SWEEP_SEED, "W", W)
    EPV, U = 16 // W, 8192 // W
    rng = np.random.RandomState(SWEEP_SEED + W)
    arrays, sels, mapqs = Arena(UNSIGNED[W], poison(W)), Arena(np.uint8, 0xFF, pad=16), Arena(np.uint8, 0xFF, pad=16)
    todo, offs = [], []
    for case in range(24):
        n = int(rng.choice([rng.randint(1, 40), rng.randint(U - 20, U + 20), rng.randint(2 * U, 12 * U)]))
        cuts = np.sort(rng.randint(0, n + 1, rng.randint(2, 40)))
        cuts = np.sort(np.concatenate([cuts, cuts[rng.randint(0, cuts.size, 3)]]))          # empty segments
        if case % 3 == 0:
            cuts = np.concatenate([[0], cuts, [n]])
        keep = rng.randint(0, 4, cuts.size - 1) > 0                                         # gaps: a dropped segment ...
        o = cuts.astype(np.int64)
        density = float(rng.choice([0.0, 0.03, 0.5, 0.97, 1.0]))
        mask = rng.random_sample(n) < density
        for b, e, k in zip(o[:-1], o[1:], keep):
            if not k:
                mask[b:e] = False                                                            # ... is a stretch nothing selects: a decoy
        pred = (int(rng.choice([0, 0x1, 0x40, 0x3])), int(rng.choice([0, 0x904, 0x4, 0x200])), int(rng.choice([0, 1, 30, 200])))
        if pred[0] & pred[1]:
            pred = (pred[0], 0, pred[2])
        x, sel_set, q = scene(rng, n, W, o, mask, pred)
        want = want_of(x, o, mask, q, pred)
        at, q_at = arrays.add(x, int(rng.randint(0, EPV))), mapqs.add(q, int(rng.randint(0, 8)))
        sel_bits = BITMAP if case % 3 else BYTES
        data, ph, off = encode(sel_set, sel_bits, int(rng.randint(0, 64)), value=int(rng.randint(1, 256)))
        offs.append(o)
        todo.append((case, n, want, at, q_at, sels.add(data, ph), off, sel_bits, pred, int(rng.choice([0, 1, 2, 3, NEVER])),
                     int(rng.choice([1, 2, 64]))))
    arrays.upload(), sels.upload(), mapqs.upload()
    d_offs = [dev64(o) for o in offs]
    batch, calls = Batch(), []
    for case, n, want, at, q_at, s_at, off, sel_bits, pred, mu, grid in todo:
        for how in ("launcher", "entry"):
            k = batch.add(MODES[(case + (how == "entry")) % 4], want, (W, "sweep", case, n, sel_bits, off, pred, mu, grid, how))
            calls.append((k, case, n, arrays.ptr(at), mapqs.ptr(q_at), sels.ptr(s_at), off, sel_bits, pred, mu, grid, how))
    batch.upload()
    for k, case, n, aptr, qptr, sptr, off, sel_bits, pred, mu, grid, how in calls:
        with policy(hip, mu):
            if how == "launcher":
                direct(launcher, batch, k, aptr, W, qptr, sptr, off, sel_bits, 0, n, d_offs[case], pred, grid)
            else:
                device_entry(hip, batch, k, aptr, n, W, qptr, sptr, off, sel_bits, d_offs[case], pred)
    batch.check()
