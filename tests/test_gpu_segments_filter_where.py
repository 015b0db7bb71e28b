"""The filtered and selected segmented flagstat on the MI355X: fsk::flagstat_segments_filter_where in its five forms (bitmap at a
byte boundary of the array's grid or funnelled, with and without the MAPQ column; bytes with the column), the byte form without
-q through fsk::flagstat_segments_filter<true>, the launcher, the three C entries and libflagstats_amd/segments_filter_where.py.
Every comparison is exact.

Expected rows never come from the code under test: segments_filter_where_oracle.want is segments_oracle.segmented_counters of the
array with the flags zeroed that fail the filter or are not selected, slot 9 from the definition; the expected `selected` is the
per-segment sum of the combined mask.  Arrays, MAPQ columns and selections sit in poisoned slabs as tests/test_gpu_segments_where.py
arranges them (its Arena, Batch and layouts are used here): the flags around an array, in front of its first segment and behind its
last are poison that PASSES the predicate of the launch and is SELECTED, the selection bytes around a bitmap or mask are 0xFF and
the unused bits of a bitmap's first and last byte are set, the MAPQ bytes around a column are 255 -- anything counted from outside
its segment shows."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_filter_where_oracle as sfwo  # noqa: E402
from filter_where_oracle import combined_mask  # noqa: E402
from segments_oracle import SEG_EPOCH, writer_ranges  # noqa: E402
from segments_where_oracle import BITMAP, BYTES, pack  # noqa: E402
from test_gpu_segments_where import (BIAS, EVERY_MIN_UNITS, GARBAGE, MODES, N_CHAIN, ONE_HOT_VALUES, SEL_BIAS, STORE, SUPERSET, Arena,  # noqa: E402
                                     Batch, P, U, chain_layout, dev8, dev16, dev64, encode, err, expect, one_hot_layout, policy,
                                     tiny_offsets, u64)

pytestmark = pytest.mark.gpu

PREDICATES = ((0, 0x904, 0), (0x2, 0x904, 30), (0x0101, 0x8080, 128), (0x40, 0x44, 30))    # (require, exclude, min_mapq); the last overlaps
SEL_FORMS = ((BITMAP, 0), (BITMAP, 1), (BITMAP, 7), (BYTES, 1))                             # (sel_bits, bit offset or byte alignment)
GUARD = 0x6A6A_6A6A_6A6A_6A6A


def poison_of(require, exclude):
    """a FLAG value that passes (require, exclude) -- every bit but the excluded ones -- and so counts in many slots"""
    return 0xFFFF if require & exclude else 0xFFFF & ~exclude


def mapq_column(rng, n):
    """random MAPQ bytes with the values around the thresholds 30 and 128 spread over every position of a vector"""
    q = rng.randint(0, 256, n).astype(np.uint8)
    for k, val in enumerate((29, 30, 31, 127, 128, 129, 0, 255)):
        q[k * 5::89] = val
    return q


@pytest.fixture(scope="module")
def launcher(hip):
    hip.fsk_segments_policy.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    hip.fsk_segments_policy.restype = None
    hip.fsk_set_segments_policy.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    hip.fsk_set_segments_policy.restype = None
    return hip.fsk_launch_segments_filter_where


def launch(launcher, a, q, s, sel_offset, sel_bits, n, off, nseg, pred, batch, k, grid):
    """through the launcher on the null stream; without -q the column is NULL"""
    rc = launcher(a, q if pred[2] else None, s, sel_offset, sel_bits, 0, n, off, nseg, pred[0], pred[1], pred[2], batch.out(k),
                  batch.selected(k), batch.mode(k), grid, None)
    assert rc == 0, (batch.items[k][5], rc)


def device_entry(hip, a, q, s, sel_offset, sel_bits, n, off, nseg, pred, batch, k, stream=None):
    rc = hip.FLAGSTATS_hip_device_u16_segments_filter_where(a, n, off, nseg, pred[0], pred[1], q if pred[2] else None, pred[2], s, sel_offset,
                                                            sel_bits, batch.out(k), batch.selected(k), batch.mode(k), stream)
    assert rc == 0, (batch.items[k][5], err(hip))


# ------------------------------------------------------------------ 1. seams smaller than the selection's granularity
def test_seams_inside_a_vector_and_a_selection_byte(hip, launcher):
    """segments of lengths 1, 2, 3, 5 and 0 in turn: boundaries inside one vector, inside one selection byte and between the MAPQ
    bytes of one load, empty segments among them; layouts that start behind offsets[0] > 0 and end before n.  Array phases 0, 3,
    5 x bit offsets 0, 1, 7 and the byte form at alignment 1 x four predicates (the last an overlapping pair) x four layouts; the
    MAPQ column at alignments 0 and 1, grids 1 and 3 through the launcher and the device entry, the four modes and a NULL
    d_selected in turn"""
    n = 3 * U + 41
    rng = np.random.RandomState(303)
    values = rng.randint(0, 65536, n).astype(np.uint16)
    values[::7] &= np.uint16(0x0143)              # more values that pass the predicates
    mask = rng.randint(0, 2, n).astype(bool)
    mapq = mapq_column(rng, n)
    layouts = [tiny_offsets(3, n - 5), tiny_offsets(U - 3, 2 * U + 5), tiny_offsets(7, U - 40), tiny_offsets(U + 17, n - 1)]
    mask[:3], mask[n - 5:], mapq[:3], mapq[n - 5:] = True, True, 255, 255
    sels, offs, mapqs = Arena(np.uint8, 0xFF, pad=16), Arena(np.int64, 0, pad=0), Arena(np.uint8, 255, pad=16)
    o_at = [offs.add(o) for o in layouts]
    q_at = [mapqs.add(mapq, align) for align in (0, 1)]
    s_at = [(sels.add(data, sel_phase), sel_offset) for data, sel_phase, sel_offset in (encode(mask, sb, where, value=0x02) for sb, where in SEL_FORMS)]
    arenas, a_at, wants = [], {}, {}
    for pi, (require, exclude, min_mapq) in enumerate(PREDICATES):
        v = values.copy()
        v[:3], v[n - 5:] = poison_of(require, exclude), poison_of(require, exclude)
        arenas.append(Arena(np.uint16, poison_of(require, exclude)))
        for phase in (0, 3, 5):
            a_at[pi, phase] = arenas[pi].add(v, phase)
        c = combined_mask(v, mask, require, exclude, mapq, min_mapq)
        assert (c[:3].all() and c[n - 5:].all()) != bool(require & exclude)       # the flags outside the segments would count
        for li, o in enumerate(layouts):
            wants[pi, li] = sfwo.want(v, o, mask, require, exclude, mapq, min_mapq, superset=True)
            assert int(wants[pi, li][1].sum()) == int(c[o[0]:o[-1]].sum()) and bool(wants[pi, li][1].any()) != bool(require & exclude)
    batch, calls, seen = Batch(), [], set()
    i = 0
    for phase in (0, 3, 5):
        for fi in range(len(SEL_FORMS)):
            for pi in range(len(PREDICATES)):
                for li in range(len(layouts)):
                    grid = (1, 3, None)[(i + i // 4) % 3]
                    align = (i // 4 + i // 64) % 2
                    seen.add((fi, pi, grid))
                    seen.add((fi, pi, "align", align))
                    k = batch.add(MODES[i % 4], wants[pi, li][0], wants[pi, li][1], (phase, SEL_FORMS[fi], PREDICATES[pi], li, grid, align),
                                  with_selected=bool(i % 5))
                    calls.append((k, pi, a_at[pi, phase], q_at[align], fi, li, grid))
                    i += 1
    assert len(seen) == len(SEL_FORMS) * len(PREDICATES) * 5, len(seen)      # every form x predicate under every grid and alignment
    for a in arenas:
        a.upload()
    sels.upload(), offs.upload(), mapqs.upload()
    batch.upload()
    assert mapqs.ptr(q_at[0]) % 2 == 0 and mapqs.ptr(q_at[1]) % 2 == 1
    for k, pi, a, q, fi, li, grid in calls:
        nseg = layouts[li].size - 1
        args = (arenas[pi].ptr(a), mapqs.ptr(q), sels.ptr(s_at[fi][0]), s_at[fi][1], SEL_FORMS[fi][0], n, offs.ptr(o_at[li]), nseg, PREDICATES[pi],
                batch, k)
        if grid is None:
            device_entry(hip, *args)
        else:
            launch(launcher, *args, grid)
    batch.check()


# ------------------------------------------------------------------ 2. which bit / byte / MAPQ byte belongs to which flag
ONE_HOT_PRED = (0x0001, 0x0800, 30)               # every ONE_HOT_VALUES passes it


def one_hot_case(hip, launcher, combos):
    """combos: (phase, sel_bits, bit offset or byte alignment, MAPQ alignment, what is one-hot).  The array is passing poison
    everywhere but at one position p.
      "sel":  the selection selects p alone, every MAPQ byte passes (also without -q: the kernels without the column, and the
              byte form through the filtered segmented kernel);
      "mapq": everything is selected, the MAPQ byte of p alone passes (exactly min_mapq, among zeros).
    Exactly one row has exactly the counts of that one flag and `selected` 1 (none when p lies outside every segment).  p walks
    over the unit, row and vector seams of the layout (lane 63 | 0 among them), the segment boundaries and every position of a
    vector"""
    import torch
    require, exclude, min_mapq = ONE_HOT_PRED
    poison = poison_of(require, exclude)
    ones = {v: sfwo.want(np.array([v], dtype=np.uint16), [0, 1], [True], require, exclude, superset=True)[0][0] for v in ONE_HOT_VALUES}
    assert all(r.any() for r in ones.values())
    arrays, sels, mapqs, offs = Arena(np.uint16, poison), Arena(np.uint8, 0xFF, pad=16), Arena(np.uint8, 255, pad=16), Arena(np.int64, 0, pad=0)
    batch, calls = Batch(), []
    i = 0
    for phase, sel_bits, where, q_align, hot in combos:
        n, o, positions = one_hot_layout(phase)
        # ... and every position of a vector, in a per-flag unit (1) and in a chained one (2)
        positions = sorted(set(positions) | {k * U - phase + d for k in (1, 2) for d in range(8)})
        w = writer_ranges(2 * phase, n, 1)
        assert w.lo0 == phase
        pieces = w.pieces(o, 1)
        assert (pieces["chain"] > 0).sum() >= 2 and (pieces["chain"] == 0).any() and ((pieces["chain"] > 0) & (pieces["tail"] > 0)).any()
        a_at = arrays.add(np.full(n, poison, dtype=np.uint16), phase)
        o_at = offs.add(o)
        nseg = o.size - 1
        every = np.full(n, hot == "mapq")                     # "sel": nothing selected but p; "mapq": everything
        data, sel_phase, sel_offset = encode(every, sel_bits, where, value=0x80)
        s_at = sels.add(data, sel_phase)
        q_at = mapqs.add(np.full(n, 255 if hot == "sel" else 0, dtype=np.uint8), q_align)
        preds = ((require, exclude, min_mapq), (require, exclude, 0)) if hot == "sel" else ((require, exclude, min_mapq),)
        for pred in preds:
            for p in positions:
                v = ONE_HOT_VALUES[i % 3]
                want_rows, want_sel = np.zeros((nseg, 32), dtype=np.uint64), np.zeros(nseg, dtype=np.uint64)
                seg = int(np.searchsorted(o, p, side="right")) - 1
                if 0 <= seg < nseg and o[seg] <= p < o[seg + 1]:
                    want_rows[seg], want_sel[seg] = ones[v], 1
                k = batch.add(MODES[i % 4], want_rows, want_sel, (phase, sel_bits, where, q_align, hot, pred, p))
                if sel_bits == BITMAP:
                    s_idx, s_val = s_at + ((sel_offset + p) >> 3), 1 << ((sel_offset + p) & 7)
                else:
                    s_idx, s_val = s_at + p, (0x01, 0x80, 0xFF)[i % 3]
                calls.append((k, a_at, n, p, v, o_at, nseg, s_at, sel_offset, sel_bits, q_at, pred, hot, s_idx, s_val))
                i += 1
    arrays.upload(), sels.upload(), mapqs.upload(), offs.upload()
    batch.upload()
    flat, sflat, qflat = arrays.t, sels.t, mapqs.t
    with policy(hip, 1):
        for k, a_at, n, p, v, o_at, nseg, s_at, sel_offset, sel_bits, q_at, pred, hot, s_idx, s_val in calls:
            flat[a_at + p] = v                       # (stream-ordered with the launch on the null stream)
            if hot == "sel":
                sflat[s_idx] += s_val                # the byte held 0 (mask) or had this bit clear (bitmap)
            else:
                qflat[q_at + p] = pred[2]
            launch(launcher, arrays.ptr(a_at), mapqs.ptr(q_at), sels.ptr(s_at), sel_offset, sel_bits, n, offs.ptr(o_at), nseg, pred, batch, k, 1)
            flat[a_at + p] = np.uint16(poison).astype(np.int16).item()     # poison again
            if hot == "sel":
                sflat[s_idx] -= s_val
            else:
                qflat[q_at + p] = 0
    torch.cuda.synchronize()
    batch.check()


@pytest.mark.parametrize("hot", ["sel", "mapq"])
def test_which_bit_and_mapq_byte_belongs_to_which_flag(hip, launcher, hot):
    """the bitmap at a byte boundary of the array's grid (shift 0) and funnelled at shifts 1, 4 and 5, the MAPQ column at both
    alignments"""
    combos = [(0, BITMAP, 0, 1, hot), (0, BITMAP, 5, 0, hot), (3, BITMAP, 3, 0, hot), (3, BITMAP, 0, 1, hot), (5, BITMAP, 1, 1, hot),
              (6, BITMAP, 7, 0, hot)]
    assert [(off + 8 - phase) & 7 for phase, _, off, _, _ in combos] == [0, 5, 0, 5, 4, 1]
    one_hot_case(hip, launcher, combos)


@pytest.mark.parametrize("hot", ["sel", "mapq"])
def test_which_byte_and_mapq_byte_belongs_to_which_flag(hip, launcher, hot):
    """byte alignments 1, 0 and 15 x array phases 0, 3 and 6, selecting bytes 0x01, 0x80 and 0xFF in turn"""
    one_hot_case(hip, launcher, [(0, BYTES, 1, 0, hot), (3, BYTES, 0, 1, hot), (6, BYTES, 15, 1, hot)])


# ------------------------------------------------------------------ 3. chain, epochs and regime changes
@pytest.mark.parametrize("sel_bits,sel_offset", [(BITMAP, 3), (BITMAP, 0), (BYTES, 0)])
def test_chain_epochs_and_regime_changes(hip, launcher, sel_bits, sel_offset):
    """grid 1 over 1200 units of flags of period 65,521 under a mask of period 8,191 and MAPQ bytes of period 251, array phase 3,
    the column at an odd address: bit offset 3 puts the bitmap on a byte boundary of the grid (shift 0), bit offset 0 funnels it
    (shift 5); the bitmap forms with and without -q, the byte form with it.  All four modes over garbage / bias"""
    import torch
    n = N_CHAIN
    pattern = np.random.RandomState(405).randint(0, 65536, P).astype(np.uint16)
    pattern[::3] &= np.uint16(0xF6FB)             # a third of the flags pass -F 0x904 whatever their other bits
    mask_pattern = np.random.RandomState(406).randint(0, 2, 8191).astype(bool)
    mapq_pattern = mapq_column(np.random.RandomState(407), 251)
    poison = np.uint16(poison_of(0, 0x904)).astype(np.int16).item()
    slab = torch.full((n + 16,), poison, dtype=torch.int16, device="cuda")
    slab[3:3 + n] = dev16(np.resize(pattern, n))
    ptr = slab.data_ptr() + 2 * 3
    w = writer_ranges(ptr % 16, n, 1)
    assert w.waves == 4 and w.lo0 == 3
    if sel_bits == BITMAP:
        assert ((sel_offset + 8 - w.lo0) & 7 == 0) == (sel_offset == 3)
    o = chain_layout(w, n)
    pieces = w.pieces(o)
    w0 = pieces["writer"] == 0
    run = [int(c) for c in pieces["chain"][w0]]
    assert 257 in run and 20 in run and run.index(257) < run.index(20) and 0 in run[run.index(257) + 1:run.index(20)], run
    big = (pieces["chain"] == 257) & w0
    assert (pieces["head"][big] > 0).all() and (pieces["tail"][big] > 0).all() and pieces["plain"][big].all() and 257 > SEG_EPOCH
    assert ((pieces["chain"] > SEG_EPOCH) & ~pieces["plain"]).any() and ((pieces["chain"] > 0) & (pieces["head"] == 0)).any()
    assert (w0 & (pieces["chain"] == 0) & (pieces["e"] - pieces["b"] > U + 7)).any()     # a whole unit below min_units: per flag
    assert o[0] >= 3 * U                                          # units 0-2 are skipped unread
    mask = np.resize(mask_pattern, n)
    if sel_bits == BITMAP:
        data = pack(mask, sel_offset, fill=1)
        preds = ((0, 0x904, 30), (0, 0x904, 0))
    else:
        data = mask.astype(np.uint8) * np.uint8(0x80)
        preds = ((0, 0x904, 30),)
    d_sel = torch.full((16 + data.size + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    d_sel[16:16 + data.size] = dev8(data)
    d_mapq = torch.full((16 + 1 + n + 16,), 255, dtype=torch.uint8, device="cuda")
    d_mapq[17:17 + n] = dev8(np.resize(mapq_pattern, n))
    assert (d_mapq.data_ptr() + 17) % 2 == 1
    d_off = dev64(o)
    batch, ks = Batch(), []
    for pred in preds:
        want_rows, want_sel = sfwo.periodic_want(pattern, o, mask_pattern, pred[0], pred[1], mapq_pattern, pred[2], superset=True)
        assert (want_sel[np.diff(o) > 50] > 0).all() and (want_sel[np.diff(o) > 0] < np.diff(o)[np.diff(o) > 0].astype(np.uint64)).all()
        ks += [(batch.add(mode, want_rows, want_sel, (sel_bits, sel_offset, pred, mode)), pred) for mode in MODES]
    batch.upload()
    with policy(hip, 2):
        for k, pred in ks:
            launch(launcher, ptr, d_mapq.data_ptr() + 17, d_sel.data_ptr() + 16, sel_offset, sel_bits, n, d_off.data_ptr(), o.size - 1, pred,
                   batch, k, 1)
        batch.check()
    del slab, d_sel, d_mapq


# ------------------------------------------------------------------ 4. every min_units through the public entries
def test_every_min_units_through_the_public_entries(hip, launcher):
    """the segments policy's chain threshold 0, 1, 2, 3, 255, 256 and 0xFFFFFFFF (per flag everywhere) under the device entry, the
    _sync form and the host form; bitmap (bit offset 5) with -q, bytes with -q, bitmap without -q and bytes without -q (the
    dispatched form) in turn: the same rows and counts under every one"""
    import torch
    from libflagstats_amd import segments_filter_where as sfw
    n = (1 << 24) + 4099          # four units per writer at one workgroup per CU of 256 CUs
    pattern = np.random.RandomState(407).randint(0, 65536, P).astype(np.uint16)
    pattern[::3] &= np.uint16(0xF6FB)
    mask_pattern = np.random.RandomState(408).randint(0, 3, 13) > 0
    mapq_pattern = np.array([0, 29, 30, 31, 60, 255, 12, 30, 128, 7, 29, 200, 31], dtype=np.uint8)    # the mask's period: a joint period of 851,773
    x, m, q = np.resize(pattern, n), np.resize(mask_pattern, n), np.resize(mapq_pattern, n)
    t, d_q = dev16(x), dev8(q)
    bits = pack(m, 5, fill=1)
    d_bits, d_mask = dev8(bits), torch.from_numpy(m).cuda()
    rng = np.random.RandomState(19)
    lengths = rng.choice([3, 100, 4095, 4097, 2 * U + 5, 3 * U, 17 * U - 1, 300_007, 1_000_003], 40)
    o = np.concatenate([[13], 13 + np.cumsum(lengths)])
    o = np.append(o[o < n - 7], n - 7).astype(np.int64)
    d_off = dev64(o)
    cus = hip.FLAGSTATS_hip_compute_units()
    forms = ((True, 30), (False, 30), (True, 0), (False, 0))      # (packed, min_mapq)
    for i, mu in enumerate(EVERY_MIN_UNITS):
        sup = bool(i % 2)
        packed, min_mapq = forms[i % 4]
        want_rows, want_sel = sfwo.periodic_want(pattern, o, mask_pattern, 0x2 * (i % 3 == 0), 0x904, mapq_pattern, min_mapq, superset=sup)
        pred = {"require": 0x2 * (i % 3 == 0), "exclude": 0x904, "min_mapq": min_mapq}
        assert want_sel.any()
        chain = writer_ranges(t.data_ptr() % 16, n, cus).pieces(o, mu)["chain"]
        assert (chain.max() > 0) == (mu <= 3), (mu, chain.max())
        kw = {"where": d_bits, "packed": True, "bit_offset": 5} if packed else {"where": d_mask}
        with policy(hip, mu):
            for store in (True, False):
                rows = torch.full((o.size - 1, 32), GARBAGE if store else BIAS, dtype=torch.int64, device="cuda")
                sel = torch.full((o.size - 1,), GARBAGE if store else SEL_BIAS, dtype=torch.int64, device="cuda")
                sfw.count_segments_torch_filter_where(t, d_off, mapq=d_q if min_mapq else None, out=rows, selected=sel, store=store, superset=sup,
                                                      **pred, **kw)
                torch.cuda.synchronize()
                w_rows, w_sel = expect(want_rows, want_sel, (STORE if store else 0) | SUPERSET)   # (want_rows has no superset slots unless sup)
                assert np.array_equal(u64(rows), w_rows), ("device", mu, store)
                assert np.array_equal(u64(sel), w_sel), ("device", mu, store)
            got = sfw.count_segments_device_ptr_filter_where(t.data_ptr(), n, o, d_bits.data_ptr() if packed else d_mask.data_ptr(),
                                                             1 if packed else 8, sel_offset=5 if packed else 0,
                                                             mapq_ptr=d_q.data_ptr() if min_mapq else 0, superset=sup, **pred)
            assert np.array_equal(got[0], want_rows) and np.array_equal(got[1], want_sel), ("sync", mu)
            got = sfw.counters_segments_filter_where(x, o, bits if packed else m, mapq=q if min_mapq else None, packed=packed,
                                                     bit_offset=5 if packed else 0, superset=sup, **pred)
            assert np.array_equal(got[0], want_rows) and np.array_equal(got[1], want_sel), ("host", mu)
    dicts = sfw.flagstats_segments_filter_where(x[:50_000], [0, 10, 30_000, 50_000], m[:50_000], exclude=0x904, mapq=q[:50_000], min_mapq=30)
    w_rows, w_sel = sfwo.want(x[:50_000], [0, 10, 30_000, 50_000], m[:50_000], 0, 0x904, q[:50_000], 30)
    assert [d["n_values"] for d in dicts] == [int(s) for s in w_sel]
    assert int(dicts[1]["passed"]["mapped"]) == int(w_sel[1]) - int(w_rows[1, 2]) - int(w_rows[1, 18])


# ------------------------------------------------------------------ 5. more than 64 segments, windows, malformed offsets, guards
def test_many_segments_windows_and_guard_words(hip, launcher):
    """some 1,400 segments over three units at grid 1 -- one unit per writer, so a writer walks hundreds of segments and reloads its
    window of 64 offsets many times --, empty ones among them; then the same with malformed offsets (a reversed stretch, offsets
    beyond n).  Nothing outside d_out / d_selected is written: the guard words on both sides stay as they were.  Rows are
    checked where the offsets are well-formed or merely run past n (clamped); with reversed offsets the counters are undefined"""
    import torch
    n = 2 * U + 100
    rng = np.random.RandomState(505)
    require, exclude, min_mapq = 0x2, 0x904, 30
    poison = poison_of(require, exclude)
    values = rng.randint(0, 65536, n).astype(np.uint16)
    values[::2] = (values[::2] & np.uint16(0xF6FB)) | np.uint16(0x2)
    mask = rng.randint(0, 4, n) > 0
    mapq = mapq_column(rng, n)
    o = [5]
    lens = (1, 0, 7, 0, 0, 30, 2, 9, 0, 8)
    while o[-1] < n - 9:
        o.append(min(o[-1] + lens[len(o) % len(lens)], n - 9))
    o = np.array(o, dtype=np.int64)
    nseg = o.size - 1
    values[:5], values[n - 9:], mask[:5], mask[n - 9:], mapq[:5], mapq[n - 9:] = poison, poison, True, True, 255, 255
    w = writer_ranges(4, n, 1)
    per_writer = np.bincount(w.pieces(o)["writer"])
    assert nseg > 1000 and per_writer.max() > 5 * 64 and (np.diff(o) == 0).sum() > 100
    past = o.copy()
    past[-40:] += n                                  # monotone, beyond the array: clamped to n, the last 39 segments empty
    past[-1] = 1 << 62
    reversed_ = o.copy()
    reversed_[200:300] = reversed_[200:300][::-1]
    reversed_[-3:] = (n + 50, 3, 1 << 62)
    arrays, sels, mapqs = Arena(np.uint16, poison), Arena(np.uint8, 0xFF, pad=16), Arena(np.uint8, 255, pad=16)
    a_at, q_at = arrays.add(values, 2), mapqs.add(mapq, 1)
    forms = [(sels.add(data, ph), so, sb) for (data, ph, so), sb in ((encode(mask, BITMAP, 3), BITMAP), (encode(mask, BITMAP, 4), BITMAP),
                                                                      (encode(mask, BYTES, 3, value=0xFF), BYTES))]
    arrays.upload(), sels.upload(), mapqs.upload()
    assert arrays.ptr(a_at) % 16 == 4
    G = 64
    words = G + nseg * 32 + G + nseg + G
    want = {"good": sfwo.want(values, o, mask, require, exclude, mapq, min_mapq, superset=True),
            "past": sfwo.want(values, np.clip(past, 0, n), mask, require, exclude, mapq, min_mapq, superset=True)}
    assert want["past"][1][-39:].sum() == 0 and want["past"][1][-40] > want["good"][1][-40]   # the clamped segment takes in the poison tail
    i = 0
    for name, offs in (("good", o), ("past", past), ("reversed", reversed_)):
        d_off = dev64(offs)
        for s_at, sel_offset, sel_bits in forms:
            for mode in MODES:
                for via in ("launcher", "entry"):
                    buf = torch.full((words,), GUARD, dtype=torch.int64, device="cuda")
                    rows, sel = buf[G:G + nseg * 32], buf[2 * G + nseg * 32:2 * G + nseg * 33]
                    rows.fill_(GARBAGE if mode & STORE else BIAS)
                    sel.fill_(GARBAGE if mode & STORE else SEL_BIAS)
                    pred = (require, exclude, min_mapq if i % 3 else 0) if name == "reversed" else (require, exclude, min_mapq)
                    args = (arrays.ptr(a_at), n, d_off.data_ptr(), nseg, pred[0], pred[1], mapqs.ptr(q_at) if pred[2] else None, pred[2],
                            sels.ptr(s_at), sel_offset, sel_bits, rows.data_ptr(), sel.data_ptr(), mode)
                    if via == "entry":
                        assert hip.FLAGSTATS_hip_device_u16_segments_filter_where(*args, None) == 0, err(hip)
                    else:
                        assert launcher(args[0], args[6], args[8], sel_offset, sel_bits, 0, n, args[2], nseg, pred[0], pred[1], pred[2], args[11],
                                        args[12], mode, 1, None) == 0
                    torch.cuda.synchronize()
                    got = u64(buf)
                    for lo, hi in ((0, G), (G + nseg * 32, 2 * G + nseg * 32), (2 * G + nseg * 33, words)):
                        assert (got[lo:hi] == np.uint64(GUARD)).all(), (name, sel_bits, sel_offset, mode, via, lo)
                    if name in want:
                        w_rows, w_sel = expect(want[name][0], want[name][1], mode)
                        assert np.array_equal(got[G:G + nseg * 32].reshape(nseg, 32), w_rows), (name, sel_bits, sel_offset, mode, via)
                        assert np.array_equal(got[2 * G + nseg * 32:2 * G + nseg * 33], w_sel), (name, sel_bits, sel_offset, mode, via)
                    i += 1


# ------------------------------------------------------------------ 6. identities with the parents
def test_identities_with_the_parents(hip, launcher):
    """on one set of poisoned inputs: an all-ones mask is the filtered segmented entry; an empty predicate is the selected
    segmented entry; one segment [0, n) is the filter_where entry; both together are the plain segmented entry (and the clamped
    lengths as counts); the dispatched form (a byte mask without -q) is the kernel forms under the equivalent bitmap, at a byte
    boundary and funnelled; mask bytes of 0x80 and 0xFF select like 1.  Each also against the oracle: the kernels could be wrong
    alike"""
    import torch
    n = 5 * U + 77
    rng = np.random.RandomState(53)
    poison = poison_of(0x2, 0x904)
    values = rng.randint(0, 65536, n).astype(np.uint16)
    values[::2] = (values[::2] & np.uint16(0xF6FB)) | np.uint16(0x2)
    mask = rng.randint(0, 3, n) > 0
    mapq = mapq_column(rng, n)
    o = np.array([5, 5, 300, U + 1, 4 * U, n - 9, n + 1000], dtype=np.int64)       # the last runs past the array
    oc = np.clip(o, 0, n)
    values[:5], mask[:5], mapq[:5] = poison, True, 255
    nseg = o.size - 1
    arrays, sels, mapqs = Arena(np.uint16, poison), Arena(np.uint8, 0xFF, pad=16), Arena(np.uint8, 255, pad=16)
    a = arrays.add(values, 3)
    qa = mapqs.add(mapq, 1)
    s_bits0, s_bits5 = sels.add(pack(mask, 3, fill=1)), sels.add(pack(mask, 0, fill=1))   # array phase 3: bit offset 3 is shift 0, 0 is shift 5
    s_b1, s_b80, s_bff = (sels.add(mask.astype(np.uint8) * np.uint8(val), 1) for val in (1, 0x80, 0xFF))
    s_ones_bits, s_ones = sels.add(np.full((n + 7) // 8 + 1, 0xFF, dtype=np.uint8)), sels.add(np.ones(n, dtype=np.uint8), 3)
    arrays.upload(), sels.upload(), mapqs.upload()
    A, Q = arrays.ptr(a), mapqs.ptr(qa)
    d_off, whole = dev64(o), dev64(np.array([0, n]))
    entry = hip.FLAGSTATS_hip_device_u16_segments_filter_where

    def fresh(words):
        return torch.full((words,), BIAS, dtype=torch.int64, device="cuda")

    def mine(off, k, pred, s, sel_offset, sel_bits, mode):
        r = fresh(k * 33)
        assert entry(A, n, off.data_ptr(), k, pred[0], pred[1], Q if pred[2] else None, pred[2], sels.ptr(s), sel_offset, sel_bits, r.data_ptr(),
                     r.data_ptr() + k * 256, mode, None) == 0, err(hip)
        return r

    def against_oracle(r, k, offs, m, pred, mode):
        w_rows, w_sel = sfwo.want(values, offs, m, pred[0], pred[1], mapq, pred[2], superset=True)
        w = expect(w_rows, w_sel, mode)
        sel_fix = np.uint64(0 if mode & STORE else SEL_BIAS - BIAS)                      # fresh() prefills the counts with BIAS too
        assert np.array_equal(u64(r[:k * 32]).reshape(k, 32), w[0]) and np.array_equal(u64(r[k * 32:]), w[1] - sel_fix), (pred, mode)
        return w_sel

    every = np.ones(n, dtype=bool)
    for mode in MODES:
        # an all-ones mask: the filtered segmented entry
        for pred in ((0x2, 0x904, 30), (0x2, 0x904, 0)):
            f = fresh(nseg * 33)
            assert hip.FLAGSTATS_hip_device_u16_segments_filter(A, n, d_off.data_ptr(), nseg, pred[0], pred[1], Q if pred[2] else None, pred[2],
                                                                f.data_ptr(), f.data_ptr() + nseg * 256, mode, None) == 0, err(hip)
            for s, sb in ((s_ones_bits, BITMAP), (s_ones, BYTES)):
                r = mine(d_off, nseg, pred, s, 0, sb, mode)
                torch.cuda.synchronize()
                assert torch.equal(r, f), ("all-ones mask", pred, sb, mode)
            assert against_oracle(r, nseg, oc, every, pred, mode).any()
        # an empty predicate: the selected segmented entry
        for s, so, sb in ((s_bits0, 3, BITMAP), (s_bits5, 0, BITMAP), (s_b80, 0, BYTES)):
            g = fresh(nseg * 33)
            assert hip.FLAGSTATS_hip_device_u16_segments_where(A, n, d_off.data_ptr(), nseg, sels.ptr(s), so, sb, g.data_ptr(),
                                                               g.data_ptr() + nseg * 256, mode, None) == 0, err(hip)
            r = mine(d_off, nseg, (0, 0, 0), s, so, sb, mode)
            torch.cuda.synchronize()
            assert torch.equal(r, g), ("empty predicate", sb, so, mode)
        against_oracle(r, nseg, oc, mask, (0, 0, 0), mode)
        # one segment [0, n): the filter_where entry
        for pred in ((0x2, 0x904, 30), (0, 0x904, 0)):
            for s, so, sb in ((s_bits0, 3, BITMAP), (s_bits5, 0, BITMAP), (s_bff, 0, BYTES)):
                g = fresh(33)
                assert hip.FLAGSTATS_hip_device_u16_filter_where(A, n, pred[0], pred[1], Q if pred[2] else None, pred[2], sels.ptr(s), so, sb,
                                                                 g.data_ptr(), g.data_ptr() + 256, mode, None) == 0, err(hip)
                r = mine(whole, 1, pred, s, so, sb, mode)
                torch.cuda.synchronize()
                assert torch.equal(r, g) and int(r[32]) not in (0, BIAS), ("one segment", pred, sb, so, mode)
            against_oracle(r, 1, [0, n], mask, pred, mode)
        # both together: the plain segmented entry, and the clamped lengths as counts
        plain = fresh(nseg * 32)
        assert hip.FLAGSTATS_hip_device_u16_segments(A, n, d_off.data_ptr(), nseg, plain.data_ptr(), mode, None) == 0, err(hip)
        lengths = np.diff(oc).astype(np.uint64) + np.uint64(0 if mode & STORE else BIAS)
        for s, sb in ((s_ones_bits, BITMAP), (s_ones, BYTES)):
            r = mine(d_off, nseg, (0, 0, 0), s, 0, sb, mode)
            torch.cuda.synchronize()
            assert torch.equal(r[:nseg * 32], plain) and np.array_equal(u64(r[nseg * 32:]), lengths), ("both", sb, mode)
        # the dispatched form (a byte mask without -q) against the kernel forms under the equivalent bitmap; 0x80 and 0xFF select like 1
        pred = (0x2, 0x904, 0)
        ref = mine(d_off, nseg, pred, s_b1, 0, BYTES, mode)
        for s, so, sb in ((s_bits0, 3, BITMAP), (s_bits5, 0, BITMAP), (s_b80, 0, BYTES), (s_bff, 0, BYTES)):
            r = mine(d_off, nseg, pred, s, so, sb, mode)
            torch.cuda.synchronize()
            assert torch.equal(r, ref), ("dispatched", sb, so, mode)
        assert against_oracle(ref, nseg, oc, mask, pred, mode).any()
        pred = (0x2, 0x904, 30)                                                         # ... and with -q, in the unit's own byte kernel
        ref = mine(d_off, nseg, pred, s_b1, 0, BYTES, mode)
        for s, so, sb in ((s_bits0, 3, BITMAP), (s_bits5, 0, BITMAP), (s_b80, 0, BYTES), (s_bff, 0, BYTES)):
            r = mine(d_off, nseg, pred, s, so, sb, mode)
            torch.cuda.synchronize()
            assert torch.equal(r, ref), ("byte values", sb, so, mode)
        assert against_oracle(ref, nseg, oc, mask, pred, mode).any()
    # nseg == 0 touches nothing, whatever else is NULL
    assert entry(A, n, None, 0, 0x2, 0x904, Q, 30, sels.ptr(s_bits0), 3, BITMAP, None, None, STORE, None) == 0
    assert hip.FLAGSTATS_hip_u16_x64_segments_filter_where(values.ctypes.data, n, None, 0, 0, 0, None, 0, mask.ctypes.data, 0, BYTES, None, None,
                                                           STORE) == 0


# ------------------------------------------------------------------ 7. host form across chunks
def test_host_form_across_chunks(hip):
    """chunks of 8,193 flags from offsets[0] = 3 on: a chunk seam falls inside a segment, inside a selection byte (with bit offset
    6 the seven chunks begin 1, 2, .. 7 bits into one) and, 8,193 being odd, every other chunk's MAPQ slice starts at an odd
    address of the column; flags in front of offsets[0] and behind offsets[nseg] are passing, selected poison that never crosses
    the bus"""
    from libflagstats_amd import _lib
    from libflagstats_amd import segments_filter_where as sfw
    n = 6 * 8193 + 77
    rng = np.random.RandomState(89)
    values = rng.randint(0, 65536, n + 1).astype(np.uint16)[1:]
    values[::2] &= np.uint16(0xF6FB)
    mask = rng.randint(0, 2, n).astype(bool)
    mapq = np.concatenate([[255], mapq_column(rng, n)]).astype(np.uint8)[1:]       # an odd host address
    o = np.array([3, 10, 10, 8193 + 2, 3 * 8193 + 500, 3 * 8193 + 501, 5 * 8193 + 3, n - 20], dtype=np.int64)
    values[:3], values[n - 20:], mask[:3], mask[n - 20:], mapq[:3], mapq[n - 20:] = 0xF6FB, 0xF6FB, True, True, 255, 255
    assert {(6 + 3 + k * 8193) & 7 for k in range(7)} == set(range(1, 8)) and (n - 20 - 3) // 8193 == 6
    byte_mask = np.concatenate([[0xFF], mask.astype(np.uint8) * 0x80]).astype(np.uint8)[1:]      # one byte into its buffer
    encodings = [(pack(mask, 6, fill=1), True, 6), (pack(mask, 0, fill=1), True, 0), (mask, False, 0)]
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", 8193), "chunk_flags")
        for where, packed, bit_offset in encodings:
            for require, exclude, min_mapq in ((0, 0x904, 30), (0x2, 0x904, 0), (0x40, 0x44, 30)):
                for sup in (False, True):
                    want_rows, want_sel = sfwo.want(values, o, mask, require, exclude, mapq, min_mapq, superset=sup)
                    assert bool(want_sel.any()) != bool(require & exclude)
                    got = sfw.counters_segments_filter_where(values, o, where, require=require, exclude=exclude, mapq=mapq if min_mapq else None,
                                                             min_mapq=min_mapq, packed=packed, bit_offset=bit_offset, superset=sup)
                    assert np.array_equal(got[0], want_rows) and np.array_equal(got[1], want_sel), (packed, bit_offset, require, min_mapq, sup)
            want_rows, want_sel = sfwo.want(values, o, mask, 0, 0x904, mapq, 30, superset=True)
            src = where if packed else byte_mask
            o64 = o.astype(np.uint64)
            for flags in (0, SUPERSET):                  # += over bias words
                rows = np.full((o.size - 1, 32), BIAS, dtype=np.uint64)
                sel = np.full(o.size - 1, SEL_BIAS, dtype=np.uint64)
                rc = hip.FLAGSTATS_hip_u16_x64_segments_filter_where(values.ctypes.data, n, o64.ctypes.data, o.size - 1, 0, 0x904, mapq.ctypes.data,
                                                                     30, src.ctypes.data, bit_offset, 1 if packed else 8, rows.ctypes.data,
                                                                     sel.ctypes.data, flags)
                assert rc == 0, err(hip)
                w = expect(want_rows, want_sel, flags)
                assert np.array_equal(rows, w[0]) and np.array_equal(sel, w[1]), (packed, bit_offset, flags)
            # one chunk only (a single staging slot), and segments that cover nothing
            for oo in (np.array([1, 50, 99]), np.array([7, 7, 7]), np.array([n, n])):
                got = sfw.counters_segments_filter_where(values, oo, where, exclude=0x904, mapq=mapq, min_mapq=30, packed=packed, bit_offset=bit_offset)
                want = sfwo.want(values, oo, mask, 0, 0x904, mapq, 30)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), oo
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old
    got = sfw.counters_segments_filter_where(values[:0], [0, 0], mask[:0])
    assert got[0].shape == (1, 32) and not got[0].any() and not got[1].any()
    got = sfw.count_segments_device_ptr_filter_where(0, 0, [0, 0, 0], 0, 1)
    assert got[0].shape == (2, 32) and not got[0].any() and not got[1].any()


# ------------------------------------------------------------------ 8. atomics and streams
def test_three_streams_add_into_one_set_of_rows(hip):
    """three launches on three side streams add into one set of rows and counts (+= form) through the torch layer, which runs on
    torch's current stream; then the store form on a side stream"""
    import torch
    from libflagstats_amd import segments_filter_where as sfw
    rng = np.random.RandomState(73)
    o = np.array([0, 50, 3 * U + 1, 3 * U + 1, 20 * U - 7, 36 * U], dtype=np.int64)
    nseg = o.size - 1
    d_off = dev64(o)
    rows = torch.zeros((nseg, 32), dtype=torch.int64, device="cuda")
    sel = torch.zeros(nseg, dtype=torch.int64, device="cuda")
    total_rows, total_sel = np.zeros((nseg, 32), dtype=np.uint64), np.zeros(nseg, dtype=np.uint64)
    inputs = []
    for n, packed, bit_offset, density, min_mapq in ((36 * U + 11, True, 0, 50, 30), (30 * U + 5, True, 5, 90, 0), (40 * U - 3, False, 0, 10, 30)):
        values = rng.randint(0, 65536, n).astype(np.uint16)
        values[::2] &= np.uint16(0xF6FB)
        mask = rng.randint(0, 100, n) < density
        mapq = mapq_column(rng, n)
        w_rows, w_sel = sfwo.want(values, np.clip(o, 0, n), mask, 0, 0x904, mapq, min_mapq, superset=True)
        assert w_sel.any()
        total_rows += w_rows
        total_sel += w_sel
        where = dev8(pack(mask, bit_offset, fill=1)) if packed else torch.from_numpy(mask).cuda()
        inputs.append((dev16(values), where, packed, bit_offset, dev8(mapq) if min_mapq else None, min_mapq, (w_rows, w_sel)))
    streams = [torch.cuda.Stream() for _ in inputs]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    for st, (t, where, packed, bit_offset, d_q, min_mapq, _) in zip(streams, inputs):
        with torch.cuda.stream(st):
            sfw.count_segments_torch_filter_where(t, d_off, where, exclude=0x904, mapq=d_q, min_mapq=min_mapq, packed=packed, bit_offset=bit_offset,
                                                  out=rows, selected=sel, store=False, superset=True)
    for st in streams:
        st.synchronize()
    assert np.array_equal(u64(rows), total_rows) and np.array_equal(u64(sel), total_sel)
    t, where, packed, bit_offset, d_q, min_mapq, want = inputs[0]
    with torch.cuda.stream(streams[1]):
        r, s = sfw.count_segments_torch_filter_where(t, d_off, where, exclude=0x904, mapq=d_q, min_mapq=min_mapq, packed=packed,
                                                     bit_offset=bit_offset, superset=True)
    streams[1].synchronize()
    assert r.dtype == torch.int64 and tuple(r.shape) == (nseg, 32) and tuple(s.shape) == (nseg,) and r.device == t.device
    assert np.array_equal(u64(r), want[0]) and np.array_equal(u64(s), want[1])


# ------------------------------------------------------------------ 9. refusals
def test_refusals(hip, launcher):
    """every refusal of the C entries and of the launcher, and what the Python layer can refuse only with a device at hand: each
    is an argument check that returns before anything is launched, and rows and counts stay as they were.  Nothing here reads past
    an allocation: the short allocations are refused by the extent check"""
    import torch
    from libflagstats_amd import segments_filter_where as sfw
    n, nseg = 4096, 3
    t = torch.zeros(n + 8, dtype=torch.int16, device="cuda")
    m8 = torch.ones(n + 8, dtype=torch.uint8, device="cuda")
    q8 = torch.full((n + 8,), 60, dtype=torch.uint8, device="cuda")
    o = np.array([0, 10, 2000, n], dtype=np.uint64)
    d_off = dev64(o)
    out = torch.full((nseg, 32), BIAS, dtype=torch.int64, device="cuda")
    sel = torch.full((nseg,), SEL_BIAS, dtype=torch.int64, device="cuda")
    h_out = np.full((nseg, 32), BIAS, dtype=np.uint64)
    h_sel = np.full(nseg, SEL_BIAS, dtype=np.uint64)
    host16 = np.zeros(n + 8, dtype=np.uint16)
    host8 = np.ones(n + 8, dtype=np.uint8)
    hostq = np.full(n + 8, 60, dtype=np.uint8)
    dev_entry = hip.FLAGSTATS_hip_device_u16_segments_filter_where
    sync_entry = hip.FLAGSTATS_hip_device_u16_segments_filter_where_sync
    host_entry = hip.FLAGSTATS_hip_u16_x64_segments_filter_where

    def untouched(what):
        torch.cuda.synchronize()
        assert (out == BIAS).all() and (sel == SEL_BIAS).all(), what
        assert (h_out == BIAS).all() and (h_sel == SEL_BIAS).all(), what

    def refused(what, text, d_array=t.data_ptr(), n_=n, offsets=o, nseg_=nseg, require=0, exclude=0x904, d_mapq=q8.data_ptr(), min_mapq=30,
                d_sel=m8.data_ptr(), sel_offset=0, sel_bits=(1, 8), flags=0, rows=True, forms=("device", "sync", "host")):
        d_o = None if offsets is None else dev64(offsets.astype(np.int64))
        for sb in sel_bits:
            for form in forms:
                if form == "device":
                    rc = dev_entry(d_array, n_, None if d_o is None else d_o.data_ptr(), nseg_, require, exclude, d_mapq, min_mapq, d_sel,
                                   sel_offset, sb, out.data_ptr() if rows else None, sel.data_ptr(), flags, None)
                elif form == "sync":
                    rc = sync_entry(d_array, n_, None if offsets is None else offsets.ctypes.data, nseg_, require, exclude, d_mapq, min_mapq, d_sel,
                                    sel_offset, sb, h_out.ctypes.data if rows else None, h_sel.ctypes.data, flags)
                else:
                    src = host16.ctypes.data + (d_array - t.data_ptr()) if d_array else None
                    rc = host_entry(src, n_, None if offsets is None else offsets.ctypes.data, nseg_, require, exclude,
                                    hostq.ctypes.data if d_mapq else None, min_mapq, host8.ctypes.data if d_sel else None, sel_offset, sb,
                                    h_out.ctypes.data if rows else None, h_sel.ctypes.data, flags)
                assert rc != 0, (what, form, sb)
                assert text in err(hip), (what, form, sb, err(hip))
        untouched(what)

    refused("require", "require must be a 16-bit FLAG mask (at most 0xFFFF)", require=0x10000)
    refused("exclude", "exclude must be a 16-bit FLAG mask (at most 0xFFFF)", exclude=0x10000)
    refused("min_mapq", "min_mapq must be at most 255 (MAPQ is one byte)", min_mapq=256)
    refused("sel_bits", "sel_bits must be 1 (an LSB-first bitmap) or 8 (one byte per element)", sel_bits=(0, 2, 4, 16, -1))
    refused("an extra flag bit", "no other bits", flags=4)
    refused("NULL rows", "with nseg > 0", rows=False)
    refused("NULL offsets", "with nseg > 0", offsets=None)
    refused("NULL array", "NULL array with n > 0", d_array=None)
    refused("NULL mapq", "NULL mapq with min_mapq > 0 and n > 0", d_mapq=None)
    refused("NULL selection", "NULL selection with n > 0", d_sel=None)
    refused("NULL selection, no -q", "NULL selection with n > 0", d_sel=None, d_mapq=None, min_mapq=0)
    refused("an odd array address", "2-byte aligned", d_array=t.data_ptr() + 1)
    refused("n * 2 is no size", "n * 2 is not a size", n_=1 << 63)
    refused("sel_offset + n is no index", "sel_offset + n is not an index", sel_offset=(1 << 64) - 5)
    refused("too many segments", "nseg is too large", nseg_=1 << 60)
    refused("decreasing offsets", "offsets must be non-decreasing", offsets=np.array([0, 20, 10, n], dtype=np.uint64), forms=("sync", "host"))
    refused("offsets past the array", "exceeds the array's", offsets=np.array([0, 10, 20, n + 1], dtype=np.uint64), forms=("sync", "host"))
    # an input somewhere else than the array: in host memory, a CPU tensor (or one of a second device) in Python
    A, F, Q, S = t.data_ptr(), d_off.data_ptr(), q8.data_ptr(), m8.data_ptr()
    rc = dev_entry(A, n, F, nseg, 0, 0x904, Q, 30, host8.ctypes.data, 0, 8, out.data_ptr(), sel.data_ptr(), 0, None)
    assert rc != 0 and "d_sel" in err(hip), err(hip)
    rc = dev_entry(A, n, F, nseg, 0, 0x904, hostq.ctypes.data, 30, S, 0, 8, out.data_ptr(), sel.data_ptr(), 0, None)
    assert rc != 0 and "d_mapq" in err(hip), err(hip)
    rc = sync_entry(A, n, o.ctypes.data, nseg, 0, 0x904, Q, 30, host8.ctypes.data, 0, 1, h_out.ctypes.data, h_sel.ctypes.data, 0)
    assert rc != 0 and "d_sel" in err(hip), err(hip)
    rc = sync_entry(A, n, o.ctypes.data, nseg, 0, 0x904, hostq.ctypes.data, 30, S, 0, 1, h_out.ctypes.data, h_sel.ctypes.data, 0)
    assert rc != 0 and "d_mapq" in err(hip), err(hip)
    tt = t[:n]
    elsewhere = [("cpu", lambda x: x.cpu())]
    if torch.cuda.device_count() > 1:
        elsewhere.append(("cuda:1", lambda x: x.to("cuda:1")))
    for where_name, move in elsewhere:
        others = {"offsets": d_off, "where": m8[:n].bool(), "mapq": q8[:n], "out": torch.zeros((3, 32), dtype=torch.int64, device="cuda"),
                  "selected": torch.zeros(3, dtype=torch.int64, device="cuda")}
        for name in others:
            kw = dict(others)
            kw[name] = move(kw[name])
            with pytest.raises(ValueError, match=r"%s must live on t's device \(cuda:0\), not on %s" % (name, where_name)):
                sfw.count_segments_torch_filter_where(tt, kw.pop("offsets"), kw.pop("where"), exclude=0x904, min_mapq=30, **kw)
    untouched("inputs elsewhere")
    # host pointers as d_out, d_selected, d_offsets
    rc = dev_entry(A, n, F, nseg, 0, 0x904, Q, 30, S, 0, 8, h_out.ctypes.data, sel.data_ptr(), 0, None)
    assert rc != 0 and "d_out" in err(hip), err(hip)
    rc = dev_entry(A, n, F, nseg, 0, 0x904, Q, 30, S, 0, 8, out.data_ptr(), h_sel.ctypes.data, 0, None)
    assert rc != 0 and "d_selected" in err(hip), err(hip)
    rc = dev_entry(A, n, o.ctypes.data, nseg, 0, 0x904, Q, 30, S, 0, 8, out.data_ptr(), sel.data_ptr(), 0, None)
    assert rc != 0 and "d_offsets" in err(hip), err(hip)
    untouched("host pointers")
    # extents: the selection one byte short of the last byte that holds an element's bit or byte (both encodings, also behind a
    # sel_offset), the column one byte short (and not looked at without -q), the array one flag short, rows, counts and offsets
    # 8 bytes short
    nbytes = 2 << 20
    raw = hip.FLAGSTATS_hip_device_alloc(nbytes)
    big = torch.zeros(8 * nbytes + 8, dtype=torch.int16, device="cuda")
    bigq = torch.zeros(8 * nbytes + 8, dtype=torch.uint8, device="cuda")
    assert raw
    try:
        assert hip.FLAGSTATS_hip_memcpy_h2d(raw, np.zeros(nbytes, dtype=np.uint8).ctypes.data, nbytes) == 0
        big_off = dev64(np.array([0, 5, 100, 1000]))
        h_big_off = np.array([0, 5, 100, 1000], dtype=np.uint64)
        for sb, n_, off in ((8, nbytes + 1, 0), (8, nbytes - 6, 7), (1, 8 * nbytes + 1, 0), (1, 8 * nbytes - 2, 3)):
            rc = dev_entry(big.data_ptr(), n_, big_off.data_ptr(), nseg, 0, 0x904, bigq.data_ptr(), 30, raw, off, sb, out.data_ptr(), sel.data_ptr(),
                           STORE, None)
            assert rc != 0 and "d_sel" in err(hip) and "1 bytes short" in err(hip), (sb, n_, off, err(hip))
            rc = sync_entry(big.data_ptr(), n_, h_big_off.ctypes.data, nseg, 0, 0x904, bigq.data_ptr(), 30, raw, off, sb, h_out.ctypes.data,
                            h_sel.ctypes.data, STORE)
            assert rc != 0 and "d_sel" in err(hip) and "1 bytes short" in err(hip), (sb, n_, off, err(hip))
        for sb in (1, 8):
            rc = dev_entry(big.data_ptr(), nbytes + 1, big_off.data_ptr(), nseg, 0, 0x904, raw, 30, bigq.data_ptr(), 0, sb, out.data_ptr(),
                           sel.data_ptr(), STORE, None)
            assert rc != 0 and "d_mapq" in err(hip) and "1 bytes short" in err(hip), (sb, err(hip))
            rc = sync_entry(big.data_ptr(), nbytes + 1, h_big_off.ctypes.data, nseg, 0, 0x904, raw, 30, bigq.data_ptr(), 0, sb, h_out.ctypes.data,
                            h_sel.ctypes.data, STORE)
            assert rc != 0 and "d_mapq" in err(hip) and "1 bytes short" in err(hip), (sb, err(hip))
        rc = dev_entry(raw, nbytes // 2 + 1, big_off.data_ptr(), nseg, 0, 0x904, Q, 0, S, 0, 1, out.data_ptr(), sel.data_ptr(), STORE, None)
        assert rc != 0 and "d_array" in err(hip) and "2 bytes short" in err(hip), err(hip)
        end = raw + nbytes
        for name, kw in (("d_out", {"rows": end - nseg * 256 + 8}), ("d_selected", {"counts": end - nseg * 8 + 8}),
                         ("d_offsets", {"offsets": end - (nseg + 1) * 8 + 8})):
            rc = dev_entry(A, n, kw.get("offsets", F), nseg, 0, 0x904, Q, 30, S, 0, 8, kw.get("rows", out.data_ptr()),
                           kw.get("counts", sel.data_ptr()), 0, None)
            assert rc != 0 and name in err(hip) and "8 bytes short" in err(hip), (name, err(hip))
        back = np.ones(nbytes, dtype=np.uint8)
        assert hip.FLAGSTATS_hip_memcpy_d2h(back.ctypes.data, raw, nbytes) == 0 and not back.any()
    finally:
        hip.FLAGSTATS_hip_device_free(raw)
    untouched("extents")
    # the launcher itself: other mode bits, no workgroups, a wave's uint32 totals, a predicate out of range, other encodings,
    # NULLs -- nothing queued
    words = torch.full((nseg * 33,), BIAS, dtype=torch.int64, device="cuda")
    p, ps = words.data_ptr(), words.data_ptr() + nseg * 256
    for sb in (1, 8):
        for q, mq in ((Q, 30), (None, 0)):
            assert launcher(A, q, S, 0, sb, 0, 8, F, nseg, 0, 0x904, mq, p, ps, 4, 1, None) != 0
            assert launcher(A, q, S, 0, sb, 0, 8, F, nseg, 0, 0x904, mq, p, ps, STORE, 0, None) != 0
            assert launcher(A, q, S, 0, sb, 0, 1 << 35, F, nseg, 0, 0x904, mq, p, ps, STORE, 1, None) != 0       # 2^33 flags per wave
            assert launcher(A, q, S, (1 << 64) - 5, sb, 0, 8, F, nseg, 0, 0x904, mq, p, ps, STORE, 1, None) != 0
            assert launcher(A, q, None, 0, sb, 0, 8, F, nseg, 0, 0x904, mq, p, ps, STORE, 1, None) != 0
            assert launcher(None, q, S, 0, sb, 0, 8, F, nseg, 0, 0x904, mq, p, ps, STORE, 1, None) != 0
            assert launcher(A + 1, q, S, 0, sb, 0, 8, F, nseg, 0, 0x904, mq, p, ps, STORE, 1, None) != 0
            assert launcher(A, q, S, 0, sb, 0, 1 << 63, F, nseg, 0, 0x904, mq, p, ps, STORE, 1, None) != 0       # m * 2 is no size
            assert launcher(A, q, S, 0, sb, 0, 8, None, nseg, 0, 0x904, mq, p, ps, STORE, 1, None) != 0
            assert launcher(A, q, S, 0, sb, 0, 8, F, nseg, 0, 0x904, mq, None, ps, STORE, 1, None) != 0
            assert launcher(A, q, S, 0, sb, 0, 8, F, nseg, 0x10000, 0, mq, p, ps, STORE, 1, None) != 0
            assert launcher(A, q, S, 0, sb, 0, 8, F, nseg, 0, 0x10000, mq, p, ps, STORE, 1, None) != 0
        assert launcher(A, None, S, 0, sb, 0, 8, F, nseg, 0, 0x904, 30, p, ps, STORE, 1, None) != 0              # -q without a column
        assert launcher(A, Q, S, 0, sb, 0, 8, F, nseg, 0, 0x904, 256, p, ps, STORE, 1, None) != 0
    assert launcher(A, Q, S, 0, 2, 0, 8, F, nseg, 0, 0x904, 30, p, ps, STORE, 1, None) != 0
    torch.cuda.synchronize()
    assert (words == BIAS).all()
    # what is no refusal: nseg == 0 does nothing; m == 0 and an overlapping pair launch nothing but the store form zeroes
    assert launcher(None, None, None, 0, 1, 0, 0, None, 0, 0, 0, 0, None, None, STORE, 1, None) == 0
    for m_, pred in ((0, (0, 0x904, 30)), (8, (0x40, 0x44, 30))):
        for sb in (1, 8):
            for mode in (STORE, 0):
                words.fill_(BIAS)
                a_, q_, s_ = (None, None, None) if m_ == 0 else (A, Q, S)
                assert launcher(a_, q_, s_, 0, sb, 0, m_, F, nseg, pred[0], pred[1], pred[2], p, ps, mode, 1, None) == 0
                torch.cuda.synchronize()
                assert (words == (0 if mode else BIAS)).all(), (m_, sb, mode)


# ------------------------------------------------------------------ 10. a seeded randomised sweep
SWEEP_PREDICATES = ((0, 0, 0), (0, 0x904, 0), (0, 0x904, 30), (0x2, 0x904, 30), (0x0101, 0x8080, 128), (0x1, 0, 1), (0x40, 0x44, 7), (0x0400, 0x0004, 255))


@pytest.mark.parametrize("seed", [20271, 20272])
def test_seeded_randomised_sweep(hip, launcher, seed):
    """100 cases per seed: n up to 6 units, random array phase, offsets (gaps in front and behind, empty segments), encoding, bit
    offset or byte alignment, byte values, density, MAPQ alignment, predicate and threshold, mode, grid, presence of `selected`,
    and the chain threshold (0, 1 or 2, applied to a third of the cases each); launched into one batch and read back once"""
    rng = np.random.RandomState(seed)
    arenas = [Arena(np.uint16, poison_of(r, e)) for r, e, _ in SWEEP_PREDICATES]
    sels, mapqs, offs = Arena(np.uint8, 0xFF, pad=16), Arena(np.uint8, 255, pad=16), Arena(np.int64, 0, pad=0)
    batch, calls = Batch(), []
    for i in range(100):
        n = int(rng.choice([rng.randint(1, 64), rng.randint(64, U + 64), rng.randint(U, 3 * U + 1), rng.randint(3 * U, 6 * U + 1)]))
        phase = int(rng.randint(0, 8))
        pi = int(rng.randint(0, len(SWEEP_PREDICATES)))
        require, exclude, min_mapq = SWEEP_PREDICATES[pi]
        values = rng.randint(0, 65536, n).astype(np.uint16)
        keep = rng.randint(0, 2, n).astype(bool)              # half of the values made to pass the FLAG test
        values[keep] = (values[keep] & np.uint16(0xFFFF & ~exclude)) | np.uint16(require)
        density = int(rng.choice([0, 1, 10, 50, 90, 99, 100]))
        mask = rng.randint(0, 100, n) < density
        mapq = mapq_column(rng, n)
        if min_mapq:
            mapq[rng.randint(0, 3, n) == 0] = np.uint8(rng.choice([min_mapq - 1, min_mapq, min(min_mapq + 1, 255)]))
        nseg = int(rng.randint(1, 12))
        cuts = np.sort(rng.randint(0, n + 1, nseg + 1))
        if rng.randint(0, 3) == 0:
            cuts[rng.randint(0, nseg + 1)] = cuts[rng.randint(0, nseg + 1)]           # an empty segment (sorted again below)
        o = np.sort(cuts).astype(np.int64)
        values[:o[0]], values[o[-1]:] = poison_of(require, exclude), poison_of(require, exclude)
        mask[:o[0]], mask[o[-1]:] = True, True
        mapq[:o[0]], mapq[o[-1]:] = 255, 255
        sel_bits = BITMAP if rng.randint(0, 3) else BYTES
        where = int(rng.randint(0, 8) if sel_bits == BITMAP else rng.randint(0, 16))
        data, sel_phase, sel_offset = encode(mask, sel_bits, where, value=int(rng.randint(1, 256)))
        want_rows, want_sel = sfwo.want(values, o, mask, require, exclude, mapq, min_mapq, superset=True)
        mode = int(rng.randint(0, 4))
        k = batch.add(mode, want_rows, want_sel, (seed, i, n, phase, o.tolist(), sel_bits, where, density, SWEEP_PREDICATES[pi]),
                      with_selected=bool(rng.randint(0, 4)))
        calls.append((k, pi, arenas[pi].add(values, phase), n, mapqs.add(mapq, int(rng.randint(0, 16))), sels.add(data, sel_phase), sel_offset, sel_bits,
                      offs.add(o), nseg, int(rng.randint(1, 4)), i % 3))
    for a in arenas:
        a.upload()
    sels.upload(), mapqs.upload(), offs.upload()
    batch.upload()
    for mu in (0, 1, 2):
        with policy(hip, mu):
            for k, pi, a_at, n, q_at, s_at, sel_offset, sel_bits, o_at, nseg, grid, which in calls:
                if which != mu:
                    continue
                launch(launcher, arenas[pi].ptr(a_at), mapqs.ptr(q_at), sels.ptr(s_at), sel_offset, sel_bits, n, offs.ptr(o_at), nseg,
                       SWEEP_PREDICATES[pi], batch, k, grid)
    batch.check()
