"""The selected-elements flagstat on the MI355X: fsk::flagstat_count_where under an LSB-first bitmap and under a byte mask, the
three C entries and libflagstats_amd/where.py.

Expected counters never come from the code under test: where_oracle.want_counters is oracle.flagstat_c of values[mask] (superset
slots from oracle.samtools_counts and the definition); the expected `selected` is int(mask.sum())."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from where_oracle import BITMAP, BYTES, pack, want_counters  # noqa: E402

pytestmark = pytest.mark.gpu

STORE, SUPERSET = 1, 2
GARBAGE, BIAS, SEL_BIAS = 0x5EED_0000_0BAD, 3, 1 << 40
S = 16384                                     # flags of one 32 KiB step
ENCODINGS = (BITMAP, BYTES)


def dev16(v):
    """a uint16 numpy array as an int16 CUDA tensor"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint16).view(np.int16)).cuda()


def dev8(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint8)).cuda()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def err(hip):
    return hip.FLAGSTATS_hip_last_error().decode(errors="replace")


def expect_row(want, mode):
    """what a row must read after a launch in `mode`: the superset counters `want` cut to the form, over BIAS in the += form"""
    w = want.copy()
    if not mode & SUPERSET:
        w[[0, 9, 16]] = 0
    return w if mode & STORE else w + np.uint64(BIAS)


def expect_selected(sel, mode):
    return sel if mode & STORE else sel + SEL_BIAS


class Rows:
    """device words for many launches, one row of 33 per launch (32 counters, then `selected`): filled with GARBAGE (store form)
    or BIAS / SEL_BIAS (+= form) in one copy, read back in one copy after every launch has been queued"""

    def __init__(self):
        self.modes, self.wants, self.notes = [], [], []

    def add(self, mode, want, selected, note):
        self.modes.append(mode)
        self.wants.append(np.concatenate([expect_row(want, mode), [np.uint64(expect_selected(selected, mode))]]).astype(np.uint64))
        self.notes.append(note)
        return len(self.modes) - 1

    def upload(self):
        import torch
        fill = np.empty((len(self.modes), 33), dtype=np.uint64)
        for k, mode in enumerate(self.modes):
            fill[k, :32] = GARBAGE if mode & STORE else BIAS
            fill[k, 32] = GARBAGE if mode & STORE else SEL_BIAS
        self.t = torch.from_numpy(fill.view(np.int64)).cuda()
        torch.cuda.synchronize()

    def out(self, k):
        return self.t.data_ptr() + 33 * 8 * k

    def selected(self, k):
        return self.out(k) + 32 * 8

    def check(self):
        import torch
        torch.cuda.synchronize()
        got = u64(self.t)
        for k, want in enumerate(self.wants):
            assert np.array_equal(got[k], want), (self.notes[k], got[k], want)


# ------------------------------------------------------------------ 1. every value
@pytest.mark.parametrize("sel_bits", ENCODINGS)
def test_every_value_through_every_form(hip, oracle_mod, sel_bits):
    """0..65535 once each among 65,536 poison flags of 0xFFFF; the mask selects the real ones -- device form (torch's stream),
    _sync form, host form"""
    import torch
    from libflagstats_amd import where
    rng = np.random.RandomState(2024)
    order = rng.permutation(131072)
    values = np.full(131072, 0xFFFF, dtype=np.uint16)
    mask = np.zeros(131072, dtype=bool)
    values[order[:65536]] = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    mask[order[:65536]] = True
    want = oracle_mod.flagstat_c(np.arange(65536, dtype=np.uint32).astype(np.uint16)).astype(np.uint64)
    packed = sel_bits == BITMAP
    sel = pack(mask) if packed else mask
    got, selected = where.counters_where(values, sel, packed=packed)                             # host form
    assert np.array_equal(got, want) and selected == 65536 and got.dtype == np.uint64, "host"
    d = where.flagstats_where(values, sel, packed=packed)
    assert d["n_values"] == 65536 and int(d["failed"]["FQCFAIL"]) == int(want[25])
    assert int(d["passed"]["mapped"]) == 65536 - int(want[2]) - int(want[18])
    t = dev16(values)
    m = dev8(sel) if packed else torch.from_numpy(mask).cuda()
    got, selected = where.count_device_ptr_where(t.data_ptr(), t.numel(), m.data_ptr(), sel_bits)   # _sync form
    assert np.array_equal(got, want) and selected == 65536, "sync"
    o, s = where.count_torch_where(t, m, packed=packed, store=True)                              # device form
    torch.cuda.synchronize()
    assert o.dtype == torch.int64 and tuple(o.shape) == (32,) and tuple(s.shape) == (1,) and o.device == t.device
    assert np.array_equal(u64(o), want) and int(u64(s)[0]) == 65536, "device"
    o2, s2 = where.count_torch_where(t, m, out=o, selected=s, packed=packed)                     # a second call adds
    torch.cuda.synchronize()
    assert o2 is o and s2 is s and np.array_equal(u64(o), 2 * want) and int(u64(s)[0]) == 2 * 65536
    # nothing to count: += touches nothing, store writes zeros
    where.count_torch_where(t[:0], m[:0], out=o, selected=s, packed=packed)
    torch.cuda.synchronize()
    assert np.array_equal(u64(o), 2 * want) and int(u64(s)[0]) == 2 * 65536
    where.count_torch_where(t[:0], m[:0], out=o, selected=s, packed=packed, store=True)
    torch.cuda.synchronize()
    assert not o.any() and not s.any()
    got, selected = where.counters_where(values[:0], sel[:0], packed=packed)
    assert not got.any() and selected == 0
    got, selected = where.count_device_ptr_where(0, 0, 0, sel_bits)
    assert not got.any() and selected == 0


# ------------------------------------------------------------------ 2. lengths, phases, offsets
LENGTHS = (0, 1, 2, 7, 8, 9, 63, 64, 65, S - 1, S, S + 1, 2 * S - 1, 2 * S + 1)
BYTE_ALIGNMENTS = (0, 1, 3, 8, 15)


def test_lengths_phases_offsets(hip, oracle_mod):
    """every length around nothing, a vector, a wave's line and one and two steps x every array phase x every bit offset
    (bitmap) / selection alignments 0, 1, 3, 8, 15 (bytes).  The array sits in a slab whose surrounding 64 flags are 0xFFFF, the
    selection in a slab whose surrounding bytes -- and the unused bits of its first and last byte -- are all ones: one element or
    bit read outside [0, n) lights every fail-QC counter.  Through fsk_launch_where at grids 1, 2, 3 and the public device entry,
    store form over garbage and += over bias words."""
    import torch
    rng = np.random.RandomState(41)
    body = rng.randint(0, 65536, LENGTHS[-1]).astype(np.uint16)
    mask = rng.randint(0, 2, LENGTHS[-1]).astype(bool)
    wants = {n: want_counters(oracle_mod, body[:n], mask[:n], superset=True) for n in LENGTHS}
    # every (n, phase) array and every (n, offset) selection, laid out in two host buffers and uploaded once
    arrays, a_at = [], {}
    pos = 0
    for n in LENGTHS:
        for phase in range(8):
            region = np.full((64 + 8 + n + 64 + 7) // 8 * 8, 0xFFFF, dtype=np.uint16)
            region[64 + phase:64 + phase + n] = body[:n]
            a_at[n, phase] = pos + 64 + phase
            arrays.append(region)
            pos += region.size
    sels, s_at = [], {}
    pos = 0
    for n in LENGTHS:
        for sel_bits, offsets in ((BITMAP, range(8)), (BYTES, BYTE_ALIGNMENTS)):
            for off in offsets:
                if sel_bits == BITMAP:
                    payload = pack(mask[:n], off, fill=1) if n else np.zeros(0, dtype=np.uint8)
                    align = (5 * off + n) % 16            # the bitmap's own first byte at varying alignments as well
                else:
                    payload = np.where(mask[:n], 1, 0).astype(np.uint8)
                    align = off
                region = np.full((16 + 16 + payload.size + 16 + 15) // 16 * 16, 0xFF, dtype=np.uint8)
                region[16 + align:16 + align + payload.size] = payload
                s_at[n, sel_bits, off] = pos + 16 + align
                sels.append(region)
                pos += region.size
    d_arrays = dev16(np.concatenate(arrays))
    d_sels = dev8(np.concatenate(sels))
    assert d_arrays.data_ptr() % 16 == 0 and d_sels.data_ptr() % 16 == 0
    rows = Rows()
    calls = []
    for n in LENGTHS:
        sel_n = int(mask[:n].sum())
        for phase in range(8):
            ptr = d_arrays.data_ptr() + 2 * a_at[n, phase]
            assert ptr % 16 == 2 * phase
            for sel_bits, offsets in ((BITMAP, range(8)), (BYTES, BYTE_ALIGNMENTS)):
                for off in offsets:
                    sptr = d_sels.data_ptr() + s_at[n, sel_bits, off]
                    sel_offset = off if sel_bits == BITMAP else 0
                    if sel_bits == BYTES:
                        assert sptr % 16 == off
                    for grid in (1, 2, 3, None):          # None: the public device entry
                        for mode in (STORE | SUPERSET, 0):
                            k = rows.add(mode, wants[n], sel_n, (n, phase, sel_bits, off, grid, mode))
                            calls.append((k, ptr, n, sptr, sel_offset, sel_bits, mode, grid))
    rows.upload()
    for k, ptr, n, sptr, sel_offset, sel_bits, mode, grid in calls:
        if grid is None:
            rc = hip.FLAGSTATS_hip_device_u16_where(ptr if n else None, n, sptr if n else None, sel_offset, sel_bits, rows.out(k),
                                                    rows.selected(k), mode, None)
            assert rc == 0, (rows.notes[k], err(hip))
        else:
            rc = hip.fsk_launch_where(ptr if n else None, n, sptr if n else None, sel_offset, sel_bits, rows.out(k), rows.selected(k),
                                      mode, grid, None)
            assert rc == 0, (rows.notes[k], rc)
    rows.check()


# ------------------------------------------------------------------ 3. which bit belongs to which flag
POSITIONS = tuple(range(18)) + (511, 512, 513, 4095, 4096, 4097, S - 1, S, S + 1, 2 * S - 1)


@pytest.mark.parametrize("sel_bits", ENCODINGS)
@pytest.mark.parametrize("phase,offset", [(0, 0), (5, 3)])
def test_which_bit_belongs_to_which_flag(hip, oracle_mod, sel_bits, phase, offset):
    """n = 2 S flags of 0xFFFF; array[p] = 0x0041 between two 0x0081.  Selecting p alone gives the row of one 0x0041; selecting
    everything but p gives the row of the array without it"""
    import torch
    n = 2 * S
    one = oracle_mod.flagstat_c(np.array([0x0041], dtype=np.uint16)).astype(np.uint64)
    pa = oracle_mod.samtools_counts(np.array([0x0041], dtype=np.uint16))["n_pair_all"]
    one[0], one[16], one[9] = pa[0], pa[1], 1 - int(one[25])
    slab = torch.full((64 + 8 + n + 64,), -1, dtype=torch.int16, device="cuda")
    arr = slab[64 + phase:64 + phase + n]
    assert arr.data_ptr() % 16 == 2 * phase
    nsel = (offset + n + 7) // 8 if sel_bits == BITMAP else n
    sel = torch.zeros(16 + nsel + 16, dtype=torch.uint8, device="cuda")
    sel_ptr = sel.data_ptr() + 16 + (offset if sel_bits == BYTES else 0)
    body = sel[16:16 + nsel] if sel_bits == BITMAP else sel[16 + offset:16 + offset + n]
    sel_offset = offset if sel_bits == BITMAP else 0
    host = np.full(n, 0xFFFF, dtype=np.uint16)
    rows = Rows()
    plan = []
    for p in POSITIONS:
        v = host.copy()
        v[p] = 0x0041
        v[max(p - 1, 0):p] = 0x0081
        v[p + 1:p + 2] = 0x0081
        hot = np.zeros(n, dtype=bool)
        hot[p] = True
        plan.append((p, rows.add(STORE | SUPERSET, one, 1, ("alone", sel_bits, phase, offset, p)),
                     rows.add(STORE | SUPERSET, want_counters(oracle_mod, v, ~hot, superset=True), n - 1, ("all but", sel_bits, phase, offset, p))))
    rows.upload()
    for p, k_alone, k_rest in plan:
        arr[p] = 0x0041
        if p > 0:
            arr[p - 1] = 0x0081
        if p + 1 < n:
            arr[p + 1] = 0x0081
        for k, background in ((k_alone, 0), (k_rest, 0xFF)):
            sel.fill_(background)
            if sel_bits == BITMAP:
                bit = 1 << ((offset + p) & 7)
                body[(offset + p) >> 3] = bit if background == 0 else 0xFF ^ bit
            else:
                body[p] = 1 if background == 0 else 0
            rc = hip.fsk_launch_where(arr.data_ptr(), n, sel_ptr, sel_offset, sel_bits, rows.out(k), rows.selected(k), STORE | SUPERSET, 3, None)
            assert rc == 0, rc
        arr[max(p - 1, 0):p + 2] = -1
    rows.check()


# ------------------------------------------------------------------ 4. densities
@pytest.mark.parametrize("sel_bits", ENCODINGS)
def test_densities(hip, oracle_mod, sel_bits):
    """mask densities 0, 1/64, 1/2, 63/64 and 1 over 3 S + 5 flags, superset on and off; density 1 is the plain count of the
    array, density 0 is nothing"""
    import torch
    n = 3 * S + 5
    rng = np.random.RandomState(17)
    values = rng.randint(0, 65536, n).astype(np.uint16)
    t = dev16(values)
    plain = np.zeros(32, dtype=np.uint64)
    assert hip.FLAGSTATS_hip_device_u16_sync(t.data_ptr(), n, plain.ctypes.data) == 0, err(hip)
    draw = rng.randint(0, 64, n)
    for name, mask in (("0", draw < 0), ("1/64", draw < 1), ("1/2", draw < 32), ("63/64", draw < 63), ("1", draw < 64)):
        m = dev8(pack(mask) if sel_bits == BITMAP else mask.astype(np.uint8))
        for sup in (0, SUPERSET):
            want = want_counters(oracle_mod, values, mask, superset=bool(sup))
            out = torch.full((32,), GARBAGE, dtype=torch.int64, device="cuda")
            sel = torch.full((1,), GARBAGE, dtype=torch.int64, device="cuda")
            rc = hip.FLAGSTATS_hip_device_u16_where(t.data_ptr(), n, m.data_ptr(), 0, sel_bits, out.data_ptr(), sel.data_ptr(), STORE | sup, None)
            assert rc == 0, err(hip)
            torch.cuda.synchronize()
            assert np.array_equal(u64(out), want), (sel_bits, name, sup, u64(out), want)
            assert int(u64(sel)[0]) == int(mask.sum()), (sel_bits, name, sup)
            if name == "1" and not sup:
                assert np.array_equal(u64(out), plain)
            if name == "0":
                assert not u64(out).any() and int(u64(sel)[0]) == 0
            # += over bias words, no `selected` asked for; then the _sync form
            out.fill_(BIAS)
            rc = hip.FLAGSTATS_hip_device_u16_where(t.data_ptr(), n, m.data_ptr(), 0, sel_bits, out.data_ptr(), None, sup, None)
            assert rc == 0, err(hip)
            torch.cuda.synchronize()
            assert np.array_equal(u64(out), want + np.uint64(BIAS)), (sel_bits, name, sup)
            o = np.full(32, BIAS, dtype=np.uint64)
            h = ctypes.c_uint64(SEL_BIAS)
            assert hip.FLAGSTATS_hip_device_u16_where_sync(t.data_ptr(), n, m.data_ptr(), 0, sel_bits, o.ctypes.data, ctypes.byref(h), sup) == 0
            assert np.array_equal(o, want + np.uint64(BIAS)) and h.value == SEL_BIAS + int(mask.sum()), (sel_bits, name, sup)


# ------------------------------------------------------------------ 5. byte values
def test_byte_values(hip, oracle_mod):
    """selection bytes 0x02, 0x80 and 0xFF (and 0x01, 0x40, 0x7F) select; only 0x00 does not"""
    import torch
    n = S + 100
    rng = np.random.RandomState(23)
    values = rng.randint(0, 65536, n).astype(np.uint16)
    sel = np.array([0x00, 0x02, 0x80, 0xFF, 0x00, 0x01, 0x40, 0x7F], dtype=np.uint8)[rng.randint(0, 8, n)]
    mask = sel != 0
    assert {0x00, 0x02, 0x80, 0xFF} <= set(sel.tolist()) and 0 < mask.sum() < n
    want = want_counters(oracle_mod, values, mask, superset=True)
    slab = torch.full((8 + n,), -1, dtype=torch.int16, device="cuda")
    slab[1:1 + n] = dev16(values)                 # one flag into a 16-byte line: a head edge step, a fast step, a tail edge step
    m = dev8(sel)
    out = torch.full((33,), GARBAGE, dtype=torch.int64, device="cuda")
    rc = hip.FLAGSTATS_hip_device_u16_where(slab.data_ptr() + 2, n, m.data_ptr(), 0, BYTES, out.data_ptr(), out.data_ptr() + 256,
                                            STORE | SUPERSET, None)
    assert rc == 0, err(hip)
    torch.cuda.synchronize()
    assert np.array_equal(u64(out)[:32], want) and int(u64(out)[32]) == int(mask.sum())
    for single in (0x02, 0x80, 0xFF):
        m.fill_(single)
        rc = hip.FLAGSTATS_hip_device_u16_where(slab.data_ptr() + 2, n, m.data_ptr(), 0, BYTES, out.data_ptr(), out.data_ptr() + 256,
                                                STORE | SUPERSET, None)
        assert rc == 0, err(hip)
        torch.cuda.synchronize()
        assert np.array_equal(u64(out)[:32], want_counters(oracle_mod, values, np.ones(n, dtype=bool), superset=True)), hex(single)
        assert int(u64(out)[32]) == n


# ------------------------------------------------------------------ 6. epochs
@pytest.mark.parametrize("sel_bits", ENCODINGS)
def test_epochs(hip, oracle_mod, sel_bits):
    """one workgroup over 258 S + 3 flags: 258 fast steps and a tail edge step, so every wave passes its staggered first flush
    (after 255, 191, 127 and 63 pushes) and wave 0 a full epoch of 255 steps"""
    import torch
    n = 258 * S + 3
    pattern = np.random.RandomState(303).randint(0, 65536, 65_521).astype(np.uint16)
    values = np.resize(pattern, n)
    mask = np.random.RandomState(304).randint(0, 3, n) != 0
    want = want_counters(oracle_mod, values, mask, superset=True)
    t = dev16(values)
    m = dev8(pack(mask, 5) if sel_bits == BITMAP else mask.astype(np.uint8))
    assert t.data_ptr() % 16 == 0
    rows = Rows()
    ks = [rows.add(mode, want, int(mask.sum()), (sel_bits, mode)) for mode in (STORE | SUPERSET, 0)]
    rows.upload()
    for k in ks:
        rc = hip.fsk_launch_where(t.data_ptr(), n, m.data_ptr(), 5 if sel_bits == BITMAP else 0, sel_bits, rows.out(k), rows.selected(k),
                                  rows.modes[k], 1, None)
        assert rc == 0, rc
    rows.check()


# ------------------------------------------------------------------ 7. atomics
def test_three_streams_add_into_one_pair(hip, oracle_mod):
    import torch
    from libflagstats_amd import where
    rng = np.random.RandomState(71)
    out = torch.zeros(32, dtype=torch.int64, device="cuda")
    selected = torch.zeros(1, dtype=torch.int64, device="cuda")
    total, total_sel = np.zeros(32, dtype=np.uint64), 0
    inputs = []
    for i, (n, packed) in enumerate(((40 * S + 11, True), (37 * S + 5, False), (43 * S - 3, True))):
        values = rng.randint(0, 65536, n).astype(np.uint16)
        mask = rng.randint(0, 2, n).astype(bool)
        total += want_counters(oracle_mod, values, mask, superset=True)
        total_sel += int(mask.sum())
        sel = dev8(pack(mask, i)) if packed else torch.from_numpy(mask).cuda()
        inputs.append((dev16(values), sel, packed, i if packed else 0))
    streams = [torch.cuda.Stream() for _ in inputs]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    for st, (t, sel, packed, off) in zip(streams, inputs):
        with torch.cuda.stream(st):
            where.count_torch_where(t, sel, out=out, selected=selected, superset=True, packed=packed, bit_offset=off)
    for st in streams:
        st.synchronize()
    assert np.array_equal(u64(out), total) and int(u64(selected)[0]) == total_sel


# ------------------------------------------------------------------ 8. host form across chunks
def test_host_form_across_chunks(hip, oracle_mod):
    """chunks of 8,192 flags, five of them and a ragged tail; bitmap bit offsets 0, 3 and 7 so that chunks start in mid-byte"""
    from libflagstats_amd import _lib, where
    n = 5 * 8192 + 77
    rng = np.random.RandomState(88)
    values = rng.randint(0, 65536, n).astype(np.uint16)
    mask = rng.randint(0, 2, n).astype(bool)
    nsel = int(mask.sum())
    wants = {sup: want_counters(oracle_mod, values, mask, superset=bool(sup)) for sup in (0, SUPERSET)}
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", 8192), "chunk_flags")
        cases = [(BITMAP, off, pack(mask, off, fill=1)) for off in (0, 3, 7)] + [(BYTES, 0, mask.astype(np.uint8))]
        for sel_bits, off, sel in cases:
            got, selected = where.counters_where(values, sel if sel_bits == BITMAP else mask, packed=sel_bits == BITMAP, bit_offset=off)
            assert np.array_equal(got, wants[0]) and selected == nsel, (sel_bits, off)
            got, selected = where.counters_where(values, sel if sel_bits == BITMAP else mask, packed=sel_bits == BITMAP, bit_offset=off,
                                                 superset=True)
            assert np.array_equal(got, wants[SUPERSET]) and selected == nsel, (sel_bits, off, "superset")
            for flags in (0, SUPERSET):                  # += over bias words
                o = np.full(32, BIAS, dtype=np.uint64)
                h = ctypes.c_uint64(SEL_BIAS)
                rc = hip.FLAGSTATS_hip_u16_x64_where(values.ctypes.data, n, sel.ctypes.data, off, sel_bits, o.ctypes.data, ctypes.byref(h), flags)
                assert rc == 0, err(hip)
                assert np.array_equal(o, expect_row(wants[SUPERSET], flags)) and h.value == SEL_BIAS + nsel, (sel_bits, off, flags)
            # one chunk only (a single staging slot), from an odd host address
            if sel_bits == BITMAP:
                got, selected = where.counters_where(values[1:100], pack(mask[1:100], off), packed=True, bit_offset=off)
            else:
                got, selected = where.counters_where(values[1:100], mask[1:100])
            assert np.array_equal(got, want_counters(oracle_mod, values[1:100], mask[1:100])) and selected == int(mask[1:100].sum())
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old
    # n == 0: += touches nothing, store writes zeros; the selection may be NULL
    for entry in (hip.FLAGSTATS_hip_u16_x64_where, hip.FLAGSTATS_hip_device_u16_where_sync):
        for sel_bits in ENCODINGS:
            o = np.full(32, BIAS, dtype=np.uint64)
            h = ctypes.c_uint64(5)
            assert entry(None, 0, None, 3, sel_bits, o.ctypes.data, ctypes.byref(h), 0) == 0 and (o == BIAS).all() and h.value == 5
            assert entry(None, 0, None, 3, sel_bits, o.ctypes.data, ctypes.byref(h), STORE) == 0 and not o.any() and h.value == 0


# ------------------------------------------------------------------ 9. refusals that need a device
def test_device_dependent_refusals(hip):
    """what the C entries and the Python layer can refuse only with a device at hand.  The branch with the selection on ANOTHER
    device (the C texts "d_sel and d_out / d_array live on different devices", Python's "not on cuda:1") runs only where
    torch sees two devices: on a one-GPU machine it is not exercised, and a selection in host memory and a CPU tensor stand in
    for it."""
    import torch
    from libflagstats_amd import where
    n = 4096
    t = torch.zeros(n + 8, dtype=torch.int16, device="cuda")
    m = torch.ones(n + 8, dtype=torch.uint8, device="cuda")
    out = torch.full((32,), BIAS, dtype=torch.int64, device="cuda")
    sel = torch.full((1,), SEL_BIAS, dtype=torch.int64, device="cuda")
    h_out = np.full(32, BIAS, dtype=np.uint64)
    h_sel = ctypes.c_uint64(SEL_BIAS)
    host16 = np.zeros(n + 8, dtype=np.uint16)
    host8 = np.ones(n + 8, dtype=np.uint8)

    def untouched(what):
        torch.cuda.synchronize()
        assert (out == BIAS).all() and int(u64(sel)[0]) == SEL_BIAS, what
        assert (h_out == BIAS).all() and h_sel.value == SEL_BIAS, what

    def refused(what, text, d_array=t.data_ptr(), n_=n, d_sel=m.data_ptr(), off=0, bits=BYTES, flags=0):
        for form in ("device", "sync", "host"):
            if form == "device":
                rc = hip.FLAGSTATS_hip_device_u16_where(d_array, n_, d_sel, off, bits, out.data_ptr(), sel.data_ptr(), flags, None)
            elif form == "sync":
                rc = hip.FLAGSTATS_hip_device_u16_where_sync(d_array, n_, d_sel, off, bits, h_out.ctypes.data, ctypes.byref(h_sel), flags)
            else:
                src = host16.ctypes.data + (d_array - t.data_ptr()) if d_array else None
                rc = hip.FLAGSTATS_hip_u16_x64_where(src, n_, host8.ctypes.data if d_sel else None, off, bits, h_out.ctypes.data,
                                                     ctypes.byref(h_sel), flags)
            assert rc != 0, (what, form)
            assert text in err(hip), (what, form, err(hip))
        untouched(what)

    for bits in (0, 2, 4, 16):
        refused("sel_bits %d" % bits, "sel_bits must be 1", bits=bits)
    refused("an odd array address", "2-byte aligned", d_array=t.data_ptr() + 1)
    refused("an extra flag bit", "no other bits", flags=4)
    refused("NULL array", "NULL array with n > 0", d_array=None)
    refused("NULL selection", "NULL selection with n > 0", d_sel=None)
    refused("an offset that wraps", "sel_offset + n is not an index", off=(1 << 64) - 8)
    # the selection somewhere else than the array: in host memory, on another device (where there is one), a CPU tensor in Python
    for bits in ENCODINGS:
        rc = hip.FLAGSTATS_hip_device_u16_where(t.data_ptr(), n, host8.ctypes.data, 0, bits, out.data_ptr(), sel.data_ptr(), 0, None)
        assert rc != 0 and "d_sel" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_u16_where_sync(t.data_ptr(), n, host8.ctypes.data, 0, bits, h_out.ctypes.data, ctypes.byref(h_sel), 0)
        assert rc != 0 and "d_sel" in err(hip), err(hip)
    if torch.cuda.device_count() > 1:
        far = torch.ones(n + 8, dtype=torch.uint8, device="cuda:1")
        rc = hip.FLAGSTATS_hip_device_u16_where(t.data_ptr(), n, far.data_ptr(), 0, BYTES, out.data_ptr(), sel.data_ptr(), 0, None)
        assert rc != 0 and "d_sel and d_out live on different devices" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_u16_where_sync(t.data_ptr(), n, far.data_ptr(), 0, BYTES, h_out.ctypes.data, ctypes.byref(h_sel), 0)
        assert rc != 0 and "d_sel and d_array live on different devices" in err(hip), err(hip)
        with pytest.raises(ValueError, match=r"where must live on t's device \(cuda:0\), not on cuda:1"):
            where.count_torch_where(t, far, packed=True)
    with pytest.raises(ValueError, match=r"where must live on t's device \(cuda:0\), not on cpu"):
        where.count_torch_where(t, torch.ones(n + 8, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"out must live on t's device \(cuda:0\), not on cpu"):
        where.count_torch_where(t, m, packed=True, out=torch.zeros(32, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"selected must live on t's device \(cuda:0\), not on cpu"):
        where.count_torch_where(t, m, packed=True, selected=torch.zeros(1, dtype=torch.int64))
    untouched("selection elsewhere")
    # a host pointer as d_out (pageable, then page-locked) or as d_selected
    rc = hip.FLAGSTATS_hip_device_u16_where(t.data_ptr(), n, m.data_ptr(), 0, BYTES, h_out.ctypes.data, sel.data_ptr(), 0, None)
    assert rc != 0 and "d_out" in err(hip), err(hip)
    rc = hip.FLAGSTATS_hip_device_u16_where(t.data_ptr(), n, m.data_ptr(), 0, BYTES, out.data_ptr(), ctypes.addressof(h_sel), 0, None)
    assert rc != 0 and "d_selected" in err(hip), err(hip)
    pinned = hip.FLAGSTATS_hip_host_alloc(512)
    assert pinned
    try:
        ctypes.memset(pinned, 0, 512)
        rc = hip.FLAGSTATS_hip_device_u16_where(t.data_ptr(), n, m.data_ptr(), 0, BYTES, pinned, sel.data_ptr(), STORE, None)
        assert rc != 0 and "d_out must be device memory" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_u16_where(t.data_ptr(), n, m.data_ptr(), 0, BYTES, out.data_ptr(), pinned, STORE, None)
        assert rc != 0 and "d_selected must be device memory" in err(hip), err(hip)
        assert not any(ctypes.string_at(pinned, 512))
    finally:
        hip.FLAGSTATS_hip_host_free(pinned)
    untouched("host pointers")
    # extents: a selection one byte short of what the last element needs (its allocation is fine for one element less), an array
    # one flag short, counters 8 bytes short
    nbytes = 2 << 20
    raw = hip.FLAGSTATS_hip_device_alloc(nbytes)
    assert raw
    try:
        assert hip.FLAGSTATS_hip_memcpy_h2d(raw, np.zeros(nbytes, dtype=np.uint8).ctypes.data, nbytes) == 0
        for bits, off in ((BITMAP, 8 * nbytes - 5), (BYTES, nbytes - 5)):
            rc = hip.FLAGSTATS_hip_device_u16_where(t.data_ptr(), 6, raw, off, bits, out.data_ptr(), sel.data_ptr(), STORE, None)
            assert rc != 0 and "d_sel" in err(hip) and "1 bytes short" in err(hip), err(hip)
            rc = hip.FLAGSTATS_hip_device_u16_where_sync(t.data_ptr(), 6, raw, off, bits, h_out.ctypes.data, ctypes.byref(h_sel), STORE)
            assert rc != 0 and "d_sel" in err(hip) and "1 bytes short" in err(hip), err(hip)
            untouched("selection extent")
            o = np.full(32, BIAS, dtype=np.uint64)
            assert hip.FLAGSTATS_hip_device_u16_where_sync(t.data_ptr(), 5, raw, off, bits, o.ctypes.data, None, STORE) == 0, err(hip)
            assert not o.any()
        # an offset exactly at the allocation's end, and one 4 KiB beyond it: the first byte needed is no byte of the allocation
        # at all, and the check runs from d_sel itself (an address past the end is nothing the runtime could vouch for)
        for bits, unit in ((BITMAP, 8), (BYTES, 1)):
            for beyond in (0, 4096):
                off = unit * (nbytes + beyond)
                short = "%d bytes short" % (beyond + 1)
                rc = hip.FLAGSTATS_hip_device_u16_where(t.data_ptr(), 1, raw, off, bits, out.data_ptr(), sel.data_ptr(), STORE, None)
                assert rc != 0 and "d_sel" in err(hip) and short in err(hip), (bits, beyond, err(hip))
                rc = hip.FLAGSTATS_hip_device_u16_where_sync(t.data_ptr(), 1, raw, off, bits, h_out.ctypes.data, ctypes.byref(h_sel), STORE)
                assert rc != 0 and "d_sel" in err(hip) and short in err(hip), (bits, beyond, err(hip))
            untouched("selection offset at or past the end")
            o = np.full(32, BIAS, dtype=np.uint64)         # the last element the allocation does hold
            assert hip.FLAGSTATS_hip_device_u16_where_sync(t.data_ptr(), 1, raw, unit * nbytes - 1, bits, o.ctypes.data, None, STORE) == 0, err(hip)
            assert not o.any()
        rc = hip.FLAGSTATS_hip_device_u16_where(raw, nbytes // 2 + 1, m.data_ptr(), 0, BITMAP, out.data_ptr(), sel.data_ptr(), STORE, None)
        assert rc != 0 and "d_array" in err(hip) and "2 bytes short" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_u16_where(t.data_ptr(), n, m.data_ptr(), 0, BYTES, raw + nbytes - 248, sel.data_ptr(), 0, None)
        assert rc != 0 and "d_out" in err(hip) and "8 bytes short" in err(hip), err(hip)
    finally:
        hip.FLAGSTATS_hip_device_free(raw)
    untouched("extents")
    # the launcher itself: other mode bits, no workgroups, other encodings, a wave's uint32 totals -- nothing queued
    words = torch.full((33,), BIAS, dtype=torch.int64, device="cuda")
    p = words.data_ptr()
    assert hip.fsk_launch_where(t.data_ptr(), 8, m.data_ptr(), 0, BYTES, p, p + 256, 4, 1, None) != 0
    assert hip.fsk_launch_where(t.data_ptr(), 8, m.data_ptr(), 0, BYTES, p, p + 256, 0, 0, None) != 0
    assert hip.fsk_launch_where(t.data_ptr(), 8, m.data_ptr(), 0, 2, p, p + 256, 0, 1, None) != 0
    assert hip.fsk_launch_where(t.data_ptr(), 1 << 35, m.data_ptr(), 0, BITMAP, p, p + 256, STORE, 1, None) != 0
    torch.cuda.synchronize()
    assert (words == BIAS).all()
