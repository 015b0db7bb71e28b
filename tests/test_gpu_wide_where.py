"""The selected-elements flagstat of int32 / int64 columns on the MI355X: fsk::flagstat_count_wide_where at both widths and in
both encodings of the selection, the three C entries and libflagstats_amd/wide_where.py.

Expected values never come from the code under test: wide_where_oracle.want is oracle.flagstat_c of the low 16 bits of
values[mask] (superset slots from oracle.samtools_counts and the definition), `selected` is int(mask.sum()) and `high` is the OR
of values[mask] with the low 16 bits cleared -- of the SELECTED elements only.  Elements that are not selected and everything
around the array are poison wherever a test can afford it: low 16 bits 0xFFFF and every bit above bit 15 set, so one leaked
element lights the fail-QC counters and `high`."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_where_oracle as wwo  # noqa: E402
from test_gpu_wide_filter import (ALL_HIGH, BIAS, GARBAGE, HIGH_BIAS, MODES, SEL_BIAS, SIGNED, STEP, UNSIGNED, WIDTHS, Rows, dev8,  # noqa: E402
                                  err, expect_row, expect_triple, signed, to_device, u64)
from wide_where_oracle import BITMAP, BYTES, pack  # noqa: E402

pytestmark = pytest.mark.gpu

STORE, SUPERSET = 1, 2
ENCODINGS = (BITMAP, BYTES)
ROW = {4: 256, 8: 128}                        # elements of one wave's row of 64 vectors
BYTE_ALIGNMENTS = (0, 1, 3, 8, 15)
PAD = 16                                      # bytes of all-ones around every selection


def poisoned(values, mask, W):
    """`values` (low 16 bits and whatever high bits they carry) where the mask selects, poison elsewhere, as unsigned W-byte"""
    v = np.asarray(values).astype(UNSIGNED[W])
    v[~np.asarray(mask, dtype=bool)] = wwo.poison(W)
    return v


def selection(mask, enc, off, byte_values=None):
    """the host bytes of a selection in a slab of all-ones bytes, and (offset of the selection pointer in it, sel_offset): the
    bitmap starts `off` bits into its first byte (unused bits of its first and last byte are ones), the byte form `off` bytes
    past a 16-byte boundary"""
    m = np.asarray(mask, dtype=bool)
    if enc == BITMAP:
        body = pack(m, off, fill=1)
        return np.concatenate([np.full(PAD, 0xFF, np.uint8), body, np.full(PAD, 0xFF, np.uint8)]), PAD, off
    body = m.astype(np.uint8) if byte_values is None else np.where(m, byte_values, 0).astype(np.uint8)
    slab = np.full((PAD + 16 + m.size + PAD + 15) // 16 * 16, 0xFF, dtype=np.uint8)
    slab[PAD + off:PAD + off + m.size] = body
    return slab, PAD + off, 0


class Packer:
    """many host arrays in one device allocation, each at a 16-byte boundary"""

    def __init__(self, dtype):
        self.dtype, self.parts, self.pos = np.dtype(dtype), [], 0

    def add(self, a):
        per = 16 // self.dtype.itemsize
        a = np.ascontiguousarray(a, dtype=self.dtype)
        padded = np.zeros((a.size + per - 1) // per * per, dtype=self.dtype)
        padded[:a.size] = a
        at = self.pos
        self.parts.append(padded)
        self.pos += padded.size
        return at

    def upload(self):
        import torch
        host = np.concatenate(self.parts) if self.parts else np.zeros(16, dtype=self.dtype)
        self.t = torch.from_numpy(host.view(SIGNED.get(self.dtype.itemsize, np.uint8)) if self.dtype.itemsize > 1 else host).cuda()
        assert self.t.data_ptr() % 16 == 0
        return self.t.data_ptr()


def launch(hip, grid, ptr, n, W, sel, off, enc, rows, k, mode):
    """through fsk_launch_wide_where at `grid` workgroups, or (grid None) the public device entry; on the null stream"""
    if grid is None:
        rc = hip.FLAGSTATS_hip_device_wide_where(ptr if n else None, n, W, sel if n else None, off, enc, rows.out(k), rows.selected(k),
                                                 rows.high(k), mode, None)
        assert rc == 0, (rows.notes[k], err(hip))
    else:
        rc = hip.fsk_launch_wide_where(ptr if n else None, n, W, sel if n else None, off, enc, rows.out(k), rows.selected(k), rows.high(k),
                                       mode, grid, None)
        assert rc == 0, (rows.notes[k], rc)


def host_call(entry, src, n, W, sel, off, enc, mode, want, selected, high, note, hip):
    """a _sync or host-form call over garbage (store) or bias words (+=), all three results checked"""
    store = bool(mode & STORE)
    o = np.full(32, GARBAGE if store else BIAS, dtype=np.uint64)
    s = ctypes.c_uint64(GARBAGE if store else SEL_BIAS)
    h = ctypes.c_uint64(GARBAGE if store else HIGH_BIAS)
    rc = entry(src, n, W, sel, off, enc, o.ctypes.data, ctypes.byref(s), ctypes.byref(h), mode)
    assert rc == 0, (note, err(hip))
    got = np.concatenate([o, [np.uint64(s.value)], [np.uint64(h.value)]])
    assert np.array_equal(got, expect_triple(want, selected, high, mode)), (note, got)


# ------------------------------------------------------------------ 1. every value through every form
@pytest.mark.parametrize("dtype", ["int32", "uint32", "int64", "uint64"])
def test_every_value_through_every_form(hip, oracle_mod, dtype):
    """0..65535 once each, shuffled among 65,536 poison elements; the mask selects exactly the real values, a few of which carry
    one bit above bit 15.  Bitmap (5 bits into its first byte) and bytes, store + superset over garbage and += over bias words,
    through the device entry, the _sync form and the host form; a second += call adds; n == 0 in both modes"""
    W = np.dtype(dtype).itemsize
    rng = np.random.RandomState(2026)
    n = 131072
    mask = np.zeros(n, dtype=bool)
    mask[rng.permutation(n)[:65536]] = True
    column = np.zeros(n, dtype=np.uint64)
    column[mask] = rng.permutation(65536)
    carriers = np.flatnonzero(mask)[11::9001]
    for k, i in enumerate(carriers):
        column[i] |= np.uint64(1) << np.uint64(16 + (5 * k) % (8 * W - 16))
    values = poisoned(column, mask, W).view(dtype)
    want, nsel, high = wwo.want(oracle_mod, values, mask, superset=True)
    assert nsel == 65536 and high not in (0, ALL_HIGH[W])
    assert np.array_equal(np.sort(wwo.low16(values)[mask]), np.arange(65536))
    t = to_device(values)
    sels = {}
    for enc in ENCODINGS:
        host, at, off = selection(mask, enc, 5)
        sels[enc] = (host, dev8(host), at, off)
    rows = Rows()
    plan = []
    for enc in ENCODINGS:
        for mode in MODES:
            plan.append((enc, mode, 65536 * 2, rows.add(mode, want, nsel, high, ("device", dtype, enc, mode)), 1))
        plan.append((enc, 0, 65536 * 2, rows.add(0, 2 * want, 2 * nsel, high, ("device twice", dtype, enc)), 2))
        for mode in MODES:
            plan.append((enc, mode, 0, rows.add(mode, np.zeros(32, dtype=np.uint64), 0, 0, ("n == 0", dtype, enc, mode)), 1))
    rows.upload()
    for enc, mode, n_, k, times in plan:
        _, d, at, off = sels[enc]
        for _ in range(times):
            launch(hip, None, t.data_ptr(), n_, W, d.data_ptr() + at, off, enc, rows, k, mode)
    rows.check()
    for name, entry, src in (("sync", hip.FLAGSTATS_hip_device_wide_where_sync, t.data_ptr()),
                             ("host", hip.FLAGSTATS_hip_wide_x64_where, values.ctypes.data)):
        for enc in ENCODINGS:
            host, d, at, off = sels[enc]
            sel = d.data_ptr() + at if name == "sync" else host.ctypes.data + at
            for mode in MODES:
                host_call(entry, src, n, W, sel, off, enc, mode, want, nsel, high, (name, dtype, enc, mode), hip)
                host_call(entry, None, 0, W, None, off, enc, mode, np.zeros(32, dtype=np.uint64), 0, 0, (name, "n == 0", enc, mode), hip)


# ------------------------------------------------------------------ 2. lengths, phases and offsets
def lengths(W):
    R, S = ROW[W], STEP[W]
    return (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, R - 1, R, R + 1, S - 1, S, S + 1, 2 * S - 1, 2 * S + 1)


@pytest.mark.parametrize("W", WIDTHS)
def test_lengths_phases_and_offsets(hip, oracle_mod, W):
    """every length around nothing, a vector, a selection byte, a wave's row and one and two steps x every element phase of a
    16-byte line x {bitmap at bit offsets 0..7, bytes at alignments 0, 1, 3, 8, 15}.  The array sits in a slab of poison and its
    own unselected elements are poison too; the selection sits in a slab of all-ones bytes and the unused bits of its first and
    last byte are ones: one element or one selection bit taken from outside [0, n), or from the wrong place, changes `selected`,
    the counters or `high`.  Through fsk_launch_wide_where at grids 1, 2, 3 and the public device entry, store form over garbage
    and += over bias"""
    LENGTHS = lengths(W)
    EPV = 16 // W
    rng = np.random.RandomState(57 + W)
    nmax = LENGTHS[-1]
    mask = rng.randint(0, 2, nmax).astype(bool)
    mask[:18] = [1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1, 0, 1]
    body = poisoned(rng.randint(0, 65536, nmax), mask, W)
    wants = {n: wwo.want(oracle_mod, body[:n], mask[:n], superset=True) for n in LENGTHS}
    for n, (_, nsel, high) in wants.items():
        assert high == 0 and (n < 7 or 0 < nsel < n), n
    arrays, a_at = Packer(UNSIGNED[W]), {}
    for n in LENGTHS:
        for phase in range(EPV):
            region = np.full(64 + EPV + n + 64, wwo.poison(W), dtype=UNSIGNED[W])
            region[64 + phase:64 + phase + n] = body[:n]
            a_at[n, phase] = arrays.add(region) + 64 + phase
    sels, s_at = Packer(np.uint8), {}
    for n in LENGTHS:
        for enc, offsets in ((BITMAP, range(8)), (BYTES, BYTE_ALIGNMENTS)):
            for o in offsets:
                host, at, off = selection(mask[:n], enc, o)
                s_at[n, enc, o] = (sels.add(host) + at, off)
    pa, ps = arrays.upload(), sels.upload()
    rows = Rows()
    calls = []
    for n in LENGTHS:
        want, nsel, high = wants[n]
        for phase in range(EPV):
            ptr = pa + W * a_at[n, phase]
            assert ptr % 16 == W * phase
            for (n_, enc, o), (at, off) in s_at.items():
                if n_ != n:
                    continue
                assert enc == BITMAP or (ps + at) % 16 == o
                for grid in (1, 2, 3, None):
                    for mode in MODES:
                        k = rows.add(mode, want, nsel, high, (W, n, phase, enc, o, grid, mode))
                        calls.append((grid, ptr, n, ps + at, off, enc, k, mode))
    rows.upload()
    for grid, ptr, n, sel, off, enc, k, mode in calls:
        launch(hip, grid, ptr, n, W, sel, off, enc, rows, k, mode)
    rows.check()


# ------------------------------------------------------------------ 3. which bit belongs to which element
def positions(W):
    R, S = ROW[W], STEP[W]
    return tuple(range(18)) + (R - 1, R, R + 1, S - 1, S, S + 1, 2 * S - 1)


@pytest.mark.parametrize("W,phase,off", [(4, 0, 0), (4, 3, 2), (8, 0, 0), (8, 1, 0)])
@pytest.mark.parametrize("enc", ENCODINGS)
def test_which_bit_belongs_to_which_element(hip, oracle_mod, W, phase, off, enc):
    """n = 2 STEP elements, all poison and none selected but one: element p = 0x0041 with its bit (byte) set alone gives the row
    of one 0x0041, selected == 1 and high == 0.  (4, 3, 2) and (8, 1, 0) put the kernel's shift at 7: lanes whose 4 or 2 bits
    straddle two bitmap bytes, next to lanes whose bits do not"""
    n = 2 * STEP[W]
    if enc == BITMAP and (W, phase, off) in ((4, 3, 2), (8, 1, 0)):
        assert (off + 8 - phase) & 7 == 7
    one, _, _ = wwo.want(oracle_mod, np.array([0x0041], dtype=UNSIGNED[W]), np.ones(1, dtype=bool), superset=True)
    slab = to_device(np.full(64 + 16 // W + n + 64, wwo.poison(W), dtype=UNSIGNED[W]))
    arr = slab[64 + phase:64 + phase + n]
    assert arr.data_ptr() % 16 == W * phase
    host, at, sel_off = selection(np.zeros(n, dtype=bool), enc, off)
    if enc == BITMAP:                      # nothing around the bitmap is set either: the one bit is the only one
        host[:] = 0
    d_sel = dev8(host)
    rows = Rows()
    plan = [(p, rows.add(STORE | SUPERSET, one, 1, 0, (W, phase, off, enc, p))) for p in positions(W)]
    rows.upload()
    for p, k in plan:
        arr[p] = 0x0041
        where = at + (sel_off + p) // 8 if enc == BITMAP else at + p
        d_sel[where] = 1 << ((sel_off + p) % 8) if enc == BITMAP else 1
        launch(hip, 3, arr.data_ptr(), n, W, d_sel.data_ptr() + at, sel_off, enc, rows, k, STORE | SUPERSET)
        arr[p] = -1
        d_sel[where] = 0
    rows.check()


# ------------------------------------------------------------------ 4. `high` is exact, local and sees selected elements only
@pytest.mark.parametrize("W", WIDTHS)
def test_high_is_exact_local_and_sees_selected_elements_only(hip, oracle_mod, W):
    """2 STEP + 100 elements one element into a line on 2 workgroups: a head edge step [0, S - 1), a fast step [S - 1, 2 S - 1),
    a tail edge step.  For every bit above bit 15, that bit alone on one element -- the first, the last, and the elements on both
    sides of the seam between the edge step and the fast step: selected, exactly that bit is reported; the same array with that
    element not selected reports 0 and counts the column without it.  Its neighbours are selected and clean.  Bitmap and bytes
    alternate; a NULL d_high or d_selected leaves the other results as they are"""
    S = STEP[W]
    n = 2 * S + 100
    spots = (0, S - 2, S - 1, n - 1)
    rng = np.random.RandomState(61 + W)
    low = rng.randint(0, 65536, n).astype(np.uint16)
    base_mask = rng.randint(0, 2, n).astype(bool)
    slab = to_device(np.full(16 // W + n + 8, wwo.poison(W), dtype=UNSIGNED[W]))
    arr = slab[1:1 + n]
    assert arr.data_ptr() % 16 == W
    arr.copy_(to_device(low.astype(UNSIGNED[W])))
    setups = {}
    for at in spots:
        on = base_mask.copy()
        on[max(at - 1, 0):at + 2] = True
        off = on.copy()
        off[at] = False
        for enc in ENCODINGS:
            for name, m in (("on", on), ("off", off)):
                host, sel_at, sel_off = selection(m, enc, 3)
                setups[at, enc, name] = (dev8(host), sel_at, sel_off, wwo.want(oracle_mod, low.astype(UNSIGNED[W]), m, superset=True))
        assert setups[at, BITMAP, "on"][3][1] == setups[at, BITMAP, "off"][3][1] + 1
    rows = Rows()
    plan = []
    for bit in range(16, 8 * W):
        for i, at in enumerate(spots):
            enc = ENCODINGS[(bit + i) & 1]
            for name in ("on", "off"):
                mode = MODES[(bit + i) & 1] if bit != 40 else STORE | SUPERSET       # HIGH_BIAS is bit 40
                want = setups[at, enc, name][3]
                assert want[2] == 0
                k = rows.add(mode, want[0], want[1], 1 << bit if name == "on" else 0, (W, bit, at, enc, name, mode))
                plan.append((k, at, bit, enc, name, mode))
    rows.upload()
    for k, at, bit, enc, name, mode in plan:
        d, sel_at, sel_off, _ = setups[at, enc, name]
        arr[at] = signed(int(low[at]) | (1 << bit), W)
        launch(hip, 2, arr.data_ptr(), n, W, d.data_ptr() + sel_at, sel_off, enc, rows, k, mode)
        arr[at] = int(low[at])
    rows.check()
    # NULL d_high, NULL d_selected, both: every high bit on a selected element
    at = S - 1
    arr[at] = signed(int(low[at]) | ALL_HIGH[W], W)
    rows = Rows()
    plan = []
    for enc in ENCODINGS:
        want = setups[at, enc, "on"][3]
        for report in ((True, False), (False, True), (False, False)):
            for mode in MODES:
                for grid in (2, None):
                    plan.append((rows.add(mode, want[0], want[1], ALL_HIGH[W], (W, "NULL words", enc, report, mode, grid), report=report),
                                 enc, report, mode, grid))
    rows.upload()
    for k, enc, report, mode, grid in plan:
        d, sel_at, sel_off, _ = setups[at, enc, "on"]
        sel = rows.selected(k) if report[0] else None
        high = rows.high(k) if report[1] else None
        if grid is None:
            assert hip.FLAGSTATS_hip_device_wide_where(arr.data_ptr(), n, W, d.data_ptr() + sel_at, sel_off, enc, rows.out(k), sel, high,
                                                       mode, None) == 0, err(hip)
        else:
            assert hip.fsk_launch_wide_where(arr.data_ptr(), n, W, d.data_ptr() + sel_at, sel_off, enc, rows.out(k), sel, high, mode, grid,
                                             None) == 0
    rows.check()
    host = arr.cpu().numpy()
    for enc in ENCODINGS:
        d, sel_at, sel_off, want = setups[at, enc, "on"]
        h_sel = d.cpu().numpy()
        for entry, src, sel in ((hip.FLAGSTATS_hip_device_wide_where_sync, arr.data_ptr(), d.data_ptr() + sel_at),
                                (hip.FLAGSTATS_hip_wide_x64_where, host.ctypes.data, h_sel.ctypes.data + sel_at)):
            for mode in MODES:
                o = np.full(32, GARBAGE if mode & STORE else BIAS, dtype=np.uint64)
                assert entry(src, n, W, sel, sel_off, enc, o.ctypes.data, None, None, mode) == 0, err(hip)
                assert np.array_equal(o, expect_row(want[0], mode))


# ------------------------------------------------------------------ 5. densities and byte values
@pytest.mark.parametrize("W", WIDTHS)
def test_densities_and_byte_values(hip, oracle_mod, W):
    """nothing selected gives zeros and high == 0 over a column of poison; everything selected is the oracle over the whole
    array, high bits included; density one half; selection bytes 1, 2, 0x80 and 0xFF all select"""
    S = STEP[W]
    n = 2 * S + 37
    phase = 16 // W - 1
    rng = np.random.RandomState(67 + W)
    full = rng.randint(0, 65536, n).astype(UNSIGNED[W])
    full[rng.randint(0, n, 9)] |= UNSIGNED[W](1 << 19)
    full[n - 1] |= UNSIGNED[W](1 << (8 * W - 1))
    half = rng.randint(0, 2, n).astype(bool)
    cases = [("none", np.full(n, wwo.poison(W), dtype=UNSIGNED[W]), np.zeros(n, dtype=bool), None),
             ("all", full, np.ones(n, dtype=bool), None),
             ("half", poisoned(full, half, W), half, None),
             ("byte values", poisoned(full, half, W), half, np.array([1, 2, 0x80, 0xFF], dtype=np.uint8)[rng.randint(0, 4, n)])]
    arrays, sels = Packer(UNSIGNED[W]), Packer(np.uint8)
    rows = Rows()
    plan = []
    for name, values, mask, byte_values in cases:
        want, nsel, high = wwo.want(oracle_mod, values, mask, superset=True)
        if name == "none":
            assert nsel == 0 and high == 0 and not want.any()
        if name == "all":
            assert nsel == n and high == (1 << 19) | (1 << (8 * W - 1))
        region = np.full(64 + n + 64, wwo.poison(W), dtype=UNSIGNED[W])
        region[64 + phase:64 + phase + n] = values
        a = arrays.add(region) + 64 + phase
        for enc in ENCODINGS if byte_values is None else (BYTES,):
            host, at, off = selection(mask, enc, 6, byte_values)
            s = sels.add(host) + at
            for mode in MODES:
                for grid in (3, None):
                    plan.append((grid, a, s, off, enc, rows.add(mode, want, nsel, high, (W, name, enc, mode, grid)), mode))
    pa, ps = arrays.upload(), sels.upload()
    rows.upload()
    for grid, a, s, off, enc, k, mode in plan:
        launch(hip, grid, pa + W * a, n, W, ps + s, off, enc, rows, k, mode)
    rows.check()


# ------------------------------------------------------------------ 6. epochs
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("enc", ENCODINGS)
def test_epochs(hip, oracle_mod, W, enc):
    """one workgroup over 258 STEP + 3 elements: 258 fast steps and a tail edge step, so every wave passes its staggered first
    flush (after 255, 191, 127 and 63 pushes) and wave 0 a full epoch of 255 steps.  The mask has density near one half; one
    selected and one unselected element carry a high bit, and only the selected one's is reported"""
    n = 258 * STEP[W] + 3
    values = np.resize(np.random.RandomState(307).randint(0, 65536, 65_521).astype(np.uint16), n).astype(UNSIGNED[W])
    mask = np.resize(np.random.RandomState(308).randint(0, 2, 65_519).astype(bool), n)
    on, off = int(np.flatnonzero(mask)[n // 4]), int(np.flatnonzero(~mask)[n // 3])
    values[on] |= UNSIGNED[W](1 << 16)
    values[off] |= UNSIGNED[W](1 << (8 * W - 1))
    want, nsel, high = wwo.want(oracle_mod, values, mask, superset=True)
    assert abs(nsel - n // 2) < n // 50 and high == 1 << 16
    t = to_device(values)
    host, at, sel_off = selection(mask, enc, 5)
    d = dev8(host)
    assert t.data_ptr() % 16 == 0
    rows = Rows()
    ks = [rows.add(mode, want, nsel, high, (W, enc, mode)) for mode in MODES]
    rows.upload()
    for k in ks:
        launch(hip, 1, t.data_ptr(), n, W, d.data_ptr() + at, sel_off, enc, rows, k, rows.modes[k])
    rows.check()


# ------------------------------------------------------------------ 7. atomics
def test_three_streams_add_into_one_triple(hip, oracle_mod):
    import torch
    from libflagstats_amd import wide_where
    rng = np.random.RandomState(79)
    out = torch.zeros(32, dtype=torch.int64, device="cuda")
    selected = torch.zeros(1, dtype=torch.int64, device="cuda")
    high = torch.zeros(1, dtype=torch.int64, device="cuda")
    total, total_sel, total_high = np.zeros(32, dtype=np.uint64), 0, 0
    inputs = []
    for W, n, packed, bit in ((4, 40 * STEP[4] + 11, True, 17), (8, 37 * STEP[8] + 5, False, 45), (4, 43 * STEP[4] - 3, True, 31)):
        mask = rng.randint(0, 3, n) > 0
        column = rng.randint(0, 65536, n).astype(UNSIGNED[W])
        column[np.flatnonzero(mask)[n // 3]] |= UNSIGNED[W](1 << bit)
        values = poisoned(column, mask, W)
        want, nsel, h = wwo.want(oracle_mod, values, mask, superset=True)
        assert nsel > 0 and h == 1 << bit
        total += want
        total_sel += nsel
        total_high |= h
        where = dev8(pack(mask, 3)) if packed else torch.from_numpy(mask).cuda()
        inputs.append((to_device(values), where, packed))
    streams = [torch.cuda.Stream() for _ in inputs]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    for st, (t, where, packed) in zip(streams, inputs):
        with torch.cuda.stream(st):
            wide_where.count_torch_ints_where(t, where, out=out, selected=selected, high=high, superset=True, packed=packed,
                                              bit_offset=3 if packed else 0)
    for st in streams:
        st.synchronize()
    assert np.array_equal(u64(out), total) and int(u64(selected)[0]) == total_sel and int(u64(high)[0]) == total_high


# ------------------------------------------------------------------ 8. host form across chunks
@pytest.mark.parametrize("W", WIDTHS)
def test_host_form_across_chunks(hip, oracle_mod, W):
    """the "chunk_flags" knob at 65544, 8192, 1000 and 8 (chunks of 32,772 / 16,386, 4,096 / 2,048, 500 / 250 and 4 / 2
    elements): all but 8192 put the chunk seams at bit positions of the bitmap that are not byte-aligned, and the bitmap starts
    5 bits into its first byte.  A high bit on one selected element of a late chunk, poison where the mask does not select"""
    from libflagstats_amd import _lib, wide_where
    rng = np.random.RandomState(91 + W)
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        for chunk_flags, n in ((65544, 70001), (8192, 70001), (1000, 70001), (1000, 1501), (8, 1501)):
            per_chunk = chunk_flags * 2 // W
            assert n > 2 * per_chunk
            mask = rng.randint(0, 2, n).astype(bool)
            column = rng.randint(0, 65536, n).astype(UNSIGNED[W])
            carrier = int(np.flatnonzero(mask)[-7])
            assert carrier >= per_chunk
            column[carrier] |= UNSIGNED[W](1 << (8 * W - 2))
            values = poisoned(column, mask, W).view(SIGNED[W])
            bits = pack(mask, 5)
            _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", chunk_flags), "chunk_flags")
            wants = {sup: wwo.want(oracle_mod, values, mask, superset=bool(sup)) for sup in (0, SUPERSET)}
            _, nsel, high = wants[0]
            assert 0 < nsel < n and high == 1 << (8 * W - 2)
            for sup in (0, SUPERSET):
                got, selected, h = wide_where.counters_ints_where(values, bits, packed=True, bit_offset=5, superset=bool(sup))
                assert np.array_equal(got, wants[sup][0]) and selected == nsel and h == high, (chunk_flags, n, "bitmap", sup)
                got, selected, h = wide_where.counters_ints_where(values, mask, superset=bool(sup))
                assert np.array_equal(got, wants[sup][0]) and selected == nsel and h == high, (chunk_flags, n, "bytes", sup)
            for flags in (0, SUPERSET):                  # += over bias words
                host_call(hip.FLAGSTATS_hip_wide_x64_where, values.ctypes.data, n, W, bits.ctypes.data, 5, BITMAP, flags, wants[SUPERSET][0],
                          nsel, high, (W, chunk_flags, n, flags), hip)
            # the chunks in front of the carrier report nothing; a single chunk
            got, selected, h = wide_where.counters_ints_where(values[:per_chunk], bits, packed=True, bit_offset=5)
            assert h == 0 and selected == int(mask[:per_chunk].sum())
            sub, subm = values[2:min(per_chunk, 99) + 2], mask[2:min(per_chunk, 99) + 2]
            got, selected, h = wide_where.counters_ints_where(sub, subm)
            want1, nsel1, high1 = wwo.want(oracle_mod, sub, subm)
            assert np.array_equal(got, want1) and selected == nsel1 and h == high1
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old


# ------------------------------------------------------------------ 9. refusals that need a device
def test_device_dependent_refusals(hip):
    """what the C entries and the launcher refuse: the lists of test_gpu_wide.test_device_refusals and
    test_gpu_where.test_device_dependent_refusals.  Every one is an argument check that returns before anything is launched, and
    the outputs stay as they were"""
    import torch
    n = 4096
    bufs = {W: torch.zeros(n + 8, dtype={4: torch.int32, 8: torch.int64}[W], device="cuda") for W in WIDTHS}
    m = torch.ones(n + 8, dtype=torch.uint8, device="cuda")
    out = torch.full((32,), BIAS, dtype=torch.int64, device="cuda")
    sel = torch.full((1,), SEL_BIAS, dtype=torch.int64, device="cuda")
    high = torch.full((1,), HIGH_BIAS, dtype=torch.int64, device="cuda")
    h_out = np.full(32, BIAS, dtype=np.uint64)
    h_sel, h_high = ctypes.c_uint64(SEL_BIAS), ctypes.c_uint64(HIGH_BIAS)
    host = np.zeros(n + 8, dtype=np.int64)
    host8 = np.ones(n + 8, dtype=np.uint8)
    p8, p4 = bufs[8].data_ptr(), bufs[4].data_ptr()

    def untouched(what):
        torch.cuda.synchronize()
        assert (out == BIAS).all() and int(u64(sel)[0]) == SEL_BIAS and int(u64(high)[0]) == HIGH_BIAS, what
        assert (h_out == BIAS).all() and h_sel.value == SEL_BIAS and h_high.value == HIGH_BIAS, what

    def refused(what, text, d_array=p8, n_=n, eb=8, d_sel=m.data_ptr(), off=0, bits=BYTES, flags=0, counters=True,
                forms=("device", "sync", "host")):
        for form in forms:
            if form == "device":
                rc = hip.FLAGSTATS_hip_device_wide_where(d_array, n_, eb, d_sel, off, bits, out.data_ptr() if counters else None,
                                                         sel.data_ptr(), high.data_ptr(), flags, None)
            elif form == "sync":
                rc = hip.FLAGSTATS_hip_device_wide_where_sync(d_array, n_, eb, d_sel, off, bits, h_out.ctypes.data if counters else None,
                                                              ctypes.byref(h_sel), ctypes.byref(h_high), flags)
            else:
                src = host.ctypes.data + (d_array - p8) % 8 if d_array else None
                rc = hip.FLAGSTATS_hip_wide_x64_where(src, n_, eb, host8.ctypes.data if d_sel else None, off, bits,
                                                      h_out.ctypes.data if counters else None, ctypes.byref(h_sel), ctypes.byref(h_high), flags)
            assert rc != 0, (what, form)
            assert text in err(hip), (what, form, err(hip))
        untouched(what)

    # the wide entries' list
    refused("elem_bytes 2", "u16 where entries", eb=2)
    refused("elem_bytes 3", "elem_bytes must be 4 or 8", eb=3)
    refused("elem_bytes 16", "elem_bytes must be 4 or 8", eb=16)
    refused("off by 2 at W = 4", "4-byte aligned", d_array=p8 + 2, eb=4)
    refused("off by 4 at W = 8", "8-byte aligned", d_array=p8 + 4, eb=8)
    refused("an extra flag bit", "no other bits", flags=4)
    refused("NULL array", "NULL array with n > 0", d_array=None, eb=4)
    refused("n * elem_bytes is no size", "n * elem_bytes is not a size", n_=1 << 62)
    # the where entries' list
    for W in WIDTHS:
        pw = bufs[W].data_ptr()
        for bits in (0, 2, 4, 16):
            refused("sel_bits %d" % bits, "sel_bits must be 1", d_array=pw, eb=W, bits=bits)
        refused("NULL selection", "NULL selection with n > 0", d_array=pw, eb=W, d_sel=None)
        refused("sel_offset + n is no index", "sel_offset + n is not an index", d_array=pw, eb=W, off=(1 << 64) - 5)
        refused("NULL counters", "NULL counters", d_array=pw, eb=W, counters=False)
        # a wave's uint32 totals: 2^60 elements on any grid this device launches.  The host form launches per chunk and cannot
        # reach the limit, so it has nothing to refuse here
        refused("a wave's totals", "a wave's uint32 totals", d_array=pw, eb=W, n_=1 << 60, forms=("device", "sync"))
    # host memory where device memory is needed: the array, the selection, d_out (pageable, then page-locked), d_selected, d_high
    for W in WIDTHS:
        pw = bufs[W].data_ptr()
        for bits in ENCODINGS:
            rc = hip.FLAGSTATS_hip_device_wide_where(host.ctypes.data, n, W, m.data_ptr(), 0, bits, out.data_ptr(), sel.data_ptr(),
                                                     high.data_ptr(), 0, None)
            assert rc != 0 and "d_array" in err(hip), err(hip)
            rc = hip.FLAGSTATS_hip_device_wide_where_sync(host.ctypes.data, n, W, m.data_ptr(), 0, bits, h_out.ctypes.data,
                                                          ctypes.byref(h_sel), ctypes.byref(h_high), 0)
            assert rc != 0 and "d_array" in err(hip), err(hip)
            rc = hip.FLAGSTATS_hip_device_wide_where(pw, n, W, host8.ctypes.data, 0, bits, out.data_ptr(), sel.data_ptr(), high.data_ptr(), 0, None)
            assert rc != 0 and "d_sel" in err(hip), err(hip)
            rc = hip.FLAGSTATS_hip_device_wide_where_sync(pw, n, W, host8.ctypes.data, 0, bits, h_out.ctypes.data, ctypes.byref(h_sel),
                                                          ctypes.byref(h_high), 0)
            assert rc != 0 and "d_sel" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_where(pw, n, W, m.data_ptr(), 0, BYTES, h_out.ctypes.data, sel.data_ptr(), high.data_ptr(), 0, None)
        assert rc != 0 and "d_out" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_where(pw, n, W, m.data_ptr(), 0, BYTES, out.data_ptr(), ctypes.addressof(h_sel), high.data_ptr(), 0, None)
        assert rc != 0 and "d_selected" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_where(pw, n, W, m.data_ptr(), 0, BYTES, out.data_ptr(), sel.data_ptr(), ctypes.addressof(h_high), 0, None)
        assert rc != 0 and "d_high" in err(hip), err(hip)
    pinned = hip.FLAGSTATS_hip_host_alloc(512)
    assert pinned
    try:
        ctypes.memset(pinned, 0, 512)
        rc = hip.FLAGSTATS_hip_device_wide_where(p8, n, 8, m.data_ptr(), 0, BYTES, pinned, sel.data_ptr(), high.data_ptr(), STORE, None)
        assert rc != 0 and "d_out must be device memory" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_where(p8, n, 8, m.data_ptr(), 0, BYTES, out.data_ptr(), pinned, high.data_ptr(), STORE, None)
        assert rc != 0 and "d_selected must be device memory" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_where(p8, n, 8, m.data_ptr(), 0, BYTES, out.data_ptr(), sel.data_ptr(), pinned, STORE, None)
        assert rc != 0 and "d_high must be device memory" in err(hip), err(hip)
        assert not any(ctypes.string_at(pinned, 512))
    finally:
        hip.FLAGSTATS_hip_host_free(pinned)
    untouched("host pointers")
    # extents: counters 8 bytes short; an array one element short; a selection one byte short (the bitmap's last byte, the byte
    # form's last byte), counted from the selection pointer
    nbytes = 2 << 20
    raw = hip.FLAGSTATS_hip_device_alloc(nbytes)
    assert raw
    try:
        assert hip.FLAGSTATS_hip_memcpy_h2d(raw, np.zeros(nbytes, dtype=np.uint8).ctypes.data, nbytes) == 0
        rc = hip.FLAGSTATS_hip_device_wide_where(p8, n, 8, m.data_ptr(), 0, BYTES, raw + nbytes - 248, sel.data_ptr(), high.data_ptr(), 0, None)
        assert rc != 0 and "d_out" in err(hip) and "8 bytes short" in err(hip), err(hip)
        for W in WIDTHS:
            big = torch.zeros(8 * nbytes + 8, dtype={4: torch.int32, 8: torch.int64}[W], device="cuda")
            pb = big.data_ptr()
            bigm = torch.ones(nbytes // W + 8, dtype=torch.uint8, device="cuda")
            rc = hip.FLAGSTATS_hip_device_wide_where(raw, nbytes // W + 1, W, bigm.data_ptr(), 0, BYTES, out.data_ptr(), sel.data_ptr(),
                                                     high.data_ptr(), STORE, None)
            assert rc != 0 and "d_array" in err(hip) and "%d bytes short" % W in err(hip), err(hip)
            rc = hip.FLAGSTATS_hip_device_wide_where_sync(raw + W, nbytes // W, W, bigm.data_ptr(), 0, BYTES, h_out.ctypes.data,
                                                          ctypes.byref(h_sel), ctypes.byref(h_high), STORE)
            assert rc != 0 and "d_array" in err(hip) and "%d bytes short" % W in err(hip), err(hip)
            for n_, off, bits in ((nbytes + 1, 0, BYTES), (nbytes, 1, BYTES), (8 * nbytes + 1, 0, BITMAP), (8 * nbytes - 2, 3, BITMAP)):
                rc = hip.FLAGSTATS_hip_device_wide_where(pb, n_, W, raw, off, bits, out.data_ptr(), sel.data_ptr(), high.data_ptr(), STORE, None)
                assert rc != 0 and "d_sel" in err(hip) and "1 bytes short" in err(hip), (n_, off, bits, err(hip))
                rc = hip.FLAGSTATS_hip_device_wide_where_sync(pb, n_, W, raw, off, bits, h_out.ctypes.data, ctypes.byref(h_sel),
                                                              ctypes.byref(h_high), STORE)
                assert rc != 0 and "d_sel" in err(hip) and "1 bytes short" in err(hip), (n_, off, bits, err(hip))
            untouched("extents")
            for n_ok, off, bits in ((nbytes, 0, BYTES), (8 * nbytes - 3, 3, BITMAP)):   # the selection to its very last byte / bit
                o = np.full(32, BIAS, dtype=np.uint64)
                s, h = ctypes.c_uint64(SEL_BIAS), ctypes.c_uint64(HIGH_BIAS)
                assert hip.FLAGSTATS_hip_device_wide_where_sync(pb, n_ok, W, raw, off, bits, o.ctypes.data, ctypes.byref(s), ctypes.byref(h),
                                                                STORE) == 0, err(hip)
                assert not o.any() and s.value == 0 and h.value == 0            # a selection of zeros
            del big, bigm
    finally:
        hip.FLAGSTATS_hip_device_free(raw)
    untouched("extents")
    # the launcher itself: other widths and encodings, misalignment, other mode bits, no workgroups, a wave's uint32 totals, an
    # offset that is no index, NULL pointers -- nothing queued
    words = torch.full((34,), BIAS, dtype=torch.int64, device="cuda")
    p = words.data_ptr()
    f = hip.fsk_launch_wide_where
    for W in WIDTHS:
        pw = bufs[W].data_ptr()
        for bits in ENCODINGS:
            assert f(pw, 8, W, m.data_ptr(), 0, bits, p, p + 256, p + 264, 4, 1, None) != 0
            assert f(pw, 8, W, m.data_ptr(), 0, bits, p, p + 256, p + 264, 0, 0, None) != 0
            assert f(pw, 1 << 35, W, m.data_ptr(), 0, bits, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(pw, 8, W, m.data_ptr(), (1 << 64) - 5, bits, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(pw, 8, W, None, 0, bits, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(None, 8, W, m.data_ptr(), 0, bits, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(pw + W // 2, 8, W, m.data_ptr(), 0, bits, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(pw, 8, W, m.data_ptr(), 0, bits, None, p + 256, p + 264, STORE, 1, None) != 0
        for bits in (0, 2, 4, 16):
            assert f(pw, 8, W, m.data_ptr(), 0, bits, p, p + 256, p + 264, STORE, 1, None) != 0
    for eb in (0, 1, 2, 3, 16):
        assert f(p4, 8, eb, m.data_ptr(), 0, BYTES, p, p + 256, p + 264, STORE, 1, None) != 0
    torch.cuda.synchronize()
    assert (words == BIAS).all()


# ------------------------------------------------------------------ 10. the Python layers
def test_python_layers(hip, oracle_mod):
    """numpy over all six dtypes (the 2-byte ones take the uint16 route and report high == 0), strict and its message -- raised
    for a selected element only --, the dict; the raw-pointer form; the torch layer's dtypes, shapes, placement and its
    device-mismatch refusals"""
    import torch
    from libflagstats_amd import where, wide, wide_where
    n = 3 * STEP[4] + 41
    rng = np.random.RandomState(101)
    low = rng.randint(0, 65536, n).astype(np.uint16)
    mask = rng.randint(0, 3, n) > 0
    bits = pack(mask, 3)
    want, nsel, _ = wwo.want(oracle_mod, low.astype(np.uint32), mask)
    want_sup = wwo.want(oracle_mod, low.astype(np.uint32), mask, superset=True)[0]
    assert 0 < nsel < n
    calls = []
    for dt in ("int16", "uint16", "int32", "uint32", "int64", "uint64"):
        v = low.astype({"int16": np.uint16}.get(dt, dt)).view(dt)
        for kw, w in (({}, mask), ({"packed": True, "bit_offset": 3}, bits)):
            got, selected, high = wide_where.counters_ints_where(v, w, **kw)
            assert got.dtype == np.uint64 and np.array_equal(got, want) and selected == nsel and high == 0, (dt, kw)
            got, selected, high = wide_where.counters_ints_where(v, w, superset=True, **kw)
            assert np.array_equal(got, want_sup) and selected == nsel and high == 0, (dt, kw)
            d = wide_where.flagstats_ints_where(v, w, **kw)
            assert d["n_values"] == nsel and int(d["failed"]["FQCFAIL"]) == int(want[25]) and "high_bits" not in d
            assert int(d["passed"]["mapped"]) == nsel - int(want[2]) - int(want[18])
            assert wide_where.flagstats_ints_where(v, w, strict=False, **kw)["high_bits"] == 0
        if v.dtype.itemsize == 2:
            continue
        W = v.dtype.itemsize
        top = 1 << (8 * W - 1)
        # garbage in a slot that is NOT selected: no high bit, no raise, the same table
        null = v.copy()
        null.view(UNSIGNED[W])[~mask] = wwo.poison(W)
        for kw, w in (({}, mask), ({"packed": True, "bit_offset": 3}, bits)):
            d = wide_where.flagstats_ints_where(null, w, **kw)
            assert d["n_values"] == nsel and int(d["failed"]["FQCFAIL"]) == int(want[25])
            assert wide_where.counters_ints_where(null, w, **kw)[2] == 0
        # a SELECTED element with a bit above bit 15: strict names the bits
        bad = null.copy()
        at = int(np.flatnonzero(mask)[5])
        bad.view(UNSIGNED[W])[at] |= UNSIGNED[W](top)
        with pytest.raises(ValueError) as e:
            wide_where.flagstats_ints_where(bad, mask)
        assert str(e.value) == wide.high_bits_message(top) and "0x%X" % top in str(e.value)
        d = wide_where.flagstats_ints_where(bad, bits, packed=True, bit_offset=3, strict=False)
        assert d["high_bits"] == top and d["n_values"] == nsel and int(d["failed"]["FQCFAIL"]) == int(want[25])
        # the raw-pointer form and the torch layer on the same column
        t, d_bits, d_mask = to_device(bad), dev8(bits), torch.from_numpy(mask).cuda()
        got, selected, high = wide_where.count_device_ptr_ints_where(t.data_ptr(), n, W, d_bits.data_ptr(), 1, sel_offset=3, superset=True)
        assert np.array_equal(got, want_sup) and selected == nsel and high == top
        got, selected, high = wide_where.count_device_ptr_ints_where(t.data_ptr(), n, W, d_mask.data_ptr(), 8)
        assert np.array_equal(got, want) and selected == nsel and high == top
        o, s, h = wide_where.count_torch_ints_where(t, d_mask)
        torch.cuda.synchronize()
        for x, numel in ((o, 32), (s, 1), (h, 1)):
            assert x.dtype == torch.int64 and tuple(x.shape) == (numel,) and x.device == t.device
        assert np.array_equal(u64(o), want) and int(u64(s)[0]) == nsel and int(u64(h)[0]) == top
        o2, s2, h2 = wide_where.count_torch_ints_where(t, d_bits, out=o, selected=s, high=h, packed=True, bit_offset=3)   # += and |=
        assert o2 is o and s2 is s and h2 is h
        torch.cuda.synchronize()
        assert np.array_equal(u64(o), 2 * want) and int(u64(s)[0]) == 2 * nsel and int(u64(h)[0]) == top
        wide_where.count_torch_ints_where(t, d_mask, out=o, selected=s, high=h, store=True, superset=True)
        torch.cuda.synchronize()
        assert np.array_equal(u64(o), want_sup) and int(u64(s)[0]) == nsel and int(u64(h)[0]) == top
    # two-byte dtypes route to the u16 entries: the wide entry is not called, `high` is left as it is (zeroed with store)
    real = where.counters_where

    def spy(*a, **kw):
        calls.append(a[0].dtype)
        return real(*a, **kw)

    where.counters_where = spy
    try:
        wide_where.counters_ints_where(low.view(np.int16), mask)
        wide_where.counters_ints_where(low.astype(np.int32), mask)
    finally:
        where.counters_where = real
    assert calls == [np.dtype(np.uint16)]
    t16 = torch.from_numpy(low.view(np.int16)).cuda()
    d_mask, d_bits = torch.from_numpy(mask).cuda(), dev8(bits)
    h = torch.full((1,), 9, dtype=torch.int64, device="cuda")
    o, s, h2 = wide_where.count_torch_ints_where(t16, d_mask, high=h)
    torch.cuda.synchronize()
    assert h2 is h and int(h[0]) == 9 and np.array_equal(u64(o), want) and int(u64(s)[0]) == nsel
    wide_where.count_torch_ints_where(t16, d_bits, out=o, selected=s, high=h, store=True, packed=True, bit_offset=3)
    torch.cuda.synchronize()
    assert int(h[0]) == 0 and np.array_equal(u64(o), want) and int(u64(s)[0]) == nsel
    # empty inputs
    o, s, h = wide_where.count_torch_ints_where(torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.bool, device="cuda"))
    torch.cuda.synchronize()
    assert not u64(o).any() and int(s[0]) == 0 and int(h[0]) == 0
    got, selected, high = wide_where.counters_ints_where(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool))
    assert not got.any() and selected == 0 and high == 0
    got, selected, high = wide_where.count_device_ptr_ints_where(0, 0, 8, 0, 1)
    assert not got.any() and selected == 0 and high == 0
    # results somewhere else than t
    t = to_device(low.astype(np.uint32))
    with pytest.raises(ValueError, match=r"where must live on t's device \(cuda:0\), not on cpu"):
        wide_where.count_torch_ints_where(t, torch.from_numpy(mask))
    with pytest.raises(ValueError, match=r"out must live on t's device \(cuda:0\), not on cpu"):
        wide_where.count_torch_ints_where(t, d_mask, out=torch.zeros(32, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"selected must live on t's device \(cuda:0\), not on cpu"):
        wide_where.count_torch_ints_where(t, d_mask, selected=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"high must live on t's device \(cuda:0\), not on cpu"):
        wide_where.count_torch_ints_where(t, d_mask, high=torch.zeros(1, dtype=torch.int64))


# ------------------------------------------------------------------ 11. a seeded randomised sweep
def test_seeded_randomised_sweep(hip, oracle_mod):
    """150 cases drawn from the parameters above: width, n up to 2 STEP + 1, array phase, encoding, bit offset or byte alignment,
    density, high bits planted on selected and on unselected elements, mode and grid.  Every case is launched and checked"""
    rng = np.random.RandomState(20261)
    packers = {W: Packer(UNSIGNED[W]) for W in WIDTHS}
    sels = Packer(np.uint8)
    rows = Rows()
    plan = []
    for case in range(150):
        W = WIDTHS[rng.randint(2)]
        S, EPV = STEP[W], 16 // W
        n = int([rng.randint(0, 40), rng.randint(0, 2 * ROW[W]), rng.randint(S - 70, S + 70), rng.randint(0, 2 * S + 2)][rng.randint(4)])
        phase = int(rng.randint(EPV))
        enc = ENCODINGS[rng.randint(2)]
        off = int(rng.randint(8) if enc == BITMAP else rng.randint(16))
        density = (0.02, 0.5, 0.97)[rng.randint(3)]
        mode = MODES[rng.randint(2)]
        grid = (1, 2, 3, None)[rng.randint(4)]
        mask = rng.random_sample(n) < density
        column = rng.randint(0, 65536, n).astype(UNSIGNED[W])
        for i in rng.randint(0, max(n, 1), 3)[:min(n, 3)]:
            column[i] |= UNSIGNED[W](1 << int(rng.randint(16, 8 * W)))
        if rng.randint(2):
            column[~mask] = wwo.poison(W)
        want, nsel, high = wwo.want(oracle_mod, column, mask, superset=True)
        region = np.full(8 + EPV + n + 8, wwo.poison(W), dtype=UNSIGNED[W])
        region[8 + phase:8 + phase + n] = column
        a = packers[W].add(region) + 8 + phase
        host, at, sel_off = selection(mask, enc, off, None if rng.randint(2) else rng.randint(1, 256, n))
        s = sels.add(host) + at
        plan.append((grid, W, a, n, s, sel_off, enc, rows.add(mode, want, nsel, high, (case, W, n, phase, enc, off, density, mode, grid)), mode))
    base = {W: packers[W].upload() for W in WIDTHS}
    ps = sels.upload()
    rows.upload()
    for grid, W, a, n, s, sel_off, enc, k, mode in plan:
        launch(hip, grid, base[W] + W * a, n, W, ps + s, sel_off, enc, rows, k, mode)
    rows.check()
    assert len(plan) == 150
