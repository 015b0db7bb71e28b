"""The filtered flagstat under a selection on the MI355X: fsk::flagstat_filter_where in its six forms ({no MAPQ, MAPQ} x {bitmap,
bitmap funnelled, bytes}), the three C entries and libflagstats_amd/filter_where.py.

Expected counters never come from the code under test: filter_where_oracle.want_counters is oracle.flagstat_c of values[mask]
(superset slots from oracle.samtools_counts and the definition) under filter_oracle.filter_mask(...) & mask; the expected
`selected` is that mask's sum.

Every input is a view into a larger buffer whose surroundings count if they are touched: flags 0xFFFF around the array, MAPQ 255
around the column, set bits / non-zero bytes around the selection's extent."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_oracle  # noqa: E402
import where_oracle  # noqa: E402
from filter_where_oracle import want_counters  # noqa: E402
from test_gpu_where import BIAS, GARBAGE, SEL_BIAS, STORE, SUPERSET, Rows, S, dev8, dev16, err, expect_row, u64  # noqa: E402
from where_oracle import BITMAP, BYTES, pack  # noqa: E402

pytestmark = pytest.mark.gpu

# one vector is 8 flags, a wave's share of a step 4,096, a step 16,384
SMALL = (1, 7, 8, 9, 63)
SEAMS = (4095, 4096, 4097, S - 1, S, S + 1, 3 * S + 5)
STARTS = (0, 2, 14)                               # bytes past a 16-byte boundary
BIG = 8 * 1_000_003 + 5
BIT_OFFSETS = (0, 1, 7, 8, 13, BIG)
MAPQ_ALIGN = (0, 1, 3)                            # bytes past a 4-byte boundary
MIN_MAPQ = (1, 30, 127, 128, 129, 255)            # and 0: the forms without the column
PREDICATES = ((0, 0), (0, 0x904), (0x2, 0x904), (0x0101, 0x8080), (0x40, 0x40), (0xFFFF, 0), (0, 0xFFFF))
MASKS = ("clear", "set", "random", "first", "last")
BYTE_VALUES = (1, 2, 0x80, 0xFF)
FORMS = ("bitmap", "funnel", "bytes")
# (array start, bit offset) pairs: the launch is funnelled iff (bit offset + 8 - start / 2) % 8 != 0
UNFUNNELLED = ((0, 0), (2, 1), (14, 7), (0, 8))
FUNNELLED = ((0, 1), (2, 0), (14, 13), (0, 7), (2, 8), (14, BIG), (0, 13), (14, 0), (2, 7), (0, BIG), (14, 1), (2, 13))


def make_mask(kind, n, rng):
    m = np.zeros(n, dtype=bool)
    if kind == "set":
        m[:] = True
    elif kind == "random":
        m = rng.randint(0, 2, n).astype(bool)
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[-1] = True
    return m


def make_body(n, rng):
    """flags of which every predicate of PREDICATES (but the overlapping pair) passes some, and MAPQ bytes on both sides of
    every threshold"""
    v = rng.randint(0, 65536, n).astype(np.uint16)
    r = rng.randint(0, 100, n)
    v[r < 4] = 0xFFFF
    v[(r >= 4) & (r < 8)] = 0
    v[(r >= 8) & (r < 30)] &= np.uint16(~0x0904 & 0xFFFF)
    v[(r >= 30) & (r < 40)] = (v[(r >= 30) & (r < 40)] & np.uint16(~0x8080 & 0xFFFF)) | np.uint16(0x0101)
    q = rng.randint(0, 256, n).astype(np.uint8)
    near = np.array([0, 1, 29, 30, 31, 126, 127, 128, 129, 130, 254, 255], dtype=np.uint8)
    pick = rng.randint(0, 2, n).astype(bool)
    q[pick] = near[rng.randint(0, near.size, int(pick.sum()))]
    return v, q


class Case:
    """one call's arguments, laid out in poisoned slabs"""

    def __init__(self, n, mq, form, start, offset, mapq_align, min_mapq, pred, mask_kind, note=None):
        self.n, self.mq, self.form, self.start, self.offset = n, mq, form, start, offset
        self.mapq_align, self.min_mapq, self.pred, self.mask_kind = mapq_align, (min_mapq if mq else 0), pred, mask_kind
        self.sel_bits = BYTES if form == "bytes" else BITMAP
        funnelled = self.sel_bits == BITMAP and (offset + 8 - start // 2) % 8 != 0
        assert funnelled == (form == "funnel"), (form, start, offset)
        self.note = note or (n, mq, form, start, offset, mapq_align, self.min_mapq, pred, mask_kind)


def build_cases():
    cases = []
    k = 0
    u = f = j = 0
    for n in SMALL + SEAMS:
        for mq in (False, True):
            for form in FORMS:
                if form == "bitmap":
                    start, offset = UNFUNNELLED[u % len(UNFUNNELLED)]
                    u += 1
                elif form == "funnel":
                    start, offset = FUNNELLED[f % len(FUNNELLED)]
                    f += 1
                else:
                    start, offset = STARTS[k % 3], (0, 5, 1, 16)[k % 4]      # bytes: sel_offset in bytes
                cases.append(Case(n, mq, form, start, offset, MAPQ_ALIGN[(j + j // 3) % 3], MIN_MAPQ[j % len(MIN_MAPQ)],
                                  PREDICATES[k % len(PREDICATES)], MASKS[(k // 3) % len(MASKS)]))
                k += 1
                j += mq
    return cases


def test_the_cases_cover_what_they_must():
    """every value of every axis appears, and every (MAPQ, selection form) pair at every seam"""
    cases = build_cases()
    assert {c.n for c in cases} == set(SMALL + SEAMS)
    for n in SEAMS:
        assert {(c.mq, c.form) for c in cases if c.n == n} == {(mq, form) for mq in (False, True) for form in FORMS}
    assert {c.start for c in cases} == set(STARTS)
    assert {c.offset for c in cases if c.sel_bits == BITMAP} == set(BIT_OFFSETS)
    assert {c.mapq_align for c in cases if c.mq} == set(MAPQ_ALIGN)
    assert {c.min_mapq for c in cases} == set(MIN_MAPQ) | {0}
    assert {c.pred for c in cases} == set(PREDICATES)
    for form in FORMS:
        assert {c.mask_kind for c in cases if c.form == form} == set(MASKS), form
    for mq in (False, True):
        assert {c.pred for c in cases if c.mq == mq} == set(PREDICATES), mq


class Laid:
    """the cases' inputs in three host slabs (flags, MAPQ bytes, selection bytes), uploaded once; expected rows from the oracle"""

    def __init__(self, oracle_mod, cases, seed=4711):
        rng = np.random.RandomState(seed)
        nmax = max(c.n for c in cases)
        self.body, self.mapq = make_body(nmax, rng)
        arrays, cols, sels = [], [], []
        pa = pq = ps = 0
        bodies = {}
        for c in cases:
            n = c.n
            if (n, c.mask_kind) not in bodies:
                bodies[n, c.mask_kind] = make_mask(c.mask_kind, n, rng)
            c.mask = bodies[n, c.mask_kind]
            c.values, c.q = self.body[:n].copy(), self.mapq[:n].copy()
            if not c.pred[0] & c.pred[1]:
                # the first, the middle and the last element pass, so a mask of one element counts one: two different values
                # next to each other, so that a selection read one place off counts something else
                for i in sorted({0, 1, n // 2, n - 2, n - 1} & set(range(n))):
                    c.values[i] = (int(c.values[i]) & ~c.pred[1] & (0xFEFF if i % 2 else 0xFFFF) & 0xFFFF) | c.pred[0]
                    c.q[i] = 255
            c.want, c.nsel = want_counters(oracle_mod, c.values, c.mask, c.pred[0], c.pred[1], c.q, c.min_mapq, superset=True)
            region = np.full((64 + 8 + n + 64 + 7) // 8 * 8, 0xFFFF, dtype=np.uint16)
            at = 64 + c.start // 2
            region[at:at + n] = c.values
            c.a_at = pa + at
            arrays.append(region)
            pa += region.size
            region = np.full((16 + 4 + n + 16 + 15) // 16 * 16, 0xFF, dtype=np.uint8)
            at = 16 + c.mapq_align
            region[at:at + n] = c.q
            c.q_at = pq + at
            cols.append(region)
            pq += region.size
            if c.sel_bits == BITMAP:
                payload = pack(c.mask, c.offset, fill=1)
                first = c.offset // 8
                assert payload.size == (c.offset + n + 7) // 8 and (payload[:first] == 0xFF).all()
            else:
                payload = np.full(c.offset + n, 0xFF, dtype=np.uint8)
                payload[c.offset:] = c.mask.astype(np.uint8) * np.resize(np.array(BYTE_VALUES, dtype=np.uint8), n)
            region = np.full((16 + 3 + payload.size + 16 + 15) // 16 * 16, 0xFF, dtype=np.uint8)
            at = 16 + (len(sels) % 4)               # the selection pointer at every byte alignment
            region[at:at + payload.size] = payload
            c.s_at = ps + at
            sels.append(region)
            ps += region.size
        self.h_arrays, self.h_cols, self.h_sels = np.concatenate(arrays), np.concatenate(cols), np.concatenate(sels)
        self.d_arrays, self.d_cols, self.d_sels = dev16(self.h_arrays), dev8(self.h_cols), dev8(self.h_sels)
        assert self.d_arrays.data_ptr() % 16 == 0 and self.d_cols.data_ptr() % 16 == 0 and self.d_sels.data_ptr() % 16 == 0
        self.cases = cases

    def device_args(self, c):
        """(d_array, d_mapq or None, d_sel) of a case"""
        ptr = self.d_arrays.data_ptr() + 2 * c.a_at
        qptr = self.d_cols.data_ptr() + c.q_at
        assert ptr % 16 == c.start and qptr % 4 == c.mapq_align
        return ptr, (qptr if c.mq else None), self.d_sels.data_ptr() + c.s_at

    def host_args(self, c):
        return (self.h_arrays.ctypes.data + 2 * c.a_at, (self.h_cols.ctypes.data + c.q_at) if c.mq else None,
                self.h_sels.ctypes.data + c.s_at)


@pytest.fixture(scope="module")
def laid(hip, oracle_mod):
    return Laid(oracle_mod, build_cases())


# ------------------------------------------------------------------ 1. the seams, on the device
def test_seams_through_the_device_entry_and_the_launcher(hip, laid):
    """every case through the public device entry (store + superset over garbage, += over bias words) and through
    fsk_launch_filter_where at grids 1, 2 and 3; the byte form's set bytes take the values 1, 2, 0x80 and 0xFF"""
    rows = Rows()
    calls = []
    for c in laid.cases:
        # the inputs are telling ones: whatever can count something does
        if c.mask_kind != "clear" and not c.pred[0] & c.pred[1] and (c.mask_kind != "random" or c.n >= 63):
            assert 0 < c.nsel <= c.n, c.note
        for grid, mode in ((None, STORE | SUPERSET), (None, 0), (1, STORE), (2, SUPERSET), (3, STORE | SUPERSET)):
            calls.append((rows.add(mode, c.want, c.nsel, (c.note, grid, mode)), c, grid, mode))
    rows.upload()
    for k, c, grid, mode in calls:
        ptr, qptr, sptr = laid.device_args(c)
        if grid is None:
            rc = hip.FLAGSTATS_hip_device_u16_filter_where(ptr, c.n, c.pred[0], c.pred[1], qptr, c.min_mapq, sptr, c.offset, c.sel_bits,
                                                           rows.out(k), rows.selected(k), mode, None)
            assert rc == 0, (rows.notes[k], err(hip))
        else:
            rc = hip.fsk_launch_filter_where(ptr, c.n, c.pred[0], c.pred[1], qptr, c.min_mapq, sptr, c.offset, c.sel_bits, rows.out(k),
                                             rows.selected(k), mode, grid, None)
            assert rc == 0, (rows.notes[k], rc)
    rows.check()


# ------------------------------------------------------------------ 2. the seams, synchronous and from host memory
def test_seams_through_the_sync_form(hip, laid):
    from libflagstats_amd import filter_where as fw
    for c in laid.cases:
        ptr, qptr, sptr = laid.device_args(c)
        for mode in (STORE | SUPERSET, 0):
            o = np.full(32, GARBAGE if mode & STORE else BIAS, dtype=np.uint64)
            h = ctypes.c_uint64(GARBAGE if mode & STORE else SEL_BIAS)
            rc = hip.FLAGSTATS_hip_device_u16_filter_where_sync(ptr, c.n, c.pred[0], c.pred[1], qptr, c.min_mapq, sptr, c.offset, c.sel_bits,
                                                                o.ctypes.data, ctypes.byref(h), mode)
            assert rc == 0, (c.note, mode, err(hip))
            assert np.array_equal(o, expect_row(c.want, mode)), (c.note, mode, o)
            assert h.value == c.nsel + (0 if mode & STORE else SEL_BIAS), (c.note, mode)
        got, selected = fw.count_device_ptr_filter_where(ptr, c.n, sptr, c.sel_bits, require=c.pred[0], exclude=c.pred[1], mapq_ptr=qptr or 0,
                                                         min_mapq=c.min_mapq, sel_offset=c.offset, superset=True)
        assert np.array_equal(got, c.want) and selected == c.nsel and got.dtype == np.uint64, c.note


def test_seams_through_the_host_form_in_chunks(hip, oracle_mod, laid):
    """the seams from host memory in chunks of 1,001 flags (at least four per array, the staging slot holding flags, column and
    selection), every bitmap at an odd bit offset so that chunks start inside a bitmap byte; the shorter arrays in chunks of 8"""
    from libflagstats_amd import _lib
    from libflagstats_amd import filter_where as fw
    extra = [Case(n, mq, "funnel" if (off + 8 - start // 2) % 8 else "bitmap", start, off, 1, 30, (0, 0x904), "random")
             for n, start, off in ((4097, 2, 13), (S + 1, 0, 7), (3 * S + 5, 14, 1), (63, 0, 13)) for mq in (False, True)]
    more = Laid(oracle_mod, extra, seed=99)
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        for lay, cases in ((laid, [c for c in laid.cases if c.n in SEAMS or c.n == 63]), (more, extra)):
            for c in cases:
                chunk = 1001 if c.n > 63 else 8
                assert c.n > 3 * chunk
                _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", chunk), "chunk_flags")
                ptr, qptr, sptr = lay.host_args(c)
                for mode in (STORE | SUPERSET, 0):
                    o = np.full(32, GARBAGE if mode & STORE else BIAS, dtype=np.uint64)
                    h = ctypes.c_uint64(GARBAGE if mode & STORE else SEL_BIAS)
                    rc = hip.FLAGSTATS_hip_u16_x64_filter_where(ptr, c.n, c.pred[0], c.pred[1], qptr, c.min_mapq, sptr, c.offset, c.sel_bits,
                                                                o.ctypes.data, ctypes.byref(h), mode)
                    assert rc == 0, (c.note, mode, err(hip))
                    assert np.array_equal(o, expect_row(c.want, mode)), (c.note, mode, o)
                    assert h.value == c.nsel + (0 if mode & STORE else SEL_BIAS), (c.note, mode)
        assert any(c.sel_bits == BITMAP and c.offset % 2 for c in extra)
        # the Python layer over the same chunks: a bitmap at an odd bit offset, then a boolean mask
        c = extra[-1 - 2]                          # 3 S + 5 flags with the column
        assert c.n == 3 * S + 5 and c.mq
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", 1001), "chunk_flags")
        plain, nsel = want_counters(oracle_mod, c.values, c.mask, 0, 0x904, c.q, 30)
        got, selected = fw.counters_filter_where(c.values, pack(c.mask, 13), exclude=0x904, mapq=c.q, min_mapq=30, packed=True, bit_offset=13)
        assert np.array_equal(got, plain) and selected == nsel == c.nsel
        got, selected = fw.counters_filter_where(c.values, c.mask, exclude=0x904, mapq=c.q, min_mapq=30, superset=True)
        assert np.array_equal(got, c.want) and selected == nsel
        d = fw.flagstats_filter_where(c.values, c.mask, exclude=0x904, mapq=c.q, min_mapq=30)
        assert d["n_values"] == nsel and int(d["failed"]["FQCFAIL"]) == int(plain[25])
        assert int(d["passed"]["mapped"]) == nsel - int(plain[2]) - int(plain[18])
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old


# ------------------------------------------------------------------ 3. a workgroup's rolling steps and its epochs
SIX = tuple((mq, form) for mq in (False, True) for form in FORMS)


@pytest.mark.parametrize("steps,grid", [(5, 2), (2 * 255 + 3, 1)])
def test_small_grids(hip, oracle_mod, steps, grid):
    """grid 2 over 5 fast steps: workgroup 0 runs the rolling step with a successor twice and then the final one, workgroup 1
    once; grid 1 over 2 * 255 + 3 fast steps: every wave flushes its epoch twice mid-launch.  All six forms, the array on a
    16-byte boundary so that every step is a fast one"""
    n = steps * S
    values = np.resize(np.random.RandomState(305).randint(0, 65536, 65_521).astype(np.uint16), n)
    mapq = np.resize(np.random.RandomState(306).randint(0, 61, 65_519).astype(np.uint8), n)
    mask = np.resize(np.random.RandomState(307).randint(0, 2, 65_537).astype(bool), n)
    t, q = dev16(values), dev8(mapq)
    assert t.data_ptr() % 16 == 0
    sels = {"bitmap": (dev8(pack(mask, 0)), 0, BITMAP), "funnel": (dev8(pack(mask, 3)), 3, BITMAP),
            "bytes": (dev8(mask.astype(np.uint8) * np.uint8(0x80)), 0, BYTES)}
    split = where_oracle.where_geometry(t.data_ptr(), n, 0, BITMAP, grid)
    assert split[2:6] == [steps, 0, steps, grid]
    rows = Rows()
    calls = []
    for mq, form in SIX:
        mn = 30 if mq else 0
        want, nsel = want_counters(oracle_mod, values, mask, 0x0001, 0x0804, mapq, mn, superset=True)
        assert 0 < nsel < mask.sum()
        for mode in (STORE | SUPERSET, 0):
            calls.append((rows.add(mode, want, nsel, (steps, grid, mq, form, mode)), mq, form, mn, mode))
    rows.upload()
    for k, mq, form, mn, mode in calls:
        d_sel, off, bits = sels[form]
        rc = hip.fsk_launch_filter_where(t.data_ptr(), n, 0x0001, 0x0804, q.data_ptr() if mq else None, mn, d_sel.data_ptr(), off, bits,
                                         rows.out(k), rows.selected(k), mode, grid, None)
        assert rc == 0, (rows.notes[k], rc)
    rows.check()


# ------------------------------------------------------------------ 4. forms of the result
def test_result_forms(hip, oracle_mod):
    """store against +=, two launches on two streams sharing d_out, superset, `selected` NULL, d_selected apart from and right
    behind d_out, the overlapping pair (zeros in the store form, nothing touched otherwise), n == 0"""
    import torch
    rng = np.random.RandomState(61)
    n = 2 * S + 77
    values, mapq = make_body(n, rng)
    mask = rng.randint(0, 2, n).astype(bool)
    t, q, m = dev16(values), dev8(mapq), torch.from_numpy(mask).cuda()
    bits = dev8(pack(mask, 5))
    plain, nsel = want_counters(oracle_mod, values, mask, 0x2, 0x904, mapq, 30)
    sup, _ = want_counters(oracle_mod, values, mask, 0x2, 0x904, mapq, 30, superset=True)
    assert 0 < nsel < n and not np.array_equal(plain, sup)
    entry = hip.FLAGSTATS_hip_device_u16_filter_where

    def run(out, sel, mode, d_sel=m, off=0, sb=BYTES, stream=None, nn=n, pred=(0x2, 0x904)):
        rc = entry(t.data_ptr() if nn else None, nn, pred[0], pred[1], q.data_ptr() if nn else None, 30, d_sel.data_ptr() if nn else None,
                   off, sb, out, sel, mode, stream)
        assert rc == 0, err(hip)

    words = torch.full((33,), GARBAGE, dtype=torch.int64, device="cuda")
    apart = torch.full((1,), GARBAGE, dtype=torch.int64, device="cuda")
    p = words.data_ptr()
    # store, d_selected right behind d_out; then += twice on top
    run(p, p + 256, STORE)
    run(p, p + 256, 0, bits, 5, BITMAP)
    run(p, p + 256, 0)
    torch.cuda.synchronize()
    assert np.array_equal(u64(words)[:32], 3 * plain) and int(u64(words)[32]) == 3 * nsel
    # store + superset with d_selected apart; `selected` NULL leaves the word behind the counters alone
    words.fill_(GARBAGE)
    run(p, apart.data_ptr(), STORE | SUPERSET, bits, 5, BITMAP)
    torch.cuda.synchronize()
    assert np.array_equal(u64(words)[:32], sup) and int(u64(apart)[0]) == nsel and int(u64(words)[32]) == GARBAGE
    words.fill_(GARBAGE)
    run(p, None, STORE | SUPERSET)
    run(p, None, SUPERSET)
    torch.cuda.synchronize()
    assert np.array_equal(u64(words)[:32], 2 * sup) and int(u64(words)[32]) == GARBAGE
    # two streams add into one pair
    words.zero_()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for st, (d_sel, off, sb) in zip(streams, ((bits, 5, BITMAP), (m, 0, BYTES))):
        run(p, p + 256, SUPERSET, d_sel, off, sb, ctypes.c_void_p(st.cuda_stream))
    for st in streams:
        st.synchronize()
    assert np.array_equal(u64(words)[:32], 2 * sup) and int(u64(words)[32]) == 2 * nsel
    # a bit both required and excluded: zeros in the store form, nothing touched otherwise (launcher and entry)
    words.fill_(BIAS)
    rc = hip.fsk_launch_filter_where(t.data_ptr(), n, 0x40, 0x40, q.data_ptr(), 30, m.data_ptr(), 0, BYTES, p, p + 256, 0, 3, None)
    assert rc == 0
    run(p, p + 256, SUPERSET, pred=(0x0140, 0x40))
    torch.cuda.synchronize()
    assert (u64(words) == BIAS).all()
    run(p, p + 256, STORE | SUPERSET, pred=(0x40, 0x40))
    torch.cuda.synchronize()
    assert not u64(words).any()
    # n == 0: += touches nothing, store writes zeros; NULL inputs are accepted
    words.fill_(BIAS)
    run(p, p + 256, 0, nn=0)
    torch.cuda.synchronize()
    assert (u64(words) == BIAS).all()
    run(p, p + 256, STORE, nn=0)
    torch.cuda.synchronize()
    assert not u64(words).any()
    for fn in (hip.FLAGSTATS_hip_u16_x64_filter_where, hip.FLAGSTATS_hip_device_u16_filter_where_sync):
        for sb in (BITMAP, BYTES):
            o = np.full(32, BIAS, dtype=np.uint64)
            h = ctypes.c_uint64(5)
            assert fn(None, 0, 1, 4, None, 30, None, 3, sb, o.ctypes.data, ctypes.byref(h), 0) == 0 and (o == BIAS).all() and h.value == 5
            assert fn(None, 0, 1, 4, None, 30, None, 3, sb, o.ctypes.data, ctypes.byref(h), STORE) == 0 and not o.any() and h.value == 0


# ------------------------------------------------------------------ 5. identities with the parents
@pytest.mark.parametrize("n", [4097, 3 * S + 5])
def test_identities_with_the_parents(hip, oracle_mod, n):
    """an all-set selection gives the filtered entry's result, the empty predicate the `where` entry's, both together the plain
    count -- each next to the oracle's"""
    import torch
    rng = np.random.RandomState(n)
    values, mapq = make_body(n, rng)
    mask = rng.randint(0, 2, n).astype(bool)
    slab = torch.full((8 + n + 8,), -1, dtype=torch.int16, device="cuda")
    slab[1:1 + n] = dev16(values)
    ptr = slab.data_ptr() + 2
    q = dev8(mapq)
    ones = np.ones(n, dtype=bool)
    sels = {(BITMAP, "set"): (dev8(pack(ones, 3)), 3), (BYTES, "set"): (dev8(ones.astype(np.uint8)), 0),
            (BITMAP, "mask"): (dev8(pack(mask, 3)), 3), (BYTES, "mask"): (dev8(mask.astype(np.uint8)), 0)}

    def ours(require, exclude, mn, sb, which):
        d_sel, off = sels[sb, which]
        o = np.zeros(32, dtype=np.uint64)
        h = ctypes.c_uint64(0)
        rc = hip.FLAGSTATS_hip_device_u16_filter_where_sync(ptr, n, require, exclude, q.data_ptr() if mn else None, mn, d_sel.data_ptr(), off, sb,
                                                            o.ctypes.data, ctypes.byref(h), STORE | SUPERSET)
        assert rc == 0, err(hip)
        return o, h.value

    for sb in (BITMAP, BYTES):
        for require, exclude, mn in ((0, 0x904, 0), (0x2, 0x904, 30), (0, 0, 129)):
            o, h = ctypes.c_uint64(0), None
            parent = np.zeros(32, dtype=np.uint64)
            assert hip.FLAGSTATS_hip_device_u16_filter_sync(ptr, n, require, exclude, q.data_ptr() if mn else None, mn, parent.ctypes.data,
                                                            ctypes.byref(o), STORE | SUPERSET) == 0, err(hip)
            got, selected = ours(require, exclude, mn, sb, "set")
            want, nsel = filter_oracle.want_counters(oracle_mod, values, require, exclude, mapq, mn, superset=True)
            assert np.array_equal(got, parent) and selected == o.value, (sb, require, exclude, mn)
            assert np.array_equal(got, want) and selected == nsel and 0 < nsel < n, (sb, require, exclude, mn)
        d_sel, off = sels[sb, "mask"]
        parent = np.zeros(32, dtype=np.uint64)
        o = ctypes.c_uint64(0)
        assert hip.FLAGSTATS_hip_device_u16_where_sync(ptr, n, d_sel.data_ptr(), off, sb, parent.ctypes.data, ctypes.byref(o),
                                                       STORE | SUPERSET) == 0, err(hip)
        got, selected = ours(0, 0, 0, sb, "mask")
        assert np.array_equal(got, parent) and selected == o.value == int(mask.sum()), sb
        assert np.array_equal(got, where_oracle.want_counters(oracle_mod, values, mask, superset=True)), sb
        plain = np.zeros(32, dtype=np.uint64)
        assert hip.FLAGSTATS_hip_device_u16_sync(ptr, n, plain.ctypes.data) == 0, err(hip)
        o = np.zeros(32, dtype=np.uint64)
        h = ctypes.c_uint64(0)
        d_sel, off = sels[sb, "set"]
        assert hip.FLAGSTATS_hip_device_u16_filter_where_sync(ptr, n, 0, 0, None, 0, d_sel.data_ptr(), off, sb, o.ctypes.data, ctypes.byref(h),
                                                              STORE) == 0, err(hip)
        assert np.array_equal(o, plain) and h.value == n, sb
        assert np.array_equal(o, oracle_mod.flagstat_c(values).astype(np.uint64)), sb


# ------------------------------------------------------------------ 6. the torch layer
@pytest.mark.parametrize("packed", [False, True])
def test_torch_layer_on_a_side_stream(hip, oracle_mod, packed):
    """count_torch_filter_where on a stream that is not the default one, with `out` / `selected` supplied (store, then += on top)
    and with them omitted"""
    import torch
    from libflagstats_amd import filter_where as fw
    rng = np.random.RandomState(17)
    n = S + 4097
    values, mapq = make_body(n, rng)
    mask = rng.randint(0, 3, n) > 0
    want, nsel = want_counters(oracle_mod, values, mask, 0, 0x904, mapq, 30)
    sup, _ = want_counters(oracle_mod, values, mask, 0, 0x904, mapq, 30, superset=True)
    t, q = dev16(values), dev8(mapq)
    where = dev8(pack(mask, 13)) if packed else torch.from_numpy(mask).cuda()
    kw = dict(exclude=0x904, mapq=q, min_mapq=30, packed=packed, bit_offset=13 if packed else 0)
    out = torch.full((32,), GARBAGE, dtype=torch.int64, device="cuda")
    selected = torch.full((1,), GARBAGE, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream() == s and s != torch.cuda.default_stream()
        o, h = fw.count_torch_filter_where(t, where, out=out, selected=selected, store=True, **kw)
        assert o is out and h is selected
        fw.count_torch_filter_where(t, where, out=out, selected=selected, **kw)
        o2, h2 = fw.count_torch_filter_where(t, where, superset=True, **kw)
        o3, h3 = fw.count_torch_filter_where(t.view(torch.uint16), where, store=True, **kw)
    s.synchronize()
    assert np.array_equal(u64(out), 2 * want) and int(u64(selected)[0]) == 2 * nsel
    assert o2.dtype == torch.int64 and tuple(o2.shape) == (32,) and tuple(h2.shape) == (1,) and o2.device == t.device
    assert np.array_equal(u64(o2), sup) and int(u64(h2)[0]) == nsel
    assert np.array_equal(u64(o3), want) and int(u64(h3)[0]) == nsel
    # no elements
    o4, h4 = fw.count_torch_filter_where(t[:0], where[:0], exclude=0x904, mapq=q[:0], min_mapq=30, packed=packed)
    torch.cuda.synchronize()
    assert not u64(o4).any() and int(u64(h4)[0]) == 0


# ------------------------------------------------------------------ 7. refusals that need a device
def test_device_dependent_refusals(hip):
    """what the C entries and the Python layer can refuse only with a device at hand: the union of the parents' refusals, in
    their texts, before anything is launched; the outputs stay as they were"""
    import torch
    from libflagstats_amd import filter_where as fw
    n = 4096
    t = torch.zeros(n + 8, dtype=torch.int16, device="cuda")
    q = torch.full((n + 8,), 60, dtype=torch.uint8, device="cuda")
    m = torch.ones(n + 8, dtype=torch.bool, device="cuda")
    out = torch.full((32,), BIAS, dtype=torch.int64, device="cuda")
    sel = torch.full((1,), SEL_BIAS, dtype=torch.int64, device="cuda")
    h_out = np.full(32, BIAS, dtype=np.uint64)
    h_sel = ctypes.c_uint64(SEL_BIAS)
    host16 = np.zeros(n + 8, dtype=np.uint16)
    host8 = np.full(n + 8, 60, dtype=np.uint8)

    def untouched(what):
        torch.cuda.synchronize()
        assert (out == BIAS).all() and int(u64(sel)[0]) == SEL_BIAS, what
        assert (h_out == BIAS).all() and h_sel.value == SEL_BIAS, what

    def refused(what, text, d_array=t.data_ptr(), n_=n, require=0, exclude=0x904, d_mapq=q.data_ptr(), mn=30, d_sel=m.data_ptr(), off=0,
                sb=BYTES, flags=0, counters=True, forms=("device", "sync", "host")):
        for form in forms:
            if form == "device":
                rc = hip.FLAGSTATS_hip_device_u16_filter_where(d_array, n_, require, exclude, d_mapq, mn, d_sel, off, sb,
                                                               out.data_ptr() if counters else None, sel.data_ptr(), flags, None)
            elif form == "sync":
                rc = hip.FLAGSTATS_hip_device_u16_filter_where_sync(d_array, n_, require, exclude, d_mapq, mn, d_sel, off, sb,
                                                                    h_out.ctypes.data if counters else None, ctypes.byref(h_sel), flags)
            else:
                src = host16.ctypes.data + (d_array - t.data_ptr()) if d_array else None
                rc = hip.FLAGSTATS_hip_u16_x64_filter_where(src, n_, require, exclude, host8.ctypes.data if d_mapq else None, mn,
                                                            host8.ctypes.data if d_sel else None, off, sb,
                                                            h_out.ctypes.data if counters else None, ctypes.byref(h_sel), flags)
            assert rc != 0, (what, form)
            assert text in err(hip), (what, form, err(hip))
        untouched(what)

    refused("require above 16 bits", "require must be a 16-bit FLAG mask", require=0x10000)
    refused("exclude above 16 bits", "exclude must be a 16-bit FLAG mask", exclude=0x10000)
    refused("min_mapq above a byte", "min_mapq must be at most 255", mn=256)
    refused("sel_bits", "sel_bits must be 1 (an LSB-first bitmap) or 8 (one byte per element)", sb=2)
    refused("NULL mapq", "NULL mapq with min_mapq > 0 and n > 0", d_mapq=None)
    refused("NULL selection", "NULL selection with n > 0", d_sel=None)
    refused("NULL array", "NULL array with n > 0", d_array=None)
    refused("an odd array address", "2-byte aligned", d_array=t.data_ptr() + 1)
    refused("an extra flag bit", "no other bits", flags=4)
    refused("NULL counters", "NULL counters", counters=False)
    refused("n * 2 is no size", "n * 2 is not a size", n_=1 << 63)
    refused("sel_offset + n is no index", "sel_offset + n is not an index", off=(1 << 64) - 64)
    refused("a wave's totals", "a wave's uint32 totals", n_=1 << 62, mn=0, d_mapq=None, forms=("device", "sync"))
    # the selection or the column somewhere else than the array
    for args, name in (((q.data_ptr(), 30, host8.ctypes.data), "d_sel"), ((host8.ctypes.data, 30, m.data_ptr()), "d_mapq")):
        rc = hip.FLAGSTATS_hip_device_u16_filter_where(t.data_ptr(), n, 0, 0x904, args[0], args[1], args[2], 0, BYTES, out.data_ptr(),
                                                       sel.data_ptr(), 0, None)
        assert rc != 0 and name in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_u16_filter_where_sync(t.data_ptr(), n, 0, 0x904, args[0], args[1], args[2], 0, BYTES, h_out.ctypes.data,
                                                            ctypes.byref(h_sel), 0)
        assert rc != 0 and name in err(hip), err(hip)
    with pytest.raises(ValueError, match=r"where must live on t's device \(cuda:0\), not on cpu"):
        fw.count_torch_filter_where(t, torch.ones(n + 8, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"mapq must live on t's device \(cuda:0\), not on cpu"):
        fw.count_torch_filter_where(t, m, mapq=torch.zeros(n + 8, dtype=torch.uint8), min_mapq=30)
    with pytest.raises(ValueError, match=r"out must live on t's device \(cuda:0\), not on cpu"):
        fw.count_torch_filter_where(t, m, out=torch.zeros(32, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"selected must live on t's device \(cuda:0\), not on cpu"):
        fw.count_torch_filter_where(t, m, selected=torch.zeros(1, dtype=torch.int64))
    untouched("inputs elsewhere")
    # host pointers as d_out / d_selected
    rc = hip.FLAGSTATS_hip_device_u16_filter_where(t.data_ptr(), n, 0, 0x904, q.data_ptr(), 30, m.data_ptr(), 0, BYTES, h_out.ctypes.data,
                                                   sel.data_ptr(), 0, None)
    assert rc != 0 and "d_out" in err(hip), err(hip)
    rc = hip.FLAGSTATS_hip_device_u16_filter_where(t.data_ptr(), n, 0, 0x904, q.data_ptr(), 30, m.data_ptr(), 0, BYTES, out.data_ptr(),
                                                   ctypes.addressof(h_sel), 0, None)
    assert rc != 0 and "d_selected" in err(hip), err(hip)
    untouched("host pointers")
    # extents: the column and the selection one byte short of what the call reads of them, an array one flag short, counters 8
    # bytes short; a bitmap is measured in the bytes that hold the n bits
    nbytes = 2 << 20
    raw = hip.FLAGSTATS_hip_device_alloc(nbytes)
    big = torch.zeros(nbytes + 8, dtype=torch.int16, device="cuda")
    big8 = torch.zeros(nbytes + 8, dtype=torch.uint8, device="cuda")
    assert raw
    try:
        assert hip.FLAGSTATS_hip_memcpy_h2d(raw, np.zeros(nbytes, dtype=np.uint8).ctypes.data, nbytes) == 0
        entry, sync = hip.FLAGSTATS_hip_device_u16_filter_where, hip.FLAGSTATS_hip_device_u16_filter_where_sync
        for d_mapq, d_sel, off, sb, nn, name in ((raw, big8.data_ptr(), 0, BYTES, nbytes + 1, "d_mapq"),
                                                 (big8.data_ptr(), raw, 0, BYTES, nbytes + 1, "d_sel"),
                                                 (big8.data_ptr(), raw, 1, BYTES, nbytes, "d_sel"),
                                                 (big8.data_ptr(), raw, 8 * nbytes - 4096 + 1, BITMAP, 4096, "d_sel")):
            rc = entry(big.data_ptr(), nn, 0, 0x904, d_mapq, 30, d_sel, off, sb, out.data_ptr(), sel.data_ptr(), STORE, None)
            assert rc != 0 and name in err(hip) and "1 bytes short" in err(hip), (name, err(hip))
            rc = sync(big.data_ptr(), nn, 0, 0x904, d_mapq, 30, d_sel, off, sb, h_out.ctypes.data, ctypes.byref(h_sel), STORE)
            assert rc != 0 and name in err(hip) and "1 bytes short" in err(hip), (name, err(hip))
        untouched("input extents")
        # the same allocations hold what a call one element shorter reads, and a column that is not read is not looked at
        for d_mapq, mn, d_sel, off, sb, nn in ((raw, 30, raw, 0, BYTES, nbytes), (raw, 0, big8.data_ptr(), 0, BYTES, nbytes + 1),
                                               (big8.data_ptr(), 30, raw, 8 * nbytes - 4096, BITMAP, 4096)):
            o = np.full(32, BIAS, dtype=np.uint64)
            h = ctypes.c_uint64(SEL_BIAS)
            assert sync(big.data_ptr(), nn, 0, 0x904, d_mapq, mn, d_sel, off, sb, o.ctypes.data, ctypes.byref(h), STORE) == 0, err(hip)
            assert not o.any() and h.value == 0           # flags 0 count nothing; MAPQ 0 < 30 or nothing selected
        rc = entry(raw, nbytes // 2 + 1, 0, 0x904, None, 0, big8.data_ptr(), 0, BYTES, out.data_ptr(), sel.data_ptr(), STORE, None)
        assert rc != 0 and "d_array" in err(hip) and "2 bytes short" in err(hip), err(hip)
        rc = entry(t.data_ptr(), n, 0, 0x904, q.data_ptr(), 30, m.data_ptr(), 0, BYTES, raw + nbytes - 248, sel.data_ptr(), 0, None)
        assert rc != 0 and "d_out" in err(hip) and "8 bytes short" in err(hip), err(hip)
    finally:
        hip.FLAGSTATS_hip_device_free(raw)
    untouched("extents")
    # the launcher itself: the union of what the parents' launchers refuse -- nothing queued
    words = torch.full((33,), BIAS, dtype=torch.int64, device="cuda")
    p = words.data_ptr()
    launch = hip.fsk_launch_filter_where
    assert launch(t.data_ptr(), 8, 0, 0x904, q.data_ptr(), 30, m.data_ptr(), 0, BYTES, p, p + 256, 4, 1, None) != 0
    assert launch(t.data_ptr(), 8, 0, 0x904, q.data_ptr(), 30, m.data_ptr(), 0, BYTES, p, p + 256, 0, 0, None) != 0
    assert launch(t.data_ptr(), 1 << 35, 0, 0x904, None, 0, m.data_ptr(), 0, BYTES, p, p + 256, STORE, 1, None) != 0
    assert launch(t.data_ptr(), 8, 0x10000, 0, None, 0, m.data_ptr(), 0, BYTES, p, p + 256, STORE, 1, None) != 0
    assert launch(t.data_ptr(), 8, 0, 0x10000, None, 0, m.data_ptr(), 0, BYTES, p, p + 256, STORE, 1, None) != 0
    assert launch(t.data_ptr(), 8, 0, 0, None, 30, m.data_ptr(), 0, BYTES, p, p + 256, STORE, 1, None) != 0
    assert launch(t.data_ptr(), 8, 0, 0, q.data_ptr(), 256, m.data_ptr(), 0, BYTES, p, p + 256, STORE, 1, None) != 0
    assert launch(t.data_ptr(), 8, 0, 0, None, 0, None, 0, BYTES, p, p + 256, STORE, 1, None) != 0
    assert launch(t.data_ptr(), 8, 0, 0, None, 0, m.data_ptr(), 0, 2, p, p + 256, STORE, 1, None) != 0
    assert launch(t.data_ptr() + 1, 8, 0, 0, None, 0, m.data_ptr(), 0, BYTES, p, p + 256, STORE, 1, None) != 0
    assert launch(t.data_ptr(), 8, 0, 0, None, 0, m.data_ptr(), (1 << 64) - 64, BITMAP, p, p + 256, STORE, 1, None) != 0
    assert launch(t.data_ptr(), 8, 0, 0, None, 0, m.data_ptr(), 0, BYTES, None, p + 256, STORE, 1, None) != 0
    torch.cuda.synchronize()
    assert (words == BIAS).all()
