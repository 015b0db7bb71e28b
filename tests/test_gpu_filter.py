"""The filtered flagstat on the MI355X: fsk::flagstat_count_filter with and without a MAPQ column, the three C entries and
libflagstats_amd/filter.py.

Expected counters never come from the code under test: filter_oracle.want_counters is oracle.flagstat_c of values[mask] (superset
slots from oracle.samtools_counts and the definition) under the numpy mask of the predicate; the expected `selected` is
int(mask.sum())."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import where_oracle  # noqa: E402
from filter_oracle import filter_mask, want_counters  # noqa: E402
from test_gpu_where import BIAS, BYTE_ALIGNMENTS, GARBAGE, LENGTHS, POSITIONS, SEL_BIAS, STORE, SUPERSET, Rows, S, dev8, dev16, err, expect_row, u64  # noqa: E402,E501

pytestmark = pytest.mark.gpu

SINGLE_BITS = tuple(1 << b for b in range(16))
PREDICATES = ([(bit, 0) for bit in SINGLE_BITS] + [(0, bit) for bit in SINGLE_BITS]
              + [(0, 0x904), (0x2, 0x900), (0x1, 0xF04), (0x0101, 0x8080), (0xFFFF, 0), (0, 0xFFFF), (0x0040, 0x0040), (0, 0)])


# ------------------------------------------------------------------ 1. every value under every kind of predicate
def test_every_value_under_every_kind_of_predicate(hip, oracle_mod):
    """0..65535 once each, shuffled (4 steps), under every single required bit, every single excluded bit, the samtools filters,
    predicates on both byte planes on both sides, everything required, everything excluded (only the value 0 passes: no
    counter, selected == 1), an overlapping pair (nothing passes, the += rows stay as they are) and the empty predicate (the
    plain count) -- store + superset form and += form over bias words, through the device entry, the _sync form and the host
    form"""
    import torch
    from libflagstats_amd import filter as flt
    values = np.random.RandomState(2025).permutation(65536).astype(np.uint16)
    t = dev16(values)
    wants = {p: want_counters(oracle_mod, values, p[0], p[1], superset=True) for p in PREDICATES}
    assert wants[0, 0xFFFF][1] == 1 and not wants[0, 0xFFFF][0][1:9].any() and not wants[0, 0xFFFF][0][10:].any()
    assert wants[0x0040, 0x0040][1] == 0 and not wants[0x0040, 0x0040][0].any()
    assert wants[0, 0][1] == 65536 and wants[0xFFFF, 0][1] == 1
    rows = Rows()
    plan = [(p, mode, rows.add(mode, wants[p][0], wants[p][1], ("device", p, mode))) for p in PREDICATES for mode in (STORE | SUPERSET, 0)]
    rows.upload()
    for (require, exclude), mode, k in plan:
        rc = hip.FLAGSTATS_hip_device_u16_filter(t.data_ptr(), 65536, require, exclude, None, 0, rows.out(k), rows.selected(k), mode, None)
        assert rc == 0, (require, exclude, mode, err(hip))
    rows.check()
    for name, entry, src in (("sync", hip.FLAGSTATS_hip_device_u16_filter_sync, t.data_ptr()),
                             ("host", hip.FLAGSTATS_hip_u16_x64_filter, values.ctypes.data)):
        for p in PREDICATES:
            for mode in (STORE | SUPERSET, 0):
                o = np.full(32, GARBAGE if mode & STORE else BIAS, dtype=np.uint64)
                h = ctypes.c_uint64(GARBAGE if mode & STORE else SEL_BIAS)
                assert entry(src, 65536, p[0], p[1], None, 0, o.ctypes.data, ctypes.byref(h), mode) == 0, (name, p, mode, err(hip))
                assert np.array_equal(o, expect_row(wants[p][0], mode)), (name, p, mode, o)
                assert h.value == wants[p][1] + (0 if mode & STORE else SEL_BIAS), (name, p, mode)
    # the empty predicate is the plain count of the same tensor
    plain = np.zeros(32, dtype=np.uint64)
    assert hip.FLAGSTATS_hip_device_u16_sync(t.data_ptr(), 65536, plain.ctypes.data) == 0, err(hip)
    got, selected = flt.count_device_ptr_filter(t.data_ptr(), 65536)
    assert np.array_equal(got, plain) and selected == 65536 and got.dtype == np.uint64
    o, s = flt.count_torch_filter(t, store=True)
    torch.cuda.synchronize()
    assert o.dtype == torch.int64 and tuple(o.shape) == (32,) and tuple(s.shape) == (1,) and o.device == t.device
    assert np.array_equal(u64(o), plain) and int(u64(s)[0]) == 65536
    # the Python layer under samtools' usual filter, and its dict
    want, nsel = want_counters(oracle_mod, values, 0x2, 0x904)
    got, selected = flt.counters_filter(values, require=0x2, exclude=0x904)
    assert np.array_equal(got, want) and selected == nsel
    d = flt.flagstats_filter(values, require=0x2, exclude=0x904)
    assert d["n_values"] == nsel and int(d["failed"]["FQCFAIL"]) == int(want[25])
    assert int(d["passed"]["mapped"]) == nsel - int(want[2]) - int(want[18])


# ------------------------------------------------------------------ 2. lengths, phases, MAPQ alignments
PRED_ONE_PLANE, PRED_BOTH_PLANES = (0x0001, 0x0004), (0x0041, 0x0900)


def test_lengths_phases_mapq_alignments(hip, oracle_mod):
    """every length around nothing, a vector, a wave's line and one and two steps x every array phase x {no MAPQ, MAPQ at byte
    alignments 0, 1, 3, 8, 15} x two predicates (one on the low byte plane, one on both).  The array sits in a slab whose
    surrounding 64 flags are 0xFFFF & ~exclude (they pass), the MAPQ in a slab whose surrounding bytes are 0xFF (they pass every
    threshold): one element read outside [0, n) changes `selected` and the counters.  Through fsk_launch_filter at grids 1, 2,
    3 and the public device entry, store form over garbage and += over bias words."""
    import torch
    rng = np.random.RandomState(43)
    nmax = LENGTHS[-1]
    body = rng.randint(0, 65536, nmax).astype(np.uint16)
    forced = rng.randint(0, 100, nmax) < 55       # these pass both predicates
    body[forced] = (body[forced] & np.uint16(~0x0904 & 0xFFFF)) | np.uint16(0x0041)
    mapq = rng.randint(15, 60, nmax).astype(np.uint8)   # two thirds reach 30
    preds = (PRED_ONE_PLANE, PRED_BOTH_PLANES)
    for p in preds:
        for q, mn in ((None, 0), (mapq, 30)):
            for n in LENGTHS:
                if n >= 63:
                    frac = filter_mask(body[:n], p[0], p[1], None if q is None else q[:n], mn).mean()
                    assert 0.25 <= frac <= 0.75, (p, mn, n, frac)
    wants = {(p, mn, n): want_counters(oracle_mod, body[:n], p[0], p[1], mapq[:n], mn, superset=True)
             for p in preds for mn in (0, 30) for n in LENGTHS}
    arrays, a_at = [], {}
    pos = 0
    for p in preds:
        for n in LENGTHS:
            for phase in range(8):
                region = np.full((64 + 8 + n + 64 + 7) // 8 * 8, 0xFFFF & ~p[1], dtype=np.uint16)
                region[64 + phase:64 + phase + n] = body[:n]
                a_at[p, n, phase] = pos + 64 + phase
                arrays.append(region)
                pos += region.size
    cols, q_at = [], {}
    pos = 0
    for n in LENGTHS:
        for align in BYTE_ALIGNMENTS:
            region = np.full((16 + 16 + n + 16 + 15) // 16 * 16, 0xFF, dtype=np.uint8)
            region[16 + align:16 + align + n] = mapq[:n]
            q_at[n, align] = pos + 16 + align
            cols.append(region)
            pos += region.size
    d_arrays = dev16(np.concatenate(arrays))
    d_cols = dev8(np.concatenate(cols))
    assert d_arrays.data_ptr() % 16 == 0 and d_cols.data_ptr() % 16 == 0
    rows = Rows()
    calls = []
    for p in preds:
        for n in LENGTHS:
            for phase in range(8):
                ptr = d_arrays.data_ptr() + 2 * a_at[p, n, phase]
                assert ptr % 16 == 2 * phase
                for align in (None,) + BYTE_ALIGNMENTS:
                    qptr = None if align is None else d_cols.data_ptr() + q_at[n, align]
                    mn = 0 if align is None else 30
                    assert align is None or qptr % 16 == align
                    want, nsel = wants[p, mn, n]
                    for grid in (1, 2, 3, None):          # None: the public device entry
                        for mode in (STORE | SUPERSET, 0):
                            k = rows.add(mode, want, nsel, (p, n, phase, align, grid, mode))
                            calls.append((k, ptr, n, p, qptr, mn, mode, grid))
    rows.upload()
    for k, ptr, n, p, qptr, mn, mode, grid in calls:
        if grid is None:
            rc = hip.FLAGSTATS_hip_device_u16_filter(ptr if n else None, n, p[0], p[1], qptr if n else None, mn, rows.out(k),
                                                     rows.selected(k), mode, None)
            assert rc == 0, (rows.notes[k], err(hip))
        else:
            rc = hip.fsk_launch_filter(ptr if n else None, n, p[0], p[1], qptr if n else None, mn, rows.out(k), rows.selected(k), mode,
                                       grid, None)
            assert rc == 0, (rows.notes[k], rc)
    rows.check()


# ------------------------------------------------------------------ 3. which MAPQ byte belongs to which flag
@pytest.mark.parametrize("phase,align", [(0, 0), (5, 3)])
def test_which_mapq_byte_belongs_to_which_flag(hip, oracle_mod, phase, align):
    """n = 2 S flags that all pass (0x0001, 0x0900); array[p] = 0x0041 between two 0x0081.  MAPQ 0 everywhere and 60 at p alone
    gives the row of one 0x0041; 60 everywhere and 0 at p gives the row of the array without it"""
    import torch
    n = 2 * S
    require, exclude, background = 0x0001, 0x0900, 0xFFFF & ~0x0900
    one, _ = want_counters(oracle_mod, np.array([0x0041], dtype=np.uint16), require, exclude, superset=True)
    slab = torch.from_numpy(np.full(64 + 8 + n + 64, background, dtype=np.uint16).view(np.int16)).cuda()
    arr = slab[64 + phase:64 + phase + n]
    assert arr.data_ptr() % 16 == 2 * phase
    col = torch.full((16 + 16 + n + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    q = col[16 + align:16 + align + n]
    assert q.data_ptr() % 16 == align
    host = np.full(n, background, dtype=np.uint16)
    near, there = np.array([0x0081], dtype=np.uint16).view(np.int16)[0], np.array([0x0041], dtype=np.uint16).view(np.int16)[0]
    rows = Rows()
    plan = []
    for p in POSITIONS:
        v = host.copy()
        v[p] = 0x0041
        v[max(p - 1, 0):p] = 0x0081
        v[p + 1:p + 2] = 0x0081
        hot = np.zeros(n, dtype=bool)
        hot[p] = True
        assert filter_mask(v, require, exclude).all()
        plan.append((p, rows.add(STORE | SUPERSET, one, 1, ("alone", phase, align, p)),
                     rows.add(STORE | SUPERSET, where_oracle.want_counters(oracle_mod, v, ~hot, superset=True), n - 1, ("all but", phase, align, p))))
    rows.upload()
    for p, k_alone, k_rest in plan:
        arr[p] = int(there)
        if p > 0:
            arr[p - 1] = int(near)
        if p + 1 < n:
            arr[p + 1] = int(near)
        for k, everywhere, at_p in ((k_alone, 0, 60), (k_rest, 60, 0)):
            q.fill_(everywhere)
            q[p] = at_p
            rc = hip.fsk_launch_filter(arr.data_ptr(), n, require, exclude, q.data_ptr(), 30, rows.out(k), rows.selected(k), STORE | SUPERSET, 3, None)
            assert rc == 0, rc
        arr[max(p - 1, 0):p + 2] = int(np.array([background], dtype=np.uint16).view(np.int16)[0])
    rows.check()


# ------------------------------------------------------------------ 4. every MAPQ value against the thresholds
THRESHOLDS = (1, 29, 30, 127, 128, 129, 254, 255)
AROUND = np.array([0, 1, 2, 28, 29, 30, 31, 126, 127, 128, 129, 130, 253, 254, 255], dtype=np.uint8)


@pytest.mark.parametrize("n", [S + 100, 2 * S + 100])
def test_every_mapq_value_against_the_thresholds(hip, oracle_mod, n):
    """n flags one flag into a 16-byte line, all 256 MAPQ values, the thresholds on both sides of every carry the byte-wise
    compare could get wrong.  S + 100 flags are a head edge step and a tail edge step (the guarded loaders); 2 S + 100 put a
    fast step between them, and every MAPQ value occurs in it.  Threshold 0 runs with a NULL column and selects everything, 256
    is refused"""
    import torch
    from steps_oracle import StepSplit
    rng = np.random.RandomState(29)
    values = rng.randint(0, 65536, n).astype(np.uint16)
    mapq = rng.randint(0, 256, n).astype(np.uint8)
    mapq[:512] = np.tile(np.arange(256, dtype=np.uint8), 2)          # every value in the head edge step ...
    mapq[-90:] = np.resize(AROUND, 90)                                # ... and the values next to every threshold in the tail's
    split = StepSplit(2, n, 1)
    assert split.head_edge and split.tail_edge and split.fast_end - split.fast_begin == (n - 100) // S - 1
    assert set(mapq.tolist()) == set(range(256)) and set(mapq[:S - 1].tolist()) == set(range(256))
    if n > 2 * S:
        assert set(mapq[S - 1:2 * S - 1].tolist()) == set(range(256))    # the fast step's elements
    slab = torch.full((8 + n + 8,), -1, dtype=torch.int16, device="cuda")
    slab[1:1 + n] = dev16(values)
    ptr = slab.data_ptr() + 2
    assert ptr % 16 == 2
    col = torch.full((16 + n + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    col[16 + 5:16 + 5 + n] = dev8(mapq)
    qptr = col.data_ptr() + 16 + 5
    rows = Rows()
    calls = []
    for require, exclude in ((0, 0), (0, 0x904)):
        for mn in THRESHOLDS:
            want, nsel = want_counters(oracle_mod, values, require, exclude, mapq, mn, superset=True)
            assert nsel == int((filter_mask(values, require, exclude) & (mapq.astype(np.int64) >= mn)).sum()) and 0 < nsel < n
            for mode in (STORE | SUPERSET, 0):
                for grid in (1, None):
                    calls.append((rows.add(mode, want, nsel, (require, exclude, mn, mode, grid)), require, exclude, qptr, mn, mode, grid))
        want, nsel = want_counters(oracle_mod, values, require, exclude, None, 0, superset=True)
        assert (require, exclude) != (0, 0) or nsel == n
        calls.append((rows.add(STORE | SUPERSET, want, nsel, (require, exclude, 0, "NULL column")), require, exclude, None, 0, STORE | SUPERSET, None))
    k_refused = rows.add(0, np.zeros(32, dtype=np.uint64), 0, "threshold 256")
    rows.upload()
    for k, require, exclude, q, mn, mode, grid in calls:
        if grid is None:
            assert hip.FLAGSTATS_hip_device_u16_filter(ptr, n, require, exclude, q, mn, rows.out(k), rows.selected(k), mode, None) == 0, err(hip)
        else:
            assert hip.fsk_launch_filter(ptr, n, require, exclude, q, mn, rows.out(k), rows.selected(k), mode, grid, None) == 0
    assert hip.FLAGSTATS_hip_device_u16_filter(ptr, n, 0, 0, qptr, 256, rows.out(k_refused), rows.selected(k_refused), 0, None) != 0
    assert "min_mapq must be at most 255" in err(hip)
    assert hip.fsk_launch_filter(ptr, n, 0, 0, qptr, 256, rows.out(k_refused), rows.selected(k_refused), 0, 1, None) != 0
    rows.check()


# ------------------------------------------------------------------ 5. epochs
@pytest.mark.parametrize("min_mapq", [0, 30])
def test_epochs(hip, oracle_mod, min_mapq):
    """one workgroup over 258 S + 3 flags: 258 fast steps and a tail edge step, so every wave passes its staggered first flush
    (after 255, 191, 127 and 63 pushes) and wave 0 a full epoch of 255 steps"""
    import torch
    n = 258 * S + 3
    pattern = np.random.RandomState(305).randint(0, 65536, 65_521).astype(np.uint16)
    values = np.resize(pattern, n)
    mapq = np.resize(np.random.RandomState(306).randint(0, 61, 65_519).astype(np.uint8), n)
    want, nsel = want_counters(oracle_mod, values, 0x0001, 0x0804, mapq, min_mapq, superset=True)
    assert 0 < nsel < n
    t = dev16(values)
    q = dev8(mapq)
    assert t.data_ptr() % 16 == 0
    rows = Rows()
    ks = [rows.add(mode, want, nsel, (min_mapq, mode)) for mode in (STORE | SUPERSET, 0)]
    rows.upload()
    for k in ks:
        rc = hip.fsk_launch_filter(t.data_ptr(), n, 0x0001, 0x0804, q.data_ptr() if min_mapq else None, min_mapq, rows.out(k),
                                   rows.selected(k), rows.modes[k], 1, None)
        assert rc == 0, rc
    rows.check()


# ------------------------------------------------------------------ 6. atomics
def test_three_streams_add_into_one_pair(hip, oracle_mod):
    import torch
    from libflagstats_amd import filter as flt
    rng = np.random.RandomState(73)
    out = torch.zeros(32, dtype=torch.int64, device="cuda")
    selected = torch.zeros(1, dtype=torch.int64, device="cuda")
    total, total_sel = np.zeros(32, dtype=np.uint64), 0
    inputs = []
    for n, require, exclude, mn in ((40 * S + 11, 0, 0x904, 30), (37 * S + 5, 0x2, 0x900, 0), (43 * S - 3, 0x0101, 0x8080, 200)):
        values = rng.randint(0, 65536, n).astype(np.uint16)
        mapq = rng.randint(0, 256, n).astype(np.uint8)
        want, nsel = want_counters(oracle_mod, values, require, exclude, mapq, mn, superset=True)
        assert nsel > 0
        total += want
        total_sel += nsel
        inputs.append((dev16(values), require, exclude, dev8(mapq) if mn else None, mn))
    streams = [torch.cuda.Stream() for _ in inputs]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    for st, (t, require, exclude, q, mn) in zip(streams, inputs):
        with torch.cuda.stream(st):
            flt.count_torch_filter(t, require=require, exclude=exclude, mapq=q, min_mapq=mn, out=out, selected=selected, superset=True)
    for st in streams:
        st.synchronize()
    assert np.array_equal(u64(out), total) and int(u64(selected)[0]) == total_sel


# ------------------------------------------------------------------ 7. host form across chunks
def test_host_form_across_chunks(hip, oracle_mod):
    """chunks of 8,192 flags, five of them and a ragged tail, with and without the MAPQ column"""
    from libflagstats_amd import _lib
    from libflagstats_amd import filter as flt
    n = 5 * 8192 + 77
    rng = np.random.RandomState(89)
    values = rng.randint(0, 65536, n).astype(np.uint16)
    mapq = rng.randint(0, 60, n).astype(np.uint8)
    require, exclude = 0x0001, 0x0804
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", 8192), "chunk_flags")
        for q, mn in ((None, 0), (mapq, 30)):
            wants = {sup: want_counters(oracle_mod, values, require, exclude, q, mn, superset=bool(sup)) for sup in (0, SUPERSET)}
            nsel = wants[0][1]
            assert 0 < nsel < n
            got, selected = flt.counters_filter(values, require, exclude, mapq=q, min_mapq=mn)
            assert np.array_equal(got, wants[0][0]) and selected == nsel, mn
            got, selected = flt.counters_filter(values, require, exclude, mapq=q, min_mapq=mn, superset=True)
            assert np.array_equal(got, wants[SUPERSET][0]) and selected == nsel, (mn, "superset")
            for flags in (0, SUPERSET):                  # += over bias words
                o = np.full(32, BIAS, dtype=np.uint64)
                h = ctypes.c_uint64(SEL_BIAS)
                rc = hip.FLAGSTATS_hip_u16_x64_filter(values.ctypes.data, n, require, exclude, q.ctypes.data if mn else None, mn,
                                                      o.ctypes.data, ctypes.byref(h), flags)
                assert rc == 0, err(hip)
                assert np.array_equal(o, expect_row(wants[SUPERSET][0], flags)) and h.value == SEL_BIAS + nsel, (mn, flags)
            # one chunk only (a single staging slot), from an odd host address
            got, selected = flt.counters_filter(values[1:100], require, exclude, mapq=None if q is None else q[1:100], min_mapq=mn)
            want, nsel = want_counters(oracle_mod, values[1:100], require, exclude, None if q is None else q[1:100], mn)
            assert np.array_equal(got, want) and selected == nsel
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old
    # n == 0: += touches nothing, store writes zeros; NULL pointers are accepted
    for entry in (hip.FLAGSTATS_hip_u16_x64_filter, hip.FLAGSTATS_hip_device_u16_filter_sync):
        for mn in (0, 30):
            o = np.full(32, BIAS, dtype=np.uint64)
            h = ctypes.c_uint64(5)
            assert entry(None, 0, 1, 4, None, mn, o.ctypes.data, ctypes.byref(h), 0) == 0 and (o == BIAS).all() and h.value == 5
            assert entry(None, 0, 1, 4, None, mn, o.ctypes.data, ctypes.byref(h), STORE) == 0 and not o.any() and h.value == 0
    got, selected = flt.counters_filter(values[:0], 1, 4, mapq=mapq[:0], min_mapq=30)
    assert not got.any() and selected == 0
    got, selected = flt.count_device_ptr_filter(0, 0, 1, 4)
    assert not got.any() and selected == 0


# ------------------------------------------------------------------ 8. refusals that need a device
def test_device_dependent_refusals(hip):
    """what the C entries and the Python layer can refuse only with a device at hand: every one is an argument check that
    returns before anything is launched, and the outputs stay as they were"""
    import torch
    from libflagstats_amd import filter as flt
    n = 4096
    t = torch.zeros(n + 8, dtype=torch.int16, device="cuda")
    q = torch.full((n + 8,), 60, dtype=torch.uint8, device="cuda")
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

    def refused(what, text, d_array=t.data_ptr(), n_=n, require=0, exclude=0x904, d_mapq=q.data_ptr(), mn=30, flags=0, counters=True,
                forms=("device", "sync", "host")):
        for form in forms:
            if form == "device":
                rc = hip.FLAGSTATS_hip_device_u16_filter(d_array, n_, require, exclude, d_mapq, mn, out.data_ptr() if counters else None,
                                                         sel.data_ptr(), flags, None)
            elif form == "sync":
                rc = hip.FLAGSTATS_hip_device_u16_filter_sync(d_array, n_, require, exclude, d_mapq, mn,
                                                              h_out.ctypes.data if counters else None, ctypes.byref(h_sel), flags)
            else:
                src = host16.ctypes.data + (d_array - t.data_ptr()) if d_array else None
                rc = hip.FLAGSTATS_hip_u16_x64_filter(src, n_, require, exclude, host8.ctypes.data if d_mapq else None, mn,
                                                      h_out.ctypes.data if counters else None, ctypes.byref(h_sel), flags)
            assert rc != 0, (what, form)
            assert text in err(hip), (what, form, err(hip))
        untouched(what)

    refused("require above 16 bits", "require must be a 16-bit FLAG mask", require=0x10000)
    refused("exclude above 16 bits", "exclude must be a 16-bit FLAG mask", exclude=0x10000)
    refused("min_mapq above a byte", "min_mapq must be at most 255", mn=256)
    refused("NULL mapq", "NULL mapq with min_mapq > 0 and n > 0", d_mapq=None)
    refused("NULL array", "NULL array with n > 0", d_array=None)
    refused("an odd array address", "2-byte aligned", d_array=t.data_ptr() + 1)
    refused("an extra flag bit", "no other bits", flags=4)
    refused("NULL counters", "NULL counters", counters=False)
    refused("n * 2 is no size", "n * 2 is not a size", n_=1 << 63)
    # a wave's uint32 totals (where's limit): 2^62 flags on any grid this device launches.  The host form launches per chunk of
    # "chunk_flags" flags and cannot reach the limit, so it has nothing to refuse here
    refused("a wave's totals", "a wave's uint32 totals", n_=1 << 62, mn=0, d_mapq=None, forms=("device", "sync"))
    # the MAPQ column somewhere else than the array: in host memory, a CPU tensor in Python
    rc = hip.FLAGSTATS_hip_device_u16_filter(t.data_ptr(), n, 0, 0x904, host8.ctypes.data, 30, out.data_ptr(), sel.data_ptr(), 0, None)
    assert rc != 0 and "d_mapq" in err(hip), err(hip)
    rc = hip.FLAGSTATS_hip_device_u16_filter_sync(t.data_ptr(), n, 0, 0x904, host8.ctypes.data, 30, h_out.ctypes.data, ctypes.byref(h_sel), 0)
    assert rc != 0 and "d_mapq" in err(hip), err(hip)
    with pytest.raises(ValueError, match=r"mapq must live on t's device \(cuda:0\), not on cpu"):
        flt.count_torch_filter(t, mapq=torch.zeros(n + 8, dtype=torch.uint8), min_mapq=30)
    with pytest.raises(ValueError, match=r"out must live on t's device \(cuda:0\), not on cpu"):
        flt.count_torch_filter(t, mapq=q, min_mapq=30, out=torch.zeros(32, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"selected must live on t's device \(cuda:0\), not on cpu"):
        flt.count_torch_filter(t, mapq=q, min_mapq=30, selected=torch.zeros(1, dtype=torch.int64))
    untouched("column elsewhere")
    # a host pointer as d_out (pageable, then page-locked) or as d_selected
    rc = hip.FLAGSTATS_hip_device_u16_filter(t.data_ptr(), n, 0, 0x904, q.data_ptr(), 30, h_out.ctypes.data, sel.data_ptr(), 0, None)
    assert rc != 0 and "d_out" in err(hip), err(hip)
    rc = hip.FLAGSTATS_hip_device_u16_filter(t.data_ptr(), n, 0, 0x904, q.data_ptr(), 30, out.data_ptr(), ctypes.addressof(h_sel), 0, None)
    assert rc != 0 and "d_selected" in err(hip), err(hip)
    pinned = hip.FLAGSTATS_hip_host_alloc(512)
    assert pinned
    try:
        ctypes.memset(pinned, 0, 512)
        rc = hip.FLAGSTATS_hip_device_u16_filter(t.data_ptr(), n, 0, 0x904, q.data_ptr(), 30, pinned, sel.data_ptr(), STORE, None)
        assert rc != 0 and "d_out must be device memory" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_u16_filter(t.data_ptr(), n, 0, 0x904, q.data_ptr(), 30, out.data_ptr(), pinned, STORE, None)
        assert rc != 0 and "d_selected must be device memory" in err(hip), err(hip)
        assert not any(ctypes.string_at(pinned, 512))
    finally:
        hip.FLAGSTATS_hip_host_free(pinned)
    untouched("host pointers")
    # extents: a column one byte short of n (its allocation is fine for n - 1, and is not looked at without a threshold), an
    # array one flag short, counters 8 bytes short
    nbytes = 2 << 20
    raw = hip.FLAGSTATS_hip_device_alloc(nbytes)
    big = torch.zeros(nbytes + 8, dtype=torch.int16, device="cuda")
    assert raw
    try:
        assert hip.FLAGSTATS_hip_memcpy_h2d(raw, np.zeros(nbytes, dtype=np.uint8).ctypes.data, nbytes) == 0
        rc = hip.FLAGSTATS_hip_device_u16_filter(big.data_ptr(), nbytes + 1, 0, 0x904, raw, 30, out.data_ptr(), sel.data_ptr(), STORE, None)
        assert rc != 0 and "d_mapq" in err(hip) and "1 bytes short" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_u16_filter_sync(big.data_ptr(), nbytes + 1, 0, 0x904, raw, 30, h_out.ctypes.data, ctypes.byref(h_sel), STORE)
        assert rc != 0 and "d_mapq" in err(hip) and "1 bytes short" in err(hip), err(hip)
        untouched("column extent")
        for n_ok, mn in ((nbytes, 30), (nbytes + 1, 0)):
            o = np.full(32, BIAS, dtype=np.uint64)
            h = ctypes.c_uint64(SEL_BIAS)
            assert hip.FLAGSTATS_hip_device_u16_filter_sync(big.data_ptr(), n_ok, 0, 0x904, raw, mn, o.ctypes.data, ctypes.byref(h), STORE) == 0, err(hip)
            assert not o.any() and h.value == (0 if mn else n_ok)          # flags 0 pass -F 0x904 and count nothing; MAPQ 0 < 30
        rc = hip.FLAGSTATS_hip_device_u16_filter(raw, nbytes // 2 + 1, 0, 0x904, None, 0, out.data_ptr(), sel.data_ptr(), STORE, None)
        assert rc != 0 and "d_array" in err(hip) and "2 bytes short" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_u16_filter(t.data_ptr(), n, 0, 0x904, q.data_ptr(), 30, raw + nbytes - 248, sel.data_ptr(), 0, None)
        assert rc != 0 and "d_out" in err(hip) and "8 bytes short" in err(hip), err(hip)
    finally:
        hip.FLAGSTATS_hip_device_free(raw)
    untouched("extents")
    # the launcher itself: other mode bits, no workgroups, a wave's uint32 totals, predicates out of range -- nothing queued
    words = torch.full((33,), BIAS, dtype=torch.int64, device="cuda")
    p = words.data_ptr()
    assert hip.fsk_launch_filter(t.data_ptr(), 8, 0, 0x904, q.data_ptr(), 30, p, p + 256, 4, 1, None) != 0
    assert hip.fsk_launch_filter(t.data_ptr(), 8, 0, 0x904, q.data_ptr(), 30, p, p + 256, 0, 0, None) != 0
    assert hip.fsk_launch_filter(t.data_ptr(), 1 << 35, 0, 0x904, None, 0, p, p + 256, STORE, 1, None) != 0
    assert hip.fsk_launch_filter(t.data_ptr(), 8, 0x10000, 0, None, 0, p, p + 256, STORE, 1, None) != 0
    assert hip.fsk_launch_filter(t.data_ptr(), 8, 0, 0x10000, None, 0, p, p + 256, STORE, 1, None) != 0
    assert hip.fsk_launch_filter(t.data_ptr(), 8, 0, 0, None, 30, p, p + 256, STORE, 1, None) != 0
    torch.cuda.synchronize()
    assert (words == BIAS).all()
