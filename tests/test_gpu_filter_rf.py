"""The filtered flagstat under samtools' whole FLAG predicate on the MI355X: fsk::flagstat_count_filter_rf in its six
instantiations, fsk_launch_filter_rf's three cases (a residue, a reduced pair handed to fsk_launch_filter, nothing can pass), the
three C entries and libflagstats_amd/filter_rf.py.

Expected counters never come from the code under test: filter_rf_oracle.want_counters is oracle.flagstat_c of values[mask]
(superset slots from oracle.samtools_counts and the definition) under the numpy mask of the predicate; the expected `selected` is
int(mask.sum())."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from filter_rf_oracle import view_mask, want_counters  # noqa: E402
from test_gpu_where import BIAS, BYTE_ALIGNMENTS, GARBAGE, LENGTHS, SEL_BIAS, STORE, SUPERSET, Rows, S, dev8, dev16, err, expect_row, u64  # noqa: E402,E501

pytestmark = pytest.mark.gpu

# (require, exclude, include_any, exclude_all)
PAIRS = tuple((1 << i) | (1 << j) for i in range(16) for j in range(i + 1, 16))     # within either byte plane and across them
RESIDUAL = ([(0, 0, a, 0) for a in PAIRS] + [(0, 0, 0, g) for g in PAIRS]
            + [(0, 0, 0xFFFF, 0), (0, 0, 0, 0xFFFF), (0, 0, 0x0050, 0x000C), (0, 0, 0x0050, 0x0050), (0, 0, 0x8001, 0x0180),
               (0x2, 0x904, 0x0050, 0), (0x2, 0x904, 0, 0x0420), (0x2, 0x904, 0x0050, 0x0420), (0x2, 0x904, 0x0050, 0x0440)])
REDUCIBLE = [(0, 0, 0x0040, 0), (0, 0, 0, 0x0400), (0x0010, 0, 0x0050, 0), (0, 0x0008, 0, 0x000C), (0, 0x0010, 0x0050, 0),
             (0x0004, 0, 0, 0x000C), (0x2, 0x904, 0x0040, 0x000C), (0x2, 0x904, 0, 0)]
EMPTY = [(0x000C, 0, 0, 0x000C), (0, 0x0050, 0x0050, 0), (0x2, 0x904, 0x0104, 0), (0x0041, 0x0041, 0x0050, 0x000C)]


def kind(hip, p):
    out = (ctypes.c_uint32 * 4)()
    return hip.fsk_filter_rf_reduce(p[0], p[1], p[2], p[3], out)


# ------------------------------------------------------------------ 1. every value under every kind of predicate
GROUPS = {"any_of_pairs": RESIDUAL[:120], "all_of_pairs": RESIDUAL[120:240], "both_reducible_empty": RESIDUAL[240:] + REDUCIBLE + EMPTY}
_EVERY_VALUE = {}


def every_value(oracle_mod):
    """0..65535 once each, shuffled (4 steps), and the expected superset counters under every predicate: made once"""
    if not _EVERY_VALUE:
        values = np.random.RandomState(2026).permutation(65536).astype(np.uint16)
        wants = {p: want_counters(oracle_mod, values, *p, superset=True) for p in RESIDUAL + REDUCIBLE + EMPTY}
        assert wants[0, 0, 0xFFFF, 0][1] == 65535 and wants[0, 0, 0, 0xFFFF][1] == 65535
        assert wants[0, 0, 0x0050, 0x0050][1] == 32768 and wants[0, 0, 0x0050, 0x000C][1] == 65536 * 3 // 4 * 3 // 4
        for p in EMPTY:
            assert wants[p][1] == 0 and not wants[p][0].any()
        for p in RESIDUAL + REDUCIBLE:
            assert 0 < wants[p][1] < 65536, p
        _EVERY_VALUE.update(values=values, wants=wants)
    return _EVERY_VALUE["values"], _EVERY_VALUE["wants"]


@pytest.mark.parametrize("group", sorted(GROUPS))
@pytest.mark.parametrize("form", ["device", "sync", "host"])
def test_every_value_under_every_kind_of_predicate(hip, oracle_mod, form, group):
    """0..65535 once each under every two-bit include_any and every two-bit exclude_all (within the low plane, within the high
    plane, across them), either mask with all 16 bits, both on (disjoint, identical, across planes), both with -f 0x2 -F 0x904,
    predicates the launcher reduces to a pair and predicates that pass nothing (the += rows stay as they are) -- store + superset
    form over garbage and += form over bias words, through the device entry, the _sync form and the host form"""
    values, wants = every_value(oracle_mod)
    for members, k in ((RESIDUAL, 2), (REDUCIBLE, 1), (EMPTY, 0)):
        for p in members:
            assert kind(hip, p) == k, p
    predicates = GROUPS[group]
    assert len(RESIDUAL[:240]) == 240 and all(p[3] == 0 for p in RESIDUAL[:120]) and all(p[2] == 0 for p in RESIDUAL[120:240])
    t = dev16(values)
    if form == "device":
        rows = Rows()
        plan = [(p, mode, rows.add(mode, wants[p][0], wants[p][1], (p, mode))) for p in predicates for mode in (STORE | SUPERSET, 0)]
        rows.upload()
        for p, mode, k in plan:
            rc = hip.FLAGSTATS_hip_device_u16_filter_rf(t.data_ptr(), 65536, p[0], p[1], p[2], p[3], None, 0, rows.out(k), rows.selected(k), mode,
                                                        None)
            assert rc == 0, (p, mode, err(hip))
        rows.check()
        return
    entry, src = ((hip.FLAGSTATS_hip_device_u16_filter_rf_sync, t.data_ptr()) if form == "sync" else
                  (hip.FLAGSTATS_hip_u16_x64_filter_rf, values.ctypes.data))
    for p in predicates:
        for mode in (STORE | SUPERSET, 0):
            o = np.full(32, GARBAGE if mode & STORE else BIAS, dtype=np.uint64)
            h = ctypes.c_uint64(GARBAGE if mode & STORE else SEL_BIAS)
            assert entry(src, 65536, p[0], p[1], p[2], p[3], None, 0, o.ctypes.data, ctypes.byref(h), mode) == 0, (form, p, mode, err(hip))
            assert np.array_equal(o, expect_row(wants[p][0], mode)), (form, p, mode, o)
            assert h.value == wants[p][1] + (0 if mode & STORE else SEL_BIAS), (form, p, mode)


def test_the_python_layer_and_the_filtered_entries(hip, oracle_mod):
    """with both options off the entries are the filtered entries; the four Python functions under a residue"""
    import torch
    from libflagstats_amd import filter_rf as rf
    values, _ = every_value(oracle_mod)
    t = dev16(values)
    for require, exclude in ((0, 0), (0x2, 0x904)):
        plain = np.zeros(32, dtype=np.uint64)
        h = ctypes.c_uint64(0)
        assert hip.FLAGSTATS_hip_device_u16_filter_sync(t.data_ptr(), 65536, require, exclude, None, 0, plain.ctypes.data, ctypes.byref(h), STORE) == 0
        got, selected = rf.count_device_ptr_filter_rf(t.data_ptr(), 65536, require, exclude)
        assert np.array_equal(got, plain) and selected == h.value and got.dtype == np.uint64
    p = (0x2, 0x904, 0x0050, 0x0420)
    want, nsel = want_counters(oracle_mod, values, *p)
    got, selected = rf.count_device_ptr_filter_rf(t.data_ptr(), 65536, *p)
    assert np.array_equal(got, want) and selected == nsel
    o, s = rf.count_torch_filter_rf(t, *p, store=True)
    torch.cuda.synchronize()
    assert o.dtype == torch.int64 and tuple(o.shape) == (32,) and tuple(s.shape) == (1,) and o.device == t.device
    assert np.array_equal(u64(o), want) and int(u64(s)[0]) == nsel
    o2, s2 = rf.count_torch_filter_rf(t, *p, out=o, selected=s)                     # a second call adds
    torch.cuda.synchronize()
    assert o2 is o and s2 is s and np.array_equal(u64(o), 2 * want) and int(u64(s)[0]) == 2 * nsel
    got, selected = rf.counters_filter_rf(values, require=p[0], exclude=p[1], include_any=p[2], exclude_all=p[3])
    assert np.array_equal(got, want) and selected == nsel
    d = rf.flagstats_filter_rf(values, require=p[0], exclude=p[1], include_any=p[2], exclude_all=p[3])
    assert d["n_values"] == nsel and int(d["failed"]["FQCFAIL"]) == int(want[25])
    assert int(d["passed"]["mapped"]) == nsel - int(want[2]) - int(want[18])


# ------------------------------------------------------------------ 2. lengths, phases, MAPQ alignments
PRED_ONE_PLANE, PRED_BOTH_PLANES = (0x0001, 0x0004, 0x0050, 0x0088), (0x0041, 0x0900, 0x0210, 0x0480)


def passing_background(p):
    """a flag with as many bits as the predicate lets pass: read outside [0, n), it changes `selected` and several counters"""
    g_bit = p[3] & -p[3]
    return 0xFFFF & ~p[1] & ~g_bit


def test_lengths_phases_mapq_alignments(hip, oracle_mod):
    """every length around nothing, a vector, a wave's line and one and two steps x every array phase x {no MAPQ, MAPQ at byte
    alignments 0, 1, 3, 8, 15} x two residual predicates (all four masks on the low byte plane; all four on both).  The array
    sits in a slab whose surrounding 64 flags pass the predicate, the MAPQ in a slab whose surrounding bytes are 0xFF (they pass
    every threshold): one element read outside [0, n) changes `selected` and the counters.  Through fsk_launch_filter_rf at
    grids 1, 2, 3 and the public device entry, store form over garbage and += over bias words."""
    rng = np.random.RandomState(47)
    nmax = LENGTHS[-1]
    preds = (PRED_ONE_PLANE, PRED_BOTH_PLANES)
    mapq = rng.randint(15, 60, nmax).astype(np.uint8)   # two thirds reach 30
    bodies = {}
    for p in preds:
        assert kind(hip, p) == 2 and view_mask(np.array([passing_background(p)], dtype=np.uint16), *p).all()
        body = rng.randint(0, 65536, nmax).astype(np.uint16)
        forced = rng.randint(0, 100, nmax) < 55           # these pass: one include_any bit set, one exclude_all bit clear
        a_bit = p[2] & -p[2]
        body[forced] = (body[forced] & np.uint16(passing_background(p))) | np.uint16(p[0] | a_bit)
        bodies[p] = body
        for q, mn in ((None, 0), (mapq, 30)):
            for n in LENGTHS:
                if n >= 63:
                    frac = view_mask(body[:n], *p, None if q is None else q[:n], mn).mean()
                    assert 0.25 <= frac <= 0.75, (p, mn, n, frac)
    wants = {(p, mn, n): want_counters(oracle_mod, bodies[p][:n], *p, mapq[:n], mn, superset=True)
             for p in preds for mn in (0, 30) for n in LENGTHS}
    arrays, a_at = [], {}
    pos = 0
    for p in preds:
        for n in LENGTHS:
            for phase in range(8):
                region = np.full((64 + 8 + n + 64 + 7) // 8 * 8, passing_background(p), dtype=np.uint16)
                region[64 + phase:64 + phase + n] = bodies[p][:n]
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
            rc = hip.FLAGSTATS_hip_device_u16_filter_rf(ptr if n else None, n, p[0], p[1], p[2], p[3], qptr if n else None, mn, rows.out(k),
                                                        rows.selected(k), mode, None)
            assert rc == 0, (rows.notes[k], err(hip))
        else:
            rc = hip.fsk_launch_filter_rf(ptr if n else None, n, p[0], p[1], p[2], p[3], qptr if n else None, mn, rows.out(k),
                                          rows.selected(k), mode, grid, None)
            assert rc == 0, (rows.notes[k], rc)
    rows.check()


# ------------------------------------------------------------------ 3. epochs
@pytest.mark.parametrize("min_mapq", [0, 30])
def test_epochs(hip, oracle_mod, min_mapq):
    """one workgroup over 258 S + 3 flags, both options on: 258 fast steps and a tail edge step, so every wave passes its
    staggered first flush (after 255, 191, 127 and 63 pushes) and wave 0 a full epoch of 255 steps (test_gpu_filter.py's shape)"""
    n = 258 * S + 3
    p = (0x0001, 0x0804, 0x0050, 0x0420)
    assert kind(hip, p) == 2
    pattern = np.random.RandomState(307).randint(0, 65536, 65_521).astype(np.uint16)
    values = np.resize(pattern, n)
    mapq = np.resize(np.random.RandomState(308).randint(0, 61, 65_519).astype(np.uint8), n)
    want, nsel = want_counters(oracle_mod, values, *p, mapq, min_mapq, superset=True)
    assert 0 < nsel < n
    t = dev16(values)
    q = dev8(mapq)
    assert t.data_ptr() % 16 == 0
    rows = Rows()
    ks = [rows.add(mode, want, nsel, (min_mapq, mode)) for mode in (STORE | SUPERSET, 0)]
    rows.upload()
    for k in ks:
        rc = hip.fsk_launch_filter_rf(t.data_ptr(), n, p[0], p[1], p[2], p[3], q.data_ptr() if min_mapq else None, min_mapq, rows.out(k),
                                      rows.selected(k), rows.modes[k], 1, None)
        assert rc == 0, rc
    rows.check()


# ------------------------------------------------------------------ 4. host form across chunks
def test_host_form_across_chunks(hip, oracle_mod):
    """chunks of 8,192 flags, five of them and a ragged tail, with and without the MAPQ column; a residue, a reduced pair and an
    empty predicate"""
    from libflagstats_amd import _lib
    from libflagstats_amd import filter_rf as rf
    n = 5 * 8192 + 77
    rng = np.random.RandomState(91)
    values = rng.randint(0, 65536, n).astype(np.uint16)
    mapq = rng.randint(0, 60, n).astype(np.uint8)
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", 8192), "chunk_flags")
        for p in ((0x0001, 0x0804, 0x0050, 0x0420), (0x0001, 0x0804, 0x0040, 0), (0, 0x0050, 0x0050, 0)):
            for q, mn in ((None, 0), (mapq, 30)):
                wants = {sup: want_counters(oracle_mod, values, *p, q, mn, superset=bool(sup)) for sup in (0, SUPERSET)}
                nsel = wants[0][1]
                assert (0 < nsel < n) == (kind(hip, p) != 0)
                got, selected = rf.counters_filter_rf(values, *p, mapq=q, min_mapq=mn)
                assert np.array_equal(got, wants[0][0]) and selected == nsel, (p, mn)
                got, selected = rf.counters_filter_rf(values, *p, mapq=q, min_mapq=mn, superset=True)
                assert np.array_equal(got, wants[SUPERSET][0]) and selected == nsel, (p, mn, "superset")
                for flags in (0, SUPERSET):                  # += over bias words
                    o = np.full(32, BIAS, dtype=np.uint64)
                    h = ctypes.c_uint64(SEL_BIAS)
                    rc = hip.FLAGSTATS_hip_u16_x64_filter_rf(values.ctypes.data, n, p[0], p[1], p[2], p[3], q.ctypes.data if mn else None, mn,
                                                             o.ctypes.data, ctypes.byref(h), flags)
                    assert rc == 0, err(hip)
                    assert np.array_equal(o, expect_row(wants[SUPERSET][0], flags)) and h.value == SEL_BIAS + nsel, (p, mn, flags)
                # one chunk only (a single staging slot), from an odd host address
                got, selected = rf.counters_filter_rf(values[1:100], *p, mapq=None if q is None else q[1:100], min_mapq=mn)
                want, nsel = want_counters(oracle_mod, values[1:100], *p, None if q is None else q[1:100], mn)
                assert np.array_equal(got, want) and selected == nsel
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old
    # n == 0: += touches nothing, store writes zeros; NULL pointers are accepted
    for entry in (hip.FLAGSTATS_hip_u16_x64_filter_rf, hip.FLAGSTATS_hip_device_u16_filter_rf_sync):
        for mn in (0, 30):
            o = np.full(32, BIAS, dtype=np.uint64)
            h = ctypes.c_uint64(5)
            assert entry(None, 0, 1, 4, 0x50, 0x420, None, mn, o.ctypes.data, ctypes.byref(h), 0) == 0 and (o == BIAS).all() and h.value == 5
            assert entry(None, 0, 1, 4, 0x50, 0x420, None, mn, o.ctypes.data, ctypes.byref(h), STORE) == 0 and not o.any() and h.value == 0
    got, selected = rf.counters_filter_rf(values[:0], 1, 4, 0x50, 0x420, mapq=mapq[:0], min_mapq=30)
    assert not got.any() and selected == 0
    got, selected = rf.count_device_ptr_filter_rf(0, 0, 1, 4, 0x50, 0x420)
    assert not got.any() and selected == 0


# ------------------------------------------------------------------ 5. atomics
def test_three_streams_add_into_one_pair(hip, oracle_mod):
    """three launches on three streams -- any-of alone with -q, all-of alone, both -- add into one (out, selected) pair"""
    import torch
    from libflagstats_amd import filter_rf as rf
    rng = np.random.RandomState(79)
    out = torch.zeros(32, dtype=torch.int64, device="cuda")
    selected = torch.zeros(1, dtype=torch.int64, device="cuda")
    total, total_sel = np.zeros(32, dtype=np.uint64), 0
    inputs = []
    for n, p, mn in ((40 * S + 11, (0, 0x904, 0x0050, 0), 30), (37 * S + 5, (0x2, 0x900, 0, 0x000C), 0),
                     (43 * S - 3, (0x0001, 0x8000, 0x0210, 0x0480), 200)):
        assert kind(hip, p) == 2
        values = rng.randint(0, 65536, n).astype(np.uint16)
        mapq = rng.randint(0, 256, n).astype(np.uint8)
        want, nsel = want_counters(oracle_mod, values, *p, mapq, mn, superset=True)
        assert nsel > 0
        total += want
        total_sel += nsel
        inputs.append((dev16(values), p, dev8(mapq) if mn else None, mn))
    streams = [torch.cuda.Stream() for _ in inputs]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    for st, (t, p, q, mn) in zip(streams, inputs):
        with torch.cuda.stream(st):
            rf.count_torch_filter_rf(t, require=p[0], exclude=p[1], include_any=p[2], exclude_all=p[3], mapq=q, min_mapq=mn, out=out,
                                     selected=selected, superset=True)
    for st in streams:
        st.synchronize()
    assert np.array_equal(u64(out), total) and int(u64(selected)[0]) == total_sel


# ------------------------------------------------------------------ 6. refusals that need a device
def test_device_dependent_refusals(hip):
    """what the C entries and the Python layer can refuse only with a device at hand: every one is an argument check that
    returns before anything is launched, and the outputs stay as they were"""
    import torch
    from libflagstats_amd import filter_rf as rf
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

    def refused(what, text, d_array=t.data_ptr(), n_=n, require=0, exclude=0x904, include_any=0x50, exclude_all=0x420, d_mapq=q.data_ptr(),
                mn=30, flags=0, counters=True, forms=("device", "sync", "host")):
        for form in forms:
            if form == "device":
                rc = hip.FLAGSTATS_hip_device_u16_filter_rf(d_array, n_, require, exclude, include_any, exclude_all, d_mapq, mn,
                                                            out.data_ptr() if counters else None, sel.data_ptr(), flags, None)
            elif form == "sync":
                rc = hip.FLAGSTATS_hip_device_u16_filter_rf_sync(d_array, n_, require, exclude, include_any, exclude_all, d_mapq, mn,
                                                                 h_out.ctypes.data if counters else None, ctypes.byref(h_sel), flags)
            else:
                src = host16.ctypes.data + (d_array - t.data_ptr()) if d_array else None
                rc = hip.FLAGSTATS_hip_u16_x64_filter_rf(src, n_, require, exclude, include_any, exclude_all,
                                                         host8.ctypes.data if d_mapq else None, mn,
                                                         h_out.ctypes.data if counters else None, ctypes.byref(h_sel), flags)
            assert rc != 0, (what, form)
            assert text in err(hip), (what, form, err(hip))
        untouched(what)

    refused("include_any above 16 bits", "include_any must be a 16-bit FLAG mask (at most 0xFFFF)", include_any=0x10000)
    refused("exclude_all above 16 bits", "exclude_all must be a 16-bit FLAG mask (at most 0xFFFF)", exclude_all=0x10000)
    refused("require above 16 bits", "require must be a 16-bit FLAG mask", require=0x10000)
    refused("exclude above 16 bits", "exclude must be a 16-bit FLAG mask", exclude=0x10000)
    refused("min_mapq above a byte", "min_mapq must be at most 255", mn=256)
    refused("NULL mapq", "NULL mapq with min_mapq > 0 and n > 0", d_mapq=None)
    refused("NULL array", "NULL array with n > 0", d_array=None)
    refused("an odd array address", "2-byte aligned", d_array=t.data_ptr() + 1)
    refused("an extra flag bit", "no other bits", flags=4)
    refused("NULL counters", "NULL counters", counters=False)
    refused("n * 2 is no size", "n * 2 is not a size", n_=1 << 63)
    refused("a wave's totals", "a wave's uint32 totals", n_=1 << 62, mn=0, d_mapq=None, forms=("device", "sync"))
    # the same refusals where the launcher would reduce the predicate or launch nothing
    refused("NULL array, a reduced pair", "NULL array with n > 0", d_array=None, include_any=0x40, exclude_all=0)
    refused("NULL mapq, nothing can pass", "NULL mapq with min_mapq > 0 and n > 0", d_mapq=None, exclude=0x50, exclude_all=0)
    # the MAPQ column somewhere else than the array: in host memory, a CPU tensor in Python
    rc = hip.FLAGSTATS_hip_device_u16_filter_rf(t.data_ptr(), n, 0, 0x904, 0x50, 0x420, host8.ctypes.data, 30, out.data_ptr(), sel.data_ptr(), 0, None)
    assert rc != 0 and "d_mapq" in err(hip), err(hip)
    rc = hip.FLAGSTATS_hip_device_u16_filter_rf_sync(t.data_ptr(), n, 0, 0x904, 0x50, 0x420, host8.ctypes.data, 30, h_out.ctypes.data,
                                                     ctypes.byref(h_sel), 0)
    assert rc != 0 and "d_mapq" in err(hip), err(hip)
    with pytest.raises(ValueError, match=r"mapq must live on t's device \(cuda:0\), not on cpu"):
        rf.count_torch_filter_rf(t, include_any=0x50, mapq=torch.zeros(n + 8, dtype=torch.uint8), min_mapq=30)
    with pytest.raises(ValueError, match=r"out must live on t's device \(cuda:0\), not on cpu"):
        rf.count_torch_filter_rf(t, include_any=0x50, mapq=q, min_mapq=30, out=torch.zeros(32, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"selected must live on t's device \(cuda:0\), not on cpu"):
        rf.count_torch_filter_rf(t, exclude_all=0xC, mapq=q, min_mapq=30, selected=torch.zeros(1, dtype=torch.int64))
    if torch.cuda.device_count() > 1:               # a column or a result on another device
        other = torch.device("cuda:1")
        with pytest.raises(ValueError, match=r"mapq must live on t's device \(cuda:0\), not on cuda:1"):
            rf.count_torch_filter_rf(t, include_any=0x50, mapq=torch.zeros(n + 8, dtype=torch.uint8, device=other), min_mapq=30)
        with pytest.raises(ValueError, match=r"out must live on t's device \(cuda:0\), not on cuda:1"):
            rf.count_torch_filter_rf(t, include_any=0x50, out=torch.zeros(32, dtype=torch.int64, device=other))
        q1 = torch.full((n + 8,), 60, dtype=torch.uint8, device=other)
        rc = hip.FLAGSTATS_hip_device_u16_filter_rf(t.data_ptr(), n, 0, 0x904, 0x50, 0x420, q1.data_ptr(), 30, out.data_ptr(), sel.data_ptr(), 0, None)
        assert rc != 0 and "d_mapq and d_out live on different devices" in err(hip), err(hip)
    untouched("column elsewhere")
    # a host pointer as d_out or as d_selected
    rc = hip.FLAGSTATS_hip_device_u16_filter_rf(t.data_ptr(), n, 0, 0x904, 0x50, 0x420, q.data_ptr(), 30, h_out.ctypes.data, sel.data_ptr(), 0, None)
    assert rc != 0 and "d_out" in err(hip), err(hip)
    rc = hip.FLAGSTATS_hip_device_u16_filter_rf(t.data_ptr(), n, 0, 0x904, 0x50, 0x420, q.data_ptr(), 30, out.data_ptr(), ctypes.addressof(h_sel), 0, None)
    assert rc != 0 and "d_selected" in err(hip), err(hip)
    untouched("host pointers")
    # extents: a column one byte short of n, an array one flag short
    nbytes = 2 << 20
    raw = hip.FLAGSTATS_hip_device_alloc(nbytes)
    big = torch.zeros(nbytes + 8, dtype=torch.int16, device="cuda")
    assert raw
    try:
        assert hip.FLAGSTATS_hip_memcpy_h2d(raw, np.zeros(nbytes, dtype=np.uint8).ctypes.data, nbytes) == 0
        rc = hip.FLAGSTATS_hip_device_u16_filter_rf(big.data_ptr(), nbytes + 1, 0, 0x904, 0x50, 0x420, raw, 30, out.data_ptr(), sel.data_ptr(), STORE, None)
        assert rc != 0 and "d_mapq" in err(hip) and "1 bytes short" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_u16_filter_rf(raw, nbytes // 2 + 1, 0, 0x904, 0x50, 0x420, None, 0, out.data_ptr(), sel.data_ptr(), STORE, None)
        assert rc != 0 and "d_array" in err(hip) and "2 bytes short" in err(hip), err(hip)
    finally:
        hip.FLAGSTATS_hip_device_free(raw)
    untouched("extents")
    # the launcher itself: other mode bits, no workgroups, a wave's uint32 totals, masks out of range -- nothing queued, whichever
    # of its three cases the predicate is
    words = torch.full((33,), BIAS, dtype=torch.int64, device="cuda")
    p = words.data_ptr()
    for a, g in ((0x50, 0x420), (0x40, 0), (0, 0)):
        assert hip.fsk_launch_filter_rf(t.data_ptr(), 8, 0, 0x904, a, g, q.data_ptr(), 30, p, p + 256, 4, 1, None) != 0
        assert hip.fsk_launch_filter_rf(t.data_ptr(), 8, 0, 0x904, a, g, q.data_ptr(), 30, p, p + 256, 0, 0, None) != 0
        assert hip.fsk_launch_filter_rf(t.data_ptr(), 1 << 35, 0, 0x904, a, g, None, 0, p, p + 256, STORE, 1, None) != 0
        assert hip.fsk_launch_filter_rf(t.data_ptr(), 8, 0, 0, a, g, None, 30, p, p + 256, STORE, 1, None) != 0
    assert hip.fsk_launch_filter_rf(t.data_ptr(), 8, 0, 0x50, 0x50, 0, q.data_ptr(), 30, p, p + 256, 4, 1, None) != 0     # nothing can pass
    for masks in ((0x10000, 0, 0, 0), (0, 0x10000, 0, 0), (0, 0, 0x10000, 0), (0, 0, 0, 0x10000)):
        assert hip.fsk_launch_filter_rf(t.data_ptr(), 8, masks[0], masks[1], masks[2], masks[3], None, 0, p, p + 256, STORE, 1, None) != 0
    torch.cuda.synchronize()
    assert (words == BIAS).all()
