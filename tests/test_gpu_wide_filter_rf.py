"""The filtered wide-input flagstat under samtools' whole FLAG predicate on the MI355X: fsk::flagstat_count_wide_filter_rf in its
twelve instantiations, fsk_launch_wide_filter_rf's three cases (a residue, a reduced pair handed to fsk_launch_wide_filter, nothing
can pass), the three C entries and libflagstats_amd/wide_filter_rf.py.

Expected values never come from the code under test: wide_filter_rf_oracle.want is filter_rf_oracle.want_counters
(oracle.flagstat_c of values[mask], superset slots from oracle.samtools_counts and the definition) of the low 16 bits, `selected`
is int(mask.sum()) and `high` is np.bitwise_or.reduce(values.view(unsigned) & ~0xFFFF) over all elements -- or 0 when a pass over
all 65,536 FLAG values finds none that satisfies the FLAG part: such a call reads no element."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_filter_rf_oracle as wro  # noqa: E402
from filter_rf_oracle import view_mask  # noqa: E402
from test_gpu_filter_rf import EMPTY, PAIRS, REDUCIBLE, RESIDUAL, kind, passing_background  # noqa: E402
from test_gpu_wide_filter import (ALL_HIGH, BIAS, BYTE_ALIGNMENTS, GARBAGE, HIGH_BIAS, MODES, SEL_BIAS, SIGNED, STEP, STORE, SUPERSET,  # noqa: E402
                                  THRESHOLDS, UNSIGNED, WIDTHS, Rows, dev8, err, expect_triple, lengths, to_device, u64)

pytestmark = pytest.mark.gpu


def device_call(hip, ptr, n, W, p, q, mn, rows, k, grid=None, report=(True, True)):
    """one launch into row k: through the launcher at `grid` workgroups, or (grid None) through the public device entry"""
    mode = rows.modes[k]
    sel = rows.selected(k) if report[0] else None
    high = rows.high(k) if report[1] else None
    if grid is None:
        rc = hip.FLAGSTATS_hip_device_wide_filter_rf(ptr if n else None, n, W, p[0], p[1], p[2], p[3], q if n else None, mn, rows.out(k), sel,
                                                     high, mode, None)
        assert rc == 0, (rows.notes[k], err(hip))
    else:
        rc = hip.fsk_launch_wide_filter_rf(ptr if n else None, n, W, p[0], p[1], p[2], p[3], q if n else None, mn, rows.out(k), sel, high, mode,
                                           grid, None)
        assert rc == 0, (rows.notes[k], rc)


def host_call(hip, entry, src, n, W, p, q, mn, mode, want, note):
    """a _sync or host-form call over garbage (store) or bias words (+=), all three results checked"""
    store = bool(mode & STORE)
    o = np.full(32, GARBAGE if store else BIAS, dtype=np.uint64)
    s = ctypes.c_uint64(GARBAGE if store else SEL_BIAS)
    h = ctypes.c_uint64(GARBAGE if store else HIGH_BIAS)
    rc = entry(src, n, W, p[0], p[1], p[2], p[3], q, mn, o.ctypes.data, ctypes.byref(s), ctypes.byref(h), mode)
    assert rc == 0, (note, err(hip))
    got = np.concatenate([o, [np.uint64(s.value)], [np.uint64(h.value)]])
    assert np.array_equal(got, expect_triple(want[0], want[1], want[2], mode)), (note, got)


# ------------------------------------------------------------------ 1. every low value under every kind of predicate
GROUPS = {"any_of_pairs": RESIDUAL[:120], "all_of_pairs": RESIDUAL[120:240], "both_reducible_empty": RESIDUAL[240:] + REDUCIBLE + EMPTY}
# two bits within the low byte plane, within the high one and across the seam between bits 7 and 8, for each option; both at once
SUBSET = [(0, 0, 0x0050, 0), (0, 0, 0x0A00, 0), (0, 0, 0x0180, 0), (0, 0, 0, 0x000C), (0, 0, 0, 0x0C00), (0, 0, 0, 0x0180),
          (0x2, 0x904, 0x0050, 0x0420), (0, 0, 0x0040, 0), (0, 0x0050, 0x0050, 0)]
_COLUMNS = {}


def every_low_value(oracle_mod, dtype, predicates):
    """0..65535 once each in the low half, shuffled (8 or 16 steps); a fixed sparse set of elements -- among them the values 0 and
    0xFFFF -- carries bits above bit 15, one of them every such bit (a negative element in the signed dtypes), so under every
    predicate that can tell elements apart some carriers pass and some fail.  The column is made once per dtype, the expected
    values once per dtype and predicate"""
    W = np.dtype(dtype).itemsize
    if dtype not in _COLUMNS:
        low = np.random.RandomState(2027).permutation(65536).astype(np.uint64)
        carriers = sorted(set(range(11, 65536, 97)) | {int(np.flatnonzero(low == 0)[0]), int(np.flatnonzero(low == 0xFFFF)[0])})
        column = low.copy()
        for k, i in enumerate(carriers):
            column[i] |= np.uint64(1) << np.uint64(16 + (7 * k) % (8 * W - 16))
        column[carriers[3]] |= np.uint64(ALL_HIGH[W])
        values = column.astype(UNSIGNED[W]).view(dtype)
        assert wro.want_high(values) == ALL_HIGH[W] and (dtype.startswith("u") or (values < 0).sum() >= 1)
        assert sorted(wro.low16(values).tolist()) == list(range(65536))
        _COLUMNS[dtype] = (values, carriers, {})
    values, carriers, wants = _COLUMNS[dtype]
    for p in predicates:
        if p not in wants:
            wants[p] = wro.want(oracle_mod, values, *p, superset=True)
            m = view_mask(wro.low16(values), *p)[carriers]
            assert wants[p][2] == (0 if p in EMPTY else ALL_HIGH[W]), p
            assert p in EMPTY or (m.any() and not m.all()), p
    return values, wants


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_every_low_value_int32(hip, oracle_mod, group):
    """an int32 column with every low half once, through the device entry, under every two-bit include_any and every two-bit
    exclude_all (within the low plane, within the high plane, across them), either mask with all 16 bits, both on, both with
    -f 0x2 -F 0x904, the predicates the launcher reduces to a pair and the ones that pass nothing (whose rows stay as they are in
    the += form and read all zero, `high` included, in the store form) -- store + superset over garbage and += over bias words"""
    values, wants = every_low_value(oracle_mod, "int32", GROUPS[group])
    for members, k in ((RESIDUAL, 2), (REDUCIBLE, 1), (EMPTY, 0)):
        for p in members:
            assert kind(hip, p) == k, p
    assert len(PAIRS) == 120 and all(p[3] == 0 for p in GROUPS["any_of_pairs"]) and all(p[2] == 0 for p in GROUPS["all_of_pairs"])
    t = to_device(values)
    rows = Rows()
    plan = [(p, rows.add(mode, *wants[p], (p, mode))) for p in GROUPS[group] for mode in MODES]
    rows.upload()
    for p, k in plan:
        device_call(hip, t.data_ptr(), 65536, 4, p, None, 0, rows, k)
    rows.check()


@pytest.mark.parametrize("dtype,form", [("uint32", "device"), ("int64", "device"), ("uint64", "device"), ("int32", "sync"), ("int32", "host"),
                                        ("int64", "sync"), ("uint64", "host")])
def test_every_low_value_other_dtypes_and_forms(hip, oracle_mod, dtype, form):
    """the same column in the other dtypes and through the _sync and host forms, under two bits within the low byte plane, two
    within the high one and two across the seam for each option, both options with -f / -F, a reducible and an empty predicate"""
    values, wants = every_low_value(oracle_mod, dtype, SUBSET)
    W = values.dtype.itemsize
    assert [kind(hip, p) for p in SUBSET] == [2] * 7 + [1, 0]
    t = to_device(values)
    if form == "device":
        rows = Rows()
        plan = [(p, rows.add(mode, *wants[p], (dtype, p, mode))) for p in SUBSET for mode in MODES]
        rows.upload()
        for p, k in plan:
            device_call(hip, t.data_ptr(), 65536, W, p, None, 0, rows, k)
        rows.check()
        return
    entry, src = ((hip.FLAGSTATS_hip_device_wide_filter_rf_sync, t.data_ptr()) if form == "sync" else
                  (hip.FLAGSTATS_hip_wide_x64_filter_rf, values.ctypes.data))
    for p in SUBSET:
        for mode in MODES:
            host_call(hip, entry, src, 65536, W, p, None, 0, mode, wants[p], (dtype, form, p, mode))


# ------------------------------------------------------------------ 2. the high half never reaches the predicate
@pytest.mark.parametrize("W", WIDTHS)
def test_the_high_half_never_reaches_the_predicate(hip, oracle_mod, W):
    """2 STEP + 100 elements one element into a 16-byte line (a head edge step, a fast step, a tail edge step).  A third of the
    elements has no bit of include_any in the low half and all of them in every higher 16-bit field: they must fail.  Another
    third carries all of exclude_all in every higher field while the low half lacks one of its bits: they must pass.  `high`
    reports those bits all the same"""
    a, g = 0x0050, 0x0420
    n = 2 * STEP[W] + 100
    rng = np.random.RandomState(61 + W)
    low = rng.randint(0, 65536, n).astype(np.uint64)
    role = rng.randint(0, 3, n)
    up = sum(1 << s for s in range(16, 8 * W, 16))          # a mask m in every higher field: m * up
    col = low.copy()
    col[role == 1] = (low[role == 1] & np.uint64(0xFFFF & ~a)) | np.uint64(a * up)
    col[role == 2] = (low[role == 2] & np.uint64(0xFFFF & ~0x0020)) | np.uint64(g * up)
    values = col.astype(UNSIGNED[W])
    low16 = wro.low16(values)
    assert not view_mask(low16, 0, 0, a, 0)[role == 1].any() and view_mask(low16, 0, 0, 0, g)[role == 2].all()
    high = wro.want_high(values)
    assert high == (a | g) * up
    slab = to_device(np.full(16 // W + n + 8, ALL_HIGH[W] | 0xFFFF, dtype=UNSIGNED[W]))
    slab[1:1 + n] = to_device(values)
    ptr = slab.data_ptr() + W
    assert ptr % 16 == W
    mapq = rng.randint(0, 61, n).astype(np.uint8)
    q = dev8(mapq)
    rows = Rows()
    plan = []
    for p in ((0, 0, a, 0), (0, 0, 0, g), (0x0001, 0x0800, a, g)):
        assert kind(hip, p) == 2
        for mn in (0, 30):
            want = wro.want(oracle_mod, values, *p, mapq, mn, superset=True)
            assert 0 < want[1] < n and want[2] == high
            for mode in MODES:
                for grid in (2, None):
                    plan.append((p, mn, grid, rows.add(mode, *want, (W, p, mn, mode, grid))))
    rows.upload()
    for p, mn, grid, k in plan:
        device_call(hip, ptr, n, W, p, q.data_ptr() if mn else None, mn, rows, k, grid)
    rows.check()


# ------------------------------------------------------------------ 3. W = 8: the two vectors of a group
@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("which", ["even", "odd"])
def test_w8_pairing(hip, oracle_mod, which, phase):
    """int64: a group of 4 flags is made of two vectors of a lane, 64 vectors = 128 elements apart.  Columns in which only the
    elements of the even vectors of a lane, or only those of the odd ones, pass the residue (by their flags; then, with flags that
    all pass, by their MAPQ bytes alone): 2 STEP + 3 elements at the start of a line and one element into it"""
    W, a, g = 8, 0x0210, 0x0480
    n = 2 * STEP[W] + 3
    rng = np.random.RandomState(67 + phase)
    position = np.arange(n) + phase                          # on the grid of elements that starts at the 16-byte line
    chosen = ((position // 2 // 64) % 2 == (0 if which == "even" else 1))
    passes = np.where(rng.randint(0, 2, n).astype(bool), 0x0010, 0x0200) | rng.randint(0, 2, n) * 0x0080 | rng.randint(0, 2, n) * 0x0041
    fails_any = rng.randint(0, 2, n) * 0x0080 | rng.randint(0, 2, n) * 0x0041              # no bit of a
    fails_all = g | 0x0010 | rng.randint(0, 2, n) * 0x0041                                 # all of g
    slab = to_device(np.full(2 + n + 8, ALL_HIGH[W] | 0x0A51, dtype=UNSIGNED[W]))
    ptr = slab.data_ptr() + W * phase
    mapq_only = np.where(chosen, 60, 10).astype(np.uint8)
    q = dev8(mapq_only)
    rows = Rows()
    columns = []
    for p, fails in (((0, 0, a, 0), fails_any), ((0, 0, 0, g), fails_all), ((0, 0, a, g), np.where(np.arange(n) % 2 == 0, fails_any, fails_all))):
        assert kind(hip, p) == 2
        flags = np.where(chosen, passes, fails).astype(UNSIGNED[W])
        assert np.array_equal(view_mask(wro.low16(flags), *p), chosen)
        for values, mn in ((flags, 0), (passes.astype(UNSIGNED[W]), 30)):
            want = wro.want(oracle_mod, values, *p, mapq_only, mn, superset=True)
            assert want[1] == int(chosen.sum()) and 0 < want[1] < n
            columns.append((values, p, mn, [rows.add(mode, *want, (which, phase, p, mn, mode)) for mode in MODES]))
    rows.upload()
    for values, p, mn, ks in columns:
        slab[phase:phase + n] = to_device(values)
        for k in ks:
            device_call(hip, ptr, n, W, p, q.data_ptr() if mn else None, mn, rows, k, 2)
    rows.check()


# ------------------------------------------------------------------ 4. lengths, phases, MAPQ alignments
@pytest.mark.parametrize("W", WIDTHS)
def test_lengths_phases_mapq_alignments(hip, oracle_mod, W):
    """test_gpu_wide_filter.py's lengths (0 among them) x every element phase of a 16-byte line x {no MAPQ, MAPQ at byte alignments
    0, 1, 3, 8, 15} x a predicate that a zero element passes (exclude_all alone) and one that it fails (include_any alone); a fifth
    of the body is zero.  The array sits in a slab whose surrounding elements pass the predicate AND carry every high bit, the
    MAPQ in a slab of 0xFF; the body carries no high bits: one element read outside [0, n) changes `selected`, the counters or
    `high`, and one zero-filled position counted changes `selected`.  Through fsk_launch_wide_filter_rf at grids 1, 2, 3 and the
    public device entry, store form over garbage and += over bias"""
    LENGTHS = lengths(W)
    EPV = 16 // W
    rng = np.random.RandomState(71 + W)
    nmax = LENGTHS[-1]
    body = rng.randint(0, 65536, nmax).astype(np.uint16)
    body[rng.randint(0, 5, nmax) == 0] = 0
    mapq = rng.randint(15, 60, nmax).astype(np.uint8)   # two thirds reach 30
    preds = ((0, 0, 0, 0x0480), (0, 0, 0x0210, 0))
    zero = np.zeros(1, dtype=np.uint16)
    assert view_mask(zero, *preds[0]).all() and not view_mask(zero, *preds[1]).any() and 0 in LENGTHS
    wide_body = body.astype(UNSIGNED[W])
    wants = {(p, mn, n): wro.want(oracle_mod, wide_body[:n], *p, mapq[:n], mn, superset=True) for p in preds for mn in (0, 30) for n in LENGTHS}
    for (p, mn, n), (_, nsel, high) in wants.items():
        assert kind(hip, p) == 2 and high == 0 and (n < 63 or 0 < nsel < n), (p, mn, n, nsel)
    arrays, a_at = [], {}
    pos = 0
    for p in preds:
        assert view_mask(np.array([passing_background(p)], dtype=np.uint16), *p).all()
        for n in LENGTHS:
            for phase in range(EPV):
                region = np.full((64 + EPV + n + 64 + EPV - 1) // EPV * EPV, passing_background(p) | ALL_HIGH[W], dtype=UNSIGNED[W])
                region[64 + phase:64 + phase + n] = wide_body[:n]
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
    d_arrays = to_device(np.concatenate(arrays))
    d_cols = dev8(np.concatenate(cols))
    assert d_arrays.data_ptr() % 16 == 0 and d_cols.data_ptr() % 16 == 0
    rows = Rows()
    calls = []
    for p in preds:
        for n in LENGTHS:
            for phase in range(EPV):
                ptr = d_arrays.data_ptr() + W * a_at[p, n, phase]
                assert ptr % 16 == W * phase
                for align in (None,) + BYTE_ALIGNMENTS:
                    qptr = None if align is None else d_cols.data_ptr() + q_at[n, align]
                    mn = 0 if align is None else 30
                    assert align is None or qptr % 16 == align
                    for grid in (1, 2, 3, None):
                        for mode in MODES:
                            k = rows.add(mode, *wants[p, mn, n], (W, p, n, phase, align, grid, mode))
                            calls.append((k, ptr, n, p, qptr, mn, grid))
    rows.upload()
    for k, ptr, n, p, qptr, mn, grid in calls:
        device_call(hip, ptr, n, W, p, qptr, mn, rows, k, grid)
    rows.check()


# ------------------------------------------------------------------ 5. the three things a call can be
@pytest.mark.parametrize("W", WIDTHS)
def test_the_three_dispatch_kinds(hip, oracle_mod, W):
    """a column with bits above bit 15 under a predicate of each kind.  Kind 0: all zero in the store form, `high` included, and
    everything as it was in the += form.  Kinds 1 and 2: the full `high`.  Kind 1 is FLAGSTATS_hip_device_wide_filter with the
    pair reduced by hand.  A NULL d_selected or d_high leaves the other results as they are"""
    import torch
    n = 2 * STEP[W] + 100
    rng = np.random.RandomState(83 + W)
    values = rng.randint(0, 65536, n).astype(UNSIGNED[W])
    values[5] |= UNSIGNED[W](1 << 17)
    values[STEP[W] + 77] |= UNSIGNED[W](1 << (8 * W - 1))
    mapq = rng.randint(0, 61, n).astype(np.uint8)
    high = (1 << 17) | (1 << (8 * W - 1))
    slab = to_device(np.full(16 // W + n + 8, ALL_HIGH[W] | 0xF0FF, dtype=UNSIGNED[W]))
    slab[1:1 + n] = to_device(values)
    ptr = slab.data_ptr() + W
    q = dev8(mapq)
    # predicate, its kind, the pair it is by hand
    cases = (((0x0001, 0x0804, 0x0050, 0x0420), 2, None), ((0, 0x0010, 0x0050, 0x0440), 1, (0x0040, 0x0410)), ((0x0001, 0x0804, 0x0040, 0), 1, (0x0041, 0x0804)),
             ((0, 0x0050, 0x0050, 0), 0, None), ((0x000C, 0, 0, 0x000C), 0, None), ((0x0041, 0x0041, 0x0050, 0x000C), 0, None))
    rows = Rows()
    plan = []
    for p, k_want, pair in cases:
        assert kind(hip, p) == k_want
        for mn in (0, 30):
            want = wro.want(oracle_mod, values, *p, mapq, mn, superset=True)
            assert want[2] == (high if k_want else 0) and (want[1] > 0) == (k_want > 0)
            if k_want == 0:
                assert not want[0].any()
            for mode in MODES:
                for grid in (2, None):
                    for report in ((True, True), (True, False), (False, True)):
                        plan.append((p, mn, grid, report, rows.add(mode, *want, (W, p, mn, mode, grid, report), report=report)))
    rows.upload()
    for p, mn, grid, report, k in plan:
        device_call(hip, ptr, n, W, p, q.data_ptr() if mn else None, mn, rows, k, grid, report)
    rows.check()
    for p, k_want, pair in cases:
        if pair is None:
            continue
        a = torch.zeros(34, dtype=torch.int64, device="cuda")
        b = torch.zeros(34, dtype=torch.int64, device="cuda")
        pa, pb = a.data_ptr(), b.data_ptr()
        assert hip.FLAGSTATS_hip_device_wide_filter_rf(ptr, n, W, p[0], p[1], p[2], p[3], q.data_ptr(), 30, pa, pa + 256, pa + 264,
                                                       STORE | SUPERSET, None) == 0, err(hip)
        assert hip.FLAGSTATS_hip_device_wide_filter(ptr, n, W, pair[0], pair[1], q.data_ptr(), 30, pb, pb + 256, pb + 264, STORE | SUPERSET,
                                                    None) == 0, err(hip)
        torch.cuda.synchronize()
        assert np.array_equal(u64(a), u64(b)) and int(u64(a)[33]) == high and int(u64(a)[32]) > 0, p
    host = slab[1:1 + n].cpu().numpy()
    for entry, src, col in ((hip.FLAGSTATS_hip_device_wide_filter_rf_sync, ptr, q.data_ptr()),
                            (hip.FLAGSTATS_hip_wide_x64_filter_rf, host.ctypes.data, mapq.ctypes.data)):
        for p, _, _ in cases:
            for mode in MODES:
                host_call(hip, entry, src, n, W, p, col, 30, mode, wro.want(oracle_mod, values, *p, mapq, 30, superset=True), (W, p, mode))


# ------------------------------------------------------------------ 6. MAPQ thresholds
@pytest.mark.parametrize("W", WIDTHS)
def test_mapq_thresholds(hip, oracle_mod, W):
    """2 STEP + 100 elements one element into a 16-byte line: a head edge step, a fast step and a tail edge step, every MAPQ value
    in the head edge step and in the fast step; thresholds on both sides of 128 under each half of the residue and under both"""
    import torch
    S = STEP[W]
    n = 2 * S + 100
    rng = np.random.RandomState(31 + W)
    values = rng.randint(0, 65536, n).astype(UNSIGNED[W])
    values[7] |= UNSIGNED[W](1 << 21)
    mapq = rng.randint(0, 256, n).astype(np.uint8)
    mapq[:512] = np.tile(np.arange(256, dtype=np.uint8), 2)
    mapq[S + 10:S + 10 + 256] = np.arange(256, dtype=np.uint8)
    values[600:620] = 0x0010                                          # these pass all three predicates at every threshold
    mapq[600:620] = 255
    slab = to_device(np.full(16 // W + n + 8, ALL_HIGH[W] | 0xF0FF, dtype=UNSIGNED[W]))
    slab[1:1 + n] = to_device(values)
    ptr = slab.data_ptr() + W
    col = torch.full((16 + n + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    col[16 + 5:16 + 5 + n] = dev8(mapq)
    qptr = col.data_ptr() + 16 + 5
    rows = Rows()
    calls = []
    for p in ((0, 0x904, 0x0050, 0), (0, 0x904, 0, 0x0420), (0, 0x904, 0x0050, 0x0420)):
        assert kind(hip, p) == 2
        for mn in THRESHOLDS:
            want = wro.want(oracle_mod, values, *p, mapq, mn, superset=True)
            assert 0 < want[1] < n and want[2] == 1 << 21
            for mode in MODES:
                for grid in (1, None):
                    calls.append((rows.add(mode, *want, (W, p, mn, mode, grid)), p, mn, grid))
    rows.upload()
    for k, p, mn, grid in calls:
        device_call(hip, ptr, n, W, p, qptr, mn, rows, k, grid)
    rows.check()


# ------------------------------------------------------------------ 7. epochs
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("min_mapq", [0, 30])
def test_epochs(hip, oracle_mod, W, min_mapq):
    """one workgroup over 258 STEP + 3 elements, both options on: 258 fast steps and a tail edge step, so every wave passes its
    staggered first flush (after 255, 191, 127 and 63 pushes) and wave 0 a full epoch of 255 steps (test_gpu_wide_filter.py's
    shape)"""
    n = 258 * STEP[W] + 3
    p = (0x0001, 0x0804, 0x0050, 0x0420)
    assert kind(hip, p) == 2
    pattern = np.random.RandomState(309).randint(0, 65536, 65_521).astype(np.uint16)
    values = np.resize(pattern, n).astype(UNSIGNED[W])
    values[n // 2] |= UNSIGNED[W](1 << 16)
    values[n - 2] |= UNSIGNED[W](1 << (8 * W - 1))
    mapq = np.resize(np.random.RandomState(310).randint(0, 61, 65_519).astype(np.uint8), n)
    want = wro.want(oracle_mod, values, *p, mapq, min_mapq, superset=True)
    assert 0 < want[1] < n and want[2] == (1 << 16) | (1 << (8 * W - 1))
    t = to_device(values)
    q = dev8(mapq)
    assert t.data_ptr() % 16 == 0
    rows = Rows()
    ks = [rows.add(mode, *want, (W, min_mapq, mode)) for mode in MODES]
    rows.upload()
    for k in ks:
        device_call(hip, t.data_ptr(), n, W, p, q.data_ptr() if min_mapq else None, min_mapq, rows, k, 1)
    rows.check()


# ------------------------------------------------------------------ 8. host form across chunks
@pytest.mark.parametrize("W", WIDTHS)
def test_host_form_across_chunks(hip, oracle_mod, W):
    """chunks of 8,192 uint16's worth of bytes (4,096 or 2,048 elements), five of them and a ragged tail, with and without the
    MAPQ column; a high bit in the fourth chunk only, on an element that fails; a residue, a reduced pair and an empty predicate"""
    from libflagstats_amd import _lib
    from libflagstats_amd import wide_filter_rf as wrf
    per_chunk = 8192 * 2 // W
    n = 5 * per_chunk + 77
    rng = np.random.RandomState(93 + W)
    values = rng.randint(0, 65536, n).astype(UNSIGNED[W])
    values[3 * per_chunk + 9] = UNSIGNED[W](0x0004 | (1 << (8 * W - 2)))         # fails -f 0x0001
    values = values.view(SIGNED[W])
    mapq = rng.randint(0, 60, n).astype(np.uint8)
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", 8192), "chunk_flags")
        for p in ((0x0001, 0x0804, 0x0050, 0x0420), (0x0001, 0x0804, 0x0040, 0), (0, 0x0050, 0x0050, 0)):
            k = kind(hip, p)
            for q, mn in ((None, 0), (mapq, 30)):
                wants = {sup: wro.want(oracle_mod, values, *p, q, mn, superset=bool(sup)) for sup in (0, SUPERSET)}
                _, nsel, high = wants[0]
                assert (0 < nsel < n) == (k != 0) and high == (1 << (8 * W - 2) if k else 0)
                for sup in (0, SUPERSET):
                    got, selected, h = wrf.counters_ints_filter_rf(values, *p, mapq=q, min_mapq=mn, superset=bool(sup))
                    assert np.array_equal(got, wants[sup][0]) and selected == nsel and h == high, (p, mn, sup)
                for flags in (0, SUPERSET):                  # += over bias words
                    host_call(hip, hip.FLAGSTATS_hip_wide_x64_filter_rf, values.ctypes.data, n, W, p, q.ctypes.data if mn else None, mn, flags,
                              wants[SUPERSET], (W, p, mn, flags))
                # the chunks without the carrier report nothing
                head = wro.want(oracle_mod, values[:3 * per_chunk], *p, q if q is None else q[:3 * per_chunk], mn)
                got, selected, h = wrf.counters_ints_filter_rf(values[:3 * per_chunk], *p, mapq=None if q is None else q[:3 * per_chunk],
                                                               min_mapq=mn)
                assert np.array_equal(got, head[0]) and selected == head[1] and h == 0
                # one chunk only (a single staging slot), the MAPQ column from an odd host address
                sub, subq = values[2:101], None if q is None else q[1:100]
                want = wro.want(oracle_mod, sub, *p, subq, mn)
                got, selected, h = wrf.counters_ints_filter_rf(sub, *p, mapq=subq, min_mapq=mn)
                assert np.array_equal(got, want[0]) and selected == want[1] and h == want[2] == 0
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old
    # n == 0: += touches nothing, store writes zeros; NULL pointers are accepted
    for entry in (hip.FLAGSTATS_hip_wide_x64_filter_rf, hip.FLAGSTATS_hip_device_wide_filter_rf_sync):
        for mn in (0, 30):
            o = np.full(32, BIAS, dtype=np.uint64)
            s, h = ctypes.c_uint64(5), ctypes.c_uint64(6)
            assert entry(None, 0, W, 1, 4, 0x50, 0x420, None, mn, o.ctypes.data, ctypes.byref(s), ctypes.byref(h), 0) == 0
            assert (o == BIAS).all() and s.value == 5 and h.value == 6
            assert entry(None, 0, W, 1, 4, 0x50, 0x420, None, mn, o.ctypes.data, ctypes.byref(s), ctypes.byref(h), STORE) == 0
            assert not o.any() and s.value == 0 and h.value == 0
    got, selected, h = wrf.counters_ints_filter_rf(values[:0], 1, 4, 0x50, 0x420, mapq=mapq[:0], min_mapq=30)
    assert not got.any() and selected == 0 and h == 0
    got, selected, h = wrf.count_device_ptr_ints_filter_rf(0, 0, W, 1, 4, 0x50, 0x420)
    assert not got.any() and selected == 0 and h == 0


# ------------------------------------------------------------------ 9. atomics
def test_three_streams_add_into_one_triple(hip, oracle_mod):
    """three launches on three streams -- any-of alone with -q on int32, all-of alone on int64, both on int32 -- add into one
    (out, selected, high) triple"""
    import torch
    from libflagstats_amd import wide_filter_rf as wrf
    rng = np.random.RandomState(77)
    out = torch.zeros(32, dtype=torch.int64, device="cuda")
    selected = torch.zeros(1, dtype=torch.int64, device="cuda")
    high = torch.zeros(1, dtype=torch.int64, device="cuda")
    total, total_sel, total_high = np.zeros(32, dtype=np.uint64), 0, 0
    inputs = []
    for W, n, p, mn, bit in ((4, 40 * STEP[4] + 11, (0, 0x904, 0x0050, 0), 30, 17), (8, 37 * STEP[8] + 5, (0x2, 0x900, 0, 0x000C), 0, 45),
                             (4, 43 * STEP[4] - 3, (0x0001, 0x8000, 0x0210, 0x0480), 200, 31)):
        assert kind(hip, p) == 2
        values = rng.randint(0, 65536, n).astype(UNSIGNED[W])
        values[n // 3] |= UNSIGNED[W](1 << bit)
        mapq = rng.randint(0, 256, n).astype(np.uint8)
        want, nsel, h = wro.want(oracle_mod, values, *p, mapq, mn, superset=True)
        assert nsel > 0 and h == 1 << bit
        total += want
        total_sel += nsel
        total_high |= h
        inputs.append((to_device(values), p, dev8(mapq) if mn else None, mn))
    streams = [torch.cuda.Stream() for _ in inputs]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    for st, (t, p, q, mn) in zip(streams, inputs):
        with torch.cuda.stream(st):
            wrf.count_torch_ints_filter_rf(t, require=p[0], exclude=p[1], include_any=p[2], exclude_all=p[3], mapq=q, min_mapq=mn, out=out,
                                           selected=selected, high=high, superset=True)
    for st in streams:
        st.synchronize()
    assert np.array_equal(u64(out), total) and int(u64(selected)[0]) == total_sel and int(u64(high)[0]) == total_high


# ------------------------------------------------------------------ 10. refusals that need a device
def test_device_dependent_refusals(hip):
    """what the C entries, the launcher and the Python layer can refuse only with a device at hand: every one is an argument check
    that returns before anything is launched, and the outputs stay as they were"""
    import torch
    from libflagstats_amd import wide_filter_rf as wrf
    n = 4096
    bufs = {W: torch.zeros(n + 8, dtype={4: torch.int32, 8: torch.int64}[W], device="cuda") for W in WIDTHS}
    q = torch.full((n + 8,), 60, dtype=torch.uint8, device="cuda")
    out = torch.full((32,), BIAS, dtype=torch.int64, device="cuda")
    sel = torch.full((1,), SEL_BIAS, dtype=torch.int64, device="cuda")
    high = torch.full((1,), HIGH_BIAS, dtype=torch.int64, device="cuda")
    h_out = np.full(32, BIAS, dtype=np.uint64)
    h_sel, h_high = ctypes.c_uint64(SEL_BIAS), ctypes.c_uint64(HIGH_BIAS)
    host = np.zeros(n + 8, dtype=np.int64)
    host8 = np.full(n + 8, 60, dtype=np.uint8)
    p8, p4 = bufs[8].data_ptr(), bufs[4].data_ptr()

    def untouched(what):
        torch.cuda.synchronize()
        assert (out == BIAS).all() and int(u64(sel)[0]) == SEL_BIAS and int(u64(high)[0]) == HIGH_BIAS, what
        assert (h_out == BIAS).all() and h_sel.value == SEL_BIAS and h_high.value == HIGH_BIAS, what

    def refused(what, text, d_array=p8, n_=n, eb=8, require=0, exclude=0x904, include_any=0x50, exclude_all=0x420, d_mapq=q.data_ptr(), mn=30,
                flags=0, counters=True, forms=("device", "sync", "host")):
        for form in forms:
            if form == "device":
                rc = hip.FLAGSTATS_hip_device_wide_filter_rf(d_array, n_, eb, require, exclude, include_any, exclude_all, d_mapq, mn,
                                                             out.data_ptr() if counters else None, sel.data_ptr(), high.data_ptr(), flags, None)
            elif form == "sync":
                rc = hip.FLAGSTATS_hip_device_wide_filter_rf_sync(d_array, n_, eb, require, exclude, include_any, exclude_all, d_mapq, mn,
                                                                  h_out.ctypes.data if counters else None, ctypes.byref(h_sel),
                                                                  ctypes.byref(h_high), flags)
            else:
                src = host.ctypes.data + (d_array - p8) % 8 if d_array else None
                rc = hip.FLAGSTATS_hip_wide_x64_filter_rf(src, n_, eb, require, exclude, include_any, exclude_all,
                                                          host8.ctypes.data if d_mapq else None, mn, h_out.ctypes.data if counters else None,
                                                          ctypes.byref(h_sel), ctypes.byref(h_high), flags)
            assert rc != 0, (what, form)
            assert text in err(hip), (what, form, err(hip))
        untouched(what)

    refused("elem_bytes 2", "u16 filter_rf entries", eb=2)
    refused("elem_bytes 3", "elem_bytes must be 4 or 8", eb=3)
    refused("off by 2 at W = 4", "4-byte aligned", d_array=p8 + 2, eb=4)
    refused("off by 4 at W = 8", "8-byte aligned", d_array=p8 + 4, eb=8)
    refused("an extra flag bit", "no other bits", flags=4)
    refused("NULL array", "NULL array with n > 0", d_array=None, eb=4)
    refused("n * elem_bytes is no size", "n * elem_bytes is not a size", n_=1 << 62)
    for W in WIDTHS:
        pw = bufs[W].data_ptr()
        refused("include_any above 16 bits", "include_any must be a 16-bit FLAG mask (at most 0xFFFF)", d_array=pw, eb=W, include_any=0x10000)
        refused("exclude_all above 16 bits", "exclude_all must be a 16-bit FLAG mask (at most 0xFFFF)", d_array=pw, eb=W, exclude_all=0x10000)
        refused("require above 16 bits", "require must be a 16-bit FLAG mask", d_array=pw, eb=W, require=0x10000)
        refused("exclude above 16 bits", "exclude must be a 16-bit FLAG mask", d_array=pw, eb=W, exclude=0x10000)
        refused("min_mapq above a byte", "min_mapq must be at most 255", d_array=pw, eb=W, mn=256)
        refused("NULL mapq", "NULL mapq with min_mapq > 0 and n > 0", d_array=pw, eb=W, d_mapq=None)
        refused("NULL counters", "NULL counters", d_array=pw, eb=W, counters=False)
        refused("a wave's totals", "a wave's uint32 totals", d_array=pw, eb=W, n_=1 << 60, mn=0, d_mapq=None, forms=("device", "sync"))
        # the same refusals where the launcher would reduce the predicate or launch nothing
        refused("NULL array, a reduced pair", "NULL array with n > 0", d_array=None, eb=W, include_any=0x40, exclude_all=0)
        refused("NULL mapq, nothing can pass", "NULL mapq with min_mapq > 0 and n > 0", d_array=pw, eb=W, d_mapq=None, exclude=0x50, exclude_all=0)
    # host memory where device memory is needed: the array, the column, d_out, d_selected, d_high
    for W in WIDTHS:
        pw = bufs[W].data_ptr()
        f = hip.FLAGSTATS_hip_device_wide_filter_rf
        for what, args in (("d_array", (host.ctypes.data, q.data_ptr(), out.data_ptr(), sel.data_ptr(), high.data_ptr())),
                           ("d_mapq", (pw, host8.ctypes.data, out.data_ptr(), sel.data_ptr(), high.data_ptr())),
                           ("d_out", (pw, q.data_ptr(), h_out.ctypes.data, sel.data_ptr(), high.data_ptr())),
                           ("d_selected", (pw, q.data_ptr(), out.data_ptr(), ctypes.addressof(h_sel), high.data_ptr())),
                           ("d_high", (pw, q.data_ptr(), out.data_ptr(), sel.data_ptr(), ctypes.addressof(h_high)))):
            rc = f(args[0], n, W, 0, 0x904, 0x50, 0x420, args[1], 30, args[2], args[3], args[4], 0, None)
            assert rc != 0 and what in err(hip), (what, err(hip))
        rc = hip.FLAGSTATS_hip_device_wide_filter_rf_sync(pw, n, W, 0, 0x904, 0x50, 0x420, host8.ctypes.data, 30, h_out.ctypes.data,
                                                          ctypes.byref(h_sel), ctypes.byref(h_high), 0)
        assert rc != 0 and "d_mapq" in err(hip), err(hip)
    untouched("host pointers")
    # extents: an array one element short, a column one byte short of n
    nbytes = 2 << 20
    raw = hip.FLAGSTATS_hip_device_alloc(nbytes)
    assert raw
    try:
        assert hip.FLAGSTATS_hip_memcpy_h2d(raw, np.zeros(nbytes, dtype=np.uint8).ctypes.data, nbytes) == 0
        for W in WIDTHS:
            big = torch.zeros(nbytes + 8, dtype={4: torch.int32, 8: torch.int64}[W], device="cuda")
            rc = hip.FLAGSTATS_hip_device_wide_filter_rf(raw, nbytes // W + 1, W, 0, 0x904, 0x50, 0x420, None, 0, out.data_ptr(), sel.data_ptr(),
                                                         high.data_ptr(), STORE, None)
            assert rc != 0 and "d_array" in err(hip) and "%d bytes short" % W in err(hip), err(hip)
            rc = hip.FLAGSTATS_hip_device_wide_filter_rf(big.data_ptr(), nbytes + 1, W, 0, 0x904, 0x50, 0x420, raw, 30, out.data_ptr(),
                                                         sel.data_ptr(), high.data_ptr(), STORE, None)
            assert rc != 0 and "d_mapq" in err(hip) and "1 bytes short" in err(hip), err(hip)
    finally:
        hip.FLAGSTATS_hip_device_free(raw)
    untouched("extents")
    # the Python layer: a column or a result somewhere else than t
    t = bufs[4]
    with pytest.raises(ValueError, match=r"mapq must live on t's device \(cuda:0\), not on cpu"):
        wrf.count_torch_ints_filter_rf(t, include_any=0x50, mapq=torch.zeros(n + 8, dtype=torch.uint8), min_mapq=30)
    for name, numel in (("out", 32), ("selected", 1), ("high", 1)):
        with pytest.raises(ValueError, match=r"%s must live on t's device \(cuda:0\), not on cpu" % name):
            wrf.count_torch_ints_filter_rf(t, exclude_all=0xC, mapq=q, min_mapq=30, **{name: torch.zeros(numel, dtype=torch.int64)})
    if torch.cuda.device_count() > 1:               # a column or a result on another device
        other = torch.device("cuda:1")
        with pytest.raises(ValueError, match=r"mapq must live on t's device \(cuda:0\), not on cuda:1"):
            wrf.count_torch_ints_filter_rf(t, include_any=0x50, mapq=torch.zeros(n + 8, dtype=torch.uint8, device=other), min_mapq=30)
        with pytest.raises(ValueError, match=r"high must live on t's device \(cuda:0\), not on cuda:1"):
            wrf.count_torch_ints_filter_rf(t, include_any=0x50, high=torch.zeros(1, dtype=torch.int64, device=other))
    untouched("the Python layer")
    # the launcher itself: other widths, misalignment, other mode bits, no workgroups, a wave's uint32 totals, masks out of range, a
    # NULL column under a threshold -- nothing queued, whichever of its three cases the predicate is
    words = torch.full((34,), BIAS, dtype=torch.int64, device="cuda")
    p = words.data_ptr()
    f = hip.fsk_launch_wide_filter_rf
    for W in WIDTHS:
        pw = bufs[W].data_ptr()
        for a, g in ((0x50, 0x420), (0x40, 0), (0, 0), (0x904, 0)):
            assert f(pw, 8, W, 0, 0x904, a, g, q.data_ptr(), 30, p, p + 256, p + 264, 4, 1, None) != 0
            assert f(pw, 8, W, 0, 0x904, a, g, q.data_ptr(), 30, p, p + 256, p + 264, 0, 0, None) != 0
            assert f(pw, 1 << 35, W, 0, 0x904, a, g, None, 0, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(pw, 8, W, 0, 0x904, a, g, None, 30, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(pw, 8, W, 0, 0x904, a, g, q.data_ptr(), 256, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(pw + W // 2, 8, W, 0, 0x904, a, g, None, 0, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(pw, 8, W, 0, 0x904, a, g, None, 0, None, p + 256, p + 264, STORE, 1, None) != 0
            for eb in (0, 1, 2, 3, 16):
                assert f(p4, 8, eb, 0, 0x904, a, g, None, 0, p, p + 256, p + 264, STORE, 1, None) != 0
        for masks in ((0x10000, 0, 0, 0), (0, 0x10000, 0, 0), (0, 0, 0x10000, 0), (0, 0, 0, 0x10000)):
            assert f(pw, 8, W, masks[0], masks[1], masks[2], masks[3], None, 0, p, p + 256, p + 264, STORE, 1, None) != 0
    torch.cuda.synchronize()
    assert (words == BIAS).all()


# ------------------------------------------------------------------ 11. the Python layers
def test_python_layers(hip, oracle_mod):
    """numpy over all six dtypes (the 2-byte ones take the uint16 route and report high == 0), strict and its message, the dict;
    the raw-pointer form; the torch layer's dtypes, shapes and placement; with both options off the entries are wide_filter's"""
    import torch
    from libflagstats_amd import wide, wide_filter
    from libflagstats_amd import wide_filter_rf as wrf
    n = 3 * STEP[4] + 41
    rng = np.random.RandomState(99)
    low = rng.randint(0, 65536, n).astype(np.uint16)
    mapq = rng.randint(0, 61, n).astype(np.uint8)
    p, mn = (0x0001, 0x0904, 0x0050, 0x0420), 30
    kw = dict(require=p[0], exclude=p[1], include_any=p[2], exclude_all=p[3])
    want, nsel, _ = wro.want(oracle_mod, low.astype(np.uint32), *p, mapq, mn)
    want_sup = wro.want(oracle_mod, low.astype(np.uint32), *p, mapq, mn, superset=True)[0]
    assert 0 < nsel < n and kind(hip, p) == 2
    for dt in ("int16", "uint16", "int32", "uint32", "int64", "uint64"):
        v = low.astype({"int16": np.uint16}.get(dt, dt)).view(dt)
        got, selected, high = wrf.counters_ints_filter_rf(v, *p, mapq=mapq, min_mapq=mn)
        assert got.dtype == np.uint64 and np.array_equal(got, want) and selected == nsel and high == 0, dt
        got, selected, high = wrf.counters_ints_filter_rf(v, mapq=mapq, min_mapq=mn, superset=True, **kw)
        assert np.array_equal(got, want_sup) and selected == nsel and high == 0, dt
        d = wrf.flagstats_ints_filter_rf(v, mapq=mapq, min_mapq=mn, **kw)
        assert d["n_values"] == nsel and int(d["failed"]["FQCFAIL"]) == int(want[25]) and "high_bits" not in d
        assert int(d["passed"]["mapped"]) == nsel - int(want[2]) - int(want[18])
        assert wrf.flagstats_ints_filter_rf(v, mapq=mapq, min_mapq=mn, strict=False, **kw)["high_bits"] == 0
        # with both options off: wide_filter's results
        a = wrf.counters_ints_filter_rf(v, p[0], p[1], mapq=mapq, min_mapq=mn)
        b = wide_filter.counters_ints_filter(v, p[0], p[1], mapq=mapq, min_mapq=mn)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
        if v.dtype.itemsize == 2:
            continue
        # one element that FAILS the predicate carries a bit above bit 15: strict refuses the column all the same
        W = v.dtype.itemsize
        bad = v.copy()
        at = int(np.flatnonzero(~view_mask(low, *p, mapq, mn))[5])
        bad.view(UNSIGNED[W])[at] |= UNSIGNED[W](1 << (8 * W - 1))
        mask = 1 << (8 * W - 1)
        with pytest.raises(ValueError) as e:
            wrf.flagstats_ints_filter_rf(bad, mapq=mapq, min_mapq=mn, **kw)
        assert str(e.value) == wide.high_bits_message(mask)
        d = wrf.flagstats_ints_filter_rf(bad, mapq=mapq, min_mapq=mn, strict=False, **kw)
        assert d["high_bits"] == mask and d["n_values"] == nsel and int(d["failed"]["FQCFAIL"]) == int(want[25])
        # a predicate nothing can pass reads no element: strict has nothing to refuse
        assert wrf.flagstats_ints_filter_rf(bad, exclude=0x50, include_any=0x50)["n_values"] == 0
        # the raw-pointer form and the torch layer on the same column
        t, q = to_device(bad), dev8(mapq)
        got, selected, high = wrf.count_device_ptr_ints_filter_rf(t.data_ptr(), n, W, *p, mapq_ptr=q.data_ptr(), min_mapq=mn, superset=True)
        assert np.array_equal(got, want_sup) and selected == nsel and high == mask
        o, s, h = wrf.count_torch_ints_filter_rf(t, mapq=q, min_mapq=mn, **kw)
        torch.cuda.synchronize()
        for x, numel in ((o, 32), (s, 1), (h, 1)):
            assert x.dtype == torch.int64 and tuple(x.shape) == (numel,) and x.device == t.device
        assert np.array_equal(u64(o), want) and int(u64(s)[0]) == nsel and int(u64(h)[0]) == mask
        o2, s2, h2 = wrf.count_torch_ints_filter_rf(t, mapq=q, min_mapq=mn, out=o, selected=s, high=h, **kw)   # += and |=
        assert o2 is o and s2 is s and h2 is h
        torch.cuda.synchronize()
        assert np.array_equal(u64(o), 2 * want) and int(u64(s)[0]) == 2 * nsel and int(u64(h)[0]) == mask
        wrf.count_torch_ints_filter_rf(t, mapq=q, min_mapq=mn, out=o, selected=s, high=h, store=True, superset=True, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(u64(o), want_sup) and int(u64(s)[0]) == nsel and int(u64(h)[0]) == mask
    # a 2-byte tensor takes the uint16 entry: `high` is left as it is, zeroed with store
    t16 = torch.from_numpy(low.view(np.int16)).cuda()
    q = dev8(mapq)
    h = torch.full((1,), 9, dtype=torch.int64, device="cuda")
    o, s, h2 = wrf.count_torch_ints_filter_rf(t16, mapq=q, min_mapq=mn, high=h, **kw)
    torch.cuda.synchronize()
    assert h2 is h and int(h[0]) == 9 and np.array_equal(u64(o), want) and int(u64(s)[0]) == nsel
    wrf.count_torch_ints_filter_rf(t16, mapq=q, min_mapq=mn, out=o, selected=s, high=h, store=True, **kw)
    torch.cuda.synchronize()
    assert int(h[0]) == 0 and np.array_equal(u64(o), want) and int(u64(s)[0]) == nsel
    # an empty tensor
    o, s, h = wrf.count_torch_ints_filter_rf(torch.zeros(0, dtype=torch.int32, device="cuda"), 1, 4, 0x50, 0x420)
    torch.cuda.synchronize()
    assert not u64(o).any() and int(s[0]) == 0 and int(h[0]) == 0
