"""The filtered wide-input flagstat on the MI355X: fsk::flagstat_count_wide_filter at both widths, with and without a MAPQ
column, the three C entries and libflagstats_amd/wide_filter.py.

Expected values never come from the code under test: wide_filter_oracle.want is filter_oracle.want_counters (oracle.flagstat_c
of values[mask], superset slots from oracle.samtools_counts and the definition) of the low 16 bits, `selected` is
int(mask.sum()) and `high` is np.bitwise_or.reduce(values.view(unsigned) & ~0xFFFF) over all elements.  The one exception is the
contract's: a pair with require & exclude != 0 reads no element, so its `high` is 0."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import where_oracle  # noqa: E402
import wide_filter_oracle as wfo  # noqa: E402
from filter_oracle import filter_mask  # noqa: E402
from test_gpu_filter import PRED_BOTH_PLANES, PRED_ONE_PLANE, PREDICATES  # noqa: E402

pytestmark = pytest.mark.gpu

STORE, SUPERSET = 1, 2
GARBAGE, BIAS, SEL_BIAS, HIGH_BIAS = 0x5EED_0000_0BAD, 3, 1 << 40, 1 << 40
WIDTHS = (4, 8)
STEP = {4: 8192, 8: 4096}                     # elements of one 32 KiB step
ALL_HIGH = {4: 0xFFFF0000, 8: 0xFFFFFFFFFFFF0000}
SIGNED = {4: np.int32, 8: np.int64}
UNSIGNED = {4: np.uint32, 8: np.uint64}
MODES = (STORE | SUPERSET, 0)


def to_device(v):
    """a numpy array of a 4- or 8-byte integer dtype as a CUDA tensor of the signed dtype of its width"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(v).view(SIGNED[v.dtype.itemsize])).cuda()


def dev8(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint8)).cuda()


def signed(x, W):
    """the Python int a tensor of W-byte signed elements takes for the unsigned element x"""
    return int(np.array([x], dtype=UNSIGNED[W]).view(SIGNED[W])[0])


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def err(hip):
    return hip.FLAGSTATS_hip_last_error().decode(errors="replace")


def expect_row(want, mode):
    """what 32 counters must read after a call in `mode`: the superset counters `want` cut to the form, over BIAS in the += form"""
    w = want.copy()
    if not mode & SUPERSET:
        w[[0, 9, 16]] = 0
    return w if mode & STORE else w + np.uint64(BIAS)


def expect_triple(want, selected, high, mode):
    store = bool(mode & STORE)
    return np.concatenate([expect_row(want, mode), [np.uint64(selected if store else selected + SEL_BIAS)],
                           [np.uint64(high if store else high | HIGH_BIAS)]]).astype(np.uint64)


def overlap_high(require, exclude, high):
    """an overlapping pair reads no element: its mask is 0"""
    return 0 if require & exclude else high


class Rows:
    """device words for many launches, one row of 34 per launch (32 counters, `selected`, `high`): filled with GARBAGE (store
    form) or BIAS / SEL_BIAS / HIGH_BIAS (+= form) in one copy, read back in one copy after every launch has been queued.  A row
    added with report=(False, ...) expects the word it does not hand to the launch to stay as it was filled."""

    def __init__(self):
        self.modes, self.wants, self.notes = [], [], []

    def add(self, mode, want, selected, high, note, report=(True, True)):
        row = expect_triple(want, selected, high, mode)
        fill = self.fill(mode)
        for i, r in enumerate(report):
            if not r:
                row[32 + i] = fill[32 + i]
        self.modes.append(mode)
        self.wants.append(row)
        self.notes.append(note)
        return len(self.modes) - 1

    @staticmethod
    def fill(mode):
        row = np.full(34, GARBAGE if mode & STORE else BIAS, dtype=np.uint64)
        if not mode & STORE:
            row[32], row[33] = SEL_BIAS, HIGH_BIAS
        return row

    def upload(self):
        import torch
        fill = np.stack([self.fill(mode) for mode in self.modes])
        self.t = torch.from_numpy(fill.view(np.int64)).cuda()
        torch.cuda.synchronize()

    def out(self, k):
        return self.t.data_ptr() + 34 * 8 * k

    def selected(self, k):
        return self.out(k) + 32 * 8

    def high(self, k):
        return self.out(k) + 33 * 8

    def check(self):
        import torch
        torch.cuda.synchronize()
        got = u64(self.t)
        for k, want in enumerate(self.wants):
            assert np.array_equal(got[k], want), (self.notes[k], got[k], want)


def host_call(entry, src, n, W, require, exclude, q, mn, mode, want, selected, high, note, hip):
    """a _sync or host-form call over garbage (store) or bias words (+=), all three results checked"""
    store = bool(mode & STORE)
    o = np.full(32, GARBAGE if store else BIAS, dtype=np.uint64)
    s = ctypes.c_uint64(GARBAGE if store else SEL_BIAS)
    h = ctypes.c_uint64(GARBAGE if store else HIGH_BIAS)
    rc = entry(src, n, W, require, exclude, q, mn, o.ctypes.data, ctypes.byref(s), ctypes.byref(h), mode)
    assert rc == 0, (note, err(hip))
    got = np.concatenate([o, [np.uint64(s.value)], [np.uint64(h.value)]])
    assert np.array_equal(got, expect_triple(want, selected, high, mode)), (note, got)


# ------------------------------------------------------------------ 1. every value under every kind of predicate
@pytest.mark.parametrize("dtype", ["int32", "uint32", "int64", "uint64"])
def test_every_value_under_every_kind_of_predicate(hip, oracle_mod, dtype):
    """0..65535 once each, shuffled, in a 4- or 8-byte dtype; a fixed sparse set of elements -- among them the values 0 and
    0xFFFF, which alone pass "everything excluded" and "everything required" -- also carries high bits, so under every predicate
    that can tell elements apart some carriers pass and some fail.  Under test_gpu_filter.PREDICATES, store + superset over
    garbage and += over bias words, through the device entry, the _sync form and the host form.  Cross-checks (not the oracle):
    the empty predicate is FLAGSTATS_hip_device_wide of the same tensor; a column without high bits gives
    FLAGSTATS_hip_device_u16_filter of astype(uint16)"""
    import torch
    W = np.dtype(dtype).itemsize
    low = np.random.RandomState(2025).permutation(65536).astype(np.uint64)
    carriers = sorted(set(range(11, 65536, 97)) | {int(np.flatnonzero(low == 0)[0]), int(np.flatnonzero(low == 0xFFFF)[0])})
    column = low.copy()
    for k, i in enumerate(carriers):
        column[i] |= np.uint64(1) << np.uint64(16 + (7 * k) % (8 * W - 16))
    column[carriers[3]] |= np.uint64(ALL_HIGH[W])       # a negative element / every high bit at once
    values = column.astype(UNSIGNED[W]).view(dtype)
    plain = low.astype(UNSIGNED[W]).view(dtype)
    high = wfo.want_high(values)
    assert high == ALL_HIGH[W] and wfo.want_high(plain) == 0
    wants = {p: wfo.want(oracle_mod, values, p[0], p[1], superset=True) for p in PREDICATES}
    for p in PREDICATES:
        m = filter_mask(wfo.low16(values), p[0], p[1])[carriers]
        assert p in ((0, 0), (0x0040, 0x0040)) or (m.any() and not m.all()), p
    assert wants[0, 0][1] == 65536 and wants[0x0040, 0x0040][1] == 0 and wants[0xFFFF, 0][1] == 1 and wants[0, 0xFFFF][1] == 1
    t, t_plain = to_device(values), to_device(plain)
    rows = Rows()
    plan = []
    for p in PREDICATES:
        for mode in MODES:
            plan.append((p, mode, rows.add(mode, wants[p][0], wants[p][1], overlap_high(p[0], p[1], high), ("device", dtype, p, mode))))
    rows.upload()
    for (require, exclude), mode, k in plan:
        rc = hip.FLAGSTATS_hip_device_wide_filter(t.data_ptr(), 65536, W, require, exclude, None, 0, rows.out(k), rows.selected(k),
                                                  rows.high(k), mode, None)
        assert rc == 0, (require, exclude, mode, err(hip))
    rows.check()
    for name, entry, src in (("sync", hip.FLAGSTATS_hip_device_wide_filter_sync, t.data_ptr()),
                             ("host", hip.FLAGSTATS_hip_wide_x64_filter, values.ctypes.data)):
        for p in PREDICATES:
            for mode in MODES:
                host_call(entry, src, 65536, W, p[0], p[1], None, 0, mode, wants[p][0], wants[p][1], overlap_high(p[0], p[1], high),
                          (name, dtype, p, mode), hip)
    # cross-checks against the entries that exist without this kernel
    wide = torch.zeros(33, dtype=torch.int64, device="cuda")
    assert hip.FLAGSTATS_hip_device_wide(t.data_ptr(), 65536, W, wide.data_ptr(), wide.data_ptr() + 256, STORE | SUPERSET, None) == 0, err(hip)
    mine = torch.zeros(34, dtype=torch.int64, device="cuda")
    assert hip.FLAGSTATS_hip_device_wide_filter(t.data_ptr(), 65536, W, 0, 0, None, 0, mine.data_ptr(), mine.data_ptr() + 256,
                                                mine.data_ptr() + 264, STORE | SUPERSET, None) == 0, err(hip)
    torch.cuda.synchronize()
    assert np.array_equal(u64(mine)[:32], u64(wide)[:32]) and int(u64(mine)[32]) == 65536 and u64(mine)[33] == u64(wide)[32]
    t16 = torch.from_numpy(low.astype(np.uint16).view(np.int16)).cuda()
    a = torch.zeros((len(PREDICATES), 34), dtype=torch.int64, device="cuda")
    b = torch.zeros((len(PREDICATES), 34), dtype=torch.int64, device="cuda")
    for k, (require, exclude) in enumerate(PREDICATES):
        pa, pb = a.data_ptr() + 34 * 8 * k, b.data_ptr() + 34 * 8 * k
        assert hip.FLAGSTATS_hip_device_wide_filter(t_plain.data_ptr(), 65536, W, require, exclude, None, 0, pa, pa + 256, pa + 264,
                                                    STORE | SUPERSET, None) == 0, err(hip)
        assert hip.FLAGSTATS_hip_device_u16_filter(t16.data_ptr(), 65536, require, exclude, None, 0, pb, pb + 256, STORE | SUPERSET, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(u64(a), u64(b))            # word 33 of b was never written: high == 0 on both sides


# ------------------------------------------------------------------ 2. lengths, phases, MAPQ alignments
BYTE_ALIGNMENTS = (0, 1, 3, 8, 15)


def lengths(W):
    S = STEP[W]
    return (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1, 2 * S - 1, 2 * S + 1)


@pytest.mark.parametrize("W", WIDTHS)
def test_lengths_phases_mapq_alignments(hip, oracle_mod, W):
    """every length around nothing, a vector, a wave's line and one and two steps x every element phase of a 16-byte line x {no
    MAPQ, MAPQ at byte alignments 0, 1, 3, 8, 15} x two predicates (one on the low byte plane, one on both).  The array sits in a
    slab whose surrounding elements pass the predicate AND carry every high bit, the MAPQ in a slab of 0xFF (which passes every
    threshold); the body carries no high bits: one element read outside [0, n) changes `selected`, the counters or `high`.
    Through fsk_launch_wide_filter at grids 1, 2, 3 and the public device entry, store form over garbage and += over bias."""
    LENGTHS = lengths(W)
    EPV = 16 // W
    rng = np.random.RandomState(43 + W)
    nmax = LENGTHS[-1]
    body = rng.randint(0, 65536, nmax).astype(np.uint16)
    forced = rng.randint(0, 100, nmax) < 55       # these pass both predicates
    body[forced] = (body[forced] & np.uint16(~0x0904 & 0xFFFF)) | np.uint16(0x0041)
    mapq = rng.randint(15, 60, nmax).astype(np.uint8)   # two thirds reach 30
    preds = (PRED_ONE_PLANE, PRED_BOTH_PLANES)
    wide_body = body.astype(UNSIGNED[W])
    wants = {(p, mn, n): wfo.want(oracle_mod, wide_body[:n], p[0], p[1], mapq[:n], mn, superset=True)
             for p in preds for mn in (0, 30) for n in LENGTHS}
    for (p, mn, n), (_, nsel, high) in wants.items():
        assert high == 0 and (n < 63 or 0 < nsel < n), (p, mn, n, nsel)
    arrays, a_at = [], {}
    pos = 0
    for p in preds:
        for n in LENGTHS:
            for phase in range(EPV):
                region = np.full((64 + EPV + n + 64 + EPV - 1) // EPV * EPV, (0xFFFF & ~p[1]) | ALL_HIGH[W], dtype=UNSIGNED[W])
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
                    want, nsel, high = wants[p, mn, n]
                    for grid in (1, 2, 3, None):          # None: the public device entry
                        for mode in MODES:
                            k = rows.add(mode, want, nsel, high, (W, p, n, phase, align, grid, mode))
                            calls.append((k, ptr, n, p, qptr, mn, mode, grid))
    rows.upload()
    for k, ptr, n, p, qptr, mn, mode, grid in calls:
        if grid is None:
            rc = hip.FLAGSTATS_hip_device_wide_filter(ptr if n else None, n, W, p[0], p[1], qptr if n else None, mn, rows.out(k),
                                                      rows.selected(k), rows.high(k), mode, None)
            assert rc == 0, (rows.notes[k], err(hip))
        else:
            rc = hip.fsk_launch_wide_filter(ptr if n else None, n, W, p[0], p[1], qptr if n else None, mn, rows.out(k), rows.selected(k),
                                            rows.high(k), mode, grid, None)
            assert rc == 0, (rows.notes[k], rc)
    rows.check()


# ------------------------------------------------------------------ 3. which MAPQ byte belongs to which element
def positions(W):
    S = STEP[W]
    return (tuple(range(18)) + tuple(range(62, 67)) + tuple(range(126, 131)) + tuple(range(254, 259)) + tuple(range(510, 515))
            + (S - 1, S, S + 1, 2 * S - 1))


@pytest.mark.parametrize("W,phase,align", [(4, 0, 0), (4, 3, 3), (8, 0, 0), (8, 1, 3)])
def test_which_mapq_byte_belongs_to_which_element(hip, oracle_mod, W, phase, align):
    """n = 2 STEP elements that all pass (0x0001, 0x0900); element p = 0x0041 between two 0x0081.  MAPQ 0 everywhere and 60 at p
    alone gives the row of one 0x0041; 60 everywhere and 0 at p gives the row of the column without it.  The positions 126..130
    are there for W = 8, where the four MAPQ bytes of one group of flags come from places 128 elements apart"""
    import torch
    n = 2 * STEP[W]
    require, exclude, background = 0x0001, 0x0900, 0xFFFF & ~0x0900
    one, _, _ = wfo.want(oracle_mod, np.array([0x0041], dtype=UNSIGNED[W]), require, exclude, superset=True)
    slab = to_device(np.full(64 + 16 // W + n + 64, background, dtype=UNSIGNED[W]))
    arr = slab[64 + phase:64 + phase + n]
    assert arr.data_ptr() % 16 == W * phase
    col = torch.full((16 + 16 + n + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    q = col[16 + align:16 + align + n]
    assert q.data_ptr() % 16 == align
    host = np.full(n, background, dtype=np.uint16)
    rows = Rows()
    plan = []
    for p in positions(W):
        v = host.copy()
        v[p] = 0x0041
        v[max(p - 1, 0):p] = 0x0081
        v[p + 1:p + 2] = 0x0081
        hot = np.zeros(n, dtype=bool)
        hot[p] = True
        assert filter_mask(v, require, exclude).all()
        plan.append((p, rows.add(STORE | SUPERSET, one, 1, 0, ("alone", W, phase, align, p)),
                     rows.add(STORE | SUPERSET, where_oracle.want_counters(oracle_mod, v, ~hot, superset=True), n - 1, 0,
                              ("all but", W, phase, align, p))))
    rows.upload()
    for p, k_alone, k_rest in plan:
        arr[p] = 0x0041
        if p > 0:
            arr[p - 1] = 0x0081
        if p + 1 < n:
            arr[p + 1] = 0x0081
        for k, everywhere, at_p in ((k_alone, 0, 60), (k_rest, 60, 0)):
            q.fill_(everywhere)
            q[p] = at_p
            rc = hip.fsk_launch_wide_filter(arr.data_ptr(), n, W, require, exclude, q.data_ptr(), 30, rows.out(k), rows.selected(k),
                                            rows.high(k), STORE | SUPERSET, 3, None)
            assert rc == 0, rc
        arr[max(p - 1, 0):p + 2] = background
    rows.check()


# ------------------------------------------------------------------ 4. MAPQ thresholds
THRESHOLDS = (1, 30, 127, 128, 255)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("steps", [1, 2])
def test_mapq_thresholds(hip, oracle_mod, W, steps):
    """n = STEP + 100 or 2 STEP + 100 elements one element into a 16-byte line: a head edge step and a tail edge step (the
    guarded loaders), for the longer n with a fast step between them.  Every MAPQ value occurs in the head edge step and, for
    the longer n, in the fast step.  Threshold 0 runs with a NULL column and selects everything the FLAG test passes; 256 is
    refused"""
    import torch
    from steps_oracle import StepSplit
    S = STEP[W]
    n = steps * S + 100
    rng = np.random.RandomState(29 + W)
    low = rng.randint(0, 65536, n).astype(np.uint16)
    values = low.astype(UNSIGNED[W])
    values[7] |= UNSIGNED[W](1 << 21)
    mapq = rng.randint(0, 256, n).astype(np.uint8)
    mapq[:512] = np.tile(np.arange(256, dtype=np.uint8), 2)          # every value in the head edge step ...
    if steps == 2:
        mapq[S + 10:S + 10 + 256] = np.arange(256, dtype=np.uint8)   # ... and in the fast step (elements [S - 1, 2 S - 1))
    split = StepSplit(W, n * W // 2, 1)
    assert split.head_edge and split.tail_edge and split.fast_end - split.fast_begin == steps - 1
    assert set(mapq[:S - 1].tolist()) == set(range(256))
    assert steps == 1 or set(mapq[S - 1:2 * S - 1].tolist()) == set(range(256))
    slab = to_device(np.full(16 // W + n + 8, ALL_HIGH[W] | 0xF0FF, dtype=UNSIGNED[W]))
    slab[1:1 + n] = to_device(values)
    ptr = slab.data_ptr() + W
    assert ptr % 16 == W
    col = torch.full((16 + n + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    col[16 + 5:16 + 5 + n] = dev8(mapq)
    qptr = col.data_ptr() + 16 + 5
    rows = Rows()
    calls = []
    for require, exclude in ((0, 0), (0, 0x904)):
        for mn in THRESHOLDS:
            want, nsel, high = wfo.want(oracle_mod, values, require, exclude, mapq, mn, superset=True)
            assert nsel == int((filter_mask(low, require, exclude) & (mapq.astype(np.int64) >= mn)).sum()) and 0 < nsel < n
            assert high == 1 << 21
            for mode in MODES:
                for grid in (1, None):
                    calls.append((rows.add(mode, want, nsel, high, (W, require, exclude, mn, mode, grid)), require, exclude, qptr, mn, mode, grid))
        want, nsel, high = wfo.want(oracle_mod, values, require, exclude, None, 0, superset=True)
        assert (require, exclude) != (0, 0) or nsel == n
        calls.append((rows.add(STORE | SUPERSET, want, nsel, high, (W, require, exclude, 0, "NULL column")), require, exclude, None, 0,
                      STORE | SUPERSET, None))
    k_refused = rows.add(0, np.zeros(32, dtype=np.uint64), 0, 0, "threshold 256")
    rows.upload()
    for k, require, exclude, q, mn, mode, grid in calls:
        if grid is None:
            assert hip.FLAGSTATS_hip_device_wide_filter(ptr, n, W, require, exclude, q, mn, rows.out(k), rows.selected(k), rows.high(k),
                                                        mode, None) == 0, err(hip)
        else:
            assert hip.fsk_launch_wide_filter(ptr, n, W, require, exclude, q, mn, rows.out(k), rows.selected(k), rows.high(k), mode, grid,
                                              None) == 0
    k = k_refused
    assert hip.FLAGSTATS_hip_device_wide_filter(ptr, n, W, 0, 0, qptr, 256, rows.out(k), rows.selected(k), rows.high(k), 0, None) != 0
    assert "min_mapq must be at most 255" in err(hip)
    assert hip.fsk_launch_wide_filter(ptr, n, W, 0, 0, qptr, 256, rows.out(k), rows.selected(k), rows.high(k), 0, 1, None) != 0
    rows.check()


# ------------------------------------------------------------------ 5. `high` is exact, local and blind to the predicate
@pytest.mark.parametrize("W", WIDTHS)
def test_high_is_exact_local_and_blind_to_the_predicate(hip, oracle_mod, W):
    """2 STEP + 100 elements one element into a line on 2 workgroups: a head edge step, a fast step, a tail edge step.  For every
    bit above bit 15, that bit alone on one element whose low bits FAIL the predicate, in the edge step and, separately, in the
    fast step: exactly that bit is reported, counters and `selected` are those of the column without it.  The same element made
    to pass: the same `high`.  A NULL d_high (or d_selected) leaves the other results as they are.  An overlapping pair leaves
    `high` at its bias word in the += form and stores 0"""
    S = STEP[W]
    n = 2 * S + 100
    require, exclude, mn = 0x0001, 0x0904, 30
    fails, passes = 0x0004, 0x0041
    spots = {"edge": 5, "fast": S + 77}            # elements [0, S - 1) are the head edge step, [S - 1, 2 S - 1) the fast step
    rng = np.random.RandomState(51 + W)
    low = rng.randint(0, 65536, n).astype(np.uint16)
    mapq = rng.randint(0, 61, n).astype(np.uint8)
    for at in spots.values():
        low[at] = fails
        mapq[at] = 60
    base = wfo.want(oracle_mod, low.astype(UNSIGNED[W]), require, exclude, mapq, mn, superset=True)
    assert base[2] == 0 and 0 < base[1] < n
    passing = {}
    for name, at in spots.items():
        v = low.copy()
        v[at] = passes
        passing[name] = wfo.want(oracle_mod, v.astype(UNSIGNED[W]), require, exclude, mapq, mn, superset=True)
        assert passing[name][1] == base[1] + 1
    slab = to_device(np.full(16 // W + n + 8, ALL_HIGH[W] | 0xF0FF, dtype=UNSIGNED[W]))
    slab[1:1 + n] = to_device(low.astype(UNSIGNED[W]))
    arr = slab[1:1 + n]
    assert arr.data_ptr() % 16 == W
    q = dev8(mapq)
    rows = Rows()
    plan = []
    for bit in range(16, 8 * W):
        for name, at in spots.items():
            for lowbits, want in ((fails, base), (passes, passing[name])):
                mode = MODES[(bit + at) & 1] if bit != 40 else STORE | SUPERSET       # HIGH_BIAS is bit 40
                k = rows.add(mode, want[0], want[1], 1 << bit, (W, bit, name, hex(lowbits), mode))
                plan.append((k, at, lowbits | (1 << bit), mode))
    rows.upload()
    for k, at, element, mode in plan:
        arr[at] = signed(element, W)
        rc = hip.fsk_launch_wide_filter(arr.data_ptr(), n, W, require, exclude, q.data_ptr(), mn, rows.out(k), rows.selected(k), rows.high(k),
                                        mode, 2, None)
        assert rc == 0, (rows.notes[k], rc)
        arr[at] = fails
    rows.check()
    # NULL d_high, NULL d_selected, both; an overlapping pair
    arr[spots["fast"]] = signed(fails | ALL_HIGH[W], W)
    rows = Rows()
    plan = []
    for report in ((True, False), (False, True), (False, False)):
        for mode in MODES:
            for grid in (2, None):
                plan.append((rows.add(mode, base[0], base[1], ALL_HIGH[W], (W, "NULL words", report, mode, grid), report=report), report,
                             require, exclude, mode, grid))
    for mode in MODES:
        for grid in (2, None):
            plan.append((rows.add(mode, np.zeros(32, dtype=np.uint64), 0, 0, (W, "overlap", mode, grid)), (True, True), 0x0040, 0x0140, mode, grid))
    rows.upload()
    for k, report, r, e, mode, grid in plan:
        sel = rows.selected(k) if report[0] else None
        high = rows.high(k) if report[1] else None
        if grid is None:
            assert hip.FLAGSTATS_hip_device_wide_filter(arr.data_ptr(), n, W, r, e, q.data_ptr(), mn, rows.out(k), sel, high, mode, None) == 0, err(hip)
        else:
            assert hip.fsk_launch_wide_filter(arr.data_ptr(), n, W, r, e, q.data_ptr(), mn, rows.out(k), sel, high, mode, grid, None) == 0
    rows.check()
    host = arr.cpu().numpy()
    for entry, src, col in ((hip.FLAGSTATS_hip_device_wide_filter_sync, arr.data_ptr(), q.data_ptr()),
                            (hip.FLAGSTATS_hip_wide_x64_filter, host.ctypes.data, mapq.ctypes.data)):
        for mode in MODES:
            host_call(entry, src, n, W, 0x0040, 0x0140, col, mn, mode, np.zeros(32, dtype=np.uint64), 0, 0, ("overlap", W, mode), hip)
            host_call(entry, src, n, W, require, exclude, col, mn, mode, base[0], base[1], ALL_HIGH[W], ("blind", W, mode), hip)
            o = np.full(32, GARBAGE if mode & STORE else BIAS, dtype=np.uint64)
            assert entry(src, n, W, require, exclude, col, mn, o.ctypes.data, None, None, mode) == 0, err(hip)
            assert np.array_equal(o, expect_row(base[0], mode))


# ------------------------------------------------------------------ 6. epochs
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("min_mapq", [0, 30])
def test_epochs(hip, oracle_mod, W, min_mapq):
    """one workgroup over 258 STEP + 3 elements: 258 fast steps and a tail edge step, so every wave passes its staggered first
    flush (after 255, 191, 127 and 63 pushes) and wave 0 a full epoch of 255 steps"""
    n = 258 * STEP[W] + 3
    pattern = np.random.RandomState(305).randint(0, 65536, 65_521).astype(np.uint16)
    values = np.resize(pattern, n).astype(UNSIGNED[W])
    values[n // 2] |= UNSIGNED[W](1 << 16)
    values[n - 2] |= UNSIGNED[W](1 << (8 * W - 1))
    mapq = np.resize(np.random.RandomState(306).randint(0, 61, 65_519).astype(np.uint8), n)
    want, nsel, high = wfo.want(oracle_mod, values, 0x0001, 0x0804, mapq, min_mapq, superset=True)
    assert 0 < nsel < n and high == (1 << 16) | (1 << (8 * W - 1))
    t = to_device(values)
    q = dev8(mapq)
    assert t.data_ptr() % 16 == 0
    rows = Rows()
    ks = [rows.add(mode, want, nsel, high, (W, min_mapq, mode)) for mode in MODES]
    rows.upload()
    for k in ks:
        rc = hip.fsk_launch_wide_filter(t.data_ptr(), n, W, 0x0001, 0x0804, q.data_ptr() if min_mapq else None, min_mapq, rows.out(k),
                                        rows.selected(k), rows.high(k), rows.modes[k], 1, None)
        assert rc == 0, rc
    rows.check()


# ------------------------------------------------------------------ 7. atomics
def test_three_streams_add_into_one_triple(hip, oracle_mod):
    import torch
    from libflagstats_amd import wide_filter
    rng = np.random.RandomState(73)
    out = torch.zeros(32, dtype=torch.int64, device="cuda")
    selected = torch.zeros(1, dtype=torch.int64, device="cuda")
    high = torch.zeros(1, dtype=torch.int64, device="cuda")
    total, total_sel, total_high = np.zeros(32, dtype=np.uint64), 0, 0
    inputs = []
    for W, n, require, exclude, mn, bit in ((4, 40 * STEP[4] + 11, 0, 0x904, 30, 17), (8, 37 * STEP[8] + 5, 0x2, 0x900, 0, 45),
                                            (4, 43 * STEP[4] - 3, 0x0101, 0x8080, 200, 31)):
        values = rng.randint(0, 65536, n).astype(UNSIGNED[W])
        values[n // 3] |= UNSIGNED[W](1 << bit)
        mapq = rng.randint(0, 256, n).astype(np.uint8)
        want, nsel, h = wfo.want(oracle_mod, values, require, exclude, mapq, mn, superset=True)
        assert nsel > 0 and h == 1 << bit
        total += want
        total_sel += nsel
        total_high |= h
        inputs.append((to_device(values), require, exclude, dev8(mapq) if mn else None, mn))
    streams = [torch.cuda.Stream() for _ in inputs]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    for st, (t, require, exclude, q, mn) in zip(streams, inputs):
        with torch.cuda.stream(st):
            wide_filter.count_torch_ints_filter(t, require=require, exclude=exclude, mapq=q, min_mapq=mn, out=out, selected=selected,
                                                high=high, superset=True)
    for st in streams:
        st.synchronize()
    assert np.array_equal(u64(out), total) and int(u64(selected)[0]) == total_sel and int(u64(high)[0]) == total_high


# ------------------------------------------------------------------ 8. host form across chunks
@pytest.mark.parametrize("W", WIDTHS)
def test_host_form_across_chunks(hip, oracle_mod, W):
    """chunks of 8,192 uint16's worth of bytes (4,096 or 2,048 elements), five of them and a ragged tail, with and without the
    MAPQ column; a high bit in the fourth chunk only"""
    from libflagstats_amd import _lib, wide_filter
    per_chunk = 8192 * 2 // W
    n = 5 * per_chunk + 77
    rng = np.random.RandomState(89 + W)
    values = rng.randint(0, 65536, n).astype(UNSIGNED[W])
    values[3 * per_chunk + 9] = UNSIGNED[W](0x0004 | (1 << (8 * W - 2)))         # fails the FLAG test below
    values = values.view(SIGNED[W])
    mapq = rng.randint(0, 60, n).astype(np.uint8)
    require, exclude = 0x0001, 0x0804
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", 8192), "chunk_flags")
        for q, mn in ((None, 0), (mapq, 30)):
            wants = {sup: wfo.want(oracle_mod, values, require, exclude, q, mn, superset=bool(sup)) for sup in (0, SUPERSET)}
            _, nsel, high = wants[0]
            assert 0 < nsel < n and high == 1 << (8 * W - 2)
            for sup in (0, SUPERSET):
                got, selected, h = wide_filter.counters_ints_filter(values, require, exclude, mapq=q, min_mapq=mn, superset=bool(sup))
                assert np.array_equal(got, wants[sup][0]) and selected == nsel and h == high, (mn, sup)
            for flags in (0, SUPERSET):                  # += over bias words
                host_call(hip.FLAGSTATS_hip_wide_x64_filter, values.ctypes.data, n, W, require, exclude, q.ctypes.data if mn else None, mn,
                          flags, wants[SUPERSET][0], nsel, high, (W, mn, flags), hip)
            # the chunks without the carrier report nothing
            got, selected, h = wide_filter.counters_ints_filter(values[:3 * per_chunk], require, exclude,
                                                                mapq=None if q is None else q[:3 * per_chunk], min_mapq=mn)
            assert h == 0 and selected == wfo.want(oracle_mod, values[:3 * per_chunk], require, exclude, q if q is None else q[:3 * per_chunk], mn)[1]
            # one chunk only (a single staging slot), the MAPQ column from an odd host address
            sub, subq = values[2:101], None if q is None else q[1:100]
            assert subq is None or subq.ctypes.data % 2 == 1
            got, selected, h = wide_filter.counters_ints_filter(sub, require, exclude, mapq=subq, min_mapq=mn)
            want, nsel1, high1 = wfo.want(oracle_mod, sub, require, exclude, subq, mn)
            assert np.array_equal(got, want) and selected == nsel1 and h == high1 == 0
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old
    # n == 0: += touches nothing, store writes zeros; NULL pointers are accepted
    for entry in (hip.FLAGSTATS_hip_wide_x64_filter, hip.FLAGSTATS_hip_device_wide_filter_sync):
        for mn in (0, 30):
            o = np.full(32, BIAS, dtype=np.uint64)
            s, h = ctypes.c_uint64(5), ctypes.c_uint64(6)
            assert entry(None, 0, W, 1, 4, None, mn, o.ctypes.data, ctypes.byref(s), ctypes.byref(h), 0) == 0
            assert (o == BIAS).all() and s.value == 5 and h.value == 6
            assert entry(None, 0, W, 1, 4, None, mn, o.ctypes.data, ctypes.byref(s), ctypes.byref(h), STORE) == 0
            assert not o.any() and s.value == 0 and h.value == 0
    got, selected, h = wide_filter.counters_ints_filter(values[:0], 1, 4, mapq=mapq[:0], min_mapq=30)
    assert not got.any() and selected == 0 and h == 0
    got, selected, h = wide_filter.count_device_ptr_ints_filter(0, 0, W, 1, 4)
    assert not got.any() and selected == 0 and h == 0


# ------------------------------------------------------------------ 9. refusals that need a device
def test_device_dependent_refusals(hip):
    """what the C entries and the launcher refuse: the lists of test_gpu_wide.test_device_refusals and
    test_gpu_filter.test_device_dependent_refusals.  Every one is an argument check that returns before anything is launched,
    and the outputs stay as they were"""
    import torch
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

    def refused(what, text, d_array=p8, n_=n, eb=8, require=0, exclude=0x904, d_mapq=q.data_ptr(), mn=30, flags=0, counters=True,
                forms=("device", "sync", "host")):
        for form in forms:
            if form == "device":
                rc = hip.FLAGSTATS_hip_device_wide_filter(d_array, n_, eb, require, exclude, d_mapq, mn, out.data_ptr() if counters else None,
                                                          sel.data_ptr(), high.data_ptr(), flags, None)
            elif form == "sync":
                rc = hip.FLAGSTATS_hip_device_wide_filter_sync(d_array, n_, eb, require, exclude, d_mapq, mn,
                                                               h_out.ctypes.data if counters else None, ctypes.byref(h_sel),
                                                               ctypes.byref(h_high), flags)
            else:
                src = host.ctypes.data + (d_array - p8) % 8 if d_array else None
                rc = hip.FLAGSTATS_hip_wide_x64_filter(src, n_, eb, require, exclude, host8.ctypes.data if d_mapq else None, mn,
                                                       h_out.ctypes.data if counters else None, ctypes.byref(h_sel), ctypes.byref(h_high),
                                                       flags)
            assert rc != 0, (what, form)
            assert text in err(hip), (what, form, err(hip))
        untouched(what)

    # the wide entries' list
    refused("elem_bytes 2", "u16 filter entries", eb=2)
    refused("elem_bytes 3", "elem_bytes must be 4 or 8", eb=3)
    refused("elem_bytes 16", "elem_bytes must be 4 or 8", eb=16)
    refused("off by 2 at W = 4", "4-byte aligned", d_array=p8 + 2, eb=4)
    refused("off by 4 at W = 8", "8-byte aligned", d_array=p8 + 4, eb=8)
    refused("an extra flag bit", "no other bits", flags=4)
    refused("NULL array", "NULL array with n > 0", d_array=None, eb=4)
    refused("n * elem_bytes is no size", "n * elem_bytes is not a size", n_=1 << 62)
    # the filter entries' list
    for W in WIDTHS:
        refused("require above 16 bits", "require must be a 16-bit FLAG mask", d_array=bufs[W].data_ptr(), eb=W, require=0x10000)
        refused("exclude above 16 bits", "exclude must be a 16-bit FLAG mask", d_array=bufs[W].data_ptr(), eb=W, exclude=0x10000)
        refused("min_mapq above a byte", "min_mapq must be at most 255", d_array=bufs[W].data_ptr(), eb=W, mn=256)
        refused("NULL mapq", "NULL mapq with min_mapq > 0 and n > 0", d_array=bufs[W].data_ptr(), eb=W, d_mapq=None)
        refused("NULL counters", "NULL counters", d_array=bufs[W].data_ptr(), eb=W, counters=False)
        # a wave's uint32 totals: 2^60 elements on any grid this device launches.  The host form launches per chunk and cannot
        # reach the limit, so it has nothing to refuse here
        refused("a wave's totals", "a wave's uint32 totals", d_array=bufs[W].data_ptr(), eb=W, n_=1 << 60, mn=0, d_mapq=None,
                forms=("device", "sync"))
    # host memory where device memory is needed: the array, the column, d_out (pageable, then page-locked), d_selected, d_high
    for W in WIDTHS:
        pw = bufs[W].data_ptr()
        rc = hip.FLAGSTATS_hip_device_wide_filter(host.ctypes.data, n, W, 0, 0x904, q.data_ptr(), 30, out.data_ptr(), sel.data_ptr(),
                                                  high.data_ptr(), 0, None)
        assert rc != 0 and "d_array" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_filter_sync(host.ctypes.data, n, W, 0, 0x904, q.data_ptr(), 30, h_out.ctypes.data,
                                                       ctypes.byref(h_sel), ctypes.byref(h_high), 0)
        assert rc != 0 and "d_array" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_filter(pw, n, W, 0, 0x904, host8.ctypes.data, 30, out.data_ptr(), sel.data_ptr(),
                                                  high.data_ptr(), 0, None)
        assert rc != 0 and "d_mapq" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_filter_sync(pw, n, W, 0, 0x904, host8.ctypes.data, 30, h_out.ctypes.data, ctypes.byref(h_sel),
                                                       ctypes.byref(h_high), 0)
        assert rc != 0 and "d_mapq" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_filter(pw, n, W, 0, 0x904, q.data_ptr(), 30, h_out.ctypes.data, sel.data_ptr(), high.data_ptr(), 0, None)
        assert rc != 0 and "d_out" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_filter(pw, n, W, 0, 0x904, q.data_ptr(), 30, out.data_ptr(), ctypes.addressof(h_sel),
                                                  high.data_ptr(), 0, None)
        assert rc != 0 and "d_selected" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_filter(pw, n, W, 0, 0x904, q.data_ptr(), 30, out.data_ptr(), sel.data_ptr(),
                                                  ctypes.addressof(h_high), 0, None)
        assert rc != 0 and "d_high" in err(hip), err(hip)
    pinned = hip.FLAGSTATS_hip_host_alloc(512)
    assert pinned
    try:
        ctypes.memset(pinned, 0, 512)
        rc = hip.FLAGSTATS_hip_device_wide_filter(p8, n, 8, 0, 0x904, q.data_ptr(), 30, pinned, sel.data_ptr(), high.data_ptr(), STORE, None)
        assert rc != 0 and "d_out must be device memory" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_filter(p8, n, 8, 0, 0x904, q.data_ptr(), 30, out.data_ptr(), pinned, high.data_ptr(), STORE, None)
        assert rc != 0 and "d_selected must be device memory" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_filter(p8, n, 8, 0, 0x904, q.data_ptr(), 30, out.data_ptr(), sel.data_ptr(), pinned, STORE, None)
        assert rc != 0 and "d_high must be device memory" in err(hip), err(hip)
        assert not any(ctypes.string_at(pinned, 512))
    finally:
        hip.FLAGSTATS_hip_host_free(pinned)
    untouched("host pointers")
    # extents: counters 8 bytes short; an array one element short; a column one byte short of n (not looked at without a threshold)
    nbytes = 2 << 20
    raw = hip.FLAGSTATS_hip_device_alloc(nbytes)
    assert raw
    try:
        assert hip.FLAGSTATS_hip_memcpy_h2d(raw, np.zeros(nbytes, dtype=np.uint8).ctypes.data, nbytes) == 0
        rc = hip.FLAGSTATS_hip_device_wide_filter(p8, n, 8, 0, 0x904, q.data_ptr(), 30, raw + nbytes - 248, sel.data_ptr(), high.data_ptr(), 0, None)
        assert rc != 0 and "d_out" in err(hip) and "8 bytes short" in err(hip), err(hip)
        for W in WIDTHS:
            big = torch.zeros(nbytes + 8, dtype={4: torch.int32, 8: torch.int64}[W], device="cuda")
            rc = hip.FLAGSTATS_hip_device_wide_filter(raw, nbytes // W + 1, W, 0, 0x904, None, 0, out.data_ptr(), sel.data_ptr(),
                                                      high.data_ptr(), STORE, None)
            assert rc != 0 and "d_array" in err(hip) and "%d bytes short" % W in err(hip), err(hip)
            rc = hip.FLAGSTATS_hip_device_wide_filter_sync(raw + W, nbytes // W, W, 0, 0x904, None, 0, h_out.ctypes.data, ctypes.byref(h_sel),
                                                           ctypes.byref(h_high), STORE)
            assert rc != 0 and "d_array" in err(hip) and "%d bytes short" % W in err(hip), err(hip)
            rc = hip.FLAGSTATS_hip_device_wide_filter(big.data_ptr(), nbytes + 1, W, 0, 0x904, raw, 30, out.data_ptr(), sel.data_ptr(),
                                                      high.data_ptr(), STORE, None)
            assert rc != 0 and "d_mapq" in err(hip) and "1 bytes short" in err(hip), err(hip)
            rc = hip.FLAGSTATS_hip_device_wide_filter_sync(big.data_ptr(), nbytes + 1, W, 0, 0x904, raw, 30, h_out.ctypes.data,
                                                           ctypes.byref(h_sel), ctypes.byref(h_high), STORE)
            assert rc != 0 and "d_mapq" in err(hip) and "1 bytes short" in err(hip), err(hip)
            untouched("extents")
            for n_ok, mn in ((nbytes, 30), (nbytes + 1, 0)):
                o = np.full(32, BIAS, dtype=np.uint64)
                s, h = ctypes.c_uint64(SEL_BIAS), ctypes.c_uint64(HIGH_BIAS)
                assert hip.FLAGSTATS_hip_device_wide_filter_sync(big.data_ptr(), n_ok, W, 0, 0x904, raw, mn, o.ctypes.data, ctypes.byref(s),
                                                                 ctypes.byref(h), STORE) == 0, err(hip)
                assert not o.any() and s.value == (0 if mn else n_ok) and h.value == 0     # zeros pass -F 0x904 and count nothing; MAPQ 0 < 30
    finally:
        hip.FLAGSTATS_hip_device_free(raw)
    untouched("extents")
    # the launcher itself: other widths, misalignment, other mode bits, no workgroups, a wave's uint32 totals, predicates out of
    # range, a NULL column under a threshold -- nothing queued
    words = torch.full((34,), BIAS, dtype=torch.int64, device="cuda")
    p = words.data_ptr()
    f = hip.fsk_launch_wide_filter
    for W in WIDTHS:
        pw = bufs[W].data_ptr()
        assert f(pw, 8, W, 0, 0x904, q.data_ptr(), 30, p, p + 256, p + 264, 4, 1, None) != 0
        assert f(pw, 8, W, 0, 0x904, q.data_ptr(), 30, p, p + 256, p + 264, 0, 0, None) != 0
        assert f(pw, 1 << 35, W, 0, 0x904, None, 0, p, p + 256, p + 264, STORE, 1, None) != 0
        assert f(pw, 8, W, 0x10000, 0, None, 0, p, p + 256, p + 264, STORE, 1, None) != 0
        assert f(pw, 8, W, 0, 0x10000, None, 0, p, p + 256, p + 264, STORE, 1, None) != 0
        assert f(pw, 8, W, 0, 0, None, 30, p, p + 256, p + 264, STORE, 1, None) != 0
        assert f(pw, 8, W, 0, 0, q.data_ptr(), 256, p, p + 256, p + 264, STORE, 1, None) != 0
        assert f(pw + W // 2, 8, W, 0, 0, None, 0, p, p + 256, p + 264, STORE, 1, None) != 0
        assert f(pw, 8, W, 0, 0, None, 0, None, p + 256, p + 264, STORE, 1, None) != 0
    for eb in (0, 1, 2, 3, 16):
        assert f(p4, 8, eb, 0, 0, None, 0, p, p + 256, p + 264, STORE, 1, None) != 0
    torch.cuda.synchronize()
    assert (words == BIAS).all()


# ------------------------------------------------------------------ 10. the Python layers
def test_python_layers(hip, oracle_mod):
    """numpy over all six dtypes (the 2-byte ones take the uint16 route and report high == 0), strict and its message, the dict;
    the raw-pointer form; the torch layer's dtypes, shapes, placement and its device-mismatch refusals"""
    import torch
    from libflagstats_amd import wide, wide_filter
    n = 3 * STEP[4] + 41
    rng = np.random.RandomState(97)
    low = rng.randint(0, 65536, n).astype(np.uint16)
    mapq = rng.randint(0, 61, n).astype(np.uint8)
    require, exclude, mn = 0x0001, 0x0904, 30
    want, nsel, _ = wfo.want(oracle_mod, low.astype(np.uint32), require, exclude, mapq, mn)
    want_sup = wfo.want(oracle_mod, low.astype(np.uint32), require, exclude, mapq, mn, superset=True)[0]
    assert 0 < nsel < n
    for dt in ("int16", "uint16", "int32", "uint32", "int64", "uint64"):
        v = low.astype({"int16": np.uint16}.get(dt, dt)).view(dt)
        got, selected, high = wide_filter.counters_ints_filter(v, require, exclude, mapq=mapq, min_mapq=mn)
        assert got.dtype == np.uint64 and np.array_equal(got, want) and selected == nsel and high == 0, dt
        got, selected, high = wide_filter.counters_ints_filter(v, require, exclude, mapq=mapq, min_mapq=mn, superset=True)
        assert np.array_equal(got, want_sup) and selected == nsel and high == 0, dt
        d = wide_filter.flagstats_ints_filter(v, require, exclude, mapq=mapq, min_mapq=mn)
        assert d["n_values"] == nsel and int(d["failed"]["FQCFAIL"]) == int(want[25]) and "high_bits" not in d
        assert int(d["passed"]["mapped"]) == nsel - int(want[2]) - int(want[18])
        assert wide_filter.flagstats_ints_filter(v, require, exclude, mapq=mapq, min_mapq=mn, strict=False)["high_bits"] == 0
        if v.dtype.itemsize == 2:
            continue
        # one element that FAILS the predicate carries a bit above bit 15: strict refuses the column all the same
        W = v.dtype.itemsize
        bad = v.copy()
        at = int(np.flatnonzero(~filter_mask(low, require, exclude, mapq, mn))[5])
        bad.view(UNSIGNED[W])[at] |= UNSIGNED[W](1 << (8 * W - 1))
        mask = 1 << (8 * W - 1)
        with pytest.raises(ValueError) as e:
            wide_filter.flagstats_ints_filter(bad, require, exclude, mapq=mapq, min_mapq=mn)
        assert str(e.value) == wide.high_bits_message(mask)
        d = wide_filter.flagstats_ints_filter(bad, require, exclude, mapq=mapq, min_mapq=mn, strict=False)
        assert d["high_bits"] == mask and d["n_values"] == nsel and int(d["failed"]["FQCFAIL"]) == int(want[25])
        # the raw-pointer form and the torch layer on the same column
        t, q = to_device(bad), dev8(mapq)
        got, selected, high = wide_filter.count_device_ptr_ints_filter(t.data_ptr(), n, W, require, exclude, mapq_ptr=q.data_ptr(), min_mapq=mn,
                                                                       superset=True)
        assert np.array_equal(got, want_sup) and selected == nsel and high == mask
        o, s, h = wide_filter.count_torch_ints_filter(t, require, exclude, mapq=q, min_mapq=mn)
        torch.cuda.synchronize()
        for x, numel in ((o, 32), (s, 1), (h, 1)):
            assert x.dtype == torch.int64 and tuple(x.shape) == (numel,) and x.device == t.device
        assert np.array_equal(u64(o), want) and int(u64(s)[0]) == nsel and int(u64(h)[0]) == mask
        o2, s2, h2 = wide_filter.count_torch_ints_filter(t, require, exclude, mapq=q, min_mapq=mn, out=o, selected=s, high=h)   # += and |=
        assert o2 is o and s2 is s and h2 is h
        torch.cuda.synchronize()
        assert np.array_equal(u64(o), 2 * want) and int(u64(s)[0]) == 2 * nsel and int(u64(h)[0]) == mask
        wide_filter.count_torch_ints_filter(t, require, exclude, mapq=q, min_mapq=mn, out=o, selected=s, high=h, store=True, superset=True)
        torch.cuda.synchronize()
        assert np.array_equal(u64(o), want_sup) and int(u64(s)[0]) == nsel and int(u64(h)[0]) == mask
    # a 2-byte tensor takes the uint16 entry: `high` is left as it is, zeroed with store
    t16 = torch.from_numpy(low.view(np.int16)).cuda()
    q = dev8(mapq)
    h = torch.full((1,), 9, dtype=torch.int64, device="cuda")
    o, s, h2 = wide_filter.count_torch_ints_filter(t16, require, exclude, mapq=q, min_mapq=mn, high=h)
    torch.cuda.synchronize()
    assert h2 is h and int(h[0]) == 9 and np.array_equal(u64(o), want) and int(u64(s)[0]) == nsel
    wide_filter.count_torch_ints_filter(t16, require, exclude, mapq=q, min_mapq=mn, out=o, selected=s, high=h, store=True)
    torch.cuda.synchronize()
    assert int(h[0]) == 0 and np.array_equal(u64(o), want) and int(u64(s)[0]) == nsel
    # an empty tensor
    o, s, h = wide_filter.count_torch_ints_filter(torch.zeros(0, dtype=torch.int32, device="cuda"), 1, 4)
    torch.cuda.synchronize()
    assert not u64(o).any() and int(s[0]) == 0 and int(h[0]) == 0
    # results somewhere else than t
    t = to_device(low.astype(np.uint32))
    with pytest.raises(ValueError, match=r"mapq must live on t's device \(cuda:0\), not on cpu"):
        wide_filter.count_torch_ints_filter(t, mapq=torch.zeros(n, dtype=torch.uint8), min_mapq=30)
    with pytest.raises(ValueError, match=r"out must live on t's device \(cuda:0\), not on cpu"):
        wide_filter.count_torch_ints_filter(t, mapq=q, min_mapq=30, out=torch.zeros(32, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"selected must live on t's device \(cuda:0\), not on cpu"):
        wide_filter.count_torch_ints_filter(t, mapq=q, min_mapq=30, selected=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"high must live on t's device \(cuda:0\), not on cpu"):
        wide_filter.count_torch_ints_filter(t, mapq=q, min_mapq=30, high=torch.zeros(1, dtype=torch.int64))
