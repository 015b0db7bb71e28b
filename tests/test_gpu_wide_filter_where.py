"""The filtered and selected flagstat of int32 / int64 columns on the MI355X: fsk::flagstat_count_wide_filter_where at both
widths, with and without a MAPQ column and in both encodings of the selection, the three C entries and
libflagstats_amd/wide_filter_where.py.

Expected values never come from the code under test: wide_filter_where_oracle.want is oracle.flagstat_c of the low 16 bits of
values[filter_mask & mask] (superset slots from oracle.samtools_counts and the definition), `selected` is that mask's sum and
`high` is the OR of values[mask] with the low 16 bits cleared -- of the SELECTED elements, passing or not.

One poison cannot catch both kinds of leak (0xFFFF fails -F 0x904 anyway, so a leaked selection bit would go unseen), so there
are two kinds of decoy.  Decoy A: elements that are not selected, and the slab around the array, hold a value that PASSES the
predicate under test, with every bit above bit 15 set and MAPQ 255 -- one leaked selection bit changes `selected`, the counters
and `high`.  Decoy B: selected elements that FAIL carry FLAG bits no passing element has (an excluded bit), or a MAPQ just below
min_mapq, and some carry chosen high bits, which must show up in `high`.  The slabs around the MAPQ column hold 255, the slabs
around the selection all-ones."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_filter_where_oracle as wfwo  # noqa: E402
import wide_where_oracle as wwo  # noqa: E402
from test_gpu_wide_filter import (ALL_HIGH, BIAS, GARBAGE, HIGH_BIAS, MODES, SEL_BIAS, SIGNED, STEP, UNSIGNED, WIDTHS, Rows, dev8,  # noqa: E402
                                  err, expect_row, expect_triple, signed, to_device, u64)
from test_gpu_wide_where import BYTE_ALIGNMENTS, ENCODINGS, ROW, Packer, lengths, selection  # noqa: E402
from wide_where_oracle import BITMAP, BYTES, pack  # noqa: E402

pytestmark = pytest.mark.gpu

STORE, SUPERSET = 1, 2
PRED_F = (0, 0x0904, 0)                       # -F 0x904
PRED_FQ = (0x0002, 0x0904, 30)                # -f 0x2 -F 0x904 -q 30
PREDS = (PRED_F, PRED_FQ)
MAPQ_ALIGNMENTS = (0, 1, 3)
MQ_PAD = 16                                   # bytes of 255 around every MAPQ column
ZEROS = np.zeros(32, dtype=np.uint64)


def decoy_a(W, pred=PRED_FQ):
    """an element that passes `pred` on its low 16 bits (paired, proper, read1 and whatever is required) and has every bit above
    bit 15 set"""
    low = (pred[0] | 0x0043) & ~pred[1] & 0xFFFF
    assert (low & pred[0]) == pred[0] and not low & pred[1]
    return UNSIGNED[W](ALL_HIGH[W] | low)


def make_column(rng, n, W, mask, low=None, plant=True):
    """(values as unsigned W-byte, mapq) under `mask`: selected elements hold `low` (random FLAGs where not given) and a MAPQ
    around 30 (0, 29, 30, 31 or 255); elements that are not selected are decoy A with MAPQ 255.  plant: a chosen high bit on two
    selected elements that fail -F 0x904 and on one that passes -f 0x2 -F 0x904 -q 30 (where the column has such elements)"""
    m = np.asarray(mask, dtype=bool)
    v = (rng.randint(0, 65536, n) if low is None else np.asarray(low)).astype(UNSIGNED[W])
    q = np.array([0, 29, 30, 31, 255], dtype=np.uint8)[rng.randint(0, 5, n)]
    if plant:
        fails = np.flatnonzero(m & ((v & UNSIGNED[W](0x0904)) != 0))
        passes = np.flatnonzero(wfwo.counted_mask(v, m, *PRED_FQ[:2], q, PRED_FQ[2]))
        for k, i in enumerate(list(fails[:1]) + list(fails[-1:]) + list(passes[len(passes) // 2:len(passes) // 2 + 1])):
            v[i] |= UNSIGNED[W](1 << (16 + (5 * k + int(i)) % (8 * W - 16)))
    v[~m] = decoy_a(W)
    q[~m] = 255
    return v, q


def mapq_slab(q, align):
    """the host bytes of a MAPQ column `align` bytes past a 16-byte boundary of a slab of 255s, and its offset in the slab"""
    slab = np.full((MQ_PAD + 16 + q.size + MQ_PAD + 15) // 16 * 16, 255, dtype=np.uint8)
    slab[MQ_PAD + align:MQ_PAD + align + q.size] = q
    return slab, MQ_PAD + align


def launch(hip, grid, ptr, n, W, pred, mq, sel, off, enc, rows, k, mode):
    """through fsk_launch_wide_filter_where at `grid` workgroups, or (grid None) the public device entry; on the null stream"""
    require, exclude, mn = pred
    args = (ptr if n else None, n, W, require, exclude, mq if n and mn else None, mn, sel if n else None, off, enc, rows.out(k),
            rows.selected(k), rows.high(k), mode)
    if grid is None:
        rc = hip.FLAGSTATS_hip_device_wide_filter_where(*args, None)
        assert rc == 0, (rows.notes[k], err(hip))
    else:
        rc = hip.fsk_launch_wide_filter_where(*args, grid, None)
        assert rc == 0, (rows.notes[k], rc)


def host_call(entry, src, n, W, pred, q, sel, off, enc, mode, want, selected, high, note, hip):
    """a _sync or host-form call over garbage (store) or bias words (+=), all three results checked"""
    store = bool(mode & STORE)
    o = np.full(32, GARBAGE if store else BIAS, dtype=np.uint64)
    s = ctypes.c_uint64(GARBAGE if store else SEL_BIAS)
    h = ctypes.c_uint64(GARBAGE if store else HIGH_BIAS)
    rc = entry(src, n, W, pred[0], pred[1], q if pred[2] else None, pred[2], sel, off, enc, o.ctypes.data, ctypes.byref(s), ctypes.byref(h),
               mode)
    assert rc == 0, (note, err(hip))
    got = np.concatenate([o, [np.uint64(s.value)], [np.uint64(h.value)]])
    assert np.array_equal(got, expect_triple(want, selected, high, mode)), (note, got)


def want_of(oracle_mod, values, mask, pred, mapq, superset=True):
    return wfwo.want(oracle_mod, values, mask, pred[0], pred[1], mapq if pred[2] else None, pred[2], superset=superset)


# ------------------------------------------------------------------ 1. every FLAG value through every form
@pytest.mark.parametrize("dtype", ["int32", "uint32", "int64", "uint64"])
def test_every_flag_value_through_every_form(hip, oracle_mod, dtype):
    """0..65535 once each, selected, shuffled among 65,536 decoys A; under -F 0x904 and -f 0x2 -F 0x904 -q 30.  Bitmap (5 bits
    into its first byte) and bytes, store + superset over garbage and += over bias words, through the device entry, the _sync
    form and the host form; a second += call adds; n == 0 in both modes"""
    W = np.dtype(dtype).itemsize
    rng = np.random.RandomState(2027)
    n = 131072
    mask = np.zeros(n, dtype=bool)
    mask[rng.permutation(n)[:65536]] = True
    low = np.zeros(n, dtype=np.uint64)
    low[mask] = rng.permutation(65536)
    column, q = make_column(rng, n, W, mask, low)
    values = column.view(dtype)
    assert np.array_equal(np.sort(wwo.low16(values)[mask]), np.arange(65536))
    wants = {pred: want_of(oracle_mod, values, mask, pred, q) for pred in PREDS}
    for pred in PREDS:
        _, nsel, high = wants[pred]
        assert 0 < nsel < 65536 and high not in (0, ALL_HIGH[W])
        assert high & ~wfwo.want_high(values, wfwo.counted_mask(values, mask, pred[0], pred[1], q, pred[2]))   # a failing carrier
    assert wants[PRED_FQ][1] < wants[PRED_F][1]
    t = to_device(values)
    q_host, q_at = mapq_slab(q, 1)
    d_q = dev8(q_host)
    sels = {}
    for enc in ENCODINGS:
        host, at, off = selection(mask, enc, 5)
        sels[enc] = (host, dev8(host), at, off)
    rows = Rows()
    plan = []
    for pred in PREDS:
        want, nsel, high = wants[pred]
        for enc in ENCODINGS:
            for mode in MODES:
                plan.append((pred, enc, mode, n, rows.add(mode, want, nsel, high, ("device", dtype, pred, enc, mode)), 1))
            plan.append((pred, enc, 0, n, rows.add(0, 2 * want, 2 * nsel, high, ("device twice", dtype, pred, enc)), 2))
            for mode in MODES:
                plan.append((pred, enc, mode, 0, rows.add(mode, ZEROS, 0, 0, ("n == 0", dtype, pred, enc, mode)), 1))
    rows.upload()
    for pred, enc, mode, n_, k, times in plan:
        _, d, at, off = sels[enc]
        for _ in range(times):
            launch(hip, None, t.data_ptr(), n_, W, pred, d_q.data_ptr() + q_at, d.data_ptr() + at, off, enc, rows, k, mode)
    rows.check()
    for name, entry, src, mq in (("sync", hip.FLAGSTATS_hip_device_wide_filter_where_sync, t.data_ptr(), d_q.data_ptr() + q_at),
                                 ("host", hip.FLAGSTATS_hip_wide_x64_filter_where, values.ctypes.data, q_host.ctypes.data + q_at)):
        for pred in PREDS:
            want, nsel, high = wants[pred]
            for enc in ENCODINGS:
                host, d, at, off = sels[enc]
                sel = d.data_ptr() + at if name == "sync" else host.ctypes.data + at
                for mode in MODES:
                    host_call(entry, src, n, W, pred, mq, sel, off, enc, mode, want, nsel, high, (name, dtype, pred, enc, mode), hip)
                    host_call(entry, None, 0, W, pred, None, None, off, enc, mode, ZEROS, 0, 0, (name, "n == 0", pred, enc, mode), hip)


# ------------------------------------------------------------------ 2. lengths, phases and offsets
@pytest.mark.parametrize("W", WIDTHS)
def test_lengths_phases_and_offsets(hip, oracle_mod, W):
    """every length around nothing, a vector, a selection byte, a wave's row and one and two steps x every element phase of a
    16-byte line x {bitmap at bit offsets 0..7, bytes at alignments 0, 1, 3, 8, 15}, each through fsk_launch_wide_filter_where at
    grids 1, 2, 3 and the public entry; MAPQ alignments 0, 1, 3, with and without -q and both modes rotate against the grids so
    that every pairing occurs.  The array sits in a slab of decoys A, the MAPQ column in a slab of 255, the selection in a slab of
    all-ones: one element, MAPQ byte or selection bit taken from outside [0, n), or from the wrong place, changes the results"""
    LENGTHS = lengths(W)
    EPV = 16 // W
    rng = np.random.RandomState(59 + W)
    nmax = LENGTHS[-1]
    mask = rng.randint(0, 2, nmax).astype(bool)
    mask[:18] = [1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1, 0, 1]
    body, q = make_column(rng, nmax, W, mask, plant=False)
    # the first elements by hand: 0 passes both predicates, 2 fails both on its FLAG, 3 passes -F 0x904 and lacks the required bit
    body[0], body[2], body[3] = 0x0043, 0x0143, 0x0041
    q[:18] = np.where(mask[:18], [30, 0, 29, 31, 0, 0, 255, 0, 30, 29, 30, 0, 0, 31, 0, 29, 0, 30], 255)
    wants = {(n, pred): want_of(oracle_mod, body[:n], mask[:n], pred, q[:n]) for n in LENGTHS for pred in PREDS}
    for n in LENGTHS:
        assert n < 4 or 0 < wants[n, PRED_FQ][1] < wants[n, PRED_F][1] < int(mask[:n].sum()), n
    arrays, a_at = Packer(UNSIGNED[W]), {}
    for n in LENGTHS:
        for phase in range(EPV):
            region = np.full(64 + EPV + n + 64, decoy_a(W), dtype=UNSIGNED[W])
            region[64 + phase:64 + phase + n] = body[:n]
            a_at[n, phase] = arrays.add(region) + 64 + phase
    bytes_, s_at, q_at = Packer(np.uint8), {}, {}
    for n in LENGTHS:
        for enc, offsets in ((BITMAP, range(8)), (BYTES, BYTE_ALIGNMENTS)):
            for o in offsets:
                host, at, off = selection(mask[:n], enc, o)
                s_at[n, enc, o] = (bytes_.add(host) + at, off)
        for align in MAPQ_ALIGNMENTS:
            host, at = mapq_slab(q[:n], align)
            q_at[n, align] = bytes_.add(host) + at
    pa, pb = arrays.upload(), bytes_.upload()
    rows = Rows()
    calls = []
    seen = set()
    combo = 0
    for n in LENGTHS:
        for phase in range(EPV):
            ptr = pa + W * a_at[n, phase]
            assert ptr % 16 == W * phase
            for (n_, enc, o), (at, off) in s_at.items():
                if n_ != n:
                    continue
                assert enc == BITMAP or (pb + at) % 16 == o
                for g, grid in enumerate((1, 2, 3, None)):
                    idx = 5 * combo + g
                    mode, pred, align = MODES[idx & 1], PREDS[(idx >> 1) & 1], MAPQ_ALIGNMENTS[idx % 3]
                    seen.add((grid, mode, pred, align))
                    want, nsel, high = wants[n, pred]
                    k = rows.add(mode, want, nsel, high, (W, n, phase, enc, o, grid, mode, pred, align))
                    assert (pb + q_at[n, align]) % 16 == align
                    calls.append((grid, ptr, n, pred, pb + q_at[n, align], pb + at, off, enc, k, mode))
                combo += 1
    assert len(seen) == 4 * 2 * 2 * 3
    rows.upload()
    for grid, ptr, n, pred, mq, sel, off, enc, k, mode in calls:
        launch(hip, grid, ptr, n, W, pred, mq, sel, off, enc, rows, k, mode)
    rows.check()


# ------------------------------------------------------------------ 3. which bit and which MAPQ byte belong to which element
def positions(W):
    R, S = ROW[W], STEP[W]
    return tuple(range(18)) + (R - 1, R, R + 1, R + 5, S - 1, S, S + 1, S + R, S + R + 1, 2 * S - 1)


@pytest.mark.parametrize("W,phase,off", [(4, 0, 0), (4, 3, 2), (8, 0, 0), (8, 1, 0)])
@pytest.mark.parametrize("enc", ENCODINGS)
def test_which_bit_and_which_mapq_byte_belong_to_which_element(hip, oracle_mod, W, phase, off, enc):
    """n = 2 STEP elements, all decoys A and none selected, under -f 0x1 -F 0x904 -q 30.  Element p = 0x0041 with its bit (byte)
    set alone and its MAPQ 30 among MAPQ bytes of 0 gives the row of one 0x0041, selected == 1 and high == 0.  Three variants
    give zeros: its bit cleared; its MAPQ 29 among MAPQ bytes of 255; its FLAG 0x0141 (excluded) -- which still reports the high
    bit it carries.  (4, 3, 2) and (8, 1, 0) put the kernel's shift at 7: lanes whose 4 or 2 bits straddle two bitmap bytes, next
    to lanes whose bits do not.  At W = 8 positions p and p + 128 are the even and the odd vector of one group of a lane"""
    pred = (0x0001, 0x0904, 30)
    n = 2 * STEP[W]
    if enc == BITMAP and (W, phase, off) in ((4, 3, 2), (8, 1, 0)):
        assert (off + 8 - phase) & 7 == 7
    one, _, _ = wwo.want(oracle_mod, np.array([0x0041], dtype=UNSIGNED[W]), np.ones(1, dtype=bool), superset=True)
    slab = to_device(np.full(64 + 16 // W + n + 64, decoy_a(W, pred), dtype=UNSIGNED[W]))
    arr = slab[64 + phase:64 + phase + n]
    assert arr.data_ptr() % 16 == W * phase
    host, at, sel_off = selection(np.zeros(n, dtype=bool), enc, off)
    if enc == BITMAP:                      # nothing around the bitmap is set either: the one bit is the only one
        host[:] = 0
    d_sel = dev8(host)
    q_host, q_at = mapq_slab(np.zeros(n, dtype=np.uint8), 3)
    d_q = dev8(q_host)
    col = d_q[q_at:q_at + n]
    mode = STORE | SUPERSET
    bit = 1 << (8 * W - 3)
    rows = Rows()
    plan = []
    for p in positions(W):
        plan.append((p, "alone", rows.add(mode, one, 1, 0, (W, phase, off, enc, p, "alone"))))
        plan.append((p, "bit cleared", rows.add(mode, ZEROS, 0, 0, (W, phase, off, enc, p, "bit cleared"))))
        plan.append((p, "mapq lowered", rows.add(mode, ZEROS, 0, 0, (W, phase, off, enc, p, "mapq lowered"))))
        plan.append((p, "flag failing", rows.add(mode, ZEROS, 0, bit, (W, phase, off, enc, p, "flag failing"))))
    rows.upload()
    for p, variant, k in plan:
        where = at + (sel_off + p) // 8 if enc == BITMAP else at + p
        arr[p] = signed(0x0141 | bit, W) if variant == "flag failing" else 0x0041
        if variant != "bit cleared":
            d_sel[where] = 1 << ((sel_off + p) % 8) if enc == BITMAP else 1
        if variant == "mapq lowered":
            col.fill_(255)
            col[p] = 29
        else:
            col[p] = 30
        launch(hip, 3, arr.data_ptr(), n, W, pred, col.data_ptr(), d_sel.data_ptr() + at, sel_off, enc, rows, k, mode)
        arr[p] = signed(int(decoy_a(W, pred)), W)
        d_sel[where] = 0
        if variant == "mapq lowered":
            col.fill_(0)
        else:
            col[p] = 0
    rows.check()


# ------------------------------------------------------------------ 4. `high`
@pytest.mark.parametrize("W", WIDTHS)
def test_high_sees_selected_elements_passing_or_not(hip, oracle_mod, W):
    """2 STEP + 100 elements one element into a line on 2 workgroups: a head edge step [0, S - 1), a fast step [S - 1, 2 S - 1),
    a tail edge step.  For every bit above bit 15, that bit alone on one element -- the first, the last, and the elements on both
    sides of the seam between the edge step and the fast step -- in three states: selected and passing (reported), selected and
    failing (reported, the element not counted), not selected and passing (not reported, not counted).  Bitmap and bytes
    alternate, as do -F 0x904 and -f 0x2 -F 0x904 -q 30; a NULL d_high or d_selected leaves the other results as they are"""
    S = STEP[W]
    n = 2 * S + 100
    spots = (0, S - 2, S - 1, n - 1)
    rng = np.random.RandomState(63 + W)
    base_mask = rng.randint(0, 2, n).astype(bool)
    low, q = make_column(rng, n, W, np.ones(n, dtype=bool), plant=False)
    for at in spots:
        low[at], q[at] = 0x0043, 31
    slab = to_device(np.full(16 // W + n + 8, decoy_a(W), dtype=UNSIGNED[W]))
    arr = slab[1:1 + n]
    assert arr.data_ptr() % 16 == W
    arr.copy_(to_device(low))
    q_host, q_at = mapq_slab(q, 1)
    d_q = dev8(q_host)
    STATES = ("passing", "failing", "unselected")
    setups = {}
    for at in spots:
        on = base_mask.copy()
        on[max(at - 1, 0):at + 2] = True
        off = on.copy()
        off[at] = False
        failing = low.copy()
        failing[at] = 0x0143                                    # secondary: excluded by 0x904
        for enc in ENCODINGS:
            sel_on, sel_off_ = selection(on, enc, 3), selection(off, enc, 3)
            for pred in PREDS:
                for state in STATES:
                    host, sel_at, sel_off = sel_off_ if state == "unselected" else sel_on
                    want = want_of(oracle_mod, failing if state == "failing" else low, off if state == "unselected" else on, pred, q)
                    setups[at, enc, pred, state] = (host, sel_at, sel_off, want)
        for pred in PREDS:
            a, b, c = (setups[at, BITMAP, pred, s][3] for s in STATES)
            assert a[1] == b[1] + 1 == c[1] + 1 and a[2] == b[2] == c[2] == 0
    d_sels = {key: dev8(v[0]) for key, v in setups.items()}
    rows = Rows()
    plan = []
    for bit in range(16, 8 * W):
        for i, at in enumerate(spots):
            enc, pred = ENCODINGS[(bit + i) & 1], PREDS[((bit + i) >> 1) & 1]
            for state in STATES:
                mode = MODES[(bit + i) & 1] if bit != 40 else STORE | SUPERSET       # HIGH_BIAS is bit 40
                want = setups[at, enc, pred, state][3]
                k = rows.add(mode, want[0], want[1], 0 if state == "unselected" else 1 << bit, (W, bit, at, enc, pred, state, mode))
                plan.append((k, at, bit, enc, pred, state, mode))
    rows.upload()
    for k, at, bit, enc, pred, state, mode in plan:
        _, sel_at, sel_off, _ = setups[at, enc, pred, state]
        arr[at] = signed((0x0143 if state == "failing" else 0x0043) | (1 << bit), W)
        launch(hip, 2, arr.data_ptr(), n, W, pred, d_q.data_ptr() + q_at, d_sels[at, enc, pred, state].data_ptr() + sel_at, sel_off, enc, rows,
               k, mode)
        arr[at] = 0x0043
    rows.check()
    # NULL d_high, NULL d_selected, both: every high bit on a selected element that fails
    at = S - 1
    arr[at] = signed(0x0143 | ALL_HIGH[W], W)
    rows = Rows()
    plan = []
    for enc in ENCODINGS:
        for pred in PREDS:
            want = setups[at, enc, pred, "failing"][3]
            for report in ((True, False), (False, True), (False, False)):
                for mode in MODES:
                    for grid in (2, None):
                        plan.append((rows.add(mode, want[0], want[1], ALL_HIGH[W], (W, "NULL words", enc, pred, report, mode, grid),
                                              report=report), enc, pred, report, mode, grid))
    rows.upload()
    for k, enc, pred, report, mode, grid in plan:
        _, sel_at, sel_off, _ = setups[at, enc, pred, "failing"]
        sel = rows.selected(k) if report[0] else None
        high = rows.high(k) if report[1] else None
        args = (arr.data_ptr(), n, W, pred[0], pred[1], d_q.data_ptr() + q_at if pred[2] else None, pred[2],
                d_sels[at, enc, pred, "failing"].data_ptr() + sel_at, sel_off, enc, rows.out(k), sel, high, mode)
        if grid is None:
            assert hip.FLAGSTATS_hip_device_wide_filter_where(*args, None) == 0, err(hip)
        else:
            assert hip.fsk_launch_wide_filter_where(*args, grid, None) == 0
    rows.check()
    host = arr.cpu().numpy()
    for enc in ENCODINGS:
        h_sel, sel_at, sel_off, want = setups[at, enc, PRED_FQ, "failing"]
        d = d_sels[at, enc, PRED_FQ, "failing"]
        for entry, src, mq, sel in ((hip.FLAGSTATS_hip_device_wide_filter_where_sync, arr.data_ptr(), d_q.data_ptr() + q_at,
                                     d.data_ptr() + sel_at),
                                    (hip.FLAGSTATS_hip_wide_x64_filter_where, host.ctypes.data, q_host.ctypes.data + q_at,
                                     h_sel.ctypes.data + sel_at)):
            for mode in MODES:
                o = np.full(32, GARBAGE if mode & STORE else BIAS, dtype=np.uint64)
                assert entry(src, n, W, PRED_FQ[0], PRED_FQ[1], mq, PRED_FQ[2], sel, sel_off, enc, o.ctypes.data, None, None, mode) == 0, err(hip)
                assert np.array_equal(o, expect_row(want[0], mode))


# ------------------------------------------------------------------ 5. degenerate identities
@pytest.mark.parametrize("W", WIDTHS)
def test_degenerate_identities(hip, oracle_mod, W):
    """an all-ones selection gives wide_filter's triple and the empty predicate wide_where's -- against the oracle and, as a
    cross-check, against the parents' entries on the same buffers; require & exclude != 0 gives zeros and high 0 in the store
    form and leaves everything untouched in +=; selection bytes 1, 2, 0x80 and 0xFF all select"""
    S = STEP[W]
    n = 2 * S + 37
    phase = 16 // W - 1
    rng = np.random.RandomState(69 + W)
    half = rng.randint(0, 2, n).astype(bool)
    ones = np.ones(n, dtype=bool)
    full, q_full = make_column(rng, n, W, ones)
    full[n - 1] |= UNSIGNED[W](1 << (8 * W - 1))
    masked, q_masked = make_column(rng, n, W, half)
    byte_values = np.array([1, 2, 0x80, 0xFF], dtype=np.uint8)[rng.randint(0, 4, n)]
    cases = [("all-ones", full, q_full, ones, PREDS, None, "filter"),
             ("empty predicate", masked, q_masked, half, ((0, 0, 0),), None, "where"),
             ("overlap", masked, q_masked, half, ((0x0040, 0x0040, 0), (0x0102, 0x0100, 30)), None, None),
             ("byte values", masked, q_masked, half, PREDS, byte_values, None)]
    arrays, bytes_ = Packer(UNSIGNED[W]), Packer(np.uint8)
    rows = Rows()
    plan = []
    for name, values, q, mask, preds, bv, parent in cases:
        region = np.full(64 + n + 64, decoy_a(W), dtype=UNSIGNED[W])
        region[64 + phase:64 + phase + n] = values
        a = arrays.add(region) + 64 + phase
        q_host, q_at = mapq_slab(q, 3)
        mq = bytes_.add(q_host) + q_at
        for pred in preds:
            want, nsel, high = want_of(oracle_mod, values, mask, pred, q)
            if name == "all-ones":
                assert (nsel, high) == (int(wfwo.counted_mask(values, ones, pred[0], pred[1], q, pred[2]).sum()), wfwo.want_high(values, ones))
                assert 0 < nsel < n and high >> (8 * W - 1)
            if name == "empty predicate":
                w2 = wwo.want(oracle_mod, values, mask, superset=True)
                assert np.array_equal(want, w2[0]) and (nsel, high) == w2[1:] and high not in (0, ALL_HIGH[W])
            if name == "overlap":
                assert nsel == 0 and high == 0 and not want.any()
            for enc in ENCODINGS if bv is None else (BYTES,):
                host, at, off = selection(mask, enc, 6, bv)
                s = bytes_.add(host) + at
                for mode in MODES:
                    for grid in (3, None):
                        plan.append((grid, a, pred, mq, s, off, enc, rows.add(mode, want, nsel, high, (W, name, pred, enc, mode, grid)), mode, None))
                    if parent:
                        plan.append((None, a, pred, mq, s, off, enc, rows.add(mode, want, nsel, high, (W, name, pred, enc, mode, parent)), mode,
                                     parent))
    pa, pb = arrays.upload(), bytes_.upload()
    rows.upload()
    for grid, a, pred, mq, s, off, enc, k, mode, parent in plan:
        ptr = pa + W * a
        if parent == "filter":
            rc = hip.FLAGSTATS_hip_device_wide_filter(ptr, n, W, pred[0], pred[1], pb + mq if pred[2] else None, pred[2], rows.out(k),
                                                      rows.selected(k), rows.high(k), mode, None)
            assert rc == 0, err(hip)
        elif parent == "where":
            rc = hip.FLAGSTATS_hip_device_wide_where(ptr, n, W, pb + s, off, enc, rows.out(k), rows.selected(k), rows.high(k), mode, None)
            assert rc == 0, err(hip)
        else:
            launch(hip, grid, ptr, n, W, pred, pb + mq, pb + s, off, enc, rows, k, mode)
    rows.check()


# ------------------------------------------------------------------ 6. epochs
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("enc", ENCODINGS)
def test_epochs(hip, oracle_mod, W, enc):
    """one workgroup over 258 STEP + 3 elements under -f 0x2 -F 0x904 -q 30: 258 fast steps and a tail edge step, so every wave
    passes its staggered first flush (after 255, 191, 127 and 63 pushes) and wave 0 a full epoch of 255 steps"""
    n = 258 * STEP[W] + 3
    rng = np.random.RandomState(311)
    mask = np.resize(rng.randint(0, 2, 65_519).astype(bool), n)
    low = np.resize(rng.randint(0, 65536, 65_521), n)
    values, q = make_column(rng, n, W, mask, low)
    want, nsel, high = want_of(oracle_mod, values, mask, PRED_FQ, q)
    # half are selected; of those one half has 0x2, one eighth none of 0x904 and three fifths a MAPQ of at least 30: n * 3 / 160
    assert n // 64 < nsel < n // 48 and high not in (0, ALL_HIGH[W])
    t = to_device(values)
    host, at, sel_off = selection(mask, enc, 5)
    d = dev8(host)
    q_host, q_at = mapq_slab(q, 1)
    d_q = dev8(q_host)
    assert t.data_ptr() % 16 == 0
    rows = Rows()
    ks = [rows.add(mode, want, nsel, high, (W, enc, mode)) for mode in MODES]
    rows.upload()
    for k in ks:
        launch(hip, 1, t.data_ptr(), n, W, PRED_FQ, d_q.data_ptr() + q_at, d.data_ptr() + at, sel_off, enc, rows, k, rows.modes[k])
    rows.check()


# ------------------------------------------------------------------ 7. atomics
def test_three_streams_add_into_one_triple(hip, oracle_mod):
    import torch
    from libflagstats_amd import wide_filter_where
    rng = np.random.RandomState(81)
    out = torch.zeros(32, dtype=torch.int64, device="cuda")
    selected = torch.zeros(1, dtype=torch.int64, device="cuda")
    high = torch.zeros(1, dtype=torch.int64, device="cuda")
    total, total_sel, total_high = np.zeros(32, dtype=np.uint64), 0, 0
    inputs = []
    for W, n, packed, pred in ((4, 40 * STEP[4] + 11, True, PRED_FQ), (8, 37 * STEP[8] + 5, False, PRED_F), (4, 43 * STEP[4] - 3, True, PRED_FQ)):
        mask = rng.randint(0, 3, n) > 0
        values, q = make_column(rng, n, W, mask)
        want, nsel, h = want_of(oracle_mod, values, mask, pred, q)
        assert nsel > 0 and h not in (0, ALL_HIGH[W])
        total += want
        total_sel += nsel
        total_high |= h
        where = dev8(pack(mask, 3)) if packed else torch.from_numpy(mask).cuda()
        inputs.append((to_device(values), where, packed, pred, dev8(q)))
    streams = [torch.cuda.Stream() for _ in inputs]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    for st, (t, where, packed, pred, d_q) in zip(streams, inputs):
        with torch.cuda.stream(st):
            wide_filter_where.count_torch_ints_filter_where(t, where, require=pred[0], exclude=pred[1], mapq=d_q if pred[2] else None,
                                                            min_mapq=pred[2], out=out, selected=selected, high=high, superset=True,
                                                            packed=packed, bit_offset=3 if packed else 0)
    for st in streams:
        st.synchronize()
    assert np.array_equal(u64(out), total) and int(u64(selected)[0]) == total_sel and int(u64(high)[0]) == total_high


# ------------------------------------------------------------------ 8. host form across chunks
@pytest.mark.parametrize("W", WIDTHS)
def test_host_form_across_chunks(hip, oracle_mod, W):
    """the "chunk_flags" knob at 65544, 8192, 1000 and 8 (chunks of 32,772 / 16,386, 4,096 / 2,048, 500 / 250 and 4 / 2
    elements): all but 8192 put the chunk seams at bit positions of the bitmap that are not byte-aligned, the bitmap starts 5
    bits into its first byte and the MAPQ column is unaligned.  A high bit on one selected element of a late chunk that fails the
    predicate; decoys A where the mask does not select"""
    from libflagstats_amd import _lib, wide_filter_where
    rng = np.random.RandomState(93 + W)
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        for chunk_flags, n in ((65544, 70001), (8192, 70001), (1000, 70001), (1000, 1501), (8, 1501)):
            per_chunk = chunk_flags * 2 // W
            assert n > 2 * per_chunk
            mask = rng.randint(0, 2, n).astype(bool)
            column, q = make_column(rng, n, W, mask, plant=False)
            carrier = int(np.flatnonzero(mask & ((column & UNSIGNED[W](0x0904)) != 0))[-3])
            assert carrier >= per_chunk
            column[carrier] |= UNSIGNED[W](1 << (8 * W - 2))
            values = column.view(SIGNED[W])
            bits = pack(mask, 5)
            q_slab, q_at = mapq_slab(q, 3)
            q_un = q_slab[q_at:q_at + n]
            assert q_un.ctypes.data % 4 in (1, 2, 3) and q_un.flags["C_CONTIGUOUS"]
            _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", chunk_flags), "chunk_flags")
            for pred in PREDS:
                kw = dict(require=pred[0], exclude=pred[1], mapq=q_un if pred[2] else None, min_mapq=pred[2])
                wants = {sup: want_of(oracle_mod, values, mask, pred, q, superset=bool(sup)) for sup in (0, SUPERSET)}
                _, nsel, high = wants[0]
                assert 0 < nsel < int(mask.sum()) and high == 1 << (8 * W - 2)
                for sup in (0, SUPERSET):
                    got, selected, h = wide_filter_where.counters_ints_filter_where(values, bits, packed=True, bit_offset=5,
                                                                                    superset=bool(sup), **kw)
                    assert np.array_equal(got, wants[sup][0]) and selected == nsel and h == high, (chunk_flags, n, pred, "bitmap", sup)
                    got, selected, h = wide_filter_where.counters_ints_filter_where(values, mask, superset=bool(sup), **kw)
                    assert np.array_equal(got, wants[sup][0]) and selected == nsel and h == high, (chunk_flags, n, pred, "bytes", sup)
                for flags in (0, SUPERSET):                  # += over bias words
                    host_call(hip.FLAGSTATS_hip_wide_x64_filter_where, values.ctypes.data, n, W, pred, q_un.ctypes.data, bits.ctypes.data, 5,
                              BITMAP, flags, wants[SUPERSET][0], nsel, high, (W, chunk_flags, n, pred, flags), hip)
                # the chunks in front of the carrier report nothing
                kw1 = dict(kw, mapq=q_un[:per_chunk].copy() if pred[2] else None)
                got, selected, h = wide_filter_where.counters_ints_filter_where(values[:per_chunk], bits, packed=True, bit_offset=5, **kw1)
                assert h == 0 and selected == int(wfwo.counted_mask(values[:per_chunk], mask[:per_chunk], pred[0], pred[1], q[:per_chunk],
                                                                    pred[2]).sum())
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old


# ------------------------------------------------------------------ 9. refusals that need a device
def test_device_dependent_refusals(hip):
    """what the C entries and the launcher refuse: the union of test_gpu_wide_where's and test_gpu_wide_filter's lists.  Every
    one is an argument check that returns before anything is launched, and the outputs stay as they were"""
    import torch
    n = 4096
    bufs = {W: torch.zeros(n + 8, dtype={4: torch.int32, 8: torch.int64}[W], device="cuda") for W in WIDTHS}
    m = torch.ones(n + 8, dtype=torch.uint8, device="cuda")
    mq = torch.full((n + 8,), 40, dtype=torch.uint8, device="cuda")
    out = torch.full((32,), BIAS, dtype=torch.int64, device="cuda")
    sel = torch.full((1,), SEL_BIAS, dtype=torch.int64, device="cuda")
    high = torch.full((1,), HIGH_BIAS, dtype=torch.int64, device="cuda")
    h_out = np.full(32, BIAS, dtype=np.uint64)
    h_sel, h_high = ctypes.c_uint64(SEL_BIAS), ctypes.c_uint64(HIGH_BIAS)
    host = np.zeros(n + 8, dtype=np.int64)
    host8 = np.ones(n + 8, dtype=np.uint8)
    p8, p4 = bufs[8].data_ptr(), bufs[4].data_ptr()
    dev = hip.FLAGSTATS_hip_device_wide_filter_where
    sync = hip.FLAGSTATS_hip_device_wide_filter_where_sync
    x64 = hip.FLAGSTATS_hip_wide_x64_filter_where

    def untouched(what):
        torch.cuda.synchronize()
        assert (out == BIAS).all() and int(u64(sel)[0]) == SEL_BIAS and int(u64(high)[0]) == HIGH_BIAS, what
        assert (h_out == BIAS).all() and h_sel.value == SEL_BIAS and h_high.value == HIGH_BIAS, what

    def refused(what, text, d_array=p8, n_=n, eb=8, require=0, exclude=0x904, d_mapq=mq.data_ptr(), mn=30, d_sel=m.data_ptr(), off=0,
                bits=BYTES, flags=0, counters=True, forms=("device", "sync", "host")):
        for form in forms:
            if form == "device":
                rc = dev(d_array, n_, eb, require, exclude, d_mapq, mn, d_sel, off, bits, out.data_ptr() if counters else None, sel.data_ptr(),
                         high.data_ptr(), flags, None)
            elif form == "sync":
                rc = sync(d_array, n_, eb, require, exclude, d_mapq, mn, d_sel, off, bits, h_out.ctypes.data if counters else None,
                          ctypes.byref(h_sel), ctypes.byref(h_high), flags)
            else:
                src = host.ctypes.data + (d_array - p8) % 8 if d_array else None
                rc = x64(src, n_, eb, require, exclude, host8.ctypes.data if d_mapq else None, mn, host8.ctypes.data if d_sel else None, off,
                         bits, h_out.ctypes.data if counters else None, ctypes.byref(h_sel), ctypes.byref(h_high), flags)
            assert rc != 0, (what, form)
            assert text in err(hip), (what, form, err(hip))
        untouched(what)

    # the wide entries' list
    refused("elem_bytes 2", "u16 filter_where entries", eb=2)
    refused("elem_bytes 3", "elem_bytes must be 4 or 8", eb=3)
    refused("elem_bytes 16", "elem_bytes must be 4 or 8", eb=16)
    refused("off by 2 at W = 4", "4-byte aligned", d_array=p8 + 2, eb=4)
    refused("off by 4 at W = 8", "8-byte aligned", d_array=p8 + 4, eb=8)
    refused("an extra flag bit", "no other bits", flags=4)
    refused("NULL array", "NULL array with n > 0", d_array=None, eb=4)
    refused("n * elem_bytes is no size", "n * elem_bytes is not a size", n_=1 << 62)
    # the filter entries' list
    refused("require above 0xFFFF", "require must be a 16-bit FLAG mask", require=0x10000)
    refused("exclude above 0xFFFF", "exclude must be a 16-bit FLAG mask", exclude=0x10000)
    refused("min_mapq above 255", "min_mapq must be at most 255", mn=256)
    refused("NULL mapq with min_mapq > 0", "NULL mapq with min_mapq > 0 and n > 0", d_mapq=None, mn=1)
    # the where entries' list
    for W in WIDTHS:
        pw = bufs[W].data_ptr()
        for bits in (0, 2, 4, 16):
            refused("sel_bits %d" % bits, "sel_bits must be 1", d_array=pw, eb=W, bits=bits)
        refused("NULL selection", "NULL selection with n > 0", d_array=pw, eb=W, d_sel=None)
        refused("NULL selection names the remedy", "FLAGSTATS_hip_device_wide_filter)", d_array=pw, eb=W, d_sel=None)
        refused("sel_offset + n is no index", "sel_offset + n is not an index", d_array=pw, eb=W, off=(1 << 64) - 5)
        refused("NULL counters", "NULL counters", d_array=pw, eb=W, counters=False)
        # a wave's uint32 totals: 2^60 elements on any grid this device launches.  The host form launches per chunk and cannot
        # reach the limit, so it has nothing to refuse here
        refused("a wave's totals", "a wave's uint32 totals", d_array=pw, eb=W, n_=1 << 60, forms=("device", "sync"))
    # host memory where device memory is needed: the array, the MAPQ column, the selection, d_out, d_selected, d_high
    for W in WIDTHS:
        pw = bufs[W].data_ptr()
        for bits in ENCODINGS:
            for what, a, q_, s_ in (("d_array", host.ctypes.data, mq.data_ptr(), m.data_ptr()), ("d_mapq", pw, host8.ctypes.data, m.data_ptr()),
                                    ("d_sel", pw, mq.data_ptr(), host8.ctypes.data)):
                rc = dev(a, n, W, 0, 0x904, q_, 30, s_, 0, bits, out.data_ptr(), sel.data_ptr(), high.data_ptr(), 0, None)
                assert rc != 0 and what in err(hip), (what, err(hip))
                rc = sync(a, n, W, 0, 0x904, q_, 30, s_, 0, bits, h_out.ctypes.data, ctypes.byref(h_sel), ctypes.byref(h_high), 0)
                assert rc != 0 and what in err(hip), (what, err(hip))
        for what, o_, s_, h_ in (("d_out", h_out.ctypes.data, sel.data_ptr(), high.data_ptr()),
                                 ("d_selected", out.data_ptr(), ctypes.addressof(h_sel), high.data_ptr()),
                                 ("d_high", out.data_ptr(), sel.data_ptr(), ctypes.addressof(h_high))):
            rc = dev(pw, n, W, 0, 0x904, mq.data_ptr(), 30, m.data_ptr(), 0, BYTES, o_, s_, h_, 0, None)
            assert rc != 0 and what in err(hip), (what, err(hip))
    pinned = hip.FLAGSTATS_hip_host_alloc(512)
    assert pinned
    try:
        ctypes.memset(pinned, 0, 512)
        for what, o_, s_, h_ in (("d_out", pinned, sel.data_ptr(), high.data_ptr()), ("d_selected", out.data_ptr(), pinned, high.data_ptr()),
                                 ("d_high", out.data_ptr(), sel.data_ptr(), pinned)):
            rc = dev(p8, n, 8, 0, 0x904, mq.data_ptr(), 30, m.data_ptr(), 0, BYTES, o_, s_, h_, STORE, None)
            assert rc != 0 and what + " must be device memory" in err(hip), err(hip)
        assert not any(ctypes.string_at(pinned, 512))
    finally:
        hip.FLAGSTATS_hip_host_free(pinned)
    untouched("host pointers")
    # extents: counters 8 bytes short; an array one element short; a MAPQ column one byte short; a selection one byte short (the
    # bitmap's last byte, the byte form's last byte), counted from the selection pointer
    nbytes = 2 << 20
    raw = hip.FLAGSTATS_hip_device_alloc(nbytes)
    assert raw
    try:
        assert hip.FLAGSTATS_hip_memcpy_h2d(raw, np.zeros(nbytes, dtype=np.uint8).ctypes.data, nbytes) == 0
        rc = dev(p8, n, 8, 0, 0x904, mq.data_ptr(), 30, m.data_ptr(), 0, BYTES, raw + nbytes - 248, sel.data_ptr(), high.data_ptr(), 0, None)
        assert rc != 0 and "d_out" in err(hip) and "8 bytes short" in err(hip), err(hip)
        for W in WIDTHS:
            big = torch.zeros(8 * nbytes + 8, dtype={4: torch.int32, 8: torch.int64}[W], device="cuda")
            pb = big.data_ptr()
            bigm = torch.ones(8 * nbytes + 8, dtype=torch.uint8, device="cuda")
            rc = dev(raw, nbytes // W + 1, W, 0, 0x904, bigm.data_ptr(), 30, bigm.data_ptr(), 0, BYTES, out.data_ptr(), sel.data_ptr(),
                     high.data_ptr(), STORE, None)
            assert rc != 0 and "d_array" in err(hip) and "%d bytes short" % W in err(hip), err(hip)
            rc = sync(raw + W, nbytes // W, W, 0, 0x904, bigm.data_ptr(), 30, bigm.data_ptr(), 0, BYTES, h_out.ctypes.data, ctypes.byref(h_sel),
                      ctypes.byref(h_high), STORE)
            assert rc != 0 and "d_array" in err(hip) and "%d bytes short" % W in err(hip), err(hip)
            rc = dev(pb, nbytes + 1, W, 0, 0x904, raw, 30, bigm.data_ptr(), 0, BYTES, out.data_ptr(), sel.data_ptr(), high.data_ptr(), STORE, None)
            assert rc != 0 and "d_mapq" in err(hip) and "1 bytes short" in err(hip), err(hip)
            rc = sync(pb, nbytes, W, 0, 0x904, raw + 1, 1, bigm.data_ptr(), 0, BYTES, h_out.ctypes.data, ctypes.byref(h_sel),
                      ctypes.byref(h_high), STORE)
            assert rc != 0 and "d_mapq" in err(hip) and "1 bytes short" in err(hip), err(hip)
            # without -q the column is no input: the same short column passes
            o = np.full(32, BIAS, dtype=np.uint64)
            assert sync(pb, nbytes, W, 0, 0x904, raw + 1, 0, bigm.data_ptr(), 0, BYTES, o.ctypes.data, None, None, STORE) == 0, err(hip)
            for n_, off, bits in ((nbytes + 1, 0, BYTES), (nbytes, 1, BYTES), (8 * nbytes + 1, 0, BITMAP), (8 * nbytes - 2, 3, BITMAP)):
                rc = dev(pb, n_, W, 0, 0x904, bigm.data_ptr(), 30, raw, off, bits, out.data_ptr(), sel.data_ptr(), high.data_ptr(), STORE, None)
                assert rc != 0 and "d_sel" in err(hip) and "1 bytes short" in err(hip), (n_, off, bits, err(hip))
                rc = sync(pb, n_, W, 0, 0x904, bigm.data_ptr(), 30, raw, off, bits, h_out.ctypes.data, ctypes.byref(h_sel), ctypes.byref(h_high),
                          STORE)
                assert rc != 0 and "d_sel" in err(hip) and "1 bytes short" in err(hip), (n_, off, bits, err(hip))
            untouched("extents")
            for n_ok, off, bits in ((nbytes, 0, BYTES), (8 * nbytes - 3, 3, BITMAP)):   # the selection to its very last byte / bit
                o = np.full(32, BIAS, dtype=np.uint64)
                s, h = ctypes.c_uint64(SEL_BIAS), ctypes.c_uint64(HIGH_BIAS)
                assert sync(pb, n_ok, W, 0, 0x904, bigm.data_ptr(), 1, raw, off, bits, o.ctypes.data, ctypes.byref(s), ctypes.byref(h),
                            STORE) == 0, err(hip)
                assert not o.any() and s.value == 0 and h.value == 0            # a selection of zeros
            del big, bigm
    finally:
        hip.FLAGSTATS_hip_device_free(raw)
    untouched("extents")
    # the launcher itself: other widths and encodings, misalignment, other mode bits, no workgroups, a wave's uint32 totals, an
    # offset that is no index, NULL pointers, a predicate that is no predicate -- nothing queued
    words = torch.full((34,), BIAS, dtype=torch.int64, device="cuda")
    p = words.data_ptr()
    f = hip.fsk_launch_wide_filter_where
    q_, s_ = mq.data_ptr(), m.data_ptr()
    for W in WIDTHS:
        pw = bufs[W].data_ptr()
        for bits in ENCODINGS:
            assert f(pw, 8, W, 0, 0x904, q_, 30, s_, 0, bits, p, p + 256, p + 264, 4, 1, None) != 0
            assert f(pw, 8, W, 0, 0x904, q_, 30, s_, 0, bits, p, p + 256, p + 264, 0, 0, None) != 0
            assert f(pw, 1 << 35, W, 0, 0x904, q_, 30, s_, 0, bits, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(pw, 8, W, 0, 0x904, q_, 30, s_, (1 << 64) - 5, bits, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(pw, 8, W, 0, 0x904, q_, 30, None, 0, bits, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(pw, 8, W, 0, 0x904, None, 30, s_, 0, bits, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(None, 8, W, 0, 0x904, q_, 30, s_, 0, bits, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(pw + W // 2, 8, W, 0, 0x904, q_, 30, s_, 0, bits, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(pw, 8, W, 0, 0x904, q_, 30, s_, 0, bits, None, p + 256, p + 264, STORE, 1, None) != 0
            assert f(pw, 8, W, 0x10000, 0, q_, 30, s_, 0, bits, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(pw, 8, W, 0, 0x10000, q_, 30, s_, 0, bits, p, p + 256, p + 264, STORE, 1, None) != 0
            assert f(pw, 8, W, 0, 0x904, q_, 256, s_, 0, bits, p, p + 256, p + 264, STORE, 1, None) != 0
        for bits in (0, 2, 4, 16):
            assert f(pw, 8, W, 0, 0x904, q_, 30, s_, 0, bits, p, p + 256, p + 264, STORE, 1, None) != 0
    for eb in (0, 1, 2, 3, 16):
        assert f(p4, 8, eb, 0, 0x904, q_, 30, s_, 0, BYTES, p, p + 256, p + 264, STORE, 1, None) != 0
    torch.cuda.synchronize()
    assert (words == BIAS).all()


# ------------------------------------------------------------------ 10. the Python layers
def test_python_layers(hip, oracle_mod):
    """numpy over all six dtypes (the 2-byte ones take the uint16 route and report high == 0), strict and its message -- raised
    for a selected element only, passing or not --, the dict; the raw-pointer form; the torch layer's dtypes, shapes, placement
    and its device-mismatch refusals"""
    import torch
    from libflagstats_amd import filter_where, wide, wide_filter_where as wfw
    n = 3 * STEP[4] + 41
    rng = np.random.RandomState(103)
    low = rng.randint(0, 65536, n).astype(np.uint16)
    mask = rng.randint(0, 3, n) > 0
    q = np.array([0, 29, 30, 31, 255], dtype=np.uint8)[rng.randint(0, 5, n)]
    bits = pack(mask, 3)
    pred = dict(require=0x0002, exclude=0x0904, mapq=q, min_mapq=30)
    want, nsel, _ = wfwo.want(oracle_mod, low.astype(np.uint32), mask, 0x0002, 0x0904, q, 30)
    want_sup = wfwo.want(oracle_mod, low.astype(np.uint32), mask, 0x0002, 0x0904, q, 30, superset=True)[0]
    assert 0 < nsel < int(mask.sum())
    for dt in ("int16", "uint16", "int32", "uint32", "int64", "uint64"):
        v = low.astype({"int16": np.uint16}.get(dt, dt)).view(dt)
        for kw, w in (({}, mask), ({"packed": True, "bit_offset": 3}, bits)):
            got, selected, high = wfw.counters_ints_filter_where(v, w, **pred, **kw)
            assert got.dtype == np.uint64 and np.array_equal(got, want) and selected == nsel and high == 0, (dt, kw)
            got, selected, high = wfw.counters_ints_filter_where(v, w, superset=True, **pred, **kw)
            assert np.array_equal(got, want_sup) and selected == nsel and high == 0, (dt, kw)
            d = wfw.flagstats_ints_filter_where(v, w, **pred, **kw)
            assert d["n_values"] == nsel and int(d["failed"]["FQCFAIL"]) == int(want[25]) and "high_bits" not in d
            assert int(d["passed"]["mapped"]) == nsel - int(want[2]) - int(want[18])
            assert wfw.flagstats_ints_filter_where(v, w, strict=False, **pred, **kw)["high_bits"] == 0
        if v.dtype.itemsize == 2:
            continue
        W = v.dtype.itemsize
        top = 1 << (8 * W - 1)
        # decoys A in the slots that are NOT selected: no high bit, no raise, the same table
        null = v.copy()
        null.view(UNSIGNED[W])[~mask] = decoy_a(W)
        for kw, w in (({}, mask), ({"packed": True, "bit_offset": 3}, bits)):
            d = wfw.flagstats_ints_filter_where(null, w, **pred, **kw)
            assert d["n_values"] == nsel and int(d["failed"]["FQCFAIL"]) == int(want[25])
            assert wfw.counters_ints_filter_where(null, w, **pred, **kw)[2] == 0
        # a SELECTED element that FAILS the predicate with a bit above bit 15: strict names the bits, the table is the same
        bad = null.copy()
        at = int(np.flatnonzero(mask & ((low & 0x0904) != 0))[5])
        bad.view(UNSIGNED[W])[at] |= UNSIGNED[W](top)
        with pytest.raises(ValueError) as e:
            wfw.flagstats_ints_filter_where(bad, mask, **pred)
        assert str(e.value) == wide.high_bits_message(top) and "0x%X" % top in str(e.value)
        d = wfw.flagstats_ints_filter_where(bad, bits, packed=True, bit_offset=3, strict=False, **pred)
        assert d["high_bits"] == top and d["n_values"] == nsel and int(d["failed"]["FQCFAIL"]) == int(want[25])
        # the raw-pointer form and the torch layer on the same column
        t, d_bits, d_mask, d_q = to_device(bad), dev8(bits), torch.from_numpy(mask).cuda(), dev8(q)
        got, selected, high = wfw.count_device_ptr_ints_filter_where(t.data_ptr(), n, W, d_bits.data_ptr(), 1, require=0x0002, exclude=0x0904,
                                                                     mapq_ptr=d_q.data_ptr(), min_mapq=30, sel_offset=3, superset=True)
        assert np.array_equal(got, want_sup) and selected == nsel and high == top
        got, selected, high = wfw.count_device_ptr_ints_filter_where(t.data_ptr(), n, W, d_mask.data_ptr(), 8, require=0x0002, exclude=0x0904,
                                                                     mapq_ptr=d_q.data_ptr(), min_mapq=30)
        assert np.array_equal(got, want) and selected == nsel and high == top
        tp = dict(require=0x0002, exclude=0x0904, mapq=d_q, min_mapq=30)
        o, s, h = wfw.count_torch_ints_filter_where(t, d_mask, **tp)
        torch.cuda.synchronize()
        for x, numel in ((o, 32), (s, 1), (h, 1)):
            assert x.dtype == torch.int64 and tuple(x.shape) == (numel,) and x.device == t.device
        assert np.array_equal(u64(o), want) and int(u64(s)[0]) == nsel and int(u64(h)[0]) == top
        o2, s2, h2 = wfw.count_torch_ints_filter_where(t, d_bits, out=o, selected=s, high=h, packed=True, bit_offset=3, **tp)   # += and |=
        assert o2 is o and s2 is s and h2 is h
        torch.cuda.synchronize()
        assert np.array_equal(u64(o), 2 * want) and int(u64(s)[0]) == 2 * nsel and int(u64(h)[0]) == top
        wfw.count_torch_ints_filter_where(t, d_mask, out=o, selected=s, high=h, store=True, superset=True, **tp)
        torch.cuda.synchronize()
        assert np.array_equal(u64(o), want_sup) and int(u64(s)[0]) == nsel and int(u64(h)[0]) == top
    # two-byte dtypes route to the u16 entries: the wide entry is not called, `high` is left as it is (zeroed with store)
    calls = []
    real = filter_where.counters_filter_where

    def spy(*a, **kw):
        calls.append(a[0].dtype)
        return real(*a, **kw)

    filter_where.counters_filter_where = spy
    try:
        wfw.counters_ints_filter_where(low.view(np.int16), mask, **pred)
        wfw.counters_ints_filter_where(low.astype(np.int32), mask, **pred)
    finally:
        filter_where.counters_filter_where = real
    assert calls == [np.dtype(np.uint16)]
    t16 = torch.from_numpy(low.view(np.int16)).cuda()
    d_mask, d_bits, d_q = torch.from_numpy(mask).cuda(), dev8(bits), dev8(q)
    tp = dict(require=0x0002, exclude=0x0904, mapq=d_q, min_mapq=30)
    h = torch.full((1,), 9, dtype=torch.int64, device="cuda")
    o, s, h2 = wfw.count_torch_ints_filter_where(t16, d_mask, high=h, **tp)
    torch.cuda.synchronize()
    assert h2 is h and int(h[0]) == 9 and np.array_equal(u64(o), want) and int(u64(s)[0]) == nsel
    wfw.count_torch_ints_filter_where(t16, d_bits, out=o, selected=s, high=h, store=True, packed=True, bit_offset=3, **tp)
    torch.cuda.synchronize()
    assert int(h[0]) == 0 and np.array_equal(u64(o), want) and int(u64(s)[0]) == nsel
    # empty inputs
    o, s, h = wfw.count_torch_ints_filter_where(torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.bool, device="cuda"),
                                                exclude=0x0904)
    torch.cuda.synchronize()
    assert not u64(o).any() and int(s[0]) == 0 and int(h[0]) == 0
    got, selected, high = wfw.counters_ints_filter_where(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool), exclude=0x0904)
    assert not got.any() and selected == 0 and high == 0
    got, selected, high = wfw.count_device_ptr_ints_filter_where(0, 0, 8, 0, 1, exclude=0x0904)
    assert not got.any() and selected == 0 and high == 0
    # results somewhere else than t
    t = to_device(low.astype(np.uint32))
    with pytest.raises(ValueError, match=r"where must live on t's device \(cuda:0\), not on cpu"):
        wfw.count_torch_ints_filter_where(t, torch.from_numpy(mask))
    with pytest.raises(ValueError, match=r"mapq must live on t's device \(cuda:0\), not on cpu"):
        wfw.count_torch_ints_filter_where(t, d_mask, mapq=torch.from_numpy(q), min_mapq=30)
    with pytest.raises(ValueError, match=r"out must live on t's device \(cuda:0\), not on cpu"):
        wfw.count_torch_ints_filter_where(t, d_mask, out=torch.zeros(32, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"selected must live on t's device \(cuda:0\), not on cpu"):
        wfw.count_torch_ints_filter_where(t, d_mask, selected=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"high must live on t's device \(cuda:0\), not on cpu"):
        wfw.count_torch_ints_filter_where(t, d_mask, high=torch.zeros(1, dtype=torch.int64))


# ------------------------------------------------------------------ 11. a seeded randomised sweep
def test_seeded_randomised_sweep(hip, oracle_mod):
    """150 cases drawn from the parameters above: width, n up to 2 STEP + 1, array phase, encoding, bit offset or byte alignment,
    MAPQ alignment, predicate (with and without -q, require bits or none, an overlapping pair now and then), density, high bits
    planted on selected and on unselected elements, mode and grid.  Every case is launched and checked"""
    rng = np.random.RandomState(20262)
    packers = {W: Packer(UNSIGNED[W]) for W in WIDTHS}
    bytes_ = Packer(np.uint8)
    rows = Rows()
    plan = []
    preds = ((0, 0, 0), PRED_F, PRED_FQ, (0x0001, 0, 0), (0, 0, 30), (0x0041, 0x0F00, 31), (0, 0x0004, 255), (0x0040, 0x0040, 0),
             (0, 0, 1), (0x0003, 0x0904, 200))
    for case in range(150):
        W = WIDTHS[rng.randint(2)]
        S, EPV = STEP[W], 16 // W
        n = int([rng.randint(0, 40), rng.randint(0, 2 * ROW[W]), rng.randint(S - 70, S + 70), rng.randint(0, 2 * S + 2)][rng.randint(4)])
        phase = int(rng.randint(EPV))
        enc = ENCODINGS[rng.randint(2)]
        off = int(rng.randint(8) if enc == BITMAP else rng.randint(16))
        align = int(rng.randint(16))
        pred = preds[rng.randint(len(preds))]
        density = (0.02, 0.5, 0.97)[rng.randint(3)]
        mode = MODES[rng.randint(2)]
        grid = (1, 2, 3, None)[rng.randint(4)]
        mask = rng.random_sample(n) < density
        column = rng.randint(0, 65536, n).astype(UNSIGNED[W])
        q = np.array([0, 1, 29, 30, 31, 199, 200, 254, 255], dtype=np.uint8)[rng.randint(0, 9, n)]
        for i in rng.randint(0, max(n, 1), 3)[:min(n, 3)]:
            column[i] |= UNSIGNED[W](1 << int(rng.randint(16, 8 * W)))
        if rng.randint(2) and not pred[0] & pred[1]:
            column[~mask] = decoy_a(W, pred)
            q[~mask] = 255
        want, nsel, high = want_of(oracle_mod, column, mask, pred, q)
        region = np.full(8 + EPV + n + 8, decoy_a(W), dtype=UNSIGNED[W])
        region[8 + phase:8 + phase + n] = column
        a = packers[W].add(region) + 8 + phase
        host, at, sel_off = selection(mask, enc, off, None if rng.randint(2) else rng.randint(1, 256, n))
        s = bytes_.add(host) + at
        q_host, q_at = mapq_slab(q, align)
        mq = bytes_.add(q_host) + q_at
        plan.append((grid, W, a, n, pred, mq, s, sel_off, enc,
                     rows.add(mode, want, nsel, high, (case, W, n, phase, enc, off, align, pred, density, mode, grid)), mode))
    base = {W: packers[W].upload() for W in WIDTHS}
    pb = bytes_.upload()
    rows.upload()
    for grid, W, a, n, pred, mq, s, sel_off, enc, k, mode in plan:
        launch(hip, grid, base[W] + W * a, n, W, pred, pb + mq, pb + s, sel_off, enc, rows, k, mode)
    rows.check()
    assert len(plan) == 150
