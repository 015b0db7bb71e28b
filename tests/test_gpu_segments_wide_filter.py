"""Filtered segmented flagstat on int32 / int64 columns on the MI355X (csrc/flagstat_segments_wide_filter.hip and the layers above
it): rows, the number of passing elements and one high-bit mask per segment, against tests/segments_wide_filter_oracle.py; every
comparison is exact.

Expected values never come from the code under test: rows and counts are segments_filter_oracle's over the low 16 bits, masks
numpy's OR per segment over ALL elements, periodic inputs get all three in O(period + nseg).  Direct launches
(fsk_launch_segments_wide_filter with a small grid) are placed with segments_wide_oracle.WideWriterSplit, the launcher's work
split mirrored, and every case asserts from the oracle that its input holds what it is there for."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_wide_filter_oracle as swfo  # noqa: E402
import segments_wide_oracle as swo  # noqa: E402

pytestmark = pytest.mark.gpu

STORE, SUPERSET = 1, 2
MODES = (1, 0, 3, 2)             # store, +=, store + superset, += + superset
GARBAGE, BIAS, SEL_BIAS, MASK_BIAS = 0x5EED_0000_0BAD, 3, 5, (1 << 48) | (1 << 17)
EVERY_MIN_UNITS = (0, 1, 2, 3, 255, 256, 0xFFFFFFFF)
NEVER = 0xFFFFFFFF               # min_units: no chain
P = 65_521                       # prime: no vector, row, unit or writer seam is a multiple of the period
SIGNED = {4: np.int32, 8: np.int64}
UNSIGNED = {4: np.uint32, 8: np.uint64}
WIDTHS = (4, 8)
PREDICATES = {"empty": (0, 0, 0), "-F 0x904": (0, 0x904, 0), "-f 0x2 -F 0x904": (2, 0x904, 0), "overlap": (0x104, 0x904, 0),
              "-q 30": (0, 0, 30), "-f 0x1 -F 0x904 -q 30": (1, 0x904, 30), "require 0xFFFF": (0xFFFF, 0, 0)}


def err(hip):
    return hip.FLAGSTATS_hip_last_error().decode(errors="replace")


def dev(x):
    """the array on the device (torch has signed tensors of every width: the bytes are what counts)"""
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[x.dtype.itemsize])).cuda()


def dev64(o):
    import torch
    return torch.from_numpy(np.ascontiguousarray(o, dtype=np.int64)).cuda()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def place(x, phase=0, slack=4):
    """x on the device, its first element `phase` elements (bytes for a uint8 column) past a 16-byte boundary: (owner, pointer)"""
    import torch
    x = np.ascontiguousarray(x)
    buf = np.zeros(x.size + phase + slack, dtype=x.dtype)
    buf[phase:phase + x.size] = x
    t = dev(buf)
    assert t.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    return t, t.data_ptr() + phase * x.dtype.itemsize


def widen(low, dtype, rng, every=37):
    """low (uint16 values) as dtype, one element in `every` with random bits above bit 15 (the sign bit among them)"""
    W = np.dtype(dtype).itemsize
    n = low.size
    u = low.astype(np.uint64)
    hot = rng.randint(0, every, n) == 0
    hi = rng.randint(0, 1 << 16, n).astype(np.uint64) << np.uint64(16)
    if W == 8:
        hi |= rng.randint(0, 1 << 32, n).astype(np.uint64) << np.uint64(32)
    u |= np.where(hot, hi, np.uint64(0)).astype(np.uint64)
    return u.astype(UNSIGNED[W]).view(dtype)


def expect(want, mode):
    """what a call in `mode` must leave in rows / counts / masks prefilled with GARBAGE (store) or BIAS / SEL_BIAS / MASK_BIAS
    (+=), given the oracle's superset triple"""
    w = want[0].copy()
    if not mode & SUPERSET:
        w[:, [0, 9, 16]] = 0
    if mode & STORE:
        return w, want[1], want[2]
    return w + np.uint64(BIAS), want[1] + np.uint64(SEL_BIAS), want[2] | np.uint64(MASK_BIAS)


def prefilled(nseg, mode, together=True):
    """device rows, counts and masks, prefilled; counts and masks behind the rows in one allocation, or each apart"""
    import torch
    store = bool(mode & STORE)
    words = torch.full((nseg * 34,), GARBAGE if store else BIAS, dtype=torch.int64, device="cuda")
    rows = words[:nseg * 32].view(nseg, 32)
    if together:
        sel, high = words[nseg * 32:nseg * 33], words[nseg * 33:]
    else:
        sel, high = (torch.empty(nseg, dtype=torch.int64, device="cuda") for _ in range(2))
    sel.fill_(GARBAGE if store else SEL_BIAS)
    high.fill_(GARBAGE if store else MASK_BIAS)
    return words, rows, sel, high


def host_words(nseg, mode):
    store = bool(mode & STORE)
    return (np.full((nseg, 32), GARBAGE if store else BIAS, dtype=np.uint64), np.full(nseg, GARBAGE if store else SEL_BIAS, dtype=np.uint64),
            np.full(nseg, GARBAGE if store else MASK_BIAS, dtype=np.uint64))


def device_form(hip, ptr, n, W, offsets, pred, qptr, mode, together=True, stream=None):
    import torch
    d_off = dev64(offsets)
    nseg = d_off.numel() - 1
    _, rows, sel, high = prefilled(nseg, mode, together)
    torch.cuda.synchronize()
    rc = hip.FLAGSTATS_hip_device_wide_segments_filter(ptr, n, W, d_off.data_ptr(), nseg, pred[0], pred[1], qptr, pred[2], rows.data_ptr(),
                                                       sel.data_ptr(), high.data_ptr(), mode, stream)
    assert rc == 0, err(hip)
    torch.cuda.synchronize()
    return u64(rows), u64(sel), u64(high)


def sync_form(hip, ptr, n, W, offsets, pred, qptr, mode):
    o = np.ascontiguousarray(offsets, dtype=np.uint64)
    rows, sel, high = host_words(o.size - 1, mode)
    rc = hip.FLAGSTATS_hip_device_wide_segments_filter_sync(ptr, n, W, o.ctypes.data, o.size - 1, pred[0], pred[1], qptr, pred[2],
                                                            rows.ctypes.data, sel.ctypes.data, high.ctypes.data, mode)
    assert rc == 0, err(hip)
    return rows, sel, high


def host_form(hip, x, offsets, pred, q, mode):
    o = np.ascontiguousarray(offsets, dtype=np.uint64)
    rows, sel, high = host_words(o.size - 1, mode)
    rc = hip.FLAGSTATS_hip_wide_x64_segments_filter(x.ctypes.data, x.size, x.dtype.itemsize, o.ctypes.data, o.size - 1, pred[0], pred[1],
                                                    None if q is None else q.ctypes.data, pred[2], rows.ctypes.data, sel.ctypes.data,
                                                    high.ctypes.data, mode)
    assert rc == 0, err(hip)
    return rows, sel, high


def same(got, want, what):
    rows, sel, high = got
    bad = np.nonzero((rows != want[0]).any(axis=1))[0]
    assert bad.size == 0, (what, "rows", bad[:8], rows[bad[:2]], want[0][bad[:2]])
    bad = np.nonzero(sel != want[1])[0]
    assert bad.size == 0, (what, "selected", bad[:8], sel[bad[:8]], want[1][bad[:8]])
    bad = np.nonzero(high != want[2])[0]
    assert bad.size == 0, (what, "masks", bad[:8], [hex(int(v)) for v in high[bad[:4]]], [hex(int(v)) for v in want[2][bad[:4]]])


@pytest.fixture(scope="module")
def launcher(hip):
    hip.fsk_segments_policy.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    hip.fsk_segments_policy.restype = None
    hip.fsk_set_segments_policy.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    hip.fsk_set_segments_policy.restype = None
    return hip.fsk_launch_segments_wide_filter   # prototype attached by _lib.lib()


def get_policy(hip):
    mu, bpc = ctypes.c_uint32(), ctypes.c_uint32()
    hip.fsk_segments_policy(ctypes.byref(mu), ctypes.byref(bpc))
    return mu.value, bpc.value


@contextlib.contextmanager
def policy(hip, min_units, blocks_per_cu=1):
    saved = get_policy(hip)
    try:
        hip.fsk_set_segments_policy(min_units, blocks_per_cu)
        assert get_policy(hip) == (min_units, blocks_per_cu)
        yield
    finally:
        hip.fsk_set_segments_policy(*saved)
    assert get_policy(hip) == saved


def direct(launcher, ptr, W, qptr, base, m, offsets, pred, mode, grid, together=True):
    """one fsk_launch_segments_wide_filter on the null stream into prefilled rows, counts and masks"""
    import torch
    d_off = dev64(offsets)
    nseg = d_off.numel() - 1
    _, rows, sel, high = prefilled(nseg, mode, together)
    torch.cuda.synchronize()
    assert launcher(ptr, W, qptr, base, m, d_off.data_ptr(), nseg, pred[0], pred[1], pred[2], rows.data_ptr(), sel.data_ptr(),
                    high.data_ptr(), mode, grid, None) == 0
    torch.cuda.synchronize()
    return u64(rows), u64(sel), u64(high)


def pass_fraction_inside(want, offsets, min_len=64):
    """every segment of at least min_len elements has a pass fraction strictly between 0 and 1"""
    length = np.diff(np.asarray(offsets)).astype(np.uint64)
    big = length >= min_len
    return big.any() and (want[1][big] > 0).all() and (want[1][big] < length[big]).all()


# ------------------------------------------------------------------ 1. every FLAG value, every predicate kind, mode and form
@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_values_and_predicates(hip, dtype):
    rng = np.random.RandomState(5)
    W = np.dtype(dtype).itemsize
    lengths = rng.randint(0, 5001, 56)
    lengths[[3, 17]] = 0
    o = 7 + np.concatenate([[0], np.cumsum(lengths)])
    n = int(o[-1]) + 11
    assert 120_000 < n < 160_000
    x = widen(np.resize(rng.permutation(65536).astype(np.uint16), n), dtype, rng)
    assert np.unique(swfo.low16(x)).size == 65536
    q = rng.randint(0, 256, n).astype(np.uint8)
    t, ptr = place(x)
    tq, qptr = place(q, 1)                                 # the column at an odd address
    for name, pred in PREDICATES.items():
        want = swfo.want(x, o, *pred[:2], q, pred[2], superset=True)
        total = int(want[1].sum())
        if name == "empty":
            assert np.array_equal(want[1], np.diff(o).astype(np.uint64))
        elif name == "overlap":
            assert total == 0 and not want[0].any() and not want[2].any()
        elif name == "require 0xFFFF":
            assert 0 < total < 10
        else:
            assert pass_fraction_inside(want, o), name
        if name != "overlap":
            assert want[2].any() and (want[2] == 0).any()   # masks set by elements that fail too; empty segments read 0
            assert np.array_equal(want[2], swo.segmented_high(x, o))
        for mode in MODES:
            w = expect(want, mode)
            qp = qptr if pred[2] else None
            same(device_form(hip, ptr, n, W, o, pred, qp, mode, together=bool(mode & 2)), w, (name, mode, "device"))
            same(sync_form(hip, ptr, n, W, o, pred, qp, mode), w, (name, mode, "sync"))
            same(host_form(hip, x, o, pred, q, mode), w, (name, mode, "host"))


# ------------------------------------------------------------------ 2. lengths at the vector, row and unit edges; every phase
@pytest.mark.parametrize("W", WIDTHS)
def test_lengths_and_phases(hip, W):
    rng = np.random.RandomState(9)
    V, R, U = 16 // W, 1024 // W, 8192 // W
    edges = [0, 1, V - 1, V, R - 1, R + 1, U - 1, U, U + 1, 2 * U + 3]
    lengths = np.concatenate([edges, rng.choice(edges, 50)])
    rng.shuffle(lengths)
    front, behind = 5, 6
    o = front + np.concatenate([[0], np.cumsum(lengths)])
    n = int(o[-1]) + behind
    x = widen(rng.randint(0, 65536, n).astype(np.uint16), SIGNED[W], rng)
    q = rng.randint(0, 256, n).astype(np.uint8)
    # the gaps in front of offsets[0] and behind offsets[nseg]: passing elements that carry high bits; they count nowhere
    gap = np.r_[0:front, int(o[-1]):n]
    x[gap] = SIGNED[W](0x0001 | (1 << 16) | (1 << 30))
    q[gap] = 255
    preds = (PREDICATES["-f 0x1 -F 0x904 -q 30"], PREDICATES["-F 0x904"])
    assert all(swfo.pass_vector(x, *p[:2], q, p[2])[gap].all() for p in preds)
    wants = [swfo.want(x, o, *p[:2], q, p[2], superset=True) for p in preds]
    for p, w in zip(preds, wants):
        assert int(w[1].sum()) == int(swfo.pass_vector(x, *p[:2], q, p[2])[front:int(o[-1])].sum()) > 0
        assert w[2].any() and (w[2] == 0).any() and pass_fraction_inside(w, o)
    for phase in range(V):
        t, ptr = place(x, phase)
        assert ptr % 16 == phase * W
        for mq_off in range(4):
            tq, qptr = place(q, mq_off)
            for mu in (1, NEVER):
                with policy(hip, mu):
                    for pred, want in zip(preds, wants):
                        mode = 3 if mu == 1 else 0
                        same(device_form(hip, ptr, n, W, o, pred, qptr, mode, together=mode == 3), expect(want, mode),
                             (W, phase, mq_off, mu, pred))
        same(host_form(hip, x, o, preds[0], q, 1), expect(wants[0], 1), (W, phase, "host"))


# ------------------------------------------------------------------ 3. masks and counts reach their own segment and no other
@pytest.mark.parametrize("W", WIDTHS)
def test_mask_and_count_isolation(hip, launcher, W):
    V, R, U = 16 // W, 1024 // W, 8192 // W
    lo0, end = 1, 40 * U - 1                              # launched grid positions [1, 40 U - 1) at grid 1: writers of 10 units
    # interior bounds on a vector, a row, a unit and a writer seam, then an all-zero segment that crosses the seam at 20 U
    bounds = np.array([5, 3 * U + 3 * V, 6 * U + 2 * R, 8 * U, 10 * U, 14 * U + 1, 20 * U + 7, 38 * U], dtype=np.int64)
    assert bounds[1] % V == 0 and bounds[1] % R and bounds[2] % R == 0 and bounds[2] % U and bounds[3] % U == 0
    o = bounds - lo0
    n = end - lo0
    w = swo.writer_ranges(lo0 * W, n, 1, W)
    assert w.waves == 4 and list(w.end + lo0) == [10 * U, 20 * U, 30 * U, end]
    p = w.pieces(o, 2)
    assert (p["chain"] > 0).any() and (p["chain"] == 0).any() and p["plain"].any() and (~p["plain"]).any()
    assert sorted(p["writer"][p["seg"] == 5].tolist()) == [1, 2] and sorted(p["writer"][p["seg"] == 6].tolist()) == [2, 3]
    FAIL, PASS = 0x0100, 0x0001                            # under -F 0x904: secondary fails, paired passes
    x = np.full(40 * U, FAIL, dtype=UNSIGNED[W])
    q = np.full(40 * U, 40, dtype=np.uint8)
    x[bounds[5]:bounds[6]] = 0                             # the all-zero-FLAG segment
    planted = {}                                           # grid position -> (flag, bit)
    bit = 16
    for B in bounds[1:5]:                                  # one position outside each edge: the neighbour's last / first element
        for pos in (int(B) - 1, int(B)):
            planted[pos] = (PASS, bit)
            bit += 1
    for pos in (4, int(bounds[-1]), 0, 40 * U - 1):        # gaps and grid slack: passing, with high bits, counted nowhere
        planted[pos] = (PASS, bit)
        bit += 1
    failing_inside = 2 * U + 17                            # a failing element with high bits inside segment 0 (a chain unit)
    planted[failing_inside] = (FAIL, 8 * W - 1)
    for pos, (flag, b) in planted.items():
        x[pos] = UNSIGNED[W](flag | (1 << b))
    t, ptr0 = place(x)
    tq, qptr0 = place(q, 3)
    arr, qa = x[lo0:end].view(SIGNED[W]), q[lo0:end]
    for pred, zero_len in ((PREDICATES["-F 0x904"], True), (PREDICATES["-f 0x1 -F 0x904 -q 30"], False), ((0, 0x904, 30), True)):
        want = swfo.want(arr, o, *pred[:2], qa, pred[2], superset=True)
        # the oracle itself: each planted element in the count and mask of the segment that holds it, gaps and slack nowhere
        sel = [0] * 7
        mask = [0] * 7
        for pos, (flag, b) in planted.items():
            s = np.nonzero((bounds[:-1] <= pos) & (pos < bounds[1:]))[0]
            if s.size:
                sel[s[0]] += flag == PASS
                mask[s[0]] |= 1 << b
        sel[5] = int(bounds[6] - bounds[5]) if zero_len else 0   # zero flags pass every predicate without a require bit
        assert [int(v) for v in want[1]] == sel and [int(v) for v in want[2]] == mask
        assert want[2][0] == np.uint64(1 << (8 * W - 1)) | np.uint64(1 << 16) and want[1][0] == 1
        for mu in (2, NEVER):
            with policy(hip, mu):
                for mode in (1, 0):
                    got = direct(launcher, ptr0 + lo0 * W, W, qptr0 + lo0, 0, n, o, pred, mode, 1, together=mode == 1)
                    same(got, expect(want, mode), (W, pred, "min_units", mu, "mode", mode))


# ------------------------------------------------------------------ 4. which MAPQ byte belongs to which element
@pytest.mark.parametrize("W", WIDTHS)
def test_mapq_pairing(hip, launcher, W):
    rng = np.random.RandomState(17 + W)
    V, R, U = 16 // W, 1024 // W, 8192 // W
    lengths = np.concatenate([[3 * U + 5, 1, 2, 3, V, V + 1, R + 1, U, 2 * U + 3], rng.choice([1, 2, 3, V, V + 1, R - 1, U, 2 * U + 3], 90)])
    o = np.concatenate([[0], np.cumsum(lengths)])
    n = int(o[-1])
    x = np.full(n, 0x0003, dtype=SIGNED[W])               # constant and passing: `selected` is the MAPQ test alone
    columns = (((np.arange(n, dtype=np.int64) * 7 + 3) & 0xFF).astype(np.uint8), rng.randint(0, 256, n).astype(np.uint8))
    for phase in (0, V - 1):                               # lo0 = 0, and a ragged first unit; the last unit is ragged either way
        t, ptr = place(x, phase)
        w = swo.writer_ranges(phase * W, n, 1, W)
        assert (w.lo0 + n) % U != 0 and (w.pieces(o, 1)["chain"] > 0).any() and (w.pieces(o, NEVER)["chain"] == 0).all()
        for q in columns:
            for mq_off in (0, 1, 2, 3):
                tq, qptr = place(q, mq_off)
                for thr in (1, 30, 128, 255):
                    pred = (0, 0x904, thr)
                    want = swfo.want(x, o, *pred[:2], q, thr, superset=True)
                    tiny = np.diff(o) <= 3
                    assert tiny.sum() > 20 and 0 < int(want[1].sum()) < n
                    if thr in (30, 128):
                        assert (want[1][tiny] > 0).any() and (want[1][tiny] == 0).any()
                    for mu in (1, NEVER):
                        with policy(hip, mu):
                            same(direct(launcher, ptr, W, qptr, 0, n, o, pred, 3, 1), expect(want, 3), (W, phase, mq_off, thr, mu))
                    if mq_off == 1 and thr == 30:
                        with policy(hip, 1):
                            same(device_form(hip, ptr, n, W, o, pred, qptr, 0, together=False), expect(want, 0), (W, phase, "device"))


# ------------------------------------------------------------------ 5. chain, epochs and seams
def periodic_inputs(W, seed, n):
    import torch
    rng = np.random.RandomState(seed)
    pattern = widen(rng.randint(0, 65536, P).astype(np.uint16), SIGNED[W], rng, every=20_000)
    mq_pattern = rng.randint(0, 256, P).astype(np.uint8)   # one joint period for the column and its MAPQ bytes
    reps = -(-(n + 16) // P)
    t, tq = dev(pattern).repeat(reps), dev(mq_pattern).repeat(reps)
    torch.cuda.synchronize()
    return pattern, mq_pattern, t, tq


@pytest.mark.parametrize("W", WIDTHS)
def test_chain_epochs_and_seams(hip, launcher, W):
    U = 8192 // W
    runs = (254, 255, 256, 511)
    n = 4 * 516 * U - 9                                    # ~16 MiB: at grid 1 each wave owns 516 units
    pattern, mq_pattern, t, tq = periodic_inputs(W, 21 + W, n)
    ptr, qptr = t.data_ptr(), tq.data_ptr() + 1            # the column one byte into its buffer: phase 1 of its period
    preds = ((PREDICATES["-F 0x904"], None), (PREDICATES["-f 0x1 -F 0x904 -q 30"], np.roll(mq_pattern, -1)))
    w = swo.writer_ranges(ptr % 16, n, 1, W)
    assert w.waves == 4 and w.lo0 == 0
    cuts = []
    for k, K in enumerate(runs):                           # in writer k: 3 elements of ragged head, K whole units, 5 of ragged tail
        g0 = int(w.begin[k]) + 2 * U
        cuts += [int(w.begin[k]) + 7, g0 - 3, g0 + K * U + 5]
    o = np.array([0] + cuts + [n], dtype=np.int64)
    pieces = w.pieces(o, 2)
    runs_of = {int(c): (int(h), int(tl)) for c, h, tl in zip(pieces["chain"], pieces["head"], pieces["tail"]) if c in runs}
    assert runs_of == {K: (3, 5) for K in runs}, runs_of   # one chain run of each length, ragged on both sides
    assert pieces["plain"].any() and (~pieces["plain"]).any() and (pieces["chain"] == 0).any()
    for pred, mqp in preds:
        want = swfo.periodic_want(pattern, o, *pred[:2], mqp, pred[2], superset=True)
        assert pass_fraction_inside(want, o) and want[2].any()
        for mode in (3, 0):
            same(direct(launcher, ptr, W, qptr if pred[2] else None, 0, n, o, pred, mode, 1, together=mode == 3), expect(want, mode),
                 (W, "runs", pred, mode))
    # grid 3: segments that end exactly on, one before and one after a writer seam
    w3 = swo.writer_ranges(ptr % 16, n, 3, W)
    seams = w3.seams()
    assert w3.waves == 12 and seams.size == 11
    o3 = np.concatenate([[0], seams + np.resize([0, -1, 1], seams.size), [n - 3]]).astype(np.int64)
    p3 = w3.pieces(o3, 2)
    on = np.isin(o3[1:-1], seams)
    assert on.sum() == 4 and np.isin(o3[1:-1] + 1, seams).sum() == 4 and np.isin(o3[1:-1] - 1, seams).sum() == 3
    assert (p3["chain"] >= 100).sum() >= 12 and (p3["chain"] == 0).any()     # a long chain run in every writer, one-element pieces
    assert p3["plain"].any() and (~p3["plain"]).any()     # rows wholly inside a writer, rows that cross a seam by one element
    for pred, mqp in preds:
        want = swfo.periodic_want(pattern, o3, *pred[:2], mqp, pred[2], superset=True)
        assert pass_fraction_inside(want, o3)
        for mode in (3, 0):
            same(direct(launcher, ptr, W, qptr if pred[2] else None, 0, n, o3, pred, mode, 3, together=mode == 0), expect(want, mode),
                 (W, "seams", pred, mode))
    del t, tq


# ------------------------------------------------------------------ 6. every min_units through the three public entries
@pytest.mark.parametrize("W", WIDTHS)
def test_every_min_units(hip, W):
    rng = np.random.RandomState(29)
    U = 8192 // W
    n = 384 * U + 77                                       # ~3 MiB
    x = widen(rng.randint(0, 65536, n).astype(np.uint16), SIGNED[W], rng, every=900)
    q = rng.randint(0, 256, n).astype(np.uint8)
    o = np.array([9, 40, 40, U + 1, 2 * U + 5, 5 * U + 5, 8 * U + 7, 100 * U + 3, 100 * U + 9, 100 * U + 9 + 255 * U, n - 5], dtype=np.int64)
    pred = PREDICATES["-f 0x1 -F 0x904 -q 30"]
    want = swfo.want(x, o, *pred[:2], q, pred[2], superset=True)
    assert pass_fraction_inside(want, o) and want[2].any()
    t, ptr = place(x)
    tq, qptr = place(q, 3)
    # the public entries launch one workgroup per CU: at this size a writer owns one or two units, so min_units 0 and 1 send whole
    # units through the chain, the larger ones (nearly) everything through the per-piece form
    w = swo.writer_ranges(ptr % 16, n, hip.FLAGSTATS_hip_compute_units(), W)
    longest = {mu: int(w.pieces(o, mu)["chain"].max()) for mu in EVERY_MIN_UNITS}
    assert longest[0] >= 1 and longest[1] >= 1 and longest[NEVER] == 0 and longest[255] == 0 and longest[256] == 0, longest
    for mu in EVERY_MIN_UNITS:
        with policy(hip, mu):
            same(device_form(hip, ptr, n, W, o, pred, qptr, 3), expect(want, 3), (W, mu, "device"))
            same(sync_form(hip, ptr, n, W, o, pred, qptr, 2), expect(want, 2), (W, mu, "sync"))
            same(host_form(hip, x, o, pred, q, 1), expect(want, 1), (W, mu, "host"))


# ------------------------------------------------------------------ 7. accumulate, streams, NULL outputs
@pytest.mark.parametrize("W", WIDTHS)
def test_accumulate_and_streams(hip, launcher, W):
    import torch
    rng = np.random.RandomState(33)
    U = 8192 // W
    n = 36 * U + 11
    x = widen(rng.randint(0, 65536, n).astype(np.uint16), SIGNED[W], rng, every=500)
    q = rng.randint(0, 256, n).astype(np.uint8)
    o = np.array([0, 50, 3 * U + 1, 3 * U + 1, 20 * U - 7, 36 * U], dtype=np.int64)
    nseg = o.size - 1
    pred = PREDICATES["-f 0x1 -F 0x904 -q 30"]
    want = swfo.want(x, o, *pred[:2], q, pred[2], superset=True)
    assert pass_fraction_inside(want, o) and want[2].any()
    t, ptr = place(x)
    tq, qptr = place(q, 1)
    d_off = dev64(o)
    grid = 64

    def launch(c0, m, rows, sel, high, mode, stream=None):
        return launcher(ptr + c0 * W, W, qptr + c0, c0, m, d_off.data_ptr(), nseg, *pred, rows.data_ptr(),
                        None if sel is None else sel.data_ptr(), None if high is None else high.data_ptr(), mode, grid, stream)

    for together in (True, False):
        # += over prefilled rows, counts and masks, twice
        _, rows, sel, high = prefilled(nseg, 0, together)
        torch.cuda.synchronize()
        for _ in range(2):
            assert launch(0, n, rows, sel, high, SUPERSET) == 0
        torch.cuda.synchronize()
        same((u64(rows), u64(sel), u64(high)), (want[0] * np.uint64(2) + np.uint64(BIAS), want[1] * np.uint64(2) + np.uint64(SEL_BIAS),
                                                want[2] | np.uint64(MASK_BIAS)), (W, together, "twice"))
        # three streams add three disjoint thirds into one set of rows: the one-call result
        _, rows, sel, high = prefilled(nseg, STORE, together)
        rows.zero_()
        sel.zero_()
        high.zero_()
        streams = [torch.cuda.Stream() for _ in range(3)]
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())
        thirds = [0, n // 3 + 1, 2 * n // 3 + 5, n]
        for st, c0, c1 in zip(streams, thirds[:-1], thirds[1:]):
            assert launch(c0, c1 - c0, rows, sel, high, SUPERSET, ctypes.c_void_p(st.cuda_stream)) == 0
        for st in streams:
            st.synchronize()
        same((u64(rows), u64(sel), u64(high)), want, (W, together, "three streams"))
    # d_selected and d_high each NULL, in both forms
    for mode in (3, 2):
        for no_sel, no_high in ((True, False), (False, True), (True, True)):
            _, rows, sel, high = prefilled(nseg, mode, False)
            torch.cuda.synchronize()
            assert launch(0, n, rows, None if no_sel else sel, None if no_high else high, mode) == 0
            rc = hip.FLAGSTATS_hip_device_wide_segments_filter(ptr, n, W, d_off.data_ptr(), nseg, *pred[:2], qptr, pred[2], rows.data_ptr(),
                                                               None if no_sel else sel.data_ptr(), None if no_high else high.data_ptr(),
                                                               mode & SUPERSET, None)
            assert rc == 0, err(hip)
            torch.cuda.synchronize()
            first = expect(want, mode)
            twice = (first[0] + want[0], first[1] + want[1], first[2] | want[2])
            untouched = np.full(nseg, GARBAGE if mode & STORE else 0, dtype=np.uint64)
            same((u64(rows), u64(sel), u64(high)),
                 (twice[0], untouched + np.uint64(0 if mode & STORE else SEL_BIAS) if no_sel else twice[1],
                  untouched + np.uint64(0 if mode & STORE else MASK_BIAS) if no_high else twice[2]), (W, mode, no_sel, no_high))


# ------------------------------------------------------------------ 8. against the entries that exist (cross-checks only)
@pytest.mark.parametrize("W", WIDTHS)
def test_equivalences(hip, W):
    import torch
    rng = np.random.RandomState(41)
    U = 8192 // W
    n = 50 * U + 3
    x = widen(rng.randint(0, 65536, n).astype(np.uint16), SIGNED[W], rng, every=300)
    q = rng.randint(0, 256, n).astype(np.uint8)
    o = np.unique(np.concatenate([[7], rng.randint(7, n - 9, 30), [12 * U, 30 * U + 1, n - 9]]))
    nseg = o.size - 1
    t, ptr = place(x)
    tq, qptr = place(q, 2)
    d_off = dev64(o)
    # the empty predicate: the wide segmented entry, selected[i] = length
    rows, sel, high = device_form(hip, ptr, n, W, o, (0, 0, 0), None, 3)
    r2 = torch.empty((nseg, 32), dtype=torch.int64, device="cuda")
    h2 = torch.empty(nseg, dtype=torch.int64, device="cuda")
    assert hip.FLAGSTATS_hip_device_wide_segments(ptr, n, W, d_off.data_ptr(), nseg, r2.data_ptr(), h2.data_ptr(), 3, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(rows, u64(r2)) and np.array_equal(high, u64(h2)) and np.array_equal(sel, np.diff(o).astype(np.uint64))
    # one segment: the wide filter entry
    pred = PREDICATES["-f 0x1 -F 0x904 -q 30"]
    one = np.array([0, n])
    rows, sel, high = device_form(hip, ptr, n, W, one, pred, qptr, 3)
    w34 = torch.empty(34, dtype=torch.int64, device="cuda")
    rc = hip.FLAGSTATS_hip_device_wide_filter(ptr, n, W, *pred[:2], qptr, pred[2], w34.data_ptr(), w34.data_ptr() + 256, w34.data_ptr() + 264,
                                              3, None)
    assert rc == 0, err(hip)
    torch.cuda.synchronize()
    g = u64(w34)
    assert np.array_equal(rows[0], g[:32]) and sel[0] == g[32] and high[0] == g[33] and 0 < int(sel[0]) < n and high[0] != 0
    # a column without high bits: narrowing, then the uint16 segmented filter entry
    low = rng.randint(0, 65536, n).astype(np.uint16)
    tz, zptr = place(low.astype(UNSIGNED[W]))
    rows, sel, high = device_form(hip, zptr, n, W, o, pred, qptr, 3, together=False)
    t16 = dev(low)
    r16 = torch.empty((nseg, 32), dtype=torch.int64, device="cuda")
    s16 = torch.empty(nseg, dtype=torch.int64, device="cuda")
    rc = hip.FLAGSTATS_hip_device_u16_segments_filter(t16.data_ptr(), n, d_off.data_ptr(), nseg, *pred[:2], qptr, pred[2], r16.data_ptr(),
                                                      s16.data_ptr(), 3, None)
    assert rc == 0, err(hip)
    torch.cuda.synchronize()
    assert np.array_equal(rows, u64(r16)) and np.array_equal(sel, u64(s16)) and not high.any() and sel.any()


# ------------------------------------------------------------------ 9. host form across chunks
@pytest.mark.parametrize("W", WIDTHS)
def test_host_form_across_chunks(hip, W):
    from libflagstats_amd import _lib
    from libflagstats_amd import segments_wide_filter as swf
    rng = np.random.RandomState(53)
    chunk_flags = 16_386                                   # 32,772 bytes: 8,193 int32 or 4,096 int64 a chunk
    c = chunk_flags * 2 // W
    n = 7 * c + 77
    x = rng.randint(0, 65536, n + 1).astype(UNSIGNED[W])[1:]
    q = rng.randint(0, 256, n + 1).astype(np.uint8)[1:]    # the column at an odd address
    assert q.ctypes.data % 2 == 1
    first = 3
    o = np.array([first, 10, 10, first + c + 7, first + c + c // 2, first + 3 * c + c // 2 + 5, first + 4 * c, n - 20], dtype=np.int64)
    # offsets[0] > 0; segment 2 spans chunks 0 and 1, segment 4 chunks 1, 2 and 3, segment 5 ends on a chunk edge
    assert o[0] > 0 and (o[5] - first) // c - (o[4] - first) // c == 2 and (o[6] - first) % c == 0
    x[first + c + c // 2 + 1] |= UNSIGNED[W](1 << 16)
    x[first + 2 * c + 9] |= UNSIGNED[W](1 << 20)
    x[first + 3 * c + c // 2 + 4] |= UNSIGNED[W](1 << (8 * W - 1))
    x[first + 4 * c] |= UNSIGNED[W](1 << 17)
    x[1], x[n - 1] = x[1] | UNSIGNED[W](1 << 30), x[n - 1] | UNSIGNED[W](1 << 29)       # outside every segment
    x = x.view(SIGNED[W])
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", chunk_flags), "chunk_flags")
        for name in ("-f 0x1 -F 0x904 -q 30", "-F 0x904", "overlap"):
            pred = PREDICATES[name]
            want = swfo.want(x, o, *pred[:2], q, pred[2], superset=True)
            if name != "overlap":
                assert [hex(int(v)) for v in want[2]] == [hex(v) for v in (0, 0, 0, 0, (1 << 16) | (1 << 20) | (1 << (8 * W - 1)), 0, 1 << 17)]
                assert pass_fraction_inside(want, o)
            for mode in MODES:
                same(host_form(hip, x, o, pred, q, mode), expect(want, mode), (W, "chunks", name, mode))
        pred = PREDICATES["-f 0x1 -F 0x904 -q 30"]
        same(swf.counters_segments_ints_filter(x, o, *pred[:2], q, pred[2], superset=True), swfo.want(x, o, *pred[:2], q, pred[2], True), (W, "python"))
        for oo in (np.array([1, 50, 99]), np.array([7, 7, 7]), np.array([n, n])):        # one chunk only; nothing covered
            same(swf.counters_segments_ints_filter(x, oo, exclude=0x904), swfo.want(x, oo, 0, 0x904), (W, oo))
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old


# ------------------------------------------------------------------ 10. refusals
@pytest.mark.parametrize("W", WIDTHS)
def test_refusals(hip, launcher, W):
    import torch
    n, nseg = 4096, 3
    t = torch.zeros(n + 8, dtype={4: torch.int32, 8: torch.int64}[W], device="cuda")
    tq = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    host, hostq = np.zeros(n + 8, dtype=SIGNED[W]), np.zeros(n + 8, dtype=np.uint8)
    o = np.array([0, 10, 2000, n], dtype=np.uint64)
    d_off = dev64(o)
    out = torch.full((nseg, 32), BIAS, dtype=torch.int64, device="cuda")
    sel = torch.full((nseg,), SEL_BIAS, dtype=torch.int64, device="cuda")
    high = torch.full((nseg,), MASK_BIAS, dtype=torch.int64, device="cuda")
    h_out = np.full((nseg, 32), BIAS, dtype=np.uint64)
    h_sel = np.full(nseg, SEL_BIAS, dtype=np.uint64)
    h_high = np.full(nseg, MASK_BIAS, dtype=np.uint64)

    def untouched(what):
        torch.cuda.synchronize()
        assert (out == BIAS).all() and (sel == SEL_BIAS).all() and (high == MASK_BIAS).all(), what
        assert (h_out == BIAS).all() and (h_sel == SEL_BIAS).all() and (h_high == MASK_BIAS).all(), what

    def refused(what, text, d_array=t.data_ptr(), n_=n, eb=W, offsets=o, nseg_=nseg, req=0, exc=0x904, mapq=True, mq=30, flags=0, rows=True,
                forms=("device", "sync", "host")):
        d_o = None if offsets is None else dev64(offsets.astype(np.int64))
        for form in forms:
            if form == "device":
                rc = hip.FLAGSTATS_hip_device_wide_segments_filter(d_array, n_, eb, None if d_o is None else d_o.data_ptr(), nseg_, req, exc,
                                                                   tq.data_ptr() if mapq else None, mq, out.data_ptr() if rows else None,
                                                                   sel.data_ptr(), high.data_ptr(), flags, None)
            elif form == "sync":
                rc = hip.FLAGSTATS_hip_device_wide_segments_filter_sync(d_array, n_, eb, None if offsets is None else offsets.ctypes.data,
                                                                        nseg_, req, exc, tq.data_ptr() if mapq else None, mq,
                                                                        h_out.ctypes.data if rows else None, h_sel.ctypes.data,
                                                                        h_high.ctypes.data, flags)
            else:
                src = host.ctypes.data + (d_array - t.data_ptr()) if d_array else None
                rc = hip.FLAGSTATS_hip_wide_x64_segments_filter(src, n_, eb, None if offsets is None else offsets.ctypes.data, nseg_, req,
                                                                exc, hostq.ctypes.data if mapq else None, mq,
                                                                h_out.ctypes.data if rows else None, h_sel.ctypes.data, h_high.ctypes.data, flags)
            assert rc != 0, (what, form)
            assert err(hip) and text in err(hip), (what, form, err(hip))
        untouched(what)

    refused("elem_bytes 2", "16-bit arrays go to the u16 segmented filter entries", eb=2)
    for eb in (0, 1, 3, 16, -4):
        refused("elem_bytes %d" % eb, "elem_bytes must be 4 or 8", eb=eb)
    refused("a misaligned array", "%d-byte aligned" % W, d_array=t.data_ptr() + W // 2)
    refused("NULL array", "NULL array with n > 0", d_array=None)
    refused("NULL mapq", "NULL mapq with min_mapq > 0 and n > 0", mapq=False)
    refused("require", "require must be a 16-bit FLAG mask", req=0x10000)
    refused("exclude", "exclude must be a 16-bit FLAG mask", exc=0x10000)
    refused("min_mapq", "min_mapq must be at most 255", mq=256)
    refused("NULL offsets", "with nseg > 0", offsets=None)
    refused("NULL rows", "with nseg > 0", rows=False)
    refused("an extra flag bit", "no other bits", flags=4)
    refused("too many segments", "nseg is too large", nseg_=1 << 60)
    refused("n * elem_bytes is no size", "is not a size", n_=1 << 63)
    refused("decreasing offsets", "offsets must be non-decreasing", offsets=np.array([0, 20, 10, n], dtype=np.uint64), forms=("sync", "host"))
    refused("offsets past the array", "exceeds the array's", offsets=np.array([0, 10, 20, n + 1], dtype=np.uint64), forms=("sync", "host"))
    # host pointers where device memory is needed
    a, f, qd = t.data_ptr(), d_off.data_ptr(), tq.data_ptr()
    good = dict(d_array=a, d_offsets=f, d_mapq=qd, d_out=out.data_ptr(), d_selected=sel.data_ptr(), d_high=high.data_ptr())
    for name, bad in (("d_out", h_out.ctypes.data), ("d_selected", h_sel.ctypes.data), ("d_high", h_high.ctypes.data),
                      ("d_offsets", o.ctypes.data), ("d_array", host.ctypes.data), ("d_mapq", hostq.ctypes.data)):
        k = {**good, name: bad}
        rc = hip.FLAGSTATS_hip_device_wide_segments_filter(k["d_array"], n, W, k["d_offsets"], nseg, 0, 0x904, k["d_mapq"], 30, k["d_out"],
                                                           k["d_selected"], k["d_high"], 0, None)
        assert rc != 0 and name in err(hip), (name, err(hip))
    rc = hip.FLAGSTATS_hip_device_wide_segments_filter_sync(a, n, W, o.ctypes.data, nseg, 0, 0x904, hostq.ctypes.data, 30, h_out.ctypes.data,
                                                            h_sel.ctypes.data, h_high.ctypes.data, 0)
    assert rc != 0 and "d_mapq" in err(hip), err(hip)
    untouched("host pointers")
    # extents: the array and the column one element short, rows, counts, masks and offsets 8 bytes short
    nbytes = 2 << 20
    raw = hip.FLAGSTATS_hip_device_alloc(nbytes)
    assert raw
    try:
        assert hip.FLAGSTATS_hip_memcpy_h2d(raw, np.zeros(nbytes, dtype=np.uint8).ctypes.data, nbytes) == 0
        big = np.array([0, 5, 100, nbytes // W], dtype=np.uint64)
        big_off = dev64(big)
        bigq = torch.zeros(nbytes // W + 8, dtype=torch.uint8, device="cuda")
        rc = hip.FLAGSTATS_hip_device_wide_segments_filter(raw, nbytes // W + 1, W, big_off.data_ptr(), nseg, 0, 0x904, bigq.data_ptr(), 30,
                                                           out.data_ptr(), sel.data_ptr(), high.data_ptr(), STORE, None)
        assert rc != 0 and "d_array" in err(hip) and "%d bytes short" % W in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_segments_filter_sync(raw, nbytes // W + 1, W, big.ctypes.data, nseg, 0, 0x904, bigq.data_ptr(), 30,
                                                                h_out.ctypes.data, h_sel.ctypes.data, h_high.ctypes.data, STORE)
        assert rc != 0 and "d_array" in err(hip) and "%d bytes short" % W in err(hip), err(hip)
        end = raw + nbytes
        rc = hip.FLAGSTATS_hip_device_wide_segments_filter(a, n, W, f, nseg, 0, 0x904, end - n + 1, 30, out.data_ptr(), sel.data_ptr(),
                                                           high.data_ptr(), 0, None)
        assert rc != 0 and "d_mapq" in err(hip) and "1 bytes short" in err(hip), err(hip)
        for name, kw in (("d_out", {"d_out": end - nseg * 256 + 8}), ("d_selected", {"d_selected": end - nseg * 8 + 8}),
                         ("d_high", {"d_high": end - nseg * 8 + 8}), ("d_offsets", {"d_offsets": end - (nseg + 1) * 8 + 8})):
            k = {**good, **kw}
            rc = hip.FLAGSTATS_hip_device_wide_segments_filter(a, n, W, k["d_offsets"], nseg, 0, 0x904, qd, 30, k["d_out"], k["d_selected"],
                                                               k["d_high"], 0, None)
            assert rc != 0 and name in err(hip) and "8 bytes short" in err(hip), (name, err(hip))
        back = np.ones(nbytes, dtype=np.uint8)
        assert hip.FLAGSTATS_hip_memcpy_d2h(back.ctypes.data, raw, nbytes) == 0 and not back.any()
    finally:
        hip.FLAGSTATS_hip_device_free(raw)
    untouched("extents")
    # the launcher itself -- nothing queued: (d_chunk, W, d_mapq, base, m, d_offsets, nseg, require, exclude, min_mapq, out, sel, high, mode, grid)
    p, ps, ph = out.data_ptr(), sel.data_ptr(), high.data_ptr()
    ok = [a, W, qd, 0, 8, f, nseg, 0, 0x904, 30, p, ps, ph, 0, 1]
    for i, bad in ((1, 2), (1, 16), (13, 4), (14, 0), (7, 0x10000), (8, 0x10000), (9, 256), (10, None), (5, None), (0, None), (2, None),
                   (0, a + W // 2), (4, 1 << 34), (4, (1 << 64) // W)):
        args = list(ok)
        args[i] = bad
        assert launcher(*args, None) != 0, (i, bad)
    assert launcher(a, W, None, 0, 8, f, 0, 0, 0, 0, None, None, None, STORE, 1, None) == 0     # nseg == 0
    assert launcher(a, W, None, 0, 8, f, nseg, 1, 0x904, 0, p, ps, ph, 0, 1, None) == 0         # min_mapq == 0 takes a NULL column
    torch.cuda.synchronize()
    untouched("launcher")                                  # (the last launch read 8 zero flags, which fail -f 0x1: nothing is added)


# ------------------------------------------------------------------ 11. the Python layers
def torch_of(x):
    """a CUDA tensor of x's own dtype (unsigned ones through a view of the signed bytes)"""
    import torch
    t = dev(x)
    return t if x.dtype.kind == "i" else t.view(getattr(torch, x.dtype.name))


@pytest.mark.parametrize("dtype", ["int16", "uint16", "int32", "uint32", "int64", "uint64"])
def test_python_layers(hip, dtype):
    import torch
    import libflagstats_amd
    from libflagstats_amd import segments_wide_filter as swf
    import segments_filter_oracle as sfo
    rng = np.random.RandomState(61)
    W = np.dtype(dtype).itemsize
    n = 30_000
    low = rng.randint(0, 65536, n).astype(np.uint16)
    clean = low.view(dtype) if W == 2 else low.astype(dtype)
    q = rng.randint(0, 256, n).astype(np.uint8)
    o = np.array([5, 5, 900, 4000, 4001, 20_000, n - 3], dtype=np.int64)
    nseg = o.size - 1
    kw = dict(require=1, exclude=0x904, min_mapq=30)
    rows_sup, sel = sfo.want(low, o, 1, 0x904, q, 30, superset=True)
    rows_plain, _ = sfo.want(low, o, 1, 0x904, q, 30)
    zero = np.zeros(nseg, dtype=np.uint64)
    assert pass_fraction_inside((rows_sup, sel), o)
    same(swf.counters_segments_ints_filter(clean, o, mapq=q, superset=True, **kw), (rows_sup, sel, zero), (dtype, "counters"))
    got = swf.flagstats_segments_ints_filter(clean, o, mapq=q, **kw)
    same(got, (rows_plain, sel, zero), (dtype, "strict, clean"))
    dicts = libflagstats_amd.segment_filter_dicts(got[0], got[1])
    assert [d["n_values"] for d in dicts] == [int(v) for v in sel]
    t, tq, d_off = torch_of(clean), dev(q), dev64(o)
    rows, s, high = swf.count_segments_torch_ints_filter(t, d_off, mapq=tq, superset=True, **kw)
    torch.cuda.synchronize()
    assert rows.dtype == torch.int64 and tuple(rows.shape) == (nseg, 32) and tuple(s.shape) == (nseg,) and tuple(high.shape) == (nseg,)
    same((u64(rows), u64(s), u64(high)), (rows_sup, sel, zero), (dtype, "torch"))
    if W > 2:
        same(swf.count_segments_device_ptr_ints_filter(t.data_ptr(), n, W, o, mapq_ptr=tq.data_ptr(), superset=True, **kw),
             (rows_sup, sel, zero), (dtype, "device ptr"))
        # a dirty column: strict names the first offending segment, whether its element passes or not
        dirty = clean.copy()
        dirty[4000] = (int(dirty[4000]) & 0xFFFF) | 0x904 | (1 << 16)          # fails -F 0x904
        dirty[25_000] = -5 if np.dtype(dtype).kind == "i" else dirty[25_000] | (1 << 31)
        want = swfo.want(dirty, o, 1, 0x904, q, 30)
        assert np.count_nonzero(want[2]) == 2 and not swfo.pass_vector(dirty, 1, 0x904, q, 30)[4000]
        with pytest.raises(ValueError, match=r"segment 3 \(offsets 4000\.\.4001\): values outside 0\.\.65535: bits 0x10000 set above bit 15"):
            swf.flagstats_segments_ints_filter(dirty, o, mapq=q, **kw)
        same(swf.flagstats_segments_ints_filter(dirty, o, mapq=q, strict=False, **kw), want, (dtype, "strict=False"))
        td = torch_of(dirty)
        # out= / selected= / high= reuse; store=False keeps their values
        got3 = swf.count_segments_torch_ints_filter(td, d_off, mapq=tq, out=rows, selected=s, high=high, store=True, **kw)
        assert got3[0] is rows and got3[1] is s and got3[2] is high
        torch.cuda.synchronize()
        same((u64(rows), u64(s), u64(high)), want, (dtype, "reuse"))
        swf.count_segments_torch_ints_filter(t, d_off, mapq=tq, out=rows, selected=s, high=high, store=False, **kw)
        torch.cuda.synchronize()
        same((u64(rows), u64(s), u64(high)), (want[0] + rows_plain, want[1] + sel, want[2]), (dtype, "store=False"))
    else:
        high.fill_(5)
        swf.count_segments_torch_ints_filter(t, d_off, mapq=tq, out=rows, selected=s, high=high, store=False, superset=True, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(u64(rows), rows_sup * np.uint64(2)) and np.array_equal(u64(s), sel * np.uint64(2)) and (high == 5).all()
        swf.count_segments_torch_ints_filter(t, d_off, mapq=tq, out=rows, selected=s, high=high, store=True, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(u64(rows), rows_plain) and np.array_equal(u64(s), sel) and not high.any()
    for bad, text in (({"out": torch.zeros((nseg, 32), dtype=torch.int64)}, r"out must live on t's device \(cuda:0\), not on cpu"),
                      ({"selected": torch.zeros(nseg, dtype=torch.int64)}, r"selected must live on t's device \(cuda:0\), not on cpu"),
                      ({"high": torch.zeros(nseg, dtype=torch.int64)}, r"high must live on t's device \(cuda:0\), not on cpu"),
                      ({"mapq": tq.cpu(), "min_mapq": 30}, r"mapq must live on t's device \(cuda:0\), not on cpu")):
        with pytest.raises(ValueError, match=text):
            swf.count_segments_torch_ints_filter(t, d_off, **bad)
    with pytest.raises(ValueError, match=r"offsets must live on t's device \(cuda:0\), not on cpu"):
        swf.count_segments_torch_ints_filter(t, d_off.cpu())


# ------------------------------------------------------------------ 12. graph capture and replay
@pytest.mark.parametrize("W, together", [(4, True), (4, False), (8, True), (8, False)])
def test_graph_capture_and_replay(hip, W, together):
    """one plain call, then the device entry and the torch layer captured with torch.cuda.graph (zeroes and one kernel: one chain,
    no branches), replayed, array / MAPQ / offsets rewritten in place, replayed again: a replay counts what the buffers hold then"""
    import torch
    from libflagstats_amd import segments_wide_filter as swf
    rng = np.random.RandomState(71 + W)
    U = 8192 // W
    n = 30 * U + 7
    nseg = 6
    pred = PREDICATES["-f 0x1 -F 0x904 -q 30"]
    sets = []
    for k in range(2):
        x = widen(rng.randint(0, 65536, n).astype(np.uint16), SIGNED[W], rng, every=400 + 300 * k)
        q = rng.randint(0, 256, n).astype(np.uint8)
        o = np.sort(np.concatenate([[3 + k], rng.randint(4, n - 5, nseg - 1), [n - 2 - k]])).astype(np.int64)
        sets.append((x, q, o, swfo.want(x, o, *pred[:2], q, pred[2], superset=True)))
    assert not np.array_equal(sets[0][3][1], sets[1][3][1]) and not np.array_equal(sets[0][3][2], sets[1][3][2])
    t, tq, d_off = dev(sets[0][0]), dev(sets[0][1]), dev64(sets[0][2])
    words, rows, sel, high = prefilled(nseg, STORE, together)
    s = torch.cuda.Stream()
    stream = ctypes.c_void_p(s.cuda_stream)

    def c_call():
        return hip.FLAGSTATS_hip_device_wide_segments_filter(t.data_ptr(), n, W, d_off.data_ptr(), nseg, *pred[:2], tq.data_ptr(), pred[2],
                                                             rows.data_ptr(), sel.data_ptr(), high.data_ptr(), STORE | SUPERSET, stream)

    def torch_call():
        swf.count_segments_torch_ints_filter(t, d_off, require=pred[0], exclude=pred[1], mapq=tq, min_mapq=pred[2], out=rows, selected=sel,
                                             high=high, store=True, superset=True)
        return 0

    for call in (c_call, torch_call):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            assert call() == 0, err(hip)
        torch.cuda.synchronize()
        same((u64(rows), u64(sel), u64(high)), sets[0][3], (W, together, "plain"))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode="global"):
            rc = call()
        assert rc == 0, err(hip)
        torch.cuda.synchronize()
        for x, q, o, want in (sets[0], sets[1], sets[0]):
            t.copy_(dev(x))
            tq.copy_(dev(q))
            d_off.copy_(dev64(o))
            rows.fill_(GARBAGE)
            sel.fill_(GARBAGE)
            high.fill_(GARBAGE)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                g.replay()
            torch.cuda.synchronize()
            same((u64(rows), u64(sel), u64(high)), want, (W, together, call.__name__, "replay"))
        del g
