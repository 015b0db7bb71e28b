"""Segmented flagstat on int32 / int64 columns on the MI355X (csrc/flagstat_segments_wide.hip and the layers above it): rows and
one high-bit mask per segment, against tests/segments_wide_oracle.py; every comparison is exact.

Expected values never come from the code under test: rows are segments_oracle's over the low 16 bits, masks numpy's OR per segment,
periodic inputs (x[i] = pattern[i % P], P prime) get both in O(nseg).  Direct launches (fsk_launch_segments_wide with a small
grid) are placed with segments_wide_oracle.WideWriterSplit, the launcher's work split mirrored, and checked to contain the runs
they are there for."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_wide_oracle as swo  # noqa: E402
from segments_oracle import SEG_EPOCH, segmented_counters  # noqa: E402

pytestmark = pytest.mark.gpu

STORE, SUPERSET = 1, 2
MODES = (1, 0, 3, 2)             # store, +=, store + superset, += + superset
GARBAGE, BIAS, MASK_BIAS = 0x5EED_0000_0BAD, 3, (1 << 48) | (1 << 17)
EVERY_MIN_UNITS = (0, 1, 2, 3, 255, 256, 0xFFFFFFFF)
P = 65_521                       # prime: no vector, row, unit or writer seam is a multiple of the period
SIGNED = {4: np.int32, 8: np.int64}
UNSIGNED = {4: np.uint32, 8: np.uint64}
WIDTHS = (4, 8)


def err(hip):
    return hip.FLAGSTATS_hip_last_error().decode(errors="replace")


def dev(x):
    """the array on the device (torch has signed tensors of every width: the bytes are what counts)"""
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view({2: np.int16, 4: np.int32, 8: np.int64}[x.dtype.itemsize])).cuda()


def dev64(o):
    import torch
    return torch.from_numpy(np.ascontiguousarray(o, dtype=np.int64)).cuda()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


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


def expect(want_sup, want_high, mode):
    """what a call in `mode` must leave in rows prefilled with GARBAGE (store) or BIAS (+=) and masks prefilled with GARBAGE or
    MASK_BIAS"""
    w = want_sup.copy()
    if not mode & SUPERSET:
        w[:, [0, 9, 16]] = 0
    if mode & STORE:
        return w, want_high
    return w + np.uint64(BIAS), want_high | np.uint64(MASK_BIAS)


def prefilled(nseg, mode, together):
    """device rows and masks, prefilled; the masks behind the rows in one allocation, or apart"""
    import torch
    words = torch.full((nseg * 33,), GARBAGE if mode & STORE else BIAS, dtype=torch.int64, device="cuda")
    rows = words[:nseg * 32].view(nseg, 32)
    high = words[nseg * 32:] if together else torch.empty(nseg, dtype=torch.int64, device="cuda")
    high.fill_(GARBAGE if mode & STORE else MASK_BIAS)
    return words, rows, high


def device_form(hip, ptr, n, W, offsets, mode, together=True):
    import torch
    d_off = dev64(offsets)
    nseg = d_off.numel() - 1
    _, rows, high = prefilled(nseg, mode, together)
    torch.cuda.synchronize()
    rc = hip.FLAGSTATS_hip_device_wide_segments(ptr, n, W, d_off.data_ptr(), nseg, rows.data_ptr(), high.data_ptr(), mode, None)
    assert rc == 0, err(hip)
    torch.cuda.synchronize()
    return u64(rows), u64(high)


def host_words(nseg, mode):
    return (np.full((nseg, 32), GARBAGE if mode & STORE else BIAS, dtype=np.uint64),
            np.full(nseg, GARBAGE if mode & STORE else MASK_BIAS, dtype=np.uint64))


def sync_form(hip, ptr, n, W, offsets, mode):
    o = np.ascontiguousarray(offsets, dtype=np.uint64)
    rows, high = host_words(o.size - 1, mode)
    rc = hip.FLAGSTATS_hip_device_wide_segments_sync(ptr, n, W, o.ctypes.data, o.size - 1, rows.ctypes.data, high.ctypes.data, mode)
    assert rc == 0, err(hip)
    return rows, high


def host_form(hip, x, offsets, mode):
    o = np.ascontiguousarray(offsets, dtype=np.uint64)
    rows, high = host_words(o.size - 1, mode)
    rc = hip.FLAGSTATS_hip_wide_x64_segments(x.ctypes.data, x.size, x.dtype.itemsize, o.ctypes.data, o.size - 1, rows.ctypes.data,
                                             high.ctypes.data, mode)
    assert rc == 0, err(hip)
    return rows, high


def same(got, want, what):
    rows, high = got
    bad = np.nonzero((rows != want[0]).any(axis=1))[0]
    assert bad.size == 0, (what, "rows", bad[:8], rows[bad[:2]], want[0][bad[:2]])
    bad = np.nonzero(high != want[1])[0]
    assert bad.size == 0, (what, "masks", bad[:8], [hex(int(v)) for v in high[bad[:4]]], [hex(int(v)) for v in want[1][bad[:4]]])


@pytest.fixture(scope="module")
def launcher(hip):
    hip.fsk_segments_policy.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    hip.fsk_segments_policy.restype = None
    hip.fsk_set_segments_policy.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    hip.fsk_set_segments_policy.restype = None
    return hip.fsk_launch_segments_wide   # prototype attached by _lib.lib()


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


def direct(launcher, ptr, W, base, m, offsets, mode, grid, together=True):
    """one fsk_launch_segments_wide on the null stream into prefilled rows and masks"""
    import torch
    d_off = dev64(offsets)
    nseg = d_off.numel() - 1
    _, rows, high = prefilled(nseg, mode, together)
    torch.cuda.synchronize()
    assert launcher(ptr, W, base, m, d_off.data_ptr(), nseg, rows.data_ptr(), high.data_ptr(), mode, grid, None) == 0
    torch.cuda.synchronize()
    return u64(rows), u64(high)


# ------------------------------------------------------------------ 1. every FLAG value, every layout, mode and form
def layouts_of(n, rng):
    dense = 3 + np.concatenate([[0], np.cumsum(rng.randint(0, 41, 900))])
    return {
        "whole": np.array([0, n]),
        "equal": np.linspace(0, n, 18).astype(np.int64),
        "random": np.sort(np.concatenate([rng.randint(0, n + 1, 40), rng.randint(0, n + 1, 5).repeat(2)])),
        "inner": np.array([101, 101, 4000, 4001, 30_000, n - 77]),
        "dense": np.concatenate([dense, [dense[-1] + 9000, n - 1]]),
    }


@pytest.mark.parametrize("dtype", ["int32", "uint32", "int64", "uint64"])
def test_every_flag_value(hip, dtype):
    rng = np.random.RandomState(5)
    W = np.dtype(dtype).itemsize
    x = widen(np.arange(65536, dtype=np.uint16), dtype, rng)
    n = x.size
    t = dev(x)
    for name, o in layouts_of(n, rng).items():
        want = swo.want(x, o, superset=True)
        assert want[0].any() and want[1].any(), name
        if name in ("random", "dense"):
            assert (want[1] == 0).any() and (np.diff(o) == 0).any(), name      # masks that stay 0, empty segments
        for mode in MODES:
            w = expect(*want, mode)
            same(device_form(hip, t.data_ptr(), n, W, o, mode, together=bool(mode & 2)), w, (name, mode, "device"))
            same(sync_form(hip, t.data_ptr(), n, W, o, mode), w, (name, mode, "sync"))
            same(host_form(hip, x, o, mode), w, (name, mode, "host"))
    # no mask wanted: rows alone
    o = layouts_of(n, rng)["equal"]
    d_off = dev64(o)
    _, rows, _ = prefilled(o.size - 1, STORE, True)
    assert hip.FLAGSTATS_hip_device_wide_segments(t.data_ptr(), n, W, d_off.data_ptr(), o.size - 1, rows.data_ptr(), None, STORE, None) == 0
    assert np.array_equal(u64(rows), expect(*swo.want(x, o, True), STORE)[0])


# ------------------------------------------------------------------ 2. lengths at the vector, row and unit edges; every base phase
@pytest.mark.parametrize("W", WIDTHS)
def test_lengths_and_phases(hip, W):
    import torch
    rng = np.random.RandomState(9)
    V, R, U = 16 // W, 1024 // W, 8192 // W
    edges = [0, 1, V - 1, V, V + 1, R - 1, R, R + 1, U - 1, U, U + 1, 4 * U - 1, 4 * U, 4 * U + 1]
    if W == 4:
        assert edges == [0, 1, 3, 4, 5, 255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193]
    lengths = np.concatenate([edges, rng.choice(edges, 150)])
    rng.shuffle(lengths)
    o = 2 + np.concatenate([[0], np.cumsum(lengths)])
    n = int(o[-1]) + 5
    full = widen(rng.randint(0, 65536, n + V).astype(np.uint16), SIGNED[W], rng)
    t = dev(full)
    assert t.data_ptr() % 16 == 0
    for phase in range(V):
        x = full[phase:phase + n]
        ptr = t.data_ptr() + phase * W
        want = swo.want(x, o, superset=True)
        assert want[1].any() and (want[1] == 0).any()
        for mu in (2, 0xFFFFFFFF):
            with policy(hip, mu):
                for mode in (3, 0):
                    same(device_form(hip, ptr, n, W, o, mode, together=mode == 3), expect(*want, mode), (W, phase, mu, mode))
        same(host_form(hip, x, o, 1), expect(*want, 1), (W, phase, "host"))
    del t
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. a bit reaches its own segment's mask and no other
def isolation_layout(W):
    """grid positions of a 40-unit array launched from position 1 to 40 U - 1 (one slack element of the 16-byte grid on either
    side), at grid 1: writers of 10 units; the segment bounds and the positions to plant bits at, with what each is there for"""
    V, R, U = 16 // W, 1024 // W, 8192 // W
    bounds = [5, U // 2 + 1, U // 2 + 3, 6 * U + 7, 6 * U + R + 3, 7 * U - 1, 7 * U + 1, 25 * U + 5, 25 * U + 5, 38 * U]
    plant = {0: "grid slack in front", 40 * U - 1: "grid slack behind", 1: "gap in front", 4: "gap in front, last",
             38 * U: "gap behind, first", 40 * U - 2: "gap behind, last",
             U // 2 + 5: "per-piece head of the chain segment", 3 * U + 17: "chain run", 5 * U + R + 1: "chain run, last unit",
             6 * U + 3: "per-piece tail of the chain segment", 6 * U + R: "same row as a boundary", 6 * U + 3 * R: "same unit as a boundary",
             10 * U - 1: "writer seam, last of writer 0", 10 * U: "writer seam, first of writer 1", 15 * U + 100: "chain run in writer 1",
             24 * U + 9: "chain run in writer 2", 25 * U + 1: "tail in writer 2", 30 * U + 3: "chain run of the last segment"}
    for b, e in zip(bounds[:-1], bounds[1:]):
        if e > b:
            plant.setdefault(b, "a segment's first")
            plant.setdefault(e - 1, "a segment's last")
    return V, R, U, np.array(bounds, dtype=np.int64), dict(sorted(plant.items()))


@pytest.mark.parametrize("W", WIDTHS)
def test_mask_isolation(hip, launcher, W):
    import torch
    V, R, U, bounds, plant = isolation_layout(W)
    lo0, end = 1, 40 * U - 1
    o = bounds - lo0                                   # array indices
    n = end - lo0
    w = swo.writer_ranges(lo0 * W, n, 1, W)
    p = w.pieces(o, 2)
    assert w.waves == 4 and list(w.end + lo0) == [10 * U, 20 * U, 30 * U, end]
    seg2 = p["seg"] == 2
    assert p["chain"][seg2].tolist() == [5] and p["head"][seg2][0] > 0 and p["tail"][seg2][0] == 7
    assert sorted(p["chain"][p["seg"] == 6].tolist()) == [2, 5, 10] and (p["chain"][np.isin(p["seg"], (0, 1, 3, 4, 5))] == 0).all()
    assert sorted(p["chain"][p["seg"] == 8].tolist()) == [4, 8]
    # a boundary's vector, row and unit hold elements of two segments
    assert bounds[1] % V != 0 and bounds[4] % R != 0 and bounds[5] % U != 0
    rng = np.random.RandomState(13)
    base = rng.randint(0, 65536, 40 * U).astype(UNSIGNED[W])
    nbits = 8 * W - 16
    positions = list(plant)
    t = torch.empty(40 * U, dtype={4: torch.int32, 8: torch.int64}[W], device="cuda")
    assert t.data_ptr() % 16 == 0
    ptr = t.data_ptr() + lo0 * W
    seen = {pos: 0 for pos in positions}
    for shift in range(nbits):
        x = base.copy()
        for j, pos in enumerate(positions):
            bit = 16 + (7 * j + shift) % nbits
            x[pos] |= UNSIGNED[W](1 << bit)
            seen[pos] |= 1 << bit
        t.copy_(dev(x))
        arr = x[lo0:end]
        want = swo.want(arr, o, superset=True)
        # the oracle itself: each planted bit in the mask of the segment that holds it, gaps and slack nowhere
        inside = [pos for pos in positions if bounds[0] <= pos < bounds[-1]]
        assert int(np.bitwise_or.reduce(want[1])) == int(np.bitwise_or.reduce(swo.unsigned(x[inside]) & swo.HIGH))
        for mu, mode in ((2, 1), (2, 0), (0xFFFFFFFF, 1), (0xFFFFFFFF, 0)):
            with policy(hip, mu):
                got = direct(launcher, ptr, W, 0, n, o, mode, 1, together=mode == 1)
            same(got, expect(*want, mode), (W, "shift", shift, "min_units", mu, "mode", mode, plant))
    assert all(v == ((1 << nbits) - 1) << 16 for v in seen.values())   # every bit 16 .. 8 W - 1 at every position
    # a single negative element: the sign bit in its own segment's mask only
    for pos in (U // 2 + 1, 3 * U + 17, 7 * U, 10 * U - 1, 4):
        x = base.copy().view(SIGNED[W])
        x[pos] = np.iinfo(SIGNED[W]).min | int(base[pos] & 0xFFFF)
        t.copy_(dev(x))
        want = swo.want(x[lo0:end], o, superset=True)
        holder = np.nonzero((o[:-1] <= pos - lo0) & (pos - lo0 < o[1:]))[0]
        assert [int(v) for v in want[1][holder]] == ([1 << (8 * W - 1)] if holder.size else []) and np.count_nonzero(want[1]) == holder.size
        same(direct(launcher, ptr, W, 0, n, o, 3, 1), expect(*want, 3), (W, "negative at", pos))


# ------------------------------------------------------------------ 4. chain, epochs and seams
RUNS = (511, 510, 509, 256, 255, 254)


def periodic_column(W, seed, n):
    import torch
    rng = np.random.RandomState(seed)
    pattern = widen(rng.randint(0, 65536, P).astype(np.uint16), SIGNED[W], rng, every=20_000)
    t = dev(pattern).repeat(-(-(n + 16) // P))
    torch.cuda.synchronize()
    return pattern, t


def runs_layout(w, delta):
    """inside every writer: a head, then runs of whole units from RUNS (first fit, each run once; 300 where none fits), every
    boundary `delta` elements off its unit boundary or writer seam"""
    U = w.unit
    left = list(RUNS)
    cuts = []
    for b, e in zip(w.begin, w.end):
        if e <= b:
            continue
        if b > 0:
            cuts.append(int(b) + delta)
        cur = int(-(-(b + w.lo0 + U) // U) * U - w.lo0)
        cuts.append(cur + delta)
        took = False
        for L in list(left) + [300]:
            if cur + (L + 1) * U < e and (L in left or not took):
                cur += L * U
                cuts.append(cur + delta)
                took = True
                if L in left:
                    left.remove(L)
        cuts.append(cur + delta + 3)                    # three elements right behind the writer's last run
    cuts = np.unique(np.clip(cuts, 0, w.n))
    return np.concatenate([[0], cuts[(cuts > 0) & (cuts < w.n)], [w.n]]).astype(np.int64)


@pytest.mark.parametrize("W", WIDTHS)
def test_chain_epochs_and_seams(hip, launcher, W):
    U = 8192 // W
    n = 4 * 770 * U + 5                                 # ~25 MB: at grid 1 each wave owns 770 units
    pattern, t = periodic_column(W, 21 + W, n)
    for grid in (1, 2):
        w = swo.writer_ranges(t.data_ptr() % 16, n, grid, W)
        assert w.waves == 4 * grid
        for delta in (0, 1, -1, 16 // W, -(16 // W)):
            o = runs_layout(w, delta)
            pieces = w.pieces(o, 2)
            chains = set(int(c) for c in pieces["chain"])
            if delta == 0:
                assert set(RUNS if grid == 1 else (254, 255, 256)).issubset(chains), (grid, sorted(chains))
                assert ((pieces["chain"] > SEG_EPOCH) & pieces["plain"]).any()
            else:
                assert max(chains) >= SEG_EPOCH and (~pieces["plain"]).any(), (grid, delta, sorted(chains))
                assert ((pieces["chain"] > 0) & ((pieces["head"] > 0) | (pieces["tail"] > 0))).any()
            assert (pieces["chain"] == 0).any()
            want = swo.periodic_want(pattern, o, superset=True)
            assert (want[1] == 0).any() and want[1].any()
            for mode in (MODES if delta == 0 else (3, 0)):
                same(direct(launcher, t.data_ptr(), W, 0, n, o, mode, grid, together=bool(mode & 1)), expect(*want, mode),
                     (W, grid, delta, mode))
    # every min_units on the layout with the exact runs, at grid 1
    w = swo.writer_ranges(t.data_ptr() % 16, n, 1, W)
    o = runs_layout(w, 0)
    want = swo.periodic_want(pattern, o, superset=True)
    for mu in EVERY_MIN_UNITS:
        chains = w.pieces(o, mu)["chain"]
        assert (chains.max() == 0) == (mu == 0xFFFFFFFF) and (mu not in (255, 256) or mu in chains), mu
        with policy(hip, mu):
            for mode in (3, 0):
                same(direct(launcher, t.data_ptr(), W, 0, n, o, mode, 1), expect(*want, mode), (W, "min_units", mu, mode))
    # a chunk of the array launched alone (base != 0): offsets before, inside and behind it are clamped to it
    c0, m = 3 * U - 1, 700 * U + 9
    clipped = np.clip(o, c0, c0 + m)
    want = swo.periodic_want(pattern, clipped, superset=True)
    assert (o < c0).any() and (o > c0 + m).any()
    for mode in (3, 0):
        same(direct(launcher, t.data_ptr() + c0 * W, W, c0, m, o, mode, 1), expect(*want, mode), (W, "chunk", mode))
    del t


# ------------------------------------------------------------------ 5. accumulate
@pytest.mark.parametrize("W", WIDTHS)
def test_accumulate_and_streams(hip, W):
    import torch
    rng = np.random.RandomState(33)
    U = 8192 // W
    n = 36 * U + 11
    x = widen(rng.randint(0, 65536, n).astype(np.uint16), SIGNED[W], rng, every=500)
    o = np.array([0, 50, 3 * U + 1, 3 * U + 1, 20 * U - 7, 36 * U], dtype=np.int64)
    nseg = o.size - 1
    want = swo.want(x, o, superset=True)
    t, d_off = dev(x), dev64(o)
    rows = torch.zeros((nseg, 32), dtype=torch.int64, device="cuda")
    high = torch.zeros(nseg, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):
        assert hip.FLAGSTATS_hip_device_wide_segments(t.data_ptr(), n, W, d_off.data_ptr(), nseg, rows.data_ptr(), high.data_ptr(), SUPERSET, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(u64(rows), want[0] * np.uint64(2)) and np.array_equal(u64(high), want[1])
    # nseg == 0 does nothing, in either form
    for flags in (0, STORE):
        assert hip.FLAGSTATS_hip_device_wide_segments(t.data_ptr(), n, W, None, 0, None, None, flags, None) == 0
        assert hip.FLAGSTATS_hip_device_wide_segments(t.data_ptr(), n, W, d_off.data_ptr(), 0, rows.data_ptr(), high.data_ptr(), flags, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(u64(rows), want[0] * np.uint64(2)) and np.array_equal(u64(high), want[1])
    # two streams, two arrays, one set of rows and masks
    y = rng.randint(0, 65536, n).astype(UNSIGNED[W])
    y[10] |= UNSIGNED[W](1 << 16)                        # segment 0, whose mask is 0 in x
    y[3 * U + 5] |= UNSIGNED[W](1 << (8 * W - 2))
    want_y = swo.want(y, o, superset=True)
    assert want[1][0] == 0 and [int(v) for v in want_y[1]] == [1 << 16, 0, 0, 1 << (8 * W - 2), 0]
    ty = dev(y)
    rows.zero_()
    high.zero_()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    for st, tt in zip(streams, (t, ty)):
        rc = hip.FLAGSTATS_hip_device_wide_segments(tt.data_ptr(), n, W, d_off.data_ptr(), nseg, rows.data_ptr(), high.data_ptr(), SUPERSET,
                                                    ctypes.c_void_p(st.cuda_stream))
        assert rc == 0, err(hip)
    for st in streams:
        st.synchronize()
    assert np.array_equal(u64(rows), want[0] + want_y[0]) and np.array_equal(u64(high), want[1] | want_y[1])


# ------------------------------------------------------------------ 6. against the entries that exist
@pytest.mark.parametrize("W", WIDTHS)
def test_cross_checks(hip, W):
    import torch
    from libflagstats_amd import segments, wide
    rng = np.random.RandomState(41)
    U = 8192 // W
    n = 50 * U + 3
    x = widen(rng.randint(0, 65536, n).astype(np.uint16), SIGNED[W], rng, every=300)
    o = np.unique(np.concatenate([[7], rng.randint(7, n - 9, 30), [12 * U, 30 * U + 1, n - 9]]))
    t, d_off = dev(x), dev64(o)
    for sup in (False, True):
        rows, high = device_form(hip, t.data_ptr(), n, W, o, STORE | (SUPERSET if sup else 0))
        out32, h1 = wide.count_torch_ints(t[int(o[0]):int(o[-1])], store=True, superset=sup)
        torch.cuda.synchronize()
        assert np.array_equal(rows.sum(axis=0), u64(out32)), sup
        assert int(np.bitwise_or.reduce(high)) == int(u64(h1)[0]) != 0
    # a zero-extended uint16 column: the rows of the uint16 entry, no mask
    low = rng.randint(0, 65536, n).astype(np.uint16)
    z = low.astype(UNSIGNED[W])
    tz = dev(z)
    rows, high = device_form(hip, tz.data_ptr(), n, W, o, STORE | SUPERSET, together=False)
    got16 = segments.count_segments_torch(dev(low), d_off, superset=True)
    torch.cuda.synchronize()
    assert np.array_equal(rows, u64(got16)) and not high.any()


# ------------------------------------------------------------------ 7. host form across chunks
@pytest.mark.parametrize("W", WIDTHS)
def test_host_form_across_chunks(hip, W):
    from libflagstats_amd import _lib
    from libflagstats_amd import segments_wide as sw
    rng = np.random.RandomState(53)
    chunk_flags = 16_386                                 # 32,772 bytes: 8,193 int32 or 4,096.5 -> 4,096 int64 a chunk
    c = chunk_flags * 2 // W
    n = 7 * c + 77
    x = rng.randint(0, 65536, n + 1).astype(UNSIGNED[W])[1:]        # no high bits yet; the array starts one element into its buffer
    first = 3
    o = np.array([first, 10, 10, first + c + 7, first + c + c // 2, first + 3 * c + c // 2 + 5, first + 4 * c, n - 20], dtype=np.int64)
    # segment 2 spans chunks 0 and 1, segment 4 chunks 1, 2 and 3, segment 6 begins on a chunk boundary;
    # masks planted in different chunks of one segment, and one in the first element of a chunk
    x[first + c + c // 2 + 1] |= UNSIGNED[W](1 << 16)
    x[first + 2 * c + 9] |= UNSIGNED[W](1 << 20)
    x[first + 3 * c + c // 2 + 4] |= UNSIGNED[W](1 << (8 * W - 1))
    x[first + 4 * c] |= UNSIGNED[W](1 << 17)
    x[1], x[n - 1] = x[1] | UNSIGNED[W](1 << 30), x[n - 1] | UNSIGNED[W](1 << 29)       # outside every segment
    x = x.view(SIGNED[W])
    want = swo.want(x, o, superset=True)
    assert [hex(int(v)) for v in want[1]] == [hex(v) for v in (0, 0, 0, 0, (1 << 16) | (1 << 20) | (1 << (8 * W - 1)), 0, 1 << 17)]
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", chunk_flags), "chunk_flags")
        for mode in MODES:
            same(host_form(hip, x, o, mode), expect(*want, mode), (W, "chunks", mode))
        got = sw.counters_segments_ints(x, o, superset=True)
        same(got, want, (W, "python"))
        for oo in (np.array([1, 50, 99]), np.array([7, 7, 7]), np.array([n, n])):        # one chunk only; nothing covered
            same(sw.counters_segments_ints(x, oo), swo.want(x, oo), (W, oo))
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old
    got = sw.counters_segments_ints(x[:0], [0, 0])
    assert got[0].shape == (1, 32) and not got[0].any() and not got[1].any()


# ------------------------------------------------------------------ 8. refusals
@pytest.mark.parametrize("W", WIDTHS)
def test_refusals(hip, launcher, W):
    import torch
    n, nseg = 4096, 3
    t = torch.zeros(n + 8, dtype={4: torch.int32, 8: torch.int64}[W], device="cuda")
    host = np.zeros(n + 8, dtype=SIGNED[W])
    o = np.array([0, 10, 2000, n], dtype=np.uint64)
    d_off = dev64(o)
    out = torch.full((nseg, 32), BIAS, dtype=torch.int64, device="cuda")
    high = torch.full((nseg,), MASK_BIAS, dtype=torch.int64, device="cuda")
    h_out = np.full((nseg, 32), BIAS, dtype=np.uint64)
    h_high = np.full(nseg, MASK_BIAS, dtype=np.uint64)

    def untouched(what):
        torch.cuda.synchronize()
        assert (out == BIAS).all() and (high == MASK_BIAS).all(), what
        assert (h_out == BIAS).all() and (h_high == MASK_BIAS).all(), what

    def refused(what, text, d_array=t.data_ptr(), n_=n, eb=W, offsets=o, nseg_=nseg, flags=0, rows=True, forms=("device", "sync", "host")):
        d_o = None if offsets is None else dev64(offsets.astype(np.int64))
        for form in forms:
            if form == "device":
                rc = hip.FLAGSTATS_hip_device_wide_segments(d_array, n_, eb, None if d_o is None else d_o.data_ptr(), nseg_,
                                                            out.data_ptr() if rows else None, high.data_ptr(), flags, None)
            elif form == "sync":
                rc = hip.FLAGSTATS_hip_device_wide_segments_sync(d_array, n_, eb, None if offsets is None else offsets.ctypes.data, nseg_,
                                                                 h_out.ctypes.data if rows else None, h_high.ctypes.data, flags)
            else:
                src = host.ctypes.data + (d_array - t.data_ptr()) if d_array else None
                rc = hip.FLAGSTATS_hip_wide_x64_segments(src, n_, eb, None if offsets is None else offsets.ctypes.data, nseg_,
                                                         h_out.ctypes.data if rows else None, h_high.ctypes.data, flags)
            assert rc != 0, (what, form)
            assert err(hip) and text in err(hip), (what, form, err(hip))
        untouched(what)

    refused("elem_bytes 2", "16-bit arrays go to the u16 entries", eb=2)
    for eb in (0, 1, 3, 16, -4):
        refused("elem_bytes %d" % eb, "elem_bytes must be 4 or 8", eb=eb)
    refused("a misaligned array", "%d-byte aligned" % W, d_array=t.data_ptr() + W // 2)
    refused("NULL array", "NULL array with n > 0", d_array=None)
    refused("NULL offsets", "with nseg > 0", offsets=None)
    refused("NULL rows", "with nseg > 0", rows=False)
    refused("an extra flag bit", "no other bits", flags=4)
    refused("too many segments", "nseg is too large", nseg_=1 << 60)
    refused("n * elem_bytes is no size", "is not a size", n_=1 << 63)
    refused("decreasing offsets", "offsets must be non-decreasing", offsets=np.array([0, 20, 10, n], dtype=np.uint64), forms=("sync", "host"))
    refused("offsets past the array", "exceeds the array's", offsets=np.array([0, 10, 20, n + 1], dtype=np.uint64), forms=("sync", "host"))
    # host pointers (pageable, then page-locked) where device memory is needed
    a, f = t.data_ptr(), d_off.data_ptr()
    for name, args in (("d_out", (a, n, W, f, nseg, h_out.ctypes.data, high.data_ptr())), ("d_high", (a, n, W, f, nseg, out.data_ptr(), h_high.ctypes.data)),
                       ("d_offsets", (a, n, W, o.ctypes.data, nseg, out.data_ptr(), high.data_ptr())),
                       ("d_array", (host.ctypes.data, n, W, f, nseg, out.data_ptr(), high.data_ptr()))):
        rc = hip.FLAGSTATS_hip_device_wide_segments(*args, 0, None)
        assert rc != 0 and name in err(hip), (name, err(hip))
    rc = hip.FLAGSTATS_hip_device_wide_segments_sync(host.ctypes.data, n, W, o.ctypes.data, nseg, h_out.ctypes.data, h_high.ctypes.data, 0)
    assert rc != 0 and "d_array" in err(hip), err(hip)
    pinned = hip.FLAGSTATS_hip_host_alloc(1024)
    assert pinned
    try:
        ctypes.memset(pinned, 0, 1024)
        rc = hip.FLAGSTATS_hip_device_wide_segments(a, n, W, f, nseg, pinned, high.data_ptr(), STORE, None)
        assert rc != 0 and "d_out must be device memory" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_segments(a, n, W, f, nseg, out.data_ptr(), pinned, STORE, None)
        assert rc != 0 and "d_high must be device memory" in err(hip), err(hip)
        assert not any(ctypes.string_at(pinned, 1024))
    finally:
        hip.FLAGSTATS_hip_host_free(pinned)
    untouched("host pointers")
    # pointers on different devices and a stream of another device need a second GPU
    if torch.cuda.device_count() > 1:
        other = torch.zeros((nseg, 32), dtype=torch.int64, device="cuda:1")
        rc = hip.FLAGSTATS_hip_device_wide_segments(a, n, W, f, nseg, other.data_ptr(), None, 0, None)
        assert rc != 0 and "different devices" in err(hip), err(hip)
        with torch.cuda.device(1):
            s1 = torch.cuda.Stream()
        rc = hip.FLAGSTATS_hip_device_wide_segments(a, n, W, f, nseg, out.data_ptr(), high.data_ptr(), 0, ctypes.c_void_p(s1.cuda_stream))
        assert rc != 0 and err(hip), err(hip)
        untouched("another device")
    # extents: the array one element short, rows, masks and offsets 8 bytes short
    nbytes = 2 << 20
    raw = hip.FLAGSTATS_hip_device_alloc(nbytes)
    assert raw
    try:
        assert hip.FLAGSTATS_hip_memcpy_h2d(raw, np.zeros(nbytes, dtype=np.uint8).ctypes.data, nbytes) == 0
        big_off = dev64(np.array([0, 5, 100, nbytes // W]))
        rc = hip.FLAGSTATS_hip_device_wide_segments(raw, nbytes // W + 1, W, big_off.data_ptr(), nseg, out.data_ptr(), high.data_ptr(), STORE, None)
        assert rc != 0 and "d_array" in err(hip) and "%d bytes short" % W in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide_segments_sync(raw, nbytes // W + 1, W, np.array([0, 5, 100, nbytes // W], dtype=np.uint64).ctypes.data,
                                                         nseg, h_out.ctypes.data, h_high.ctypes.data, STORE)
        assert rc != 0 and "d_array" in err(hip) and "%d bytes short" % W in err(hip), err(hip)
        end = raw + nbytes
        for name, kw in (("d_out", {"rows": end - nseg * 256 + 8}), ("d_high", {"masks": end - nseg * 8 + 8}),
                         ("d_offsets", {"offsets": end - (nseg + 1) * 8 + 8})):
            rc = hip.FLAGSTATS_hip_device_wide_segments(a, n, W, kw.get("offsets", f), nseg, kw.get("rows", out.data_ptr()),
                                                        kw.get("masks", high.data_ptr()), 0, None)
            assert rc != 0 and name in err(hip) and "8 bytes short" in err(hip), (name, err(hip))
        back = np.ones(nbytes, dtype=np.uint8)
        assert hip.FLAGSTATS_hip_memcpy_d2h(back.ctypes.data, raw, nbytes) == 0 and not back.any()
    finally:
        hip.FLAGSTATS_hip_device_free(raw)
    untouched("extents")
    # the launcher itself: other widths and mode bits, no workgroups, NULLs, misalignment, a wave's uint32 totals -- nothing queued
    p, ph = out.data_ptr(), high.data_ptr()
    for args in ((a, 2, 0, 8, f, nseg, p, ph, 0, 1), (a, W, 0, 8, f, nseg, p, ph, 4, 1), (a, W, 0, 8, f, nseg, p, ph, 0, 0),
                 (a, W, 0, 8, f, nseg, None, ph, 0, 1), (a, W, 0, 8, None, nseg, p, ph, 0, 1), (None, W, 0, 8, f, nseg, p, ph, 0, 1),
                 (a + W // 2, W, 0, 8, f, nseg, p, ph, 0, 1), (a, W, 0, 1 << 34, f, nseg, p, ph, 0, 1)):
        assert launcher(*args, None) != 0, args
    assert launcher(a, W, 0, 8, f, 0, None, None, STORE, 1, None) == 0
    untouched("launcher")


# ------------------------------------------------------------------ 9. the Python layers
def torch_of(x):
    """a CUDA tensor of x's own dtype (unsigned ones through a view of the signed bytes)"""
    import torch
    t = dev(x)
    return t if x.dtype.kind == "i" else t.view(getattr(torch, x.dtype.name))


@pytest.mark.parametrize("dtype", ["int16", "uint16", "int32", "uint32", "int64", "uint64"])
def test_python_layers(hip, dtype):
    import torch
    from libflagstats_amd import segments_wide as sw
    rng = np.random.RandomState(61)
    W = np.dtype(dtype).itemsize
    n = 30_000
    low = rng.randint(0, 65536, n).astype(np.uint16)
    clean = low.view(dtype) if W == 2 else low.astype(dtype)
    o = np.array([5, 5, 900, 4000, 4001, 20_000, n - 3], dtype=np.int64)
    nseg = o.size - 1
    want_rows = segmented_counters(low, o, superset=True)
    plain_rows = segmented_counters(low, o)
    zero = np.zeros(nseg, dtype=np.uint64)
    # clean columns: all four functions, strict does not raise
    same(sw.counters_segments_ints(clean, o, superset=True), (want_rows, zero), (dtype, "counters"))
    same(sw.flagstats_segments_ints(clean, o), (plain_rows, zero), (dtype, "strict, clean"))
    t = torch_of(clean)
    d_off = dev64(o)
    rows, high = sw.count_segments_torch_ints(t, d_off, superset=True)
    torch.cuda.synchronize()
    assert rows.dtype == torch.int64 and tuple(rows.shape) == (nseg, 32) and tuple(high.shape) == (nseg,)
    same((u64(rows), u64(high)), (want_rows, zero), (dtype, "torch"))
    if W > 2:
        same(sw.count_segments_device_ptr_ints(t.data_ptr(), n, W, o, superset=True), (want_rows, zero), (dtype, "device ptr"))
        # a dirty column: strict names the first offending segment
        dirty = clean.copy()
        dirty[4000] = dirty[4000] | (1 << 16)
        dirty[25_000] = -5 if np.dtype(dtype).kind == "i" else dirty[25_000] | (1 << 31)
        want = swo.want(dirty, o)
        assert np.count_nonzero(want[1]) == 2
        with pytest.raises(ValueError, match=r"segment 3 \(offsets 4000\.\.4001\): values outside 0\.\.65535: bits 0x10000 set above bit 15"):
            sw.flagstats_segments_ints(dirty, o)
        same(sw.flagstats_segments_ints(dirty, o, strict=False), want, (dtype, "strict=False"))
        td = torch_of(dirty)
        same(sw.count_segments_device_ptr_ints(td.data_ptr(), n, W, o), want, (dtype, "device ptr, dirty"))
        # out= / high= reuse, store=False
        rows2, high2 = sw.count_segments_torch_ints(td, d_off, out=rows, high=high, store=True)
        assert rows2 is rows and high2 is high
        torch.cuda.synchronize()
        same((u64(rows), u64(high)), want, (dtype, "reuse"))
        sw.count_segments_torch_ints(t, d_off, out=rows, high=high, store=False)
        torch.cuda.synchronize()
        same((u64(rows), u64(high)), (want[0] + plain_rows, want[1]), (dtype, "store=False"))
    else:
        high.fill_(5)
        sw.count_segments_torch_ints(t, d_off, out=rows, high=high, store=False, superset=True)
        torch.cuda.synchronize()
        assert np.array_equal(u64(rows), want_rows * np.uint64(2)) and (high == 5).all()
        sw.count_segments_torch_ints(t, d_off, out=rows, high=high, store=True)
        torch.cuda.synchronize()
        assert np.array_equal(u64(rows), plain_rows) and not high.any()
    # the wrong device, dtype and shape
    for kw, text in (({"out": torch.zeros((nseg, 32), dtype=torch.int64)}, r"out must live on t's device \(cuda:0\), not on cpu"),
                     ({"high": torch.zeros(nseg, dtype=torch.int64)}, r"high must live on t's device \(cuda:0\), not on cpu"),
                     ({"out": torch.zeros((nseg, 32), dtype=torch.int32, device="cuda")}, r"out must be a contiguous int64 tensor of shape"),
                     ({"high": torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")}, r"high must be a contiguous int64 tensor of shape"),
                     ({"out": torch.zeros((nseg + 1, 32), dtype=torch.int64, device="cuda")}, r"out must be a contiguous int64 tensor of shape")):
        with pytest.raises(ValueError, match=text):
            sw.count_segments_torch_ints(t, d_off, **kw)
    with pytest.raises(ValueError, match=r"offsets must live on t's device \(cuda:0\), not on cpu"):
        sw.count_segments_torch_ints(t, d_off.cpu())
    with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
        sw.count_segments_torch_ints(t.cpu(), d_off)


# ------------------------------------------------------------------ 10. graph capture
@pytest.mark.parametrize("W, together", [(4, True), (4, False), (8, True), (8, False)])
def test_graph_capture_and_replay(hip, W, together):
    """one plain call, then the device entry captured with torch.cuda.graph (its zeroes and its kernel: one chain, no branches),
    replayed, array / offsets / outputs rewritten in place, replayed again: a replay counts what the buffers hold then"""
    import torch
    rng = np.random.RandomState(71 + W)
    U = 8192 // W
    n = 30 * U + 7
    nseg = 6
    sets = []
    for k in range(2):
        x = widen(rng.randint(0, 65536, n).astype(np.uint16), SIGNED[W], rng, every=400 + 300 * k)
        o = np.sort(np.concatenate([[3 + k], rng.randint(4, n - 5, nseg - 1), [n - 2 - k]])).astype(np.int64)
        sets.append((x, o, swo.want(x, o, superset=True)))
    assert not np.array_equal(sets[0][2][1], sets[1][2][1])
    t, d_off = dev(sets[0][0]), dev64(sets[0][1])
    words, rows, high = prefilled(nseg, STORE, together)
    s = torch.cuda.Stream()
    stream = ctypes.c_void_p(s.cuda_stream)

    def call():
        return hip.FLAGSTATS_hip_device_wide_segments(t.data_ptr(), n, W, d_off.data_ptr(), nseg, rows.data_ptr(), high.data_ptr(),
                                                      STORE | SUPERSET, stream)

    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert call() == 0, err(hip)
    torch.cuda.synchronize()
    same((u64(rows), u64(high)), sets[0][2], (W, together, "plain"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="global"):
        rc = call()
    assert rc == 0, err(hip)
    torch.cuda.synchronize()
    for x, o, want in (sets[0], sets[1], sets[0]):
        t.copy_(dev(x))
        d_off.copy_(dev64(o))
        rows.fill_(GARBAGE)
        high.fill_(GARBAGE)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        same((u64(rows), u64(high)), want, (W, together, "replay"))
    del g
