"""The wide-input flagstat on the MI355X: int32 / int64 FLAG arrays counted in place (fsk::flagstat_count_wide, the three C
entries, libflagstats_amd/wide.py), with the mask of bits seen above bit 15.

Expected counters never come from the code under test: oracle.flagstat_c of the low 16 bits (superset slots from
oracle.samtools_counts and the definition), segments_oracle.periodic_counters for periodic inputs; the expected mask is
np.bitwise_or.reduce(v.view(unsigned) & ~0xFFFF).  Layouts are checked against steps_oracle.StepSplit(addr % 16, n * W / 2, grid),
the launcher's step split."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from segments_oracle import periodic_counters  # noqa: E402
from steps_oracle import EPOCH, StepSplit, k1_starts  # noqa: E402

pytestmark = pytest.mark.gpu

STORE, SUPERSET = 1, 2
GARBAGE, BIAS = 0x5EED_0000_0BAD, 3
WIDTHS = (4, 8)
STEP = {4: 8192, 8: 4096}                     # elements of one 32 KiB step
ALL_HIGH = {4: 0xFFFF0000, 8: 0xFFFFFFFFFFFF0000}
SIGNED = {2: np.int16, 4: np.int32, 8: np.int64}
UNSIGNED = {2: np.uint16, 4: np.uint32, 8: np.uint64}


def tdtype(W):
    import torch
    return {4: torch.int32, 8: torch.int64}[W]


def low16(v):
    return (np.asarray(v).view(UNSIGNED[v.dtype.itemsize]) & 0xFFFF).astype(np.uint16)


def want_counters(oracle_mod, v, superset=False):
    x = low16(v)
    if x.size == 0:
        return np.zeros(32, dtype=np.uint64)
    c = oracle_mod.flagstat_c(x).astype(np.uint64)
    if superset:
        pa = oracle_mod.samtools_counts(x)["n_pair_all"]
        c[0], c[16] = pa[0], pa[1]
        c[9] = x.size - int(c[25])
    return c


def want_high(v):
    u = np.asarray(v).view(UNSIGNED[v.dtype.itemsize])
    if u.size == 0:
        return 0
    return int(np.bitwise_or.reduce(u & UNSIGNED[v.dtype.itemsize](ALL_HIGH[v.dtype.itemsize])))


def to_device(v):
    """a numpy array of a 4- or 8-byte integer dtype as a CUDA tensor of the signed dtype of its width"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(v).view(SIGNED[v.dtype.itemsize])).cuda()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def err(hip):
    return hip.FLAGSTATS_hip_last_error().decode(errors="replace")


def launch(hip, ptr, n, W, mode, grid, out=None, high=None, no_high=False):
    """fsk_launch_wide into fresh device words: += into BIAS / 1 << 40, or store over GARBAGE; returns (uint64[32], high)"""
    import torch
    store = bool(mode & STORE)
    if out is None:
        out = torch.full((32,), GARBAGE if store else BIAS, dtype=torch.int64, device="cuda")
    if high is None:
        high = torch.full((1,), GARBAGE if store else 1 << 40, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = hip.fsk_launch_wide(ptr, n, W, out.data_ptr(), None if no_high else high.data_ptr(), mode, grid, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return u64(out), int(u64(high)[0])


def expect_row(want, mode):
    """what a launch() row must read: the superset counters `want` cut to the form, over BIAS in the += form"""
    w = want.copy()
    if not mode & SUPERSET:
        w[[0, 9, 16]] = 0
    return w if mode & STORE else w + np.uint64(BIAS)


def expect_mask(h, mode):
    return h if mode & STORE else h | (1 << 40)


# ------------------------------------------------------------------ 1. every value
@pytest.mark.parametrize("dtype", ["int32", "uint32", "int64", "uint64"])
def test_every_value_through_every_form(hip, oracle_mod, dtype):
    """0..65535 once each: SURVEY Appendix A's K = 65536 vector, high == 0; the same values | 0xFFFF0000: the same counters, high
    == 0xFFFF0000 -- device form (torch's stream), _sync form, host form"""
    import torch
    from libflagstats_amd import wide
    base = np.arange(65536, dtype=np.uint64)
    want = oracle_mod.flagstat_c(np.arange(65536, dtype=np.uint32).astype(np.uint16)).astype(np.uint64)
    W = np.dtype(dtype).itemsize
    for orv, hexp in ((0, 0), (0xFFFF0000, 0xFFFF0000)):
        v = (base | np.uint64(orv)).astype(UNSIGNED[W]).view(dtype)
        assert want_high(v) == hexp and np.array_equal(low16(v), base.astype(np.uint16))
        got, high = wide.counters_ints(v)                                               # host form
        assert np.array_equal(got, want) and high == hexp, (dtype, orv, "host")
        t = to_device(v)
        got, high = wide.count_device_ptr_ints(t.data_ptr(), t.numel(), W)              # _sync form
        assert np.array_equal(got, want) and high == hexp, (dtype, orv, "sync")
        o, h = wide.count_torch_ints(t, store=True)                                     # device form
        torch.cuda.synchronize()
        assert np.array_equal(u64(o), want) and int(u64(h)[0]) == hexp, (dtype, orv, "device")


# ------------------------------------------------------------------ 2. lengths and phases
@pytest.mark.parametrize("W", WIDTHS)
def test_lengths_and_phases(hip, oracle_mod, W):
    """n around nothing, a vector and one and two steps, at every element phase of a 16-byte line, inside a slab whose
    surrounding 64 elements are all-ones: one element read outside [0, n) lights every fail-QC counter and every mask bit"""
    import torch
    S = STEP[W]
    rng = np.random.RandomState(100 + W)
    body = rng.randint(0, 65536, 2 * S + 1).astype(SIGNED[W])
    slab = torch.full((64 + 4 + 2 * S + 1 + 64,), -1, dtype=tdtype(W), device="cuda")
    assert slab.data_ptr() % 16 == 0
    body_t = to_device(body)
    stream = None
    for n in (0, 1, 2, 3, 4, 5, 7, 8, 9, S - 1, S, S + 1, 2 * S - 1, 2 * S + 1):
        want = want_counters(oracle_mod, body[:n], superset=True)
        for phase in range(16 // W):
            slab.fill_(-1)
            slab[64 + phase:64 + phase + n] = body_t[:n]
            ptr = slab.data_ptr() + W * (64 + phase)
            assert ptr % 16 == phase * W
            for flags in (STORE | SUPERSET, 0):
                out = torch.full((32,), GARBAGE if flags & STORE else BIAS, dtype=torch.int64, device="cuda")
                high = torch.full((1,), GARBAGE if flags & STORE else 1 << 40, dtype=torch.int64, device="cuda")
                rc = hip.FLAGSTATS_hip_device_wide(ptr if n else None, n, W, out.data_ptr(), high.data_ptr(), flags, stream)
                assert rc == 0, err(hip)
                torch.cuda.synchronize()
                what = (W, n, phase, flags)
                assert np.array_equal(u64(out), expect_row(want, flags)), (what, u64(out), expect_row(want, flags))
                assert int(u64(high)[0]) == expect_mask(0, flags), (what, hex(int(u64(high)[0])))


# ------------------------------------------------------------------ 3. the mask is exact and local
def mask_positions(W, phase, n, grid):
    """element positions that exercise every place a dword can sit: array ends, both sides of a 16-byte vector, a wave's 8 KiB
    and a step boundary, the head and tail edge steps, a fast step owned by the last workgroup"""
    s = StepSplit(phase * W, n * W // 2, grid)
    epv, S = 16 // W, STEP[W]
    lo = phase
    assert s.grid == grid and s.head_edge and s.tail_edge and s.fast_end - s.fast_begin >= 2 * grid
    last_fast = [st for st in s.pushes(grid - 1) if s.fast_begin <= st < s.fast_end]
    assert last_fast and last_fast[-1] % grid == grid - 1
    g = lambda q: q - lo                                     # grid position -> array index  # noqa: E731
    pos = {"first": 0, "last": n - 1,
           "vector end": g(S + 5 * epv) - 1, "vector begin": g(S + 5 * epv),
           "wave end": g(S + S // 4) - 1, "wave begin": g(S + S // 4),
           "step end": g(3 * S) - 1, "step begin": g(3 * S),
           "head edge": g(S) - 7, "tail edge": g((s.nsteps - 1) * S) + 3,
           "last workgroup": g(last_fast[-1] * S) + 777}
    assert (pos["head edge"] + lo) // S == 0 and (pos["tail edge"] + lo) // S == s.nsteps - 1
    assert all(0 <= p < n for p in pos.values())
    return pos


@pytest.mark.parametrize("W", WIDTHS)
def test_mask_is_exact_and_local(hip, oracle_mod, W):
    import torch
    S = STEP[W]
    phase, grid = 16 // W - 1, 3
    n = 9 * S + S // 3
    rng = np.random.RandomState(7 + W)
    pattern = rng.randint(0, 65536, 977).astype(np.uint16)
    body = np.resize(pattern, n).astype(SIGNED[W])
    want = want_counters(oracle_mod, body, superset=True)
    slab = torch.full((64 + phase + n + 64,), -1, dtype=tdtype(W), device="cuda")
    slab[64 + phase:64 + phase + n] = to_device(body)
    arr = slab[64 + phase:64 + phase + n]
    ptr = arr.data_ptr()
    assert ptr % 16 == phase * W
    out = torch.empty((32,), dtype=torch.int64, device="cuda")
    high = torch.empty((1,), dtype=torch.int64, device="cuda")
    got, h = launch(hip, ptr, n, W, STORE | SUPERSET, grid)
    assert np.array_equal(got, want) and h == 0
    for name, p in mask_positions(W, phase, n, grid).items():
        for b in range(16, 8 * W):
            bit = 1 << b
            signed = bit - (1 << 8 * W) if b == 8 * W - 1 else bit
            arr[p] = int(body[p]) | signed
            got, h = launch(hip, ptr, n, W, STORE | SUPERSET, grid, out=out, high=high)
            assert h == bit, (W, name, p, b, hex(h))
            assert np.array_equal(got, want), (W, name, p, b)
        arr[p] = int(body[p])
    # all 0xFFFF: no high bit; all -1: every bit above 15
    arr.fill_(0xFFFF)
    got, h = launch(hip, ptr, n, W, STORE, grid)
    assert h == 0 and got[25] == n
    arr.fill_(-1)
    ones = got.copy()
    got, h = launch(hip, ptr, n, W, STORE, grid)
    assert h == ALL_HIGH[W] and np.array_equal(got, ones)
    # += ORs onto a pre-set word, store overwrites it, NULL d_high is fine
    arr[:] = to_device(body)
    arr[n // 2] = int(body[n // 2]) | (1 << 17)
    got, h = launch(hip, ptr, n, W, 0, grid)
    assert h == (1 << 40) | (1 << 17) and np.array_equal(got, expect_row(want, 0))
    got, h = launch(hip, ptr, n, W, STORE, grid)
    assert h == 1 << 17 and np.array_equal(got, expect_row(want, STORE))
    for mode in (0, STORE | SUPERSET):
        got, h = launch(hip, ptr, n, W, mode, grid, no_high=True)
        assert np.array_equal(got, expect_row(want, mode)) and h == (GARBAGE if mode & STORE else 1 << 40)
    for flags in (0, STORE):
        o = torch.full((32,), BIAS, dtype=torch.int64, device="cuda")
        assert hip.FLAGSTATS_hip_device_wide(ptr, n, W, o.data_ptr(), None, flags, None) == 0, err(hip)
        torch.cuda.synchronize()
        assert np.array_equal(u64(o), expect_row(want, flags))
    o = np.full(32, BIAS, dtype=np.uint64)
    assert hip.FLAGSTATS_hip_device_wide_sync(ptr, n, W, o.ctypes.data, None, 0) == 0, err(hip)
    assert np.array_equal(o, expect_row(want, 0))


# ------------------------------------------------------------------ 4. epoch regimes
GRIDS = (1, 2, 3, 7)
# the issue's per-workgroup push counts, and the ones that put a workgroup at the first flush of the staggered waves (they start
# their count at 64, 128 and 192: first flush after 191, 127 and 63 pushes)
COUNTS = (254, 255, 256, 509, 510, 511, 1003) + (62, 63, 64, 126, 127, 128, 190, 191, 192)
# prime periods, values with bits above 15 in some elements (W = 8: up to bit 62)
PERIODIC_LOW = np.random.RandomState(303).randint(0, 65536, 65_521).astype(np.uint16)
RICH_LOW = np.resize(np.array([0x443, 0x4C3, 0x643, 0x483, 0xC43, 0x543, 0x44B, 0x647], dtype=np.uint16), 977)
PATTERNS_LOW = (PERIODIC_LOW, RICH_LOW)
PATTERN_HIGH = {4: (0x00A50000, 0x5A000000), 8: (0x00A5_0000_1234_0000, 0x4A00_00F0_0000_0000)}   # per pattern


def wide_pattern(W, pidx):
    x = PATTERNS_LOW[pidx].astype(UNSIGNED[W])
    x[::7] |= UNSIGNED[W](PATTERN_HIGH[W][pidx] & 0x0F0F_0F0F_0F0F_0F0F)
    x[3::11] |= UNSIGNED[W](PATTERN_HIGH[W][pidx] & 0xF0F0_F0F0_F0F0_F0F0)
    assert want_high(x) == PATTERN_HIGH[W][pidx]
    return x.view(SIGNED[W])


@pytest.fixture(scope="module")
def regime_slabs(hip):
    """one slab per width, shared by the module: x[i] = pattern[i % P] for the two patterns, side by side"""
    import torch
    slabs = {}
    for W in WIDTHS:
        n_max = (1004 * 7 + 4) * STEP[W] + 8
        ts = []
        for pidx in range(len(PATTERNS_LOW)):
            p = torch.from_numpy(wide_pattern(W, pidx)).cuda()
            ts.append(p.repeat(-(-n_max // p.numel()))[:n_max].contiguous())
        slabs[W] = ts
    yield slabs
    slabs.clear()
    torch.cuda.empty_cache()


def regime_layouts(W, grid):
    """(phase, n, the push count it is there for): nsteps = c * grid + grid // 2, so that on grids > 1 each launch has workgroups
    with c and with c + 1 pushes; base phases 0 and non-zero; exact and ragged ends"""
    S = STEP[W]
    out = []
    for i, c in enumerate(COUNTS):
        nsteps = c * grid + grid // 2
        for phase in (0, 1 + i % (16 // W - 1)):
            gap = (0, 5, S // 2 - 1)[(i + phase) % 3]
            out.append((phase, nsteps * S - phase - gap, c))
    return out


@functools.lru_cache(maxsize=None)
def regime_want(pidx, n, phase):
    return periodic_counters(PATTERNS_LOW[pidx], [0, n], superset=True, phase=phase)[0]


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("W", WIDTHS)
def test_epoch_regimes(hip, regime_slabs, W, grid):
    layouts = regime_layouts(W, grid)
    starts = k1_starts(True)
    seen, phases = set(), set()
    by_start = {s: set() for s in starts}
    for phase, n, c in layouts:
        s = StepSplit(phase * W, n * W // 2, grid)
        counts = set(s.counts().tolist())
        assert s.grid == grid and c in counts, (W, grid, phase, n, c, counts)
        if grid > 1:
            assert len(counts) == 2, (W, grid, n, counts)
        seen |= counts
        phases.add(phase)
        for st in starts:
            by_start[st] |= {int(k) - (EPOCH - st) for k in counts}
    assert set(COUNTS) <= seen and 0 in phases and len(phases) > 1
    for st in starts:   # every wave: its first flush one push after the last, at the last, one before it; and runs past two epochs
        assert {-1, 0, 1} <= by_start[st] and max(by_start[st]) > EPOCH, (st, sorted(by_start[st]))
    for li, (phase, n, c) in enumerate(layouts):
        for mode in (0, STORE, SUPERSET, STORE | SUPERSET):
            pidx = (li + mode) % len(PATTERNS_LOW)
            t = regime_slabs[W][pidx]
            ptr = t.data_ptr() + W * phase
            assert ptr % 16 == W * phase and phase + n <= t.numel()
            got, h = launch(hip, ptr, n, W, mode, grid)
            want = expect_row(regime_want(pidx, n, phase), mode)
            assert np.array_equal(got, want), (W, grid, phase, n, c, mode, pidx, got, want)
            assert h == expect_mask(PATTERN_HIGH[W][pidx], mode), (W, grid, phase, n, c, mode, hex(h))


def test_launcher_refuses_what_a_wave_cannot_count(hip):
    """a wave's totals are uint32: grid 1 over 2^34 elements is refused before anything is queued (nothing is read: the pointer
    is never dereferenced)"""
    import torch
    out = torch.full((33,), BIAS, dtype=torch.int64, device="cuda")
    for W in WIDTHS:
        assert hip.fsk_launch_wide(out.data_ptr(), 1 << 34, W, out.data_ptr(), out.data_ptr() + 256, STORE, 1, None) != 0
        assert hip.fsk_launch_wide(out.data_ptr(), 8, W, out.data_ptr(), None, 4, 1, None) != 0      # a mode bit that is none
        assert hip.fsk_launch_wide(out.data_ptr(), 8, W, out.data_ptr(), None, 0, 0, None) != 0      # no workgroups
    assert hip.fsk_launch_wide(out.data_ptr(), 8, 2, out.data_ptr(), None, 0, 1, None) != 0
    torch.cuda.synchronize()
    assert (out == BIAS).all()


# ------------------------------------------------------------------ 5. public forms agree
@pytest.mark.parametrize("W", WIDTHS)
def test_public_forms_agree(hip, oracle_mod, W):
    """the device form on a non-default torch stream, the _sync form and the host form -- from pageable and from page-locked
    memory, in chunks of 16 KiB, five of them and a ragged tail, high bits in the first, a middle and the last chunk"""
    import torch
    from libflagstats_amd import _lib
    chunk = 8192 * 2 // W
    n = 5 * chunk + chunk // 3 + 1
    rng = np.random.RandomState(55 + W)
    v = rng.randint(0, 65536, n).astype(SIGNED[W])
    v[3] |= 1 << 17
    v[2 * chunk + 5] |= 1 << 29
    v[n - 1] |= SIGNED[W](-(1 << (8 * W - 1)))        # a negative element, in the ragged tail
    hexp = (1 << 17) | (1 << 29) | (1 << (8 * W - 1))
    assert want_high(v) == hexp
    wants = {sup: want_counters(oracle_mod, v, superset=bool(sup)) for sup in (0, SUPERSET)}
    t = to_device(v)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for sup in (0, SUPERSET):
        for store in (0, STORE):
            flags = sup | store
            out = torch.full((32,), GARBAGE if store else BIAS, dtype=torch.int64, device="cuda")
            high = torch.full((1,), GARBAGE if store else 1 << 40, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            rc = hip.FLAGSTATS_hip_device_wide(t.data_ptr(), n, W, out.data_ptr(), high.data_ptr(), flags, ctypes.c_void_p(side.cuda_stream))
            assert rc == 0, err(hip)
            side.synchronize()
            assert np.array_equal(u64(out), expect_row(wants[SUPERSET], flags)), ("device", W, flags)
            assert int(u64(high)[0]) == expect_mask(hexp, flags)
            o = np.full(32, GARBAGE if store else BIAS, dtype=np.uint64)
            h = ctypes.c_uint64(GARBAGE if store else 1 << 40)
            assert hip.FLAGSTATS_hip_device_wide_sync(t.data_ptr(), n, W, o.ctypes.data, ctypes.byref(h), flags) == 0, err(hip)
            assert np.array_equal(o, expect_row(wants[SUPERSET], flags)) and h.value == expect_mask(hexp, flags), ("sync", W, flags)
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    pinned = hip.FLAGSTATS_hip_host_alloc(v.nbytes)
    assert pinned
    try:
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", 8192), "chunk_flags")
        ctypes.memmove(pinned, v.ctypes.data, v.nbytes)
        for src, where in ((v.ctypes.data, "pageable"), (pinned, "page-locked")):
            for flags in (0, STORE, SUPERSET, STORE | SUPERSET):
                store = flags & STORE
                o = np.full(32, GARBAGE if store else BIAS, dtype=np.uint64)
                h = ctypes.c_uint64(GARBAGE if store else 1 << 40)
                assert hip.FLAGSTATS_hip_wide_x64(src, n, W, o.ctypes.data, ctypes.byref(h), flags) == 0, err(hip)
                assert np.array_equal(o, expect_row(wants[SUPERSET], flags)), ("host", where, W, flags)
                assert h.value == expect_mask(hexp, flags), ("host", where, W, flags, hex(h.value))
        # one chunk only (a single staging slot), and n == 0
        o = np.zeros(32, dtype=np.uint64)
        h = ctypes.c_uint64(0)
        assert hip.FLAGSTATS_hip_wide_x64(v.ctypes.data, 100, W, o.ctypes.data, ctypes.byref(h), STORE) == 0, err(hip)
        assert np.array_equal(o, want_counters(oracle_mod, v[:100])) and h.value == 1 << 17
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
        hip.FLAGSTATS_hip_host_free(pinned)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old
    # n == 0: += touches nothing, store writes zeros
    for entry, args in ((hip.FLAGSTATS_hip_wide_x64, ()), (hip.FLAGSTATS_hip_device_wide_sync, ())):
        o = np.full(32, BIAS, dtype=np.uint64)
        h = ctypes.c_uint64(5)
        assert entry(None, 0, W, o.ctypes.data, ctypes.byref(h), 0) == 0 and (o == BIAS).all() and h.value == 5
        assert entry(None, 0, W, o.ctypes.data, ctypes.byref(h), STORE) == 0 and not o.any() and h.value == 0


# ------------------------------------------------------------------ 6. Python
@pytest.mark.parametrize("dtype", ["int16", "uint16", "int32", "uint32", "int64", "uint64"])
def test_python_numpy_layer(hip, oracle_mod, dtype):
    from libflagstats_amd import pyflagstats, wide
    rng = np.random.RandomState(77)
    n = 300_007
    x16 = rng.randint(0, 65536, n).astype(np.uint16)
    W = np.dtype(dtype).itemsize
    v = x16.view(np.int16) if dtype == "int16" else x16.astype(dtype)
    want = want_counters(oracle_mod, x16)
    got, high = wide.counters_ints(v)
    assert np.array_equal(got, want) and high == 0 and got.dtype == np.uint64
    got, high = wide.counters_ints(v, superset=True)
    assert np.array_equal(got, want_counters(oracle_mod, x16, superset=True)) and high == 0
    d = wide.flagstats_ints(v)
    ref = pyflagstats.flagstats_x64(x16)
    assert d["n_values"] == n and d["passed"] == ref["passed"] and d["failed"] == ref["failed"] and "high_bits" not in d
    assert wide.flagstats_ints(v, strict=False)["high_bits"] == 0
    # a non-contiguous view
    got, high = wide.counters_ints(v[::3])
    assert np.array_equal(got, want_counters(oracle_mod, x16[::3])) and high == 0
    # empty
    got, high = wide.counters_ints(v[:0])
    assert not got.any() and high == 0
    if W == 2:
        return
    bad = v.copy()
    bad[n // 2] = np.dtype(dtype).type(int(x16[n // 2]) + 65536)
    bad[5] = np.dtype(dtype).type(int(x16[5]) | (1 << 20))
    hexp = (1 << 16) | (1 << 20)
    if np.dtype(dtype).kind == "i":
        bad[n - 1] = -1 - int(x16[n - 1] ^ 0xFFFF)          # the same low 16 bits, every bit above them set
        hexp = ALL_HIGH[W]
    assert want_high(bad) == hexp and np.array_equal(low16(bad), x16)
    with pytest.raises(ValueError, match=r"^values outside 0\.\.65535: bits 0x%X set above bit 15$" % hexp):
        wide.flagstats_ints(bad)
    d = wide.flagstats_ints(bad, strict=False)
    assert d["high_bits"] == hexp and d["passed"] == ref["passed"] and d["failed"] == ref["failed"]
    got, high = wide.counters_ints(bad[::-1])               # negative stride
    assert np.array_equal(got, want) and high == hexp


def test_python_torch_layer(hip, oracle_mod):
    import torch
    from libflagstats_amd import wide
    rng = np.random.RandomState(79)
    n = 200_003
    x16 = rng.randint(0, 65536, n).astype(np.uint16)
    want = want_counters(oracle_mod, x16)
    want_sup = want_counters(oracle_mod, x16, superset=True)
    for dt, W in ((torch.int16, 2), (torch.int32, 4), (torch.int64, 8)):
        t = torch.from_numpy(x16.view(np.int16).copy()).cuda() if W == 2 else torch.from_numpy(x16.astype(SIGNED[W])).cuda()
        assert t.dtype == dt
        hexp = 0
        if W != 2:
            t[7] |= 1 << 18
            hexp = 1 << 18
        out, high = wide.count_torch_ints(t)                                       # fresh tensors
        assert out.dtype == torch.int64 and tuple(out.shape) == (32,) and tuple(high.shape) == (1,) and out.device == t.device
        o2, h2 = wide.count_torch_ints(t, out=out, high=high)                      # a second call adds into them
        assert o2 is out and h2 is high
        torch.cuda.synchronize()
        assert np.array_equal(u64(out), 2 * want) and int(u64(high)[0]) == hexp, W
        out.fill_(GARBAGE)
        high.fill_(1 << 41)
        wide.count_torch_ints(t, out=out, high=high, store=True)
        torch.cuda.synchronize()
        assert np.array_equal(u64(out), want) and int(u64(high)[0]) == hexp, W
        high.fill_(1 << 41)
        wide.count_torch_ints(t, out=out, high=high, superset=True)
        torch.cuda.synchronize()
        assert np.array_equal(u64(out), want + want_sup), W
        assert int(u64(high)[0]) == (1 << 41) | hexp, W                           # 2-byte tensors leave high as it is
        wide.count_torch_ints(t, out=out, high=high, store=True, superset=True)
        torch.cuda.synchronize()
        assert np.array_equal(u64(out), want_sup) and int(u64(high)[0]) == hexp, W
        out.fill_(BIAS)
        wide.count_torch_ints(t[:0], out=out, high=high)
        torch.cuda.synchronize()
        assert (out == BIAS).all() and int(u64(high)[0]) == hexp
        wide.count_torch_ints(t[:0], out=out, high=high, store=True)
        torch.cuda.synchronize()
        assert not out.any() and not high.any()
        # on a side stream: ordered behind what that stream holds, nothing else synchronised
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            o3, h3 = wide.count_torch_ints(t, store=True)
        side.synchronize()
        assert np.array_equal(u64(o3), want) and int(u64(h3)[0]) == hexp


def test_python_torch_refusals_that_need_a_device(hip):
    """out / high that do not live on t's device, and a CUDA tensor of the wrong shape: ValueError, nothing launched"""
    import torch
    from libflagstats_amd import wide
    t = torch.zeros(64, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match=r"out must live on t's device \(cuda:0\), not on cpu"):
        wide.count_torch_ints(t, out=torch.zeros(32, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"high must live on t's device \(cuda:0\), not on cpu"):
        wide.count_torch_ints(t, high=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
        wide.count_torch_ints(t[::2])
    with pytest.raises(ValueError, match=r"t must have an integer dtype"):
        wide.count_torch_ints(t.float())


# ------------------------------------------------------------------ 7. refusals on the device
def test_device_refusals(hip):
    import torch
    n = 4096
    bufs = {W: torch.zeros(n + 8, dtype=tdtype(W), device="cuda") for W in WIDTHS}
    out = torch.full((32,), BIAS, dtype=torch.int64, device="cuda")
    high = torch.full((1,), 1 << 40, dtype=torch.int64, device="cuda")
    h_out = np.full(32, BIAS, dtype=np.uint64)
    h_high = ctypes.c_uint64(1 << 40)
    host = np.zeros(n + 8, dtype=np.int64)

    def refused(what, d_array, n_, eb, flags=0, d_out=None, text=None):
        d_out = out.data_ptr() if d_out is None else d_out
        for form in ("device", "sync", "host"):
            if form == "device":
                rc = hip.FLAGSTATS_hip_device_wide(d_array, n_, eb, d_out, high.data_ptr(), flags, None)
            elif form == "sync":
                rc = hip.FLAGSTATS_hip_device_wide_sync(d_array, n_, eb, h_out.ctypes.data, ctypes.byref(h_high), flags)
            else:
                src = host.ctypes.data + (d_array - bufs[8].data_ptr()) % 8 if d_array else None
                rc = hip.FLAGSTATS_hip_wide_x64(src, n_, eb, h_out.ctypes.data, ctypes.byref(h_high), flags)
            assert rc != 0, (what, form)
            assert text in err(hip), (what, form, err(hip))
        untouched(what)

    def untouched(what):
        torch.cuda.synchronize()
        assert (out == BIAS).all() and int(u64(high)[0]) == 1 << 40, what
        assert (h_out == BIAS).all() and h_high.value == 1 << 40, what

    p8 = bufs[8].data_ptr()
    refused("elem_bytes 2", p8, n, 2, text="u16 entries")
    refused("elem_bytes 3", p8, n, 3, text="elem_bytes must be 4 or 8")
    refused("elem_bytes 16", p8, n, 16, text="elem_bytes must be 4 or 8")
    refused("off by 2 at W = 4", p8 + 2, n, 4, text="4-byte aligned")
    refused("off by 4 at W = 8", p8 + 4, n, 8, text="8-byte aligned")
    refused("an extra flag bit", p8, n, 8, flags=4, text="no other bits")
    refused("NULL array", None, n, 4, text="NULL array with n > 0")
    # device form only: a host pointer as d_out (pageable, then page-locked), a host pointer as d_high
    for W in WIDTHS:
        rc = hip.FLAGSTATS_hip_device_wide(bufs[W].data_ptr(), n, W, h_out.ctypes.data, high.data_ptr(), 0, None)
        assert rc != 0 and "d_out" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide(bufs[W].data_ptr(), n, W, out.data_ptr(), ctypes.addressof(h_high), 0, None)
        assert rc != 0 and "d_high" in err(hip), err(hip)
    pinned = hip.FLAGSTATS_hip_host_alloc(512)
    assert pinned
    try:
        ctypes.memset(pinned, 0, 512)
        rc = hip.FLAGSTATS_hip_device_wide(p8, n, 8, pinned, high.data_ptr(), STORE, None)
        assert rc != 0 and "d_out must be device memory" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_wide(p8, n, 8, out.data_ptr(), pinned, STORE, None)
        assert rc != 0 and "d_high must be device memory" in err(hip), err(hip)
        assert not any(ctypes.string_at(pinned, 512))
    finally:
        hip.FLAGSTATS_hip_host_free(pinned)
    untouched("host pointers")
    # Extents.  First a d_out 8 bytes short of its 256, in the += form over an all-zero array: were the check ever skipped, that
    # launch would add nothing anywhere.  Then an array extent one element short of its allocation; the allocation itself is fine.
    nbytes = 2 << 20
    raw = hip.FLAGSTATS_hip_device_alloc(nbytes)
    assert raw
    try:
        rc = hip.FLAGSTATS_hip_device_wide(p8, n, 8, raw + nbytes - 248, high.data_ptr(), 0, None)
        assert rc != 0 and "d_out" in err(hip) and "8 bytes short" in err(hip), err(hip)
        for W in WIDTHS:
            zeros = np.zeros(nbytes, dtype=np.uint8)
            assert hip.FLAGSTATS_hip_memcpy_h2d(raw, zeros.ctypes.data, nbytes) == 0
            rc = hip.FLAGSTATS_hip_device_wide(raw, nbytes // W + 1, W, out.data_ptr(), high.data_ptr(), STORE, None)
            assert rc != 0 and "d_array" in err(hip) and "%d bytes short" % W in err(hip), err(hip)
            rc = hip.FLAGSTATS_hip_device_wide_sync(raw + W, nbytes // W, W, h_out.ctypes.data, ctypes.byref(h_high), STORE)
            assert rc != 0 and "d_array" in err(hip) and "%d bytes short" % W in err(hip), err(hip)
            untouched("extent")
            o = np.full(32, BIAS, dtype=np.uint64)
            assert hip.FLAGSTATS_hip_device_wide_sync(raw, nbytes // W, W, o.ctypes.data, None, STORE) == 0, err(hip)
            assert not o.any()
    finally:
        hip.FLAGSTATS_hip_device_free(raw)
    untouched("extents")
