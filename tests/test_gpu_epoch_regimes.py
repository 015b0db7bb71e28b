"""The positional popcount and K1 on the MI355X across their epoch flushes: direct launches of fsk_launch_pospopcnt and fsk_launch
on grids of 1-7 workgroups, so that each workgroup pushes hundreds of steps, with its last push placed one before, at and one
after a flush (every 255 pushes; K1's waves start their count at 64 * w under the epoch stagger).

Every layout is checked with steps_oracle.StepSplit (the launchers' step geometry, mirrored) to really put a workgroup where it
is there to test.  Inputs are periodic (x[i] = pattern[i % P]), so every expected result comes in O(P) from
steps_oracle.periodic_pospopcnt or segments_oracle.periodic_counters, at any size.  A wave counts at most 2^32 words
(flagstat_pospopcnt.hip); the 16 GiB run stays below that."""
import contextlib
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from segments_oracle import periodic_counters  # noqa: E402
from steps_oracle import EPOCH, STEP_WORDS, StepSplit, k1_starts, periodic_pospopcnt  # noqa: E402

pytestmark = pytest.mark.gpu

S = STEP_WORDS
GARBAGE, BIAS = 0x5EED_0000_0BAD, 3
GRIDS = (1, 2, 3, 7)
SCHEDULES = (9, 25, 71)

ONES = np.array([0xFFFF], dtype=np.uint16)
# period 65,521 (prime, so coprime with the 16,384 words of a step)
PERIODIC = np.random.RandomState(303).randint(0, 65536, 65_521).astype(np.uint16)
# about one set bit in 61 words: 16 single-bit words, one per bit position, in a prime period of 977
SPARSE = np.zeros(977, dtype=np.uint16)
SPARSE[np.random.RandomState(305).choice(977, 16, replace=False)] = 1 << np.arange(16, dtype=np.uint16)
# the segments regime patterns: every slot lit in turn, and dense (several counters count every flag)
RICH = np.array([0x443, 0x4C3, 0x643, 0x483, 0xC43, 0x543, 0x44B, 0x647], dtype=np.uint16)
CONSTANTISH = np.array([0x443, 0x4C3, 0x483, 0x463], dtype=np.uint16)
K1_PATTERNS = (CONSTANTISH, RICH, PERIODIC)


def pattern_tensor(pattern, n):
    """int16 CUDA tensor of n words, x[i] = pattern[i % P]"""
    import torch
    reps = -(-n // pattern.size)
    return torch.from_numpy(pattern.view(np.int16)).cuda().repeat(reps)[:n]


# ------------------------------------------------------------------ pospopcnt
@pytest.fixture(scope="module")
def pos(hip):
    f = hip.fsk_launch_pospopcnt
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_int]
    return f


POS_COUNTS = (254, 255, 256, 509, 510, 511, 1003)


def pos_layouts(grid):
    """(shift, n, the per-workgroup push count it is there for): every count exactly and ragged, at base shifts 0-7; on grids
    > 1, nsteps % grid != 0, so that one launch has workgroups on both sides of the count"""
    out = []
    for ci, c in enumerate(POS_COUNTS):
        nsteps = c * grid + grid // 2
        for shift, gap in ((0, 0), (1 + ci % 7, 0), (0, 9), (1 + (ci + 3) % 7, 5)):
            out.append((shift, nsteps * S - shift - gap, c))
    return out


@pytest.fixture(scope="module")
def pos_buffers(hip):
    n_max = (POS_COUNTS[-1] * 7 + 3) * S
    bufs = {name: (pat, PosSlab(pat, n_max)) for name, pat in (("ones", ONES), ("periodic", PERIODIC), ("sparse", SPARSE))}
    yield bufs
    bufs.clear()


class PosSlab:
    """x[0:n) = pattern[i % P], placed at any base shift with 0xFFFF around it: a read before or past the launched range adds
    to every count"""

    def __init__(self, pattern, n_max):
        import torch
        self.n_max = n_max
        self.body = pattern_tensor(pattern, n_max)
        self.t = torch.full((n_max + 48,), -1, dtype=torch.int16, device="cuda")

    @contextlib.contextmanager
    def placed(self, shift, n):
        """x[0:n) at word 8 + shift, 0xFFFF in the 8 + shift words before it and the 16 words after it"""
        import torch
        assert 0 <= shift < 8 and 0 < n <= self.n_max
        t = self.t
        t[:8 + shift] = -1
        t[8 + shift:8 + shift + n] = self.body[:n]
        t[8 + shift + n:8 + shift + n + 16] = -1
        torch.cuda.synchronize()
        yield t.data_ptr() + 2 * (8 + shift)


def pos_run(pos, ptr, n, grid, direct, grid_req=None):
    import torch
    g = grid_req or grid
    out = torch.full((16,), BIAS, dtype=torch.int64, device="cuda")
    parts = torch.full((16 * g,), GARBAGE, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert pos(ptr, n, g, parts.data_ptr(), out.data_ptr(), None, direct) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64) - np.uint64(BIAS)


@pytest.mark.parametrize("grid", GRIDS)
def test_pospopcnt_epoch_seams(pos, pos_buffers, grid):
    layouts = pos_layouts(grid)
    seen, ragged, shifted = set(), False, set()
    for shift, n, c in layouts:
        s = StepSplit(2 * shift, n, grid)
        assert s.grid == grid and c in set(s.counts().tolist()), (grid, shift, n, c, s.counts())
        if grid > 1:
            assert s.nsteps % grid != 0 and len(set(s.counts().tolist())) == 2, (grid, n)
        seen.update(s.counts().tolist())
        ragged |= s.head_edge and s.tail_edge
        shifted.add(shift)
    assert set(POS_COUNTS) <= seen and ragged and shifted == set(range(8)), (seen, shifted)
    for name, (pat, slab) in pos_buffers.items():
        for shift, n, c in layouts:
            want = periodic_pospopcnt(pat, 0, n)
            with slab.placed(shift, n) as ptr:
                for direct in (1, 0):
                    got = pos_run(pos, ptr, n, grid, direct)
                    assert np.array_equal(got, want), (name, grid, shift, n, c, direct, got, want)


def test_pospopcnt_two_step_edges(pos, pos_buffers):
    """lo != 0 and nsteps = 2: the tail edge step is step fast_begin itself; requested grids above nsteps are clamped (the
    partials are sized for the requested grid)"""
    for name, (pat, slab) in pos_buffers.items():
        for shift, n in ((3, S + 100), (7, 2 * S - 8), (1, S), (5, S - 4)):
            s = StepSplit(2 * shift, n, 7)
            assert s.nsteps == 2 and s.fast_begin == 1 and s.fast_end == 1 and s.tail_block is not None
            assert s.pushes(0) == [0] and s.pushes(1) == [1] and s.grid == 2
            want = periodic_pospopcnt(pat, 0, n)
            with slab.placed(shift, n) as ptr:
                for grid in (1, 2, 7):
                    for direct in (1, 0):
                        got = pos_run(pos, ptr, n, grid, direct, grid_req=grid)
                        assert np.array_equal(got, want), (name, shift, n, grid, direct, got, want)


def test_pospopcnt_lane_counters_past_2_16(pos, pos_buffers):
    """grid 1, 1,025+ steps of all-ones: each lane's 16 counters pass 2^16"""
    pat, slab = pos_buffers["ones"]
    for shift, n in ((0, 1025 * S), (3, 1030 * S - 3 - 11)):
        s = StepSplit(2 * shift, n, 1)
        assert s.counts()[0] >= 1025 and s.counts()[0] * 64 > 1 << 16
        with slab.placed(shift, n) as ptr:
            for direct in (1, 0):
                got = pos_run(pos, ptr, n, 1, direct)
                assert (got == n).all(), (shift, n, direct, got)


def test_pospopcnt_wave_totals_past_2_31(pos):
    """grid 1 on 2^33 + 2^20 all-ones words (16 GiB): each wave's per-bit total passes 2^31, the workgroup's 2^33"""
    import torch
    n = (1 << 33) + (1 << 20)
    t = torch.full((n,), -1, dtype=torch.int16, device="cuda")
    s = StepSplit(0, n, 1)
    assert s.grid == 1 and n // 4 > 1 << 31 and n // 4 < 1 << 32   # per wave: below the kernel's limit of 2^32 words
    for direct in (1, 0):
        got = pos_run(pos, t.data_ptr(), n, 1, direct)
        assert (got == n).all(), (direct, got)
    del t
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ K1
@pytest.fixture(scope="module")
def k1(hip):
    f = hip.fsk_launch
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    hip.fsk_partials_bytes.restype = ctypes.c_size_t
    hip.fsk_partials_bytes.argtypes = [ctypes.c_uint32]
    hip.fsk_last_mode.restype = ctypes.c_int
    return f


@contextlib.contextmanager
def stagger(hip, on):
    from libflagstats_amd import _lib
    old = hip.FLAGSTATS_hip_get(b"epoch_stagger")
    try:
        _lib.check(hip.FLAGSTATS_hip_set(b"epoch_stagger", on), "set epoch_stagger")
        assert hip.FLAGSTATS_hip_get(b"epoch_stagger") == on
        yield
    finally:
        hip.FLAGSTATS_hip_set(b"epoch_stagger", old)
    assert hip.FLAGSTATS_hip_get(b"epoch_stagger") == old


# form name -> (variant bits, store, superset, the K1 mode bits the launch must run with)
K1_FORMS = {
    "direct": (2048, False, False, 4),
    "k2_acc": (0, False, False, 0),
    "k2_store": (256, True, False, 1),
    "superset_acc": (1024, False, True, 2),
    "superset_store": (1280, True, True, 3),
    "superset_direct": (3072, False, True, 6),
}


def k1_expect(want_sup, store, superset):
    w = want_sup.copy()
    if not superset:
        w[[0, 9, 16]] = 0
    return w if store else w + np.uint64(BIAS)


def k1_run(hip, k1, ptr, n, grid, variant, store):
    import torch
    nbytes = hip.fsk_partials_bytes(grid)
    ws = torch.zeros((nbytes // 8,), dtype=torch.int64, device="cuda")   # partials[21][grid], then the ticket block
    out = torch.full((32,), GARBAGE if store else BIAS, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ticket = ws.data_ptr() + 8 * 21 * grid
    assert k1(ptr, n, grid, variant, ws.data_ptr(), ticket, out.data_ptr(), None, None, 0) == 0
    torch.cuda.synchronize()
    assert not ws[21 * grid:].any(), "the ticket block is left zero"
    return out.cpu().numpy().view(np.uint64)


K1_COUNTS = (62, 63, 64, 126, 127, 128, 190, 191, 192, 254, 255, 256, 601)


def k1_layouts(grid):
    """(shift, n, push counts it is there for): on grid 1 every count; on larger grids nsteps = c * grid + grid // 2, so that
    each launch has workgroups with c and with c + 1 pushes"""
    counts = K1_COUNTS if grid == 1 else (62, 63, 126, 127, 190, 191, 254, 255, 601)
    out = []
    for i, c in enumerate(counts):
        nsteps = c * grid + grid // 2
        shift = i % 8
        gap = (0, 5, 8191)[i % 3]
        out.append((shift, nsteps * S - shift - gap, c))
    return out


@functools.lru_cache(maxsize=None)
def k1_want(pidx, n, phase):
    return periodic_counters(K1_PATTERNS[pidx], [0, n], superset=True, phase=phase)[0]


@pytest.fixture(scope="module")
def k1_buffers(hip):
    n_max = (601 * 7 + 4) * S + 8
    ts = [pattern_tensor(p, n_max) for p in K1_PATTERNS]
    yield ts
    ts.clear()


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_k1_epoch_seams(hip, k1, k1_buffers, schedule, grid):
    for on in (1, 0):
        starts = k1_starts(bool(on))
        layouts = k1_layouts(grid)
        offsets = set()
        for shift, n, c in layouts:
            s = StepSplit(2 * shift, n, grid, plain=schedule == 9)
            assert s.grid == grid and c in set(s.counts().tolist()), (schedule, grid, shift, n, c)
            offsets |= s.seam_offsets(starts)
        # each wave's first flush one before, at and one after the last push, and runs past two epochs
        assert {-1, 0, 1} <= offsets and max(offsets) > EPOCH, offsets
        with stagger(hip, on):
            for li, (shift, n, c) in enumerate(layouts):
                for fi, (form, (bits, store, sup, mode)) in enumerate(K1_FORMS.items()):
                    pidx = (li + fi) % len(K1_PATTERNS)
                    ptr = k1_buffers[pidx].data_ptr() + 2 * shift
                    got = k1_run(hip, k1, ptr, n, grid, schedule | bits, store)
                    assert hip.fsk_last_mode() == mode | (16 if on else 0), (form, hip.fsk_last_mode())
                    want = k1_expect(k1_want(pidx, n, shift), store, sup)
                    assert np.array_equal(got, want), (schedule, on, grid, shift, n, c, form, pidx, got, want)


def test_k1_completion_word_form(hip, k1, k1_buffers):
    """the grid-1 latency form (mode bit 32): K1 stores its own 32 {value, sequence} pairs into page-locked host memory, at
    base shifts 0 and 1-7, plain and superset, across the epoch seams"""
    import torch
    pairs_p = hip.FLAGSTATS_hip_host_alloc(64 * 8)
    assert pairs_p
    pairs = (ctypes.c_uint64 * 64).from_address(pairs_p)
    try:
        seq = 0x1234_5678_9ABC_0000
        for schedule in SCHEDULES:
            for on in (1, 0):
                with stagger(hip, on):
                    for i, (c, shift) in enumerate(((63, 0), (64, 3), (191, 5), (256, 0), (255, 7), (601, 1))):
                        n = c * S - shift - (0, 5, 8191)[i % 3]
                        s = StepSplit(2 * shift, n, 1, plain=schedule == 9)
                        assert s.counts().tolist() == [c]
                        pidx = i % len(K1_PATTERNS)
                        ptr = k1_buffers[pidx].data_ptr() + 2 * shift
                        for sup in (False, True):
                            seq += 1
                            for k in range(64):
                                pairs[k] = GARBAGE
                            ws = torch.zeros((hip.fsk_partials_bytes(1) // 8,), dtype=torch.int64, device="cuda")
                            out = torch.full((32,), GARBAGE, dtype=torch.int64, device="cuda")
                            torch.cuda.synchronize()
                            variant = schedule | 256 | (1024 if sup else 0)
                            assert k1(ptr, n, 1, variant, ws.data_ptr(), ws.data_ptr() + 8 * 21, out.data_ptr(), None,
                                      pairs_p, seq) == 0
                            torch.cuda.synchronize()
                            assert hip.fsk_last_mode() & 32, hip.fsk_last_mode()
                            got = np.array(pairs[:], dtype=np.uint64).reshape(32, 2)
                            want = k1_expect(k1_want(pidx, n, shift), True, sup)
                            what = (schedule, on, c, shift, sup)
                            assert (got[:, 1] == seq).all(), (what, got[:, 1])
                            assert np.array_equal(got[:, 0], want), (what, got[:, 0], want)
                            assert (out.cpu().numpy().view(np.uint64) == GARBAGE).all(), what   # out[] untouched
                            assert not ws.any(), what
    finally:
        hip.FLAGSTATS_hip_host_free(pairs_p)
