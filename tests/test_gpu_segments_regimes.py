"""Segmented flagstat on the MI355X, regime by regime: the carry-save chain (runs of whole 4096-flag units inside one segment, its
epoch flush every 255 units), the per-flag path, the seams between them and between writers, in every output form.

Most launches here call fsk_launch_segments directly with a small grid, so that a few waves own hundreds or thousands of units of
an array of tens of MiB; the rest go through the public entries under every segments policy.  Inputs are periodic
(x[i] = pattern[i % P], P prime), so every expected row comes from segments_oracle.periodic_counters in O(nseg), at any size.
Every layout is checked with segments_oracle.WriterSplit (the launcher's work split, mirrored) to really contain the run it is
there to test.  Direct launches stay below 2^32 flags per wave (the wave totals are uint32; flagstat_segments.h)."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from segments_oracle import SEG_EPOCH, SEG_UNIT, periodic_counters, writer_ranges  # noqa: E402

pytestmark = pytest.mark.gpu

U = SEG_UNIT
P = 65_521                       # prime: no unit, row or writer seam is a multiple of the period
GARBAGE, BIAS = 0x5EED_0000_0BAD, 3
MODES = (1, 0, 3, 2)             # store, +=, store + superset, += + superset
EVERY_MIN_UNITS = (0, 1, 2, 3, 255, 256, 0xFFFFFFFF)


def random_pattern(seed, period=P):
    return np.random.RandomState(seed).randint(0, 65536, period).astype(np.uint16)


# every flag paired + proper + DUP, read1 / read2 / QC-fail / supplementary / secondary / unmapped in turn: lights every slot
RICH = np.array([0x443, 0x4C3, 0x643, 0x483, 0xC43, 0x543, 0x44B, 0x647], dtype=np.uint16)
# no QC fail: several counters (proper pair, read1, DUP, primary paired) count every flag, so bit-columns fill up
CONSTANTISH = np.array([0x443, 0x4C3, 0x483, 0x463], dtype=np.uint16)


def expect(want_sup, mode):
    """the rows a launch in `mode` must leave in an out[] prefilled with GARBAGE (store) or BIAS (+=)"""
    w = want_sup.copy()
    if not mode & 2:
        w[:, [0, 9, 16]] = 0
    return w if mode & 1 else w + np.uint64(BIAS)


@pytest.fixture(scope="module")
def launcher(hip):
    f = hip.fsk_launch_segments
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                  ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p]
    hip.fsk_segments_policy.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    hip.fsk_segments_policy.restype = None
    hip.fsk_set_segments_policy.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    hip.fsk_set_segments_policy.restype = None
    return f


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


def periodic_tensor(pattern, n, slack=16):
    """int16 CUDA tensor of n + slack flags, x[i] = pattern[i % len(pattern)], filled on the device"""
    import torch
    reps = -(-(n + slack) // pattern.size)
    t = torch.from_numpy(pattern.view(np.int16)).cuda().repeat(reps)
    torch.cuda.synchronize()
    return t


def direct(launcher, ptr, base, m, offsets, mode, grid):
    """one fsk_launch_segments on the null stream into a prefilled out[]; returns the rows"""
    import torch
    o = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).cuda()
    nseg = o.numel() - 1
    out = torch.full((nseg, 32), GARBAGE if mode & 1 else BIAS, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert launcher(ptr, base, m, o.data_ptr(), nseg, out.data_ptr(), mode, grid, None) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


def check_all_modes(launcher, ptr, base, m, offsets, grid, want_sup, what):
    for mode in MODES:
        got = direct(launcher, ptr, base, m, offsets, mode, grid)
        want = expect(want_sup, mode)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (what, "mode", mode, "rows", bad[:8], got[bad[:2]], want[bad[:2]])


# ------------------------------------------------------------------ layouts (array indices of the launched chunk)
LENGTH_UNITS = (254, 255, 256, 509, 510, 511)
DELTAS = (0, 1, -1, 8, -8)


def lengths_layout(w, n):
    """segments of 254..511 and 1000+ whole units, then the same lengths +1 / -1 / +8 / -8 flags, laid end to end from the first
    writer seam (the flags before it are one more segment): exact unit counts first, then ragged heads and tails"""
    seams = w.seams()
    start = int(seams[0]) if seams.size else 3
    lengths = [L * U + d for d in DELTAS for L in LENGTH_UNITS] + [1000 * U, 1003 * U + 1, 1021 * U - 8, 1000 * U - 1]
    o = [0, start]
    for L in lengths:
        if o[-1] + L > n:
            break
        o.append(o[-1] + L)
    return np.array(o + ([n] if o[-1] < n else []), dtype=np.int64)


def seams_layout(w, n):
    """a boundary at every writer seam -1 / 0 / +1 in turn, and inside every writer a 1..9-flag segment after 257 whole units
    (unit boundary +0 / +1 / -1 / +8), so each writer changes chain -> per-flag -> chain"""
    cuts = []
    for k, (b, e) in enumerate(zip(w.begin, w.end)):
        if e <= b:
            continue
        if b > 0:
            cuts.append(int(b) + (-1, 0, 1)[k % 3])
        g = int(-(-(b + w.lo0) // U) * U - w.lo0) + 257 * U + (0, 1, -1, 8)[k % 4]
        if g + 10 + 3 * U < e:
            cuts += [g, g + 1 + k % 9]
    cuts = np.unique(np.clip(cuts, 0, n))
    return np.concatenate([[0], cuts[(cuts > 0) & (cuts < n)], [n]]).astype(np.int64)


def dense_long_layout(w, n, seed):
    """random short segments (0..3000 flags) across the first seam, then 600 whole units, dense again, then the rest"""
    rng = np.random.RandomState(seed)
    seams = w.seams()
    mid = int(seams[0]) if seams.size else n // 2
    o = [max(mid - 200_000, 0)]
    while o[-1] < mid + 150_000:
        o.append(o[-1] + int(rng.randint(0, 3001)))
    o.append(o[-1] + 600 * U + 5)
    while o[-1] < o[1] + 600 * U + 500_000:
        o.append(o[-1] + int(rng.randint(0, 3001)))
    o = np.array([0] + o + [n], dtype=np.int64)
    return np.unique(np.clip(o, 0, n))


def reach(w, offsets, min_units=2):
    """what the mirror says a launch over these offsets runs through"""
    p = w.pieces(offsets, min_units)
    chain = p["chain"]
    return {
        "max_chain": int(chain.max()) if chain.size else 0,
        "chains": set(int(c) for c in chain[chain > 0]),
        "epoch_atomic": bool(((chain > SEG_EPOCH) & ~p["plain"]).any()),
        "epoch_plain": bool(((chain > SEG_EPOCH) & p["plain"]).any()),
        "ragged_both": bool(((chain > 0) & (p["head"] > 0) & (p["tail"] > 0)).any()),
        "per_flag": bool(((chain == 0) | (p["head"] > 0) | (p["tail"] > 0)).any()),
        # a writer that goes chain -> per-flag piece -> chain over consecutive segments
        "switch": any(((p["writer"][i] == p["writer"][i + 1] == p["writer"][i + 2]) and chain[i] > 0 and chain[i + 1] == 0
                       and chain[i + 2] > 0) for i in range(chain.size - 2)),
    }


N_DIRECT = (1 << 26) - 12_345    # ~128 MiB: at grid 1 each wave owns ~4,100 units, at grid 7 ~585


@pytest.fixture(scope="module")
def periodic_array(hip):
    pat = random_pattern(101)
    t = periodic_tensor(pat, N_DIRECT)
    yield pat, t
    del t


@pytest.mark.parametrize("grid", [1, 2, 3, 7])
def test_direct_chain_lengths_and_seams(launcher, periodic_array, grid):
    pat, t = periodic_array
    n = N_DIRECT
    w = writer_ranges(t.data_ptr() % 16, n, grid)
    assert w.waves == 4 * grid
    layouts = {"lengths": lengths_layout(w, n), "seams": seams_layout(w, n), "dense_long": dense_long_layout(w, n, grid)}
    r = {name: reach(w, o) for name, o in layouts.items()}
    # the runs each layout is there for
    assert r["lengths"]["epoch_plain"], r["lengths"]
    assert r["lengths"]["max_chain"] > SEG_EPOCH and r["lengths"]["ragged_both"], r["lengths"]
    assert r["seams"]["epoch_atomic"] and r["seams"]["switch"], r["seams"]
    assert r["dense_long"]["per_flag"] and r["dense_long"]["max_chain"] > SEG_EPOCH, r["dense_long"]
    if grid == 1:
        assert {254, 255, 256, 509, 510, 511}.issubset(r["lengths"]["chains"]) and r["lengths"]["max_chain"] >= 1000
    for name, o in layouts.items():
        check_all_modes(launcher, t.data_ptr(), 0, n, o, grid, periodic_counters(pat, o, superset=True), (grid, name))


def test_direct_min_units_edges(hip, launcher, periodic_array):
    """min_units = 255 / 256 around the epoch and 0xFFFFFFFF (per-flag everywhere) on the same launches"""
    pat, t = periodic_array
    n = N_DIRECT
    w = writer_ranges(t.data_ptr() % 16, n, 1)
    o = lengths_layout(w, n)
    want = periodic_counters(pat, o, superset=True)
    for mu in (0, 1, 255, 256, 0xFFFFFFFF):
        r = reach(w, o, mu)
        assert (r["max_chain"] == 0) == (mu == 0xFFFFFFFF) and (mu not in (255, 256) or mu in r["chains"]), (mu, r)
        with policy(hip, mu):
            check_all_modes(launcher, t.data_ptr(), 0, n, o, 1, want, ("min_units", mu))


def test_direct_base_pointer_shifts(launcher, periodic_array):
    pat, t = periodic_array
    n = N_DIRECT - 8
    for shift in range(8):
        ptr = t.data_ptr() + 2 * shift
        w = writer_ranges(ptr % 16, n, 3)
        for name, o in (("lengths", lengths_layout(w, n)), ("seams", seams_layout(w, n))):
            r = reach(w, o)
            assert r["max_chain"] > SEG_EPOCH and r["per_flag"], (shift, name, r)
            want = periodic_counters(pat, o, superset=True, phase=shift)
            check_all_modes(launcher, ptr, 0, n, o, 3, want, ("shift", shift, name))


@pytest.mark.parametrize("grid", [1, 2])
def test_direct_chunk_launches(launcher, periodic_array, grid):
    """base != 0: one chunk of the array launched alone, with global offsets before, inside and after it (clamped to the
    chunk), and consecutive chunks of the host form's shape (+=) summing to the whole rows"""
    pat, t = periodic_array
    n = N_DIRECT
    o = lengths_layout(writer_ranges(t.data_ptr() % 16, n, grid), n)
    want_all = periodic_counters(pat, o, superset=True)
    for c0, m in ((1000 * U + 5, 5000 * U + 3), (3 * U - 1, 700 * U + 9), (int(o[3]) - 1, int(o[8] - o[3]) + 2)):
        ptr = t.data_ptr() + 2 * c0
        w = writer_ranges(ptr % 16, m, grid)
        clipped = np.clip(o, c0, c0 + m)
        r = reach(w, clipped - c0)
        assert r["max_chain"] > (SEG_EPOCH if m > 5000 * U else 80) and r["per_flag"], (c0, m, r)
        assert (o < c0).any() and (o > c0 + m).any()
        check_all_modes(launcher, ptr, c0, m, o, grid, periodic_counters(pat, clipped, superset=True), ("chunk", c0, m))
    # offsets entirely before / after the chunk: every row empty
    c0, m = 2 * U + 3, 100 * U
    for outside in (np.array([0, 1, c0]), np.array([c0 + m, c0 + m + 5, n])):
        got = direct(launcher, t.data_ptr() + 2 * c0, c0, m, outside, 3, grid)
        assert not got.any(), outside
    # the host form's loop: chunks of 9,000,001 flags, every launch adding into the same rows
    import torch
    d_off = torch.from_numpy(o).cuda()
    nseg = o.size - 1
    for mode in (0, 2):
        out = torch.zeros((nseg, 32), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for pos in range(int(o[0]), int(o[-1]), 9_000_001):
            c = min(9_000_001, int(o[-1]) - pos)
            assert launcher(t.data_ptr() + 2 * pos, pos, c, d_off.data_ptr(), nseg, out.data_ptr(), mode, grid, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), expect(want_all, mode | 1)), ("chunked", mode)


# ------------------------------------------------------------------ counter widths
@pytest.mark.parametrize("name, pattern", [("rich", RICH), ("constantish", CONSTANTISH)])
def test_per_lane_counters_past_2_16(hip, launcher, name, pattern):
    """one long segment over 2^25 flags at grid 1: per-flag everywhere (each lane's counters pass 2^17), then the chain"""
    n = (1 << 25) + 3 * U + 5
    t = periodic_tensor(pattern, n)
    o = np.array([0, 2, n - 3, n], dtype=np.int64)
    w = writer_ranges(t.data_ptr() % 16, n, 1)
    p = w.pieces(o, 0xFFFFFFFF)
    long_pieces = (p["e"] - p["b"])[p["seg"] == 1]
    assert long_pieces.size == 4 and long_pieces.min() >= 1 << 23 and (p["chain"] == 0).all()   # >= 2^17 flags per lane
    assert reach(w, o)["max_chain"] >= 2048
    want = periodic_counters(pattern, o, superset=True)
    for mu in (0xFFFFFFFF, 2):
        with policy(hip, mu):
            check_all_modes(launcher, t.data_ptr(), 0, n, o, 1, want, (name, mu))
    del t


def test_wave_total_past_2_31(hip, launcher):
    """grid 1 on ~2^33 flags (16 GiB, filled on the device): each of the 4 waves totals > 2^31 flags of one segment, and
    several counters count every one of them"""
    import torch
    n = (1 << 33) + (1 << 21) + 5
    t = periodic_tensor(CONSTANTISH, n)
    o = np.array([0, 3, n - 2, n], dtype=np.int64)
    w = writer_ranges(t.data_ptr() % 16, n, 1)
    p = w.pieces(o)
    main = p["seg"] == 1
    assert main.sum() == 4 and (p["chain"][main] > SEG_EPOCH).all()
    for b, e in zip(p["b"][main], p["e"][main]):
        assert (1 << 31) < e - b < (1 << 32)                      # the direct-launch limit: below 2^32 flags per wave
        assert periodic_counters(CONSTANTISH, [b, e], superset=True)[0].max() > (1 << 31)
    want = periodic_counters(CONSTANTISH, o, superset=True)
    for mode in (3, 0):
        got = direct(launcher, t.data_ptr(), 0, n, o, mode, 1)
        assert np.array_equal(got, expect(want, mode)), ("chain", mode, got[1], expect(want, mode)[1])
    with policy(hip, 0xFFFFFFFF):
        got = direct(launcher, t.data_ptr(), 0, n, o, 3, 1)
        assert np.array_equal(got, expect(want, 3)), ("per-flag", got[1], want[1])
    del t
    torch.cuda.empty_cache()   # 8-16 GiB back to the device for the tests after this one


# ------------------------------------------------------------------ the public entries under every policy
N_POLICY = (1 << 26) + 4099


def test_policy_sweep_public_entries(hip):
    import torch
    from libflagstats_amd import _lib, segments
    pat = random_pattern(202)
    n = N_POLICY
    t = periodic_tensor(pat, n, slack=0)[:n]
    x = np.resize(pat, n)
    rng = np.random.RandomState(17)
    lengths = rng.choice([3, 100, 4095, 4097, 2 * U + 5, 3 * U, 17 * U - 1, 1_000_003, 7_000_001, 20_000_011], 60)
    o = np.concatenate([[13], 13 + np.cumsum(lengths)])
    o = np.append(o[o < n - 7], n - 7).astype(np.int64)
    want = periodic_counters(pat, o, superset=True)
    d_off = torch.from_numpy(o).cuda()
    nseg = o.size - 1
    cus = hip.FLAGSTATS_hip_compute_units()
    old_chunk = hip.FLAGSTATS_hip_get(b"chunk_flags")
    saved = get_policy(hip)
    try:
        for bpc in (1, 2, 8):
            for i, mu in enumerate(EVERY_MIN_UNITS):
                sup = bool((i + bpc) % 2)
                mode = 2 if sup else 0
                # device form (async): where the mirror says the chain runs
                r = reach(writer_ranges(t.data_ptr() % 16, n, cus * bpc), o, mu)
                assert (r["max_chain"] > 0) == (mu <= 3), (bpc, mu, r)   # 255 / 256 need longer arrays at this grid
                hip.fsk_set_segments_policy(mu, bpc)
                assert get_policy(hip) == (mu, bpc)
                for store in (True, False):
                    out = torch.full((nseg, 32), GARBAGE if store else BIAS, dtype=torch.int64, device="cuda")
                    segments.count_segments_torch(t, d_off, out=out, store=store, superset=sup)
                    torch.cuda.synchronize()
                    got = out.cpu().numpy().view(np.uint64)
                    assert np.array_equal(got, expect(want, mode | store)), ("device", bpc, mu, store)
                # _sync form
                assert np.array_equal(segments.count_segments_device_ptr(t.data_ptr(), n, o, superset=sup),
                                      expect(want, mode | 1)), ("sync", bpc, mu)
                # host-array form, chunks that are multiples of neither 8 nor 4096
                for chunk in (9_000_001, 33_554_431):
                    if bpc == 1 and mu == 2:
                        first = np.clip(o, o[0], o[0] + chunk) - o[0]   # the first chunk (staging buffers are 16-B aligned)
                        rc = reach(writer_ranges(0, chunk, cus), first, mu)
                        assert rc["max_chain"] > 0, (chunk, rc)
                    _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", chunk), "chunk_flags")
                    assert np.array_equal(segments.flagstats_segments(x, o, superset=sup), expect(want, mode | 1)), \
                        ("host", bpc, mu, chunk)
    finally:
        hip.fsk_set_segments_policy(*saved)
        hip.FLAGSTATS_hip_set(b"chunk_flags", old_chunk)
    assert get_policy(hip) == saved and hip.FLAGSTATS_hip_get(b"chunk_flags") == old_chunk
    del t
