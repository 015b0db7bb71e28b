"""Segmented flagstat on the MI355X: every form, bit-exact against the segmented numpy oracle (tests/segments_oracle.py) and,
at full size, against oracle.flagstat_generated per segment."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from segments_oracle import segmented_counters  # noqa: E402

pytestmark = pytest.mark.gpu

EDGES = [0, 1, 7, 8, 9, 511, 512, 513, 4095, 4096, 4097, 16383, 16384, 16385]


class Dev:
    """raw device buffer owned by the library"""

    def __init__(self, lib, nbytes):
        self.lib = lib
        self.ptr = lib.FLAGSTATS_hip_device_alloc(max(nbytes, 8))
        assert self.ptr

    def put(self, a, at=0):
        a = np.ascontiguousarray(a)
        assert self.lib.FLAGSTATS_hip_memcpy_h2d(self.ptr + at, a.ctypes.data, a.nbytes) == 0
        return self

    def get(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        assert self.lib.FLAGSTATS_hip_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes) == 0
        return out

    def free(self):
        self.lib.FLAGSTATS_hip_device_free(self.ptr)


def flags_of(kind, n, seed):
    import oracle
    if kind == "uniform":
        return oracle.generate(oracle.GEN_UNIFORM, seed, 0xFFFF, 0, n)   # bits 12-15 set too
    return oracle.generate(oracle.GEN_NA12878, seed, 0, 0, n)


def random_lengths(rng, count):
    """lengths drawn from the vector, row, unit and K1-step edges and a few random ones"""
    return rng.choice(EDGES + list(rng.randint(0, 3000, 16)), count).astype(np.int64)


def device_counts(hip, d_ptr, n, o, flags, garbage=True):
    """async device form into a garbage-filled (store) or zeroed (+=) device buffer, read back."""
    nseg = o.size - 1
    off = Dev(hip, o.nbytes).put(o.astype(np.uint64))
    out = Dev(hip, max(nseg, 1) * 256)
    fill = np.full((max(nseg, 1), 32), 0xDEADBEEF if (garbage and flags & 1) else 0, dtype=np.uint64)
    out.put(fill)
    assert hip.FLAGSTATS_hip_device_u16_segments(d_ptr, n, off.ptr, nseg, out.ptr, flags, None) == 0, hip.FLAGSTATS_hip_last_error()
    assert hip.FLAGSTATS_hip_synchronize() == 0
    got = out.get((max(nseg, 1), 32), np.uint64)[:nseg]
    off.free()
    out.free()
    return got


@pytest.mark.parametrize("kind", ["uniform", "na12878"])
def test_layouts_all_forms(hip, kind):
    from libflagstats_amd import device
    rng = np.random.RandomState(5 if kind == "uniform" else 6)
    n = 3_000_017
    x = flags_of(kind, n, 41)
    d = device.DeviceFlags(n + 8)
    d.upload(x)
    layouts = {
        "whole": np.array([0, n]),
        "equal": np.append(np.arange(0, n, 100_001), n),
        "random": np.concatenate([[0], np.cumsum(random_lengths(rng, 2000))]),
        "inner": 12_345 + np.concatenate([[0], np.cumsum(random_lengths(rng, 700))]),
        "dense": 3 + np.concatenate([[0], np.cumsum(rng.randint(0, 2000, 2500))]),
    }
    for name, o in layouts.items():
        o = o.astype(np.int64)
        o = o[o <= n]
        assert o.size >= 2
        for sup in (False, True):
            want = segmented_counters(x, o, superset=sup)
            flags = 2 if sup else 0
            got = device_counts(hip, d.ptr, n, o, flags | 1)
            assert np.array_equal(got, want), (name, sup, "store")
            got = device_counts(hip, d.ptr, n, o, flags)
            assert np.array_equal(got, want), (name, sup, "+=")
            out = np.zeros((o.size - 1, 32), dtype=np.uint64)
            assert hip.FLAGSTATS_hip_device_u16_segments_sync(d.ptr, n, o.astype(np.uint64).ctypes.data, o.size - 1, out.ctypes.data, flags) == 0
            assert np.array_equal(out, want), (name, sup, "sync")
        # invariant: the rows sum to the existing entry's count of [offsets[0], offsets[-1])
        whole = d.count(offset=int(o[0]), n=int(o[-1] - o[0]))
        assert np.array_equal(segmented_counters(x, o).sum(axis=0), whole) and np.array_equal(
            device_counts(hip, d.ptr, n, o, 1).sum(axis=0), whole), name
    # one segment equal to the whole array matches FLAGSTATS_hip_device_u16_store
    ref = Dev(hip, 256)
    assert hip.FLAGSTATS_hip_device_u16_store(d.ptr, n, ref.ptr, None) == 0 and hip.FLAGSTATS_hip_synchronize() == 0
    assert np.array_equal(device_counts(hip, d.ptr, n, np.array([0, n]), 1)[0], ref.get(32, np.uint64))
    ref.free()
    d.free()


def test_base_pointer_offsets_and_store_garbage(hip):
    from libflagstats_amd import device
    rng = np.random.RandomState(9)
    n = 1_000_003
    x = flags_of("uniform", n + 8, 3)
    d = device.DeviceFlags(n + 8)
    d.upload(x)
    for shift in range(1, 8):
        xs = x[shift:shift + n]
        o = np.concatenate([[0], np.cumsum(random_lengths(rng, 400))])
        o = np.append(o[o < n], n)
        want = segmented_counters(xs, o)
        got = device_counts(hip, d.ptr + 2 * shift, n, o, 1)          # garbage-filled out[] overwritten
        assert np.array_equal(got, want), shift
        empty = o[1:] == o[:-1]
        assert not got[empty].any()
        dead = [s for s in range(32) if s not in (2, 6, 7, 8, 10, 11, 12, 13, 14, 18, 22, 23, 24, 25, 26, 27, 28, 29, 30)]
        assert not got[:, dead].any()
    d.free()


def test_accumulate_doubles_and_nseg_zero(hip):
    from libflagstats_amd import device
    n = 500_000
    x = flags_of("na12878", n, 7)
    d = device.DeviceFlags(n).upload(x)
    o = np.concatenate([[0], np.cumsum(np.random.RandomState(1).randint(0, 5000, 150))])
    o = np.append(o[o < n], n).astype(np.uint64)
    nseg = o.size - 1
    off = Dev(hip, o.nbytes).put(o)
    out = Dev(hip, nseg * 256).put(np.zeros((nseg, 32), dtype=np.uint64))
    for _ in range(2):
        assert hip.FLAGSTATS_hip_device_u16_segments(d.ptr, n, off.ptr, nseg, out.ptr, 0, None) == 0
    assert hip.FLAGSTATS_hip_synchronize() == 0
    assert np.array_equal(out.get((nseg, 32), np.uint64), 2 * segmented_counters(x, o))
    # nseg == 0: nothing, success, on every form
    h = np.full(32, 5, dtype=np.uint64)
    assert hip.FLAGSTATS_hip_device_u16_segments(d.ptr, n, off.ptr, 0, out.ptr, 1, None) == 0
    assert hip.FLAGSTATS_hip_device_u16_segments_sync(d.ptr, n, o.ctypes.data, 0, h.ctypes.data, 1) == 0
    assert hip.FLAGSTATS_hip_u16_x64_segments(x.ctypes.data, n, o.ctypes.data, 0, h.ctypes.data, 1) == 0
    assert (h == 5).all()
    off.free()
    out.free()
    d.free()


def test_a_million_tiny_segments(hip):
    from libflagstats_amd import device
    rng = np.random.RandomState(21)
    lengths = rng.randint(0, 4, (1 << 20) + 77)
    o = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(o[-1]) + 5
    x = flags_of("uniform", n, 8)
    d = device.DeviceFlags(n).upload(x)
    for flags in (1, 3):
        got = device_counts(hip, d.ptr, n, o, flags)
        assert np.array_equal(got, segmented_counters(x, o, superset=bool(flags & 2))), flags
    d.free()


def test_host_array_form_spans_chunks(hip):
    from libflagstats_amd import _lib, segments
    rng = np.random.RandomState(33)
    n = 5_000_011
    x = flags_of("uniform", n, 12)
    o = np.concatenate([[0], np.cumsum(rng.randint(0, 400_000, 30))])
    o = 17 + np.append(o[o < n - 40], n - 40)
    want = segmented_counters(x, o)
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    p = hip.FLAGSTATS_hip_host_alloc(x.nbytes)
    assert p
    try:
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", 1_000_003), "chunk_flags")
        assert np.array_equal(segments.flagstats_segments(x, o), want)                         # pageable
        assert np.array_equal(segments.flagstats_segments(x, o, superset=True), segmented_counters(x, o, superset=True))
        ctypes.memmove(p, x.ctypes.data, x.nbytes)
        acc = np.ones((o.size - 1, 32), dtype=np.uint64)
        oo = o.astype(np.uint64)
        assert hip.FLAGSTATS_hip_u16_x64_segments(p, n, oo.ctypes.data, o.size - 1, acc.ctypes.data, 0) == 0   # page-locked, +=
        assert np.array_equal(acc, want + 1)
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
        hip.FLAGSTATS_hip_host_free(p)
    # default chunk, dicts per segment
    got = segments.flagstats_segments(x, o)
    assert np.array_equal(got, want)
    dicts = segments.segment_dicts(got, o)
    assert dicts[3]["n_values"] == int(o[4] - o[3]) and dicts[3]["failed"]["FQCFAIL"] == want[3, 25]


def test_host_array_form_many_small_segments_over_many_chunks(hip):
    """Thousands of ~1,000-flag segments over a couple of dozen chunks: every chunk's launch meets the segments after it (clamped
    to empty at the chunk's end) and must stop at its range's end, the counts exact whatever the chunk boundaries cut."""
    from libflagstats_amd import _lib, segments
    rng = np.random.RandomState(8)
    n = 6_000_007
    x = flags_of("na12878", n, 19)
    o = 5 + np.concatenate([[0], np.cumsum(rng.randint(0, 2001, 7000))])
    o = np.append(o[o < n - 11], n - 11)
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        for chunk in (262_147, 4096, old):
            _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", chunk), "chunk_flags")
            assert np.array_equal(segments.flagstats_segments(x, o), segmented_counters(x, o)), chunk
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", 262_147), "chunk_flags")
        assert np.array_equal(segments.flagstats_segments(x, o, superset=True), segmented_counters(x, o, superset=True))
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)


def test_device_ptr_helper(hip):
    from libflagstats_amd import device, segments
    n = 777_777
    d = device.DeviceFlags(n).generate(device.GEN_NA12878, seed=4, mask=0)
    x = d.download()
    o = segments.offsets_from_lengths([0, 1000, 70_000, 0, 5, 300_000])
    assert np.array_equal(segments.count_segments_device_ptr(d.ptr, n, o), segmented_counters(x, o))
    d.free()


def test_torch_two_streams(hip):
    import torch
    from libflagstats_amd import segments
    rng = np.random.RandomState(2)
    n = 2_000_003
    x = flags_of("uniform", n, 31)
    t = torch.from_numpy(x.view(np.int16)).cuda()
    o1 = segments.offsets_from_lengths(rng.randint(0, 20_000, 150))
    o2 = segments.offsets_from_lengths(rng.randint(0, 3_000, 500)) + 1000
    o1, o2 = o1[o1 <= n], o2[o2 <= n]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    offs = [torch.from_numpy(o.astype(np.int64)).cuda() for o in (o1, o2)]
    torch.cuda.synchronize()
    outs = []
    for rep in range(3):
        with torch.cuda.stream(s1):
            a = segments.count_segments_torch(t, offs[0])
        with torch.cuda.stream(s2):
            b = segments.count_segments_torch(t, offs[1], superset=True)
            b2 = torch.zeros_like(b)
            segments.count_segments_torch(t, offs[1], out=b2, store=False)
            segments.count_segments_torch(t, offs[1], out=b2, store=False)
        outs.append((a, b, b2))
    torch.cuda.synchronize()
    for a, b, b2 in outs:
        assert np.array_equal(a.cpu().numpy().astype(np.uint64), segmented_counters(x, o1))
        assert np.array_equal(b.cpu().numpy().astype(np.uint64), segmented_counters(x, o2, superset=True))
        assert np.array_equal(b2.cpu().numpy().astype(np.uint64), 2 * segmented_counters(x, o2))
    with pytest.raises(ValueError):
        segments.count_segments_torch(t, offs[0].to(torch.int32))


def test_error_paths_leave_out_untouched(hip):
    from libflagstats_amd import device
    n = 100_000
    d = device.DeviceFlags(n).generate(device.GEN_UNIFORM, seed=1)
    x = d.download()
    out = np.full((3, 32), 9, dtype=np.uint64)
    cases = {
        "decreasing": np.array([0, 50, 40, 100], dtype=np.uint64),
        "beyond n": np.array([0, 50, 60, n + 1], dtype=np.uint64),
    }
    for name, o in cases.items():
        for rc in (hip.FLAGSTATS_hip_device_u16_segments_sync(d.ptr, n, o.ctypes.data, 3, out.ctypes.data, 0),
                   hip.FLAGSTATS_hip_u16_x64_segments(x.ctypes.data, n, o.ctypes.data, 3, out.ctypes.data, 0)):
            assert rc != 0 and hip.FLAGSTATS_hip_last_error(), name
            assert (out == 9).all(), name
    good = np.array([0, 10, 20, 30], dtype=np.uint64)
    assert hip.FLAGSTATS_hip_u16_x64_segments(x.ctypes.data, n, None, 3, out.ctypes.data, 0) != 0
    assert hip.FLAGSTATS_hip_u16_x64_segments(x.ctypes.data, n, good.ctypes.data, 3, None, 0) != 0
    assert hip.FLAGSTATS_hip_u16_x64_segments(None, n, good.ctypes.data, 3, out.ctypes.data, 0) != 0
    assert hip.FLAGSTATS_hip_device_u16_segments_sync(None, n, good.ctypes.data, 3, out.ctypes.data, 0) != 0
    assert hip.FLAGSTATS_hip_device_u16_segments(d.ptr, n, None, 3, None, 0, None) != 0
    for absurd in (1 << 62, (1 << 56) + 3, 1 << 40):  # nseg * 256 bytes of counters: not a size / not allocatable
        assert hip.FLAGSTATS_hip_device_u16_segments_sync(d.ptr, n, good.ctypes.data, absurd, out.ctypes.data, 0) != 0
        assert hip.FLAGSTATS_hip_u16_x64_segments(x.ctypes.data, n, good.ctypes.data, absurd, out.ctypes.data, 0) != 0
        assert hip.FLAGSTATS_hip_last_error()
    assert (out == 9).all()
    # device form: counters buffer or offsets too short for nseg are refused before the launch
    off = Dev(hip, good.nbytes).put(good)
    small = Dev(hip, 256)
    assert hip.FLAGSTATS_hip_device_u16_segments(d.ptr, n, off.ptr, 3, small.ptr, 1, None) != 0
    assert hip.FLAGSTATS_hip_device_u16_segments(d.ptr, n, off.ptr, 1 << 40, small.ptr, 1, None) != 0
    # host counters are refused for the device form
    assert hip.FLAGSTATS_hip_device_u16_segments(d.ptr, n, off.ptr, 3, out.ctypes.data, 1, None) != 0
    assert (out == 9).all()
    # malformed DEVICE offsets (decreasing, beyond n) are clamped: counters undefined, nothing read or written out of bounds
    bad = Dev(hip, 32).put(np.array([70_000, 10, 1 << 60, 5], dtype=np.uint64))
    big = Dev(hip, 3 * 256 + 256).put(np.full((4, 32), 3, dtype=np.uint64))
    assert hip.FLAGSTATS_hip_device_u16_segments(d.ptr, n, bad.ptr, 3, big.ptr, 1, None) == 0
    assert hip.FLAGSTATS_hip_synchronize() == 0
    assert (big.get((4, 32), np.uint64)[3] == 3).all()   # the row past nseg is untouched
    for b in (off, small, bad, big):
        b.free()
    d.free()


@pytest.mark.parametrize("layout", ["blocks", "random", "whole", "long"])
def test_full_size_device_resident(hip, layout):
    """2^32 flags on the device cut into 512,000-flag blocks (the column store's block size), random lengths, one segment (1,024
    units per wave: four chain epochs each) or long unaligned segments of 1-8 M flags; every segment checked against the
    oracle's generator without a host copy of the 8 GiB, in the store and += forms; then the same layout over a periodic array
    (filled on the device) with superset, against segments_oracle.periodic_counters."""
    import oracle
    import torch
    from libflagstats_amd import device
    from segments_oracle import SEG_EPOCH, periodic_counters, writer_ranges
    n = 1 << 32
    kind, seed, mask = oracle.GEN_UNIFORM, 77, 0xFFFF
    d = device.DeviceFlags(n).generate(kind, seed=seed, mask=mask)
    if layout == "blocks":
        o = np.append(np.arange(0, n, 512_000, dtype=np.int64), n)
    elif layout == "random":
        rng = np.random.RandomState(4)
        o = np.concatenate([[0], np.cumsum(rng.randint(0, 1_024_000, 9000))]).astype(np.int64) + 999
        o = np.append(o[o < n - 5], n - 5)
    elif layout == "whole":
        o = np.array([0, n], dtype=np.int64)
    else:
        rng = np.random.RandomState(5)
        o = np.concatenate([[0], np.cumsum(rng.randint(1_000_000, 8_000_001, 1100))]).astype(np.int64) + 7
        o = np.append(o[o < n - 3], n - 3)
    w = writer_ranges(d.ptr % 16, n, hip.FLAGSTATS_hip_compute_units())
    chain = w.pieces(o)["chain"]
    if layout == "whole":
        assert (chain == 1024).all() and chain.size == w.waves == 1024, (chain.min(), chain.max())
    if layout == "long":
        assert chain.max() > SEG_EPOCH
    got = device_counts(hip, d.ptr, n, o, 1)
    acc = device_counts(hip, d.ptr, n, o, 0)
    for i in range(o.size - 1):
        want = oracle.flagstat_generated(kind, seed, mask, first_index=int(o[i]), n=int(o[i + 1] - o[i]), threads=16)
        assert np.array_equal(got[i], want), (layout, i)
        assert np.array_equal(acc[i], want), (layout, i, "+=")
    assert np.array_equal(got.sum(axis=0), d.count(offset=int(o[0]), n=int(o[-1] - o[0])))
    d.free()
    pattern = np.random.RandomState(78).randint(0, 65536, 65_521).astype(np.uint16)
    t = torch.from_numpy(pattern.view(np.int16)).cuda().repeat(-(-n // pattern.size))
    torch.cuda.synchronize()
    want = periodic_counters(pattern, o, superset=True)
    for flags in (3, 2):
        assert np.array_equal(device_counts(hip, t.data_ptr(), n, o, flags), want), (layout, "superset", flags)
    del t
    torch.cuda.empty_cache()   # 8-16 GiB back to the device for the tests after this one
