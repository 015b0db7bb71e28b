"""Segmented flagstat, host side (no GPU): the Python module's argument checks, the offsets helper, the test oracle itself,
and the C entries' loud failure on a box without a GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from segments_oracle import segmented_counters  # noqa: E402


@pytest.mark.parametrize("offsets, why", [
    ([0, 5, 3, 10], "non-decreasing"),
    ([0, 5, 11], "exceeds"),
    (np.array([[0, 5], [5, 10]]), "1-D"),
    (np.array([0.0, 5.0, 10.0]), "integer"),
    (np.array([-1, 5, 10], dtype=np.int64), "negative"),
    (np.array([], dtype=np.uint64), ">= 1"),
])
def test_bad_offsets_raise_before_the_library_is_touched(monkeypatch, offsets, why):
    from libflagstats_amd import _lib, segments

    def untouchable():
        raise AssertionError("the library was called before the offsets were checked")

    monkeypatch.setattr(_lib, "lib", untouchable)
    values = np.zeros(10, dtype=np.uint16)
    with pytest.raises(ValueError, match=why):
        segments.flagstats_segments(values, offsets)
    with pytest.raises(ValueError, match=why):
        segments.count_segments_device_ptr(0x1000, 10, offsets)


def test_flagstats_segments_wants_a_uint16_vector(monkeypatch):
    from libflagstats_amd import _lib, segments
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    with pytest.raises(ValueError):
        segments.flagstats_segments(np.zeros(10, dtype=np.int32), [0, 10])
    with pytest.raises(ValueError):
        segments.flagstats_segments(np.zeros((2, 5), dtype=np.uint16), [0, 10])


def test_offsets_from_lengths_round_trips():
    from libflagstats_amd.segments import offsets_from_lengths
    rng = np.random.RandomState(3)
    for lengths in ([], [0], [5], [0, 0, 3, 0], rng.randint(0, 2000, 1000)):
        o = offsets_from_lengths(lengths)
        assert o.dtype == np.uint64 and o.size == len(lengths) + 1 and o[0] == 0
        assert np.array_equal(np.diff(o.astype(np.int64)), np.asarray(lengths, dtype=np.int64))
    assert np.array_equal(offsets_from_lengths(np.array([2, 3], dtype=np.int32)), [0, 2, 5])
    with pytest.raises(ValueError):
        offsets_from_lengths([3, -1])
    with pytest.raises(ValueError):
        offsets_from_lengths([[1, 2]])


def test_segment_dicts_shape():
    from libflagstats_amd.segments import segment_dicts
    c = np.zeros((2, 32), dtype=np.uint64)
    c[1, 2] = 3          # FUNMAP pass
    d = segment_dicts(c, [0, 4, 10])
    assert [x["n_values"] for x in d] == [4, 6]
    assert d[1]["passed"]["FUNMAP"] == 3 and d[1]["passed"]["mapped"] == 3
    with pytest.raises(ValueError):
        segment_dicts(c, [0, 4])


def test_segmented_oracle_agrees_with_the_oracle_per_segment(oracle_mod):
    rng = np.random.RandomState(11)
    x = rng.randint(0, 65536, 400_000).astype(np.uint16)
    lengths = rng.choice([0, 0, 1, 2, 7, 8, 9, 100, 1000, 4095, 4096, 4097, 16383, 16384, 16385], 60)
    for head, tail in ((0, 0), (13, 0), (0, 17), (5, 9)):
        o = head + np.concatenate([[0], np.cumsum(lengths)])
        assert o[-1] + tail <= x.size
        xs = x[:o[-1] + tail]
        got = segmented_counters(xs, o)
        for i in range(len(lengths)):
            assert np.array_equal(got[i], oracle_mod.flagstat_hist(xs[o[i]:o[i + 1]])), (head, tail, i)
        # superset slots: 0/16 primary paired by QC class, 9 = length - slot 25
        sup = segmented_counters(xs, o, superset=True)
        for i in range(len(lengths)):
            a = xs[o[i]:o[i + 1]]
            pp = ((a & 0x100) == 0) & ((a & 0x800) == 0) & ((a & 1) == 1)
            fail = (a & 0x200) != 0
            want = oracle_mod.flagstat_hist(a).copy()
            want[0], want[16], want[9] = int((pp & ~fail).sum()), int((pp & fail).sum()), a.size - int(fail.sum())
            assert np.array_equal(sup[i], want), (head, tail, i)
    # all empty, no segments, an empty array
    assert not segmented_counters(x, [5, 5, 5]).any()
    assert segmented_counters(x, [7]).shape == (0, 32)
    assert segmented_counters(x[:0], [0, 0]).shape == (1, 32)


def test_no_gpu_means_the_segment_entries_fail_loudly():
    """Without a GPU the segmented entries return non-zero with a message and leave `out` alone; nothing is computed on the
    CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from libflagstats_amd import _lib, segments
    lib = _lib.lib()
    a = np.arange(100, dtype=np.uint16)
    o = np.array([0, 40, 100], dtype=np.uint64)
    out = np.full((2, 32), 7, dtype=np.uint64)
    calls = [
        ("FLAGSTATS_u16_x64_segments", lambda: lib.FLAGSTATS_hip_u16_x64_segments(a.ctypes.data, a.size, o.ctypes.data, 2, out.ctypes.data, 0)),
        ("device_u16_segments_sync", lambda: lib.FLAGSTATS_hip_device_u16_segments_sync(a.ctypes.data, a.size, o.ctypes.data, 2, out.ctypes.data, 1)),
        ("device_u16_segments", lambda: lib.FLAGSTATS_hip_device_u16_segments(a.ctypes.data, a.size, o.ctypes.data, 2, out.ctypes.data, 0, None)),
    ]
    for name, call in calls:
        assert call() != 0, name
        assert lib.FLAGSTATS_hip_last_error(), name
        assert (out == 7).all(), name
    with pytest.raises(_lib.FlagstatsHipError):
        segments.flagstats_segments(a, o)
    # nseg == 0 does nothing and succeeds, GPU or not
    assert lib.FLAGSTATS_hip_u16_x64_segments(a.ctypes.data, a.size, o.ctypes.data, 0, out.ctypes.data, 0) == 0


def test_periodic_oracle_agrees_with_the_segmented_oracle():
    from segments_oracle import periodic_counters, segmented_counters_many
    rng = np.random.RandomState(23)
    for trial in range(40):
        period = int(rng.choice([1, 2, 3, 4, 7, 8, 64, 511, 4096, 4099, rng.randint(1, 20_000)]))
        pattern = rng.randint(0, 65536, period).astype(np.uint16)
        phase = int(rng.randint(0, 3 * period))
        n = int(rng.randint(1, 200_000))
        x = np.resize(np.roll(pattern, -(phase % period)), n)
        cuts = np.sort(rng.randint(0, n + 1, rng.randint(0, 60)))
        o = np.concatenate([[0], cuts, [n]]) if trial % 2 else np.concatenate([cuts[:1], cuts, cuts[-1:]]) if cuts.size else np.array([0, n])
        for sup in (False, True):
            want = segmented_counters(x, o, superset=sup)
            assert np.array_equal(periodic_counters(pattern, o, superset=sup, phase=phase), want), (trial, period, sup)
            assert np.array_equal(segmented_counters_many(x, [o, o[::2]], superset=sup)[0], want), (trial, sup)
    # far past any host array: the counts scale by whole periods
    pattern = rng.randint(0, 65536, 4099).astype(np.uint16)
    big = periodic_counters(pattern, [0, 4099 * (1 << 22), 4099 * (1 << 22) + 4099], superset=True)
    one = segmented_counters(pattern, [0, 4099], superset=True)[0]
    assert np.array_equal(big[0], one * np.uint64(1 << 22)) and np.array_equal(big[1], one)


def test_batched_oracle_matches_per_layout():
    from segments_oracle import segmented_counters_many
    rng = np.random.RandomState(29)
    x = rng.randint(0, 65536, 300_001).astype(np.uint16)
    layouts = [np.array([0, x.size]), np.array([5, 5, 7, 4096, 4097, 300_000]), np.array([9]),
               np.concatenate([[0], np.sort(rng.randint(0, x.size + 1, 500)), [x.size]])]
    for sup in (False, True):
        for o, got in zip(layouts, segmented_counters_many(x, layouts, superset=sup)):
            assert np.array_equal(got, segmented_counters(x, o, superset=sup))


def _source(*parts):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, *parts)) as f:
        return f.read()


def test_writer_mirror_matches_the_sources():
    """The writer split the GPU regime tests place their boundaries by (segments_oracle.WriterSplit) restates the launcher's
    and the kernel prologue's arithmetic: if either changes, this test names what to update."""
    import re

    import segments_oracle as so
    hdr = _source("libflagstats_amd", "csrc", "flagstat_segments.h")
    src = re.sub(r"\s+", " ", _source("libflagstats_amd", "csrc", "flagstat_segments.hip"))
    k1 = _source("libflagstats_amd", "csrc", "flagstat_kernels.h")
    core = re.sub(r"\s+", " ", _source("libflagstats_amd", "csrc", "flagstat_count_core.h"))
    assert int(re.search(r"constexpr int kSegWaveFlags = (\d+);", hdr).group(1)) == so.SEG_UNIT
    assert int(re.search(r"constexpr int kThreads = (\d+);", k1).group(1)) == 64 * so.SEG_WAVES_PER_BLOCK
    assert (1 << int(re.search(r"constexpr int kSegDepth = (\d+);", src).group(1))) - 1 == so.SEG_EPOCH
    assert "static std::atomic<uint32_t> g_seg_min_units{%d};" % so.SEG_MIN_UNITS in src
    # the launcher's shape and the kernel's walk are the segmented kernels' shared ones (flagstat_segments_shared.h), which this
    # unit instantiates for its unit of kSegWaveFlags elements of 8192 / kSegWaveFlags = 2 bytes
    shared = re.sub(r"\s+", " ", _source("libflagstats_amd", "csrc", "flagstat_segments_shared.h"))
    assert "fsseg::launch_shape(addr, m, fsk::kSegWaveFlags, grid, &lo0, &nunits, &g);" in src
    assert "reinterpret_cast<const uint4*>(a0), lo0, lo0 + m, base," in src and "seg_walk<kSegWaveFlags>( lo0, hi0, base," in src
    assert "constexpr int kSegUnitVecs = kSegWaveFlags / 8;" in shared
    for rule in ("const uint64_t W = fsk::kSegUnitVecs * 16 / ue;",
                 "*lo0 = (addr & 15u) / W;",
                 "*nunits = (*lo0 + m + ue - 1) / ue;",
                 "const uint64_t want = (*nunits + 3) / 4;",
                 "*g = want < grid ? static_cast<uint32_t>(want) : grid;",
                 "const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (kThreads / 64);",
                 "const uint64_t u_begin = gw * nunits / waves, u_end = (gw + 1) * nunits / waves;",
                 "const uint64_t p0 = u_begin * UE > lo0 ? u_begin * UE : lo0;",
                 "const uint64_t E = u_end * UE < hi0 ? u_end * UE : hi0;",
                 "if (k >= min_units && k > 0) {",
                 "(mode & 1) && b_ >= p0 && e_ <= E"):
        assert shared.count(rule) == 1, rule
    # the epoch test lives once in the shared end_step, which the chain step calls at the segmented kernel's depth
    assert core.count("if (blk == (1u << DEPTH) - 1u) {") == 1 and "end_step<kSegDepth>(s, blk);" in src


def test_writer_mirror_partitions_the_array():
    from segments_oracle import SEG_UNIT, writer_ranges
    rng = np.random.RandomState(31)
    for addr in range(0, 16, 2):
        for n, grid in ((1, 1), (4096, 1), (4096 * 9 + 3, 2), (1 << 20, 7), (12_345_679, 3), (1 << 25, 1024)):
            w = writer_ranges(addr, n, grid)
            assert w.begin[0] == 0 and w.end[-1] == n and (w.begin[1:] == w.end[:-1]).all() and (w.end >= w.begin).all()
            assert w.grid == min(grid, (w.nunits + 3) // 4) and w.waves == 4 * w.grid
            inner = (w.u_end * SEG_UNIT - w.lo0)[:-1]   # every seam is a unit boundary
            assert np.array_equal(w.end[:-1], np.clip(inner, 0, n))
            cuts = np.sort(rng.randint(0, n + 1, 50))
            o = np.concatenate([[0], cuts, [n]])
            for mu in (0, 1, 2, 255, 0xFFFFFFFF):
                p = w.pieces(o, mu)
                lengths = np.bincount(p["seg"], weights=p["e"] - p["b"], minlength=o.size - 1)
                assert np.array_equal(lengths, np.diff(o)), (addr, n, grid)
                assert np.array_equal(p["head"] + p["chain"] * SEG_UNIT + p["tail"], p["e"] - p["b"])
                assert (p["head"] >= 0).all() and (p["tail"] >= 0).all() and (p["tail"] < SEG_UNIT).all()
                assert (p["chain"] == 0).all() or mu != 0xFFFFFFFF
                assert ((p["head"][p["chain"] > 0] + p["b"][p["chain"] > 0] + w.lo0) % SEG_UNIT == 0).all()
                # the store form's plain rows are exactly the segments held by one writer
                per_seg = np.bincount(p["seg"], minlength=o.size - 1)
                assert np.array_equal(p["plain"], per_seg[p["seg"]] == 1)
