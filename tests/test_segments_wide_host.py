"""Segmented flagstat on int32 / int64 columns (libflagstats_amd/segments_wide.py, csrc/flagstat_segments_wide.hip) on the CPU: the
package's exports, the refusals of the Python layer -- raised before the library is loaded --, the text of the strict error, the
symbols in the binding table, the built library and the header, the oracle against oracle_mod segment by segment, the writer
mirror against the sources, and the C entries' loud failure on a box without a GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_wide_oracle as swo  # noqa: E402
import wide_filter_oracle  # noqa: E402

from libflagstats_amd import segments_wide as sw  # noqa: E402  (fails at import where the feature is missing)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = {"FLAGSTATS_hip_device_wide_segments": 9, "FLAGSTATS_hip_device_wide_segments_sync": 8, "FLAGSTATS_hip_wide_x64_segments": 8}
PY_NAMES = ("counters_segments_ints", "flagstats_segments_ints", "count_segments_device_ptr_ints", "count_segments_torch_ints")
DTYPES = (np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64)


@pytest.fixture()
def no_library(monkeypatch):
    """loading the library fails the test: the refusals must come first"""
    from libflagstats_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were refused")

    monkeypatch.setattr(_lib, "lib", boom)


def test_exports_and_shared_checks():
    import libflagstats_amd
    from libflagstats_amd import segments, wide
    for name in PY_NAMES:
        assert getattr(libflagstats_amd, name) is getattr(sw, name) and name in libflagstats_amd.__all__
    # the checks are the other modules', not restated
    assert sw.check_offsets is segments.check_offsets and sw._check_values is wide._check_values
    assert sw._check_tensor is wide._check_tensor and sw.high_bits_message is wide.high_bits_message


BAD_OFFSETS = (([0, 5, 3, 10], "non-decreasing"), ([0, 5, 11], "exceeds"), (np.array([[0, 5], [5, 10]]), "1-D"),
               (np.array([0.0, 5.0, 10.0]), "integer"), (np.array([-1, 5, 10], dtype=np.int64), "negative"),
               (np.array([], dtype=np.uint64), ">= 1"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_offsets_and_values_raise_before_the_library_is_touched(no_library, dtype):
    values = np.zeros(10, dtype=dtype)
    for offsets, why in BAD_OFFSETS:
        for f in (sw.counters_segments_ints, sw.flagstats_segments_ints):
            with pytest.raises(ValueError, match=why):
                f(values, offsets)
        with pytest.raises(ValueError, match=why):
            sw.count_segments_device_ptr_ints(0x1000, 10, 8, offsets)
    for f in (sw.counters_segments_ints, sw.flagstats_segments_ints):
        with pytest.raises(ValueError, match=r"values must be a numpy\.ndarray, not list"):
            f([1, 2, 3], [0, 3])
        for bad in (np.zeros(10, dtype=np.int8), np.zeros(10, dtype=np.float32), np.zeros(10, dtype=bool)):
            with pytest.raises(ValueError, match=r"values must have an integer dtype of 2, 4 or 8 bytes"):
                f(bad, [0, 10])
        with pytest.raises(ValueError, match=r"values must be 1-D, not 2-D"):
            f(np.zeros((2, 5), dtype=dtype), [0, 10])
        with pytest.raises(ValueError, match=r"native"):
            f(np.zeros(10, dtype=np.dtype(dtype).newbyteorder(">")), [0, 10])


def test_device_pointer_and_torch_refusals(no_library):
    import torch
    f = sw.count_segments_device_ptr_ints
    o = np.array([0, 4, 10])
    for eb in (2, 1, 16, 0, None):
        with pytest.raises(ValueError, match=r"elem_bytes must be 4 or 8"):
            f(0x1000, 10, eb, o)
    with pytest.raises(ValueError, match=r"n must not be negative"):
        f(0x1000, -1, 4, o)
    with pytest.raises(ValueError, match=r"ptr must be an int, not float"):
        f(4096.0, 10, 4, o)
    with pytest.raises(ValueError, match=r"n must fit an unsigned 64-bit integer"):
        f(0x1000, 1 << 64, 4, o)
    g = sw.count_segments_torch_ints
    t = torch.zeros(20, dtype=torch.int32)
    off = torch.tensor([0, 7, 20], dtype=torch.int64)
    with pytest.raises(ValueError, match=r"t must be a torch\.Tensor, not ndarray"):
        g(np.zeros(20, dtype=np.int32), off)
    for dt in (torch.uint8, torch.int8, torch.bool, torch.float32):
        with pytest.raises(ValueError, match=r"t must have an integer dtype of 2, 4 or 8 bytes"):
            g(torch.zeros(20, dtype=dt), off)
    for bad in (torch.zeros((4, 5), dtype=torch.int64), torch.zeros(40, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
            g(bad, off)
    for bad in (np.array([0, 20]), torch.tensor([0, 20], dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int64),
                torch.zeros(0, dtype=torch.int64), torch.zeros(6, dtype=torch.int64)[::2]):
        with pytest.raises(ValueError, match=r"offsets must be a 1-D contiguous int64 tensor \(nseg \+ 1 values\)"):
            g(t, bad)
    for bad in (torch.zeros((3, 32), dtype=torch.int64), torch.zeros((2, 32), dtype=torch.int32), torch.zeros(64, dtype=torch.int64),
                np.zeros((2, 32), dtype=np.int64)):
        with pytest.raises(ValueError, match=r"out must be a contiguous int64 tensor of shape \(2, 32\)"):
            g(t, off, out=bad)
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int64), 0):
        with pytest.raises(ValueError, match=r"high must be a contiguous int64 tensor of shape \(2,\)"):
            g(t, off, high=bad)
    with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
        g(t, off)


def test_strict_names_the_first_offending_segment(monkeypatch):
    o = np.array([3, 10, 10, 25, 40], dtype=np.int64)
    high = np.array([0, 0, 0x80000000, 0x10000], dtype=np.uint64)
    text = sw.strict_message(high, o)
    assert text == "segment 2 (offsets 10..25): values outside 0..65535: bits 0x80000000 set above bit 15"
    rows = np.zeros((4, 32), dtype=np.uint64)
    calls = []

    def fake(values, offsets, superset=False):
        calls.append(superset)
        return rows, fake.high

    monkeypatch.setattr(sw, "counters_segments_ints", fake)
    fake.high = high
    with pytest.raises(ValueError, match=re.escape(text)):
        sw.flagstats_segments_ints(np.zeros(40, dtype=np.int32), o)
    got = sw.flagstats_segments_ints(np.zeros(40, dtype=np.int32), o, superset=True, strict=False)
    assert got[0] is rows and got[1] is high and calls == [False, True]
    fake.high = np.zeros(4, dtype=np.uint64)
    assert sw.flagstats_segments_ints(np.zeros(40, dtype=np.int32), o)[1] is fake.high
    fake.high = np.array([0, 0, 0, 1 << 63], dtype=np.uint64)
    with pytest.raises(ValueError, match=r"segment 3 \(offsets 25\.\.40\): .*bits 0x8000000000000000 set"):
        sw.flagstats_segments_ints(np.zeros(40, dtype=np.int64), o)


def test_symbols_in_the_table_the_library_and_the_header():
    import ctypes

    from libflagstats_amd import _lib
    for name, nargs in PUBLIC.items():
        assert name in _lib.SIGNATURES and name not in _lib.INTERNAL_SIGNATURES, name
        args = _lib.SIGNATURES[name][1]
        assert len(args) == nargs, name
        assert args[1] is ctypes.c_uint64 and args[2] is ctypes.c_int and args[4] is ctypes.c_uint64, name   # n, elem_bytes, nseg
    assert len(_lib.INTERNAL_SIGNATURES["fsk_launch_segments_wide"][1]) == 11 and "fsk_launch_segments_wide" not in _lib.SIGNATURES
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in tuple(PUBLIC) + ("fsk_launch_segments_wide",):
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    assert header.index("wide input per segment:") > header.index("filtered wide input:")
    for name, nargs in PUBLIC.items():
        m = re.search(r"\bint %s\(([^)]*)\)" % name, header)
        assert m and len(m.group(1).split(",")) == nargs, name
    decl = open(os.path.join(ROOT, "libflagstats_amd", "csrc", "flagstat_segments_wide.h")).read()
    m = re.search(r"\bhipError_t fsk_launch_segments_wide\(([^)]*)\)", decl)
    assert m and len(m.group(1).split(",")) == 11 and "fsk_launch_segments_wide" not in header


def test_code_objects():
    """K1's code object is the one profiles/traffic.json was measured on; one gfx950 code object defines both
    fsk::flagstat_segments_wide instantiations and no other unit's kernel"""
    import json

    from libflagstats_amd import _lib, kernel_id
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        assert kernel_id.kernel_id(_lib.LIB_PATH) == json.load(f)["kernel_source_id"]
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    holders = []
    for co in kernel_id._code_objects(so):
        secs = kernel_id._sections(co)
        names = b"".join(co[secs[t][0]:secs[t][0] + secs[t][1]] for t in (".strtab", ".dynstr") if t in secs)
        if b"_ZN3fsk22flagstat_segments_wideILi4" in names:
            assert b"_ZN3fsk22flagstat_segments_wideILi8" in names
            for other in (b"_ZN3fsk14flagstat_count", b"_ZN3fsk17flagstat_segmentsE", b"_ZN3fsk19flagstat_count_wide",
                          b"_ZN3fsk24flagstat_segments_filter", b"_ZN3fsk26flagstat_count_wide_filter"):
                assert other not in names, other
            holders.append(co)
        else:
            assert b"_ZN3fsk22flagstat_segments_wide" not in names
    assert len(holders) == 1


def wide_column(rng, n, dtype, every=97):
    """random FLAG values widened to dtype, one element in `every` carrying random bits above bit 15 (negative ones included)"""
    W = np.dtype(dtype).itemsize
    u = rng.randint(0, 65536, n).astype(np.uint64)
    hot = rng.randint(0, every, n) == 0
    hi = rng.randint(0, 1 << 16, n).astype(np.uint64) << np.uint64(16)
    if W == 8:
        hi |= rng.randint(0, 1 << 32, n).astype(np.uint64) << np.uint64(32)
    u |= np.where(hot, hi, np.uint64(0)).astype(np.uint64)
    return u.astype(np.uint32 if W == 4 else np.uint64).view(dtype)


@pytest.mark.parametrize("dtype", DTYPES[2:])
def test_oracle_against_oracle_mod_per_segment(oracle_mod, dtype):
    rng = np.random.RandomState(7)
    n = 60_000
    x = wide_column(rng, n, dtype)
    assert (swo.unsigned(x) >> np.uint64(16)).any()
    if np.dtype(dtype).kind == "i":
        assert (x < 0).any()
    lengths = rng.choice([0, 0, 1, 2, 3, 5, 100, 1000, 2047, 2048, 2049, 4097], 40)
    o = 13 + np.concatenate([[0], np.cumsum(lengths)])
    assert o[-1] + 9 <= n
    bits = 8 * np.dtype(dtype).itemsize
    for sup in (False, True):
        rows, high = swo.want(x, o, sup)
        assert rows.shape == (40, 32) and high.shape == (40,) and high.dtype == np.uint64
        for i in range(40):
            a = x[o[i]:o[i + 1]]
            lo = wide_filter_oracle.low16(a)
            w = oracle_mod.flagstat_hist(lo).copy()
            if sup:
                pp = ((lo & 0x100) == 0) & ((lo & 0x800) == 0) & ((lo & 1) == 1)
                fail = (lo & 0x200) != 0
                w[0], w[16], w[9] = int((pp & ~fail).sum()), int((pp & fail).sum()), a.size - int(fail.sum())
            assert np.array_equal(rows[i], w), (sup, i)
            m = 0
            for v in a.tolist():
                m |= (v & ((1 << bits) - 1)) & ~0xFFFF
            assert int(high[i]) == m, (i, hex(int(high[i])), hex(m))
    # one segment over the whole array: wide's mask
    assert int(swo.segmented_high(x, [0, n])[0]) == wide_filter_oracle.want_high(x)
    assert int(np.bitwise_or.reduce(swo.segmented_high(x, o))) == wide_filter_oracle.want_high(x[o[0]:o[-1]])
    # the periodic form against the materialised array
    pattern = x[:997]
    for phase in (0, 5):
        big = np.resize(np.roll(pattern, -phase), 3200)
        oo = np.array([0, 1, 996, 997, 998, 1994, 1994, 3100, 3200], dtype=np.int64)
        r1, h1 = swo.periodic_want(pattern, oo, True, phase)
        r2, h2 = swo.want(big, oo, True)
        assert np.array_equal(r1, r2) and np.array_equal(h1, h2), phase
    assert swo.want(x, [5])[0].shape == (0, 32) and swo.want(x, [5])[1].shape == (0,)


def test_writer_mirror_matches_the_sources_and_partitions_the_array():
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "libflagstats_amd", "csrc", "flagstat_segments_wide.hip")).read())
    hdr = open(os.path.join(ROOT, "libflagstats_amd", "csrc", "flagstat_segments_wide.h")).read()
    assert int(re.search(r"constexpr int kSegWideUnitBytes = (\d+);", hdr).group(1)) == swo.UNIT_BYTES
    assert (1 << int(re.search(r"constexpr int kSegWideDepth = (\d+);", src).group(1))) - 1 == swo.SEG_EPOCH
    # the launcher's shape and the kernel's walk are the segmented kernels' shared ones (flagstat_segments_shared.h), which this
    # unit instantiates for its unit of UE elements of 8192 / UE = W bytes
    shared = re.sub(r"\s+", " ", open(os.path.join(ROOT, "libflagstats_amd", "csrc", "flagstat_segments_shared.h")).read())
    for rule in ("constexpr uint64_t UE = kSegWideUnitBytes / W;",
                 "fsseg::launch_shape(addr, m, fsk::kSegWideUnitBytes / W, grid, &lo0, &nunits, &g);",
                 "seg_walk<UE>( lo0, hi0, base,",
                 "end_step<kSegWideDepth>(s, blk);"):
        assert rule in src, rule
    assert "constexpr int kSegUnitVecs = kSegWaveFlags / 8;" in shared and swo.UNIT_BYTES == 4096 // 8 * 16
    for rule in ("const uint64_t W = fsk::kSegUnitVecs * 16 / ue;",
                 "*lo0 = (addr & 15u) / W;",
                 "*nunits = (*lo0 + m + ue - 1) / ue;",
                 "const uint64_t want = (*nunits + 3) / 4;",
                 "*g = want < grid ? static_cast<uint32_t>(want) : grid;",
                 "const uint64_t u_begin = gw * nunits / waves, u_end = (gw + 1) * nunits / waves;",
                 "const uint64_t p0 = u_begin * UE > lo0 ? u_begin * UE : lo0;",
                 "const uint64_t E = u_end * UE < hi0 ? u_end * UE : hi0;",
                 "if (k >= min_units && k > 0) {",
                 "(mode & 1) && b_ >= p0 && e_ <= E"):
        assert shared.count(rule) == 1, rule
    rng = np.random.RandomState(31)
    for W in (4, 8):
        U = swo.UNIT_BYTES // W
        for addr in range(0, 16, W):
            for n, grid in ((1, 1), (U, 1), (U * 9 + 3, 2), (1 << 19, 7), (3_345_679, 3)):
                w = swo.writer_ranges(addr, n, grid, W)
                assert w.begin[0] == 0 and w.end[-1] == n and (w.begin[1:] == w.end[:-1]).all() and (w.end >= w.begin).all()
                assert w.grid == min(grid, (w.nunits + 3) // 4) and w.waves == 4 * w.grid
                cuts = np.sort(rng.randint(0, n + 1, 30))
                o = np.concatenate([[0], cuts, [n]])
                for mu in (0, 2, 255, 0xFFFFFFFF):
                    p = w.pieces(o, mu)
                    lengths = np.bincount(p["seg"], weights=p["e"] - p["b"], minlength=o.size - 1)
                    assert np.array_equal(lengths, np.diff(o)), (W, addr, n, grid)
                    assert np.array_equal(p["head"] + p["chain"] * U + p["tail"], p["e"] - p["b"])
                    assert (p["chain"] == 0).all() or mu != 0xFFFFFFFF


def test_no_gpu_means_the_entries_fail_loudly():
    """Without a GPU the three entries return non-zero with a message and leave `out` and `high` alone; nothing is computed on the
    CPU.  (With one, tests/test_gpu_segments_wide.py runs them.)"""
    import torch
    from libflagstats_amd import _lib
    lib = _lib.lib()
    o = np.array([0, 40, 100], dtype=np.uint64)
    out = np.full((2, 32), 7, dtype=np.uint64)
    high = np.full(2, 7, dtype=np.uint64)
    for dtype in (np.int32, np.int64):
        a = np.arange(100, dtype=dtype)
        W = a.dtype.itemsize
        # nseg == 0 does nothing and succeeds, GPU or not
        assert lib.FLAGSTATS_hip_wide_x64_segments(a.ctypes.data, a.size, W, o.ctypes.data, 0, out.ctypes.data, high.ctypes.data, 1) == 0
        assert lib.FLAGSTATS_hip_device_wide_segments(a.ctypes.data, a.size, W, o.ctypes.data, 0, out.ctypes.data, high.ctypes.data, 1, None) == 0
        assert (out == 7).all() and (high == 7).all()
        if torch.cuda.is_available():
            continue
        calls = [
            ("x64", lambda: lib.FLAGSTATS_hip_wide_x64_segments(a.ctypes.data, a.size, W, o.ctypes.data, 2, out.ctypes.data, high.ctypes.data, 1)),
            ("sync", lambda: lib.FLAGSTATS_hip_device_wide_segments_sync(a.ctypes.data, a.size, W, o.ctypes.data, 2, out.ctypes.data,
                                                                         high.ctypes.data, 1)),
            ("device", lambda: lib.FLAGSTATS_hip_device_wide_segments(a.ctypes.data, a.size, W, o.ctypes.data, 2, out.ctypes.data,
                                                                      high.ctypes.data, 0, None)),
        ]
        for name, call in calls:
            assert call() != 0, name
            assert lib.FLAGSTATS_hip_last_error(), name
            assert (out == 7).all() and (high == 7).all(), name
        with pytest.raises(_lib.FlagstatsHipError):
            sw.counters_segments_ints(a, o)
        with pytest.raises(_lib.FlagstatsHipError):
            sw.count_segments_device_ptr_ints(a.ctypes.data, a.size, W, o)
