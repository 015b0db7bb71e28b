"""The selected-elements segmented flagstat (libflagstats_amd/segments_where.py, csrc/flagstat_segments_where.hip) on the CPU: the
package's exports, every refusal of the Python layer -- raised before the library is loaded --, the symbols in the binding tables,
the built library and the headers, the identity of the code objects, the launcher's geometry against its mirror in
segments_where_oracle, and that oracle (zeroing) against a per-segment loop over the C oracle on the compacted values."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_where_oracle as swo  # noqa: E402
import where_oracle  # noqa: E402
from segments_where_oracle import BITMAP, BYTES  # noqa: E402

from libflagstats_amd import segments_where as sw  # noqa: E402  (fails at import where the feature is missing)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ("FLAGSTATS_hip_device_u16_segments_where", "FLAGSTATS_hip_device_u16_segments_where_sync",
          "FLAGSTATS_hip_u16_x64_segments_where")
INTERNAL = ("fsk_launch_segments_where", "fsk_segments_where_geometry")
PY_NAMES = ("counters_segments_where", "flagstats_segments_where", "count_segments_device_ptr_where", "count_segments_torch_where")


@pytest.fixture()
def no_library(monkeypatch):
    """loading the library fails the test: the refusals must come first"""
    from libflagstats_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were refused")

    monkeypatch.setattr(_lib, "lib", boom)


def test_exports():
    import libflagstats_amd
    for name in PY_NAMES:
        assert getattr(libflagstats_amd, name) is getattr(sw, name) and name in libflagstats_amd.__all__
    assert "segments_where" in libflagstats_amd.__doc__


def offsets_refusals(call, n):
    """segments.check_offsets' refusals; call(offsets) runs the entry over n flags"""
    for bad, text in ((np.zeros((2, 2), dtype=np.int64), r"offsets must be 1-D"),
                      (np.zeros(0, dtype=np.int64), r"offsets must hold nseg \+ 1 >= 1 values"),
                      (np.array([0.0, 1.0]), r"offsets must have an integer dtype, not float64"),
                      (np.array([-1, 2]), r"offsets must not be negative"),
                      (np.array([0, 5, 4, n]), r"offsets must be non-decreasing: offsets\[1\] = 5 > offsets\[2\] = 4"),
                      (np.array([0, n + 1]), r"offsets\[-1\] = %d exceeds the array's %d flags" % (n + 1, n))):
        with pytest.raises(ValueError, match=text):
            call(bad)


@pytest.mark.parametrize("fn", ["counters_segments_where", "flagstats_segments_where"])
def test_numpy_refusals(no_library, fn):
    f = getattr(sw, fn)
    v = np.zeros(20, dtype=np.uint16)
    m = np.zeros(20, dtype=bool)
    o = np.array([0, 7, 20])
    with pytest.raises(ValueError, match=r"values must be a numpy\.ndarray, not list"):
        f([1, 2, 3], o, m)
    for bad in (np.zeros(20, dtype=np.int16), np.zeros(20, dtype=np.int32), np.zeros(20, dtype=bool)):
        with pytest.raises(ValueError, match=r"values must have dtype uint16, not " + re.escape(str(bad.dtype))):
            f(bad, o, m)
    with pytest.raises(ValueError, match=r"values must be 1-D, not 2-D"):
        f(np.zeros((4, 5), dtype=np.uint16), o, m)
    with pytest.raises(ValueError, match=r"where must be a numpy\.ndarray, not list"):
        f(v, o, [True] * 20)
    with pytest.raises(ValueError, match=r"where must be 1-D, not 2-D"):
        f(v, o, np.zeros((4, 5), dtype=bool))
    for bad in (np.zeros(20, dtype=np.uint8), np.zeros(20, dtype=np.int64), np.zeros(20, dtype=np.float32)):
        with pytest.raises(ValueError, match=r"where must have dtype bool \(packed=True: a uint8 bitmap\), not " + re.escape(str(bad.dtype))):
            f(v, o, bad)
    for bad in (np.zeros(20, dtype=bool), np.zeros(20, dtype=np.int8)):
        with pytest.raises(ValueError, match=r"where must have dtype uint8 with packed=True \(an LSB-first bitmap\), not "
                                             + re.escape(str(bad.dtype))):
            f(v, o, bad, packed=True)
    for size in (0, 19, 21):
        with pytest.raises(ValueError, match=r"where must have one element per value \(20\), not %d" % size):
            f(v, o, np.zeros(size, dtype=bool))
    with pytest.raises(ValueError, match=r"where holds 2 bytes, 20 values from bit 0 on need 3"):
        f(v, o, np.zeros(2, dtype=np.uint8), packed=True)
    with pytest.raises(ValueError, match=r"where holds 3 bytes, 20 values from bit 5 on need 4"):
        f(v, o, np.zeros(3, dtype=np.uint8), packed=True, bit_offset=5)
    with pytest.raises(ValueError, match=r"bit_offset needs packed=True"):
        f(v, o, m, bit_offset=3)
    with pytest.raises(ValueError, match=r"bit_offset must not be negative"):
        f(v, o, np.zeros(3, dtype=np.uint8), packed=True, bit_offset=-1)
    for bad in (1.0, "1", None, True):
        with pytest.raises(ValueError, match=r"bit_offset must be an int, not"):
            f(v, o, np.zeros(3, dtype=np.uint8), packed=True, bit_offset=bad)
    offsets_refusals(lambda bad: f(v, bad, m), 20)
    offsets_refusals(lambda bad: f(v, bad, np.zeros(3, dtype=np.uint8), packed=True, bit_offset=2), 20)


def test_device_pointer_refusals(no_library):
    f = sw.count_segments_device_ptr_where
    o = np.array([0, 4, 10])
    for sb in (0, 2, 4, 16, "1", True):
        with pytest.raises(ValueError, match=r"sel_bits must be 1 \(an LSB-first bitmap\) or 8 \(one byte per element\), not"):
            f(0x1000, 10, o, 0x2000, sb)
    with pytest.raises(ValueError, match=r"n must not be negative"):
        f(0x1000, -1, o, 0x2000, 1)
    with pytest.raises(ValueError, match=r"sel_offset must not be negative"):
        f(0x1000, 1, o, 0x2000, 8, sel_offset=-1)
    for name, args, kw in (("ptr", (4096.0, 10, o, 0x2000, 1), {}), ("n", (0x1000, 10.0, o, 0x2000, 1), {}),
                           ("n", (0x1000, True, o, 0x2000, 1), {}), ("sel_ptr", (0x1000, 10, o, None, 8), {}),
                           ("sel_offset", (0x1000, 10, o, 0x2000, 8), {"sel_offset": 3.0})):
        with pytest.raises(ValueError, match=r"%s must be an int, not" % name):
            f(*args, **kw)
    for name, args, kw in (("ptr", (1 << 64, 10, o, 0x2000, 1), {}), ("ptr", (-8, 10, o, 0x2000, 1), {}), ("n", (0x1000, 1 << 64, o, 0x2000, 1), {}),
                           ("sel_ptr", (0x1000, 10, o, 1 << 64, 8), {}), ("sel_offset", (0x1000, 10, o, 0x2000, 8), {"sel_offset": 1 << 64})):
        with pytest.raises(ValueError, match=r"%s must fit an unsigned 64-bit integer, not" % name):
            f(*args, **kw)
    offsets_refusals(lambda bad: f(0x1000, 10, bad, 0x2000, 1, sel_offset=5), 10)


def test_torch_refusals(no_library):
    import torch
    f = sw.count_segments_torch_where
    t = torch.zeros(20, dtype=torch.int16)
    m = torch.zeros(20, dtype=torch.bool)
    o = torch.tensor([0, 7, 20], dtype=torch.int64)
    with pytest.raises(ValueError, match=r"t must be a torch\.Tensor, not ndarray"):
        f(np.zeros(20, dtype=np.uint16), o, m)
    for dt in (torch.int32, torch.int64, torch.uint8, torch.bool, torch.float16):
        with pytest.raises(ValueError, match=r"t must have dtype int16 or uint16, not " + re.escape(str(dt))):
            f(torch.zeros(20, dtype=dt), o, m)
    for bad in (torch.zeros((4, 5), dtype=torch.int16), torch.zeros(40, dtype=torch.int16)[::2]):
        with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
            f(bad, o, m)
    with pytest.raises(ValueError, match=r"where must be a torch\.Tensor, not ndarray"):
        f(t, o, np.zeros(20, dtype=bool))
    for bad in (torch.zeros((4, 5), dtype=torch.bool), torch.zeros(40, dtype=torch.bool)[::2]):
        with pytest.raises(ValueError, match=r"where must be 1-D and contiguous"):
            f(t, o, bad)
    for dt in (torch.uint8, torch.int8, torch.int64):
        with pytest.raises(ValueError, match=r"where must have dtype torch\.bool \(packed=True: a torch\.uint8 bitmap\), not " + re.escape(str(dt))):
            f(t, o, torch.zeros(20, dtype=dt))
    for dt in (torch.bool, torch.int8):
        with pytest.raises(ValueError, match=r"where must have dtype torch\.uint8 with packed=True \(an LSB-first bitmap\), not "
                                             + re.escape(str(dt))):
            f(t, o, torch.zeros(20, dtype=dt), packed=True)
    for size in (0, 19, 21):
        with pytest.raises(ValueError, match=r"where must have one element per value \(20\), not %d" % size):
            f(t, o, torch.zeros(size, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"where holds 2 bytes, 20 values from bit 0 on need 3"):
        f(t, o, torch.zeros(2, dtype=torch.uint8), packed=True)
    with pytest.raises(ValueError, match=r"where holds 3 bytes, 20 values from bit 7 on need 4"):
        f(t, o, torch.zeros(3, dtype=torch.uint8), packed=True, bit_offset=7)
    with pytest.raises(ValueError, match=r"bit_offset needs packed=True"):
        f(t, o, m, bit_offset=1)
    with pytest.raises(ValueError, match=r"bit_offset must not be negative"):
        f(t, o, torch.zeros(3, dtype=torch.uint8), packed=True, bit_offset=-8)
    for bad in (np.array([0, 20]), torch.tensor([0, 20], dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int64),
                torch.zeros(0, dtype=torch.int64), torch.zeros(6, dtype=torch.int64)[::2]):
        with pytest.raises(ValueError, match=r"offsets must be a 1-D contiguous int64 tensor \(nseg \+ 1 values\)"):
            f(t, bad, m)
    for bad in (torch.zeros((3, 32), dtype=torch.int64), torch.zeros((2, 32), dtype=torch.int32), torch.zeros(64, dtype=torch.int64),
                np.zeros((2, 32), dtype=np.int64)):
        with pytest.raises(ValueError, match=r"out must be a contiguous int64 tensor of shape \(2, 32\)"):
            f(t, o, m, out=bad)
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int64), 0):
        with pytest.raises(ValueError, match=r"selected must be a contiguous int64 tensor of shape \(2,\)"):
            f(t, o, m, selected=bad)
    with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
        f(t, o, m)
    with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
        f(t, o, torch.zeros(3, dtype=torch.uint8), packed=True, bit_offset=3)
    # (offsets / where / out / selected on another device than t: tests/test_gpu_segments_where.py::test_refusals)


def test_symbols_in_the_tables_the_library_and_the_headers():
    from libflagstats_amd import _lib
    for name in PUBLIC:
        assert name in _lib.SIGNATURES and name not in _lib.INTERNAL_SIGNATURES, name
    for name in INTERNAL:
        assert name in _lib.INTERNAL_SIGNATURES and name not in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_u16_segments_where"][1]) == 11
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_u16_segments_where_sync"][1]) == 10
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_u16_x64_segments_where"][1]) == 10
    assert len(_lib.INTERNAL_SIGNATURES["fsk_launch_segments_where"][1]) == 13
    assert len(_lib.INTERNAL_SIGNATURES["fsk_segments_where_geometry"][1]) == 6
    for name in PUBLIC:
        args = _lib.SIGNATURES[name][1]
        assert args[1] is ctypes.c_uint64 and args[3] is ctypes.c_uint64, name           # n, nseg
        assert args[5] is ctypes.c_uint64 and args[6] is ctypes.c_int, name              # sel_offset, sel_bits
    args = _lib.INTERNAL_SIGNATURES["fsk_launch_segments_where"][1]
    assert [args[i] for i in (2, 4, 5, 7)] == [ctypes.c_uint64] * 4 and args[3] is ctypes.c_int and args[11] is ctypes.c_uint32
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in PUBLIC + INTERNAL:
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    assert header.index("selected elements per segment:") > header.index("filtered segments:")
    assert "tests/test_gpu_segments_where.py: device_u16_segments_where" in header      # the sentence on graph capture
    for name in PUBLIC:
        m = re.search(r"\bint %s\(([^)]*)\)" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    csrc = os.path.join(ROOT, "libflagstats_amd", "csrc")
    for name in INTERNAL:
        declared = [h for h in sorted(os.listdir(csrc)) if h.endswith(".h") and re.search(r"\bhipError_t %s\(" % name, open(os.path.join(csrc, h)).read())]
        assert declared == ["flagstat_segments_where.h"] and name not in header, (name, declared)
        m = re.search(r"\bhipError_t %s\(([^)]*)\)" % name, open(os.path.join(csrc, declared[0])).read())
        assert len(m.group(1).split(",")) == len(_lib.INTERNAL_SIGNATURES[name][1]), name


def test_code_objects():
    """K1's code object is still the one profiles/traffic.json was measured on; exactly one gfx950 code object defines
    fsk::flagstat_segments_where, funnelled and not, and it is not K1's nor a parent's; the parents' kernels -- the segmented,
    the where and the filtered segmented kernel -- are still defined exactly once each"""
    from libflagstats_amd import _lib, kernel_id
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        recorded = json.load(f)["kernel_source_id"]
    assert kernel_id.kernel_id(_lib.LIB_PATH) == recorded
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    found = {k: [] for k in ("k1", "segments", "where", "segments_filter", "segments_where")}
    for i, co in enumerate(kernel_id._code_objects(so)):
        secs = kernel_id._sections(co)
        names = b"".join(co[secs[t][0]:secs[t][0] + secs[t][1]] for t in (".strtab", ".dynstr") if t in secs)
        for key, prefix in (("k1", b"_ZN3fsk14flagstat_count"), ("segments", b"_ZN3fsk17flagstat_segmentsE"),
                            ("where", b"_ZN3fsk20flagstat_count_where"), ("segments_filter", b"_ZN3fsk24flagstat_segments_filter")):
            if prefix in names:
                found[key].append(i)
        if b"_ZN3fsk23flagstat_segments_whereILb0" in names:
            assert b"_ZN3fsk23flagstat_segments_whereILb1" in names
            found["segments_where"].append(i)
        else:
            assert b"_ZN3fsk23flagstat_segments_where" not in names
    assert all(len(v) == 1 for v in found.values()), found
    assert len({v[0] for v in found.values()}) == len(found), found


# ------------------------------------------------------------------ geometry
def geometry():
    from libflagstats_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    f = lib.fsk_segments_where_geometry
    f.restype, f.argtypes = _lib.INTERNAL_SIGNATURES["fsk_segments_where_geometry"]
    return f


SIZES = (1, 7, 8, 9, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193)
BIT_OFFSETS = list(range(8)) + [8, 13, 8 * 4099 + 5, (1 << 40) + 3]
BYTE_OFFSETS = list(range(16)) + [4099, 1 << 40]


def test_geometry_equals_the_mirror():
    """fsk_segments_where_geometry (the arithmetic fsk_launch_segments_where launches with; host code, no GPU) against
    segments_where_oracle: every array phase x every bit offset (bitmap) and byte alignment (bytes) x sizes around a vector, a row
    and one and two units x grids 1, 3 and 256; geo[5 .. 7) is exactly the set of selection bytes that hold an element's bit or
    byte, and bit geo[4] of byte j of the base geo[3] is the bit of grid position 8 j"""
    f = geometry()
    geo = (ctypes.c_uint64 * 7)()
    for n in SIZES:
        for phase in range(8):
            addr = 0x7F00_0000_1000 + 2 * phase
            for sel_bits, offsets in ((BITMAP, BIT_OFFSETS), (BYTES, BYTE_OFFSETS)):
                for off in offsets:
                    for grid in (1, 3, 256):
                        assert f(addr, n, off, sel_bits, grid, geo) == 0
                        assert list(geo) == swo.segments_where_geometry(addr, n, off, sel_bits, grid), (n, phase, sel_bits, off, grid)
                    lo0, adjust, shift = geo[0], geo[3] - (1 << 64) if geo[3] >> 63 else geo[3], geo[4]
                    assert lo0 == phase
                    # element 0 sits at grid position lo0: the kernel's address of its bit or byte is the caller's
                    if sel_bits == BITMAP:
                        assert 8 * adjust + shift + lo0 == off and 0 <= shift < 8
                    else:
                        assert adjust + lo0 == off and shift == 0
                    if off < 1 << 30:
                        held = swo.selection_bytes(n, off, sel_bits)
                        assert np.array_equal(held, np.arange(geo[5], geo[6], dtype=np.uint64)), (n, sel_bits, off)


def test_geometry_refusals():
    f = geometry()
    geo = (ctypes.c_uint64 * 7)(*([7] * 7))
    for sel_bits in (BITMAP, BYTES):
        assert f(0x1000, 0, 5, sel_bits, 4, geo) == 0 and list(geo) == [0] * 7       # m == 0: all zeros
        assert f(0x1001, 10, 0, sel_bits, 4, geo) != 0                                # an odd address
        assert f(0x1000, 10, 0, sel_bits, 0, geo) != 0                                # no workgroups
        assert f(0x1000, 10, (1 << 64) - 5, sel_bits, 4, geo) != 0                    # sel_offset + m is no index
        assert f(0x1000, 1 << 63, 0, sel_bits, 4, geo) != 0                           # m * 2 is no size
        assert f(0x1000, 10, (1 << 63) + 1, sel_bits, 4, geo) == 0                    # any uint64 offset that is one
        assert geo[5] == ((1 << 63) + 1 >> 3 if sel_bits == BITMAP else (1 << 63) + 1)
        # a wave's totals are uint32: grid 1 over 2^35 flags is refused, the same array on 256 workgroups is not
        assert f(0x1000, 1 << 35, 0, sel_bits, 1, geo) != 0
        assert f(0x1000, 1 << 35, 0, sel_bits, 256, geo) == 0
        n_ok = ((1 << 32) // 4096 - 1) * 4 * 4096 - 8
        assert f(0x1000, n_ok, 0, sel_bits, 1, geo) == 0 and (geo[1] + 3) // 4 * 4096 < 1 << 32
        assert f(0x1000, n_ok + 4 * 4096, 0, sel_bits, 1, geo) != 0
    for sel_bits in (0, 2, 4, 16, -1):
        assert f(0x1000, 10, 0, sel_bits, 4, geo) != 0
    assert f(0x1000, 10, 0, BITMAP, 4, None) != 0


# ------------------------------------------------------------------ the oracle against a per-segment loop
LAYOUTS = {
    "whole": [0, 1000],
    "gaps and empties": [3, 3, 40, 40, 41, 500, 500, 997],
    "short": list(range(0, 1001, 7)) + [1000],
    "one flag each": list(range(100, 164)),
    "nothing": [17],
}


def test_oracle_against_a_per_segment_loop(oracle_mod):
    """segments_where_oracle.want (zeroing the unselected flags) and .periodic_want on 1,000 values against
    where_oracle.want_counters (the C oracle on the COMPACTED values[b:e][mask[b:e]]) segment by segment: several layouts and mask
    densities, with and without the superset slots"""
    rng = np.random.RandomState(11)
    v = rng.randint(0, 65536, 1000).astype(np.uint16)
    v[200:230] = 0
    any_selected = False
    for density in (0, 3, 50, 97, 100):
        mask = rng.randint(0, 100, 1000) < density
        for name, o in LAYOUTS.items():
            o = np.array(o, dtype=np.int64)
            for superset in (False, True):
                rows, selected = swo.want(v, o, mask, superset)
                assert rows.dtype == np.uint64 and rows.shape == (o.size - 1, 32) and selected.dtype == np.uint64
                for i in range(o.size - 1):
                    b, e = int(o[i]), int(o[i + 1])
                    w = where_oracle.want_counters(oracle_mod, v[b:e], mask[b:e], superset)
                    assert np.array_equal(rows[i], w), (name, density, superset, i, rows[i], w)
                    assert int(selected[i]) == int(mask[b:e].sum())
                any_selected |= bool(selected.any())
                if density == 0:
                    assert not rows.any() and not selected.any()
        # the periodic form: periods 997 (flags) and 13 (mask), both shifted, against the materialised array
        pattern, mask_pattern = v[:997], mask[:13]
        for phase, mask_phase in ((0, 0), (5, 11)):
            big = np.resize(np.roll(pattern, -phase), 40_000)
            big_m = np.resize(np.roll(mask_pattern, -mask_phase), 40_000)
            oo = np.array([0, 1, 996, 997, 998, 12961, 12961, 12962, 39_000, 40_000], dtype=np.int64)
            got = swo.periodic_want(pattern, oo, mask_pattern, True, phase, mask_phase)
            ref = swo.want(big, oo, big_m, True)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (density, phase, mask_phase)
    assert any_selected
