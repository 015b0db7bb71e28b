"""The selected-elements flagstat (libflagstats_amd/where.py, csrc/flagstat_where.hip) on the CPU: the package's exports, every
refusal of the Python layer -- raised before the library is loaded --, the symbols in the binding tables, the built library and
the headers, the identity of K1's code object, and the launcher's geometry against where_oracle."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from where_oracle import BITMAP, BYTES, pack, selection_bytes, where_geometry  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ("FLAGSTATS_hip_device_u16_where", "FLAGSTATS_hip_device_u16_where_sync", "FLAGSTATS_hip_u16_x64_where")
INTERNAL = ("fsk_launch_where", "fsk_where_geometry")
PY_NAMES = ("counters_where", "flagstats_where", "count_device_ptr_where", "count_torch_where")


@pytest.fixture()
def no_library(monkeypatch):
    """loading the library fails the test: the refusals must come first"""
    from libflagstats_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were refused")

    monkeypatch.setattr(_lib, "lib", boom)


def test_exports():
    import libflagstats_amd
    from libflagstats_amd import where
    for name in PY_NAMES:
        assert getattr(libflagstats_amd, name) is getattr(where, name) and name in libflagstats_amd.__all__


@pytest.mark.parametrize("fn", ["counters_where", "flagstats_where"])
def test_numpy_refusals(no_library, fn):
    from libflagstats_amd import where
    f = getattr(where, fn)
    v = np.zeros(20, dtype=np.uint16)
    m = np.zeros(20, dtype=bool)
    with pytest.raises(ValueError, match=r"values must be a numpy\.ndarray, not list"):
        f([1, 2, 3], m)
    for bad in (np.zeros(20, dtype=np.int16), np.zeros(20, dtype=np.int32), np.zeros(20, dtype=np.uint8),
                np.zeros(20, dtype=np.float32), np.zeros(20, dtype=bool), np.zeros(20, dtype=">u2")):
        with pytest.raises(ValueError, match=r"values must have dtype uint16, not " + re.escape(str(bad.dtype))):
            f(bad, m)
    with pytest.raises(ValueError, match=r"values must be 1-D, not 2-D"):
        f(np.zeros((4, 5), dtype=np.uint16), m)
    with pytest.raises(ValueError, match=r"values must be 1-D, not 0-D"):
        f(np.array(5, dtype=np.uint16), m)
    with pytest.raises(ValueError, match=r"where must be a numpy\.ndarray, not list"):
        f(v, [True] * 20)
    with pytest.raises(ValueError, match=r"where must be 1-D, not 2-D"):
        f(v, np.zeros((4, 5), dtype=bool))
    for bad in (np.zeros(20, dtype=np.uint8), np.zeros(20, dtype=np.int8), np.zeros(20, dtype=np.int64), np.zeros(20, dtype=np.float32)):
        with pytest.raises(ValueError, match=r"where must have dtype bool \(packed=True: a uint8 bitmap\), not " + re.escape(str(bad.dtype))):
            f(v, bad)
    for bad in (np.zeros(20, dtype=bool), np.zeros(20, dtype=np.int8), np.zeros(20, dtype=np.uint16)):
        with pytest.raises(ValueError, match=r"where must have dtype uint8 with packed=True \(an LSB-first bitmap\), not "
                                             + re.escape(str(bad.dtype))):
            f(v, bad, packed=True)
    for size in (0, 19, 21):
        with pytest.raises(ValueError, match=r"where must have one element per value \(20\), not %d" % size):
            f(v, np.zeros(size, dtype=bool))
    with pytest.raises(ValueError, match=r"where holds 2 bytes, 20 values from bit 0 on need 3"):
        f(v, np.zeros(2, dtype=np.uint8), packed=True)
    with pytest.raises(ValueError, match=r"where holds 3 bytes, 20 values from bit 5 on need 4"):
        f(v, np.zeros(3, dtype=np.uint8), packed=True, bit_offset=5)
    with pytest.raises(ValueError, match=r"bit_offset needs packed=True"):
        f(v, m, bit_offset=3)
    with pytest.raises(ValueError, match=r"bit_offset must not be negative"):
        f(v, np.zeros(3, dtype=np.uint8), packed=True, bit_offset=-1)
    for bad in (1.0, "1", None, True):
        with pytest.raises(ValueError, match=r"bit_offset must be an int, not"):
            f(v, np.zeros(3, dtype=np.uint8), packed=True, bit_offset=bad)


def test_device_pointer_refusals(no_library):
    from libflagstats_amd import where
    for sb in (0, 2, 4, 16, "1", True):
        with pytest.raises(ValueError, match=r"sel_bits must be 1 \(an LSB-first bitmap\) or 8 \(one byte per element\), not"):
            where.count_device_ptr_where(0x1000, 10, 0x2000, sb)
    with pytest.raises(ValueError, match=r"n must not be negative"):
        where.count_device_ptr_where(0x1000, -1, 0x2000, 1)
    with pytest.raises(ValueError, match=r"sel_offset must not be negative"):
        where.count_device_ptr_where(0x1000, 1, 0x2000, 8, sel_offset=-1)
    for name, args, kw in (("ptr", (4096.0, 10, 0x2000, 1), {}), ("n", (0x1000, 10.0, 0x2000, 1), {}), ("n", (0x1000, "10", 0x2000, 1), {}),
                           ("n", (0x1000, True, 0x2000, 1), {}), ("sel_ptr", (0x1000, 10, None, 8), {}),
                           ("sel_offset", (0x1000, 10, 0x2000, 8), {"sel_offset": 3.0})):
        with pytest.raises(ValueError, match=r"%s must be an int, not" % name):
            where.count_device_ptr_where(*args, **kw)
    for name, args, kw in (("ptr", (1 << 64, 10, 0x2000, 1), {}), ("ptr", (-8, 10, 0x2000, 1), {}), ("n", (0x1000, 1 << 64, 0x2000, 1), {}),
                           ("sel_ptr", (0x1000, 10, 1 << 64, 8), {}), ("sel_offset", (0x1000, 10, 0x2000, 8), {"sel_offset": 1 << 64})):
        with pytest.raises(ValueError, match=r"%s must fit an unsigned 64-bit integer, not" % name):
            where.count_device_ptr_where(*args, **kw)


def test_torch_refusals(no_library):
    import torch
    from libflagstats_amd import where
    f = where.count_torch_where
    t = torch.zeros(20, dtype=torch.int16)
    m = torch.zeros(20, dtype=torch.bool)
    with pytest.raises(ValueError, match=r"t must be a torch\.Tensor, not ndarray"):
        f(np.zeros(20, dtype=np.uint16), m)
    for dt in (torch.int32, torch.int64, torch.uint8, torch.int8, torch.bool, torch.float16, torch.float32):
        with pytest.raises(ValueError, match=r"t must have dtype int16 or uint16, not " + re.escape(str(dt))):
            f(torch.zeros(20, dtype=dt), m)
    for bad in (torch.zeros((4, 5), dtype=torch.int16), torch.zeros(40, dtype=torch.int16)[::2], torch.zeros((), dtype=torch.int16)):
        with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
            f(bad, m)
    with pytest.raises(ValueError, match=r"where must be a torch\.Tensor, not ndarray"):
        f(t, np.zeros(20, dtype=bool))
    for bad in (torch.zeros((4, 5), dtype=torch.bool), torch.zeros(40, dtype=torch.bool)[::2]):
        with pytest.raises(ValueError, match=r"where must be 1-D and contiguous"):
            f(t, bad)
    for dt in (torch.uint8, torch.int8, torch.int64, torch.float32):
        with pytest.raises(ValueError, match=r"where must have dtype torch\.bool \(packed=True: a torch\.uint8 bitmap\), not "
                                             + re.escape(str(dt))):
            f(t, torch.zeros(20, dtype=dt))
    for dt in (torch.bool, torch.int8, torch.int16):
        with pytest.raises(ValueError, match=r"where must have dtype torch\.uint8 with packed=True \(an LSB-first bitmap\), not "
                                             + re.escape(str(dt))):
            f(t, torch.zeros(20, dtype=dt), packed=True)
    for size in (0, 19, 21):
        with pytest.raises(ValueError, match=r"where must have one element per value \(20\), not %d" % size):
            f(t, torch.zeros(size, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"where holds 2 bytes, 20 values from bit 0 on need 3"):
        f(t, torch.zeros(2, dtype=torch.uint8), packed=True)
    with pytest.raises(ValueError, match=r"where holds 3 bytes, 20 values from bit 7 on need 4"):
        f(t, torch.zeros(3, dtype=torch.uint8), packed=True, bit_offset=7)
    with pytest.raises(ValueError, match=r"bit_offset needs packed=True"):
        f(t, m, bit_offset=1)
    with pytest.raises(ValueError, match=r"bit_offset must not be negative"):
        f(t, torch.zeros(3, dtype=torch.uint8), packed=True, bit_offset=-8)
    for bad in (torch.zeros(31, dtype=torch.int64), torch.zeros(32, dtype=torch.int32), torch.zeros(64, dtype=torch.int64)[::2],
                np.zeros(32, dtype=np.int64)):
        with pytest.raises(ValueError, match=r"out must be a contiguous int64 tensor of 32 elements"):
            f(t, m, out=bad)
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 0):
        with pytest.raises(ValueError, match=r"selected must be a contiguous int64 tensor of 1 element$"):
            f(t, m, selected=bad)
    with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
        f(t, m)                                   # host tensors
    with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
        f(t, torch.zeros(3, dtype=torch.uint8), packed=True, out=torch.zeros(32, dtype=torch.int64))
    # (where / out / selected on another device than t: tests/test_gpu_where.py::test_device_dependent_refusals)


def test_symbols_in_the_tables_the_library_and_the_headers():
    from libflagstats_amd import _lib
    for name in PUBLIC:
        assert name in _lib.SIGNATURES and name not in _lib.INTERNAL_SIGNATURES, name
    for name in INTERNAL:
        assert name in _lib.INTERNAL_SIGNATURES and name not in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_u16_where"][1]) == 9
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_u16_where_sync"][1]) == 8
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_u16_x64_where"][1]) == 8
    assert len(_lib.INTERNAL_SIGNATURES["fsk_launch_where"][1]) == 10
    assert len(_lib.INTERNAL_SIGNATURES["fsk_where_geometry"][1]) == 6
    for name in PUBLIC + INTERNAL[:1]:
        table = _lib.SIGNATURES if name in PUBLIC else _lib.INTERNAL_SIGNATURES
        assert table[name][1][3] is ctypes.c_uint64 and table[name][1][4] is ctypes.c_int, name    # sel_offset, sel_bits
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in PUBLIC + INTERNAL:
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    for name in PUBLIC:
        assert re.search(r"\bint %s\(" % name, header), name
    internal = open(os.path.join(ROOT, "libflagstats_amd", "csrc", "flagstat_where.h")).read()
    for name in INTERNAL:
        assert re.search(r"\bhipError_t %s\(" % name, internal) and name not in header, name


def test_code_objects():
    """K1's code object is still the one profiles/traffic.json was measured on; exactly one gfx950 code object defines
    fsk::flagstat_count_where, in both encodings, and it is neither K1's nor the wide kernel's"""
    from libflagstats_amd import _lib, kernel_id
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        recorded = json.load(f)["kernel_source_id"]
    assert kernel_id.kernel_id(_lib.LIB_PATH) == recorded
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    k1, wide, where = [], [], []
    for i, co in enumerate(kernel_id._code_objects(so)):
        secs = kernel_id._sections(co)
        names = b"".join(co[secs[t][0]:secs[t][0] + secs[t][1]] for t in (".strtab", ".dynstr") if t in secs)
        if b"_ZN3fsk14flagstat_count" in names:
            k1.append(i)
        if b"_ZN3fsk19flagstat_count_wideILi4" in names:
            wide.append(i)
        if b"_ZN3fsk20flagstat_count_whereILi1" in names:
            assert b"_ZN3fsk20flagstat_count_whereILi8" in names
            where.append(i)
        else:
            assert b"_ZN3fsk20flagstat_count_where" not in names
    assert len(k1) == 1 and len(wide) == 1 and len(where) == 1, (k1, wide, where)
    assert where[0] not in (k1[0], wide[0]), (k1, wide, where)


def test_oracle_helpers():
    """where_oracle.pack against numpy, and the unused bits"""
    rng = np.random.RandomState(3)
    for n in (1, 7, 8, 9, 100):
        m = rng.randint(0, 2, n).astype(bool)
        for off in range(8):
            for fill in (0, 1):
                p = pack(m, off, fill)
                bits = np.unpackbits(p, bitorder="little").astype(bool)
                assert p.size == (off + n + 7) // 8 and np.array_equal(bits[off:off + n], m)
                assert (bits[:off] == bool(fill)).all() and (bits[off + n:] == bool(fill)).all()
    assert np.array_equal(pack(np.array([1, 0, 0, 0, 0, 0, 0, 0, 1], dtype=bool), 0, 0), np.array([1, 1], dtype=np.uint8))


def geometry():
    from libflagstats_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    f = lib.fsk_where_geometry
    f.restype, f.argtypes = _lib.INTERNAL_SIGNATURES["fsk_where_geometry"]
    return f


SIZES = (1, 7, 8, 9, 16383, 16384, 16385, 32769)


def test_geometry_equals_the_mirror():
    """fsk_where_geometry (the arithmetic fsk_launch_where launches with; host code, no GPU) against where_oracle: every array
    phase x bit offset (bitmap) and byte alignment (bytes) x the sizes around a vector and one and two steps; geo[6 .. 8) is
    exactly the range of selection bytes that hold an element's bit or byte"""
    f = geometry()
    geo = (ctypes.c_uint64 * 8)()
    for n in SIZES:
        for phase in range(8):
            addr = 0x7F00_0000_1000 + 2 * phase
            for sel_bits, offsets in ((BITMAP, list(range(8)) + [8, 13, 8 * 4099 + 5, (1 << 40) + 3]), (BYTES, list(range(16)) + [4099, 1 << 40])):
                for off in offsets:
                    for grid in (1, 3, 256):
                        assert f(addr, n, off, sel_bits, grid, geo) == 0
                        assert list(geo) == where_geometry(addr, n, off, sel_bits, grid), (n, phase, sel_bits, off, grid)
                    if off < 1 << 30:
                        held = selection_bytes(n, off, sel_bits)
                        assert np.array_equal(held, np.arange(geo[6], geo[7], dtype=np.uint64)), (n, sel_bits, off)


def test_geometry_refusals():
    f = geometry()
    geo = (ctypes.c_uint64 * 8)(*([7] * 8))
    for sel_bits in (BITMAP, BYTES):
        assert f(0x1000, 0, 5, sel_bits, 4, geo) == 0 and list(geo) == [0] * 8       # n == 0: all zeros
        assert f(0x1001, 10, 0, sel_bits, 4, geo) != 0                                # an odd address
        assert f(0x1000, 10, 0, sel_bits, 0, geo) != 0                                # no workgroups
        assert f(0x1000, 10, (1 << 64) - 5, sel_bits, 4, geo) != 0                    # sel_offset + n is no index
        assert f(0x1000, 10, (1 << 63) + 1, sel_bits, 4, geo) == 0                    # any uint64 offset that is one
        assert geo[6] == ((1 << 63) + 1 >> 3 if sel_bits == BITMAP else (1 << 63) + 1)
        # a wave's totals are uint32: grid 1 over 2^35 flags is refused, the same array on 256 workgroups is not
        assert f(0x1000, 1 << 35, 0, sel_bits, 1, geo) != 0
        assert f(0x1000, 1 << 35, 0, sel_bits, 256, geo) == 0
        n_ok = ((1 << 32) // 4096 - 4) * 16384
        assert f(0x1000, n_ok, 0, sel_bits, 1, geo) == 0 and (geo[2] + 2) * 4096 < 1 << 32
    for sel_bits in (0, 2, 4, 16, -1):
        assert f(0x1000, 10, 0, sel_bits, 4, geo) != 0
