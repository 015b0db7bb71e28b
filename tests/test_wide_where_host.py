"""The selected-elements flagstat of int32 / int64 columns (libflagstats_amd/wide_where.py, csrc/flagstat_wide_where.hip) on the
CPU: the package's exports, every refusal of the Python layer -- raised before the library is loaded --, the symbols in the
binding tables, the built library and the headers, the identity of the code objects, the launcher's geometry against
wide_where_oracle, and a model of the selection addresses the kernel's fast path forms: none outside the bytes that hold an
element's bit or byte, and the bits extracted from them are the mask."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_where_oracle as wwo  # noqa: E402
from wide_where_oracle import BITMAP, BYTES, pack, selection_bytes, step_elems, wide_where_geometry  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ("FLAGSTATS_hip_device_wide_where", "FLAGSTATS_hip_device_wide_where_sync", "FLAGSTATS_hip_wide_x64_where")
INTERNAL = ("fsk_launch_wide_where", "fsk_wide_where_geometry")
PY_NAMES = ("counters_ints_where", "flagstats_ints_where", "count_device_ptr_ints_where", "count_torch_ints_where")
INT_DTYPES = ("int16", "uint16", "int32", "uint32", "int64", "uint64")
BIT_OFFSETS = list(range(8)) + [8, 13, 8 * 4099 + 5, (1 << 40) + 3]
BYTE_OFFSETS = list(range(16)) + [4099, 1 << 40]


@pytest.fixture()
def no_library(monkeypatch):
    """loading the library fails the test: the refusals must come first"""
    from libflagstats_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were refused")

    monkeypatch.setattr(_lib, "lib", boom)


def test_exports():
    import libflagstats_amd
    from libflagstats_amd import wide_where
    for name in PY_NAMES:
        assert getattr(libflagstats_amd, name) is getattr(wide_where, name) and name in libflagstats_amd.__all__


@pytest.mark.parametrize("fn", ["counters_ints_where", "flagstats_ints_where"])
def test_numpy_refusals(no_library, fn):
    from libflagstats_amd import wide_where
    f = getattr(wide_where, fn)
    m = np.zeros(20, dtype=bool)
    # the value checks are wide.py's
    with pytest.raises(ValueError, match=r"values must be a numpy\.ndarray, not list"):
        f([1, 2, 3], m)
    for bad in (np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.float64), np.zeros(4, dtype=bool),
                np.array([1, 2], dtype=object), np.zeros(4, dtype=np.int8), np.zeros(4, dtype=np.uint8),
                np.zeros(4, dtype="S2"), np.zeros(4, dtype=np.complex64)):
        with pytest.raises(ValueError, match=r"values must have an integer dtype of 2, 4 or 8 bytes \(int16, uint16, int32, "
                                             r"uint32, int64, uint64\), not " + re.escape(str(bad.dtype))):
            f(bad, m)
    with pytest.raises(ValueError, match=r"native \(little-endian\) byte order"):
        f(np.zeros(4, dtype=">i4"), m)
    for dt in INT_DTYPES:
        v = np.zeros(20, dtype=dt)
        with pytest.raises(ValueError, match=r"values must be 1-D, not 2-D"):
            f(np.zeros((2, 3), dtype=dt), m)
        with pytest.raises(ValueError, match=r"values must be 1-D, not 0-D"):
            f(np.array(5, dtype=dt), m)
        # the selection checks are where.py's
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
    from libflagstats_amd import wide_where
    f = wide_where.count_device_ptr_ints_where
    for eb in (2, 3, 16, 0, "4"):
        with pytest.raises(ValueError, match=r"elem_bytes must be 4 or 8 \(16-bit arrays: where\.count_device_ptr_where\), not"):
            f(0x1000, 10, eb, 0x2000, 1)
    for W in (4, 8):
        for sb in (0, 2, 4, 16, "1", True):
            with pytest.raises(ValueError, match=r"sel_bits must be 1 \(an LSB-first bitmap\) or 8 \(one byte per element\), not"):
                f(0x1000, 10, W, 0x2000, sb)
        with pytest.raises(ValueError, match=r"n must not be negative"):
            f(0x1000, -1, W, 0x2000, 1)
        with pytest.raises(ValueError, match=r"sel_offset must not be negative"):
            f(0x1000, 1, W, 0x2000, 8, sel_offset=-1)
        for name, args, kw in (("ptr", (4096.0, 10, W, 0x2000, 1), {}), ("n", (0x1000, 10.0, W, 0x2000, 1), {}),
                               ("n", (0x1000, "10", W, 0x2000, 1), {}), ("n", (0x1000, True, W, 0x2000, 1), {}),
                               ("sel_ptr", (0x1000, 10, W, None, 8), {}), ("sel_offset", (0x1000, 10, W, 0x2000, 8), {"sel_offset": 3.0})):
            with pytest.raises(ValueError, match=r"%s must be an int, not" % name):
                f(*args, **kw)
        for name, args, kw in (("ptr", (1 << 64, 10, W, 0x2000, 1), {}), ("ptr", (-8, 10, W, 0x2000, 1), {}),
                               ("n", (0x1000, 1 << 64, W, 0x2000, 1), {}), ("sel_ptr", (0x1000, 10, W, 1 << 64, 8), {}),
                               ("sel_offset", (0x1000, 10, W, 0x2000, 8), {"sel_offset": 1 << 64})):
            with pytest.raises(ValueError, match=r"%s must fit an unsigned 64-bit integer, not" % name):
                f(*args, **kw)


def test_torch_refusals(no_library):
    import torch
    from libflagstats_amd import wide_where
    f = wide_where.count_torch_ints_where
    m = torch.zeros(20, dtype=torch.bool)
    with pytest.raises(ValueError, match=r"t must be a torch\.Tensor, not ndarray"):
        f(np.zeros(4, dtype=np.int32), m)
    for dt in (torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.bool, torch.int8, torch.uint8, torch.complex64):
        with pytest.raises(ValueError, match=r"t must have an integer dtype of 2, 4 or 8 bytes, not " + re.escape(str(dt))):
            f(torch.zeros(4, dtype=dt), m)
    for dt in (torch.int16, torch.int32, torch.int64):
        t = torch.zeros(20, dtype=dt)
        for bad in (torch.zeros((2, 3), dtype=dt), torch.zeros(8, dtype=dt)[::2], torch.zeros((), dtype=dt)):
            with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
                f(bad, m)
        with pytest.raises(ValueError, match=r"where must be a torch\.Tensor, not ndarray"):
            f(t, np.zeros(20, dtype=bool))
        for bad in (torch.zeros((4, 5), dtype=torch.bool), torch.zeros(40, dtype=torch.bool)[::2]):
            with pytest.raises(ValueError, match=r"where must be 1-D and contiguous"):
                f(t, bad)
        for wdt in (torch.uint8, torch.int8, torch.int64, torch.float32):
            with pytest.raises(ValueError, match=r"where must have dtype torch\.bool \(packed=True: a torch\.uint8 bitmap\), not "
                                                 + re.escape(str(wdt))):
                f(t, torch.zeros(20, dtype=wdt))
        for wdt in (torch.bool, torch.int8, torch.int16):
            with pytest.raises(ValueError, match=r"where must have dtype torch\.uint8 with packed=True \(an LSB-first bitmap\), not "
                                                 + re.escape(str(wdt))):
                f(t, torch.zeros(20, dtype=wdt), packed=True)
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
        for name in ("selected", "high"):
            for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 0):
                with pytest.raises(ValueError, match=r"%s must be a contiguous int64 tensor of 1 element$" % name):
                    f(t, m, **{name: bad})
        with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
            f(t, m)                                   # host tensors
        with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
            f(t, torch.zeros(3, dtype=torch.uint8), packed=True, out=torch.zeros(32, dtype=torch.int64),
              selected=torch.zeros(1, dtype=torch.int64), high=torch.zeros(1, dtype=torch.int64))
    # (where / out / selected / high on another device than t: tests/test_gpu_wide_where.py::test_python_layers)


def test_the_checks_are_shared_not_copied():
    """wide_where.py holds no refusal text of wide.py's or where.py's: it calls their functions"""
    src = open(os.path.join(ROOT, "libflagstats_amd", "wide_where.py")).read()
    for text in ("must be a numpy.ndarray", "integer dtype of 2, 4 or 8 bytes", "byte order", "must be 1-D", "one element per value",
                 "must have dtype", "needs packed=True", "sel_bits must be", "values outside 0..65535", "must be a torch.Tensor",
                 "must be a CUDA tensor"):
        assert text not in src, text
    for call in ("_wide._check_values(", "_wide._check_tensor(", "_wide.high_bits_message(", "_where._check_selection_numpy(",
                 "_where._check_selection_torch(", "_where._check_sel_bits("):
        assert call in src, call


def test_symbols_in_the_tables_the_library_and_the_headers():
    from libflagstats_amd import _lib
    for name in PUBLIC:
        assert name in _lib.SIGNATURES and name not in _lib.INTERNAL_SIGNATURES, name
    for name in INTERNAL:
        assert name in _lib.INTERNAL_SIGNATURES and name not in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_wide_where"][1]) == 11
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_wide_where_sync"][1]) == 10
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_wide_x64_where"][1]) == 10
    assert len(_lib.INTERNAL_SIGNATURES["fsk_launch_wide_where"][1]) == 12
    assert len(_lib.INTERNAL_SIGNATURES["fsk_wide_where_geometry"][1]) == 7
    for name in PUBLIC + INTERNAL[:1]:
        args = (_lib.SIGNATURES if name in PUBLIC else _lib.INTERNAL_SIGNATURES)[name][1]
        assert args[1] is ctypes.c_uint64 and args[2] is ctypes.c_int, name                            # n, elem_bytes
        assert args[3] is ctypes.c_void_p and args[4] is ctypes.c_uint64 and args[5] is ctypes.c_int, name   # sel, sel_offset, sel_bits
        assert args[6:9] == [ctypes.c_void_p] * 3 and args[9] is ctypes.c_int, name                    # out, selected, high, flags
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in PUBLIC + INTERNAL:
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    for name in PUBLIC:
        m = re.search(r"\bint %s\(([^)]*)\)" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    internal = open(os.path.join(ROOT, "libflagstats_amd", "csrc", "flagstat_wide_where.h")).read()
    for name in INTERNAL:
        m = re.search(r"\bhipError_t %s\(([^)]*)\)" % name, internal)
        assert m and name not in header, name
        assert len(m.group(1).split(",")) == len(_lib.INTERNAL_SIGNATURES[name][1]), name
    # both say whose bits `high` holds
    assert "SELECTED elements ONLY" in header and "SELECTED elements only" in internal


def test_code_objects():
    """K1's code object is still the one profiles/traffic.json was measured on; exactly one gfx950 code object defines
    fsk::flagstat_count_wide_where, it holds all six instantiations (W 4 and 8; bitmap plain and funnelled, bytes), and it is
    not the code object of K1, wide, where or wide_filter"""
    from libflagstats_amd import _lib, kernel_id
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        recorded = json.load(f)["kernel_source_id"]
    assert kernel_id.kernel_id(_lib.LIB_PATH) == recorded
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    others = {"k1": b"_ZN3fsk14flagstat_count", "wide": b"_ZN3fsk19flagstat_count_wide", "where": b"_ZN3fsk20flagstat_count_where",
              "wide_filter": b"_ZN3fsk26flagstat_count_wide_filter"}
    new = [b"_ZN3fsk25flagstat_count_wide_whereILi%dELi%dELb%dE" % (W, bits, funnel)
           for W in (4, 8) for bits, funnel in ((1, 0), (1, 1), (8, 0))]
    found = {k: [] for k in others}
    mine = []
    for i, co in enumerate(kernel_id._code_objects(so)):
        secs = kernel_id._sections(co)
        names = b"".join(co[secs[t][0]:secs[t][0] + secs[t][1]] for t in (".strtab", ".dynstr") if t in secs)
        for k, prefix in others.items():
            if prefix in names:
                found[k].append(i)
        if b"flagstat_count_wide_where" in names:
            assert all(n in names for n in new), i
            mine.append(i)
    assert all(len(v) == 1 for v in found.values()), found
    assert len(mine) == 1 and all(mine[0] != v[0] for v in found.values()), (mine, found)


def geometry():
    from libflagstats_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    f = lib.fsk_wide_where_geometry
    f.restype, f.argtypes = _lib.INTERNAL_SIGNATURES["fsk_wide_where_geometry"]
    return f


def sizes(W):
    S = step_elems(W)
    return (1, 2, 3, 4, 5, 7, 8, 9, S - 1, S, S + 1, 2 * S, 2 * S + 1)   # 2 S: the last fast vector ends the array


def cases():
    """(W, n, address, phase) over every size and array phase"""
    for W in (4, 8):
        for n in sizes(W):
            for phase in range(16 // W):
                yield W, n, 0x7F00_0000_1000 + W * phase, phase


def test_geometry_equals_the_mirror():
    """fsk_wide_where_geometry (the arithmetic fsk_launch_wide_where launches with; host code, no GPU) against wide_where_oracle:
    every array phase x bit offset (bitmap) and byte offset (bytes) x the sizes around a vector and one and two steps; geo[6 .. 8)
    is exactly the set of selection bytes that hold an element's bit or byte, enumerated element by element"""
    f = geometry()
    geo = (ctypes.c_uint64 * 8)()
    for W, n, addr, phase in cases():
        for sel_bits, offsets in ((BITMAP, BIT_OFFSETS), (BYTES, BYTE_OFFSETS)):
            for off in offsets:
                for grid in (1, 3, 256):
                    assert f(addr, n, W, off, sel_bits, grid, geo) == 0
                    assert list(geo) == wide_where_geometry(addr, n, W, off, sel_bits, grid), (W, n, phase, sel_bits, off, grid)
                if off < 1 << 30:
                    held = selection_bytes(n, off, sel_bits)
                    assert np.array_equal(held, np.arange(geo[6], geo[7], dtype=np.uint64)), (W, n, sel_bits, off)


def test_geometry_refusals():
    f = geometry()
    geo = (ctypes.c_uint64 * 8)(*([7] * 8))
    for W in (4, 8):
        for sel_bits in (BITMAP, BYTES):
            assert f(0x1000, 0, W, 5, sel_bits, 4, geo) == 0 and list(geo) == [0] * 8      # n == 0: all zeros
            assert f(0x1000 + W // 2, 10, W, 0, sel_bits, 4, geo) != 0                     # a misaligned address
            assert f(0x1000, 10, W, 0, sel_bits, 0, geo) != 0                              # no workgroups
            assert f(0x1000, 10, W, (1 << 64) - 5, sel_bits, 4, geo) != 0                  # sel_offset + n is no index
            assert f(0x1000, 10, W, (1 << 63) + 1, sel_bits, 4, geo) == 0                  # any uint64 offset that is one
            assert geo[6] == ((1 << 63) + 1 >> 3 if sel_bits == BITMAP else (1 << 63) + 1)
            # a wave's totals are uint32: grid 1 over 2^35 elements is refused, the same array on 256 workgroups is not
            assert f(0x1000, 1 << 35, W, 0, sel_bits, 1, geo) != 0
            assert f(0x1000, 1 << 35, W, 0, sel_bits, 256, geo) == 0
            wave_elems = step_elems(W) // 4
            n_ok = ((1 << 32) // wave_elems - 4) * step_elems(W)
            assert f(0x1000, n_ok, W, 0, sel_bits, 1, geo) == 0 and (geo[2] + 2) * wave_elems < 1 << 32
        for sel_bits in (0, 2, 4, 16, -1):
            assert f(0x1000, 10, W, 0, sel_bits, 4, geo) != 0
    for W in (0, 1, 2, 3, 16, -4):
        assert f(0x1000, 10, W, 0, BITMAP, 4, geo) != 0


def test_selection_addresses_of_the_fast_path():
    """The guard against an over-read of the selection: a model of the addresses the kernel's fast path forms -- a lane's byte
    index, its shift and which two adjacent bytes it loads when its bits may straddle (its own and the next one, or the one in
    front and its own), derived from the launcher's own geometry as the kernel derives them -- forms no address outside
    geo[6 .. 8), and the bits it extracts from a random bitmap are the mask.  (4 bits at a shift of at most 4 lie in one byte:
    a blind pair [k, k + 1] would lie one byte past the bitmap where the last fast vector ends the array, a blind [k - 1, k] one
    byte in front of it where the first fast vector begins it.)"""
    f = geometry()
    geo = (ctypes.c_uint64 * 8)()
    rng = np.random.RandomState(11)
    checked = straddling = funnelled_without_straddle = 0
    for W, n, addr, phase in cases():
        EPV = 16 // W
        mask = rng.randint(0, 2, n).astype(bool)
        for off in BIT_OFFSETS:
            assert f(addr, n, W, off, BITMAP, 3, geo) == 0
            g = list(geo)
            j, first, d, sh, funnel = wwo.fast_path_bitmap_model(g, W, off)
            if j.size == 0:
                continue
            last = first + 1 if funnel else first          # the funnelled form loads two adjacent bytes, the plain form one
            assert (first >= g[6]).all() and (last < g[7]).all(), (W, n, phase, off)
            if not funnel:
                assert not d.any()
            else:
                assert j.min() >= wwo.VPS                  # step 0 is never a fast step of a funnelled launch
            assert (sh + EPV <= (16 if funnel else 8)).all()   # the bits lie inside what was loaded
            straddling += int(d.sum())
            funnelled_without_straddle += int(funnel and (d == 0).any())
            if off < 1 << 30:
                sel = pack(mask, off)
                assert sel.size == g[7]
                w = sel[first].astype(np.uint32) | (sel[last].astype(np.uint32) << 8 if funnel else 0)
                bits = (w >> sh.astype(np.uint32)) & ((1 << EPV) - 1)
                lo = g[0]
                for e in range(EPV):
                    assert np.array_equal((bits >> e) & 1, mask[j * EPV + e - lo].astype(np.uint32)), (W, n, phase, off, e)
                checked += 1
        for off in BYTE_OFFSETS:
            assert f(addr, n, W, off, BYTES, 3, geo) == 0
            g = list(geo)
            j, first, count = wwo.fast_path_bytes_model(g, W, off)
            if j.size == 0:
                continue
            assert (first >= g[6]).all() and (first + count <= g[7]).all(), (W, n, phase, off)
            assert np.array_equal(first - off, j * EPV - g[0])      # byte e of vector j is element j * EPV + e - lo
    assert checked and straddling and funnelled_without_straddle


def test_oracle_on_hand_made_columns(oracle_mod):
    """wide_where_oracle.want: counters, count and `high` all see the selected elements only"""
    for dt, top in (("int32", 31), ("uint32", 31), ("int64", 63), ("uint64", 63)):
        U = wwo.UNSIGNED[np.dtype(dt).itemsize]
        v = np.array([0x0041, 0x0004 | (1 << 16), 0x0041 | (1 << 20), 0x0905, 0x0001 | (1 << top)], dtype=U).view(dt)
        c, selected, high = wwo.want(oracle_mod, v, np.array([1, 0, 1, 0, 0], dtype=bool))
        assert selected == 2 and high == 1 << 20
        assert np.array_equal(c, oracle_mod.flagstat_c(np.array([0x0041, 0x0041], dtype=np.uint16)).astype(np.uint64))
        c, selected, high = wwo.want(oracle_mod, v, np.zeros(5, dtype=bool))
        assert selected == 0 and high == 0 and not c.any()
        c, selected, high = wwo.want(oracle_mod, v, np.ones(5, dtype=bool))
        assert selected == 5 and high == (1 << 16) | (1 << 20) | (1 << top)
        c, selected, high = wwo.want(oracle_mod, v[:0], np.zeros(0, dtype=bool))
        assert selected == 0 and high == 0 and not c.any()
        p = np.full(3, wwo.poison(v.dtype.itemsize)).view(dt)
        assert wwo.low16(p).tolist() == [0xFFFF] * 3 and wwo.want(oracle_mod, p, np.ones(3, dtype=bool))[2] == (1 << (top + 1)) - (1 << 16)
