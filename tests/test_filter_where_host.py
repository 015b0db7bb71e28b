"""The filtered flagstat under a selection (libflagstats_amd/filter_where.py, csrc/flagstat_filter_where.hip) on the CPU: the
package's exports, every refusal of the Python layer -- raised before the library is loaded --, the symbols in the binding
tables, the built library and the headers, the identity of the code objects, and filter_where_oracle's combined mask against a
per-element loop."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from filter_where_oracle import combined_mask  # noqa: E402
from where_oracle import pack  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ("FLAGSTATS_hip_device_u16_filter_where", "FLAGSTATS_hip_device_u16_filter_where_sync", "FLAGSTATS_hip_u16_x64_filter_where")
INTERNAL = ("fsk_launch_filter_where",)
PY_NAMES = ("counters_filter_where", "flagstats_filter_where", "count_device_ptr_filter_where", "count_torch_filter_where")
KERNEL = b"_ZN3fsk21flagstat_filter_where"
FORMS = tuple(b"ILb%dELi%dELb%dE" % (mapq, bits, funnel) for mapq in (0, 1) for bits, funnel in ((1, 0), (1, 1), (8, 0)))


@pytest.fixture()
def no_library(monkeypatch):
    """loading the library fails the test: the refusals must come first"""
    from libflagstats_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were refused")

    monkeypatch.setattr(_lib, "lib", boom)


def test_exports():
    import libflagstats_amd
    from libflagstats_amd import filter_where as fw
    for name in PY_NAMES:
        assert getattr(libflagstats_amd, name) is getattr(fw, name) and name in libflagstats_amd.__all__


def predicate_refusals(call):
    """the filtered entries' refusals, in their texts; call(**kw) runs the entry with a MAPQ column and a selection at hand"""
    for name in ("require", "exclude"):
        for bad in (1.0, "4", None, True, np.float32(2)):
            with pytest.raises(ValueError, match=r"%s must be an int, not" % name):
                call(**{name: bad})
        for bad in (-1, 65536, 1 << 32):
            with pytest.raises(ValueError, match=r"%s must be a 16-bit FLAG mask \(0\.\.65535\), not %d" % (name, bad)):
                call(**{name: bad})
    for bad in (1.0, "30", None, True):
        with pytest.raises(ValueError, match=r"min_mapq must be an int, not"):
            call(min_mapq=bad)
    for bad in (-1, 256, 1000):
        with pytest.raises(ValueError, match=r"min_mapq must be in 0\.\.255 \(MAPQ is one byte\), not %d" % bad):
            call(min_mapq=bad)


def bit_offset_refusals(call):
    """the `where` entries' refusals of bit_offset; call(**kw) runs the entry with a bitmap at hand when packed=True"""
    for bad in (1.0, "3", None, True):
        with pytest.raises(ValueError, match=r"bit_offset must be an int, not"):
            call(packed=True, bit_offset=bad)
    for bad in (-1, 1 << 63):
        with pytest.raises(ValueError, match=r"bit_offset must not be negative \(and below 2\*\*63\), not %d" % bad):
            call(packed=True, bit_offset=bad)
    with pytest.raises(ValueError, match=r"bit_offset needs packed=True"):
        call(packed=False, bit_offset=3)


@pytest.mark.parametrize("fn", ["counters_filter_where", "flagstats_filter_where"])
def test_numpy_refusals(no_library, fn):
    from libflagstats_amd import filter_where as fw
    f = getattr(fw, fn)
    v = np.zeros(20, dtype=np.uint16)
    q = np.zeros(20, dtype=np.uint8)
    m = np.ones(20, dtype=bool)
    bits = np.zeros(4, dtype=np.uint8)
    with pytest.raises(ValueError, match=r"values must be a numpy\.ndarray, not list"):
        f([1, 2, 3], m)
    for bad in (np.zeros(20, dtype=np.int16), np.zeros(20, dtype=np.int32), np.zeros(20, dtype=np.uint8),
                np.zeros(20, dtype=np.float32), np.zeros(20, dtype=bool), np.zeros(20, dtype=">u2")):
        with pytest.raises(ValueError, match=r"values must have dtype uint16, not " + re.escape(str(bad.dtype))):
            f(bad, m)
    with pytest.raises(ValueError, match=r"values must be 1-D, not 2-D"):
        f(np.zeros((4, 5), dtype=np.uint16), m)
    # the selection
    with pytest.raises(ValueError, match=r"where must be a numpy\.ndarray, not list"):
        f(v, [True] * 20)
    with pytest.raises(ValueError, match=r"where must be a numpy\.ndarray, not NoneType"):
        f(v, None)
    with pytest.raises(ValueError, match=r"where must be 1-D, not 2-D"):
        f(v, np.ones((4, 5), dtype=bool))
    for bad in (np.ones(20, dtype=np.uint8), np.ones(20, dtype=np.int8), np.ones(20, dtype=np.float32)):
        with pytest.raises(ValueError, match=r"where must have dtype bool \(packed=True: a uint8 bitmap\), not " + re.escape(str(bad.dtype))):
            f(v, bad)
    for size in (0, 19, 21):
        with pytest.raises(ValueError, match=r"where must have one element per value \(20\), not %d" % size):
            f(v, np.ones(size, dtype=bool))
    for bad in (np.ones(4, dtype=bool), np.ones(4, dtype=np.int8), np.ones(4, dtype=np.uint16)):
        with pytest.raises(ValueError, match=r"where must have dtype uint8 with packed=True \(an LSB-first bitmap\), not " + re.escape(str(bad.dtype))):
            f(v, bad, packed=True)
    with pytest.raises(ValueError, match=r"where holds 2 bytes, 20 values from bit 0 on need 3"):
        f(v, np.zeros(2, dtype=np.uint8), packed=True)
    with pytest.raises(ValueError, match=r"where holds 3 bytes, 20 values from bit 5 on need 4"):
        f(v, np.zeros(3, dtype=np.uint8), packed=True, bit_offset=5)
    bit_offset_refusals(lambda packed, **kw: f(v, bits if packed else m, packed=packed, **kw))
    # the column
    with pytest.raises(ValueError, match=r"mapq must be a numpy\.ndarray, not list"):
        f(v, m, mapq=[0] * 20, min_mapq=1)
    for bad in (np.zeros(20, dtype=np.int8), np.zeros(20, dtype=bool), np.zeros(20, dtype=np.uint16), np.zeros(20, dtype=np.float32)):
        with pytest.raises(ValueError, match=r"mapq must have dtype uint8, not " + re.escape(str(bad.dtype))):
            f(v, m, mapq=bad, min_mapq=1)
    with pytest.raises(ValueError, match=r"mapq must be 1-D, not 2-D"):
        f(v, m, mapq=np.zeros((4, 5), dtype=np.uint8), min_mapq=1)
    for size in (0, 19, 21):
        with pytest.raises(ValueError, match=r"mapq must have one element per value \(20\), not %d" % size):
            f(v, m, mapq=np.zeros(size, dtype=np.uint8))
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
        f(v, m, min_mapq=30)
    predicate_refusals(lambda **kw: f(v, m, mapq=q, **kw))
    predicate_refusals(lambda **kw: f(v, bits, mapq=q, packed=True, bit_offset=7, **kw))


def test_device_pointer_refusals(no_library):
    from libflagstats_amd import filter_where as fw
    f = fw.count_device_ptr_filter_where
    for bad in (0, 2, 16, True, None, "1"):
        with pytest.raises(ValueError, match=r"sel_bits must be 1 \(an LSB-first bitmap\) or 8 \(one byte per element\), not"):
            f(0x1000, 10, 0x3000, bad)
    with pytest.raises(ValueError, match=r"n must not be negative"):
        f(0x1000, -1, 0x3000, 1)
    with pytest.raises(ValueError, match=r"sel_offset must not be negative"):
        f(0x1000, 10, 0x3000, 1, sel_offset=-1)
    for name, args, kw in (("ptr", (4096.0, 10, 0x3000, 8), {}), ("n", (0x1000, 10.0, 0x3000, 8), {}), ("n", (0x1000, True, 0x3000, 8), {}),
                           ("sel_ptr", (0x1000, 10, None, 8), {}), ("sel_ptr", (0x1000, 10, 12288.0, 1), {}),
                           ("sel_offset", (0x1000, 10, 0x3000, 1), {"sel_offset": 1.0}),
                           ("mapq_ptr", (0x1000, 10, 0x3000, 8), {"mapq_ptr": None}), ("mapq_ptr", (0x1000, 10, 0x3000, 8), {"mapq_ptr": 8192.0})):
        with pytest.raises(ValueError, match=r"%s must be an int, not" % name):
            f(*args, **kw)
    for name, args, kw in (("ptr", (1 << 64, 10, 0x3000, 8), {}), ("ptr", (-8, 10, 0x3000, 8), {}), ("n", (0x1000, 1 << 64, 0x3000, 8), {}),
                           ("sel_ptr", (0x1000, 10, 1 << 64, 1), {}), ("sel_offset", (0x1000, 10, 0x3000, 1), {"sel_offset": 1 << 64}),
                           ("mapq_ptr", (0x1000, 10, 0x3000, 8), {"mapq_ptr": 1 << 64})):
        with pytest.raises(ValueError, match=r"%s must fit an unsigned 64-bit integer, not" % name):
            f(*args, **kw)
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
        f(0x1000, 10, 0x3000, 1, min_mapq=1)
    for sel_bits in (1, 8):
        predicate_refusals(lambda **kw: f(0x1000, 10, 0x3000, sel_bits, mapq_ptr=0x2000, **kw))


def test_torch_refusals(no_library):
    import torch
    from libflagstats_amd import filter_where as fw
    f = fw.count_torch_filter_where
    t = torch.zeros(20, dtype=torch.int16)
    q = torch.zeros(20, dtype=torch.uint8)
    m = torch.ones(20, dtype=torch.bool)
    bits = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"t must be a torch\.Tensor, not ndarray"):
        f(np.zeros(20, dtype=np.uint16), m)
    for dt in (torch.int32, torch.int64, torch.uint8, torch.int8, torch.bool, torch.float16, torch.float32):
        with pytest.raises(ValueError, match=r"t must have dtype int16 or uint16, not " + re.escape(str(dt))):
            f(torch.zeros(20, dtype=dt), m)
    for bad in (torch.zeros((4, 5), dtype=torch.int16), torch.zeros(40, dtype=torch.int16)[::2], torch.zeros((), dtype=torch.int16)):
        with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
            f(bad, m)
    # the selection
    with pytest.raises(ValueError, match=r"where must be a torch\.Tensor, not ndarray"):
        f(t, np.ones(20, dtype=bool))
    with pytest.raises(ValueError, match=r"where must be a torch\.Tensor, not NoneType"):
        f(t, None)
    for bad in (torch.ones((4, 5), dtype=torch.bool), torch.ones(40, dtype=torch.bool)[::2]):
        with pytest.raises(ValueError, match=r"where must be 1-D and contiguous"):
            f(t, bad)
    for dt in (torch.uint8, torch.int8, torch.int64, torch.float32):
        with pytest.raises(ValueError, match=r"where must have dtype torch\.bool \(packed=True: a torch\.uint8 bitmap\), not " + re.escape(str(dt))):
            f(t, torch.ones(20, dtype=dt))
    for size in (0, 19, 21):
        with pytest.raises(ValueError, match=r"where must have one element per value \(20\), not %d" % size):
            f(t, torch.ones(size, dtype=torch.bool))
    for dt in (torch.bool, torch.int8, torch.int16):
        with pytest.raises(ValueError, match=r"where must have dtype torch\.uint8 with packed=True \(an LSB-first bitmap\), not " + re.escape(str(dt))):
            f(t, torch.ones(4, dtype=dt), packed=True)
    with pytest.raises(ValueError, match=r"where holds 3 bytes, 20 values from bit 5 on need 4"):
        f(t, torch.zeros(3, dtype=torch.uint8), packed=True, bit_offset=5)
    bit_offset_refusals(lambda packed, **kw: f(t, bits if packed else m, packed=packed, **kw))
    # the column
    with pytest.raises(ValueError, match=r"mapq must be a torch\.Tensor, not ndarray"):
        f(t, m, mapq=np.zeros(20, dtype=np.uint8), min_mapq=1)
    for dt in (torch.int8, torch.bool, torch.int16, torch.int64, torch.float32):
        with pytest.raises(ValueError, match=r"mapq must have dtype torch\.uint8, not " + re.escape(str(dt))):
            f(t, m, mapq=torch.zeros(20, dtype=dt), min_mapq=1)
    for bad in (torch.zeros((4, 5), dtype=torch.uint8), torch.zeros(40, dtype=torch.uint8)[::2]):
        with pytest.raises(ValueError, match=r"mapq must be 1-D and contiguous"):
            f(t, m, mapq=bad, min_mapq=1)
    for size in (0, 19, 21):
        with pytest.raises(ValueError, match=r"mapq must have one element per value \(20\), not %d" % size):
            f(t, m, mapq=torch.zeros(size, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
        f(t, m, min_mapq=30)
    predicate_refusals(lambda **kw: f(t, m, mapq=q, **kw))
    predicate_refusals(lambda **kw: f(t, bits, mapq=q, packed=True, bit_offset=3, **kw))
    # the result pair
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
        f(t, bits, require=2, exclude=0x904, mapq=q, min_mapq=30, packed=True, bit_offset=1, out=torch.zeros(32, dtype=torch.int64))
    # (where / mapq / out / selected on another device than t: tests/test_gpu_filter_where.py)


def test_symbols_in_the_tables_the_library_and_the_headers():
    from libflagstats_amd import _lib
    for name in PUBLIC:
        assert name in _lib.SIGNATURES and name not in _lib.INTERNAL_SIGNATURES, name
    for name in INTERNAL:
        assert name in _lib.INTERNAL_SIGNATURES and name not in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_u16_filter_where"][1]) == 13
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_u16_filter_where_sync"][1]) == 12
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_u16_x64_filter_where"][1]) == 12
    assert len(_lib.INTERNAL_SIGNATURES["fsk_launch_filter_where"][1]) == 14
    for name in PUBLIC + INTERNAL:
        table = _lib.SIGNATURES if name in PUBLIC else _lib.INTERNAL_SIGNATURES
        restype, args = table[name]
        assert restype is ctypes.c_int, name
        assert args[1] is ctypes.c_uint64 and args[4] is ctypes.c_void_p, name                                  # n, mapq
        assert args[2] is ctypes.c_uint32 and args[3] is ctypes.c_uint32 and args[5] is ctypes.c_uint32, name   # require, exclude, min_mapq
        assert args[6] is ctypes.c_void_p and args[7] is ctypes.c_uint64 and args[8] is ctypes.c_int, name      # sel, sel_offset, sel_bits
        assert args[0] is ctypes.c_void_p and args[9] is ctypes.c_void_p and args[10] is ctypes.c_void_p and args[11] is ctypes.c_int, name
    assert _lib.SIGNATURES["FLAGSTATS_hip_device_u16_filter_where"][1][12] is ctypes.c_void_p                   # stream
    assert _lib.INTERNAL_SIGNATURES["fsk_launch_filter_where"][1][12:] == [ctypes.c_uint32, ctypes.c_void_p]     # grid, stream
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in PUBLIC + INTERNAL:
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    for name in PUBLIC:
        m = re.search(r"\bint %s\(([^)]*)\)" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    internal = open(os.path.join(ROOT, "libflagstats_amd", "csrc", "flagstat_filter_where.h")).read()
    for name in INTERNAL:
        m = re.search(r"\bhipError_t %s\(([^)]*)\)" % name, internal)
        assert m and name not in header, name
        assert len(m.group(1).split(",")) == len(_lib.INTERNAL_SIGNATURES[name][1]), name


def test_code_objects():
    """K1's code object is still the one profiles/traffic.json was measured on; exactly one gfx950 code object defines
    fsk::flagstat_filter_where, in all six instantiations (MAPQ x {bitmap, bitmap funnelled, bytes}), and it is not K1's, the
    wide kernel's, the where kernel's or the filtered kernel's"""
    from libflagstats_amd import _lib, kernel_id
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        recorded = json.load(f)["kernel_source_id"]
    assert kernel_id.kernel_id(_lib.LIB_PATH) == recorded
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    k1, wide, where, flt, both = [], [], [], [], []
    for i, co in enumerate(kernel_id._code_objects(so)):
        secs = kernel_id._sections(co)
        names = b"".join(co[secs[t][0]:secs[t][0] + secs[t][1]] for t in (".strtab", ".dynstr") if t in secs)
        if b"_ZN3fsk14flagstat_count" in names:
            k1.append(i)
        if b"_ZN3fsk19flagstat_count_wide" in names:
            wide.append(i)
        if b"_ZN3fsk20flagstat_count_where" in names:
            where.append(i)
        if b"_ZN3fsk21flagstat_count_filter" in names:
            flt.append(i)
        if KERNEL in names:
            for form in FORMS:
                assert KERNEL + form in names, form
            assert len(set(re.findall(re.escape(KERNEL) + rb"ILb[01]ELi[0-9]+ELb[01]E", names))) == 6
            both.append(i)
    assert len(k1) == 1 and len(wide) == 1 and len(where) == 1 and len(flt) == 1 and len(both) == 1, (k1, wide, where, flt, both)
    assert both[0] not in (k1[0], wide[0], where[0], flt[0]), (k1, wide, where, flt, both)


def test_oracle_mask_against_a_loop():
    """filter_where_oracle.combined_mask, element by element in plain Python, on 1,000 values: the mask read back out of a bitmap
    at an odd bit offset and out of bytes with several non-zero values, predicates on one and both byte planes, an overlapping
    pair, thresholds on both sides of 128"""
    rng = np.random.RandomState(11)
    v = rng.randint(0, 65536, 1000).astype(np.uint16)
    v[:64] &= np.uint16(0x00FF)                   # some values that pass predicates with many excluded bits
    v[64:128] = 0
    q = rng.randint(0, 256, 1000).astype(np.uint8)
    q[:8] = (0, 1, 29, 30, 127, 128, 129, 255)
    mask = rng.randint(0, 2, 1000).astype(bool)
    bitmap = pack(mask, 13, fill=1)
    as_bytes = mask.astype(np.uint8) * np.resize(np.array([1, 2, 0x80, 0xFF], dtype=np.uint8), 1000)
    any_overlap = False
    for require, exclude in ((0, 0), (0, 0x904), (0x2, 0x904), (0x0101, 0x8080), (0x40, 0x40), (0xFFFF, 0), (0, 0xFFFF)):
        for min_mapq in (0, 1, 30, 127, 128, 129, 255):
            want = []
            for i in range(1000):
                x, m = int(v[i]), int(q[i])
                sel_bit = (int(bitmap[(13 + i) >> 3]) >> ((13 + i) & 7)) & 1
                assert bool(sel_bit) == (int(as_bytes[i]) != 0)
                want.append((x & require) == require and (x & exclude) == 0 and (min_mapq == 0 or m >= min_mapq) and sel_bit == 1)
            got = combined_mask(v, mask, require, exclude, q, min_mapq)
            assert got.dtype == np.bool_ and got.tolist() == want, (require, exclude, min_mapq)
            assert not (got & ~mask).any()
            if require & exclude:
                any_overlap = True
                assert not got.any()
    assert any_overlap
    assert np.array_equal(combined_mask(v, mask, 0, 0), mask)
    assert 0 < combined_mask(v, mask, 0, 0x904, q, 30).sum() < mask.sum()
    assert not combined_mask(v, np.zeros(1000, dtype=bool), 0, 0).any()
