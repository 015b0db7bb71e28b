"""The selected-elements segmented flagstat of int32 / int64 columns (libflagstats_amd/segments_wide_where.py,
csrc/flagstat_segments_wide_where.hip) on the CPU: the package's exports, the symbols in the binding tables, the built library
and the headers, the identity of the code objects, every refusal of the Python layers -- raised before the library is loaded --
and of the C entries before the GPU is touched, the launcher's geometry against segments_wide_where_oracle, a model of every
selection address the kernel's unguarded paths form (none outside the bytes that hold an element's bit or byte, and the bits
extracted from them are the mask), the kernel's own copy of the walk against the shared one rule by rule, and the oracle against
compaction."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_wide_where_oracle as swwo  # noqa: E402
from segments_wide_where_oracle import BITMAP, BYTES, pack, segments_wide_where_geometry, unit_elems  # noqa: E402
from where_oracle import selection_bytes  # noqa: E402

from libflagstats_amd import segments_wide_where as sww  # noqa: E402  (fails at import where the feature is missing)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libflagstats_amd", "csrc")
PUBLIC = {"FLAGSTATS_hip_device_wide_segments_where": 13, "FLAGSTATS_hip_device_wide_segments_where_sync": 12,
          "FLAGSTATS_hip_wide_x64_segments_where": 12}
INTERNAL = {"fsk_launch_segments_wide_where": 15, "fsk_segments_wide_where_geometry": 7}
PY_NAMES = ("counters_segments_ints_where", "flagstats_segments_ints_where", "count_segments_device_ptr_ints_where",
            "count_segments_torch_ints_where")
DTYPES = (np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64)
BIT_OFFSETS = list(range(8)) + [8, 13, 8 * 4099 + 5, (1 << 40) + 3]
BYTE_OFFSETS = list(range(8)) + [4099, 1 << 40]


@pytest.fixture()
def no_library(monkeypatch):
    """loading the library fails the test: the refusals must come first"""
    from libflagstats_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were refused")

    monkeypatch.setattr(_lib, "lib", boom)


def test_exports_and_shared_checks():
    import libflagstats_amd
    from libflagstats_amd import segments, segments_filter, segments_where, segments_wide, where, wide
    for name in PY_NAMES:
        assert getattr(libflagstats_amd, name) is getattr(sww, name) and name in libflagstats_amd.__all__
    assert len(set(libflagstats_amd.__all__)) == len(libflagstats_amd.__all__)
    assert "segments_wide_where" in libflagstats_amd.__doc__
    # the checks and the shaping are the other modules', not restated
    assert sww.check_offsets is segments.check_offsets and sww._check_values is wide._check_values
    assert sww._check_tensor is wide._check_tensor and sww.strict_message is segments_wide.strict_message
    assert sww._check_selection_numpy is where._check_selection_numpy and sww._check_selection_torch is where._check_selection_torch
    assert sww._check_sel_bits is where._check_sel_bits and sww.segment_filter_dicts is segments_filter.segment_filter_dicts
    assert sww.count_segments_torch_where is segments_where.count_segments_torch_where
    assert sww.counters_segments_where is segments_where.counters_segments_where
    src = open(os.path.join(ROOT, "libflagstats_amd", "segments_wide_where.py")).read()
    for text in ("must be a numpy.ndarray", "integer dtype of 2, 4 or 8 bytes", "byte order", "must be 1-D, not", "must have one element per value",
                 "must have dtype", "needs packed=True", "sel_bits must be", "values outside 0..65535", "must be a torch.Tensor",
                 "non-decreasing"):
        assert text not in src, text


def test_symbols_in_the_tables_the_library_and_the_headers():
    from libflagstats_amd import _lib
    for name, nargs in PUBLIC.items():
        assert name in _lib.SIGNATURES and name not in _lib.INTERNAL_SIGNATURES, name
        args = _lib.SIGNATURES[name][1]
        assert len(args) == nargs and _lib.SIGNATURES[name][0] is ctypes.c_int, name
        # n, elem_bytes, nseg, sel_offset, sel_bits, flags
        assert args[1] is ctypes.c_uint64 and args[2] is ctypes.c_int and args[4] is ctypes.c_uint64, name
        assert args[6] is ctypes.c_uint64 and args[7] is ctypes.c_int and args[11] is ctypes.c_int, name
        assert args[8:11] == [ctypes.c_void_p] * 3, name
    for name, nargs in INTERNAL.items():
        assert name in _lib.INTERNAL_SIGNATURES and name not in _lib.SIGNATURES, name
        assert len(_lib.INTERNAL_SIGNATURES[name][1]) == nargs, name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in tuple(PUBLIC) + tuple(INTERNAL):
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    section = header[header.index("selected elements of wide input per segment:"):]
    for name, nargs in PUBLIC.items():
        m = re.search(r"\bint %s\(([^)]*)\)" % name, section)
        assert m and len(m.group(1).split(",")) == nargs, name
    # both headers say whose bits `high` holds
    assert "SELECTED elements ONLY" in section[:section.index("int FLAGSTATS_hip_device_wide_segments_where(")]
    # the internal declarations live in the new internal header and nowhere else
    for fn in sorted(os.listdir(CSRC)) + [os.path.join(ROOT, "include", "libflagstats_hip.h"),
                                          os.path.join(ROOT, "include", "libflagstats_hip_probe.h")]:
        if not fn.endswith(".h"):
            continue
        text = open(os.path.join(CSRC, fn)).read()
        for name, nargs in INTERNAL.items():
            m = re.search(r"\bhipError_t %s\(([^)]*)\)" % name, text)
            if os.path.basename(fn) == "flagstat_segments_wide_where.h":
                assert m and len(m.group(1).split(",")) == nargs, name
                assert "SELECTED" in text and "ONLY" in text
            else:
                assert name not in text, (fn, name)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1)
    hdrs = re.search(r"^HDRS\s*:=(.*)$", mk, re.M).group(1)
    assert "$(HERE)flagstat_segments_wide_where.hip" in srcs.split()
    for h in ("flagstat_segments_wide_where.h", "flagstat_wide_where_device.h"):
        assert "$(HERE)" + h in hdrs.split(), h


def test_code_objects():
    """K1's code object is still the one profiles/traffic.json was measured on; exactly one gfx950 code object defines
    fsk::flagstat_segments_wide_where, it holds all six instantiations (W 4 and 8; bitmap plain and funnelled, bytes), and it is
    the code object of no parent: the unit instantiates no other unit's kernel"""
    from libflagstats_amd import _lib, kernel_id
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        assert kernel_id.kernel_id(_lib.LIB_PATH) == json.load(f)["kernel_source_id"]
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    parents = (b"_ZN3fsk14flagstat_count", b"_ZN3fsk17flagstat_segmentsE", b"_ZN3fsk19flagstat_count_wide", b"_ZN3fsk20flagstat_count_where",
               b"_ZN3fsk24flagstat_segments_filter", b"_ZN3fsk26flagstat_count_wide_filter", b"_ZN3fsk22flagstat_segments_wideI",
               b"_ZN3fsk29flagstat_segments_wide_filterI", b"_ZN3fsk23flagstat_segments_whereI", b"_ZN3fsk25flagstat_count_wide_whereI")
    new = [b"_ZN3fsk28flagstat_segments_wide_whereILi%dELi%dELb%dE" % (W, bits, funnel)
           for W in (4, 8) for bits, funnel in ((1, 0), (1, 1), (8, 0))]
    holders = 0
    seen = {p: 0 for p in parents}
    for co in kernel_id._code_objects(so):
        secs = kernel_id._sections(co)
        names = b"".join(co[secs[t][0]:secs[t][0] + secs[t][1]] for t in (".strtab", ".dynstr") if t in secs)
        for p in parents:
            seen[p] += p in names
        if b"_ZN3fsk28flagstat_segments_wide_whereI" not in names:
            continue
        holders += 1
        for inst in new:
            assert inst in names, inst
        for other in parents:
            assert other not in names, other
    assert holders == 1
    # every parent kernel's mangled prefix still lies in exactly one code object
    for p in parents[1:]:
        assert seen[p] == 1, (p, seen[p])


# ------------------------------------------------------------------ refusals of the Python layers, before the library is loaded
BAD_OFFSETS = (([0, 5, 3, 10], "non-decreasing"), ([0, 5, 11], "exceeds"), (np.array([[0, 5], [5, 10]]), "1-D"),
               (np.array([0.0, 5.0, 10.0]), "integer"), (np.array([-1, 5, 10], dtype=np.int64), "negative"),
               (np.array([], dtype=np.uint64), ">= 1"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_layers_refuse_before_the_library_is_touched(no_library, dtype):
    values = np.zeros(10, dtype=dtype)
    m = np.zeros(10, dtype=bool)
    for f in (sww.counters_segments_ints_where, sww.flagstats_segments_ints_where):
        for offsets, why in BAD_OFFSETS:
            with pytest.raises(ValueError, match=why):
                f(values, offsets, m)
        with pytest.raises(ValueError, match=r"values must be a numpy\.ndarray, not list"):
            f([1, 2, 3], [0, 3], m)
        for bad in (np.zeros(10, dtype=np.int8), np.zeros(10, dtype=np.float32)):
            with pytest.raises(ValueError, match=r"values must have an integer dtype of 2, 4 or 8 bytes"):
                f(bad, [0, 10], m)
        with pytest.raises(ValueError, match=r"values must be 1-D, not 2-D"):
            f(np.zeros((2, 5), dtype=dtype), [0, 10], m)
        # the selection checks are where.py's
        with pytest.raises(ValueError, match=r"where must be a numpy\.ndarray, not list"):
            f(values, [0, 10], [True] * 10)
        with pytest.raises(ValueError, match=r"where must be 1-D, not 2-D"):
            f(values, [0, 10], np.zeros((2, 5), dtype=bool))
        with pytest.raises(ValueError, match=r"where must have dtype bool \(packed=True: a uint8 bitmap\), not uint8"):
            f(values, [0, 10], np.zeros(10, dtype=np.uint8))
        with pytest.raises(ValueError, match=r"where must have dtype uint8 with packed=True \(an LSB-first bitmap\), not bool"):
            f(values, [0, 10], m, packed=True)
        with pytest.raises(ValueError, match=r"where must have one element per value \(10\), not 9"):
            f(values, [0, 10], np.zeros(9, dtype=bool))
        with pytest.raises(ValueError, match=r"where holds 1 bytes, 10 values from bit 0 on need 2"):
            f(values, [0, 10], np.zeros(1, dtype=np.uint8), packed=True)
        with pytest.raises(ValueError, match=r"where holds 2 bytes, 10 values from bit 7 on need 3"):
            f(values, [0, 10], np.zeros(2, dtype=np.uint8), packed=True, bit_offset=7)
        with pytest.raises(ValueError, match=r"bit_offset needs packed=True"):
            f(values, [0, 10], m, bit_offset=3)
        with pytest.raises(ValueError, match=r"bit_offset must not be negative"):
            f(values, [0, 10], np.zeros(2, dtype=np.uint8), packed=True, bit_offset=-1)


def test_device_pointer_and_torch_refusals(no_library):
    import torch
    f = sww.count_segments_device_ptr_ints_where
    o = np.array([0, 4, 10])
    for eb in (2, 1, 16, 0, None):
        with pytest.raises(ValueError, match=r"elem_bytes must be 4 or 8 \(16-bit arrays: segments_where\.count_segments_device_ptr_where\)"):
            f(0x1000, 10, eb, o, 0x2000, 1)
    for sb in (0, 2, 4, 16, "1", True):
        with pytest.raises(ValueError, match=r"sel_bits must be 1 \(an LSB-first bitmap\) or 8 \(one byte per element\), not"):
            f(0x1000, 10, 4, o, 0x2000, sb)
    with pytest.raises(ValueError, match=r"n must not be negative"):
        f(0x1000, -1, 4, o, 0x2000, 1)
    with pytest.raises(ValueError, match=r"sel_offset must not be negative"):
        f(0x1000, 10, 8, o, 0x2000, 8, sel_offset=-1)
    with pytest.raises(ValueError, match=r"sel_ptr must be an int, not float"):
        f(0x1000, 10, 4, o, 1.0, 8)
    with pytest.raises(ValueError, match=r"ptr must fit an unsigned 64-bit integer, not"):
        f(1 << 64, 10, 4, o, 0x2000, 8)
    for offsets, why in BAD_OFFSETS:
        with pytest.raises(ValueError, match=why):
            f(0x1000, 10, 8, offsets, 0x2000, 1)
    g = sww.count_segments_torch_ints_where
    t = torch.zeros(20, dtype=torch.int32)
    off = torch.tensor([0, 7, 20], dtype=torch.int64)
    m = torch.zeros(20, dtype=torch.bool)
    with pytest.raises(ValueError, match=r"t must be a torch\.Tensor, not ndarray"):
        g(np.zeros(20, dtype=np.int32), off, m)
    for dt in (torch.uint8, torch.bool, torch.float32):
        with pytest.raises(ValueError, match=r"t must have an integer dtype of 2, 4 or 8 bytes"):
            g(torch.zeros(20, dtype=dt), off, m)
    with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
        g(torch.zeros(40, dtype=torch.int32)[::2], off, m)
    for bad in (np.array([0, 20]), torch.tensor([0, 20], dtype=torch.int32), torch.zeros(0, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"offsets must be a 1-D contiguous int64 tensor \(nseg \+ 1 values\)"):
            g(t, bad, m)
    with pytest.raises(ValueError, match=r"where must be a torch\.Tensor, not ndarray"):
        g(t, off, np.zeros(20, dtype=bool))
    with pytest.raises(ValueError, match=r"where must have dtype torch\.bool \(packed=True: a torch\.uint8 bitmap\), not torch\.uint8"):
        g(t, off, torch.zeros(20, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"where must have dtype torch\.uint8 with packed=True \(an LSB-first bitmap\), not torch\.bool"):
        g(t, off, m, packed=True)
    with pytest.raises(ValueError, match=r"where must be 1-D and contiguous"):
        g(t, off, torch.zeros(40, dtype=torch.bool)[::2])
    with pytest.raises(ValueError, match=r"where must have one element per value \(20\), not 19"):
        g(t, off, torch.zeros(19, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"where holds 2 bytes, 20 values from bit 0 on need 3"):
        g(t, off, torch.zeros(2, dtype=torch.uint8), packed=True)
    with pytest.raises(ValueError, match=r"bit_offset needs packed=True"):
        g(t, off, m, bit_offset=1)
    for bad in (torch.zeros((3, 32), dtype=torch.int64), torch.zeros((2, 32), dtype=torch.int32), np.zeros((2, 32), dtype=np.int64)):
        with pytest.raises(ValueError, match=r"out must be a contiguous int64 tensor of shape \(2, 32\)"):
            g(t, off, m, out=bad)
    for name in ("selected", "high"):
        for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int64), 0):
            with pytest.raises(ValueError, match=r"%s must be a contiguous int64 tensor of shape \(2,\)" % name):
                g(t, off, m, **{name: bad})
    for tt in (t, torch.zeros(20, dtype=torch.int16), torch.zeros(20, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
            g(tt, off, m)


def test_strict_names_the_first_offending_segment(monkeypatch):
    o = np.array([3, 10, 10, 25, 40], dtype=np.int64)
    rows, sel = np.zeros((4, 32), dtype=np.uint64), np.array([2, 0, 5, 1], dtype=np.uint64)
    calls = []

    def fake(values, offsets, where, **kw):
        calls.append(kw)
        return rows, sel, fake.high

    monkeypatch.setattr(sww, "counters_segments_ints_where", fake)
    m = np.ones(40, dtype=bool)
    fake.high = np.array([0, 0, 0x80000000, 0x10000], dtype=np.uint64)
    with pytest.raises(ValueError, match=re.escape("segment 2 (offsets 10..25): values outside 0..65535: bits 0x80000000 set above bit 15")):
        sww.flagstats_segments_ints_where(np.zeros(40, dtype=np.int32), o, m)
    got = sww.flagstats_segments_ints_where(np.zeros(40, dtype=np.int32), o, m, packed=False, strict=False)
    assert [d["n_values"] for d in got] == [2, 0, 5, 1] and [d["high_bits"] for d in got] == [0, 0, 0x80000000, 0x10000]
    assert calls[1] == dict(packed=False, bit_offset=0)
    fake.high = np.zeros(4, dtype=np.uint64)
    got = sww.flagstats_segments_ints_where(np.zeros(40, dtype=np.int64), o, m)
    assert [d["n_values"] for d in got] == [2, 0, 5, 1] and "high_bits" not in got[0]


# ------------------------------------------------------------------ refusals of the C entries that come before the GPU is touched
def c_calls(lib, a, W, o, nseg, s, so, sb, out, sel, high, flags, n=100):
    ap = a if isinstance(a, int) or a is None else a.ctypes.data
    sp = s if isinstance(s, int) or s is None else s.ctypes.data
    op = None if o is None else o.ctypes.data
    outp = None if out is None else out.ctypes.data
    return (("x64", lambda: lib.FLAGSTATS_hip_wide_x64_segments_where(ap, n, W, op, nseg, sp, so, sb, outp, sel.ctypes.data,
                                                                      high.ctypes.data, flags)),
            ("sync", lambda: lib.FLAGSTATS_hip_device_wide_segments_where_sync(ap, n, W, op, nseg, sp, so, sb, outp, sel.ctypes.data,
                                                                               high.ctypes.data, flags)),
            ("device", lambda: lib.FLAGSTATS_hip_device_wide_segments_where(ap, n, W, op, nseg, sp, so, sb, outp, sel.ctypes.data,
                                                                            high.ctypes.data, flags, None)))


def test_c_entries_refuse_before_the_gpu_and_leave_the_outputs_alone():
    from libflagstats_amd import _lib
    lib = _lib.lib()
    o = np.array([0, 40, 100], dtype=np.uint64)
    out = np.full((2, 32), 7, dtype=np.uint64)
    sel = np.full(2, 7, dtype=np.uint64)
    high = np.full(2, 7, dtype=np.uint64)
    a = np.arange(104, dtype=np.int64)
    s = np.zeros(100, dtype=np.uint8)
    ok = dict(a=a, W=8, o=o, nseg=2, s=s, so=0, sb=8, out=out, sel=sel, high=high, flags=1)
    cases = (
        (dict(W=2), r"elem_bytes 2: 16-bit arrays go to the u16 segments_where entries \(FLAGSTATS_hip_u16_x64_segments_where, "
                    r"FLAGSTATS_hip_device_u16_segments_where\)"),
        (dict(W=3), "elem_bytes must be 4 or 8"), (dict(W=16), "elem_bytes must be 4 or 8"),
        (dict(sb=0), r"sel_bits must be 1 \(an LSB-first bitmap\) or 8 \(one byte per element\)"),
        (dict(sb=4), r"sel_bits must be 1 \(an LSB-first bitmap\) or 8 \(one byte per element\)"),
        (dict(flags=4), "flags: bit 0 store, bit 1 superset; no other bits"),
        (dict(o=None), "NULL d?_?offsets or d?_?out with nseg > 0"), (dict(out=None), "NULL d?_?offsets or d?_?out with nseg > 0"),
        (dict(nseg=(1 << 64) // 256), "nseg is too large"), (dict(a=None), "NULL array with n > 0"),
        (dict(s=None), "NULL selection with n > 0"),
        (dict(a=a.ctypes.data + 4), r"array must be 8-byte aligned \(elem_bytes 8\)"),
        (dict(a=a.ctypes.data + 2, W=4), r"array must be 4-byte aligned \(elem_bytes 4\)"),
        (dict(n=(1 << 64) // 8), "n \\* elem_bytes is not a size"),
        (dict(so=(1 << 64) - 120), "sel_offset \\+ n is not an index"),
    )
    for change, text in cases:
        for name, call in c_calls(lib, **{**ok, **change}):
            assert call() != 0, (change, name)
            assert re.search(text, lib.FLAGSTATS_hip_last_error().decode()), (change, name, lib.FLAGSTATS_hip_last_error())
            assert (out == 7).all() and (sel == 7).all() and (high == 7).all(), (change, name)
    # malformed host offsets are refused with check_host_offsets' words -- by the forms that take host offsets, where a GPU lets
    # them get that far; without one they fail earlier, loudly
    # nseg == 0 does nothing and succeeds, GPU or not, whatever the pointers
    for name, call in c_calls(lib, **{**ok, "nseg": 0}):
        assert call() == 0, name
    for name, call in c_calls(lib, **{**ok, "nseg": 0, "o": None, "out": None, "a": None, "s": None}):
        assert call() == 0, name
    assert (out == 7).all() and (sel == 7).all() and (high == 7).all()


def test_no_gpu_means_the_entries_fail_loudly():
    """Without a GPU the three entries return non-zero with a message and leave the outputs alone; nothing is computed on the CPU.
    (With one, tests/test_gpu_segments_wide_where.py runs them.)"""
    import torch
    if torch.cuda.is_available():
        return
    from libflagstats_amd import _lib
    lib = _lib.lib()
    o = np.array([0, 40, 100], dtype=np.uint64)
    out = np.full((2, 32), 7, dtype=np.uint64)
    sel = np.full(2, 7, dtype=np.uint64)
    high = np.full(2, 7, dtype=np.uint64)
    for dtype in (np.int32, np.int64):
        a = np.arange(100, dtype=dtype)
        for sb, s in ((8, np.ones(100, dtype=np.uint8)), (1, np.full(14, 0xFF, dtype=np.uint8))):
            for name, call in c_calls(lib, a, a.dtype.itemsize, o, 2, s, 3 if sb == 1 else 0, sb, out, sel, high, 1):
                assert call() != 0, name
                assert lib.FLAGSTATS_hip_last_error(), name
                assert (out == 7).all() and (sel == 7).all() and (high == 7).all(), name
        with pytest.raises(_lib.FlagstatsHipError):
            sww.counters_segments_ints_where(a, o, np.ones(100, dtype=bool))
        with pytest.raises(_lib.FlagstatsHipError):
            sww.count_segments_device_ptr_ints_where(a.ctypes.data, a.size, a.dtype.itemsize, o, a.ctypes.data, 8)


# ------------------------------------------------------------------ geometry and the selection addresses
def geometry():
    from libflagstats_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    f = lib.fsk_segments_wide_where_geometry
    f.restype, f.argtypes = _lib.INTERNAL_SIGNATURES["fsk_segments_wide_where_geometry"]
    return f


def sizes(W):
    U = unit_elems(W)
    return (1, 2, 3, 4, 5, 7, 8, 9, U - 1, U, U + 1, 2 * U, 2 * U + 1, 3 * U + 5, 5 * U - 3)


def cases():
    """(W, n, address, phase) over every size and array phase"""
    for W in (4, 8):
        for n in sizes(W):
            for phase in range(16 // W):
                yield W, n, 0x7F00_0000_1000 + W * phase, phase


def test_geometry_equals_the_mirror():
    """fsk_segments_wide_where_geometry (the arithmetic fsk_launch_segments_wide_where launches with; host code, no GPU) against
    segments_wide_where_oracle: every array phase x n x W x sel_offset 0-7 and large ones x sel_bits x grids; geo[6 .. 8) is
    exactly the set of selection bytes that hold an element's bit or byte, enumerated element by element"""
    f = geometry()
    geo = (ctypes.c_uint64 * 8)()
    for W, n, addr, phase in cases():
        for sel_bits, offsets in ((BITMAP, BIT_OFFSETS), (BYTES, BYTE_OFFSETS)):
            for off in offsets:
                for grid in (1, 3, 256):
                    assert f(addr, n, W, off, sel_bits, grid, geo) == 0
                    want = segments_wide_where_geometry(addr, n, W, off, sel_bits, grid)
                    assert list(geo) == want, (W, n, phase, sel_bits, off, grid)
                    assert geo[0] == phase and geo[5] == (sel_bits == BITMAP and (off + 8 - phase) % 8 != 0)
                if off < 1 << 30:
                    held = selection_bytes(n, off, sel_bits)
                    assert np.array_equal(held, np.arange(geo[6], geo[7], dtype=np.uint64)), (W, n, sel_bits, off)


def test_geometry_refusals():
    f = geometry()
    geo = (ctypes.c_uint64 * 8)(*([7] * 8))
    for W in (4, 8):
        for sel_bits in (BITMAP, BYTES):
            assert f(0x1000, 0, W, 5, sel_bits, 4, geo) == 0 and list(geo) == [0] * 8      # m == 0: all zeros
            assert f(0x1000 + W // 2, 10, W, 0, sel_bits, 4, geo) != 0                     # a misaligned address
            assert f(0x1000, 10, W, 0, sel_bits, 0, geo) != 0                              # no workgroups
            assert f(0x1000, 10, W, (1 << 64) - 5, sel_bits, 4, geo) != 0                  # sel_offset + m is no index
            assert f(0x1000, 10, W, (1 << 63) + 1, sel_bits, 4, geo) == 0                  # any uint64 offset that is one
            assert geo[6] == ((1 << 63) + 1 >> 3 if sel_bits == BITMAP else (1 << 63) + 1)
            assert f(0x1000, (1 << 64) // W, W, 0, sel_bits, 4, geo) != 0                  # m * elem_bytes is no size
            # a wave's totals are uint32: grid 1 over 2^35 elements is refused, the same array on 256 workgroups is not
            assert f(0x1000, 1 << 35, W, 0, sel_bits, 1, geo) != 0
            assert f(0x1000, 1 << 35, W, 0, sel_bits, 256, geo) == 0
        for sel_bits in (0, 2, 4, 16, -1):
            assert f(0x1000, 10, W, 0, sel_bits, 4, geo) != 0
    for W in (0, 1, 2, 3, 16, -4):
        assert f(0x1000, 10, W, 0, BITMAP, 4, geo) != 0


def test_selection_addresses_of_the_unguarded_paths():
    """The guard against an over-read of the selection: a model of every address the kernel's unguarded loaders form, in the
    chain regime and for a per-piece unit that lies wholly inside the array -- a lane's byte index, its shift and which two
    adjacent bytes it loads when the launch is funnelled (its own and the next one, or the one in front and its own), derived from
    the launcher's own geometry as the kernel derives them -- forms no address outside geo[6 .. 8), and the bits it extracts from
    a random selection are the mask.  Grid unit 0 of a funnelled launch is not among the unguarded units: at EPV = 4 or 2 a lane
    whose bits do not straddle loads [k - 1, k], and for the array's first vectors k - 1 lies in front of the first byte that holds
    an element's bit (an aligned array under sel_offset & 7 != 0; every chunk of the host form)."""
    f = geometry()
    geo = (ctypes.c_uint64 * 8)()
    rng = np.random.RandomState(19)
    checked = straddling = funnelled_without_straddle = unit0_plain = unit0_held_back = hazard = 0
    for W, n, addr, phase in cases():
        EPV = 16 // W
        U = unit_elems(W)
        mask = rng.randint(0, 2, n).astype(bool)
        for off in BIT_OFFSETS:
            assert f(addr, n, W, off, BITMAP, 3, geo) == 0
            g = list(geo)
            funnel = bool(g[5])
            units = swwo.unguarded_units(g, n, W)
            whole0 = g[0] == 0 and n >= U
            if funnel:
                assert 0 not in units
                unit0_held_back += whole0
                if whole0:
                    # what the rule is for: lane 0 of unit 0, where its bits do not straddle, would load the byte in front of
                    # the first one that holds an element's bit
                    lane_bit = g[4]
                    if (lane_bit & 7) + EPV <= 8:
                        k = swwo._signed(g[3]) + (lane_bit >> 3)
                        assert k - 1 < g[6]
                        hazard += 1
            else:
                assert (0 in units) == whole0
                unit0_plain += whole0
            q, first, count, d, sh = swwo.unguarded_selection_model(g, n, W, BITMAP)
            assert q.size == units.size * 512
            if q.size == 0:
                continue
            assert count == (2 if funnel else 1)
            last = first + count - 1
            assert (first >= g[6]).all() and (last < g[7]).all(), (W, n, phase, off)
            assert (q >= g[0]).all() and (q + EPV <= g[0] + n).all()
            if not funnel:
                assert not d.any()
            assert (sh + EPV <= 8 * count).all()               # the bits lie inside what was loaded
            straddling += int(d.sum())
            funnelled_without_straddle += int(funnel and (d == 0).any())
            if off < 1 << 30:
                sel = pack(mask, off)
                assert sel.size == g[7]
                w = sel[first].astype(np.uint32) | (sel[last].astype(np.uint32) << 8 if funnel else 0)
                bits = (w >> sh.astype(np.uint32)) & ((1 << EPV) - 1)
                for e in range(EPV):
                    assert np.array_equal((bits >> e) & 1, mask[q + e - g[0]].astype(np.uint32)), (W, n, phase, off, e)
                checked += 1
        for off in BYTE_OFFSETS:
            assert f(addr, n, W, off, BYTES, 3, geo) == 0
            g = list(geo)
            assert not g[5]
            q, first, count, d, sh = swwo.unguarded_selection_model(g, n, W, BYTES)
            if q.size == 0:
                continue
            assert count == EPV and (first >= g[6]).all() and (first + count <= g[7]).all(), (W, n, phase, off)
            assert np.array_equal(first - off, q - g[0])          # byte e of the vector at q is element q + e - lo0
    assert checked and straddling and funnelled_without_straddle and unit0_plain and unit0_held_back and hazard


def test_the_walk_is_the_shared_one_rule_by_rule():
    """flagstat_segments_wide_where.hip keeps its own copy of seg_walk<UE> (an occupancy step, as flagstat_segments_wide_filter.hip
    does): it must state the shared walk's rules, plus the one of its own, grid unit 0 of a funnelled launch"""
    src = re.sub(r"\s+", " ", open(os.path.join(CSRC, "flagstat_segments_wide_where.hip")).read())
    parent = re.sub(r"\s+", " ", open(os.path.join(CSRC, "flagstat_segments_wide.hip")).read())
    other = re.sub(r"\s+", " ", open(os.path.join(CSRC, "flagstat_segments_wide_filter.hip")).read())
    shared = re.sub(r"\s+", " ", open(os.path.join(CSRC, "flagstat_segments_shared.h")).read())
    hdr = open(os.path.join(CSRC, "flagstat_segments_wide.h")).read()
    assert int(re.search(r"constexpr int kSegWideUnitBytes = (\d+);", hdr).group(1)) == swwo.UNIT_BYTES
    from segments_wide_oracle import SEG_EPOCH
    assert (1 << int(re.search(r"constexpr int kSegWideWhereDepth = (\d+);", src).group(1))) - 1 == SEG_EPOCH
    assert "seg_walk<UE>(" not in src and "seg_walk<UE>( lo0, hi0, base," in parent
    for rule in ("const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (kThreads / 64);",
                 "const uint64_t gw = static_cast<uint64_t>(blockIdx.x) * (kThreads / 64) + wave;",
                 "const uint64_t u_begin = gw * nunits / waves, u_end = (gw + 1) * nunits / waves;",
                 "const uint64_t p0 = u_begin * UE > lo0 ? u_begin * UE : lo0;",
                 "const uint64_t E = u_end * UE < hi0 ? u_end * UE : hi0;",
                 "if (p0 >= E) return;",
                 "SegWalk sw{off, nseg, base, hi0 - lo0, lo0, lane, 0, 0, 0};",
                 "uint64_t s = sw.first_segment(p0); if (s >= nseg) return; sw.load_window(s);",
                 "uint64_t u = p0 / UE; while (s < nseg && u < u_end) { sw.bounds(s, sb, se); const uint64_t w0 = u * UE; "
                 "const uint64_t x = w0 > p0 ? w0 : p0;",
                 "if (sb >= E) break; if (se <= sb || se <= x) {",
                 "if (sb >= w0 + UE) {",
                 "u = sb / UE; continue; }",
                 "const uint64_t seg_e = se < E ? se : E;",
                 "if (sb <= w0 && w0 >= lo0) { const uint64_t k = (seg_e - w0) / UE;",
                 "if (k >= min_units && k > 0) {",
                 "u += k; open = true; if (u * UE >= se) { emit(s, sb, se); open = false; ++s; } continue; }",
                 "w0 >= lo0 && w0 + UE <= hi0",
                 "const uint64_t w1 = w0 + UE; uint64_t xx = x; for (;;) {",
                 "const uint64_t b = sb > xx ? sb : xx, e = se < w1 ? se : w1;",
                 "open = true; if (e < se) break;",
                 "emit(s, sb, se); open = false; ++s; xx = e; bool more = false; while (s < nseg) { sw.bounds(s, sb, se); "
                 "if (sb >= E) break;",
                 "if (se <= sb || se <= xx) { ++s; continue; } more = sb < w1; break; } if (!more) break; } ++u; }",
                 "if (open) emit(s, sb, se);",
                 "(mode & 1) && b_ >= p0 && e_ <= E"):
        assert rule in src, rule
        assert shared.count(rule) == 1, rule
        assert rule in other, rule
    # the one rule of its own
    assert "const bool guard0 = FUNNEL && u == 0;" in src and "if (!guard0) {" in src
    assert "if (w0 >= lo0 && w0 + UE <= hi0 && !guard0) {" in src and "guard0" not in shared
    for rule in ("constexpr uint64_t UE = kSegWideUnitBytes / W;", "fsk_segments_policy(&min_units, &blocks_per_cu);"):
        assert rule in src and rule in parent, rule
    assert "fsseg::launch_shape(static_cast<uintptr_t>(address), m, fsk::kSegWideUnitBytes / W, grid, &lo0, &nunits, &g);" in src
    assert "end_step<kSegWideWhereDepth>(s, blk);" in src
    assert "seg_emit<true, true>(st, blk, cnt, or_even, or_odd, red, out, selected, high, seg, 0," in src
    # the shared pieces are included, not restated
    for name in ("void select_elements(uint4&", "uint32_t load_bits_wide_guarded(const", "mask_vec_wide(uint4", "valid_bits_wide(uint64_t",
                 "load_mapq_wide_guarded(const", "void count_piece_wide_with(", "uint32_t bytes_mask(uint32_t"):
        holders = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip")) and name in open(os.path.join(CSRC, fn)).read()]
        assert len(holders) == 1 and holders[0].endswith("_device.h"), (name, holders)


# ------------------------------------------------------------------ the oracle itself
def test_oracle_against_compaction_on_hand_made_columns(oracle_mod):
    """segments_wide_where_oracle.want segment by segment against oracle.flagstat_c of values[b:e][mask[b:e]] & 0xFFFF: rows,
    counts and masks all see the selected elements of their own segment only"""
    rng = np.random.RandomState(5)
    for dt, top in (("int32", 31), ("uint32", 31), ("int64", 63), ("uint64", 63)):
        W = np.dtype(dt).itemsize
        UT = swwo.UNSIGNED[W]
        n = 5000
        u = rng.randint(0, 65536, n).astype(UT)
        hot = rng.randint(0, 9, n) == 0
        u[hot] |= (UT(1) << rng.randint(16, top + 1, int(hot.sum())).astype(UT))
        v = u.view(dt)
        mask = rng.randint(0, 3, n) > 0
        mask[100:140] = False                               # a segment with nothing selected
        v.view(UT)[100:140] = swwo.poison(W)
        o = np.array([7, 7, 8, 100, 140, 141, 1000, 1000, 3111, 4990], dtype=np.int64)
        for sup in (False, True):
            rows, sel, high = swwo.want(v, o, mask, sup)
            assert rows.shape == (9, 32) and sel.shape == (9,) and high.shape == (9,) and high.dtype == np.uint64
            for i in range(9):
                b, e = int(o[i]), int(o[i + 1])
                picked = u[b:e][mask[b:e]]
                lo = (picked & UT(0xFFFF)).astype(np.uint16)
                w = oracle_mod.flagstat_c(lo).astype(np.uint64)
                if sup:
                    pp = ((lo & 0x100) == 0) & ((lo & 0x800) == 0) & ((lo & 1) == 1)
                    fail = (lo & 0x200) != 0
                    w[0], w[16], w[9] = int((pp & ~fail).sum()), int((pp & fail).sum()), lo.size - int(fail.sum())
                assert np.array_equal(rows[i], w), (dt, sup, i)
                assert int(sel[i]) == picked.size
                m = 0
                for x in picked.tolist():
                    m |= x & ~0xFFFF
                assert int(high[i]) == m, (dt, i, hex(int(high[i])), hex(m))
            assert int(sel[3]) == 0 and int(high[3]) == 0 and not rows[3].any() and not rows[0].any() and not rows[6].any()
            assert high.any()
        # all selected: the unmasked oracle; one segment: wide_where_oracle
        import segments_wide_oracle
        import wide_where_oracle
        r1, h1 = segments_wide_oracle.want(v, o)
        r2, s2, h2 = swwo.want(v, o, np.ones(n, dtype=bool))
        assert np.array_equal(r1, r2) and np.array_equal(h1, h2) and np.array_equal(s2, np.diff(o).astype(np.uint64))
        c, s, h = wide_where_oracle.want(oracle_mod, v[5:n - 3], mask[5:n - 3])
        r3, s3, h3 = swwo.want(v, [5, n - 3], mask)
        assert np.array_equal(r3[0], c) and int(s3[0]) == s and int(h3[0]) == h
        assert [a.shape for a in swwo.want(v, [5], mask)] == [(0, 32), (0,), (0,)]
