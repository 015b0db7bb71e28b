"""The segmented flagstat of int32 / int64 columns under samtools' filter and a selection together
(libflagstats_amd/segments_wide_filter_where.py, csrc/flagstat_segments_wide_filter_where.hip) on the CPU: the package's exports,
the symbols in the binding tables, the built library and the headers, the identity of the code objects, every refusal of the
Python layers -- raised before the library is loaded -- and of the C entries before the GPU is touched, the kernel's own copy of
the walk against flagstat_segments_wide_where.hip's rule by rule, the selection addresses of its unguarded paths against
segments_wide_where_oracle's model, and the oracle against a per-element loop and against compaction."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_wide_filter_where_oracle as swfwo  # noqa: E402
import segments_wide_where_oracle as swwo  # noqa: E402
from segments_wide_where_oracle import BITMAP, BYTES, pack, unit_elems  # noqa: E402

from libflagstats_amd import segments_wide_filter_where as swfw  # noqa: E402  (fails at import where the feature is missing)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libflagstats_amd", "csrc")
UNIT = "flagstat_segments_wide_filter_where"
PUBLIC = {"FLAGSTATS_hip_device_wide_segments_filter_where": 17, "FLAGSTATS_hip_device_wide_segments_filter_where_sync": 16,
          "FLAGSTATS_hip_wide_x64_segments_filter_where": 16}
LAUNCHER, LAUNCHER_ARGS = "fsk_launch_segments_wide_masked_filter", 19
PY_NAMES = ("counters_segments_ints_filter_where", "flagstats_segments_ints_filter_where", "count_segments_device_ptr_ints_filter_where",
            "count_segments_torch_ints_filter_where")
DTYPES = (np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64)
BIT_OFFSETS = list(range(8)) + [8, 13, 8 * 4099 + 5, (1 << 40) + 3]     # test_segments_wide_where_host.py's
BYTE_OFFSETS = list(range(8)) + [4099, 1 << 40]
KERNEL = b"_ZN3fsk35flagstat_segments_wide_filter_whereI"


@pytest.fixture()
def no_library(monkeypatch):
    """loading the library fails the test: the refusals must come first"""
    from libflagstats_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were refused")

    monkeypatch.setattr(_lib, "lib", boom)


def test_exports_and_shared_checks():
    import libflagstats_amd
    from libflagstats_amd import filter, segments, segments_filter, segments_filter_where, segments_wide, where, wide
    for name in PY_NAMES:
        assert getattr(libflagstats_amd, name) is getattr(swfw, name) and name in libflagstats_amd.__all__
    assert len(set(libflagstats_amd.__all__)) == len(libflagstats_amd.__all__)
    assert "segments_wide_filter_where" in libflagstats_amd.__doc__
    # the checks and the shaping are the other modules', not restated
    assert swfw.check_offsets is segments.check_offsets and swfw._check_values is wide._check_values
    assert swfw._check_tensor is wide._check_tensor and swfw.strict_message is segments_wide.strict_message
    assert swfw._check_selection_numpy is where._check_selection_numpy and swfw._check_selection_torch is where._check_selection_torch
    assert swfw._check_sel_bits is where._check_sel_bits and swfw.segment_filter_dicts is segments_filter.segment_filter_dicts
    assert swfw._check_predicate is filter._check_predicate and swfw._check_mapq_numpy is filter._check_mapq_numpy
    assert swfw._check_mapq_torch is filter._check_mapq_torch
    assert swfw.counters_segments_filter_where is segments_filter_where.counters_segments_filter_where
    assert swfw.count_segments_torch_filter_where is segments_filter_where.count_segments_torch_filter_where
    src = open(os.path.join(ROOT, "libflagstats_amd", "segments_wide_filter_where.py")).read()
    for text in ("must be a numpy.ndarray", "integer dtype of 2, 4 or 8 bytes", "byte order", "must be 1-D, not", "must have one element per value",
                 "must have dtype", "needs packed=True", "sel_bits must be", "values outside 0..65535", "must be a torch.Tensor",
                 "non-decreasing", "16-bit FLAG mask", "needs mapq", "must be in 0..255"):
        assert text not in src, text


def test_symbols_in_the_tables_the_library_the_headers_and_the_makefile():
    from libflagstats_amd import _lib
    for name, nargs in PUBLIC.items():
        assert name in _lib.SIGNATURES and name not in _lib.INTERNAL_SIGNATURES, name
        args = _lib.SIGNATURES[name][1]
        assert len(args) == nargs and _lib.SIGNATURES[name][0] is ctypes.c_int, name
        # n, elem_bytes, nseg, require, exclude, min_mapq, sel_offset, sel_bits, flags
        assert args[1] is ctypes.c_uint64 and args[2] is ctypes.c_int and args[4] is ctypes.c_uint64, name
        assert args[5] is ctypes.c_uint32 and args[6] is ctypes.c_uint32 and args[8] is ctypes.c_uint32, name
        assert args[10] is ctypes.c_uint64 and args[11] is ctypes.c_int and args[15] is ctypes.c_int, name
        assert args[12:15] == [ctypes.c_void_p] * 3, name
    assert LAUNCHER in _lib.INTERNAL_SIGNATURES and LAUNCHER not in _lib.SIGNATURES
    assert len(_lib.INTERNAL_SIGNATURES[LAUNCHER][1]) == LAUNCHER_ARGS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in tuple(PUBLIC) + (LAUNCHER,):
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    section = header[header.index("filtered and selected wide input per segment:"):]
    for name, nargs in PUBLIC.items():
        m = re.search(r"\bint %s\(([^)]*)\)" % name, section)
        assert m and len(m.group(1).split(",")) == nargs, name
    # the section says whose bits `high` holds
    intro = section[:section.index("int FLAGSTATS_hip_device_wide_segments_filter_where(")]
    assert "SELECTED elements ONLY" in intro and "PASSING OR NOT" in intro
    # the launcher is declared in the new internal header and nowhere else
    for fn in sorted(os.listdir(CSRC)) + [os.path.join(ROOT, "include", "libflagstats_hip.h"),
                                          os.path.join(ROOT, "include", "libflagstats_hip_probe.h")]:
        if not fn.endswith(".h"):
            continue
        text = open(os.path.join(CSRC, fn)).read()
        m = re.search(r"\bhipError_t %s\(([^)]*)\)" % LAUNCHER, text)
        if os.path.basename(fn) == UNIT + ".h":
            assert m and len(m.group(1).split(",")) == LAUNCHER_ARGS
            assert "SELECTED" in text and "ONLY" in text
        else:
            assert LAUNCHER not in text, fn
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1)
    hdrs = re.search(r"^HDRS\s*:=(.*)$", mk, re.M).group(1)
    assert "$(HERE)%s.hip" % UNIT in srcs.split() and "$(HERE)%s.h" % UNIT in hdrs.split()


def test_code_objects():
    """K1's code object is still the one profiles/traffic.json was measured on; exactly one gfx950 code object defines
    fsk::flagstat_segments_wide_filter_where, it holds all twelve instantiations (W 4 and 8; MAPQ read or not; bitmap plain and
    funnelled, bytes), and it is the code object of no parent: the unit instantiates no other unit's kernel"""
    from libflagstats_amd import _lib, kernel_id
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        assert kernel_id.kernel_id(_lib.LIB_PATH) == json.load(f)["kernel_source_id"]
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    parents = (b"_ZN3fsk14flagstat_count", b"_ZN3fsk17flagstat_segmentsE", b"_ZN3fsk19flagstat_count_wide", b"_ZN3fsk20flagstat_count_where",
               b"_ZN3fsk24flagstat_segments_filter", b"_ZN3fsk26flagstat_count_wide_filter", b"_ZN3fsk22flagstat_segments_wideI",
               b"_ZN3fsk29flagstat_segments_wide_filterI", b"_ZN3fsk23flagstat_segments_whereI", b"_ZN3fsk25flagstat_count_wide_whereI",
               b"_ZN3fsk28flagstat_segments_wide_whereI", b"_ZN3fsk21flagstat_filter_whereI",
               b"_ZN3fsk30flagstat_segments_filter_whereI", b"_ZN3fsk32flagstat_count_wide_filter_whereI")
    new = [KERNEL + b"Li%dELb%dELi%dELb%dE" % (W, mapq, bits, funnel)
           for W in (4, 8) for mapq in (0, 1) for bits, funnel in ((1, 0), (1, 1), (8, 0))]
    assert len(set(new)) == 12
    holders = 0
    seen = {p: 0 for p in parents}
    for co in kernel_id._code_objects(so):
        secs = kernel_id._sections(co)
        names = b"".join(co[secs[t][0]:secs[t][0] + secs[t][1]] for t in (".strtab", ".dynstr") if t in secs)
        for p in parents:
            seen[p] += p in names
        if KERNEL not in names:
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
BAD_PREDICATES = ((dict(require=0x10000), "require must be a 16-bit FLAG mask"), (dict(exclude=-1), "exclude must be a 16-bit FLAG mask"),
                  (dict(min_mapq=256, mapq="q"), r"min_mapq must be in 0\.\.255"), (dict(min_mapq=30), "min_mapq > 0 needs mapq"),
                  (dict(require=1.5), "require"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_layers_refuse_before_the_library_is_touched(no_library, dtype):
    values = np.zeros(10, dtype=dtype)
    m = np.zeros(10, dtype=bool)
    q = np.zeros(10, dtype=np.uint8)
    for f in (swfw.counters_segments_ints_filter_where, swfw.flagstats_segments_ints_filter_where):
        for offsets, why in BAD_OFFSETS:
            with pytest.raises(ValueError, match=why):
                f(values, offsets, m)
        for kw, why in BAD_PREDICATES:
            kw = {k: (q if isinstance(v, str) else v) for k, v in kw.items()}
            with pytest.raises(ValueError, match=why):
                f(values, [0, 10], m, **kw)
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
        with pytest.raises(ValueError, match=r"where must have dtype bool \(packed=True: a uint8 bitmap\), not uint8"):
            f(values, [0, 10], np.zeros(10, dtype=np.uint8))
        with pytest.raises(ValueError, match=r"where must have dtype uint8 with packed=True \(an LSB-first bitmap\), not bool"):
            f(values, [0, 10], m, packed=True)
        with pytest.raises(ValueError, match=r"where must have one element per value \(10\), not 9"):
            f(values, [0, 10], np.zeros(9, dtype=bool))
        with pytest.raises(ValueError, match=r"where holds 2 bytes, 10 values from bit 7 on need 3"):
            f(values, [0, 10], np.zeros(2, dtype=np.uint8), packed=True, bit_offset=7)
        with pytest.raises(ValueError, match=r"bit_offset needs packed=True"):
            f(values, [0, 10], m, bit_offset=3)
        # the MAPQ checks are filter.py's
        with pytest.raises(ValueError, match="mapq"):
            f(values, [0, 10], m, mapq=np.zeros(9, dtype=np.uint8), min_mapq=1)
        with pytest.raises(ValueError, match="mapq"):
            f(values, [0, 10], m, mapq=np.zeros(10, dtype=np.int32), min_mapq=1)


def test_device_pointer_and_torch_refusals(no_library):
    import torch
    f = swfw.count_segments_device_ptr_ints_filter_where
    o = np.array([0, 4, 10])
    for eb in (2, 1, 16, 0, None):
        with pytest.raises(ValueError, match=r"elem_bytes must be 4 or 8 \(16-bit arrays: "
                                             r"segments_filter_where\.count_segments_device_ptr_filter_where\)"):
            f(0x1000, 10, eb, o, 0x2000, 1)
    for sb in (0, 2, 4, 16, "1", True):
        with pytest.raises(ValueError, match=r"sel_bits must be 1 \(an LSB-first bitmap\) or 8 \(one byte per element\), not"):
            f(0x1000, 10, 4, o, 0x2000, sb)
    with pytest.raises(ValueError, match=r"n must not be negative"):
        f(0x1000, -1, 4, o, 0x2000, 1)
    with pytest.raises(ValueError, match=r"sel_offset must not be negative"):
        f(0x1000, 10, 8, o, 0x2000, 8, sel_offset=-1)
    with pytest.raises(ValueError, match=r"mapq_ptr must be an int, not float"):
        f(0x1000, 10, 4, o, 0x2000, 8, mapq_ptr=1.0)
    with pytest.raises(ValueError, match="min_mapq > 0 needs mapq"):
        f(0x1000, 10, 4, o, 0x2000, 8, min_mapq=3)
    with pytest.raises(ValueError, match="require must be a 16-bit FLAG mask"):
        f(0x1000, 10, 4, o, 0x2000, 8, require=1 << 16)
    for offsets, why in BAD_OFFSETS:
        with pytest.raises(ValueError, match=why):
            f(0x1000, 10, 8, offsets, 0x2000, 1)
    g = swfw.count_segments_torch_ints_filter_where
    t = torch.zeros(20, dtype=torch.int32)
    off = torch.tensor([0, 7, 20], dtype=torch.int64)
    m = torch.zeros(20, dtype=torch.bool)
    with pytest.raises(ValueError, match=r"t must be a torch\.Tensor, not ndarray"):
        g(np.zeros(20, dtype=np.int32), off, m)
    for dt in (torch.uint8, torch.bool, torch.float32):
        with pytest.raises(ValueError, match=r"t must have an integer dtype of 2, 4 or 8 bytes"):
            g(torch.zeros(20, dtype=dt), off, m)
    for bad in (np.array([0, 20]), torch.tensor([0, 20], dtype=torch.int32), torch.zeros(0, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"offsets must be a 1-D contiguous int64 tensor \(nseg \+ 1 values\)"):
            g(t, bad, m)
    with pytest.raises(ValueError, match=r"where must be a torch\.Tensor, not ndarray"):
        g(t, off, np.zeros(20, dtype=bool))
    with pytest.raises(ValueError, match=r"where must have one element per value \(20\), not 19"):
        g(t, off, torch.zeros(19, dtype=torch.bool))
    with pytest.raises(ValueError, match="min_mapq > 0 needs mapq"):
        g(t, off, m, min_mapq=1)
    with pytest.raises(ValueError, match="mapq"):
        g(t, off, m, mapq=torch.zeros(19, dtype=torch.uint8), min_mapq=1)
    with pytest.raises(ValueError, match="exclude must be a 16-bit FLAG mask"):
        g(t, off, m, exclude=0x10000)
    for bad in (torch.zeros((3, 32), dtype=torch.int64), torch.zeros((2, 32), dtype=torch.int32), np.zeros((2, 32), dtype=np.int64)):
        with pytest.raises(ValueError, match=r"out must be a contiguous int64 tensor of shape \(2, 32\)"):
            g(t, off, m, out=bad)
    for name in ("selected", "high"):
        for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), 0):
            with pytest.raises(ValueError, match=r"%s must be a contiguous int64 tensor of shape \(2,\)" % name):
                g(t, off, m, **{name: bad})
    for tt in (t, torch.zeros(20, dtype=torch.int16), torch.zeros(20, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
            g(tt, off, m)


def test_strict_sees_the_selected_elements_whatever_the_filter_says(monkeypatch):
    o = np.array([3, 10, 10, 25, 40], dtype=np.int64)
    rows, sel = np.zeros((4, 32), dtype=np.uint64), np.array([2, 0, 5, 1], dtype=np.uint64)
    calls = []

    def fake(values, offsets, where, **kw):
        calls.append(kw)
        return rows, sel, fake.high

    monkeypatch.setattr(swfw, "counters_segments_ints_filter_where", fake)
    m = np.ones(40, dtype=bool)
    fake.high = np.array([0, 0, 0x80000000, 0x10000], dtype=np.uint64)
    with pytest.raises(ValueError, match=re.escape("segment 2 (offsets 10..25): values outside 0..65535: bits 0x80000000 set above bit 15")):
        swfw.flagstats_segments_ints_filter_where(np.zeros(40, dtype=np.int32), o, m, exclude=0x904)
    got = swfw.flagstats_segments_ints_filter_where(np.zeros(40, dtype=np.int32), o, m, require=1, strict=False)
    assert [d["n_values"] for d in got] == [2, 0, 5, 1] and [d["high_bits"] for d in got] == [0, 0, 0x80000000, 0x10000]
    assert calls[1] == dict(require=1, exclude=0, mapq=None, min_mapq=0, packed=False, bit_offset=0)
    fake.high = np.zeros(4, dtype=np.uint64)
    got = swfw.flagstats_segments_ints_filter_where(np.zeros(40, dtype=np.int64), o, m)
    assert [d["n_values"] for d in got] == [2, 0, 5, 1] and "high_bits" not in got[0]


# ------------------------------------------------------------------ refusals of the C entries that come before the GPU is touched
def c_calls(lib, a, W, o, nseg, req, exc, q, mq, s, so, sb, out, sel, high, flags, n=100):
    def p(x):
        return x if isinstance(x, int) or x is None else x.ctypes.data
    args = (p(a), n, W, p(o), nseg, req, exc, p(q), mq, p(s), so, sb, p(out), sel.ctypes.data, high.ctypes.data, flags)
    return (("x64", lambda: lib.FLAGSTATS_hip_wide_x64_segments_filter_where(*args)),
            ("sync", lambda: lib.FLAGSTATS_hip_device_wide_segments_filter_where_sync(*args)),
            ("device", lambda: lib.FLAGSTATS_hip_device_wide_segments_filter_where(*args, None)))


def test_c_entries_refuse_before_the_gpu_and_leave_the_outputs_alone():
    from libflagstats_amd import _lib
    lib = _lib.lib()
    o = np.array([0, 40, 100], dtype=np.uint64)
    out = np.full((2, 32), 7, dtype=np.uint64)
    sel = np.full(2, 7, dtype=np.uint64)
    high = np.full(2, 7, dtype=np.uint64)
    a = np.arange(104, dtype=np.int64)
    s = np.zeros(100, dtype=np.uint8)
    q = np.zeros(100, dtype=np.uint8)
    ok = dict(a=a, W=8, o=o, nseg=2, req=1, exc=4, q=q, mq=30, s=s, so=0, sb=8, out=out, sel=sel, high=high, flags=1)
    cases = (
        (dict(W=2), r"elem_bytes 2: 16-bit arrays go to the u16 segments_filter_where entries "
                    r"\(FLAGSTATS_hip_u16_x64_segments_filter_where, FLAGSTATS_hip_device_u16_segments_filter_where\)"),
        (dict(W=3), "elem_bytes must be 4 or 8"), (dict(W=16), "elem_bytes must be 4 or 8"),
        (dict(sb=0), r"sel_bits must be 1 \(an LSB-first bitmap\) or 8 \(one byte per element\)"),
        (dict(sb=4), r"sel_bits must be 1 \(an LSB-first bitmap\) or 8 \(one byte per element\)"),
        (dict(flags=4), "flags: bit 0 store, bit 1 superset; no other bits"),
        (dict(req=0x10000), r"require must be a 16-bit FLAG mask \(at most 0xFFFF\)"),
        (dict(exc=0x10000), r"exclude must be a 16-bit FLAG mask \(at most 0xFFFF\)"),
        (dict(mq=256), r"min_mapq must be at most 255 \(MAPQ is one byte\)"),
        (dict(q=None), "NULL mapq with min_mapq > 0 and n > 0"),
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
    # nseg == 0 does nothing and succeeds, GPU or not, whatever the pointers
    for name, call in c_calls(lib, **{**ok, "nseg": 0}):
        assert call() == 0, name
    for name, call in c_calls(lib, **{**ok, "nseg": 0, "o": None, "out": None, "a": None, "s": None, "q": None}):
        assert call() == 0, name
    assert (out == 7).all() and (sel == 7).all() and (high == 7).all()


def test_no_gpu_means_the_entries_fail_loudly():
    """Without a GPU the three entries return non-zero with a message and leave the outputs alone; nothing is computed on the CPU.
    (With one, tests/test_gpu_segments_wide_filter_where.py runs them.)"""
    import torch
    if torch.cuda.is_available():
        return
    from libflagstats_amd import _lib
    lib = _lib.lib()
    o = np.array([0, 40, 100], dtype=np.uint64)
    out = np.full((2, 32), 7, dtype=np.uint64)
    sel = np.full(2, 7, dtype=np.uint64)
    high = np.full(2, 7, dtype=np.uint64)
    q = np.full(100, 40, dtype=np.uint8)
    for dtype in (np.int32, np.int64):
        a = np.arange(100, dtype=dtype)
        for sb, s in ((8, np.ones(100, dtype=np.uint8)), (1, np.full(14, 0xFF, dtype=np.uint8))):
            for mq in (0, 30):
                for name, call in c_calls(lib, a, a.dtype.itemsize, o, 2, 0, 0x904, q, mq, s, 3 if sb == 1 else 0, sb, out, sel, high, 1):
                    assert call() != 0, name
                    assert lib.FLAGSTATS_hip_last_error(), name
                    assert (out == 7).all() and (sel == 7).all() and (high == 7).all(), name
        with pytest.raises(_lib.FlagstatsHipError):
            swfw.counters_segments_ints_filter_where(a, o, np.ones(100, dtype=bool), exclude=0x904, mapq=q, min_mapq=30)
        with pytest.raises(_lib.FlagstatsHipError):
            swfw.count_segments_device_ptr_ints_filter_where(a.ctypes.data, a.size, a.dtype.itemsize, o, a.ctypes.data, 8)


# ------------------------------------------------------------------ the walk and the selection addresses
def flat(name):
    return re.sub(r"\s+", " ", open(os.path.join(CSRC, name)).read())


def test_the_walk_is_the_parents_rule_by_rule():
    """flagstat_segments_wide_filter_where.hip keeps its own copy of seg_walk<UE>, as both parents do: it must state the rules
    flagstat_segments_wide_where.hip states, one by one, grid unit 0 of a funnelled launch (`guard0`) included"""
    src = flat(UNIT + ".hip")
    where = flat("flagstat_segments_wide_where.hip")
    filt = flat("flagstat_segments_wide_filter.hip")
    shared = flat("flagstat_segments_shared.h")
    from segments_wide_oracle import SEG_EPOCH
    assert (1 << int(re.search(r"constexpr int kSegWideFilterWhereDepth = (\d+);", src).group(1))) - 1 == SEG_EPOCH
    assert "seg_walk<UE>(" not in src
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
        assert rule in where and rule in filt and shared.count(rule) == 1, rule
    # the rule the selection adds, in flagstat_segments_wide_where.hip's words
    for rule in ("const bool guard0 = FUNNEL && u == 0;", "if (!guard0) {", "if (w0 >= lo0 && w0 + UE <= hi0 && !guard0) {"):
        assert rule in src and rule in where, rule
    for rule in ("constexpr uint64_t UE = kSegWideUnitBytes / W;", "fsk_segments_policy(&min_units, &blocks_per_cu);"):
        assert rule in src and rule in where and rule in filt, rule
    assert "end_step<kSegWideFilterWhereDepth>(s, blk);" in src
    assert "seg_emit<true, true>(st, blk, cnt, or_even, or_odd, red, out, selected, high, seg, 0," in src
    # the launcher's selection geometry is flagstat_segments_wide_where.h's function, called, not restated
    assert "fsk_segments_wide_where_geometry(addr, m, elem_bytes, sel_offset, sel_bits, grid, geo);" in src
    assert "launch_shape" not in src and "where_extent(m," not in src
    # the shared pieces are included, not restated
    for name in ("void select_elements(uint4&", "uint32_t load_bits_wide_guarded(const", "mask_vec_wide(uint4", "valid_bits_wide(uint64_t",
                 "load_mapq_wide_guarded(const", "void count_piece_wide_with(", "uint32_t bytes_mask(uint32_t", "uint32_t counted_bits(uint32_t",
                 "uint32_t counted_bytes(uint32_t", "uint32_t pass4(const", "uint32_t nibble_to_bit7(uint32_t"):
        holders = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip")) and name in open(os.path.join(CSRC, fn)).read()]
        assert len(holders) == 1 and holders[0].endswith("_device.h"), (name, holders)
    # the three maskings of a piece and the two uses of the selection in a chain step are there
    for text in ("select_elements<W, 1>(v[r], bits, 0u, unused);", "mp & in_piece", "nibble_to_bit7(n0)", "nibble_to_bit7(n1)",
                 "select_elements<W, SEL_BITS>(v[u], xs, sh, unused);", "SEL_BITS == 1 ? counted_bits(p, sb) : counted_bytes(p, sb)",
                 "held_sel = sb;"):
        assert text in src, text


def test_selection_addresses_of_the_unguarded_paths():
    """The kernel forms the selection addresses of its unguarded paths (the chain regime and a per-piece unit wholly inside the
    array, never grid unit 0 of a funnelled launch) in flagstat_segments_wide_where.hip's own expressions, from the geometry that
    launcher's function reports; segments_wide_where_oracle's model of exactly those expressions forms no address outside the
    bytes that hold an element's bit or byte, for the bit and byte offsets test_segments_wide_where_host.py uses, and the bits it
    extracts are the mask.  The MAPQ bytes of an unguarded vector at grid position q are mq[q .. q + EPV): elements all."""
    src, where = flat(UNIT + ".hip"), flat("flagstat_segments_wide_where.hip")
    for expr in ("const uint32_t lane_bit = lane * EPV + (SEL_BITS == 1 ? shift : 0u);",
                 "const uint32_t d = FUNNEL && (lane_bit & 7u) + EPV > 8u ? 1u : 0u;",
                 "const uint32_t sh = SEL_BITS == 1 ? (lane_bit & 7u) + (FUNNEL ? 8u * (1u - d) : 0u) : 0u;",
                 "const int32_t lane_sel = static_cast<int32_t>(SEL_BITS == 1 ? lane_bit >> 3 : lane_bit) + "
                 "(FUNNEL ? static_cast<int32_t>(d) - 1 : 0);",
                 "const uint8_t* ps = sel + u * SU + lane_sel;",
                 "constexpr int SS = kSegRowVecs * EPV / SDIV;", "constexpr int SU = kSegUnitVecs * EPV / SDIV;",
                 "return static_cast<uint32_t>(*reinterpret_cast<const u16_any*>(p));", "return static_cast<uint32_t>(*p);",
                 "return load_mapq_wide<W>(p);",
                 "const uint8_t* sel = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_sel) + geo[3]);",
                 "const uint32_t shift = static_cast<uint32_t>(geo[4]);"):
        assert expr in src and expr in where, expr
    assert src.count("sel + u * SU + lane_sel") == 2 and src.count("load_sel(ps + r * SS)") == 2 and "psn = ps + SU" in src
    assert "const uint8_t* pm = mq + (u * kSegUnitVecs + lane) * EPV;" in src and "mq + (j0 + r * kSegRowVecs) * EPV" in src
    from libflagstats_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    f = lib.fsk_segments_wide_where_geometry
    f.restype, f.argtypes = _lib.INTERNAL_SIGNATURES["fsk_segments_wide_where_geometry"]
    geo = (ctypes.c_uint64 * 8)()
    rng = np.random.RandomState(23)
    checked = funnelled = 0
    for W in (4, 8):
        EPV, U = 16 // W, unit_elems(W)
        for n in (1, EPV, U - 1, U, U + 1, 2 * U + 1, 5 * U - 3):
            for phase in range(EPV):
                addr = 0x7F00_0000_1000 + W * phase
                mask = rng.randint(0, 2, n).astype(bool)
                for sel_bits, offsets in ((BITMAP, BIT_OFFSETS), (BYTES, BYTE_OFFSETS)):
                    for off in offsets:
                        assert f(addr, n, W, off, sel_bits, 3, geo) == 0
                        g = list(geo)
                        units = swwo.unguarded_units(g, n, W)
                        assert not (g[5] and 0 in units)
                        q, first, count, d, sh = swwo.unguarded_selection_model(g, n, W, sel_bits)
                        if q.size == 0:
                            continue
                        assert (first >= g[6]).all() and (first + count <= g[7]).all(), (W, n, phase, sel_bits, off)
                        assert (q >= g[0]).all() and (q + EPV <= g[0] + n).all()      # so are the vector's MAPQ bytes mq[q .. q + EPV)
                        if sel_bits == BYTES:
                            assert np.array_equal(first - off, q - g[0])
                        elif off < 1 << 30:
                            sel = pack(mask, off)
                            w = sel[first].astype(np.uint32) | (sel[first + 1].astype(np.uint32) << 8 if g[5] else 0)
                            bits = (w >> sh.astype(np.uint32)) & ((1 << EPV) - 1)
                            for e in range(EPV):
                                assert np.array_equal((bits >> e) & 1, mask[q + e - g[0]].astype(np.uint32)), (W, n, phase, off, e)
                            checked += 1
                            funnelled += bool(g[5])
    assert checked and funnelled


# ------------------------------------------------------------------ the oracle itself
def test_oracle_against_a_loop_and_against_compaction(oracle_mod):
    """segments_wide_filter_where_oracle.want segment by segment against a per-element Python loop (which elements count, which
    enter `high`) and against oracle.flagstat_c of the compacted, narrowed segment"""
    rng = np.random.RandomState(5)
    for dt, top in (("int32", 31), ("uint32", 31), ("int64", 63), ("uint64", 63)):
        W = np.dtype(dt).itemsize
        UT = swwo.UNSIGNED[W]
        n = 3000
        u = rng.randint(0, 65536, n).astype(UT)
        hot = rng.randint(0, 9, n) == 0
        u[hot] |= (UT(1) << rng.randint(16, top + 1, int(hot.sum())).astype(UT))
        v = u.view(dt)
        mask = rng.randint(0, 3, n) > 0
        mask[100:140] = False                               # a segment with nothing selected
        v.view(UT)[100:140] = swwo.poison(W)
        mapq = rng.randint(0, 61, n).astype(np.uint8)
        o = np.array([7, 7, 8, 100, 140, 141, 1000, 1000, 2111, 2990], dtype=np.int64)
        for require, exclude, min_mapq in ((0, 0, 0), (0, 0x904, 30), (1, 0x4, 0), (0x40, 0, 1), (0, 0, 61), (0x10, 0x10, 0)):
            for sup in (False, True):
                rows, sel, high = swfwo.want(v, o, mask, require, exclude, mapq if min_mapq else None, min_mapq, sup)
                assert rows.shape == (9, 32) and sel.shape == (9,) and high.shape == (9,) and high.dtype == np.uint64
                for i in range(9):
                    b, e = int(o[i]), int(o[i + 1])
                    counted, hb = [], 0
                    for j in range(b, e):
                        x = int(u[j])
                        f = x & 0xFFFF
                        if not mask[j]:
                            continue
                        if not (require & exclude):
                            hb |= x & ~0xFFFF
                        if (f & require) == require and (f & exclude) == 0 and (min_mapq == 0 or int(mapq[j]) >= min_mapq):
                            counted.append(f)
                    lo = np.array(counted, dtype=np.uint16)
                    w = oracle_mod.flagstat_c(lo).astype(np.uint64)
                    if sup:
                        pp = ((lo & 0x100) == 0) & ((lo & 0x800) == 0) & ((lo & 1) == 1)
                        fail = (lo & 0x200) != 0
                        w[0], w[16], w[9] = int((pp & ~fail).sum()), int((pp & fail).sum()), lo.size - int(fail.sum())
                    assert np.array_equal(rows[i], w), (dt, require, exclude, min_mapq, sup, i)
                    assert int(sel[i]) == lo.size and int(high[i]) == hb, (dt, i, hex(int(high[i])), hex(hb))
                assert int(sel[3]) == 0 and int(high[3]) == 0 and not rows[3].any() and not rows[0].any()
                if require & exclude:
                    assert not rows.any() and not sel.any() and not high.any()
                elif (require, exclude, min_mapq) == (0, 0, 61):
                    assert not sel.any() and high.any()             # nothing passes, the selected elements still report their bits
                else:
                    assert sel.any() and high.any()
        # the empty predicate is the selected oracle, an all-ones mask the filtered one
        import segments_wide_filter_oracle
        for a, b in zip(swfwo.want(v, o, mask, superset=True), swwo.want(v, o, mask, True)):
            assert np.array_equal(a, b)
        for a, b in zip(swfwo.want(v, o, np.ones(n, dtype=bool), 0, 0x904, mapq, 30),
                        segments_wide_filter_oracle.want(v, o, 0, 0x904, mapq, 30)):
            assert np.array_equal(a, b)
        assert [a.shape for a in swfwo.want(v, [5], mask)] == [(0, 32), (0,), (0,)]
