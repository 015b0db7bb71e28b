"""The filtered wide-input flagstat under samtools' whole FLAG predicate (libflagstats_amd/wide_filter_rf.py,
csrc/flagstat_wide_filter_rf.hip) on the CPU: wide_filter_rf_oracle against a per-element loop, the package's exports, every
refusal of the Python layer -- raised before the library is loaded -- and of the C entries, the symbols in the binding tables, the
built library, the headers and the Makefile, and the identity of the code object."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_filter_rf_oracle as wro  # noqa: E402
from test_filter_host import no_library, predicate_refusals  # noqa: E402,F401  (no_library is a fixture)
from test_filter_rf_host import rf_refusals  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libflagstats_amd", "csrc")
UNIT = "flagstat_wide_filter_rf"
KERNEL = b"_ZN3fsk29flagstat_count_wide_filter_rf"
PUBLIC = {"FLAGSTATS_hip_device_wide_filter_rf": 14, "FLAGSTATS_hip_device_wide_filter_rf_sync": 13, "FLAGSTATS_hip_wide_x64_filter_rf": 13}
LAUNCHER, LAUNCHER_ARGS = "fsk_launch_wide_filter_rf", 15
PY_NAMES = ("counters_ints_filter_rf", "flagstats_ints_filter_rf", "count_device_ptr_ints_filter_rf", "count_torch_ints_filter_rf")
INT_DTYPES = ("int16", "uint16", "int32", "uint32", "int64", "uint64")


# ------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_oracle_against_a_loop(oracle_mod, dtype):
    """wide_filter_rf_oracle.want on 1,000 values, negatives and values >= 65,536 among them, against a loop over the elements in
    plain Python ints: which elements pass (so `selected`, and the counters as oracle.flagstat_c of exactly those low halves) and
    the OR of the bits above bit 15 of every element; the predicates that no FLAG value satisfies report high == 0"""
    W = np.dtype(dtype).itemsize
    rng = np.random.RandomState(13 + W)
    v = rng.randint(0, 65536, 1000).astype(dtype)
    v[::7] |= np.array(1 << 16, dtype=dtype)
    v[5::11] = -v[5::11] - 1                      # negative: every bit above bit 15 set, the low half inverted
    v[3::13] += np.array(1 << (8 * W - 2), dtype=dtype)
    v[:4] = (0, -1, 65536, 0xFFFF)
    assert (v < 0).sum() > 50 and (v >= 65536).sum() > 100
    q = rng.randint(0, 256, 1000).astype(np.uint8)
    ints = [int(x) for x in v]
    loop_high = 0
    for x in ints:
        loop_high |= (x & ((1 << 8 * W) - 1)) & ~0xFFFF
    assert loop_high == wro.ALL_HIGH[W]
    seen = set()
    for require, exclude in ((0, 0), (0x2, 0x904), (0x0101, 0x8080), (0x0040, 0x0040)):
        for include_any in (0, 0x50, 0x0140, 0x0904, 0x8080):
            for exclude_all in (0, 0x000C, 0x0108, 0x0101, 0xFFFF):
                for min_mapq in (0, 30, 200):
                    passing = []
                    for i, x in enumerate(ints):
                        f = x & 0xFFFF
                        if ((f & require) == require and (f & exclude) == 0 and (include_any == 0 or (f & include_any) != 0)
                                and (exclude_all == 0 or (f & exclude_all) != exclude_all) and (min_mapq == 0 or int(q[i]) >= min_mapq)):
                            passing.append(f)
                    p = (require, exclude, include_any, exclude_all)
                    counters, selected, high = wro.want(oracle_mod, v, *p, q, min_mapq)
                    assert selected == len(passing), (p, min_mapq)
                    assert np.array_equal(counters, oracle_mod.flagstat_c(np.array(passing, dtype=np.uint16)).astype(np.uint64)), (p, min_mapq)
                    assert high == (loop_high if wro.satisfiable(*p) else 0), (p, min_mapq)
                    seen.add((bool(include_any), bool(exclude_all), wro.satisfiable(*p), 0 < len(passing) < 1000))
    assert {(True, True, True, True), (True, False, True, True), (False, True, True, True), (True, True, False, False),
            (True, False, False, False), (False, True, False, False)} <= seen
    # satisfiable(): the numpy pass over all 65,536 values against the same pass in plain Python
    for p, some in (((0, 0, 0, 0), True), ((0x2, 0x904, 0x50, 0xC), True), ((0x0040, 0x0040, 0, 0), False), ((0, 0x50, 0x50, 0), False),
                    ((0xC, 0, 0, 0xC), False), ((0x2, 0x904, 0x0904, 0), False), ((0x0101, 0x8080, 0x8080, 0x0101), False),
                    ((0x0101, 0x8080, 0x8081, 0x0103), True), ((0, 0, 0xFFFF, 0xFFFF), True), ((0xFFFF, 0, 0, 0xFFFF), False)):
        loop = any((f & p[0]) == p[0] and (f & p[1]) == 0 and (p[2] == 0 or (f & p[2]) != 0) and (p[3] == 0 or (f & p[3]) != p[3])
                   for f in range(65536))
        assert loop == some and wro.satisfiable(*p) == some, p
    # nothing passes although something could: the mask is still the column's
    assert wro.want(oracle_mod, v[:1], 0x1, 0, 0x50, 0)[1:] == (0, 0) and wro.want(oracle_mod, v[2:3], 0x1, 0, 0x50, 0)[1:] == (0, 1 << 16)
    assert wro.want(oracle_mod, v[:0], 0, 0, 0x50, 0xC)[1:] == (0, 0)


# ------------------------------------------------------------------ the Python layer
def test_exports_and_shared_checks():
    import libflagstats_amd
    from libflagstats_amd import filter as flt
    from libflagstats_amd import filter_rf as rf
    from libflagstats_amd import wide
    from libflagstats_amd import wide_filter_rf as wrf
    for name in PY_NAMES:
        assert getattr(libflagstats_amd, name) is getattr(wrf, name) and name in libflagstats_amd.__all__
    assert len(set(libflagstats_amd.__all__)) == len(libflagstats_amd.__all__)
    assert "``wide_filter_rf``" in libflagstats_amd.__doc__
    # the checks are wide.py's, filter.py's and filter_rf.py's, not restated
    assert wrf._wide is wide and wrf._filter is flt and wrf._filter_rf is rf
    src = open(os.path.join(ROOT, "libflagstats_amd", "wide_filter_rf.py")).read()
    for text in ("must be a numpy.ndarray", "integer dtype of 2, 4 or 8 bytes", "byte order", "must be 1-D", "16-bit FLAG mask",
                 "min_mapq must be in", "needs mapq", "one element per value", "must have dtype", "values outside 0..65535",
                 "must be a torch.Tensor", "must be a CUDA tensor", "must be an int", "elem_bytes must be"):
        assert text not in src, text
    for call in ("_wide._check_values(", "_wide._check_tensor(", "_wide.high_bits_message(", "_filter_rf._check_predicate_rf(",
                 "_filter._check_mapq_numpy(", "_filter._check_mapq_torch(", "_checks.check_elem_bytes(", "_checks.place_result_triple("):
        assert call in src, call


@pytest.mark.parametrize("fn", ["counters_ints_filter_rf", "flagstats_ints_filter_rf"])
def test_numpy_refusals(no_library, fn):  # noqa: F811
    from libflagstats_amd import wide_filter_rf as wrf
    f = getattr(wrf, fn)
    q = np.zeros(20, dtype=np.uint8)
    with pytest.raises(ValueError, match=r"values must be a numpy\.ndarray, not list"):
        f([1, 2, 3])
    for bad in (np.zeros(4, dtype=np.float32), np.zeros(4, dtype=bool), np.zeros(4, dtype=np.int8), np.zeros(4, dtype=np.uint8)):
        with pytest.raises(ValueError, match=r"values must have an integer dtype of 2, 4 or 8 bytes \(int16, uint16, int32, "
                                             r"uint32, int64, uint64\), not " + re.escape(str(bad.dtype))):
            f(bad)
    with pytest.raises(ValueError, match=r"native \(little-endian\) byte order"):
        f(np.zeros(4, dtype=">i4"))
    for dt in INT_DTYPES:
        v = np.zeros(20, dtype=dt)
        with pytest.raises(ValueError, match=r"values must be 1-D, not 2-D"):
            f(np.zeros((2, 3), dtype=dt))
        with pytest.raises(ValueError, match=r"mapq must be a numpy\.ndarray, not list"):
            f(v, mapq=[0] * 20, min_mapq=1)
        with pytest.raises(ValueError, match=r"mapq must have dtype uint8, not int8"):
            f(v, mapq=np.zeros(20, dtype=np.int8), min_mapq=1)
        with pytest.raises(ValueError, match=r"mapq must be 1-D, not 2-D"):
            f(v, mapq=np.zeros((4, 5), dtype=np.uint8), min_mapq=1)
        for size in (0, 19, 21):
            with pytest.raises(ValueError, match=r"mapq must have one element per value \(20\), not %d" % size):
                f(v, mapq=np.zeros(size, dtype=np.uint8))
        with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
            f(v, include_any=0x50, min_mapq=30)
    for dt in ("uint16", "int32", "int64"):
        v = np.zeros(20, dtype=dt)
        rf_refusals(lambda **kw: f(v, mapq=q, **kw))


def test_device_pointer_refusals(no_library):  # noqa: F811
    from libflagstats_amd import wide_filter_rf as wrf
    f = wrf.count_device_ptr_ints_filter_rf
    for eb in (2, 3, 16, 0, "4"):
        with pytest.raises(ValueError, match=r"elem_bytes must be 4 or 8 \(16-bit arrays: filter_rf\.count_device_ptr_filter_rf\), not"):
            f(0x1000, 10, eb)
    for W in (4, 8):
        with pytest.raises(ValueError, match=r"n must not be negative"):
            f(0x1000, -1, W)
        for name, args, kw in (("ptr", (4096.0, 10, W), {}), ("n", (0x1000, 10.0, W), {}), ("n", (0x1000, True, W), {}),
                               ("mapq_ptr", (0x1000, 10, W), {"mapq_ptr": None}), ("mapq_ptr", (0x1000, 10, W), {"mapq_ptr": 8192.0})):
            with pytest.raises(ValueError, match=r"%s must be an int, not" % name):
                f(*args, **kw)
        for name, args, kw in (("ptr", (1 << 64, 10, W), {}), ("ptr", (-8, 10, W), {}), ("n", (0x1000, 1 << 64, W), {}),
                               ("mapq_ptr", (0x1000, 10, W), {"mapq_ptr": 1 << 64})):
            with pytest.raises(ValueError, match=r"%s must fit an unsigned 64-bit integer, not" % name):
                f(*args, **kw)
        with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
            f(0x1000, 10, W, exclude_all=0xC, min_mapq=1)
        rf_refusals(lambda **kw: f(0x1000, 10, W, mapq_ptr=0x2000, **kw))


def test_torch_refusals(no_library):  # noqa: F811
    import torch
    from libflagstats_amd import wide_filter_rf as wrf
    f = wrf.count_torch_ints_filter_rf
    q = torch.zeros(20, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"t must be a torch\.Tensor, not ndarray"):
        f(np.zeros(4, dtype=np.int32))
    for dt in (torch.float32, torch.bool, torch.int8, torch.uint8):
        with pytest.raises(ValueError, match=r"t must have an integer dtype of 2, 4 or 8 bytes, not " + re.escape(str(dt))):
            f(torch.zeros(4, dtype=dt))
    for dt in (torch.int16, torch.int32, torch.int64):
        t = torch.zeros(20, dtype=dt)
        for bad in (torch.zeros((2, 3), dtype=dt), torch.zeros(8, dtype=dt)[::2]):
            with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
                f(bad)
        with pytest.raises(ValueError, match=r"mapq must be a torch\.Tensor, not ndarray"):
            f(t, mapq=np.zeros(20, dtype=np.uint8), min_mapq=1)
        with pytest.raises(ValueError, match=r"mapq must have dtype torch\.uint8, not torch\.int8"):
            f(t, mapq=torch.zeros(20, dtype=torch.int8), min_mapq=1)
        with pytest.raises(ValueError, match=r"mapq must be 1-D and contiguous"):
            f(t, mapq=torch.zeros(40, dtype=torch.uint8)[::2], min_mapq=1)
        for size in (0, 19, 21):
            with pytest.raises(ValueError, match=r"mapq must have one element per value \(20\), not %d" % size):
                f(t, mapq=torch.zeros(size, dtype=torch.uint8))
        with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
            f(t, include_any=0x50, exclude_all=0xC, min_mapq=30)
        rf_refusals(lambda **kw: f(t, mapq=q, **kw))
        for bad in (torch.zeros(31, dtype=torch.int64), torch.zeros(32, dtype=torch.int32), np.zeros(32, dtype=np.int64)):
            with pytest.raises(ValueError, match=r"out must be a contiguous int64 tensor of 32 elements"):
                f(t, out=bad)
        for name in ("selected", "high"):
            for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 0):
                with pytest.raises(ValueError, match=r"%s must be a contiguous int64 tensor of 1 element$" % name):
                    f(t, **{name: bad})
        with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
            f(t, require=2, exclude=0x904, include_any=0x50, exclude_all=0xC, mapq=q, min_mapq=30, out=torch.zeros(32, dtype=torch.int64),
              selected=torch.zeros(1, dtype=torch.int64), high=torch.zeros(1, dtype=torch.int64))
    # (mapq / out / selected / high on another device than t: tests/test_gpu_wide_filter_rf.py::test_device_dependent_refusals)


# ------------------------------------------------------------------ the C entries' own refusals (before any HIP call)
def test_c_refusals_before_any_hip_call():
    """the filtered wide entries' list in its order with the two new masks directly behind the predicate; the outputs stay as they
    were"""
    from libflagstats_amd import _lib
    lib = _lib.lib()
    a = np.zeros(104, dtype=np.int64)
    q = np.zeros(104, dtype=np.uint8)
    out = np.full(32, 7, dtype=np.uint64)
    sel, high = ctypes.c_uint64(7), ctypes.c_uint64(7)

    def call(name, eb=8, require=1, exclude=4, include_any=0x50, exclude_all=0xC, flags=1, array=a.ctypes.data, mapq=q.ctypes.data,
             counters=True):
        args = [array, 100, eb, require, exclude, include_any, exclude_all, mapq, 30, out.ctypes.data if counters else None,
                ctypes.byref(sel), ctypes.byref(high), flags]
        rc = getattr(lib, name)(*(args + [None] if PUBLIC[name] == 14 else args))
        assert (out == 7).all() and sel.value == 7 and high.value == 7
        return rc, lib.FLAGSTATS_hip_last_error().decode()

    for name in PUBLIC:
        for mask in ("include_any", "exclude_all"):
            for bad in (0x10000, 0xFFFFFFFF):
                for eb in (4, 8):
                    rc, text = call(name, eb=eb, **{mask: bad})
                    assert rc != 0 and text.endswith("%s must be a 16-bit FLAG mask (at most 0xFFFF)" % mask), (name, mask, text)
        # the order: elem_bytes, the predicate, the two new masks, flags, the array, the column, the layout, the counters
        rc, text = call(name, eb=2, exclude=0x10000)
        assert rc != 0 and "u16 filter_rf entries" in text and "FLAGSTATS_hip_device_u16_filter_rf" in text, text
        rc, text = call(name, eb=3, include_any=0x10000)
        assert rc != 0 and "elem_bytes must be 4 or 8" in text, text
        rc, text = call(name, exclude=0x10000, include_any=0x10000)
        assert rc != 0 and "exclude must be a 16-bit FLAG mask (at most 0xFFFF)" in text
        rc, text = call(name, include_any=0x10000, exclude_all=0x10000)
        assert rc != 0 and "include_any must be" in text
        rc, text = call(name, exclude_all=0x10000, flags=4)
        assert rc != 0 and "exclude_all must be" in text
        rc, text = call(name, exclude_all=0x10000, array=None)
        assert rc != 0 and "exclude_all must be" in text
        rc, text = call(name, flags=4, array=None)
        assert rc != 0 and "no other bits" in text
        rc, text = call(name, array=None, mapq=None)
        assert rc != 0 and "NULL array with n > 0" in text
        rc, text = call(name, mapq=None, array=a.ctypes.data + 4)
        assert rc != 0 and "NULL mapq with min_mapq > 0 and n > 0" in text
        rc, text = call(name, array=a.ctypes.data + 4, counters=False)
        assert rc != 0 and "8-byte aligned" in text
        rc, text = call(name, eb=4, array=a.ctypes.data + 2)
        assert rc != 0 and "4-byte aligned" in text
        rc, text = call(name, counters=False)
        assert rc != 0 and "NULL counters" in text
        # the same where the launcher would reduce the predicate or launch nothing
        rc, text = call(name, include_any=0x40, exclude_all=0, array=None)
        assert rc != 0 and "NULL array with n > 0" in text
        rc, text = call(name, exclude=0x50, exclude_all=0, mapq=None)
        assert rc != 0 and "NULL mapq with min_mapq > 0 and n > 0" in text
    # the text of the rule stands in flagstat_derived_host.h and in no unit
    holders = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip")) and "16-bit FLAG mask" in open(os.path.join(CSRC, fn)).read()]
    assert holders == ["flagstat_derived_host.h"]


# ------------------------------------------------------------------ symbols
def test_symbols_in_the_tables_the_library_the_headers_and_the_makefile():
    from libflagstats_amd import _lib
    u32, u64, vp, ci = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int
    for name, nargs in PUBLIC.items():
        assert name in _lib.SIGNATURES and name not in _lib.INTERNAL_SIGNATURES, name
        restype, args = _lib.SIGNATURES[name]
        assert restype is ci and len(args) == nargs, name
        # array, n, elem_bytes, require, exclude, include_any, exclude_all, mapq, min_mapq, out, selected, high, flags
        assert args[:13] == [vp, u64, ci, u32, u32, u32, u32, vp, u32, vp, vp, vp, ci], name
    assert _lib.SIGNATURES["FLAGSTATS_hip_device_wide_filter_rf"][1][13] is vp                       # the stream
    assert LAUNCHER in _lib.INTERNAL_SIGNATURES and LAUNCHER not in _lib.SIGNATURES
    assert _lib.INTERNAL_SIGNATURES[LAUNCHER][1] == [vp, u64, ci, u32, u32, u32, u32, vp, u32, vp, vp, vp, ci, u32, vp]
    assert len(_lib.INTERNAL_SIGNATURES[LAUNCHER][1]) == LAUNCHER_ARGS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in tuple(PUBLIC) + (LAUNCHER,):
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    begin = header.index("filtered wide input, the whole predicate:")
    assert header.index("filtered wide input:") < begin < header.index("selected elements of wide input:")
    section = header[begin:header.index("selected elements of wide input:")]
    for name, nargs in PUBLIC.items():
        m = re.search(r"\bint %s\(([^)]*)\)" % name, section)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert len(re.findall(r"\b%s\(" % name, header)) == 1, name
    # the section states the predicate and the three things a call can be
    intro = section[:section.index("int FLAGSTATS_hip_device_wide_filter_rf(")]
    for text in ("(include_any == 0 || (f(i) & include_any) != 0)", "(exclude_all == 0 || (f(i) & exclude_all) != exclude_all)",
                 "NO ELEMENT", "IS READ", "the filtered wide entries' kernel", "fsk::flagstat_count_wide_filter_rf", "above 0xFFFF",
                 "low 16 bits"):
        assert text in intro, text
    # the launcher is declared in the unit's internal header and nowhere else
    for path in [os.path.join(CSRC, fn) for fn in sorted(os.listdir(CSRC))] + [os.path.join(ROOT, "include", "libflagstats_hip.h"),
                                                                               os.path.join(ROOT, "include", "libflagstats_hip_probe.h")]:
        if not path.endswith(".h"):
            continue
        text = open(path).read()
        m = re.search(r"^hipError_t %s\(([^)]*)\)" % LAUNCHER, text, re.M)
        if os.path.basename(path) == UNIT + ".h":
            assert m and len(m.group(1).split(",")) == LAUNCHER_ARGS
            assert "NO ELEMENT IS READ" in text
        else:
            assert LAUNCHER not in text, path
    # the reduction is called, not redeclared; the residue's device code is included, not restated
    unit = open(os.path.join(CSRC, UNIT + ".hip")).read()
    assert '#include "flagstat_filter_rf.h"' in unit and '#include "flagstat_filter_rf_device.h"' in unit
    assert "int fsk_filter_rf_reduce(" not in unit and "fsk_filter_rf_reduce(require, exclude, include_any, exclude_all, m)" in unit
    for name in ("uint32_t pass4_rf(const", "struct FilterRfArgs", "FilterRfArgs filter_rf_args_of(uint32_t", "uint32_t and_nonzero_bytes(uint32_t"):
        holders = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip")) and name in open(os.path.join(CSRC, fn)).read()]
        assert holders == ["flagstat_filter_rf_device.h"], (name, holders)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1)
    hdrs = re.search(r"^HDRS\s*:=(.*)$", mk, re.M).group(1)
    assert "$(HERE)%s.hip" % UNIT in srcs.split() and "$(HERE)%s.h" % UNIT in hdrs.split()
    assert "$(HERE)flagstat_filter_rf_device.h" in hdrs.split()


def test_code_objects():
    """K1's code object is still the one profiles/traffic.json was measured on; exactly one gfx950 code object defines
    fsk::flagstat_count_wide_filter_rf, it holds all 12 instantiations (two widths; MAPQ read or not; the any-of test, the all-of
    test, both) and no other fsk::flagstat_* kernel: the unit calls fsk_launch_wide_filter and instantiates no other unit's
    kernel"""
    from libflagstats_amd import _lib, kernel_id
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        assert kernel_id.kernel_id(_lib.LIB_PATH) == json.load(f)["kernel_source_id"]
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    new = [KERNEL + b"ILi%dELb%dELb%dELb%dEE" % (W, mapq, any_of, all_of) for W in (4, 8) for mapq in (0, 1)
           for any_of, all_of in ((1, 0), (0, 1), (1, 1))]
    assert len(set(new)) == 12
    holders = 0
    for co in kernel_id._code_objects(so):
        secs = kernel_id._sections(co)
        names = b"".join(co[secs[t][0]:secs[t][0] + secs[t][1]] for t in (".strtab", ".dynstr") if t in secs)
        if KERNEL not in names:
            continue
        holders += 1
        for inst in new:
            assert inst in names, inst
        for W in (4, 8):
            for mapq in (0, 1):
                assert KERNEL + b"ILi%dELb%dELb0ELb0EE" % (W, mapq) not in names
        assert len(set(re.findall(re.escape(KERNEL) + rb"ILi\dELb\dELb\dELb\dEE", names))) == 12
        kernels = set(re.findall(rb"_ZN3fsk\d+flagstat_[a-z0-9_]+", names))
        assert kernels == {KERNEL}, kernels
    assert holders == 1
    # the existing tests find their kernels by these prefixes: the new name falls under none of them
    for prefix in (b"_ZN3fsk21flagstat_count_filter", b"_ZN3fsk21flagstat_filter_where", b"_ZN3fsk14flagstat_count",
                   b"_ZN3fsk24flagstat_segments_filter", b"_ZN3fsk20flagstat_count_where", b"_ZN3fsk19flagstat_count_wide",
                   b"_ZN3fsk26flagstat_count_wide_filter", b"_ZN3fsk24flagstat_count_filter_rf", b"_ZN3fsk17flagstat_segments",
                   b"_ZN3fsk22flagstat_segments_wide", b"_ZN3fsk29flagstat_segments_wide_filterI", b"_ZN3fsk23flagstat_segments_where",
                   b"_ZN3fsk25flagstat_count_wide_whereI", b"_ZN3fsk28flagstat_segments_wide_whereI", b"_ZN3fsk30flagstat_segments_filter_where",
                   b"_ZN3fsk35flagstat_segments_wide_filter_whereI"):
        assert not KERNEL.startswith(prefix) and prefix not in KERNEL
