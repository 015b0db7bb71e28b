"""The filtered wide-input flagstat (libflagstats_amd/wide_filter.py, csrc/flagstat_wide_filter.hip) on the CPU: the package's
exports, every refusal of the Python layer and its text -- raised before the library is loaded --, the symbols in the binding
tables, the built library and the headers, the identity of the code objects, and wide_filter_oracle on hand-made columns."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_filter_oracle  # noqa: E402
from test_filter_host import predicate_refusals  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ("FLAGSTATS_hip_device_wide_filter", "FLAGSTATS_hip_device_wide_filter_sync", "FLAGSTATS_hip_wide_x64_filter")
INTERNAL = ("fsk_launch_wide_filter",)
PY_NAMES = ("counters_ints_filter", "flagstats_ints_filter", "count_device_ptr_ints_filter", "count_torch_ints_filter")
INT_DTYPES = ("int16", "uint16", "int32", "uint32", "int64", "uint64")


@pytest.fixture()
def no_library(monkeypatch):
    """loading the library fails the test: the refusals must come first"""
    from libflagstats_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were refused")

    monkeypatch.setattr(_lib, "lib", boom)


def test_exports():
    import libflagstats_amd
    from libflagstats_amd import wide_filter
    for name in PY_NAMES:
        assert getattr(libflagstats_amd, name) is getattr(wide_filter, name) and name in libflagstats_amd.__all__


@pytest.mark.parametrize("fn", ["counters_ints_filter", "flagstats_ints_filter"])
def test_numpy_refusals(no_library, fn):
    from libflagstats_amd import wide_filter
    f = getattr(wide_filter, fn)
    q = np.zeros(20, dtype=np.uint8)
    # the value checks are wide.py's
    with pytest.raises(ValueError, match=r"values must be a numpy\.ndarray, not list"):
        f([1, 2, 3])
    for bad in (np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.float64), np.zeros(4, dtype=bool),
                np.array([1, 2], dtype=object), np.zeros(4, dtype=np.int8), np.zeros(4, dtype=np.uint8),
                np.zeros(4, dtype="S2"), np.zeros(4, dtype=np.complex64)):
        with pytest.raises(ValueError, match=r"values must have an integer dtype of 2, 4 or 8 bytes \(int16, uint16, int32, "
                                             r"uint32, int64, uint64\), not " + re.escape(str(bad.dtype))):
            f(bad)
    with pytest.raises(ValueError, match=r"native \(little-endian\) byte order"):
        f(np.zeros(4, dtype=">i4"))
    for dt in INT_DTYPES:
        v = np.zeros(20, dtype=dt)
        with pytest.raises(ValueError, match=r"values must be 1-D, not 2-D"):
            f(np.zeros((2, 3), dtype=dt))
        with pytest.raises(ValueError, match=r"values must be 1-D, not 0-D"):
            f(np.array(5, dtype=dt))
        # the MAPQ and predicate checks are filter.py's
        with pytest.raises(ValueError, match=r"mapq must be a numpy\.ndarray, not list"):
            f(v, mapq=[0] * 20, min_mapq=1)
        for bad in (np.zeros(20, dtype=np.int8), np.zeros(20, dtype=bool), np.zeros(20, dtype=np.uint16), np.zeros(20, dtype=np.float32)):
            with pytest.raises(ValueError, match=r"mapq must have dtype uint8, not " + re.escape(str(bad.dtype))):
                f(v, mapq=bad, min_mapq=1)
        with pytest.raises(ValueError, match=r"mapq must be 1-D, not 2-D"):
            f(v, mapq=np.zeros((4, 5), dtype=np.uint8), min_mapq=1)
        for size in (0, 19, 21):
            with pytest.raises(ValueError, match=r"mapq must have one element per value \(20\), not %d" % size):
                f(v, mapq=np.zeros(size, dtype=np.uint8))
        with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
            f(v, min_mapq=30)
    for dt in ("uint16", "int32", "int64"):
        v = np.zeros(20, dtype=dt)
        predicate_refusals(lambda **kw: f(v, mapq=q, **kw))


def test_device_pointer_refusals(no_library):
    from libflagstats_amd import wide_filter
    f = wide_filter.count_device_ptr_ints_filter
    for eb in (2, 3, 16, 0, "4"):
        with pytest.raises(ValueError, match=r"elem_bytes must be 4 or 8 \(16-bit arrays: filter\.count_device_ptr_filter\), not"):
            f(0x1000, 10, eb)
    for W in (4, 8):
        with pytest.raises(ValueError, match=r"n must not be negative"):
            f(0x1000, -1, W)
        for name, args, kw in (("ptr", (4096.0, 10, W), {}), ("n", (0x1000, 10.0, W), {}), ("n", (0x1000, "10", W), {}),
                               ("n", (0x1000, True, W), {}), ("mapq_ptr", (0x1000, 10, W), {"mapq_ptr": None}),
                               ("mapq_ptr", (0x1000, 10, W), {"mapq_ptr": 8192.0})):
            with pytest.raises(ValueError, match=r"%s must be an int, not" % name):
                f(*args, **kw)
        for name, args, kw in (("ptr", (1 << 64, 10, W), {}), ("ptr", (-8, 10, W), {}), ("n", (0x1000, 1 << 64, W), {}),
                               ("mapq_ptr", (0x1000, 10, W), {"mapq_ptr": 1 << 64})):
            with pytest.raises(ValueError, match=r"%s must fit an unsigned 64-bit integer, not" % name):
                f(*args, **kw)
        with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
            f(0x1000, 10, W, min_mapq=1)
        predicate_refusals(lambda **kw: f(0x1000, 10, W, mapq_ptr=0x2000, **kw))


def test_torch_refusals(no_library):
    import torch
    from libflagstats_amd import wide_filter
    f = wide_filter.count_torch_ints_filter
    q = torch.zeros(20, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"t must be a torch\.Tensor, not ndarray"):
        f(np.zeros(4, dtype=np.int32))
    for dt in (torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.bool, torch.int8, torch.uint8, torch.complex64):
        with pytest.raises(ValueError, match=r"t must have an integer dtype of 2, 4 or 8 bytes, not " + re.escape(str(dt))):
            f(torch.zeros(4, dtype=dt))
    for dt in (torch.int16, torch.int32, torch.int64):
        t = torch.zeros(20, dtype=dt)
        for bad in (torch.zeros((2, 3), dtype=dt), torch.zeros(8, dtype=dt)[::2], torch.zeros((), dtype=dt)):
            with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
                f(bad)
        with pytest.raises(ValueError, match=r"mapq must be a torch\.Tensor, not ndarray"):
            f(t, mapq=np.zeros(20, dtype=np.uint8), min_mapq=1)
        for qdt in (torch.int8, torch.bool, torch.int16, torch.int64, torch.float32):
            with pytest.raises(ValueError, match=r"mapq must have dtype torch\.uint8, not " + re.escape(str(qdt))):
                f(t, mapq=torch.zeros(20, dtype=qdt), min_mapq=1)
        for bad in (torch.zeros((4, 5), dtype=torch.uint8), torch.zeros(40, dtype=torch.uint8)[::2]):
            with pytest.raises(ValueError, match=r"mapq must be 1-D and contiguous"):
                f(t, mapq=bad, min_mapq=1)
        for size in (0, 19, 21):
            with pytest.raises(ValueError, match=r"mapq must have one element per value \(20\), not %d" % size):
                f(t, mapq=torch.zeros(size, dtype=torch.uint8))
        with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
            f(t, min_mapq=30)
        predicate_refusals(lambda **kw: f(t, mapq=q, **kw))
        for bad in (torch.zeros(31, dtype=torch.int64), torch.zeros(32, dtype=torch.int32), torch.zeros(64, dtype=torch.int64)[::2],
                    np.zeros(32, dtype=np.int64)):
            with pytest.raises(ValueError, match=r"out must be a contiguous int64 tensor of 32 elements"):
                f(t, out=bad)
        for name in ("selected", "high"):
            for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 0):
                with pytest.raises(ValueError, match=r"%s must be a contiguous int64 tensor of 1 element$" % name):
                    f(t, **{name: bad})
        with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
            f(t)                                  # a host tensor
        with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
            f(t, require=2, exclude=0x904, mapq=q, min_mapq=30, out=torch.zeros(32, dtype=torch.int64),
              selected=torch.zeros(1, dtype=torch.int64), high=torch.zeros(1, dtype=torch.int64))
    # (mapq / out / selected / high on another device than t: tests/test_gpu_wide_filter.py::test_python_layers)


def test_the_checks_are_shared_not_copied():
    """wide_filter.py holds no refusal text of wide.py's or filter.py's: it calls their functions"""
    src = open(os.path.join(ROOT, "libflagstats_amd", "wide_filter.py")).read()
    for text in ("must be a numpy.ndarray", "integer dtype of 2, 4 or 8 bytes", "byte order", "must be 1-D", "16-bit FLAG mask",
                 "min_mapq must be in", "needs mapq", "one element per value", "must have dtype", "values outside 0..65535",
                 "must be a torch.Tensor", "must be a CUDA tensor"):
        assert text not in src, text
    for call in ("_wide._check_values(", "_wide._check_tensor(", "_wide.high_bits_message(", "_filter._check_predicate(",
                 "_filter._check_mapq_numpy(", "_filter._check_mapq_torch("):
        assert call in src, call


def test_symbols_in_the_tables_the_library_and_the_headers():
    from libflagstats_amd import _lib
    for name in PUBLIC:
        assert name in _lib.SIGNATURES and name not in _lib.INTERNAL_SIGNATURES, name
    for name in INTERNAL:
        assert name in _lib.INTERNAL_SIGNATURES and name not in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_wide_filter"][1]) == 12
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_wide_filter_sync"][1]) == 11
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_wide_x64_filter"][1]) == 11
    assert len(_lib.INTERNAL_SIGNATURES["fsk_launch_wide_filter"][1]) == 13
    for name in PUBLIC + INTERNAL:
        table = _lib.SIGNATURES if name in PUBLIC else _lib.INTERNAL_SIGNATURES
        args = table[name][1]
        assert args[1] is ctypes.c_uint64 and args[2] is ctypes.c_int, name                                     # n, elem_bytes
        assert args[3] is ctypes.c_uint32 and args[4] is ctypes.c_uint32 and args[6] is ctypes.c_uint32, name   # require, exclude, min_mapq
        assert args[5] is ctypes.c_void_p and args[7:10] == [ctypes.c_void_p] * 3 and args[10] is ctypes.c_int, name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in PUBLIC + INTERNAL:
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    for name in PUBLIC:
        m = re.search(r"\bint %s\(([^)]*)\)" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    internal = open(os.path.join(ROOT, "libflagstats_amd", "csrc", "flagstat_wide_filter.h")).read()
    for name in INTERNAL:
        m = re.search(r"\bhipError_t %s\(([^)]*)\)" % name, internal)
        assert m and name not in header, name
        assert len(m.group(1).split(",")) == len(_lib.INTERNAL_SIGNATURES[name][1]), name
    # the header says what an overlapping pair does to the mask
    assert "NO ELEMENT IS READ" in internal and "NO ELEMENT IS READ" in header


def test_code_objects():
    """K1's code object is still the one profiles/traffic.json was measured on; every derived kernel that existed is still in
    exactly one code object; the four instantiations of fsk::flagstat_count_wide_filter sit together in one code object that
    holds none of the others"""
    from libflagstats_amd import _lib, kernel_id
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        recorded = json.load(f)["kernel_source_id"]
    assert kernel_id.kernel_id(_lib.LIB_PATH) == recorded
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    existing = {"k1": b"_ZN3fsk14flagstat_count", "wide": b"_ZN3fsk19flagstat_count_wide", "where": b"_ZN3fsk20flagstat_count_where",
                "filter": b"_ZN3fsk21flagstat_count_filter", "segments": b"_ZN3fsk17flagstat_segments",
                "segments_filter": b"_ZN3fsk24flagstat_segments_filter"}
    new = [b"_ZN3fsk26flagstat_count_wide_filterILi%dELb%dE" % (W, q) for W in (4, 8) for q in (0, 1)]
    found = {k: [] for k in existing}
    mine = []
    for i, co in enumerate(kernel_id._code_objects(so)):
        secs = kernel_id._sections(co)
        names = b"".join(co[secs[t][0]:secs[t][0] + secs[t][1]] for t in (".strtab", ".dynstr") if t in secs)
        for k, prefix in existing.items():
            if prefix in names:
                found[k].append(i)
        if any(n in names for n in new):
            assert all(n in names for n in new), i
            mine.append(i)
    assert all(len(v) == 1 for v in found.values()), found
    assert len(mine) == 1 and all(mine[0] != v[0] for v in found.values()), (mine, found)


def test_oracle_on_hand_made_columns(oracle_mod):
    """wide_filter_oracle.want: the counters see the low 16 bits of the elements that pass, `high` every element"""
    for dt, top in (("int32", 31), ("uint32", 31), ("int64", 63), ("uint64", 63)):
        U = wide_filter_oracle.UNSIGNED[np.dtype(dt).itemsize]
        v = np.array([0x0041, 0x0004 | (1 << 16), 0x0041 | (1 << 20), 0x0905, 0x0001 | (1 << top)], dtype=U).view(dt)
        q = np.array([60, 60, 10, 60, 60], dtype=np.uint8)
        c, selected, high = wide_filter_oracle.want(oracle_mod, v, 0x0001, 0x0904, q, 30)
        assert selected == 2 and high == (1 << 16) | (1 << 20) | (1 << top)          # elements 0 and 4 pass; 1 and 2 only report
        assert np.array_equal(c, oracle_mod.flagstat_c(np.array([0x0041, 0x0001], dtype=np.uint16)).astype(np.uint64))
        c, selected, high = wide_filter_oracle.want(oracle_mod, v, 0x0040, 0x0040)
        assert selected == 0 and not c.any() and high == (1 << 16) | (1 << 20) | (1 << top)
        c, selected, high = wide_filter_oracle.want(oracle_mod, v[:1], 0, 0)
        assert selected == 1 and high == 0
        c, selected, high = wide_filter_oracle.want(oracle_mod, v[:0], 0, 0)
        assert selected == 0 and high == 0 and not c.any()
    assert wide_filter_oracle.low16(np.array([-1, 65536 + 7], dtype=np.int64)).tolist() == [0xFFFF, 7]
