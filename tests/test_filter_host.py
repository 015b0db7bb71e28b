"""The filtered flagstat (libflagstats_amd/filter.py, csrc/flagstat_filter.hip) on the CPU: the package's exports, every refusal
of the Python layer -- raised before the library is loaded --, the symbols in the binding tables, the built library and the
headers, the identity of the code objects, and filter_oracle's mask against a per-element loop."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from filter_oracle import filter_mask  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ("FLAGSTATS_hip_device_u16_filter", "FLAGSTATS_hip_device_u16_filter_sync", "FLAGSTATS_hip_u16_x64_filter")
INTERNAL = ("fsk_launch_filter",)
PY_NAMES = ("counters_filter", "flagstats_filter", "count_device_ptr_filter", "count_torch_filter")


@pytest.fixture()
def no_library(monkeypatch):
    """loading the library fails the test: the refusals must come first"""
    from libflagstats_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were refused")

    monkeypatch.setattr(_lib, "lib", boom)


def test_exports():
    import libflagstats_amd
    from libflagstats_amd import filter as flt
    for name in PY_NAMES:
        assert getattr(libflagstats_amd, name) is getattr(flt, name) and name in libflagstats_amd.__all__


def predicate_refusals(call):
    """the refusals every entry shares; call(**kw) runs it with a MAPQ column at hand"""
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


@pytest.mark.parametrize("fn", ["counters_filter", "flagstats_filter"])
def test_numpy_refusals(no_library, fn):
    from libflagstats_amd import filter as flt
    f = getattr(flt, fn)
    v = np.zeros(20, dtype=np.uint16)
    q = np.zeros(20, dtype=np.uint8)
    with pytest.raises(ValueError, match=r"values must be a numpy\.ndarray, not list"):
        f([1, 2, 3])
    for bad in (np.zeros(20, dtype=np.int16), np.zeros(20, dtype=np.int32), np.zeros(20, dtype=np.uint8),
                np.zeros(20, dtype=np.float32), np.zeros(20, dtype=bool), np.zeros(20, dtype=">u2")):
        with pytest.raises(ValueError, match=r"values must have dtype uint16, not " + re.escape(str(bad.dtype))):
            f(bad)
    with pytest.raises(ValueError, match=r"values must be 1-D, not 2-D"):
        f(np.zeros((4, 5), dtype=np.uint16))
    with pytest.raises(ValueError, match=r"values must be 1-D, not 0-D"):
        f(np.array(5, dtype=np.uint16))
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
    predicate_refusals(lambda **kw: f(v, mapq=q, **kw))


def test_device_pointer_refusals(no_library):
    from libflagstats_amd import filter as flt
    f = flt.count_device_ptr_filter
    with pytest.raises(ValueError, match=r"n must not be negative"):
        f(0x1000, -1)
    for name, args, kw in (("ptr", (4096.0, 10), {}), ("n", (0x1000, 10.0), {}), ("n", (0x1000, "10"), {}), ("n", (0x1000, True), {}),
                           ("mapq_ptr", (0x1000, 10), {"mapq_ptr": None}), ("mapq_ptr", (0x1000, 10), {"mapq_ptr": 8192.0})):
        with pytest.raises(ValueError, match=r"%s must be an int, not" % name):
            f(*args, **kw)
    for name, args, kw in (("ptr", (1 << 64, 10), {}), ("ptr", (-8, 10), {}), ("n", (0x1000, 1 << 64), {}),
                           ("mapq_ptr", (0x1000, 10), {"mapq_ptr": 1 << 64})):
        with pytest.raises(ValueError, match=r"%s must fit an unsigned 64-bit integer, not" % name):
            f(*args, **kw)
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
        f(0x1000, 10, min_mapq=1)
    predicate_refusals(lambda **kw: f(0x1000, 10, mapq_ptr=0x2000, **kw))


def test_torch_refusals(no_library):
    import torch
    from libflagstats_amd import filter as flt
    f = flt.count_torch_filter
    t = torch.zeros(20, dtype=torch.int16)
    q = torch.zeros(20, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"t must be a torch\.Tensor, not ndarray"):
        f(np.zeros(20, dtype=np.uint16))
    for dt in (torch.int32, torch.int64, torch.uint8, torch.int8, torch.bool, torch.float16, torch.float32):
        with pytest.raises(ValueError, match=r"t must have dtype int16 or uint16, not " + re.escape(str(dt))):
            f(torch.zeros(20, dtype=dt))
    for bad in (torch.zeros((4, 5), dtype=torch.int16), torch.zeros(40, dtype=torch.int16)[::2], torch.zeros((), dtype=torch.int16)):
        with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
            f(bad)
    with pytest.raises(ValueError, match=r"mapq must be a torch\.Tensor, not ndarray"):
        f(t, mapq=np.zeros(20, dtype=np.uint8), min_mapq=1)
    for dt in (torch.int8, torch.bool, torch.int16, torch.int64, torch.float32):
        with pytest.raises(ValueError, match=r"mapq must have dtype torch\.uint8, not " + re.escape(str(dt))):
            f(t, mapq=torch.zeros(20, dtype=dt), min_mapq=1)
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
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 0):
        with pytest.raises(ValueError, match=r"selected must be a contiguous int64 tensor of 1 element$"):
            f(t, selected=bad)
    with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
        f(t)                                      # host tensors
    with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
        f(t, require=2, exclude=0x904, mapq=q, min_mapq=30, out=torch.zeros(32, dtype=torch.int64))
    # (mapq / out / selected on another device than t: tests/test_gpu_filter.py::test_device_dependent_refusals)


def test_symbols_in_the_tables_the_library_and_the_headers():
    from libflagstats_amd import _lib
    for name in PUBLIC:
        assert name in _lib.SIGNATURES and name not in _lib.INTERNAL_SIGNATURES, name
    for name in INTERNAL:
        assert name in _lib.INTERNAL_SIGNATURES and name not in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_u16_filter"][1]) == 10
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_u16_filter_sync"][1]) == 9
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_u16_x64_filter"][1]) == 9
    assert len(_lib.INTERNAL_SIGNATURES["fsk_launch_filter"][1]) == 11
    for name in PUBLIC + INTERNAL:
        table = _lib.SIGNATURES if name in PUBLIC else _lib.INTERNAL_SIGNATURES
        args = table[name][1]
        assert args[2] is ctypes.c_uint32 and args[3] is ctypes.c_uint32 and args[5] is ctypes.c_uint32, name   # require, exclude, min_mapq
        assert args[1] is ctypes.c_uint64 and args[4] is ctypes.c_void_p, name                                  # n, mapq
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in PUBLIC + INTERNAL:
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    for name in PUBLIC:
        m = re.search(r"\bint %s\(([^)]*)\)" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    internal = open(os.path.join(ROOT, "libflagstats_amd", "csrc", "flagstat_filter.h")).read()
    for name in INTERNAL:
        m = re.search(r"\bhipError_t %s\(([^)]*)\)" % name, internal)
        assert m and name not in header, name
        assert len(m.group(1).split(",")) == len(_lib.INTERNAL_SIGNATURES[name][1]), name


def test_code_objects():
    """K1's code object is still the one profiles/traffic.json was measured on; exactly one gfx950 code object defines
    fsk::flagstat_count_filter, with and without the MAPQ column, and it is not K1's, the wide kernel's or the where kernel's;
    no other code object defines a where or a wide kernel"""
    from libflagstats_amd import _lib, kernel_id
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        recorded = json.load(f)["kernel_source_id"]
    assert kernel_id.kernel_id(_lib.LIB_PATH) == recorded
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    k1, wide, where, flt = [], [], [], []
    for i, co in enumerate(kernel_id._code_objects(so)):
        secs = kernel_id._sections(co)
        names = b"".join(co[secs[t][0]:secs[t][0] + secs[t][1]] for t in (".strtab", ".dynstr") if t in secs)
        if b"_ZN3fsk14flagstat_count" in names:
            k1.append(i)
        if b"_ZN3fsk19flagstat_count_wide" in names:
            wide.append(i)
        if b"_ZN3fsk20flagstat_count_where" in names:
            where.append(i)
        if b"_ZN3fsk21flagstat_count_filterILb0" in names:
            assert b"_ZN3fsk21flagstat_count_filterILb1" in names
            flt.append(i)
        else:
            assert b"_ZN3fsk21flagstat_count_filter" not in names
    assert len(k1) == 1 and len(wide) == 1 and len(where) == 1 and len(flt) == 1, (k1, wide, where, flt)
    assert flt[0] not in (k1[0], wide[0], where[0]), (k1, wide, where, flt)


def test_oracle_mask_against_a_loop():
    """filter_oracle.filter_mask, element by element in plain Python, on 1,000 values: predicates on one and both byte planes, an
    overlapping pair, and thresholds on both sides of 128"""
    rng = np.random.RandomState(7)
    v = rng.randint(0, 65536, 1000).astype(np.uint16)
    v[:64] &= np.uint16(0x00FF)                   # some values that pass predicates with many excluded bits
    v[64:128] = 0
    q = rng.randint(0, 256, 1000).astype(np.uint8)
    q[:8] = (0, 1, 29, 30, 127, 128, 129, 255)
    any_overlap = False
    for require, exclude in ((0, 0), (0, 0x904), (0x2, 0x900), (0x1, 0xF04), (0x0101, 0x8080), (0x0040, 0x0040), (0x0443, 0x0141), (0xFFFF, 0),
                             (0, 0xFFFF)):
        for min_mapq in (0, 1, 30, 127, 128, 129, 200, 255):
            want = []
            for i in range(1000):
                x, m = int(v[i]), int(q[i])
                want.append((x & require) == require and (x & exclude) == 0 and (min_mapq == 0 or m >= min_mapq))
            got = filter_mask(v, require, exclude, q, min_mapq)
            assert got.dtype == np.bool_ and got.tolist() == want, (require, exclude, min_mapq)
            if require & exclude:
                any_overlap = True
                assert not got.any()
    assert any_overlap
    assert filter_mask(v, 0, 0).all() and filter_mask(v, 0, 0, None, 0).sum() == 1000
    assert 0 < filter_mask(v, 0, 0x904, q, 30).sum() < 1000
