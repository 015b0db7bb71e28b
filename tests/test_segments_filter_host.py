"""The filtered segmented flagstat (libflagstats_amd/segments_filter.py, csrc/flagstat_segments_filter.hip) on the CPU: the
package's exports, every refusal of the Python layer -- raised before the library is loaded --, the symbols in the binding tables,
the built library and the headers, the identity of the code objects, and segments_filter_oracle against a per-segment loop over
where_oracle.want_counters."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_filter_oracle as sfo  # noqa: E402
import where_oracle  # noqa: E402
from filter_oracle import filter_mask  # noqa: E402
from test_filter_host import predicate_refusals  # noqa: E402

from libflagstats_amd import segments_filter as sf  # noqa: E402  (fails at import where the feature is missing)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ("FLAGSTATS_hip_device_u16_segments_filter", "FLAGSTATS_hip_device_u16_segments_filter_sync",
          "FLAGSTATS_hip_u16_x64_segments_filter")
INTERNAL = ("fsk_launch_segments_filter",)
PY_NAMES = ("flagstats_segments_filter", "count_segments_device_ptr_filter", "count_segments_torch_filter", "segment_filter_dicts")


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
        assert getattr(libflagstats_amd, name) is getattr(sf, name) and name in libflagstats_amd.__all__


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


def test_numpy_refusals(no_library):
    f = sf.flagstats_segments_filter
    v = np.zeros(20, dtype=np.uint16)
    q = np.zeros(20, dtype=np.uint8)
    o = np.array([0, 7, 20])
    with pytest.raises(ValueError, match=r"values must be a numpy\.ndarray, not list"):
        f([1, 2, 3], o)
    for bad in (np.zeros(20, dtype=np.int16), np.zeros(20, dtype=np.int32), np.zeros(20, dtype=bool)):
        with pytest.raises(ValueError, match=r"values must have dtype uint16, not " + re.escape(str(bad.dtype))):
            f(bad, o)
    with pytest.raises(ValueError, match=r"values must be 1-D, not 2-D"):
        f(np.zeros((4, 5), dtype=np.uint16), o)
    with pytest.raises(ValueError, match=r"mapq must be a numpy\.ndarray, not list"):
        f(v, o, mapq=[0] * 20, min_mapq=1)
    with pytest.raises(ValueError, match=r"mapq must have dtype uint8, not int8"):
        f(v, o, mapq=np.zeros(20, dtype=np.int8), min_mapq=1)
    with pytest.raises(ValueError, match=r"mapq must be 1-D, not 2-D"):
        f(v, o, mapq=np.zeros((4, 5), dtype=np.uint8), min_mapq=1)
    for size in (0, 19, 21):
        with pytest.raises(ValueError, match=r"mapq must have one element per value \(20\), not %d" % size):
            f(v, o, mapq=np.zeros(size, dtype=np.uint8))
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
        f(v, o, min_mapq=30)
    predicate_refusals(lambda **kw: f(v, o, mapq=q, **kw))
    offsets_refusals(lambda bad: f(v, bad, mapq=q, min_mapq=30), 20)


def test_device_pointer_refusals(no_library):
    f = sf.count_segments_device_ptr_filter
    o = np.array([0, 4, 10])
    with pytest.raises(ValueError, match=r"n must not be negative"):
        f(0x1000, -1, o)
    for name, args, kw in (("ptr", (4096.0, 10, o), {}), ("n", (0x1000, 10.0, o), {}), ("n", (0x1000, True, o), {}),
                           ("mapq_ptr", (0x1000, 10, o), {"mapq_ptr": None}), ("mapq_ptr", (0x1000, 10, o), {"mapq_ptr": 8192.0})):
        with pytest.raises(ValueError, match=r"%s must be an int, not" % name):
            f(*args, **kw)
    for name, args, kw in (("ptr", (1 << 64, 10, o), {}), ("ptr", (-8, 10, o), {}), ("n", (0x1000, 1 << 64, o), {}),
                           ("mapq_ptr", (0x1000, 10, o), {"mapq_ptr": 1 << 64})):
        with pytest.raises(ValueError, match=r"%s must fit an unsigned 64-bit integer, not" % name):
            f(*args, **kw)
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
        f(0x1000, 10, o, min_mapq=1)
    predicate_refusals(lambda **kw: f(0x1000, 10, o, mapq_ptr=0x2000, **kw))
    offsets_refusals(lambda bad: f(0x1000, 10, bad, mapq_ptr=0x2000, min_mapq=30), 10)


def test_torch_refusals(no_library):
    import torch
    f = sf.count_segments_torch_filter
    t = torch.zeros(20, dtype=torch.int16)
    q = torch.zeros(20, dtype=torch.uint8)
    o = torch.tensor([0, 7, 20], dtype=torch.int64)
    with pytest.raises(ValueError, match=r"t must be a torch\.Tensor, not ndarray"):
        f(np.zeros(20, dtype=np.uint16), o)
    for dt in (torch.int32, torch.int64, torch.uint8, torch.bool, torch.float16):
        with pytest.raises(ValueError, match=r"t must have dtype int16 or uint16, not " + re.escape(str(dt))):
            f(torch.zeros(20, dtype=dt), o)
    for bad in (torch.zeros((4, 5), dtype=torch.int16), torch.zeros(40, dtype=torch.int16)[::2]):
        with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
            f(bad, o)
    for bad in (np.array([0, 20]), torch.tensor([0, 20], dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int64),
                torch.zeros(0, dtype=torch.int64), torch.zeros(6, dtype=torch.int64)[::2]):
        with pytest.raises(ValueError, match=r"offsets must be a 1-D contiguous int64 tensor \(nseg \+ 1 values\)"):
            f(t, bad)
    with pytest.raises(ValueError, match=r"mapq must be a torch\.Tensor, not ndarray"):
        f(t, o, mapq=np.zeros(20, dtype=np.uint8), min_mapq=1)
    with pytest.raises(ValueError, match=r"mapq must have dtype torch\.uint8, not torch\.int8"):
        f(t, o, mapq=torch.zeros(20, dtype=torch.int8), min_mapq=1)
    with pytest.raises(ValueError, match=r"mapq must be 1-D and contiguous"):
        f(t, o, mapq=torch.zeros(40, dtype=torch.uint8)[::2], min_mapq=1)
    for size in (0, 19, 21):
        with pytest.raises(ValueError, match=r"mapq must have one element per value \(20\), not %d" % size):
            f(t, o, mapq=torch.zeros(size, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
        f(t, o, min_mapq=30)
    predicate_refusals(lambda **kw: f(t, o, mapq=q, **kw))
    for bad in (torch.zeros((3, 32), dtype=torch.int64), torch.zeros((2, 32), dtype=torch.int32), torch.zeros(64, dtype=torch.int64),
                np.zeros((2, 32), dtype=np.int64)):
        with pytest.raises(ValueError, match=r"out must be a contiguous int64 tensor of shape \(2, 32\)"):
            f(t, o, out=bad)
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int64), 0):
        with pytest.raises(ValueError, match=r"selected must be a contiguous int64 tensor of shape \(2,\)"):
            f(t, o, selected=bad)
    with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
        f(t, o, require=2, exclude=0x904, mapq=q, min_mapq=30)
    # (offsets / mapq / out / selected on another device than t: tests/test_gpu_segments_filter.py::test_refusals)


def test_segment_filter_dicts():
    rows = np.zeros((2, 32), dtype=np.uint64)
    rows[1, 2], rows[1, 18], rows[1, 25] = 3, 1, 2
    d = sf.segment_filter_dicts(rows, np.array([0, 10], dtype=np.uint64))
    assert [x["n_values"] for x in d] == [0, 10]
    assert int(d[1]["passed"]["mapped"]) == 10 - 3 - 1 and int(d[1]["failed"]["FQCFAIL"]) == 2
    for rows_, sel in ((rows, np.zeros(3)), (np.zeros((2, 31)), np.zeros(2)), (np.zeros(32), np.zeros(1))):
        with pytest.raises(ValueError, match=r"counters must be \[nseg, 32\] with nseg selected counts"):
            sf.segment_filter_dicts(rows_, sel)


def test_symbols_in_the_tables_the_library_and_the_headers():
    from libflagstats_amd import _lib
    for name in PUBLIC:
        assert name in _lib.SIGNATURES and name not in _lib.INTERNAL_SIGNATURES, name
    for name in INTERNAL:
        assert name in _lib.INTERNAL_SIGNATURES and name not in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_u16_segments_filter"][1]) == 12
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_u16_segments_filter_sync"][1]) == 11
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_u16_x64_segments_filter"][1]) == 11
    assert len(_lib.INTERNAL_SIGNATURES["fsk_launch_segments_filter"][1]) == 14
    for name in PUBLIC:
        args = _lib.SIGNATURES[name][1]
        assert args[1] is ctypes.c_uint64 and args[3] is ctypes.c_uint64, name                                  # n, nseg
        assert args[4] is ctypes.c_uint32 and args[5] is ctypes.c_uint32 and args[7] is ctypes.c_uint32, name   # require, exclude, min_mapq
    args = _lib.INTERNAL_SIGNATURES["fsk_launch_segments_filter"][1]
    assert [args[i] for i in (2, 3, 5)] == [ctypes.c_uint64] * 3 and [args[i] for i in (6, 7, 8, 12)] == [ctypes.c_uint32] * 4
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in PUBLIC + INTERNAL:
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    assert header.index("filtered segments:") > header.index("filtered: flagstat under samtools' view filter")
    for name in PUBLIC:
        m = re.search(r"\bint %s\(([^)]*)\)" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    csrc = os.path.join(ROOT, "libflagstats_amd", "csrc")
    for name in INTERNAL:
        declared = [h for h in sorted(os.listdir(csrc)) if h.endswith(".h") and re.search(r"\bhipError_t %s\(" % name, open(os.path.join(csrc, h)).read())]
        assert declared == ["flagstat_segments_filter.h"] and name not in header, (name, declared)
        m = re.search(r"\bhipError_t %s\(([^)]*)\)" % name, open(os.path.join(csrc, declared[0])).read())
        assert len(m.group(1).split(",")) == len(_lib.INTERNAL_SIGNATURES[name][1]), name


def test_code_objects():
    """K1's code object is still the one profiles/traffic.json was measured on; exactly one gfx950 code object defines
    fsk::flagstat_segments_filter, with and without the MAPQ column, and it is not K1's, the segmented, the wide, the where or the
    filter kernel's"""
    from libflagstats_amd import _lib, kernel_id
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        recorded = json.load(f)["kernel_source_id"]
    assert kernel_id.kernel_id(_lib.LIB_PATH) == recorded
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    found = {k: [] for k in ("k1", "segments", "wide", "where", "filter", "segments_filter")}
    for i, co in enumerate(kernel_id._code_objects(so)):
        secs = kernel_id._sections(co)
        names = b"".join(co[secs[t][0]:secs[t][0] + secs[t][1]] for t in (".strtab", ".dynstr") if t in secs)
        for key, prefix in (("k1", b"_ZN3fsk14flagstat_count"), ("segments", b"_ZN3fsk17flagstat_segmentsE"),
                            ("wide", b"_ZN3fsk19flagstat_count_wide"), ("where", b"_ZN3fsk20flagstat_count_where"),
                            ("filter", b"_ZN3fsk21flagstat_count_filter")):
            if prefix in names:
                found[key].append(i)
        if b"_ZN3fsk24flagstat_segments_filterILb0" in names:
            assert b"_ZN3fsk24flagstat_segments_filterILb1" in names
            found["segments_filter"].append(i)
        else:
            assert b"_ZN3fsk24flagstat_segments_filter" not in names
    assert all(len(v) == 1 for v in found.values()), found
    assert len({v[0] for v in found.values()}) == len(found), found


# ------------------------------------------------------------------ the oracle against a per-segment loop
LAYOUTS = {
    "whole": [0, 1000],
    "gaps and empties": [3, 3, 40, 40, 41, 500, 500, 997],
    "short": list(range(0, 1001, 7)) + [1000],
    "one flag each": list(range(100, 164)),
    "nothing": [17],
}
PREDICATES = ((0, 0), (0, 0x904), (0x2, 0x900), (0x1, 0xF04), (0x0101, 0x8080), (0x0040, 0x0040), (0xFFFF, 0), (0, 0xFFFF))


def test_oracle_against_a_per_segment_loop(oracle_mod):
    """segments_filter_oracle.want and .periodic_want on 1,000 values against where_oracle.want_counters (the C oracle on
    values[mask]) segment by segment: several layouts, predicates on one and both byte planes, an overlapping pair, thresholds on
    both sides of 128, with and without the superset slots"""
    rng = np.random.RandomState(11)
    v = rng.randint(0, 65536, 1000).astype(np.uint16)
    v[:200] &= np.uint16(0x06FF)                    # values that pass predicates with many excluded bits
    v[200:230] = 0
    q = rng.randint(0, 256, 1000).astype(np.uint8)
    q[:8] = (0, 1, 29, 30, 127, 128, 129, 255)
    pattern, mq_pattern = v[:997], q[:997]          # a prime period for the periodic form
    any_selected = any_overlap = False
    for name, o in LAYOUTS.items():
        o = np.array(o, dtype=np.int64)
        for require, exclude in PREDICATES:
            for min_mapq in (0, 1, 30, 127, 128, 129, 255):
                mask = filter_mask(v, require, exclude, q, min_mapq)
                for superset in (False, True):
                    rows, selected = sfo.want(v, o, require, exclude, q, min_mapq, superset)
                    assert rows.dtype == np.uint64 and rows.shape == (o.size - 1, 32) and selected.dtype == np.uint64
                    for i in range(o.size - 1):
                        inside = np.zeros(1000, dtype=bool)
                        inside[o[i]:o[i + 1]] = True
                        w = where_oracle.want_counters(oracle_mod, v, mask & inside, superset)
                        assert np.array_equal(rows[i], w), (name, require, exclude, min_mapq, superset, i, rows[i], w)
                        assert int(selected[i]) == int((mask & inside).sum())
                    any_selected |= bool(selected.any())
                    if require & exclude:
                        any_overlap = True
                        assert not rows.any() and not selected.any()
                # the periodic form: 3 periods and a bit, shifted by a phase, against the materialised array
                for phase in (0, 5):
                    big = np.resize(np.roll(pattern, -phase), 3200)
                    big_q = np.resize(np.roll(mq_pattern, -phase), 3200)
                    oo = np.array([0, 1, 996, 997, 998, 1994, 1994, 3100, 3200], dtype=np.int64)
                    rows, selected = sfo.periodic_want(pattern, oo, require, exclude, mq_pattern, min_mapq, True, phase)
                    rows2, selected2 = sfo.want(big, oo, require, exclude, big_q, min_mapq, True)
                    assert np.array_equal(rows, rows2) and np.array_equal(selected, selected2), (name, require, exclude, min_mapq, phase)
    assert any_selected and any_overlap
    rows, selected = sfo.want(v, [0, 1000], 0, 0, None, 0, True)
    assert int(selected[0]) == 1000 and np.array_equal(rows[0], where_oracle.want_counters(oracle_mod, v, np.ones(1000, dtype=bool), True))
