"""Filtered segmented flagstat on int32 / int64 columns (libflagstats_amd/segments_wide_filter.py,
csrc/flagstat_segments_wide_filter.hip) on the CPU: the package's exports, the prototypes in the binding table, the library and
both headers, every refusal that comes before the GPU is touched (text checked, outputs left alone), the oracle against a
brute-force loop and against wide_filter_oracle, the writer mirror against the new source, and the C entries' loud failure on a
box without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_wide_filter_oracle as swfo  # noqa: E402
import wide_filter_oracle  # noqa: E402

from libflagstats_amd import segments_wide_filter as swf  # noqa: E402  (fails at import where the feature is missing)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libflagstats_amd", "csrc")
PUBLIC = {"FLAGSTATS_hip_device_wide_segments_filter": 14, "FLAGSTATS_hip_device_wide_segments_filter_sync": 13,
          "FLAGSTATS_hip_wide_x64_segments_filter": 13}
LAUNCHER = "fsk_launch_segments_wide_filter"
PY_NAMES = ("counters_segments_ints_filter", "flagstats_segments_ints_filter", "count_segments_device_ptr_ints_filter",
            "count_segments_torch_ints_filter")
DTYPES = (np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64)


@pytest.fixture()
def no_library(monkeypatch):
    """loading the library fails the test: the refusals must come first"""
    from libflagstats_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were refused")

    monkeypatch.setattr(_lib, "lib", boom)


def test_exports_and_shared_checks():
    import libflagstats_amd
    from libflagstats_amd import filter, segments, segments_filter, segments_wide, wide
    for name in PY_NAMES:
        assert getattr(libflagstats_amd, name) is getattr(swf, name) and name in libflagstats_amd.__all__
    assert len(set(libflagstats_amd.__all__)) == len(libflagstats_amd.__all__)
    assert "segments_wide_filter" in libflagstats_amd.__doc__
    # the checks and the shaping are the other modules', not restated
    assert swf.check_offsets is segments.check_offsets and swf._check_values is wide._check_values
    assert swf._check_tensor is wide._check_tensor and swf.strict_message is segments_wide.strict_message
    assert swf._check_predicate is filter._check_predicate and swf._check_mapq_torch is filter._check_mapq_torch
    assert swf._check_mapq_numpy is filter._check_mapq_numpy
    assert swf.count_segments_torch_filter is segments_filter.count_segments_torch_filter
    assert not [n for n in dir(swf) if n.endswith("_dicts")]       # segment_filter_dicts is reused, no fifth shaping function
    rows = np.zeros((2, 32), dtype=np.uint64)
    assert [d["n_values"] for d in libflagstats_amd.segment_filter_dicts(rows, [5, 0])] == [5, 0]


def test_prototypes_in_the_table_the_library_and_both_headers():
    from libflagstats_amd import _lib
    for name, nargs in PUBLIC.items():
        assert name in _lib.SIGNATURES and name not in _lib.INTERNAL_SIGNATURES, name
        args = _lib.SIGNATURES[name][1]
        assert len(args) == nargs and _lib.SIGNATURES[name][0] is ctypes.c_int, name
        # n, elem_bytes, nseg, require, exclude, min_mapq, flags
        assert args[1] is ctypes.c_uint64 and args[2] is ctypes.c_int and args[4] is ctypes.c_uint64, name
        assert args[5] is ctypes.c_uint32 and args[6] is ctypes.c_uint32 and args[8] is ctypes.c_uint32 and args[12] is ctypes.c_int, name
    assert len(_lib.INTERNAL_SIGNATURES[LAUNCHER][1]) == 16 and LAUNCHER not in _lib.SIGNATURES
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in tuple(PUBLIC) + (LAUNCHER,):
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    assert header.index("filtered wide input per segment:") > header.index("wide input per segment:")
    for name, nargs in PUBLIC.items():
        m = re.search(r"\bint %s\(([^)]*)\)" % name, header)
        assert m and len(m.group(1).split(",")) == nargs, name
    # the launcher is declared in the new internal header and nowhere else
    for fn in sorted(os.listdir(CSRC)) + [os.path.join(ROOT, "include", "libflagstats_hip.h"),
                                          os.path.join(ROOT, "include", "libflagstats_hip_probe.h")]:
        if not fn.endswith(".h"):
            continue
        text = open(os.path.join(CSRC, fn)).read()
        m = re.search(r"\bhipError_t %s\(([^)]*)\)" % LAUNCHER, text)
        if os.path.basename(fn) == "flagstat_segments_wide_filter.h":
            assert m and len(m.group(1).split(",")) == 16
        else:
            assert LAUNCHER not in text, fn
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1)
    hdrs = re.search(r"^HDRS\s*:=(.*)$", mk, re.M).group(1)
    assert "$(HERE)flagstat_segments_wide_filter.hip" in srcs.split()
    for h in ("flagstat_segments_wide_filter.h", "flagstat_segments_wide_device.h", "flagstat_wide_filter_device.h"):
        assert "$(HERE)" + h in hdrs.split(), h


def test_code_objects():
    """K1's code object is the one profiles/traffic.json was measured on; one gfx950 code object defines the four
    fsk::flagstat_segments_wide_filter instantiations and no other unit's kernel"""
    import json

    from libflagstats_amd import _lib, kernel_id
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        assert kernel_id.kernel_id(_lib.LIB_PATH) == json.load(f)["kernel_source_id"]
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    holders = 0
    for co in kernel_id._code_objects(so):
        secs = kernel_id._sections(co)
        names = b"".join(co[secs[t][0]:secs[t][0] + secs[t][1]] for t in (".strtab", ".dynstr") if t in secs)
        if b"_ZN3fsk29flagstat_segments_wide_filterI" not in names:
            continue
        holders += 1
        for inst in (b"Li4ELb0E", b"Li4ELb1E", b"Li8ELb0E", b"Li8ELb1E"):
            assert b"_ZN3fsk29flagstat_segments_wide_filterI" + inst in names, inst
        for other in (b"_ZN3fsk14flagstat_count", b"_ZN3fsk17flagstat_segmentsE", b"_ZN3fsk19flagstat_count_wide",
                      b"_ZN3fsk24flagstat_segments_filter", b"_ZN3fsk26flagstat_count_wide_filter", b"_ZN3fsk22flagstat_segments_wideI"):
            assert other not in names, other
    assert holders == 1


# ------------------------------------------------------------------ refusals of the Python layer, before the library is loaded
BAD_OFFSETS = (([0, 5, 3, 10], "non-decreasing"), ([0, 5, 11], "exceeds"), (np.array([[0, 5], [5, 10]]), "1-D"),
               (np.array([0.0, 5.0, 10.0]), "integer"), (np.array([-1, 5, 10], dtype=np.int64), "negative"),
               (np.array([], dtype=np.uint64), ">= 1"))
BAD_PREDICATES = ((dict(require=0x10000), "require must be a 16-bit FLAG mask"), (dict(exclude=-1), "exclude must be a 16-bit FLAG mask"),
                  (dict(min_mapq=256, mapq="q"), r"min_mapq must be in 0\.\.255"), (dict(min_mapq=30), "min_mapq > 0 needs mapq"),
                  (dict(require=1.5), "require"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_layers_refuse_before_the_library_is_touched(no_library, dtype):
    values = np.zeros(10, dtype=dtype)
    q = np.zeros(10, dtype=np.uint8)
    for f in (swf.counters_segments_ints_filter, swf.flagstats_segments_ints_filter):
        for offsets, why in BAD_OFFSETS:
            with pytest.raises(ValueError, match=why):
                f(values, offsets)
        for kw, why in BAD_PREDICATES:
            kw = {k: (q if isinstance(v, str) else v) for k, v in kw.items()}
            with pytest.raises(ValueError, match=why):
                f(values, [0, 10], **kw)
        with pytest.raises(ValueError, match=r"values must be a numpy\.ndarray, not list"):
            f([1, 2, 3], [0, 3])
        for bad in (np.zeros(10, dtype=np.int8), np.zeros(10, dtype=np.float32)):
            with pytest.raises(ValueError, match=r"values must have an integer dtype of 2, 4 or 8 bytes"):
                f(bad, [0, 10])
        with pytest.raises(ValueError, match=r"values must be 1-D, not 2-D"):
            f(np.zeros((2, 5), dtype=dtype), [0, 10])
        with pytest.raises(ValueError, match=r"mapq must be a numpy\.ndarray, not list"):
            f(values, [0, 10], mapq=[0] * 10)
        with pytest.raises(ValueError, match=r"mapq must have dtype uint8, not int8"):
            f(values, [0, 10], mapq=np.zeros(10, dtype=np.int8))
        with pytest.raises(ValueError, match=r"mapq must have one element per value \(10\), not 9"):
            f(values, [0, 10], mapq=np.zeros(9, dtype=np.uint8))
        with pytest.raises(ValueError, match=r"mapq must be 1-D, not 2-D"):
            f(values, [0, 10], mapq=np.zeros((2, 5), dtype=np.uint8))


def test_device_pointer_and_torch_refusals(no_library):
    import torch
    f = swf.count_segments_device_ptr_ints_filter
    o = np.array([0, 4, 10])
    for eb in (2, 1, 16, 0, None):
        with pytest.raises(ValueError, match=r"elem_bytes must be 4 or 8 \(16-bit arrays: segments_filter\.count_segments_device_ptr_filter\)"):
            f(0x1000, 10, eb, o)
    with pytest.raises(ValueError, match=r"n must not be negative"):
        f(0x1000, -1, 4, o)
    with pytest.raises(ValueError, match=r"mapq_ptr must be an int, not float"):
        f(0x1000, 10, 4, o, mapq_ptr=1.0)
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
        f(0x1000, 10, 4, o, min_mapq=3)
    with pytest.raises(ValueError, match=r"exclude must be a 16-bit FLAG mask"):
        f(0x1000, 10, 8, o, exclude=1 << 16)
    for offsets, why in BAD_OFFSETS:
        with pytest.raises(ValueError, match=why):
            f(0x1000, 10, 8, offsets)
    g = swf.count_segments_torch_ints_filter
    t = torch.zeros(20, dtype=torch.int32)
    off = torch.tensor([0, 7, 20], dtype=torch.int64)
    with pytest.raises(ValueError, match=r"t must be a torch\.Tensor, not ndarray"):
        g(np.zeros(20, dtype=np.int32), off)
    for dt in (torch.uint8, torch.bool, torch.float32):
        with pytest.raises(ValueError, match=r"t must have an integer dtype of 2, 4 or 8 bytes"):
            g(torch.zeros(20, dtype=dt), off)
    with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
        g(torch.zeros(40, dtype=torch.int32)[::2], off)
    for bad in (np.array([0, 20]), torch.tensor([0, 20], dtype=torch.int32), torch.zeros(0, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"offsets must be a 1-D contiguous int64 tensor \(nseg \+ 1 values\)"):
            g(t, bad)
    # mapq: count_torch_ints_filter's checks
    with pytest.raises(ValueError, match=r"mapq must be a torch\.Tensor, not ndarray"):
        g(t, off, mapq=np.zeros(20, dtype=np.uint8))
    with pytest.raises(ValueError, match=r"mapq must have dtype torch\.uint8, not torch\.int8"):
        g(t, off, mapq=torch.zeros(20, dtype=torch.int8))
    with pytest.raises(ValueError, match=r"mapq must be 1-D and contiguous"):
        g(t, off, mapq=torch.zeros(40, dtype=torch.uint8)[::2])
    with pytest.raises(ValueError, match=r"mapq must have one element per value \(20\), not 19"):
        g(t, off, mapq=torch.zeros(19, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
        g(t, off, min_mapq=30)
    with pytest.raises(ValueError, match=r"require must be a 16-bit FLAG mask"):
        g(t, off, require=70000)
    for bad in (torch.zeros((3, 32), dtype=torch.int64), torch.zeros((2, 32), dtype=torch.int32), np.zeros((2, 32), dtype=np.int64)):
        with pytest.raises(ValueError, match=r"out must be a contiguous int64 tensor of shape \(2, 32\)"):
            g(t, off, out=bad)
    for name in ("selected", "high"):
        for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int64), 0):
            with pytest.raises(ValueError, match=r"%s must be a contiguous int64 tensor of shape \(2,\)" % name):
                g(t, off, **{name: bad})
    with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
        g(t, off, mapq=torch.zeros(20, dtype=torch.uint8), min_mapq=1)


def test_strict_names_the_first_offending_segment(monkeypatch):
    o = np.array([3, 10, 10, 25, 40], dtype=np.int64)
    rows, sel = np.zeros((4, 32), dtype=np.uint64), np.arange(4, dtype=np.uint64)
    calls = []

    def fake(values, offsets, **kw):
        calls.append(kw)
        return rows, sel, fake.high

    monkeypatch.setattr(swf, "counters_segments_ints_filter", fake)
    fake.high = np.array([0, 0, 0x80000000, 0x10000], dtype=np.uint64)
    with pytest.raises(ValueError, match=re.escape("segment 2 (offsets 10..25): values outside 0..65535: bits 0x80000000 set above bit 15")):
        swf.flagstats_segments_ints_filter(np.zeros(40, dtype=np.int32), o, exclude=0x904)
    got = swf.flagstats_segments_ints_filter(np.zeros(40, dtype=np.int32), o, require=2, exclude=0x904, superset=True, strict=False)
    assert got[0] is rows and got[1] is sel and got[2] is fake.high
    assert calls[1] == dict(require=2, exclude=0x904, mapq=None, min_mapq=0, superset=True)
    fake.high = np.zeros(4, dtype=np.uint64)
    assert swf.flagstats_segments_ints_filter(np.zeros(40, dtype=np.int64), o)[2] is fake.high


# ------------------------------------------------------------------ refusals of the C entries that come before the GPU is touched
def c_calls(lib, a, W, o, nseg, req, exc, q, mq, out, sel, high, flags):
    ap = a if isinstance(a, int) or a is None else a.ctypes.data
    qp = q if isinstance(q, int) or q is None else q.ctypes.data
    op = None if o is None else o.ctypes.data
    outp = None if out is None else out.ctypes.data
    n = 100
    return (("x64", lambda: lib.FLAGSTATS_hip_wide_x64_segments_filter(ap, n, W, op, nseg, req, exc, qp, mq, outp, sel.ctypes.data,
                                                                       high.ctypes.data, flags)),
            ("sync", lambda: lib.FLAGSTATS_hip_device_wide_segments_filter_sync(ap, n, W, op, nseg, req, exc, qp, mq, outp,
                                                                                sel.ctypes.data, high.ctypes.data, flags)),
            ("device", lambda: lib.FLAGSTATS_hip_device_wide_segments_filter(ap, n, W, op, nseg, req, exc, qp, mq, outp,
                                                                             sel.ctypes.data, high.ctypes.data, flags, None)))


def test_c_entries_refuse_before_the_gpu_and_leave_the_outputs_alone():
    from libflagstats_amd import _lib
    lib = _lib.lib()
    o = np.array([0, 40, 100], dtype=np.uint64)
    out = np.full((2, 32), 7, dtype=np.uint64)
    sel = np.full(2, 7, dtype=np.uint64)
    high = np.full(2, 7, dtype=np.uint64)
    a = np.arange(104, dtype=np.int64)
    q = np.zeros(100, dtype=np.uint8)
    ok = dict(a=a, W=8, o=o, nseg=2, req=0, exc=0, q=q, mq=0, out=out, sel=sel, high=high, flags=1)
    cases = (
        (dict(W=2), r"elem_bytes 2: 16-bit arrays go to the u16 segmented filter entries \(FLAGSTATS_hip_u16_x64_segments_filter, "
                    r"FLAGSTATS_hip_device_u16_segments_filter\)"),
        (dict(W=3), "elem_bytes must be 4 or 8"), (dict(W=16), "elem_bytes must be 4 or 8"),
        (dict(req=0x10000), "require must be a 16-bit FLAG mask"), (dict(exc=0x10000), "exclude must be a 16-bit FLAG mask"),
        (dict(mq=256), "min_mapq must be at most 255"), (dict(flags=4), "flags: bit 0 store, bit 1 superset; no other bits"),
        (dict(o=None), "NULL d?_?offsets or d?_?out with nseg > 0"), (dict(out=None), "NULL d?_?offsets or d?_?out with nseg > 0"),
        (dict(nseg=(1 << 64) // 256), "nseg is too large"), (dict(a=None), "NULL array with n > 0"),
        (dict(q=None, mq=30), "NULL mapq with min_mapq > 0 and n > 0"),
        (dict(a=a.ctypes.data + 4), r"array must be 8-byte aligned \(elem_bytes 8\)"),
        (dict(a=a.ctypes.data + 2, W=4), r"array must be 4-byte aligned \(elem_bytes 4\)"),
    )
    for change, text in cases:
        for name, call in c_calls(lib, **{**ok, **change}):
            assert call() != 0, (change, name)
            assert re.search(text, lib.FLAGSTATS_hip_last_error().decode()), (change, name, lib.FLAGSTATS_hip_last_error())
            assert (out == 7).all() and (sel == 7).all() and (high == 7).all(), (change, name)
    # n * elem_bytes is not a size
    rc = lib.FLAGSTATS_hip_wide_x64_segments_filter(a.ctypes.data, (1 << 64) // 8, 8, o.ctypes.data, 2, 0, 0, None, 0, out.ctypes.data,
                                                    sel.ctypes.data, high.ctypes.data, 1)
    assert rc != 0 and b"n * elem_bytes is not a size" in lib.FLAGSTATS_hip_last_error()
    # nseg == 0 does nothing and succeeds, GPU or not, whatever the pointers
    for name, call in c_calls(lib, **{**ok, "nseg": 0}):
        assert call() == 0, name
    for name, call in c_calls(lib, **{**ok, "nseg": 0, "o": None, "out": None, "a": None}):
        assert call() == 0, name
    assert (out == 7).all() and (sel == 7).all() and (high == 7).all()


def test_no_gpu_means_the_entries_fail_loudly():
    """Without a GPU the three entries return non-zero with a message and leave the outputs alone; nothing is computed on the CPU.
    (With one, tests/test_gpu_segments_wide_filter.py runs them.)"""
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
        for mq in (0, 30):
            for name, call in c_calls(lib, a, a.dtype.itemsize, o, 2, 0, 0x904, q, mq, out, sel, high, 1):
                assert call() != 0, name
                assert lib.FLAGSTATS_hip_last_error(), name
                assert (out == 7).all() and (sel == 7).all() and (high == 7).all(), name
        with pytest.raises(_lib.FlagstatsHipError):
            swf.counters_segments_ints_filter(a, o, exclude=0x904)
        with pytest.raises(_lib.FlagstatsHipError):
            swf.count_segments_device_ptr_ints_filter(a.ctypes.data, a.size, a.dtype.itemsize, o, mapq_ptr=q.ctypes.data, min_mapq=3)


# ------------------------------------------------------------------ the oracle itself
def wide_column(rng, n, dtype, every=37):
    W = np.dtype(dtype).itemsize
    u = rng.randint(0, 65536, n).astype(np.uint64)
    hot = rng.randint(0, every, n) == 0
    hi = rng.randint(0, 1 << 16, n).astype(np.uint64) << np.uint64(16)
    if W == 8:
        hi |= rng.randint(0, 1 << 32, n).astype(np.uint64) << np.uint64(32)
    u |= np.where(hot, hi, np.uint64(0)).astype(np.uint64)
    return u.astype(np.uint32 if W == 4 else np.uint64).view(dtype)


PREDICATES = ((0, 0, 0), (0, 0x904, 0), (2, 0x904, 0), (4, 0x904, 0), (0, 0, 30), (1, 0x904, 30), (0xFFFF, 0, 0))


@pytest.mark.parametrize("dtype", DTYPES[2:])
def test_oracle_against_a_brute_force_loop_and_wide_filter_oracle(oracle_mod, dtype):
    rng = np.random.RandomState(11)
    n = 30_000
    x = wide_column(rng, n, dtype)
    x[:200] = (0xFFFF | (1 << 20))      # some elements pass require = 0xFFFF
    mapq = rng.randint(0, 256, n).astype(np.uint8)
    lengths = rng.choice([0, 0, 1, 2, 3, 5, 100, 1000, 2047, 2048, 2049], 30)
    o = 13 + np.concatenate([[0], np.cumsum(lengths)])
    assert o[-1] + 9 <= n
    bits = 8 * np.dtype(dtype).itemsize
    for req, exc, mq in PREDICATES:
        for sup in (False, True):
            rows, sel, high = swfo.want(x, o, req, exc, mapq, mq, sup)
            assert rows.shape == (30, 32) and sel.shape == (30,) and high.shape == (30,) and high.dtype == np.uint64
            for i in range(30):
                a, qa = x[o[i]:o[i + 1]], mapq[o[i]:o[i + 1]]
                passing, mask = [], 0
                for v, qq in zip(a.tolist(), qa.tolist()):
                    u = v & ((1 << bits) - 1)
                    mask |= u & ~0xFFFF
                    f = u & 0xFFFF
                    if (f & req) == req and (f & exc) == 0 and (mq == 0 or qq >= mq):
                        passing.append(f)
                lo = np.array(passing, dtype=np.uint16)
                w = oracle_mod.flagstat_hist(lo).copy()
                if sup:
                    pp = ((lo & 0x100) == 0) & ((lo & 0x800) == 0) & ((lo & 1) == 1)
                    fail = (lo & 0x200) != 0
                    w[0], w[16], w[9] = int((pp & ~fail).sum()), int((pp & fail).sum()), lo.size - int(fail.sum())
                assert np.array_equal(rows[i], w), (req, exc, mq, sup, i)
                assert int(sel[i]) == len(passing)
                assert int(high[i]) == (0 if req & exc else mask), (i, hex(int(high[i])), hex(mask))
            if not (req & exc):
                assert 0 < int(sel.sum()) and (int(sel.sum()) < int(np.diff(o).sum()) or (req, exc, mq) == (0, 0, 0))
            # one segment: wide_filter_oracle
            c1, s1, h1 = wide_filter_oracle.want(oracle_mod, x[5:n - 3], req, exc, mapq[5:n - 3], mq, sup)
            r, s, h = swfo.want(x, [5, n - 3], req, exc, mapq, mq, sup)
            assert np.array_equal(r[0], c1) and int(s[0]) == s1 and int(h[0]) == (0 if req & exc else h1)
    # the periodic form against the materialised arrays: coprime prime periods, and one joint period
    pattern, mqp = x[:997], mapq[:13]
    for phase in (0, 5):
        big = np.resize(np.roll(pattern, -phase), 14_000)
        bigq = np.resize(np.roll(np.resize(mqp, 997 * 13), -phase), 14_000)
        oo = np.array([0, 1, 996, 997, 998, 1994, 1994, 13_100, 14_000], dtype=np.int64)
        for req, exc, mq in ((0, 0x904, 0), (1, 0x904, 30), (4, 4, 0)):
            got = swfo.periodic_want(pattern, oo, req, exc, mqp, mq, True, phase)
            ref = swfo.want(big, oo, req, exc, bigq, mq, True)
            assert all(np.array_equal(g, w) for g, w in zip(got, ref)), (phase, req, exc, mq)
    got = swfo.periodic_want(pattern, [0, 3000], 0, 0x904, mapq[:997], 30, False, 0)
    ref = swfo.want(np.resize(pattern, 3000), [0, 3000], 0, 0x904, np.resize(mapq[:997], 3000), 30, False)
    assert all(np.array_equal(g, w) for g, w in zip(got, ref))
    assert [a.shape for a in swfo.want(x, [5], 0, 0x904)] == [(0, 32), (0,), (0,)]


def test_writer_mirror_matches_the_new_source():
    """the writer-split rules, read out of flagstat_segments_wide_filter.hip: WideWriterSplit describes this kernel's writers too"""
    src = re.sub(r"\s+", " ", open(os.path.join(CSRC, "flagstat_segments_wide_filter.hip")).read())
    parent = re.sub(r"\s+", " ", open(os.path.join(CSRC, "flagstat_segments_wide.hip")).read())
    hdr = open(os.path.join(CSRC, "flagstat_segments_wide.h")).read()
    assert int(re.search(r"constexpr int kSegWideUnitBytes = (\d+);", hdr).group(1)) == swfo.UNIT_BYTES
    assert (1 << int(re.search(r"constexpr int kSegWideFilterDepth = (\d+);", src).group(1))) - 1 == swfo.SEG_EPOCH
    # the parent's walk is the segmented kernels' shared one (seg_walk<UE> of flagstat_segments_shared.h); this kernel keeps a
    # walk of its own (HISTORY.md), which must state the same rules; the launcher's shape is the shared one for both
    shared = re.sub(r"\s+", " ", open(os.path.join(CSRC, "flagstat_segments_shared.h")).read())
    assert "seg_walk<UE>( lo0, hi0, base," in parent and "seg_walk<UE>(" not in src
    for rule in ("const uint64_t W = fsk::kSegUnitVecs * 16 / ue;",
                 "*lo0 = (addr & 15u) / W;",
                 "*nunits = (*lo0 + m + ue - 1) / ue;",
                 "const uint64_t want = (*nunits + 3) / 4;",
                 "*g = want < grid ? static_cast<uint32_t>(want) : grid;"):
        assert shared.count(rule) == 1, rule
    for rule in ("const uint64_t u_begin = gw * nunits / waves, u_end = (gw + 1) * nunits / waves;",
                 "const uint64_t p0 = u_begin * UE > lo0 ? u_begin * UE : lo0;",
                 "const uint64_t E = u_end * UE < hi0 ? u_end * UE : hi0;",
                 "if (sb >= E) break; if (se <= sb || se <= x) {",
                 "if (sb <= w0 && w0 >= lo0) { const uint64_t k = (seg_e - w0) / UE;",
                 "if (k >= min_units && k > 0) {",
                 "(mode & 1) && b_ >= p0 && e_ <= E"):
        assert rule in src and shared.count(rule) == 1, rule
    for rule in ("constexpr uint64_t UE = kSegWideUnitBytes / W;",
                 "fsseg::launch_shape(addr, m, fsk::kSegWideUnitBytes / W, grid, &lo0, &nunits, &g);",
                 "fsk_segments_policy(&min_units, &blocks_per_cu);"):
        assert rule in src and rule in parent, rule
    assert "end_step<kSegWideFilterDepth>(s, blk);" in src
    # the shared pieces are included, not restated
    for name in ("mask_vec_wide(uint4", "valid_bits_wide(uint64_t", "load_mapq_wide_guarded(const", "void wide_filter_step_with(",
                 "void count_piece_wide_with("):
        holders = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip")) and name in open(os.path.join(CSRC, fn)).read()]
        assert len(holders) == 1 and holders[0].endswith("_device.h"), (name, holders)
