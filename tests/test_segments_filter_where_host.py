"""The filtered and selected segmented flagstat (libflagstats_amd/segments_filter_where.py,
csrc/flagstat_segments_filter_where.hip) on the CPU: the package's exports, every refusal of the Python layer -- raised before
the library is loaded --, the symbols in the binding tables, the built library and the headers, the identity of the code
objects, and segments_filter_where_oracle against a per-element, per-segment loop and against compaction.  (The unit takes the
segmented kernels' shared walk as it is, so there is no copy of the walk to hold to it here.)"""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_filter_where_oracle as sfwo  # noqa: E402
import where_oracle  # noqa: E402
from test_filter_where_host import bit_offset_refusals, no_library, predicate_refusals  # noqa: E402,F401  (no_library: a fixture)
from test_segments_where_host import offsets_refusals  # noqa: E402
from where_oracle import pack  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ("FLAGSTATS_hip_device_u16_segments_filter_where", "FLAGSTATS_hip_device_u16_segments_filter_where_sync",
          "FLAGSTATS_hip_u16_x64_segments_filter_where")
INTERNAL = ("fsk_launch_segments_filter_where",)
PY_NAMES = ("counters_segments_filter_where", "flagstats_segments_filter_where", "count_segments_device_ptr_filter_where",
            "count_segments_torch_filter_where")
KERNEL = b"_ZN3fsk30flagstat_segments_filter_where"
FORMS = tuple(b"ILb%dELi%dELb%dE" % f for f in ((0, 1, 0), (0, 1, 1), (1, 1, 0), (1, 1, 1), (1, 8, 0)))   # <MAPQ, SEL_BITS, FUNNEL>
OTHERS = {"K1": b"_ZN3fsk14flagstat_count", "filter_where": b"_ZN3fsk21flagstat_filter_where",
          "segments_filter": b"_ZN3fsk24flagstat_segments_filter", "segments_where": b"_ZN3fsk23flagstat_segments_where"}


def test_exports():
    import libflagstats_amd
    from libflagstats_amd import segments_filter_where as sfw
    for name in PY_NAMES:
        assert getattr(libflagstats_amd, name) is getattr(sfw, name) and name in libflagstats_amd.__all__
    assert "segments_filter_where" in libflagstats_amd.__doc__


@pytest.mark.parametrize("fn", ["counters_segments_filter_where", "flagstats_segments_filter_where"])
def test_numpy_refusals(no_library, fn):  # noqa: F811
    from libflagstats_amd import segments_filter_where as sfw
    f = getattr(sfw, fn)
    v = np.zeros(20, dtype=np.uint16)
    q = np.zeros(20, dtype=np.uint8)
    m = np.ones(20, dtype=bool)
    bits = np.zeros(4, dtype=np.uint8)
    o = np.array([0, 7, 20])
    with pytest.raises(ValueError, match=r"values must be a numpy\.ndarray, not list"):
        f([1, 2, 3], o, m)
    for bad in (np.zeros(20, dtype=np.int16), np.zeros(20, dtype=np.int32), np.zeros(20, dtype=np.uint8), np.zeros(20, dtype=bool)):
        with pytest.raises(ValueError, match=r"values must have dtype uint16, not " + re.escape(str(bad.dtype))):
            f(bad, o, m)
    with pytest.raises(ValueError, match=r"values must be 1-D, not 2-D"):
        f(np.zeros((4, 5), dtype=np.uint16), o, m)
    # the selection
    with pytest.raises(ValueError, match=r"where must be a numpy\.ndarray, not list"):
        f(v, o, [True] * 20)
    with pytest.raises(ValueError, match=r"where must be a numpy\.ndarray, not NoneType"):
        f(v, o, None)
    with pytest.raises(ValueError, match=r"where must be 1-D, not 2-D"):
        f(v, o, np.ones((4, 5), dtype=bool))
    for bad in (np.ones(20, dtype=np.uint8), np.ones(20, dtype=np.int8), np.ones(20, dtype=np.float32)):
        with pytest.raises(ValueError, match=r"where must have dtype bool \(packed=True: a uint8 bitmap\), not " + re.escape(str(bad.dtype))):
            f(v, o, bad)
    for size in (0, 19, 21):
        with pytest.raises(ValueError, match=r"where must have one element per value \(20\), not %d" % size):
            f(v, o, np.ones(size, dtype=bool))
    for bad in (np.ones(4, dtype=bool), np.ones(4, dtype=np.int8), np.ones(4, dtype=np.uint16)):
        with pytest.raises(ValueError, match=r"where must have dtype uint8 with packed=True \(an LSB-first bitmap\), not " + re.escape(str(bad.dtype))):
            f(v, o, bad, packed=True)
    with pytest.raises(ValueError, match=r"where holds 2 bytes, 20 values from bit 0 on need 3"):
        f(v, o, np.zeros(2, dtype=np.uint8), packed=True)
    with pytest.raises(ValueError, match=r"where holds 3 bytes, 20 values from bit 5 on need 4"):
        f(v, o, np.zeros(3, dtype=np.uint8), packed=True, bit_offset=5)
    bit_offset_refusals(lambda packed, **kw: f(v, o, bits if packed else m, packed=packed, **kw))
    # the column
    with pytest.raises(ValueError, match=r"mapq must be a numpy\.ndarray, not list"):
        f(v, o, m, mapq=[0] * 20, min_mapq=1)
    for bad in (np.zeros(20, dtype=np.int8), np.zeros(20, dtype=bool), np.zeros(20, dtype=np.uint16), np.zeros(20, dtype=np.float32)):
        with pytest.raises(ValueError, match=r"mapq must have dtype uint8, not " + re.escape(str(bad.dtype))):
            f(v, o, m, mapq=bad, min_mapq=1)
    with pytest.raises(ValueError, match=r"mapq must be 1-D, not 2-D"):
        f(v, o, m, mapq=np.zeros((4, 5), dtype=np.uint8), min_mapq=1)
    for size in (0, 19, 21):
        with pytest.raises(ValueError, match=r"mapq must have one element per value \(20\), not %d" % size):
            f(v, o, m, mapq=np.zeros(size, dtype=np.uint8))
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
        f(v, o, m, min_mapq=30)
    predicate_refusals(lambda **kw: f(v, o, m, mapq=q, **kw))
    predicate_refusals(lambda **kw: f(v, o, bits, mapq=q, packed=True, bit_offset=7, **kw))
    # the offsets
    offsets_refusals(lambda bad: f(v, bad, m), 20)
    offsets_refusals(lambda bad: f(v, bad, bits, require=2, exclude=0x904, mapq=q, min_mapq=30, packed=True, bit_offset=2), 20)


def test_device_pointer_refusals(no_library):  # noqa: F811
    from libflagstats_amd import segments_filter_where as sfw
    f = sfw.count_segments_device_ptr_filter_where
    o = [0, 3, 10]
    for bad in (0, 2, 16, True, None, "1"):
        with pytest.raises(ValueError, match=r"sel_bits must be 1 \(an LSB-first bitmap\) or 8 \(one byte per element\), not"):
            f(0x1000, 10, o, 0x3000, bad)
    with pytest.raises(ValueError, match=r"n must not be negative"):
        f(0x1000, -1, o, 0x3000, 1)
    with pytest.raises(ValueError, match=r"sel_offset must not be negative"):
        f(0x1000, 10, o, 0x3000, 1, sel_offset=-1)
    for name, args, kw in (("ptr", (4096.0, 10, o, 0x3000, 8), {}), ("n", (0x1000, 10.0, o, 0x3000, 8), {}),
                           ("n", (0x1000, True, o, 0x3000, 8), {}), ("sel_ptr", (0x1000, 10, o, None, 8), {}),
                           ("sel_ptr", (0x1000, 10, o, 12288.0, 1), {}), ("sel_offset", (0x1000, 10, o, 0x3000, 1), {"sel_offset": 1.0}),
                           ("mapq_ptr", (0x1000, 10, o, 0x3000, 8), {"mapq_ptr": None}),
                           ("mapq_ptr", (0x1000, 10, o, 0x3000, 8), {"mapq_ptr": 8192.0})):
        with pytest.raises(ValueError, match=r"%s must be an int, not" % name):
            f(*args, **kw)
    for name, args, kw in (("ptr", (1 << 64, 10, o, 0x3000, 8), {}), ("ptr", (-8, 10, o, 0x3000, 8), {}),
                           ("n", (0x1000, 1 << 64, o, 0x3000, 8), {}), ("sel_ptr", (0x1000, 10, o, 1 << 64, 1), {}),
                           ("sel_offset", (0x1000, 10, o, 0x3000, 1), {"sel_offset": 1 << 64}),
                           ("mapq_ptr", (0x1000, 10, o, 0x3000, 8), {"mapq_ptr": 1 << 64})):
        with pytest.raises(ValueError, match=r"%s must fit an unsigned 64-bit integer, not" % name):
            f(*args, **kw)
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
        f(0x1000, 10, o, 0x3000, 1, min_mapq=1)
    for sel_bits in (1, 8):
        predicate_refusals(lambda **kw: f(0x1000, 10, o, 0x3000, sel_bits, mapq_ptr=0x2000, **kw))
    offsets_refusals(lambda bad: f(0x1000, 10, bad, 0x2000, 1, sel_offset=5, exclude=0x904, mapq_ptr=0x3000, min_mapq=30), 10)
    offsets_refusals(lambda bad: f(0x1000, 10, bad, 0x2000, 8), 10)


def test_torch_refusals(no_library):  # noqa: F811
    import torch
    from libflagstats_amd import segments_filter_where as sfw
    f = sfw.count_segments_torch_filter_where
    t = torch.zeros(20, dtype=torch.int16)
    q = torch.zeros(20, dtype=torch.uint8)
    m = torch.ones(20, dtype=torch.bool)
    bits = torch.zeros(4, dtype=torch.uint8)
    o = torch.tensor([0, 7, 20], dtype=torch.int64)
    with pytest.raises(ValueError, match=r"t must be a torch\.Tensor, not ndarray"):
        f(np.zeros(20, dtype=np.uint16), o, m)
    for dt in (torch.int32, torch.int64, torch.uint8, torch.bool, torch.float16):
        with pytest.raises(ValueError, match=r"t must have dtype int16 or uint16, not " + re.escape(str(dt))):
            f(torch.zeros(20, dtype=dt), o, m)
    for bad in (torch.zeros((4, 5), dtype=torch.int16), torch.zeros(40, dtype=torch.int16)[::2]):
        with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
            f(bad, o, m)
    # the selection
    with pytest.raises(ValueError, match=r"where must be a torch\.Tensor, not ndarray"):
        f(t, o, np.ones(20, dtype=bool))
    with pytest.raises(ValueError, match=r"where must be a torch\.Tensor, not NoneType"):
        f(t, o, None)
    for bad in (torch.ones((4, 5), dtype=torch.bool), torch.ones(40, dtype=torch.bool)[::2]):
        with pytest.raises(ValueError, match=r"where must be 1-D and contiguous"):
            f(t, o, bad)
    for dt in (torch.uint8, torch.int8, torch.int64):
        with pytest.raises(ValueError, match=r"where must have dtype torch\.bool \(packed=True: a torch\.uint8 bitmap\), not " + re.escape(str(dt))):
            f(t, o, torch.ones(20, dtype=dt))
    for dt in (torch.bool, torch.int8):
        with pytest.raises(ValueError, match=r"where must have dtype torch\.uint8 with packed=True \(an LSB-first bitmap\), not " + re.escape(str(dt))):
            f(t, o, torch.ones(4, dtype=dt), packed=True)
    for size in (0, 19, 21):
        with pytest.raises(ValueError, match=r"where must have one element per value \(20\), not %d" % size):
            f(t, o, torch.ones(size, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"where holds 3 bytes, 20 values from bit 5 on need 4"):
        f(t, o, torch.zeros(3, dtype=torch.uint8), packed=True, bit_offset=5)
    bit_offset_refusals(lambda packed, **kw: f(t, o, bits if packed else m, packed=packed, **kw))
    # the column
    with pytest.raises(ValueError, match=r"mapq must be a torch\.Tensor, not ndarray"):
        f(t, o, m, mapq=np.zeros(20, dtype=np.uint8), min_mapq=1)
    for dt in (torch.int8, torch.bool, torch.int16, torch.float32):
        with pytest.raises(ValueError, match=r"mapq must have dtype torch\.uint8, not " + re.escape(str(dt))):
            f(t, o, m, mapq=torch.zeros(20, dtype=dt), min_mapq=1)
    for bad in (torch.zeros((4, 5), dtype=torch.uint8), torch.zeros(40, dtype=torch.uint8)[::2]):
        with pytest.raises(ValueError, match=r"mapq must be 1-D and contiguous"):
            f(t, o, m, mapq=bad, min_mapq=1)
    for size in (0, 19, 21):
        with pytest.raises(ValueError, match=r"mapq must have one element per value \(20\), not %d" % size):
            f(t, o, m, mapq=torch.zeros(size, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
        f(t, o, m, min_mapq=30)
    predicate_refusals(lambda **kw: f(t, o, m, mapq=q, **kw))
    predicate_refusals(lambda **kw: f(t, o, bits, mapq=q, packed=True, bit_offset=3, **kw))
    # the offsets and the results
    for bad in (np.array([0, 20]), torch.tensor([0, 20], dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int64),
                torch.zeros(0, dtype=torch.int64), torch.zeros(6, dtype=torch.int64)[::2]):
        with pytest.raises(ValueError, match=r"offsets must be a 1-D contiguous int64 tensor \(nseg \+ 1 values\)"):
            f(t, bad, m)
    for bad in (torch.zeros((3, 32), dtype=torch.int64), torch.zeros((2, 32), dtype=torch.int32), torch.zeros(64, dtype=torch.int64),
                np.zeros((2, 32), dtype=np.int64)):
        with pytest.raises(ValueError, match=r"out must be a contiguous int64 tensor of shape \(2, 32\)"):
            f(t, o, m, out=bad)
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int64), 0):
        with pytest.raises(ValueError, match=r"selected must be a contiguous int64 tensor of shape \(2,\)"):
            f(t, o, m, selected=bad)
    with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
        f(t, o, m)                                    # host tensors
    with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
        f(t, o, bits, require=2, exclude=0x904, mapq=q, min_mapq=30, packed=True, bit_offset=1)
    # (offsets / where / mapq / out / selected on another device than t: tests/test_gpu_segments_filter_where.py::test_refusals)


def test_symbols_in_the_tables_the_library_and_the_headers():
    from libflagstats_amd import _lib
    for name in PUBLIC:
        assert name in _lib.SIGNATURES and name not in _lib.INTERNAL_SIGNATURES, name
    for name in INTERNAL:
        assert name in _lib.INTERNAL_SIGNATURES and name not in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_u16_segments_filter_where"][1]) == 15
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_u16_segments_filter_where_sync"][1]) == 14
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_u16_x64_segments_filter_where"][1]) == 14
    assert len(_lib.INTERNAL_SIGNATURES["fsk_launch_segments_filter_where"][1]) == 17
    P, U64, U32, I = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    for name in PUBLIC:
        restype, args = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int, name
        # array, n, offsets, nseg, require, exclude, mapq, min_mapq, sel, sel_offset, sel_bits, out, selected, flags
        assert args[:14] == [P, U64, P, U64, U32, U32, P, U32, P, U64, I, P, P, I], name
    assert _lib.SIGNATURES["FLAGSTATS_hip_device_u16_segments_filter_where"][1][14] is P                        # stream
    restype, args = _lib.INTERNAL_SIGNATURES["fsk_launch_segments_filter_where"]
    # chunk, mapq, sel, sel_offset, sel_bits, base, m, offsets, nseg, require, exclude, min_mapq, out, selected, mode, grid, stream
    assert restype is ctypes.c_int and args == [P, P, P, U64, I, U64, U64, P, U64, U32, U32, U32, P, P, I, U32, P]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in PUBLIC + INTERNAL:
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    for name in PUBLIC:
        m = re.search(r"\bint %s\(([^)]*)\)" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    internal = open(os.path.join(ROOT, "libflagstats_amd", "csrc", "flagstat_segments_filter_where.h")).read()
    for name in INTERNAL:
        m = re.search(r"\bhipError_t %s\(([^)]*)\)" % name, internal)
        assert m and name not in header, name
        assert len(m.group(1).split(",")) == len(_lib.INTERNAL_SIGNATURES[name][1]), name


def test_code_objects():
    """K1's code object is still the one profiles/traffic.json was measured on; exactly one gfx950 code object defines
    fsk::flagstat_segments_filter_where, in exactly five instantiations -- the bitmap with and without MAPQ, each at a byte
    boundary and funnelled, and bytes with MAPQ; bytes without MAPQ (<0, 8, 0>) is the filtered segmented kernel's business --
    and it is none of K1's, the filter_where kernel's, the filtered segmented kernel's or the selected segmented kernel's"""
    from libflagstats_amd import _lib, kernel_id
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        recorded = json.load(f)["kernel_source_id"]
    assert kernel_id.kernel_id(_lib.LIB_PATH) == recorded
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    mine, others = [], {k: [] for k in OTHERS}
    for i, co in enumerate(kernel_id._code_objects(so)):
        secs = kernel_id._sections(co)
        names = b"".join(co[secs[t][0]:secs[t][0] + secs[t][1]] for t in (".strtab", ".dynstr") if t in secs)
        for k, sym in OTHERS.items():
            if sym in names:
                others[k].append(i)
        if KERNEL in names:
            found = set(re.findall(re.escape(KERNEL) + rb"(ILb[01]ELi[0-9]+ELb[01]E)", names))
            assert found == set(FORMS), found
            assert KERNEL + b"ILb0ELi8ELb0E" not in names
            mine.append(i)
    assert len(mine) == 1, mine
    for k, where in others.items():
        assert len(where) == 1 and where[0] != mine[0], (k, where, mine)


LAYOUTS = {
    "end to end": [0, 1, 3, 6, 11, 11, 400, 401, 999, 1000],
    "gaps around": [17, 17, 250, 250, 251, 777, 990],
    "one": [0, 1000],
    "tiny": list(range(100, 160, 3)) + [160, 160, 161],
}
PREDICATES = ((0, 0), (0, 0x904), (0x2, 0x904), (0x0101, 0x8080), (0x40, 0x40), (0x0400, 0x0004))   # one plane, both, an overlapping pair
THRESHOLDS = (0, 1, 30, 127, 128, 129, 255)


def test_oracle_against_a_per_element_per_segment_loop(oracle_mod):
    """segments_filter_where_oracle.want on 1,000 values against (a) a plain Python loop over the segments and their elements that
    reads the selection out of a bitmap at an odd bit offset and out of bytes of values 1, 2, 0x80 and 0xFF, tests FLAG and MAPQ
    with Python ints and hands the kept values to the C oracle, and (b) compaction with numpy, oracle.flagstat_c of
    values[b:e][m[b:e]]: predicates on one and on both byte planes, an overlapping pair, thresholds on both sides of 128"""
    rng = np.random.RandomState(21)
    n = 1000
    v = rng.randint(0, 65536, n).astype(np.uint16)
    v[:64] &= np.uint16(0x00FF)                   # some values that pass predicates with many excluded bits
    v[64:128] = 0
    v[128:192] &= np.uint16(0x0103)
    q = rng.randint(0, 256, n).astype(np.uint8)
    q[:8] = (0, 1, 29, 30, 127, 128, 129, 255)
    mask = rng.randint(0, 3, n) > 0
    bitmap = pack(mask, 13, fill=1)
    as_bytes = mask.astype(np.uint8) * np.resize(np.array([1, 2, 0x80, 0xFF], dtype=np.uint8), n)
    counted_some, overlap = False, False
    for pi, (require, exclude) in enumerate(PREDICATES):
        for ti, min_mapq in enumerate(THRESHOLDS):
            name = list(LAYOUTS)[(pi + ti) % len(LAYOUTS)]
            o = np.array(LAYOUTS[name], dtype=np.int64)
            for superset in (False, True):
                rows, selected = sfwo.want(v, o, mask, require, exclude, q, min_mapq, superset)
                assert rows.dtype == np.uint64 and rows.shape == (o.size - 1, 32) and selected.dtype == np.uint64
                m = ((v & require) == require) & ((v & exclude) == 0) & ((q >= min_mapq) if min_mapq else True) & mask
                for i in range(o.size - 1):
                    b, e = int(o[i]), int(o[i + 1])
                    kept = []
                    for j in range(b, e):
                        x, mq = int(v[j]), int(q[j])
                        sel_bit = (int(bitmap[(13 + j) >> 3]) >> ((13 + j) & 7)) & 1
                        assert bool(sel_bit) == (int(as_bytes[j]) != 0)
                        if (x & require) == require and (x & exclude) == 0 and (min_mapq == 0 or mq >= min_mapq) and sel_bit:
                            kept.append(x)
                    kept = np.array(kept, dtype=np.uint16)
                    w = where_oracle.want_counters(oracle_mod, kept, np.ones(kept.size, dtype=bool), superset)
                    assert np.array_equal(rows[i], w), (name, require, exclude, min_mapq, superset, i, rows[i], w)
                    assert int(selected[i]) == kept.size
                    c = where_oracle.want_counters(oracle_mod, v[b:e], m[b:e], superset)      # compaction
                    assert np.array_equal(rows[i], c) and int(selected[i]) == int(m[b:e].sum())
                counted_some |= bool(selected.any())
                if require & exclude:
                    overlap = True
                    assert not rows.any() and not selected.any()
    assert counted_some and overlap
    # without a column the threshold must be 0; an empty predicate is the selected segmented oracle, an all-ones mask the filtered
    import segments_filter_oracle
    import segments_where_oracle
    o = np.array(LAYOUTS["end to end"], dtype=np.int64)
    a, b = sfwo.want(v, o, mask, 0, 0, superset=True), segments_where_oracle.want(v, o, mask, True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    a = sfwo.want(v, o, np.ones(n, dtype=bool), 0x2, 0x904, q, 30, True)
    b = segments_filter_oracle.want(v, o, 0x2, 0x904, q, 30, True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_periodic_want_equals_want_on_the_materialised_array():
    """periods 997 (flags), 13 (mask) and 7 (MAPQ): their joint period, 90,727, is shorter than the array, so the rows come from
    the periodic form; with the periods 997, 1,009 and 1,013 it is longer and the array itself is materialised"""
    rng = np.random.RandomState(22)
    for sizes, n in (((997, 13, 7), 200_000), ((997, 1009, 1013), 50_000)):
        pattern = rng.randint(0, 65536, sizes[0]).astype(np.uint16)
        mask_pattern = rng.randint(0, 3, sizes[1]) > 0
        mapq_pattern = rng.randint(0, 256, sizes[2]).astype(np.uint8)
        oo = np.array([0, 1, 996, 997, 998, 12961, 12961, 12962, n - 1000, n], dtype=np.int64)
        for phase in (0, 5):
            big = np.resize(np.roll(pattern, -phase), n)
            big_m, big_q = np.resize(mask_pattern, n), np.resize(mapq_pattern, n)
            for require, exclude, min_mapq in ((0, 0x904, 0), (0x2, 0x904, 30), (0x0101, 0x8080, 128)):
                got = sfwo.periodic_want(pattern, oo, mask_pattern, require, exclude, mapq_pattern, min_mapq, True, phase)
                ref = sfwo.want(big, oo, big_m, require, exclude, big_q, min_mapq, True)
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (sizes, phase, require, exclude, min_mapq)
                assert got[1].any()
