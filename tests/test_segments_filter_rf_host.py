"""The filtered segmented flagstat under samtools' whole FLAG predicate (libflagstats_amd/segments_filter_rf.py,
csrc/flagstat_segments_filter_rf.hip) on the CPU: segments_filter_rf_oracle against a plain loop, the package's exports, every
refusal of the Python layer -- raised before the library is loaded -- and of the C entries for the two new masks, the symbols in
the binding tables, the built library, the headers and the Makefile, the identity of the code object, what the reduction makes
of the predicates the GPU tests rely on, and that those predicates tell seven wrong kernels from the right one."""
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
import segments_filter_rf_oracle as sfro  # noqa: E402
import where_oracle  # noqa: E402
from segments_filter_oracle import segment_sums  # noqa: E402
from test_filter_host import no_library  # noqa: E402,F401  (a fixture)
from test_filter_rf_host import rf_refusals  # noqa: E402
from test_segments_filter_host import offsets_refusals  # noqa: E402

from libflagstats_amd import segments_filter_rf as sfr  # noqa: E402  (fails at import where the feature is missing)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libflagstats_amd", "csrc")
UNIT = "flagstat_segments_filter_rf"
KERNEL = b"_ZN3fsk27flagstat_segments_filter_rf"
PUBLIC = {"FLAGSTATS_hip_device_u16_segments_filter_rf": 14, "FLAGSTATS_hip_device_u16_segments_filter_rf_sync": 13,
          "FLAGSTATS_hip_u16_x64_segments_filter_rf": 13}
LAUNCHER, LAUNCHER_ARGS = "fsk_launch_segments_filter_rf", 16
PY_NAMES = ("flagstats_segments_filter_rf", "count_segments_device_ptr_filter_rf", "count_segments_torch_filter_rf")
NEW_MASKS = ("include_any", "exclude_all")


# ------------------------------------------------------------------ the oracle
LAYOUTS = {
    "whole": [0, 1000],
    "gaps and empties": [3, 3, 40, 40, 41, 500, 500, 997],
    "short": list(range(0, 1001, 7)) + [1000],
    "nothing": [17],
}


def test_oracle_against_a_loop(oracle_mod):
    """segments_filter_rf_oracle.want on 1,000 values: which flags pass is decided element by element in plain Python, segment by
    segment, and the passing flags of a segment are counted by the C oracle; the periodic form against the materialised array;
    with both options off the oracle is segments_filter_oracle's"""
    rng = np.random.RandomState(12)
    v = rng.randint(0, 65536, 1000).astype(np.uint16)
    v[:200] &= np.uint16(0x06FF)
    v[200:230] = 0
    v[230:240] = 0xFFFF
    q = rng.randint(0, 256, 1000).astype(np.uint8)
    q[:8] = (0, 1, 29, 30, 127, 128, 129, 255)
    some = False
    for name, o in LAYOUTS.items():
        o = np.array(o, dtype=np.int64)
        for require, exclude, include_any, exclude_all in [p for p, _, _ in sfro.TABLE] + [(0x2, 0x900, 0x50, 0xC), (0, 0, 0, 0), (0, 0x904, 0, 0)]:
            for min_mapq in (0, 30, 128):
                for superset in (False, True):
                    rows, selected = sfro.want(v, o, require, exclude, include_any, exclude_all, q, min_mapq, superset)
                    assert rows.dtype == np.uint64 and rows.shape == (o.size - 1, 32) and selected.dtype == np.uint64
                    for i in range(o.size - 1):
                        inside = np.zeros(1000, dtype=bool)
                        for j in range(int(o[i]), int(o[i + 1])):
                            x, m = int(v[j]), int(q[j])
                            inside[j] = ((x & require) == require and (x & exclude) == 0 and (include_any == 0 or (x & include_any) != 0)
                                         and (exclude_all == 0 or (x & exclude_all) != exclude_all) and (min_mapq == 0 or m >= min_mapq))
                        w = where_oracle.want_counters(oracle_mod, v, inside, superset)
                        assert np.array_equal(rows[i], w), (name, require, exclude, include_any, exclude_all, min_mapq, superset, i)
                        assert int(selected[i]) == int(inside.sum())
                    some |= bool(selected.any())
                    if include_any == 0 and exclude_all == 0:
                        rows2, selected2 = sfo.want(v, o, require, exclude, q, min_mapq, superset)
                        assert np.array_equal(rows, rows2) and np.array_equal(selected, selected2)
    assert some
    pattern, mq_pattern = v[:997], q[:997]
    oo = np.array([0, 1, 996, 997, 998, 1994, 1994, 3100, 3200], dtype=np.int64)
    for require, exclude, include_any, exclude_all in ((0x1, 0x804, 0x110, 0x2200), (0, 0x904, 0x50, 0), (0, 0, 0, 0x420)):
        for phase in (0, 5):
            big, big_q = np.resize(np.roll(pattern, -phase), 3200), np.resize(np.roll(mq_pattern, -phase), 3200)
            for min_mapq in (0, 30):
                a = sfro.periodic_want(pattern, oo, require, exclude, include_any, exclude_all, mq_pattern, min_mapq, True, phase)
                b = sfro.want(big, oo, require, exclude, include_any, exclude_all, big_q, min_mapq, True)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and b[1].any()


# ------------------------------------------------------------------ the Python layer
def test_exports_and_shared_checks():
    import libflagstats_amd
    from libflagstats_amd import filter_rf, segments_filter
    for name in PY_NAMES:
        assert getattr(libflagstats_amd, name) is getattr(sfr, name) and name in libflagstats_amd.__all__
    assert len(set(libflagstats_amd.__all__)) == len(libflagstats_amd.__all__)
    assert "``segments_filter_rf``" in libflagstats_amd.__doc__
    # the checks and the row shaper are the parents', not restated
    assert sfr._check_predicate_rf is filter_rf._check_predicate_rf and sfr.segment_filter_dicts is segments_filter.segment_filter_dicts
    assert sfr._check_numpy is segments_filter._check_numpy and sfr._check_mapq_torch is segments_filter._check_mapq_torch
    src = open(os.path.join(ROOT, "libflagstats_amd", "segments_filter_rf.py")).read()
    for text in ("must be a numpy.ndarray", "must have dtype", "must be 1-D", "must have one element per value", "must be a torch.Tensor",
                 "16-bit FLAG mask", "needs mapq", "must be in 0..255", "must be an int", "non-decreasing"):
        assert text not in src, text


def test_numpy_refusals(no_library):  # noqa: F811
    f = sfr.flagstats_segments_filter_rf
    v = np.zeros(20, dtype=np.uint16)
    q = np.zeros(20, dtype=np.uint8)
    o = np.array([0, 7, 20])
    with pytest.raises(ValueError, match=r"values must have dtype uint16, not int16"):
        f(np.zeros(20, dtype=np.int16), o)
    for size in (0, 19, 21):
        with pytest.raises(ValueError, match=r"mapq must have one element per value \(20\), not %d" % size):
            f(v, o, mapq=np.zeros(size, dtype=np.uint8))
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
        f(v, o, include_any=0x50, min_mapq=30)
    rf_refusals(lambda **kw: f(v, o, mapq=q, **kw))
    offsets_refusals(lambda bad: f(v, bad, include_any=0x50, mapq=q, min_mapq=30), 20)


def test_device_pointer_refusals(no_library):  # noqa: F811
    f = sfr.count_segments_device_ptr_filter_rf
    o = np.array([0, 4, 10])
    with pytest.raises(ValueError, match=r"n must not be negative"):
        f(0x1000, -1, o)
    with pytest.raises(ValueError, match=r"mapq_ptr must be an int, not"):
        f(0x1000, 10, o, mapq_ptr=None)
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
        f(0x1000, 10, o, exclude_all=0xC, min_mapq=1)
    rf_refusals(lambda **kw: f(0x1000, 10, o, mapq_ptr=0x2000, **kw))
    offsets_refusals(lambda bad: f(0x1000, 10, bad, exclude_all=0xC, mapq_ptr=0x2000, min_mapq=30), 10)


def test_torch_refusals(no_library):  # noqa: F811
    import torch
    f = sfr.count_segments_torch_filter_rf
    t = torch.zeros(20, dtype=torch.int16)
    q = torch.zeros(20, dtype=torch.uint8)
    o = torch.tensor([0, 7, 20], dtype=torch.int64)
    with pytest.raises(ValueError, match=r"t must have dtype int16 or uint16, not torch\.int32"):
        f(torch.zeros(20, dtype=torch.int32), o)
    with pytest.raises(ValueError, match=r"offsets must be a 1-D contiguous int64 tensor \(nseg \+ 1 values\)"):
        f(t, np.array([0, 20]))
    with pytest.raises(ValueError, match=r"mapq must have dtype torch\.uint8, not torch\.int8"):
        f(t, o, mapq=torch.zeros(20, dtype=torch.int8), min_mapq=1)
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
        f(t, o, include_any=0x50, exclude_all=0xC, min_mapq=30)
    rf_refusals(lambda **kw: f(t, o, mapq=q, **kw))
    with pytest.raises(ValueError, match=r"out must be a contiguous int64 tensor of shape \(2, 32\)"):
        f(t, o, out=torch.zeros((3, 32), dtype=torch.int64))
    with pytest.raises(ValueError, match=r"selected must be a contiguous int64 tensor of shape \(2,\)"):
        f(t, o, selected=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
        f(t, o, require=2, exclude=0x904, include_any=0x50, exclude_all=0xC, mapq=q, min_mapq=30)


# ------------------------------------------------------------------ the C entries' own refusals (before any HIP call)
def test_c_refusals_of_the_new_masks():
    """include_any or exclude_all above 0xFFFF, in the shared text, asked after the parent's predicate and before everything
    else; rows and counts stay as they were"""
    from libflagstats_amd import _lib
    lib = _lib.lib()
    a = np.zeros(104, dtype=np.uint16)
    q = np.zeros(104, dtype=np.uint8)
    o = np.array([0, 10, 100], dtype=np.uint64)
    out = np.full((2, 32), 7, dtype=np.uint64)
    sel = np.full(2, 7, dtype=np.uint64)

    def call(name, require=1, exclude=4, include_any=0x50, exclude_all=0xC, min_mapq=30, flags=1, array=a.ctypes.data, offsets=o.ctypes.data,
             nseg=2):
        args = [array, 100, offsets, nseg, require, exclude, include_any, exclude_all, q.ctypes.data, min_mapq, out.ctypes.data,
                sel.ctypes.data, flags]
        rc = getattr(lib, name)(*(args + [None] if PUBLIC[name] == 14 else args))
        assert (out == 7).all() and (sel == 7).all()
        return rc, lib.FLAGSTATS_hip_last_error().decode()

    for name in PUBLIC:
        for mask in NEW_MASKS:
            for bad in (0x10000, 0xFFFFFFFF):
                rc, text = call(name, **{mask: bad})
                assert rc != 0 and text.endswith("%s must be a 16-bit FLAG mask (at most 0xFFFF)" % mask), (name, mask, text)
        rc, text = call(name, include_any=0x10000, exclude_all=0x10000)
        assert rc != 0 and "include_any must be" in text
        # the parent's predicate is asked first
        rc, text = call(name, exclude=0x10000, include_any=0x10000)
        assert rc != 0 and "exclude must be a 16-bit FLAG mask (at most 0xFFFF)" in text
        rc, text = call(name, min_mapq=256, exclude_all=0x10000)
        assert rc != 0 and "min_mapq must be at most 255" in text
        # ... and the new masks before the flags, the segments and the array, also with no segment at all
        rc, text = call(name, exclude_all=0x10000, flags=4)
        assert rc != 0 and "exclude_all must be" in text
        rc, text = call(name, include_any=0x10000, offsets=None)
        assert rc != 0 and "include_any must be" in text
        rc, text = call(name, exclude_all=0x10000, array=None)
        assert rc != 0 and "exclude_all must be" in text
        rc, text = call(name, include_any=0x10000, nseg=0)
        assert rc != 0 and "include_any must be" in text
        rc, text = call(name, flags=4)
        assert rc != 0 and "no other bits" in text
        rc, text = call(name, offsets=None)
        assert rc != 0 and "with nseg > 0" in text
    # the text of the rule stands in flagstat_derived_host.h and in no unit
    holders = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip")) and "16-bit FLAG mask" in open(os.path.join(CSRC, fn)).read()]
    assert holders == ["flagstat_derived_host.h"]


# ------------------------------------------------------------------ symbols
def test_symbols_in_the_tables_the_library_the_headers_and_the_makefile():
    from libflagstats_amd import _lib
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    for name, nargs in PUBLIC.items():
        assert name in _lib.SIGNATURES and name not in _lib.INTERNAL_SIGNATURES, name
        restype, args = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(args) == nargs, name
        # array, n, offsets, nseg, require, exclude, include_any, exclude_all, mapq, min_mapq, out, selected, flags
        assert args[:13] == [vp, u64, vp, u64, u32, u32, u32, u32, vp, u32, vp, vp, ctypes.c_int], name
    assert LAUNCHER in _lib.INTERNAL_SIGNATURES and LAUNCHER not in _lib.SIGNATURES
    # chunk, mapq chunk, base, m, offsets, nseg, require, exclude, include_any, exclude_all, min_mapq, out, selected, mode, grid, stream
    assert _lib.INTERNAL_SIGNATURES[LAUNCHER][1] == [vp, vp, u64, u64, vp, u64, u32, u32, u32, u32, u32, vp, vp, ctypes.c_int, u32, vp]
    parent = _lib.INTERNAL_SIGNATURES["fsk_launch_segments_filter"][1]
    assert _lib.INTERNAL_SIGNATURES[LAUNCHER][1] == parent[:8] + [u32, u32] + parent[8:]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in tuple(PUBLIC) + (LAUNCHER,):
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    start = header.index("filtered segments, the whole predicate:")
    assert start > max(m.start() for m in re.finditer(r"/\* =================", header[:start])) > header.index("streaming sessions")
    section = header[start:]
    for name, nargs in PUBLIC.items():
        m = re.search(r"\bint %s\(([^)]*)\)" % name, section)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert len(re.findall(r"\b%s\(" % name, header)) == 1, name
    intro = section[:section.index("int FLAGSTATS_hip_device_u16_segments_filter_rf(")]
    for text in ("(include_any == 0 || (array[j] & include_any) != 0)", "(exclude_all == 0 || (array[j] & exclude_all) != exclude_all)",
                 "nothing is launched", "the filtered segmented entries' kernel", "fsk::flagstat_segments_filter_rf", "above 0xFFFF",
                 "slot 9 = selected[i]", "minus slot 25", "min_mapq == 0 reads no byte of `mapq`, which may then be NULL",
                 "malformed offsets give undefined counters and never an access outside"):
        assert text in intro, text
    # the launcher is declared in the unit's internal header and nowhere else
    for fn in sorted(os.listdir(CSRC)) + [os.path.join(ROOT, "include", "libflagstats_hip.h"),
                                          os.path.join(ROOT, "include", "libflagstats_hip_probe.h")]:
        if not fn.endswith(".h"):
            continue
        text = open(os.path.join(CSRC, fn)).read()
        m = re.search(r"^hipError_t %s\(([^)]*)\)" % LAUNCHER, text, re.M)
        if os.path.basename(fn) == UNIT + ".h":
            assert m and len(m.group(1).split(",")) == LAUNCHER_ARGS
        else:
            assert LAUNCHER not in text, fn
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1)
    hdrs = re.search(r"^HDRS\s*:=(.*)$", mk, re.M).group(1)
    assert "$(HERE)%s.hip" % UNIT in srcs.split() and "$(HERE)%s.h" % UNIT in hdrs.split()
    # the device test and the reduction are taken from their holders, not restated
    unit = open(os.path.join(CSRC, UNIT + ".hip")).read()
    assert '#include "flagstat_filter_rf_device.h"' in unit and '#include "flagstat_filter_rf.h"' in unit
    for text in ("and_nonzero_bytes", "struct FilterRfArgs", "filter_rf_args_of(uint32_t"):
        assert text not in unit, text
    assert "seg_walk<kSegWaveFlags>" in unit and "seg_emit<true, false>" in unit and "SegWalk sw" not in unit


def test_code_objects():
    """K1's code object is still the one profiles/traffic.json was measured on; exactly one gfx950 code object defines
    fsk::flagstat_segments_filter_rf, it holds all six instantiations (MAPQ read or not; the any-of test, the all-of test, both)
    and no other fsk::flagstat_* kernel: the unit calls fsk_launch_segments_filter and instantiates no other unit's kernel"""
    from libflagstats_amd import _lib, kernel_id
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        assert kernel_id.kernel_id(_lib.LIB_PATH) == json.load(f)["kernel_source_id"]
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    new = [KERNEL + b"ILb%dELb%dELb%dEE" % (mapq, any_of, all_of) for mapq in (0, 1) for any_of, all_of in ((1, 0), (0, 1), (1, 1))]
    holders = 0
    for co in kernel_id._code_objects(so):
        secs = kernel_id._sections(co)
        names = b"".join(co[secs[t][0]:secs[t][0] + secs[t][1]] for t in (".strtab", ".dynstr") if t in secs)
        if KERNEL not in names:
            continue
        holders += 1
        for inst in new:
            assert inst in names, inst
        assert KERNEL + b"ILb0ELb0ELb0EE" not in names and KERNEL + b"ILb1ELb0ELb0EE" not in names
        kernels = set(re.findall(rb"_ZN3fsk\d+flagstat_[a-z0-9_]+", names))
        assert kernels == {KERNEL}, kernels
    assert holders == 1
    # the existing tests find their kernels by these prefixes: the new name falls under none of them
    for prefix in (b"_ZN3fsk21flagstat_count_filter", b"_ZN3fsk21flagstat_filter_where", b"_ZN3fsk14flagstat_count",
                   b"_ZN3fsk24flagstat_segments_filter", b"_ZN3fsk17flagstat_segmentsE", b"_ZN3fsk20flagstat_count_where",
                   b"_ZN3fsk19flagstat_count_wide", b"_ZN3fsk24flagstat_count_filter_rf", b"_ZN3fsk30flagstat_segments_filter_where"):
        assert not KERNEL.startswith(prefix)


# ------------------------------------------------------------------ what the GPU tests rely on
def test_reduction_kinds_of_the_predicates():
    """the answer of the reduction, and the pair it leaves, for the eleven named predicates; every two-bit mask alone is a
    residue that comes back as it is"""
    from libflagstats_amd import _lib
    reduce_ = _lib.lib().fsk_filter_rf_reduce
    out = (ctypes.c_uint32 * 4)()
    assert len(sfro.TABLE) == 11 and [k for _, k, _ in sfro.TABLE].count(2) == 6
    for given, kind, pair in sfro.TABLE:
        assert reduce_(*given, out) == kind, given
        if kind == 2:
            assert tuple(out) == given, (given, tuple(out))            # already reduced: the kernel sees these four masks
        elif kind == 1:
            assert tuple(out) == pair + (0, 0), (given, tuple(out))
        else:
            assert tuple(out) == (0, 0, 0, 0)
    assert len(sfro.TWO_BITS) == 120
    planes = {(bool(m & 0x00FF), bool(m & 0xFF00)) for m in sfro.TWO_BITS}
    assert planes == {(True, False), (False, True), (True, True)}
    for given in sfro.RESIDUES:
        assert reduce_(*given, out) == 2 and tuple(out) == given, given
    assert len(sfro.RESIDUES) == 246 and set(sfro.RESIDUES) <= set(sfro.PREDICATES) and len(sfro.PREDICATES) == 251


def _pass(v, r, e, any_test, all_test):
    return ((v & r) == r) & ((v & e) == 0) & any_test & all_test


def _any(v, a, plane=0xFFFF):
    return np.ones(v.shape, dtype=bool) if a == 0 else (v & (a & plane)) != 0


def _all(v, g, plane=0xFFFF):
    return np.ones(v.shape, dtype=bool) if g == 0 else (~v & (g & plane)) != 0


# (name, applies to the residue (a, g), the flags it passes): a kernel that is wrong in one way
WRONG_MODELS = (
    ("--rf treated as -f", lambda a, g: a != 0, lambda v, r, e, a, g: _pass(v, r | a, e, True, _all(v, g))),
    ("-G treated as -F", lambda a, g: g != 0, lambda v, r, e, a, g: _pass(v, r, e | g, _any(v, a), True)),
    ("--rf ignored", lambda a, g: a != 0, lambda v, r, e, a, g: _pass(v, r, e, True, _all(v, g))),
    ("-G ignored", lambda a, g: g != 0, lambda v, r, e, a, g: _pass(v, r, e, _any(v, a), True)),
    ("the two tests swapped", lambda a, g: a != g, lambda v, r, e, a, g: _pass(v, r, e, _any(v, g), _all(v, a))),
    ("only the low byte plane seen", lambda a, g: (a | g) & 0xFF00 != 0,
     lambda v, r, e, a, g: _pass(v, r, e, _any(v, a, 0x00FF), _all(v, g, 0x00FF))),
    ("only the high byte plane seen", lambda a, g: (a | g) & 0x00FF != 0,
     lambda v, r, e, a, g: _pass(v, r, e, _any(v, a, 0xFF00), _all(v, g, 0xFF00))),
)


def test_the_predicates_tell_wrong_kernels_from_the_right_one():
    """on the GPU file's 0..65535 input and layout, each of seven wrong models changes `selected` of at least one segment, for
    every residue predicate that file uses and that the model touches (a model of --rf says nothing under a predicate without
    --rf; one that sees a single byte plane is right for masks that lie in that plane).  Every model is touched by many
    predicates and every predicate touches at least three models."""
    from filter_rf_oracle import view_mask
    values, o = sfro.every_value_input()
    assert np.array_equal(np.sort(values), np.arange(65536, dtype=np.uint16)) and (np.diff(o) == 0).any() and o.size > 50
    v = values.astype(np.int64)
    applied = {name: 0 for name, _, _ in WRONG_MODELS}
    for r, e, a, g in sfro.RESIDUES:
        right = view_mask(values, r, e, a, g)
        assert np.array_equal(right, _pass(v, r, e, _any(v, a), _all(v, g)))
        right_sel = segment_sums(right, o)
        touched = 0
        for name, applies, model in WRONG_MODELS:
            if not applies(a, g):
                continue
            touched += 1
            applied[name] += 1
            wrong_sel = segment_sums(model(v, r, e, a, g), o)
            assert (wrong_sel != right_sel).any(), (name, hex(r), hex(e), hex(a), hex(g))
        assert touched >= 3, (r, e, a, g)
    assert all(count >= 100 for count in applied.values()), applied
