"""The filtered flagstat under samtools' whole FLAG predicate (libflagstats_amd/filter_rf.py, csrc/flagstat_filter_rf.hip) on the
CPU: the exact reduction of the four masks against brute force, filter_rf_oracle's mask against a per-element loop, the package's
exports, every refusal of the Python layer -- raised before the library is loaded -- and of the C entries, the symbols in the
binding tables, the built library, the headers and the Makefile, and the identity of the code object."""
import ctypes
import itertools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from filter_rf_oracle import view_mask  # noqa: E402
from test_filter_host import no_library, predicate_refusals  # noqa: E402,F401  (no_library is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libflagstats_amd", "csrc")
UNIT = "flagstat_filter_rf"
KERNEL = b"_ZN3fsk24flagstat_count_filter_rf"
PUBLIC = {"FLAGSTATS_hip_device_u16_filter_rf": 12, "FLAGSTATS_hip_device_u16_filter_rf_sync": 11, "FLAGSTATS_hip_u16_x64_filter_rf": 11}
INTERNAL = {"fsk_launch_filter_rf": ("hipError_t", 13), "fsk_filter_rf_reduce": ("int", 5)}
PY_NAMES = ("counters_filter_rf", "flagstats_filter_rf", "count_device_ptr_filter_rf", "count_torch_filter_rf")
NEW_MASKS = ("include_any", "exclude_all")


# ------------------------------------------------------------------ the reduction
BITS = (0, 2, 7, 8, 15)                            # both byte planes and the seam between them
SUBSETS = np.array([sum(1 << BITS[k] for k in range(5) if s >> k & 1) for s in range(32)], dtype=np.uint32)


def passes(flags, r, e, a, g):
    """bool[len(r), len(flags)]: the definition, for columns of masks against a row of flags"""
    f = flags[None, :]
    r, e, a, g = (x[:, None] for x in (r, e, a, g))
    return ((f & r) == r) & ((f & e) == 0) & ((a == 0) | ((f & a) != 0)) & ((g == 0) | ((f & g) != g))


def bit_count(x):
    return sum((x >> b) & 1 for b in range(16))


def test_reduction_against_brute_force():
    """every quadruple of masks built from the subsets of bits {0, 2, 7, 8, 15} -- 32^4 -- through fsk_filter_rf_reduce: the
    reduced predicate passes exactly the flags the given one passes, on every flag built from those bits; 0 is returned exactly
    when nothing passes, 1 exactly when something passes and no residue is left; a residue has two bits or more and shares none
    with the reduced require | exclude, which are disjoint"""
    from libflagstats_amd import _lib
    reduce_ = _lib.lib().fsk_filter_rf_reduce
    out = (ctypes.c_uint32 * 4)()
    masks = [int(m) for m in SUBSETS]
    got = np.empty((32 ** 4, 5), dtype=np.uint32)
    for i, (r, e, a, g) in enumerate(itertools.product(masks, repeat=4)):
        rc = reduce_(r, e, a, g, out)
        got[i] = (rc, out[0], out[1], out[2], out[3])
    idx = np.indices((32, 32, 32, 32)).reshape(4, -1)
    r, e, a, g = (SUBSETS[idx[k]] for k in range(4))         # itertools.product's order
    rc, r2, e2, a2, g2 = got.T
    assert set(np.unique(rc).tolist()) == {0, 1, 2}
    flags = SUBSETS
    want = passes(flags, r, e, a, g)
    nonempty = want.any(axis=1)
    assert np.array_equal(rc != 0, nonempty)
    assert not got[rc == 0, 1:].any()
    live = rc != 0
    assert np.array_equal(passes(flags, r2[live], e2[live], a2[live], g2[live]), want[live])
    assert np.array_equal(rc == 1, live & (a2 == 0) & (g2 == 0)) and np.array_equal(rc == 2, (a2 | g2) != 0)
    assert not (r2 & e2).any() and not ((a2 | g2) & (r2 | e2)).any()
    for residue in (a2, g2):
        assert ((residue == 0) | (bit_count(residue) >= 2)).all()
    # the reduced masks hold no bit that was not given, and a plain pair comes back as it is
    assert not ((r2 | e2 | a2 | g2) & ~(r | e | a | g)).any()
    plain = live & (a == 0) & (g == 0)
    assert np.array_equal(r2[plain], r[plain]) and np.array_equal(e2[plain], e[plain]) and (rc[plain] == 1).all()


@pytest.mark.parametrize("given,want", [
    ((0, 0, 0, 0), (1, 0, 0, 0, 0)),
    ((0x2, 0x904, 0, 0), (1, 0x2, 0x904, 0, 0)),
    ((0x40, 0x40, 0x3, 0xC), (0, 0, 0, 0, 0)),                    # require & exclude
    ((0, 0, 0x50, 0), (2, 0, 0, 0x50, 0)),                        # --rf 0x50: first or reverse
    ((0, 0, 0, 0xC), (2, 0, 0, 0, 0xC)),                          # -G 0xC: read and mate both unmapped
    ((0, 0, 0x40, 0), (1, 0x40, 0, 0, 0)),                        # a single --rf bit is a required bit
    ((0, 0, 0, 0x400), (1, 0, 0x400, 0, 0)),                      # a single -G bit is an excluded bit
    ((0x10, 0, 0x50, 0), (1, 0x10, 0, 0, 0)),                     # --rf touches -f: satisfied
    ((0, 0x8, 0, 0xC), (1, 0, 0x8, 0, 0)),                        # -G touches -F: never all set
    ((0, 0x10, 0x50, 0), (1, 0x40, 0x10, 0, 0)),                  # --rf loses its excluded bit, one is left
    ((0x4, 0, 0, 0xC), (1, 0x4, 0x8, 0, 0)),                      # -G loses its required bit, one is left
    ((0, 0x50, 0x50, 0), (0, 0, 0, 0, 0)),                        # include_any within exclude
    ((0xC, 0, 0, 0xC), (0, 0, 0, 0, 0)),                          # exclude_all within require
    ((0, 0x10, 0x50, 0x440), (1, 0x40, 0x410, 0, 0)),             # the bit --rf moves into -f leaves -G with one, which moves to -F
    ((0x400, 0, 0x41, 0x401), (1, 0x440, 0x1, 0, 0)),             # the bit -G moves into -F leaves --rf with one: a second round
    ((0, 0x400, 0x41, 0x401), (2, 0, 0x400, 0x41, 0)),
    ((0x2, 0x900, 0x50, 0xC), (2, 0x2, 0x900, 0x50, 0xC)),
    ((0x2, 0x904, 0x50, 0xC), (2, 0x2, 0x904, 0x50, 0)),          # -F 0x904 drops every unmapped read: -G 0xC has nothing to add
    ((0, 0, 0xFFFF, 0xFFFF), (2, 0, 0, 0xFFFF, 0xFFFF)),
])
def test_reduction_of_named_cases(given, want):
    from libflagstats_amd import _lib
    out = (ctypes.c_uint32 * 4)()
    rc = _lib.lib().fsk_filter_rf_reduce(*given, out)
    assert (rc,) + tuple(out) == want


# ------------------------------------------------------------------ the oracle
def test_oracle_mask_against_a_loop():
    """filter_rf_oracle.view_mask, element by element in plain Python, on 1,000 values: the two options off, on within either byte
    plane and across them, overlapping each other and -f / -F, with thresholds on both sides of 128"""
    rng = np.random.RandomState(11)
    v = rng.randint(0, 65536, 1000).astype(np.uint16)
    v[:64] &= np.uint16(0x00FF)
    v[64:128] &= np.uint16(0xFF00)
    v[128:160] = 0
    v[160:176] = 0xFFFF
    q = rng.randint(0, 256, 1000).astype(np.uint8)
    q[:8] = (0, 1, 29, 30, 127, 128, 129, 255)
    seen = set()
    for require, exclude in ((0, 0), (0x2, 0x904), (0x0101, 0x8080), (0x0040, 0x0040)):
        for include_any in (0, 0x50, 0x0300, 0x0140, 0x0002, 0x0904, 0xFFFF):
            for exclude_all in (0, 0x000C, 0x0C00, 0x0108, 0x0100, 0x0050, 0xFFFF):
                for min_mapq in (0, 30, 127, 128, 200):
                    want = []
                    for i in range(1000):
                        x, m = int(v[i]), int(q[i])
                        want.append((x & require) == require and (x & exclude) == 0 and (include_any == 0 or (x & include_any) != 0)
                                    and (exclude_all == 0 or (x & exclude_all) != exclude_all) and (min_mapq == 0 or m >= min_mapq))
                    got = view_mask(v, require, exclude, include_any, exclude_all, q, min_mapq)
                    assert got.dtype == np.bool_ and got.tolist() == want, (require, exclude, include_any, exclude_all, min_mapq)
                    seen.add((bool(include_any), bool(exclude_all), bool(include_any & exclude_all), 0 < sum(want) < 1000))
    assert {(True, True, True, True), (True, False, False, True), (False, True, False, True), (False, False, False, True)} <= seen
    assert view_mask(v).all() and view_mask(v, 0, 0, 0, 0, None, 0).sum() == 1000
    from filter_oracle import filter_mask
    assert np.array_equal(view_mask(v, 0x2, 0x904, 0, 0, q, 30), filter_mask(v, 0x2, 0x904, q, 30))


# ------------------------------------------------------------------ the Python layer
def test_exports_and_shared_checks():
    import libflagstats_amd
    from libflagstats_amd import filter as flt
    from libflagstats_amd import filter_rf as rf
    for name in PY_NAMES:
        assert getattr(libflagstats_amd, name) is getattr(rf, name) and name in libflagstats_amd.__all__
    assert len(set(libflagstats_amd.__all__)) == len(libflagstats_amd.__all__)
    assert "``filter_rf``" in libflagstats_amd.__doc__
    # the checks are filter.py's, not restated
    assert rf._check_predicate is flt._check_predicate and rf._check_numpy is flt._check_numpy
    assert rf._check_mapq_numpy is flt._check_mapq_numpy and rf._check_mapq_torch is flt._check_mapq_torch
    src = open(os.path.join(ROOT, "libflagstats_amd", "filter_rf.py")).read()
    for text in ("must be a numpy.ndarray", "must have dtype", "must be 1-D", "must have one element per value", "must be a torch.Tensor",
                 "16-bit FLAG mask", "needs mapq", "must be in 0..255", "must be an int"):
        assert text not in src, text


def rf_refusals(call):
    """the refusals of the two new masks, in require's words; then the ones every filter entry shares"""
    for name in NEW_MASKS:
        for bad in (1.0, "4", None, True, np.float32(2)):
            with pytest.raises(ValueError, match=r"%s must be an int, not" % name):
                call(**{name: bad})
        for bad in (-1, 65536, 1 << 32):
            with pytest.raises(ValueError, match=r"%s must be a 16-bit FLAG mask \(0\.\.65535\), not %d" % (name, bad)):
                call(**{name: bad})
    # filter's predicate is asked first
    with pytest.raises(ValueError, match=r"exclude must be a 16-bit FLAG mask"):
        call(exclude=-1, include_any=65536)
    with pytest.raises(ValueError, match=r"min_mapq must be in 0\.\.255"):
        call(min_mapq=256, exclude_all=65536)
    predicate_refusals(call)


@pytest.mark.parametrize("fn", ["counters_filter_rf", "flagstats_filter_rf"])
def test_numpy_refusals(no_library, fn):  # noqa: F811
    from libflagstats_amd import filter_rf as rf
    f = getattr(rf, fn)
    v = np.zeros(20, dtype=np.uint16)
    q = np.zeros(20, dtype=np.uint8)
    with pytest.raises(ValueError, match=r"values must be a numpy\.ndarray, not list"):
        f([1, 2, 3])
    for bad in (np.zeros(20, dtype=np.int16), np.zeros(20, dtype=np.int32), np.zeros(20, dtype=bool), np.zeros(20, dtype=">u2")):
        with pytest.raises(ValueError, match=r"values must have dtype uint16, not " + re.escape(str(bad.dtype))):
            f(bad)
    with pytest.raises(ValueError, match=r"values must be 1-D, not 2-D"):
        f(np.zeros((4, 5), dtype=np.uint16))
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
    rf_refusals(lambda **kw: f(v, mapq=q, **kw))


def test_device_pointer_refusals(no_library):  # noqa: F811
    from libflagstats_amd import filter_rf as rf
    f = rf.count_device_ptr_filter_rf
    with pytest.raises(ValueError, match=r"n must not be negative"):
        f(0x1000, -1)
    for name, args, kw in (("ptr", (4096.0, 10), {}), ("n", (0x1000, 10.0), {}), ("n", (0x1000, True), {}),
                           ("mapq_ptr", (0x1000, 10), {"mapq_ptr": None}), ("mapq_ptr", (0x1000, 10), {"mapq_ptr": 8192.0})):
        with pytest.raises(ValueError, match=r"%s must be an int, not" % name):
            f(*args, **kw)
    for name, args, kw in (("ptr", (1 << 64, 10), {}), ("ptr", (-8, 10), {}), ("n", (0x1000, 1 << 64), {}),
                           ("mapq_ptr", (0x1000, 10), {"mapq_ptr": 1 << 64})):
        with pytest.raises(ValueError, match=r"%s must fit an unsigned 64-bit integer, not" % name):
            f(*args, **kw)
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq"):
        f(0x1000, 10, exclude_all=0xC, min_mapq=1)
    rf_refusals(lambda **kw: f(0x1000, 10, mapq_ptr=0x2000, **kw))


def test_torch_refusals(no_library):  # noqa: F811
    import torch
    from libflagstats_amd import filter_rf as rf
    f = rf.count_torch_filter_rf
    t = torch.zeros(20, dtype=torch.int16)
    q = torch.zeros(20, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"t must be a torch\.Tensor, not ndarray"):
        f(np.zeros(20, dtype=np.uint16))
    for dt in (torch.int32, torch.int64, torch.uint8, torch.bool, torch.float32):
        with pytest.raises(ValueError, match=r"t must have dtype int16 or uint16, not " + re.escape(str(dt))):
            f(torch.zeros(20, dtype=dt))
    for bad in (torch.zeros((4, 5), dtype=torch.int16), torch.zeros(40, dtype=torch.int16)[::2]):
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
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 0):
        with pytest.raises(ValueError, match=r"selected must be a contiguous int64 tensor of 1 element$"):
            f(t, selected=bad)
    with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
        f(t, require=2, exclude=0x904, include_any=0x50, exclude_all=0xC, mapq=q, min_mapq=30, out=torch.zeros(32, dtype=torch.int64))
    # (mapq / out / selected on another device than t: tests/test_gpu_filter_rf.py::test_device_dependent_refusals)


# ------------------------------------------------------------------ the C entries' own refusals (before any HIP call)
def test_c_refusals_of_the_new_masks():
    """include_any or exclude_all above 0xFFFF, in require's words, asked after filter's predicate and before everything else;
    the outputs stay as they were"""
    from libflagstats_amd import _lib
    lib = _lib.lib()
    a = np.zeros(104, dtype=np.uint16)
    q = np.zeros(104, dtype=np.uint8)
    out = np.full(32, 7, dtype=np.uint64)
    sel = ctypes.c_uint64(7)

    def call(name, require=1, exclude=4, include_any=0x50, exclude_all=0xC, flags=1, array=a.ctypes.data):
        args = [array, 100, require, exclude, include_any, exclude_all, q.ctypes.data, 30, out.ctypes.data, ctypes.byref(sel), flags]
        rc = getattr(lib, name)(*(args + [None] if PUBLIC[name] == 12 else args))
        assert (out == 7).all() and sel.value == 7
        return rc, lib.FLAGSTATS_hip_last_error().decode()

    for name in PUBLIC:
        for mask in NEW_MASKS:
            for bad in (0x10000, 0xFFFFFFFF):
                rc, text = call(name, **{mask: bad})
                assert rc != 0 and text.endswith("%s must be a 16-bit FLAG mask (at most 0xFFFF)" % mask), (name, mask, text)
        rc, text = call(name, include_any=0x10000, exclude_all=0x10000)
        assert rc != 0 and "include_any must be" in text
        rc, text = call(name, exclude=0x10000, include_any=0x10000)
        assert rc != 0 and "exclude must be a 16-bit FLAG mask (at most 0xFFFF)" in text
        rc, text = call(name, exclude_all=0x10000, flags=4)
        assert rc != 0 and "exclude_all must be" in text
        rc, text = call(name, exclude_all=0x10000, array=None)
        assert rc != 0 and "exclude_all must be" in text
        rc, text = call(name, flags=4)
        assert rc != 0 and "no other bits" in text
    # the text of the rule stands in flagstat_derived_host.h and in no unit
    holders = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip")) and "16-bit FLAG mask" in open(os.path.join(CSRC, fn)).read()]
    assert holders == ["flagstat_derived_host.h"]


# ------------------------------------------------------------------ symbols
def test_symbols_in_the_tables_the_library_the_headers_and_the_makefile():
    from libflagstats_amd import _lib
    u32, vp = ctypes.c_uint32, ctypes.c_void_p
    for name, nargs in PUBLIC.items():
        assert name in _lib.SIGNATURES and name not in _lib.INTERNAL_SIGNATURES, name
        restype, args = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(args) == nargs, name
        # array, n, require, exclude, include_any, exclude_all, mapq, min_mapq, out, selected, flags
        assert args[:11] == [vp, ctypes.c_uint64, u32, u32, u32, u32, vp, u32, vp, vp, ctypes.c_int], name
    for name, (_, nargs) in INTERNAL.items():
        assert name in _lib.INTERNAL_SIGNATURES and name not in _lib.SIGNATURES, name
        assert len(_lib.INTERNAL_SIGNATURES[name][1]) == nargs, name
    assert _lib.INTERNAL_SIGNATURES["fsk_launch_filter_rf"][1][:8] == [vp, ctypes.c_uint64, u32, u32, u32, u32, vp, u32]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in tuple(PUBLIC) + tuple(INTERNAL):
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    section = header[header.index("filtered, the whole predicate:"):header.index("filtered and selected:")]
    for name, nargs in PUBLIC.items():
        m = re.search(r"\bint %s\(([^)]*)\)" % name, section)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert len(re.findall(r"\b%s\(" % name, header)) == 1, name
    # the section states the predicate and the three things a call can be
    intro = section[:section.index("int FLAGSTATS_hip_device_u16_filter_rf(")]
    for text in ("(include_any == 0 || (array[i] & include_any) != 0)", "(exclude_all == 0 || (array[i] & exclude_all) != exclude_all)",
                 "nothing is launched or read", "the filtered entries' kernel", "fsk::flagstat_count_filter_rf", "above 0xFFFF"):
        assert text in intro, text
    # the launcher and the reduction are declared in the unit's internal header and nowhere else
    for fn in sorted(os.listdir(CSRC)) + [os.path.join(ROOT, "include", "libflagstats_hip.h"),
                                          os.path.join(ROOT, "include", "libflagstats_hip_probe.h")]:
        if not fn.endswith(".h"):
            continue
        text = open(os.path.join(CSRC, fn)).read()
        for name, (restype, nargs) in INTERNAL.items():
            m = re.search(r"^%s %s\(([^)]*)\)" % (restype, name), text, re.M)
            if os.path.basename(fn) == UNIT + ".h":
                assert m and len(m.group(1).split(",")) == nargs, name
            else:
                assert name not in text, (fn, name)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1)
    hdrs = re.search(r"^HDRS\s*:=(.*)$", mk, re.M).group(1)
    assert "$(HERE)%s.hip" % UNIT in srcs.split() and "$(HERE)%s.h" % UNIT in hdrs.split()


def test_code_objects():
    """K1's code object is still the one profiles/traffic.json was measured on; exactly one gfx950 code object defines
    fsk::flagstat_count_filter_rf, it holds all six instantiations (MAPQ read or not; the any-of test, the all-of test, both) and
    no other fsk::flagstat_* kernel: the unit calls fsk_launch_filter and instantiates no other unit's kernel"""
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
                   b"_ZN3fsk24flagstat_segments_filter", b"_ZN3fsk20flagstat_count_where", b"_ZN3fsk19flagstat_count_wide"):
        assert not KERNEL.startswith(prefix)
