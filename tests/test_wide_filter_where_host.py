"""The filtered and selected flagstat of int32 / int64 columns (libflagstats_amd/wide_filter_where.py,
csrc/flagstat_wide_filter_where.hip) on the CPU: the package's exports, every refusal of the Python layer -- raised before the
library is loaded --, the symbols in the binding tables, the built library and the headers, the identity of the code objects,
wide_filter_where_oracle against a per-element loop, and the model of the selection addresses the kernel's fast path forms.  The
kernel addresses its selection exactly as flagstat_count_wide_where does and launches on fsk_wide_where_geometry, so the model is
wide_where_oracle's, driven here over the cases in which a funnelled launch's first or last fast vector ends the array."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_filter_where_oracle as wfwo  # noqa: E402
import wide_where_oracle as wwo  # noqa: E402
from test_wide_where_host import BIT_OFFSETS, BYTE_OFFSETS, geometry  # noqa: E402
from wide_where_oracle import BITMAP, BYTES, pack, step_elems  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ("FLAGSTATS_hip_device_wide_filter_where", "FLAGSTATS_hip_device_wide_filter_where_sync", "FLAGSTATS_hip_wide_x64_filter_where")
INTERNAL = ("fsk_launch_wide_filter_where",)
PY_NAMES = ("counters_ints_filter_where", "flagstats_ints_filter_where", "count_device_ptr_ints_filter_where",
            "count_torch_ints_filter_where")
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
    from libflagstats_amd import wide_filter_where
    for name in PY_NAMES:
        assert getattr(libflagstats_amd, name) is getattr(wide_filter_where, name) and name in libflagstats_amd.__all__


def predicate_refusals(call, has_mapq_kw):
    """filter.py's refusals of (require, exclude, min_mapq); `call(**kw)` runs the entry with otherwise valid arguments and no
    MAPQ column, `has_mapq_kw` are the keywords that hand it one"""
    for name in ("require", "exclude"):
        for bad in (-1, 0x10000, 1 << 40):
            with pytest.raises(ValueError, match=r"%s must be a 16-bit FLAG mask \(0\.\.65535\), not %d" % (name, bad)):
                call(**{name: bad})
        for bad in (1.0, "4", None, True):
            with pytest.raises(ValueError, match=r"%s must be an int, not" % name):
                call(**{name: bad})
    for bad in (-1, 256):
        with pytest.raises(ValueError, match=r"min_mapq must be in 0\.\.255 \(MAPQ is one byte\), not %d" % bad):
            call(min_mapq=bad, **has_mapq_kw)
    for bad in (30.0, "30", True):
        with pytest.raises(ValueError, match=r"min_mapq must be an int, not"):
            call(min_mapq=bad, **has_mapq_kw)
    with pytest.raises(ValueError, match=r"min_mapq > 0 needs mapq \(one uint8 per value\)"):
        call(min_mapq=30)


@pytest.mark.parametrize("fn", ["counters_ints_filter_where", "flagstats_ints_filter_where"])
def test_numpy_refusals(no_library, fn):
    from libflagstats_amd import wide_filter_where
    f = getattr(wide_filter_where, fn)
    m = np.zeros(20, dtype=bool)
    q = np.zeros(20, dtype=np.uint8)
    # the value checks are wide.py's
    with pytest.raises(ValueError, match=r"values must be a numpy\.ndarray, not list"):
        f([1, 2, 3], m)
    for bad in (np.zeros(4, dtype=np.float32), np.zeros(4, dtype=bool), np.zeros(4, dtype=np.int8), np.zeros(4, dtype=np.uint8)):
        with pytest.raises(ValueError, match=r"values must have an integer dtype of 2, 4 or 8 bytes \(int16, uint16, int32, "
                                             r"uint32, int64, uint64\), not " + re.escape(str(bad.dtype))):
            f(bad, m)
    with pytest.raises(ValueError, match=r"native \(little-endian\) byte order"):
        f(np.zeros(4, dtype=">i4"), m)
    for dt in INT_DTYPES:
        v = np.zeros(20, dtype=dt)
        with pytest.raises(ValueError, match=r"values must be 1-D, not 2-D"):
            f(np.zeros((2, 3), dtype=dt), m)
        # the selection checks are where.py's
        with pytest.raises(ValueError, match=r"where must be a numpy\.ndarray, not list"):
            f(v, [True] * 20)
        with pytest.raises(ValueError, match=r"where must be 1-D, not 2-D"):
            f(v, np.zeros((4, 5), dtype=bool))
        with pytest.raises(ValueError, match=r"where must have dtype bool \(packed=True: a uint8 bitmap\), not uint8"):
            f(v, np.zeros(20, dtype=np.uint8))
        with pytest.raises(ValueError, match=r"where must have dtype uint8 with packed=True \(an LSB-first bitmap\), not bool"):
            f(v, m, packed=True)
        for size in (0, 19, 21):
            with pytest.raises(ValueError, match=r"where must have one element per value \(20\), not %d" % size):
                f(v, np.zeros(size, dtype=bool))
        with pytest.raises(ValueError, match=r"where holds 3 bytes, 20 values from bit 5 on need 4"):
            f(v, np.zeros(3, dtype=np.uint8), packed=True, bit_offset=5)
        with pytest.raises(ValueError, match=r"bit_offset needs packed=True"):
            f(v, m, bit_offset=3)
        with pytest.raises(ValueError, match=r"bit_offset must not be negative"):
            f(v, np.zeros(3, dtype=np.uint8), packed=True, bit_offset=-1)
        # the MAPQ and predicate checks are filter.py's
        with pytest.raises(ValueError, match=r"mapq must be a numpy\.ndarray, not list"):
            f(v, m, mapq=[0] * 20, min_mapq=1)
        with pytest.raises(ValueError, match=r"mapq must have dtype uint8, not int8"):
            f(v, m, mapq=np.zeros(20, dtype=np.int8), min_mapq=1)
        with pytest.raises(ValueError, match=r"mapq must be 1-D, not 2-D"):
            f(v, m, mapq=np.zeros((4, 5), dtype=np.uint8), min_mapq=1)
        for size in (0, 19, 21):
            with pytest.raises(ValueError, match=r"mapq must have one element per value \(20\), not %d" % size):
                f(v, m, mapq=np.zeros(size, dtype=np.uint8), min_mapq=1)
        predicate_refusals(lambda **kw: f(v, m, **kw), {"mapq": q})


def test_device_pointer_refusals(no_library):
    from libflagstats_amd import wide_filter_where
    f = wide_filter_where.count_device_ptr_ints_filter_where
    for eb in (2, 3, 16, 0, "4"):
        with pytest.raises(ValueError, match=r"elem_bytes must be 4 or 8 \(16-bit arrays: filter_where\.count_device_ptr_filter_where\), not"):
            f(0x1000, 10, eb, 0x2000, 1)
    for W in (4, 8):
        for sb in (0, 2, 4, 16, "1", True):
            with pytest.raises(ValueError, match=r"sel_bits must be 1 \(an LSB-first bitmap\) or 8 \(one byte per element\), not"):
                f(0x1000, 10, W, 0x2000, sb)
        with pytest.raises(ValueError, match=r"n must not be negative"):
            f(0x1000, -1, W, 0x2000, 1)
        with pytest.raises(ValueError, match=r"sel_offset must not be negative"):
            f(0x1000, 1, W, 0x2000, 8, sel_offset=-1)
        for name, args, kw in (("ptr", (4096.0, 10, W, 0x2000, 1), {}), ("n", (0x1000, 10.0, W, 0x2000, 1), {}),
                               ("sel_ptr", (0x1000, 10, W, None, 8), {}), ("sel_offset", (0x1000, 10, W, 0x2000, 8), {"sel_offset": 3.0}),
                               ("mapq_ptr", (0x1000, 10, W, 0x2000, 8), {"mapq_ptr": None})):
            with pytest.raises(ValueError, match=r"%s must be an int, not" % name):
                f(*args, **kw)
        for name, args, kw in (("ptr", (1 << 64, 10, W, 0x2000, 1), {}), ("ptr", (-8, 10, W, 0x2000, 1), {}),
                               ("n", (0x1000, 1 << 64, W, 0x2000, 1), {}), ("sel_ptr", (0x1000, 10, W, 1 << 64, 8), {}),
                               ("sel_offset", (0x1000, 10, W, 0x2000, 8), {"sel_offset": 1 << 64}),
                               ("mapq_ptr", (0x1000, 10, W, 0x2000, 8), {"mapq_ptr": -1})):
            with pytest.raises(ValueError, match=r"%s must fit an unsigned 64-bit integer, not" % name):
                f(*args, **kw)
        predicate_refusals(lambda **kw: f(0x1000, 10, W, 0x2000, 1, **kw), {"mapq_ptr": 0x3000})


def test_torch_refusals(no_library):
    import torch
    from libflagstats_amd import wide_filter_where
    f = wide_filter_where.count_torch_ints_filter_where
    m = torch.zeros(20, dtype=torch.bool)
    q = torch.zeros(20, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"t must be a torch\.Tensor, not ndarray"):
        f(np.zeros(4, dtype=np.int32), m)
    for dt in (torch.float32, torch.bool, torch.int8, torch.uint8):
        with pytest.raises(ValueError, match=r"t must have an integer dtype of 2, 4 or 8 bytes, not " + re.escape(str(dt))):
            f(torch.zeros(4, dtype=dt), m)
    for dt in (torch.int16, torch.int32, torch.int64):
        t = torch.zeros(20, dtype=dt)
        for bad in (torch.zeros((2, 3), dtype=dt), torch.zeros(8, dtype=dt)[::2]):
            with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
                f(bad, m)
        with pytest.raises(ValueError, match=r"where must be a torch\.Tensor, not ndarray"):
            f(t, np.zeros(20, dtype=bool))
        with pytest.raises(ValueError, match=r"where must be 1-D and contiguous"):
            f(t, torch.zeros((4, 5), dtype=torch.bool))
        with pytest.raises(ValueError, match=r"where must have dtype torch\.bool \(packed=True: a torch\.uint8 bitmap\), not torch\.uint8"):
            f(t, torch.zeros(20, dtype=torch.uint8))
        with pytest.raises(ValueError, match=r"where must have dtype torch\.uint8 with packed=True \(an LSB-first bitmap\), not torch\.bool"):
            f(t, m, packed=True)
        for size in (0, 19, 21):
            with pytest.raises(ValueError, match=r"where must have one element per value \(20\), not %d" % size):
                f(t, torch.zeros(size, dtype=torch.bool))
        with pytest.raises(ValueError, match=r"where holds 3 bytes, 20 values from bit 7 on need 4"):
            f(t, torch.zeros(3, dtype=torch.uint8), packed=True, bit_offset=7)
        with pytest.raises(ValueError, match=r"bit_offset needs packed=True"):
            f(t, m, bit_offset=1)
        with pytest.raises(ValueError, match=r"mapq must be a torch\.Tensor, not ndarray"):
            f(t, m, mapq=np.zeros(20, dtype=np.uint8), min_mapq=1)
        with pytest.raises(ValueError, match=r"mapq must have dtype torch\.uint8, not torch\.int8"):
            f(t, m, mapq=torch.zeros(20, dtype=torch.int8), min_mapq=1)
        with pytest.raises(ValueError, match=r"mapq must be 1-D and contiguous"):
            f(t, m, mapq=torch.zeros(40, dtype=torch.uint8)[::2], min_mapq=1)
        for size in (0, 19, 21):
            with pytest.raises(ValueError, match=r"mapq must have one element per value \(20\), not %d" % size):
                f(t, m, mapq=torch.zeros(size, dtype=torch.uint8), min_mapq=1)
        predicate_refusals(lambda **kw: f(t, m, **kw), {"mapq": q})
        for bad in (torch.zeros(31, dtype=torch.int64), torch.zeros(32, dtype=torch.int32), np.zeros(32, dtype=np.int64)):
            with pytest.raises(ValueError, match=r"out must be a contiguous int64 tensor of 32 elements"):
                f(t, m, out=bad)
        for name in ("selected", "high"):
            for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 0):
                with pytest.raises(ValueError, match=r"%s must be a contiguous int64 tensor of 1 element$" % name):
                    f(t, m, **{name: bad})
        with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
            f(t, m, mapq=q, min_mapq=3)               # host tensors
    # (where / mapq / out / selected / high on another device than t: tests/test_gpu_wide_filter_where.py::test_python_layers)


def test_the_checks_are_shared_not_copied():
    """wide_filter_where.py holds no refusal text of wide.py's, where.py's or filter.py's: it calls their functions"""
    src = open(os.path.join(ROOT, "libflagstats_amd", "wide_filter_where.py")).read()
    for text in ("must be a numpy.ndarray", "integer dtype of 2, 4 or 8 bytes", "byte order", "must be 1-D", "one element per value",
                 "must have dtype", "needs packed=True", "sel_bits must be", "values outside 0..65535", "must be a torch.Tensor",
                 "must be a CUDA tensor", "16-bit FLAG mask", "needs mapq"):
        assert text not in src, text
    for call in ("_wide._check_values(", "_wide._check_tensor(", "_wide.high_bits_message(", "_where._check_selection_numpy(",
                 "_where._check_selection_torch(", "_where._check_sel_bits(", "_filter._check_mapq_numpy(", "_filter._check_mapq_torch(",
                 "_filter._check_predicate("):
        assert call in src, call


def test_symbols_in_the_tables_the_library_and_the_headers():
    from libflagstats_amd import _lib
    for name in PUBLIC:
        assert name in _lib.SIGNATURES and name not in _lib.INTERNAL_SIGNATURES, name
    for name in INTERNAL:
        assert name in _lib.INTERNAL_SIGNATURES and name not in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_wide_filter_where"][1]) == 15
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_wide_filter_where_sync"][1]) == 14
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_wide_x64_filter_where"][1]) == 14
    assert len(_lib.INTERNAL_SIGNATURES["fsk_launch_wide_filter_where"][1]) == 16
    for name in PUBLIC + INTERNAL:
        args = (_lib.SIGNATURES if name in PUBLIC else _lib.INTERNAL_SIGNATURES)[name][1]
        assert args[1] is ctypes.c_uint64 and args[2] is ctypes.c_int, name                              # n, elem_bytes
        assert args[3] is ctypes.c_uint32 and args[4] is ctypes.c_uint32, name                           # require, exclude
        assert args[5] is ctypes.c_void_p and args[6] is ctypes.c_uint32, name                           # mapq, min_mapq
        assert args[7] is ctypes.c_void_p and args[8] is ctypes.c_uint64 and args[9] is ctypes.c_int, name   # sel, sel_offset, sel_bits
        assert args[10:13] == [ctypes.c_void_p] * 3 and args[13] is ctypes.c_int, name                   # out, selected, high, flags
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in PUBLIC + INTERNAL:
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    for name in PUBLIC:
        m = re.search(r"\bint %s\(([^)]*)\)" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    internal = open(os.path.join(ROOT, "libflagstats_amd", "csrc", "flagstat_wide_filter_where.h")).read()
    for name in INTERNAL:
        m = re.search(r"\bhipError_t %s\(([^)]*)\)" % name, internal)
        assert m and name not in header, name
        assert len(m.group(1).split(",")) == len(_lib.INTERNAL_SIGNATURES[name][1]), name
    # both say whose bits `high` holds
    assert "PASSING OR NOT" in header and "PASSING OR NOT" in internal


def test_code_objects():
    """K1's code object is still the one profiles/traffic.json was measured on; exactly one gfx950 code object defines
    fsk::flagstat_count_wide_filter_where, it holds all twelve instantiations (W 4 and 8; with and without MAPQ; bitmap plain and
    funnelled, bytes), and it is not the code object of K1 or of either parent"""
    from libflagstats_amd import _lib, kernel_id
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        recorded = json.load(f)["kernel_source_id"]
    assert kernel_id.kernel_id(_lib.LIB_PATH) == recorded
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    others = {"k1": b"_ZN3fsk14flagstat_count", "wide_filter": b"_ZN3fsk26flagstat_count_wide_filter",
              "wide_where": b"_ZN3fsk25flagstat_count_wide_where", "filter_where": b"_ZN3fsk21flagstat_filter_where"}
    new = [b"_ZN3fsk32flagstat_count_wide_filter_whereILi%dELb%dELi%dELb%dE" % (W, mapq, bits, funnel)
           for W in (4, 8) for mapq in (0, 1) for bits, funnel in ((1, 0), (1, 1), (8, 0))]
    assert len(set(new)) == 12
    found = {k: [] for k in others}
    mine = []
    for i, co in enumerate(kernel_id._code_objects(so)):
        secs = kernel_id._sections(co)
        names = b"".join(co[secs[t][0]:secs[t][0] + secs[t][1]] for t in (".strtab", ".dynstr") if t in secs)
        for k, prefix in others.items():
            if prefix in names:
                found[k].append(i)
        if b"flagstat_count_wide_filter_where" in names:
            assert all(n in names for n in new), i
            mine.append(i)
    assert all(len(v) == 1 for v in found.values()), found
    assert len(mine) == 1 and all(mine[0] != v[0] for v in found.values()), (mine, found)


def test_oracle_equals_a_loop_over_the_elements(oracle_mod):
    """wide_filter_where_oracle.want against the definition, element by element, on a few hundred random elements: an element is
    counted when it passes and is selected, `high` takes the selected ones, passing or not"""
    rng = np.random.RandomState(5)
    for dt in ("int32", "uint32", "int64", "uint64"):
        W = np.dtype(dt).itemsize
        n = 300
        u = rng.randint(0, 65536, n).astype(wwo.UNSIGNED[W])
        for i in rng.randint(0, n, 40):
            u[i] |= wwo.UNSIGNED[W](1 << int(rng.randint(16, 8 * W)))
        v = u.view(dt)
        mask = rng.randint(0, 2, n).astype(bool)
        mapq = rng.randint(0, 61, n).astype(np.uint8)
        for require, exclude, min_mapq in ((0, 0, 0), (0, 0x904, 0), (0x2, 0x904, 30), (0x1, 0, 60), (0x40, 0x40, 0), (0, 0, 255)):
            kept, high, count = [], 0, 0
            for i in range(n):
                e = int(u[i])
                f = e & 0xFFFF
                if mask[i]:
                    high |= e & ~0xFFFF
                if mask[i] and (f & require) == require and (f & exclude) == 0 and (min_mapq == 0 or mapq[i] >= min_mapq):
                    kept.append(f)
                    count += 1
            if require & exclude:
                high = 0
            c, selected, h = wfwo.want(oracle_mod, v, mask, require, exclude, mapq, min_mapq)
            assert selected == count and h == high, (dt, require, exclude, min_mapq)
            assert np.array_equal(c, oracle_mod.flagstat_c(np.array(kept, dtype=np.uint16)).astype(np.uint64))
            sup = wfwo.want(oracle_mod, v, mask, require, exclude, mapq, min_mapq, superset=True)[0]
            assert int(sup[9]) == count - int(c[25]) and np.array_equal(np.delete(sup, [0, 9, 16]), np.delete(c, [0, 9, 16]))
    v = np.zeros(0, dtype=np.int32)
    c, selected, h = wfwo.want(oracle_mod, v, np.zeros(0, dtype=bool), 0, 0x904)
    assert not c.any() and selected == 0 and h == 0


def end_cases():
    """(W, n, address): sizes around a vector and one, two and three steps at every array phase -- among them the arrays whose
    last fast vector ends the array (phase 0, n a multiple of a step) and, funnelled, those whose first fast vector is the first
    of step 1"""
    for W in (4, 8):
        S = step_elems(W)
        for n in (1, 3, 16 // W, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S, 3 * S - 16 // W):
            for phase in range(16 // W):
                yield W, n, 0x7F00_0000_1000 + W * phase, phase


def test_selection_addresses_of_the_fast_path():
    """The kernel launches on fsk_wide_where_geometry and addresses its selection as flagstat_count_wide_where does: a lane's
    byte index, its shift, and which two adjacent bytes it loads when funnelled.  The model forms no address outside
    geo[6 .. 8) -- including funnelled launches whose first or last fast vector ends the array --, a funnelled launch has no fast
    vector in step 0, and the bits the model extracts from a random bitmap are the mask"""
    f = geometry()
    geo = (ctypes.c_uint64 * 8)()
    rng = np.random.RandomState(23)
    checked = funnelled_to_the_end = funnelled_from_step_one = 0
    for W, n, addr, phase in end_cases():
        EPV = 16 // W
        mask = rng.randint(0, 2, n).astype(bool)
        for off in BIT_OFFSETS:
            for grid in (1, 3):
                assert f(addr, n, W, off, BITMAP, grid, geo) == 0
                g = list(geo)
                j, first, d, sh, funnel = wwo.fast_path_bitmap_model(g, W, off)
                if j.size == 0:
                    continue
                last = first + 1 if funnel else first
                assert (first >= g[6]).all() and (last < g[7]).all(), (W, n, phase, off)
                assert (sh + EPV <= (16 if funnel else 8)).all()
                if funnel:
                    assert j.min() >= wwo.VPS
                    funnelled_to_the_end += int((j.max() + 1) * EPV == g[1])        # the last fast vector ends the array
                    funnelled_from_step_one += int(j.min() == wwo.VPS)
                if off < 1 << 30 and grid == 1:
                    sel = pack(mask, off)
                    w = sel[first].astype(np.uint32) | (sel[last].astype(np.uint32) << 8 if funnel else 0)
                    bits = (w >> sh.astype(np.uint32)) & ((1 << EPV) - 1)
                    for e in range(EPV):
                        assert np.array_equal((bits >> e) & 1, mask[j * EPV + e - g[0]].astype(np.uint32)), (W, n, phase, off, e)
                    checked += 1
        for off in BYTE_OFFSETS:
            assert f(addr, n, W, off, BYTES, 3, geo) == 0
            g = list(geo)
            j, first, count = wwo.fast_path_bytes_model(g, W, off)
            if j.size == 0:
                continue
            assert (first >= g[6]).all() and (first + count <= g[7]).all(), (W, n, phase, off)
            # the MAPQ bytes of the same vector: count bytes from j * EPV - lo of d_mapq[0 .. n)
            mq = j * EPV - g[0]
            assert (mq >= 0).all() and (mq + count <= n).all(), (W, n, phase)
    assert checked and funnelled_to_the_end and funnelled_from_step_one


def test_the_kernel_addresses_its_selection_as_the_parent_does():
    """what lets the model above stand for this kernel: the lines that derive a lane's byte, shift and straddle, the funnelled
    start and the launcher's funnelled step split are the parent's, character for character"""
    here = os.path.join(ROOT, "libflagstats_amd", "csrc")
    mine = open(os.path.join(here, "flagstat_wide_filter_where.hip")).read()
    parent = open(os.path.join(here, "flagstat_wide_where.hip")).read()
    for line in ("const uint32_t lane_bit = lane_vec * EPV + (SEL_BITS == 1 ? shift : 0u);",
                 "const uint32_t d = FUNNEL && (lane_bit & 7u) + EPV > 8u ? 1u : 0u;",
                 "const uint32_t sh = SEL_BITS == 1 ? (lane_bit & 7u) + (FUNNEL ? 8u * (1u - d) : 0u) : 0u;",
                 "const uint8_t* ps = sel + st * (VPS * EPV / SDIV) + (SEL_BITS == 1 ? lane_bit >> 3 : lane_bit);",
                 "if constexpr (FUNNEL) ps = ps + d - 1;",
                 "const uint64_t bit0 = sel_offset + 8 - lo;",
                 "sel = reinterpret_cast<const uint8_t*>(sel0 + (bit0 >> 3) - 1);",
                 "geo[3] = 1;",
                 "if (geo[4] < 1) geo[4] = 1;"):
        assert line in mine and line in parent, line
    assert "fsk_wide_where_geometry(" in mine
