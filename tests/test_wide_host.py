"""The wide-input flagstat (int32 / int64 FLAG arrays, libflagstats_amd/wide.py, csrc/flagstat_wide.hip) on the CPU: every
refusal of the Python layer and its text -- raised before the library is loaded --, the symbols in the binding table and in the
built library, the identity of K1's code object, and the launcher's step constants and geometry against steps_oracle."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from steps_oracle import EPOCH, STAGGER, STEP_WORDS, WAVES, StepSplit  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("FLAGSTATS_hip_device_wide", "FLAGSTATS_hip_device_wide_sync", "FLAGSTATS_hip_wide_x64", "fsk_launch_wide",
               "fsk_wide_geometry")


@pytest.fixture()
def no_library(monkeypatch):
    """loading the library fails the test: the refusals must come first"""
    from libflagstats_amd import _lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were refused")

    monkeypatch.setattr(_lib, "lib", boom)


def test_exports():
    import libflagstats_amd
    from libflagstats_amd import wide
    for name in ("counters_ints", "flagstats_ints", "count_device_ptr_ints", "count_torch_ints"):
        assert getattr(libflagstats_amd, name) is getattr(wide, name) and name in libflagstats_amd.__all__


@pytest.mark.parametrize("fn", ["counters_ints", "flagstats_ints"])
def test_numpy_refusals(no_library, fn):
    from libflagstats_amd import wide
    f = getattr(wide, fn)
    with pytest.raises(ValueError, match=r"values must be a numpy\.ndarray, not list"):
        f([1, 2, 3])
    for bad in (np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.float64), np.zeros(4, dtype=bool),
                np.array([1, 2], dtype=object), np.zeros(4, dtype=np.int8), np.zeros(4, dtype=np.uint8),
                np.zeros(4, dtype="S2"), np.zeros(4, dtype=np.complex64)):
        with pytest.raises(ValueError, match=r"values must have an integer dtype of 2, 4 or 8 bytes \(int16, uint16, int32, "
                                             r"uint32, int64, uint64\), not " + re.escape(str(bad.dtype))):
            f(bad)
    for dt in ("int16", "uint16", "int32", "uint32", "int64", "uint64"):
        with pytest.raises(ValueError, match=r"values must be 1-D, not 2-D"):
            f(np.zeros((2, 3), dtype=dt))
        with pytest.raises(ValueError, match=r"values must be 1-D, not 0-D"):
            f(np.array(5, dtype=dt))
    with pytest.raises(ValueError, match=r"native \(little-endian\) byte order"):
        f(np.zeros(4, dtype=">i4"))


def test_device_pointer_refusals(no_library):
    from libflagstats_amd import wide
    for eb in (2, 3, 16, 0, "4"):
        with pytest.raises(ValueError, match=r"elem_bytes must be 4 or 8 \(16-bit arrays: device\.count_device_ptr\), not"):
            wide.count_device_ptr_ints(0x1000, 10, eb)
    with pytest.raises(ValueError, match=r"n must not be negative"):
        wide.count_device_ptr_ints(0x1000, -1, 4)


def test_torch_refusals(no_library):
    import torch
    from libflagstats_amd import wide
    f = wide.count_torch_ints
    with pytest.raises(ValueError, match=r"t must be a torch\.Tensor, not ndarray"):
        f(np.zeros(4, dtype=np.int32))
    for dt in (torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.bool, torch.int8, torch.uint8, torch.complex64):
        with pytest.raises(ValueError, match=r"t must have an integer dtype of 2, 4 or 8 bytes, not " + re.escape(str(dt))):
            f(torch.zeros(4, dtype=dt))
    for dt in (torch.int16, torch.int32, torch.int64):
        with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
            f(torch.zeros(4, dtype=dt))       # a host tensor
    for dt in (torch.int16, torch.int32, torch.int64):
        with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
            f(torch.zeros((2, 3), dtype=dt))
        with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
            f(torch.zeros(8, dtype=dt)[::2])
        with pytest.raises(ValueError, match=r"t must be 1-D and contiguous"):
            f(torch.zeros((), dtype=dt))
    t = torch.zeros(4, dtype=torch.int32)
    for bad in (torch.zeros(31, dtype=torch.int64), torch.zeros(32, dtype=torch.int32), torch.zeros(64, dtype=torch.int64)[::2],
                np.zeros(32, dtype=np.int64)):
        with pytest.raises(ValueError, match=r"out must be a contiguous int64 tensor of 32 elements"):
            f(t, out=bad)
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 0):
        with pytest.raises(ValueError, match=r"high must be a contiguous int64 tensor of 1 element$"):
            f(t, high=bad)
    with pytest.raises(ValueError, match=r"t must be a CUDA tensor"):
        f(t, out=torch.zeros(32, dtype=torch.int64), high=torch.zeros(1, dtype=torch.int64))
    # (out / high on another device than t: tests/test_gpu_wide.py::test_python_torch_refusals_that_need_a_device)


def test_strict_message():
    from libflagstats_amd import wide
    assert wide.high_bits_message(0xFFFF0000) == "values outside 0..65535: bits 0xFFFF0000 set above bit 15"
    assert wide.high_bits_message(1 << 63) == "values outside 0..65535: bits 0x8000000000000000 set above bit 15"


def test_symbols_in_the_table_and_the_library():
    from libflagstats_amd import _lib
    # the public entries sit in SIGNATURES (which test_host_logic.py holds equal to the public headers), the two launcher symbols
    # of csrc/flagstat_wide.h in INTERNAL_SIGNATURES; lib() attaches both tables
    for name in NEW_SYMBOLS[:3]:
        assert name in _lib.SIGNATURES, name
    for name in NEW_SYMBOLS[3:]:
        assert name in _lib.INTERNAL_SIGNATURES and name not in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["FLAGSTATS_hip_device_wide"][1][2] is ctypes.c_int
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_wide"][1]) == 7
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_device_wide_sync"][1]) == 6
    assert len(_lib.SIGNATURES["FLAGSTATS_hip_wide_x64"][1]) == 6
    assert len(_lib.INTERNAL_SIGNATURES["fsk_launch_wide"][1]) == 8
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in NEW_SYMBOLS:
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "libflagstats_hip.h")).read()
    for name in NEW_SYMBOLS[:3]:
        assert re.search(r"\bint %s\(" % name, header), name
    internal = open(os.path.join(ROOT, "libflagstats_amd", "csrc", "flagstat_wide.h")).read()
    for name in NEW_SYMBOLS[3:]:
        assert re.search(r"\bhipError_t %s\(" % name, internal), name


def test_k1_code_object_is_the_recorded_one():
    """fsk::flagstat_count's code object is the one profiles/traffic.json was measured on (the wide kernel lives in a translation
    unit, hence a code object, of its own), and exactly one other gfx950 code object defines fsk::flagstat_count_wide"""
    from libflagstats_amd import _lib, kernel_id
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        recorded = json.load(f)["kernel_source_id"]
    assert kernel_id.kernel_id(_lib.LIB_PATH) == recorded
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    k1, wide = [], []
    for i, co in enumerate(kernel_id._code_objects(so)):
        secs = kernel_id._sections(co)
        names = b"".join(co[secs[t][0]:secs[t][0] + secs[t][1]] for t in (".strtab", ".dynstr") if t in secs)
        if b"_ZN3fsk14flagstat_count" in names:
            k1.append(i)
        if b"_ZN3fsk19flagstat_count_wideILi4" in names:
            assert b"_ZN3fsk19flagstat_count_wideILi8" in names
            wide.append(i)
    assert len(k1) == 1 and len(wide) == 1 and k1 != wide, (k1, wide)


def _source(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return re.sub(r"\s+", " ", f.read())


def test_wide_step_mirror_matches_the_sources():
    """steps_oracle.StepSplit(addr % 16, n * W / 2, grid) is the wide launcher's step split: its constants and rules, read back
    out of flagstat_wide.hip"""
    k1h = _source("libflagstats_amd", "csrc", "flagstat_kernels.h")
    w = _source("libflagstats_amd", "csrc", "flagstat_wide.hip")
    core = _source("libflagstats_amd", "csrc", "flagstat_count_core.h")      # the shared device pieces
    host = _source("libflagstats_amd", "csrc", "flagstat_derived_host.h")    # the shared step split
    threads = int(re.search(r"constexpr int kThreads = (\d+);", k1h).group(1))
    unroll = int(re.search(r"constexpr int kUnroll = (\d+);", k1h).group(1))
    assert threads == 64 * WAVES and threads * unroll * 16 == 2 * STEP_WORDS == 32768     # 32 KiB steps
    assert host.count("constexpr int kStepBytes = fsk::kVecPerStep * 16;") == 1 and "constexpr int VPS = kVecPerStep;" in w
    assert (1 << int(re.search(r"constexpr int kWideDepth = (\d+);", w).group(1))) - 1 == EPOCH
    assert core.count("if (blk == (1u << DEPTH) - 1u) { flush(s, (1u << DEPTH) - 1u); blk = 0; }") == 1
    assert "wide_step<W, ROLL>(s, v, blk, or_even, or_odd, cur, next); end_step<kWideDepth>(s, blk);" in w
    assert core.count("return (wave & 3u) * %du;" % STAGGER) == 1 and "uint32_t blk = stagger_start(wave);" in w
    for rule in ("const uint64_t base = addr & ~static_cast<uint64_t>(15);",
                 "const uint64_t epv = 16 / W;",
                 "const uint64_t lo = (addr - base) / W, hi = lo + n;",
                 "const uint64_t nvec = (hi + epv - 1) / epv;",
                 "const uint64_t vps = fsk::kVecPerStep;",
                 "const uint64_t nsteps = (nvec + vps - 1) / vps;",
                 "uint64_t fast_begin = (lo == 0) ? 0 : 1;",
                 "uint64_t fast_end = (hi / epv) / vps;",
                 "if (fast_end < fast_begin) fast_end = fast_begin;",
                 "if (static_cast<uint64_t>(grid) > nsteps) grid = static_cast<uint32_t>(nsteps);"):
        assert host.count(rule) == 1, rule
    assert "return fsdrv::step_split(address, n, elem_bytes, grid, geo);" in w
    # the kernel's push order: head edge, tail edge, fast steps from b (+G below fast_begin)
    assert "if (fast_begin != 0 && blockIdx.x == 0) edge_step(0);" in w
    assert "if (nsteps > fast_end && nsteps - 1 >= fast_begin && (nsteps - 1) % G == blockIdx.x) edge_step(nsteps - 1);" in w
    assert "uint64_t st = blockIdx.x; if (st < fast_begin) st += G;" in w
    assert w.index("edge_step(0);") < w.index("edge_step(nsteps - 1);") < w.index("if (st < fast_end) {")
    # rolling re-issue at a distance of 6 vectors, each wave a contiguous 8 KiB
    assert core.count("constexpr int kRollDistance = 6;") == 1 and core.count("constexpr int kWaveStride = 64;") == 1
    assert "reissue<ROLL>(u, v, cur, next, kWaveStride, load_vec<true>);" in w and "constexpr int US = kWaveStride;" in w
    assert "constexpr int RD = kRollDistance;" in w and "for (int u = 0; u < RD; ++u) {" in w


def test_wide_geometry_equals_the_step_split():
    """fsk_wide_geometry (the arithmetic fsk_launch_wide launches with; host code, no GPU) against StepSplit, at every element
    phase of a 16-byte line, and what the launcher refuses"""
    from libflagstats_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    f = lib.fsk_wide_geometry
    f.restype, f.argtypes = _lib.INTERNAL_SIGNATURES["fsk_wide_geometry"]
    geo = (ctypes.c_uint64 * 6)()
    rng = np.random.RandomState(5)
    for W in (4, 8):
        S = 32768 // W
        sizes = [1, 2, 3, 5, S - 1, S, S + 1, 2 * S - 1, 2 * S + 1, 255 * S, 7 * 1003 * S + 11]
        sizes += [int(x) for x in rng.randint(1, 40 * S, 40)]
        for phase in range(16 // W):
            for n in sizes:
                for grid in (1, 2, 3, 7, 256):
                    addr = 0x7F00_0000_1000 + phase * W
                    assert f(addr, n, W, grid, geo) == 0
                    s = StepSplit(addr % 16, n * W // 2, grid)
                    assert list(geo) == [s.lo * 2 // W, s.hi * 2 // W, s.nsteps, s.fast_begin, s.fast_end, s.grid], (W, phase, n, grid)
        assert f(0x1000, 0, W, 4, geo) == 0 and list(geo) == [0] * 6
        assert f(0x1000 + W // 2, 10, W, 4, geo) != 0          # misaligned
        assert f(0x1000, 10, W, 0, geo) != 0                   # no workgroups
        # a wave's totals are uint32: grid 1 over 2^34 elements is refused, the same array on 256 workgroups is not
        assert f(0x1000, 1 << 34, W, 1, geo) != 0
        assert f(0x1000, 1 << 34, W, 256, geo) == 0
        per_wave_step = S // 4
        n_ok = ((1 << 32) // per_wave_step - 4) * S
        assert f(0x1000, n_ok, W, 1, geo) == 0 and (geo[2] + 2) * per_wave_step < 1 << 32
    for W in (0, 1, 2, 3, 16):
        assert f(0x1000, 10, W, 4, geo) != 0
