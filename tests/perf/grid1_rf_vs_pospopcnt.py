"""Launch-only times of the grid-1 calls of tests/test_gpu_derived_limits.py::test_rf_units_one_workgroup_past_2_pow_32 beside
their yardstick, tests/test_gpu_epoch_regimes.py::test_pospopcnt_wave_totals_past_2_31, in one process: device events around each
single launch on the null stream, nothing of the tests' oracle or set-up inside.  One workgroup reads the whole column, so the
figure is what ONE workgroup sustains, bytes read over the event time; the yardstick scaled by bytes plus 15 % is the allowance.
The filtered parent (fsk_launch_filter, fsk_launch_wide_filter) under -q 1 on the same columns is timed as well: it reads the
same bytes without the --rf / -G tests.

    python tests/perf/grid1_rf_vs_pospopcnt.py          # needs about 45 GiB of device memory
"""
import ctypes
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import periodic_oracle as po  # noqa: E402
import test_gpu_derived_limits as lim  # noqa: E402
from libflagstats_amd import _lib  # noqa: E402

REPEATS = 3
GIB = float(1 << 30)


def timed(launch):
    """milliseconds of each of REPEATS single launches, by device events"""
    out = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        rc = launch()
        b.record()
        torch.cuda.synchronize()
        assert rc == 0, rc
        out.append(a.elapsed_time(b))
    return out


def report(name, nbytes, ms, yard=None):
    best = min(ms)
    rate = nbytes / GIB / (best / 1e3)
    line = "%-46s %6.2f GiB  %s ms  best %8.2f ms = %6.2f GiB/s" % (name, nbytes / GIB, " ".join("%8.2f" % m for m in ms), best, rate)
    if yard is not None:
        allowed = yard * nbytes * 1.15
        line += "   allowance %8.2f ms: %s (%.3f of the yardstick's time per byte)" % (allowed, "inside" if best <= allowed else "OVER",
                                                                                      best / (yard * nbytes))
    print(line, flush=True)
    return best / nbytes


def main():
    hip = _lib.lib()
    assert hip.FLAGSTATS_hip_available() == 1
    pos = hip.fsk_launch_pospopcnt
    pos.restype = ctypes.c_int
    pos.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    # the yardstick first: 2^33 + 2^20 all-ones words, grid 1, both epilogue forms
    n = (1 << 33) + (1 << 20)
    t = torch.full((n,), -1, dtype=torch.int16, device="cuda")
    out = torch.zeros(16, dtype=torch.int64, device="cuda")
    parts = torch.zeros(16, dtype=torch.int64, device="cuda")
    yard = min(report("fsk_launch_pospopcnt grid 1 direct=%d" % d, 2 * n, timed(lambda: pos(t.data_ptr(), n, 1, parts.data_ptr(), out.data_ptr(), None, d)))
               for d in (1, 0))
    del t
    torch.cuda.empty_cache()
    shared = lim.Shared()
    require, exclude, include_any, exclude_all, min_mapq = po.RF_DENSE
    Q = shared.mapq.data_ptr() + lim.PAD
    res = torch.zeros(34, dtype=torch.int64, device="cuda")
    OUT, SEL, HIGH = res.data_ptr(), res.data_ptr() + 256, res.data_ptr() + 264
    mode = lim.STORE | lim.SUPERSET
    for W in (2, 4):
        slab = lim.Slab(W)
        A, m = slab.base, slab.n
        nbytes = m * W + m
        if W == 2:
            report("fsk_launch_filter grid 1, -q 1 (uint16)", nbytes,
                   timed(lambda: hip.fsk_launch_filter(A, m, 0, 0, Q, min_mapq, OUT, SEL, mode, 1, None)), yard)
            report("fsk_launch_filter_rf grid 1, RF_DENSE (uint16)", nbytes,
                   timed(lambda: hip.fsk_launch_filter_rf(A, m, require, exclude, include_any, exclude_all, Q, min_mapq, OUT, SEL, mode, 1, None)), yard)
        else:
            report("fsk_launch_wide_filter grid 1, -q 1 (int32)", nbytes,
                   timed(lambda: hip.fsk_launch_wide_filter(A, m, 4, 0, 0, Q, min_mapq, OUT, SEL, HIGH, mode, 1, None)), yard)
            report("fsk_launch_wide_filter_rf grid 1, RF_DENSE (int32)", nbytes,
                   timed(lambda: hip.fsk_launch_wide_filter_rf(A, m, 4, require, exclude, include_any, exclude_all, Q, min_mapq, OUT, SEL, HIGH,
                                                               mode, 1, None)), yard)
        slab.t = None
        del slab
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
