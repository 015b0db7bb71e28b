#!/usr/bin/env python3
"""Filtered wide-input flagstat under samtools' whole FLAG predicate at full size: `python3 tests/perf/wide_filter_rf_sweep.py
[--bytes N] [--rounds R] [--reps K] [--buffers B] [--check-elements N] [--quick]` -- per width, B (default 2) device-resident
columns of N bytes (default 8 GiB: every pass reads 32 times the 256 MiB cache) of int32 / int64 elements whose low halves are
NA12878-like flags (filled on the device) and one uint8 MAPQ column beside them (three quarters 60, the rest uniform in 0..59),
timed with hipEvents after warm-up.  The calls of a timed window rotate over the B columns.  Every arm is -F 0x904 plus what it
names, without and with -q 30, and runs ALTERNATING with its yardstick in the same process, both widths in one run:

  (a)  FLAGSTATS_hip_device_wide_filter with -F 0x904 [-q 30]: fsk::flagstat_count_wide_filter, which moves the same bytes
  (b1) FLAGSTATS_hip_device_wide_filter_rf with --rf 0x50         the any-of test alone      flagstat_count_wide_filter_rf<W, ., 1, 0>
  (b2) ... with -G 0x420                                          the all-of test alone      <W, ., 0, 1>
  (b3) ... with --rf 0x210 -G 0x480                               both, across byte planes   <W, ., 1, 1>
  (b4) ... with --rf 0x40                                         reduced to -f 0x40 -F 0x904: flagstat_count_wide_filter itself

The yardstick of (b) is (a)'s time in the same rounds plus 3 %: the bytes moved are the same.  Printed: median ms per call over
the rounds with the spread, (b)/(a), MET or MISSED, and the element rate.  Before anything is timed the counters and `selected`
of (b) over the first --check-elements elements (default 2^28) of every column are compared with the uint16 entry's
(filter_rf.count_torch_filter_rf) over .to(int16) of the same slice, and `high` with 0.  --quick: one call of each after one
warm-up."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from libflagstats_amd import _lib, device, filter_rf, kernel_id  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bytes", type=int, default=8 << 30)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--buffers", type=int, default=2)
ap.add_argument("--check-elements", type=int, default=1 << 28)
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()

import torch  # noqa: E402

lib = _lib.lib()
_lib.check(lib.FLAGSTATS_hip_init(0), "init")
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
nbytes = args.bytes // 32768 * 32768
print("wide_filter_rf_sweep: %d bytes (%.2f GiB) per column, %d columns per width, NA12878-like low halves; rounds %d x reps %d; "
      "K1 code object %s" % (nbytes, nbytes / 2 ** 30, args.buffers, args.rounds, args.reps, kernel_id.kernel_id()), flush=True)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


EXCLUDE = 0x904
# name, text, include_any, exclude_all, what fsk_filter_rf_reduce answers
ARMS = (("b1", "--rf 0x50", 0x0050, 0, 2), ("b2", "-G 0x420", 0, 0x0420, 2), ("b3", "--rf 0x210 -G 0x480", 0x0210, 0x0480, 2),
        ("b4", "--rf 0x40 (reduced)", 0x0040, 0, 1))
base_out = torch.zeros(34, dtype=torch.int64, device="cuda")
out = torch.zeros(34, dtype=torch.int64, device="cuda")
u16_out = torch.zeros(32, dtype=torch.int64, device="cuda")
u16_sel = torch.zeros(1, dtype=torch.int64, device="cuda")
reduced = (ctypes.c_uint32 * 4)()

for W, dt in ((4, torch.int32), (8, torch.int64)):
    n = nbytes // W
    n_check = min(n, args.check_elements)
    flags16 = torch.empty(n, dtype=torch.int16, device="cuda")
    cols = []
    step = 1 << 26
    for b in range(args.buffers):
        device.generate_torch(flags16, device.GEN_NA12878, seed=11 + b, mask=0)
        t = torch.empty(n, dtype=dt, device="cuda")
        for i in range(0, n, step):
            t[i:i + step] = flags16[i:i + step].to(dt) & 0xFFFF
        cols.append(t)
    del flags16
    mapq = torch.empty(n, dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    for i in range(0, n, step):
        c = min(step, n - i)
        low = torch.randint(0, 60, (c,), device="cuda", generator=gen, dtype=torch.uint8)
        keep = torch.rand(c, device="cuda", generator=gen) < 0.25
        mapq[i:i + c] = torch.where(keep, low, torch.full_like(low, 60))
    del low, keep
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

    for name, text, include_any, exclude_all, kind in ARMS:
        assert lib.fsk_filter_rf_reduce(0, EXCLUDE, include_any, exclude_all, reduced) == kind, (name, tuple(reduced))
        for min_mapq in (0, 30):
            label = "-F 0x904 %s%s" % (text, " -q 30" if min_mapq else "")
            per_elem = W + (1 if min_mapq else 0)
            q = mapq.data_ptr() if min_mapq else None

            def base(i, flags=0, count=n):
                t = cols[i % len(cols)]
                _lib.check(lib.FLAGSTATS_hip_device_wide_filter(t.data_ptr(), count, W, 0, EXCLUDE, q, min_mapq, base_out.data_ptr(),
                                                                base_out.data_ptr() + 256, base_out.data_ptr() + 264, flags, stream),
                           "FLAGSTATS_hip_device_wide_filter")

            def mine(i, flags=0, count=n):
                t = cols[i % len(cols)]
                _lib.check(lib.FLAGSTATS_hip_device_wide_filter_rf(t.data_ptr(), count, W, 0, EXCLUDE, include_any, exclude_all, q, min_mapq,
                                                                   out.data_ptr(), out.data_ptr() + 256, out.data_ptr() + 264, flags, stream),
                           "FLAGSTATS_hip_device_wide_filter_rf")

            # parity of what is measured, over a slice of every column: one pass == narrow + the uint16 entry, high == 0
            for b in range(len(cols)):
                mine(b, 1, n_check)
                filter_rf.count_torch_filter_rf(cols[b][:n_check].to(torch.int16), exclude=EXCLUDE, include_any=include_any,
                                                exclude_all=exclude_all, mapq=mapq[:n_check] if min_mapq else None, min_mapq=min_mapq,
                                                out=u16_out, selected=u16_sel, store=True)
                torch.cuda.synchronize()
                assert torch.equal(out[:32], u16_out) and int(out[32]) == int(u16_sel[0]) and int(out[33]) == 0, \
                    "wide filter_rf differs from .to(int16) + count_torch_filter_rf"
            mine(0, 1)
            torch.cuda.synchronize()
            print("W = %d (%s) %s: %d of %d elements pass in the first column; counters and selected over the first %d elements of every "
                  "column equal .to(int16) + count_torch_filter_rf's, high == 0" % (W, name, label, int(out[32]), n, n_check), flush=True)
            base(0)
            mine(1)
            torch.cuda.synchronize()
            if args.quick:
                continue
            bs, ws = [], []
            for _ in range(args.rounds):
                bs.append(timed(base, args.reps))
                ws.append(timed(mine, args.reps))
            bm, wm = statistics.median(bs), statistics.median(ws)
            rate = lambda ms: per_elem * n / ms / 1e9      # noqa: E731   TB/s
            ratio = wm / bm
            print("W = %d (%s) %-39s: (a) wide filter -F 0x904%s %.4f ms = %.3f TB/s [%.4f .. %.4f ms]   (b) wide filter_rf %.4f ms = "
                  "%.3f TB/s at %d B/element [%.4f .. %.4f ms]   (b)/(a) time %.4f, yardstick 1.030: %s   (b) %.1f Gelements/s"
                  % (W, name, label, " -q 30" if min_mapq else "", bm, rate(bm), min(bs), max(bs), wm, rate(wm), per_elem, min(ws), max(ws),
                     ratio, "MET" if ratio <= 1.03 else "MISSED", n / wm / 1e6), flush=True)
    del cols, mapq
    torch.cuda.empty_cache()
