#!/usr/bin/env python3
"""Filtered flagstat under samtools' whole FLAG predicate at full size: `python3 tests/perf/filter_rf_sweep.py [--bytes N]
[--rounds R] [--reps K] [--today-flags N] [--quick]` -- N bytes (default 8 GiB = 2^32 flags: every pass reads 32 times the 256 MiB
cache) of device-resident NA12878-like uint16 flags (filled on the device) and a uint8 MAPQ column beside them (three quarters 60,
the rest uniform in 0..59), timed with hipEvents after warm-up.  Every arm is -F 0x904 plus what it names, without and with
-q 30, and runs ALTERNATING with its yardstick in the same process:

  (a)  FLAGSTATS_hip_device_u16_filter with -F 0x904 [-q 30]: fsk::flagstat_count_filter, which moves the same bytes
  (b1) FLAGSTATS_hip_device_u16_filter_rf with --rf 0x50          the any-of test alone       flagstat_count_filter_rf<., 1, 0>
  (b2) ... with -G 0x420                                          the all-of test alone       <., 0, 1>
  (b3) ... with --rf 0x210 -G 0x480                               both, across byte planes    <., 1, 1>
  (b4) ... with --rf 0x40                                         reduced to -f 0x40 -F 0x904: flagstat_count_filter itself
  (c)  what a torch caller does today, over the first --today-flags flags (default 2^28): the torch expression for the mask
       followed by where.count_torch_where, beside (b) over the same slice

The yardstick of (b) is (a)'s time in the same rounds plus 3 %: the bytes moved are the same.  Printed: median ms per call over
the rounds with the spread, (b)/(a), MET or MISSED, the flag rate, and (c)/(b).  Before anything is timed the counters and
`selected` of (b) over the slice are compared with (c)'s.  --quick: one call of each after one warm-up."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from libflagstats_amd import _lib, device, kernel_id, where  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bytes", type=int, default=8 << 30)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--today-flags", type=int, default=1 << 28)
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()

import torch  # noqa: E402

lib = _lib.lib()
_lib.check(lib.FLAGSTATS_hip_init(0), "init")
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
n = args.bytes // 32768 * 16384
n_today = min(n, args.today_flags) // 16384 * 16384
print("filter_rf_sweep: %d flags (%.2f GiB) + %d MAPQ bytes, NA12878-like; rounds %d x reps %d; (c) over %d flags; K1 code object %s"
      % (n, 2 * n / 2 ** 30, n, args.rounds, args.reps, n_today, kernel_id.kernel_id()), flush=True)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


t = torch.empty(n, dtype=torch.int16, device="cuda")
device.generate_torch(t, device.GEN_NA12878, seed=11, mask=0)
mapq = torch.empty(n, dtype=torch.uint8, device="cuda")
gen = torch.Generator(device="cuda")
gen.manual_seed(5)
step = 1 << 26
for i in range(0, n, step):
    c = min(step, n - i)
    low = torch.randint(0, 60, (c,), device="cuda", generator=gen, dtype=torch.uint8)
    keep = torch.rand(c, device="cuda", generator=gen) < 0.25
    mapq[i:i + c] = torch.where(keep, low, torch.full_like(low, 60))
del low, keep
torch.cuda.synchronize()
base_out = torch.zeros(33, dtype=torch.int64, device="cuda")
out = torch.zeros(33, dtype=torch.int64, device="cuda")
today_out = torch.zeros(32, dtype=torch.int64, device="cuda")
today_sel = torch.zeros(1, dtype=torch.int64, device="cuda")
ts, qs = t[:n_today], mapq[:n_today]
EXCLUDE = 0x904

# name, text, include_any, exclude_all, what fsk_filter_rf_reduce answers
ARMS = (("b1", "--rf 0x50", 0x0050, 0, 2), ("b2", "-G 0x420", 0, 0x0420, 2), ("b3", "--rf 0x210 -G 0x480", 0x0210, 0x0480, 2),
        ("b4", "--rf 0x40 (reduced)", 0x0040, 0, 1))


def run_base(count, min_mapq, flags):
    _lib.check(lib.FLAGSTATS_hip_device_u16_filter(t.data_ptr(), count, 0, EXCLUDE, mapq.data_ptr() if min_mapq else None, min_mapq,
                                                   base_out.data_ptr(), base_out.data_ptr() + 256, flags, stream), "FLAGSTATS_hip_device_u16_filter")


def run_rf(count, include_any, exclude_all, min_mapq, flags):
    _lib.check(lib.FLAGSTATS_hip_device_u16_filter_rf(t.data_ptr(), count, 0, EXCLUDE, include_any, exclude_all,
                                                      mapq.data_ptr() if min_mapq else None, min_mapq, out.data_ptr(), out.data_ptr() + 256,
                                                      flags, stream), "FLAGSTATS_hip_device_u16_filter_rf")


def today_mask(include_any, exclude_all, min_mapq):
    m = (ts & EXCLUDE) == 0
    if include_any:
        m = m & ((ts & include_any) != 0)
    if exclude_all:
        m = m & ((ts & exclude_all) != exclude_all)
    if min_mapq:
        m = m & (qs >= min_mapq)
    return m


def run_today(include_any, exclude_all, min_mapq, store=False):
    where.count_torch_where(ts, today_mask(include_any, exclude_all, min_mapq), out=today_out, selected=today_sel, store=store)


reduced = (ctypes.c_uint32 * 4)()
for name, text, include_any, exclude_all, kind in ARMS:
    assert lib.fsk_filter_rf_reduce(0, EXCLUDE, include_any, exclude_all, reduced) == kind, (name, tuple(reduced))
    for min_mapq in (0, 30):
        label = "-F 0x904 %s%s" % (text, " -q 30" if min_mapq else "")
        per_flag = 3.0 if min_mapq else 2.0
        # parity of what is measured, over the slice (c) takes: filter_rf == where under torch's mask
        run_rf(n_today, include_any, exclude_all, min_mapq, 1)
        run_today(include_any, exclude_all, min_mapq, store=True)
        torch.cuda.synchronize()
        assert torch.equal(out[:32], today_out) and int(out[32]) == int(today_sel[0]), "filter_rf counters differ from where's under torch's mask"
        nsel_today = int(out[32])
        run_rf(n, include_any, exclude_all, min_mapq, 1)
        torch.cuda.synchronize()
        print("(%s) %s: %d of %d flags pass; counters and selected over the first %d flags (%d pass) equal count_torch_where's under "
              "torch's mask" % (name, label, int(out[32]), n, n_today, nsel_today), flush=True)

        def base():
            run_base(n, min_mapq, 0)

        def full():
            run_rf(n, include_any, exclude_all, min_mapq, 0)

        def part():
            run_rf(n_today, include_any, exclude_all, min_mapq, 0)

        def today():
            run_today(include_any, exclude_all, min_mapq)

        full()
        base()
        part()
        today()
        torch.cuda.synchronize()
        if args.quick:
            continue
        bs, ws, ss, cs = [], [], [], []
        for _ in range(args.rounds):
            bs.append(timed(base, args.reps))
            ws.append(timed(full, args.reps))
            ss.append(timed(part, args.reps))
            cs.append(timed(today, max(1, args.reps // 5)))
        bm, wm, sm, cm = (statistics.median(x) for x in (bs, ws, ss, cs))
        rate = lambda ms: per_flag * n / ms / 1e9      # noqa: E731   TB/s
        ratio = wm / bm
        print("(%s) %-34s: (a) filter -F 0x904%s %.4f ms = %.3f TB/s [%.4f .. %.4f ms]   (b) filter_rf %.4f ms = %.3f TB/s at %.0f B/flag "
              "[%.4f .. %.4f ms]   (b)/(a) time %.4f, yardstick 1.030: %s   (b) %.1f Gflags/s   over %d flags: (b) %.4f ms, (c) torch mask "
              "+ count_torch_where %.4f ms   (c)/(b) %.2f x"
              % (name, label, " -q 30" if min_mapq else "", bm, rate(bm), min(bs), max(bs), wm, rate(wm), per_flag, min(ws), max(ws), ratio,
                 "MET" if ratio <= 1.03 else "MISSED", n / wm / 1e6, n_today, sm, cm, cm / sm), flush=True)
