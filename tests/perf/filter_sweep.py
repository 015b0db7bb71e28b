#!/usr/bin/env python3
"""Filtered flagstat at full size: `python3 tests/perf/filter_sweep.py [--bytes N] [--rounds R] [--reps K] [--today-flags N]
[--quick]` -- N bytes (default 8 GiB: every pass reads 32 times the 256 MiB cache) of device-resident NA12878-like uint16 flags
(filled on the device) and a uint8 MAPQ column beside them (three quarters 60, the rest uniform in 0..59), timed with hipEvents
after warm-up.  In one run, ALTERNATING:

  (a)  FLAGSTATS_hip_device_u16 over the same array -- K1 on this build, which reads 2 B per flag
  (b1) FLAGSTATS_hip_device_u16_filter with -F 0x904                   2 B per flag
  (b2) ... with -f 0x2 -F 0x904                                        2 B per flag
  (b3) ... with -F 0x904 -q 30                                         3 B per flag
  (c)  what a torch caller does today, over the first --today-flags flags (default 2^30): the torch expression for the mask
       followed by where.count_torch_where, beside (b) over the same slice

Printed: median ms per call over the rounds, the byte rates of (a) and (b) with their spread (min / max over the rounds), their
ratio, the flag rates, and (c) / (b).  Before anything is timed the counters and `selected` of (b) over the slice are compared
with (c)'s.  --quick: one call of each after one warm-up (for rocprofv3 --kernel-trace --stats runs)."""
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
ap.add_argument("--today-flags", type=int, default=1 << 30)
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()

import torch  # noqa: E402

lib = _lib.lib()
_lib.check(lib.FLAGSTATS_hip_init(0), "init")
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
n = args.bytes // 32768 * 16384
n_today = min(n, args.today_flags) // 16384 * 16384
print("filter_sweep: %d flags (%.2f GiB) + %d MAPQ bytes, NA12878-like; rounds %d x reps %d; (c) over %d flags; K1 code object %s"
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
k1_out = torch.zeros(32, dtype=torch.int64, device="cuda")
out = torch.zeros(33, dtype=torch.int64, device="cuda")
today_out = torch.zeros(32, dtype=torch.int64, device="cuda")
today_sel = torch.zeros(1, dtype=torch.int64, device="cuda")
ts, qs = t[:n_today], mapq[:n_today]

CASES = (("b1", "-F 0x904", 0, 0x904, 0, 2.0), ("b2", "-f 0x2 -F 0x904", 0x2, 0x904, 0, 2.0), ("b3", "-F 0x904 -q 30", 0, 0x904, 30, 3.0))


def k1():
    _lib.check(lib.FLAGSTATS_hip_device_u16(t.data_ptr(), n, k1_out.data_ptr(), stream), "FLAGSTATS_hip_device_u16")


def run_filter(count, require, exclude, min_mapq, flags):
    _lib.check(lib.FLAGSTATS_hip_device_u16_filter(t.data_ptr(), count, require, exclude, mapq.data_ptr() if min_mapq else None, min_mapq,
                                                   out.data_ptr(), out.data_ptr() + 256, flags, stream), "FLAGSTATS_hip_device_u16_filter")


def today_mask(require, exclude, min_mapq):
    m = (ts & exclude) == 0
    if require:
        m = m & ((ts & require) == require)
    if min_mapq:
        m = m & (qs >= min_mapq)
    return m


def run_today(require, exclude, min_mapq, store=False):
    where.count_torch_where(ts, today_mask(require, exclude, min_mapq), out=today_out, selected=today_sel, store=store)


for name, text, require, exclude, min_mapq, per_flag in CASES:
    # parity of what is measured, over the slice (c) takes: filter == where under torch's mask
    run_filter(n_today, require, exclude, min_mapq, 1)
    run_today(require, exclude, min_mapq, store=True)
    torch.cuda.synchronize()
    assert torch.equal(out[:32], today_out) and int(out[32]) == int(today_sel[0]), "filter counters differ from where's under torch's mask"
    nsel_today = int(out[32])
    run_filter(n, require, exclude, min_mapq, 1)
    torch.cuda.synchronize()
    nsel = int(out[32])
    print("(%s) %s: %d of %d flags pass; counters and selected over the first %d flags (%d pass) equal count_torch_where's under "
          "torch's mask" % (name, text, nsel, n, n_today, nsel_today), flush=True)

    def full():
        run_filter(n, require, exclude, min_mapq, 0)

    def part():
        run_filter(n_today, require, exclude, min_mapq, 0)

    def today():
        run_today(require, exclude, min_mapq)

    full()
    k1()
    part()
    today()
    torch.cuda.synchronize()
    if args.quick:
        continue
    ks, ws, ss, cs = [], [], [], []
    for _ in range(args.rounds):
        ks.append(timed(k1, args.reps))
        ws.append(timed(full, args.reps))
        ss.append(timed(part, args.reps))
        cs.append(timed(today, max(1, args.reps // 5)))
    km, wm, sm, cm = (statistics.median(x) for x in (ks, ws, ss, cs))
    k_rate = lambda ms: 2 * n / ms / 1e9             # noqa: E731   TB/s
    w_rate = lambda ms: per_flag * n / ms / 1e9      # noqa: E731
    print("(%s) %-16s: (a) K1 %.4f ms = %.3f TB/s [spread %.3f .. %.3f]   (b) filter %.4f ms = %.3f TB/s at %.3f B/flag "
          "[%.3f .. %.3f]   (b)/(a) byte rate %.4f, time %.4f   (b) %.1f Gflags/s   over %d flags: (b) %.4f ms, (c) torch mask + "
          "count_torch_where %.4f ms   (c)/(b) %.2f x"
          % (name, text, km, k_rate(km), k_rate(max(ks)), k_rate(min(ks)), wm, w_rate(wm), per_flag, w_rate(max(ws)),
             w_rate(min(ws)), w_rate(wm) / k_rate(km), wm / km, n / wm / 1e6, n_today, sm, cm, cm / sm), flush=True)
    if sm >= cm:
        print("(%s) FINDING: (b) is not faster than (c) over the same %d flags" % (name, n_today), flush=True)
