#!/usr/bin/env python3
"""Selected-elements flagstat at full size: `python3 tests/perf/where_sweep.py [--bytes N] [--rounds R] [--reps K]
[--today-flags N] [--quick]` -- N bytes (default 8 GiB: every pass reads 32 times the 256 MiB cache) of device-resident
NA12878-like uint16 flags (filled on the device) under masks of density 0, 0.01, 0.5 and 1, as an LSB-first bitmap and as one
byte per flag, timed with hipEvents after warm-up.  Per density and encoding, in one run, ALTERNATING:

  (a) FLAGSTATS_hip_device_u16 over the same array -- K1 on this build, which reads 2 B per flag
  (b) FLAGSTATS_hip_device_u16_where over array and selection: 2.125 B per flag (bitmap) or 3 B per flag (bytes)
  (c) what a torch caller does today, over the first --today-flags flags (default 2^30; torch's mask indexing stops below 2^31
      elements): t[m] followed by device.count_torch, beside (b) over the same slice

Printed: median ms per call over the rounds, the byte rates of (a) and (b) with their spread (min / max over the rounds), their
ratio, the flag rates, and (c) / (b).  Before anything is timed the counters of (b) are compared with K1's over t[m], `selected`
with m.sum().  --quick: one call of each after one warm-up (for rocprofv3 --kernel-trace --stats runs)."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from libflagstats_amd import _lib, device, kernel_id  # noqa: E402

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
print("where_sweep: %d flags (%.2f GiB), NA12878-like; rounds %d x reps %d; (c) over %d flags; K1 code object %s"
      % (n, 2 * n / 2 ** 30, args.rounds, args.reps, n_today, kernel_id.kernel_id()), flush=True)


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
mask = torch.empty(n, dtype=torch.bool, device="cuda")
bitmap = torch.empty(n // 8, dtype=torch.uint8, device="cuda")
weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device="cuda")
k1_out = torch.zeros(32, dtype=torch.int64, device="cuda")
out = torch.zeros(33, dtype=torch.int64, device="cuda")
gen = torch.Generator(device="cuda")
gen.manual_seed(5)


def k1():
    _lib.check(lib.FLAGSTATS_hip_device_u16(t.data_ptr(), n, k1_out.data_ptr(), stream), "FLAGSTATS_hip_device_u16")


for density in (0.0, 0.01, 0.5, 1.0):
    step = 1 << 26
    for i in range(0, n, step):
        m = torch.rand(min(step, n - i), device="cuda", generator=gen) < density
        mask[i:i + step] = m
        bitmap[i // 8:(i + step) // 8] = (m.view(-1, 8).to(torch.uint8) * weights).sum(dim=1, dtype=torch.uint8)
    del m
    torch.cuda.synchronize()
    nsel = int(mask.sum())
    nsel_today = int(mask[:n_today].sum())
    # parity of what is measured, over the slice (c) can take: where == K1 over t[m]
    want = device.count_torch(t[:n_today][mask[:n_today]], store=True).clone() if nsel_today else torch.zeros(32, dtype=torch.int64, device="cuda")
    for sel_bits, sel in ((1, bitmap), (8, mask)):
        _lib.check(lib.FLAGSTATS_hip_device_u16_where(t.data_ptr(), n_today, sel.data_ptr(), 0, sel_bits, out.data_ptr(), out.data_ptr() + 256,
                                                      1, stream), "where")
        torch.cuda.synchronize()
        assert torch.equal(out[:32], want) and int(out[32]) == nsel_today, "where counters differ from K1's over t[m]"
        _lib.check(lib.FLAGSTATS_hip_device_u16_where(t.data_ptr(), n, sel.data_ptr(), 0, sel_bits, out.data_ptr(), out.data_ptr() + 256,
                                                      1, stream), "where")
        torch.cuda.synchronize()
        assert int(out[32]) == nsel
    print("density %.2f: %d of %d flags selected; counters over the first %d flags equal K1's over t[m], both encodings"
          % (density, nsel, n, n_today), flush=True)

    for sel_bits, sel, name, per_flag in ((1, bitmap, "bitmap", 2.125), (8, mask, "bytes", 3.0)):
        def where_full():
            _lib.check(lib.FLAGSTATS_hip_device_u16_where(t.data_ptr(), n, sel.data_ptr(), 0, sel_bits, out.data_ptr(), out.data_ptr() + 256,
                                                          0, stream), "FLAGSTATS_hip_device_u16_where")

        def where_slice():
            _lib.check(lib.FLAGSTATS_hip_device_u16_where(t.data_ptr(), n_today, sel.data_ptr(), 0, sel_bits, out.data_ptr(),
                                                          out.data_ptr() + 256, 0, stream), "FLAGSTATS_hip_device_u16_where")

        def today():
            device.count_torch(t[:n_today][mask[:n_today]], k1_out)

        where_full()
        k1()
        where_slice()
        today()
        torch.cuda.synchronize()
        if args.quick:
            continue
        ks, ws, ss, cs = [], [], [], []
        for _ in range(args.rounds):
            ks.append(timed(k1, args.reps))
            ws.append(timed(where_full, args.reps))
            ss.append(timed(where_slice, args.reps))
            cs.append(timed(today, max(1, args.reps // 5)))
        km, wm, sm, cm = (statistics.median(x) for x in (ks, ws, ss, cs))
        k_rate = lambda ms: 2 * n / ms / 1e9             # noqa: E731   TB/s
        w_rate = lambda ms: per_flag * n / ms / 1e9      # noqa: E731
        print("density %.2f %-6s: (a) K1 %.4f ms = %.3f TB/s [spread %.3f .. %.3f]   (b) where %.4f ms = %.3f TB/s at %.3f B/flag "
              "[%.3f .. %.3f]   (b)/(a) byte rate %.4f, time %.4f   (b) %.1f Gflags/s   over %d flags: (b) %.4f ms, (c) t[m] + "
              "count_torch %.4f ms   (c)/(b) %.2f x"
              % (density, name, km, k_rate(km), k_rate(max(ks)), k_rate(min(ks)), wm, w_rate(wm), per_flag, w_rate(max(ws)),
                 w_rate(min(ws)), w_rate(wm) / k_rate(km), wm / km, n / wm / 1e6, n_today, sm, cm, cm / sm), flush=True)
