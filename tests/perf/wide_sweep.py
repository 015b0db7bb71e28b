#!/usr/bin/env python3
"""Wide-input flagstat at full size: `python3 tests/perf/wide_sweep.py [--bytes N] [--rounds R] [--reps K] [--host-bytes N]
[--quick]` -- N bytes (default 8 GiB) of device-resident int32 / int64 elements whose low halves are NA12878-like flags (filled
on the device), timed with hipEvents after warm-up.  In one run, ALTERNATING:

  (a) FLAGSTATS_hip_device_u16 over the same N bytes read as uint16 -- K1 on this build: the yardstick is its bytes per second
  (b) FLAGSTATS_hip_device_wide at W = 4 (N / 4 elements) and W = 8 (N / 8 elements), += and store
  (c) what a torch caller does without it, in a second device buffer: t.to(torch.int16) followed by device.count_torch

Printed per width and form: median ms per call over the rounds, the byte rate of (a), (b) and their ratio with (a)'s own spread
(min / max over its rounds), the flag rate of (b) and (c) and their ratio.  --host-bytes N (default 2 GiB; 0: off): the HOST form
FLAGSTATS_hip_wide_x64 over N bytes of int32 in page-locked memory, host clock around each call, alternating with FLAGSTATS_u16_x64
over the same byte count (the same bytes cross the bus).  --quick: one call of each after one warm-up (for rocprofv3
--kernel-trace --stats runs)."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from libflagstats_amd import _lib, device, kernel_id  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bytes", type=int, default=8 << 30)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--host-bytes", type=int, default=2 << 30)
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()

import torch  # noqa: E402

lib = _lib.lib()
_lib.check(lib.FLAGSTATS_hip_init(0), "init")
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
nbytes = args.bytes // 32768 * 32768
print("wide_sweep: %d bytes (%.2f GiB), NA12878-like low halves; rounds %d x reps %d; K1 code object %s"
      % (nbytes, nbytes / 2 ** 30, args.rounds, args.reps, kernel_id.kernel_id()), flush=True)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


k1_out = torch.zeros(32, dtype=torch.int64, device="cuda")
out = torch.zeros(33, dtype=torch.int64, device="cuda")
for W, dt in ((4, torch.int32), (8, torch.int64)):
    n = nbytes // W
    # the flags are made as uint16 in a tensor of their own (freed before the timing), then widened into t slice by slice
    t = torch.empty(n, dtype=dt, device="cuda")
    flags16 = torch.empty(n, dtype=torch.int16, device="cuda")
    device.generate_torch(flags16, device.GEN_NA12878, seed=11, mask=0)
    step = 1 << 26
    for i in range(0, n, step):
        t[i:i + step] = flags16[i:i + step].to(dt) & 0xFFFF
    torch.cuda.synchronize()
    as16 = t.view(torch.int16)     # the same bytes read as uint16: (a)'s input

    def k1():
        _lib.check(lib.FLAGSTATS_hip_device_u16(as16.data_ptr(), as16.numel(), k1_out.data_ptr(), stream), "FLAGSTATS_hip_device_u16")

    def today():
        device.count_torch(t.to(torch.int16), k1_out)

    # parity of what is measured: wide counters == K1's over the narrowed copy, mask 0
    want = device.count_torch(flags16, store=True).clone()
    _lib.check(lib.FLAGSTATS_hip_device_wide(t.data_ptr(), n, W, out.data_ptr(), out.data_ptr() + 256, 1, stream), "wide")
    torch.cuda.synchronize()
    assert torch.equal(out[:32], want) and int(out[32]) == 0, "wide counters differ from K1's over the same flags"
    print("W = %d: %d elements; counters equal K1's over the same flags, high == 0" % (W, n), flush=True)
    del flags16
    torch.cuda.empty_cache()

    for flags, form in ((0, "+="), (1, "store")):
        def wide():
            _lib.check(lib.FLAGSTATS_hip_device_wide(t.data_ptr(), n, W, out.data_ptr(), out.data_ptr() + 256, flags, stream),
                       "FLAGSTATS_hip_device_wide")
        wide()
        k1()
        today()
        torch.cuda.synchronize()
        if args.quick:
            continue
        ks, ws, cs = [], [], []
        for _ in range(args.rounds):
            ks.append(timed(k1, args.reps))
            ws.append(timed(wide, args.reps))
            cs.append(timed(today, max(1, args.reps // 5)))
        km, wm, cm = statistics.median(ks), statistics.median(ws), statistics.median(cs)
        rate = lambda ms: nbytes / ms / 1e9  # noqa: E731   TB/s
        print("W = %d %-5s: (a) K1 %.4f ms = %.3f TB/s [spread %.3f .. %.3f TB/s]   (b) wide %.4f ms = %.3f TB/s [%.3f .. %.3f]   "
              "(b)/(a) byte rate %.4f   (b) %.1f Gflags/s   (c) .to(int16) + count_torch %.4f ms = %.1f Gflags/s   (b)/(c) %.3f x"
              % (W, form, km, rate(km), rate(max(ks)), rate(min(ks)), wm, rate(wm), rate(max(ws)), rate(min(ws)), km / wm,
                 n / wm / 1e6, cm, n / cm / 1e6, cm / wm), flush=True)
    del t, as16
    torch.cuda.empty_cache()

# ---- the host form: the array crosses the bus as it is
if args.host_bytes and not args.quick:
    hb = args.host_bytes // 32768 * 32768
    n4, n2 = hb // 4, hb // 2
    hp = lib.FLAGSTATS_hip_host_alloc(hb)
    assert hp, "host_alloc"
    src = torch.empty(min(n4, 1 << 26), dtype=torch.int16, device="cuda")
    device.generate_torch(src, device.GEN_NA12878, seed=13, mask=0)
    piece = (src.to(torch.int32) & 0xFFFF).cpu().numpy()
    host = np.ctypeslib.as_array(ctypes.cast(hp, ctypes.POINTER(ctypes.c_int32)), shape=(n4,))
    for i in range(0, n4, piece.size):
        host[i:i + piece.size] = piece[:min(piece.size, n4 - i)]
    o, h = np.zeros(32, dtype=np.uint64), ctypes.c_uint64(0)

    def host_wide():
        _lib.check(lib.FLAGSTATS_hip_wide_x64(hp, n4, 4, o.ctypes.data, ctypes.byref(h), 1), "FLAGSTATS_hip_wide_x64")

    def host_u16():
        _lib.check(lib.FLAGSTATS_u16_x64(hp, n2, o.ctypes.data), "FLAGSTATS_u16_x64")

    host_wide()
    host_u16()
    us, ws = [], []
    for _ in range(args.rounds):
        for fn, acc in ((host_u16, us), (host_wide, ws)):
            t0 = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t0) * 1e3)
    um, wm = statistics.median(us), statistics.median(ws)
    print("host form, %d bytes (%.2f GiB) page-locked: FLAGSTATS_hip_wide_x64 (int32) %.2f ms = %.1f GB/s [min %.2f max %.2f ms]   "
          "FLAGSTATS_u16_x64 over the same bytes %.2f ms = %.1f GB/s   time ratio %.3f"
          % (hb, hb / 2 ** 30, wm, hb / wm / 1e6, min(ws), max(ws), um, hb / um / 1e6, wm / um), flush=True)
    lib.FLAGSTATS_hip_host_free(hp)
