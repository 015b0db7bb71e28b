#!/usr/bin/env python3
"""Filtered wide-input flagstat at full size: `python3 tests/perf/wide_filter_sweep.py [--bytes N] [--rounds R] [--reps K]
[--buffers B] [--quick]` -- per width, B (default 2) device-resident columns of N bytes (default 8 GiB: every pass reads 32 times
the 256 MiB cache) of int32 / int64 elements whose low halves are NA12878-like flags (filled on the device) and one uint8 MAPQ
column beside them (three quarters 60, the rest uniform in 0..59), timed with hipEvents after warm-up.  The calls of a timed
window rotate over the B columns.  In one run, ALTERNATING:

  (a)  fsk_launch_wide alone over the column (the wide kernel of this build: W bytes per element)
  (b1) fsk_launch_wide_filter with -F 0x904                            W bytes per element
  (b2) ... with -f 0x2 -F 0x904                                        W bytes per element
  (b3) ... with -F 0x904 -q 30                                         W + 1 bytes per element
  (c)  the route a caller had without this kernel: t.to(torch.int16) followed by filter.count_torch_filter, on the same tensors

Printed per width and predicate: median ms per call over the rounds, the byte rates of (a) and (b) with their spread (min / max
over the rounds), their ratio, the element rate, and (c) / (b).  Before anything is timed the counters and `selected` of (b) are
compared with (c)'s and `high` with 0.  --quick: one call of each after one warm-up (for rocprofv3 --kernel-trace --stats runs)."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from libflagstats_amd import _lib, device, filter as flt, kernel_id  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bytes", type=int, default=8 << 30)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--buffers", type=int, default=2)
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()

import torch  # noqa: E402

lib = _lib.lib()
_lib.check(lib.FLAGSTATS_hip_init(0), "init")
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
bpc = lib.FLAGSTATS_hip_get(b"blocks_per_cu")
grid = lib.FLAGSTATS_hip_compute_units() * (bpc if bpc else 1)      # the public entries' grid
nbytes = args.bytes // 32768 * 32768
print("wide_filter_sweep: %d bytes (%.2f GiB) per column, %d columns per width, NA12878-like low halves; rounds %d x reps %d; "
      "launcher grid %d; K1 code object %s" % (nbytes, nbytes / 2 ** 30, args.buffers, args.rounds, args.reps, grid, kernel_id.kernel_id()),
      flush=True)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def check_hip(rc, what):
    assert rc == 0, "%s: hipError %d" % (what, rc)


CASES = (("b1", "-F 0x904", 0, 0x904, 0), ("b2", "-f 0x2 -F 0x904", 0x2, 0x904, 0), ("b3", "-F 0x904 -q 30", 0, 0x904, 30))
wide_out = torch.zeros(33, dtype=torch.int64, device="cuda")
out = torch.zeros(34, dtype=torch.int64, device="cuda")
today_out = torch.zeros(32, dtype=torch.int64, device="cuda")
today_sel = torch.zeros(1, dtype=torch.int64, device="cuda")

for W, dt in ((4, torch.int32), (8, torch.int64)):
    n = nbytes // W
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

    def wide(i, mode=0):
        t = cols[i % len(cols)]
        check_hip(lib.fsk_launch_wide(t.data_ptr(), n, W, wide_out.data_ptr(), wide_out.data_ptr() + 256, mode, grid, stream), "fsk_launch_wide")

    for name, text, require, exclude, min_mapq in CASES:
        per_elem = W + (1 if min_mapq else 0)

        def mine(i, mode=0):
            t = cols[i % len(cols)]
            check_hip(lib.fsk_launch_wide_filter(t.data_ptr(), n, W, require, exclude, mapq.data_ptr() if min_mapq else None, min_mapq,
                                                 out.data_ptr(), out.data_ptr() + 256, out.data_ptr() + 264, mode, grid, stream),
                      "fsk_launch_wide_filter")

        def today(i, store=False):
            t = cols[i % len(cols)]
            flt.count_torch_filter(t.to(torch.int16), require=require, exclude=exclude, mapq=mapq if min_mapq else None, min_mapq=min_mapq,
                                   out=today_out, selected=today_sel, store=store)

        # parity of what is measured, on every column: one pass == narrow + the uint16 filter, high == 0
        for b in range(len(cols)):
            mine(b, 1)
            today(b, store=True)
            torch.cuda.synchronize()
            assert torch.equal(out[:32], today_out) and int(out[32]) == int(today_sel[0]) and int(out[33]) == 0, \
                "wide filter differs from .to(int16) + count_torch_filter"
        print("W = %d (%s) %s: %d of %d elements pass in the last column; counters and selected equal .to(int16) + count_torch_filter's on "
              "every column, high == 0" % (W, name, text, int(out[32]), n), flush=True)
        wide(0)
        torch.cuda.synchronize()
        if args.quick:
            continue
        ks, ws, cs = [], [], []
        for _ in range(args.rounds):
            ks.append(timed(wide, args.reps))
            ws.append(timed(mine, args.reps))
            cs.append(timed(today, max(2, args.reps // 5)))
        km, wm, cm = (statistics.median(x) for x in (ks, ws, cs))
        k_rate = lambda ms: W * n / ms / 1e9             # noqa: E731   TB/s
        w_rate = lambda ms: per_elem * n / ms / 1e9      # noqa: E731
        print("W = %d (%s) %-16s: (a) wide %.4f ms = %.3f TB/s [spread %.3f .. %.3f]   (b) wide filter %.4f ms = %.3f TB/s at %d B/element "
              "[%.3f .. %.3f]   (b)/(a) byte rate %.4f, time %.4f   (b) %.1f Gelements/s   (c) .to(int16) + count_torch_filter %.4f ms   "
              "(c)/(b) %.2f x"
              % (W, name, text, km, k_rate(km), k_rate(max(ks)), k_rate(min(ks)), wm, w_rate(wm), per_elem, w_rate(max(ws)), w_rate(min(ws)),
                 w_rate(wm) / k_rate(km), wm / km, n / wm / 1e6, cm, cm / wm), flush=True)
        if wm >= cm:
            print("W = %d (%s) FINDING: the one-pass kernel (b) is not faster than (c) on the same tensors" % (W, name), flush=True)
    del cols, mapq
    torch.cuda.empty_cache()
