#!/usr/bin/env python3
"""Segmented flagstat on int32 / int64 columns at full size: `python3 tests/perf/segments_wide_sweep.py [--bytes N] [--rounds R]
[--reps K] [--buffers B] [--quick]` -- per width, B (default 2) device-resident columns of N bytes (default 8 GiB: every pass reads
32 times the 256 MiB cache) of int32 / int64 elements whose low halves are NA12878-like flags (filled on the device), timed with
hipEvents after warm-up; the calls of a timed window rotate over the B columns.  In one run, ALTERNATING per layout:

  (a) fsk_launch_wide alone over the column (the wide kernel of this build, no segments)
  (b) fsk_launch_segments_wide in the store form (its zeroing included), at the default policy
  (c) the route a caller had without this kernel: t.to(torch.int16) followed by segments.count_segments_torch

Layouts: one segment; blocks of 512,000 elements; segments of ~1,000 elements (uniform in 500..1500); segments of 5,000 elements
(2.4 units at W = 4, 4.9 at W = 8: the lengths at which min_units decides the regime).  Then, for the blocks and the 5,000-element
layout, (b) under min_units in {1, 2, 3, 4, 8}, alternating, the policy restored afterwards.

Printed per width and layout: median ms per call over the rounds with the spread (min .. max), (b) / (a) in time -- the number the
uint16 segmented kernel's 1.02 against its single-range entry is compared with -- and (c) / (b).  Before anything is timed the
rows of (b) are compared with (c)'s, their sum with (a)'s counters, and the masks with 0.  --quick: one call of each after one
warm-up."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from libflagstats_amd import _lib, device, kernel_id, segments  # noqa: E402

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
lib.fsk_segments_policy.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
lib.fsk_segments_policy.restype = None
lib.fsk_set_segments_policy.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
lib.fsk_set_segments_policy.restype = None
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
bpc = lib.FLAGSTATS_hip_get(b"blocks_per_cu")
cus = lib.FLAGSTATS_hip_compute_units()
wide_grid = cus * (bpc if bpc else 1)                   # the wide entries' grid
mu0, seg_bpc = ctypes.c_uint32(), ctypes.c_uint32()
lib.fsk_segments_policy(ctypes.byref(mu0), ctypes.byref(seg_bpc))
seg_grid = cus * seg_bpc.value                          # the segmented entries' grid
nbytes = args.bytes // 32768 * 32768
print("segments_wide_sweep: %d bytes (%.2f GiB) per column, %d columns per width, NA12878-like low halves; rounds %d x reps %d; wide grid "
      "%d, segments grid %d, min_units %d; K1 code object %s"
      % (nbytes, nbytes / 2 ** 30, args.buffers, args.rounds, args.reps, wide_grid, seg_grid, mu0.value, kernel_id.kernel_id()), flush=True)


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


def med(xs):
    return "%.4f ms [%.4f .. %.4f]" % (statistics.median(xs), min(xs), max(xs))


def layouts(n):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    short = torch.randint(500, 1501, (n // 1000 + 1,), device="cuda", generator=gen, dtype=torch.int64).cumsum(0)
    short = short[short < n]

    def csr(cuts):
        return torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), cuts, torch.full((1,), n, dtype=torch.int64, device="cuda")])

    return (("one segment", csr(torch.zeros(0, dtype=torch.int64, device="cuda"))),
            ("512,000-element blocks", csr(torch.arange(512_000, n, 512_000, dtype=torch.int64, device="cuda"))),
            ("~1,000-element segments", csr(short)),
            ("5,000-element segments", csr(torch.arange(5_000, n, 5_000, dtype=torch.int64, device="cuda"))))


wide_out = torch.zeros(33, dtype=torch.int64, device="cuda")

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
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

    def wide(i, mode=0):
        t = cols[i % len(cols)]
        check_hip(lib.fsk_launch_wide(t.data_ptr(), n, W, wide_out.data_ptr(), wide_out.data_ptr() + 256, mode, wide_grid, stream), "fsk_launch_wide")

    for name, off in layouts(n):
        nseg = off.numel() - 1
        words = torch.zeros(nseg * 33, dtype=torch.int64, device="cuda")
        rows, high = words[:nseg * 32].view(nseg, 32), words[nseg * 32:]
        today_rows = torch.zeros((nseg, 32), dtype=torch.int64, device="cuda")

        def mine(i):
            t = cols[i % len(cols)]
            check_hip(lib.fsk_launch_segments_wide(t.data_ptr(), W, 0, n, off.data_ptr(), nseg, rows.data_ptr(), high.data_ptr(), 1, seg_grid,
                                                   stream), "fsk_launch_segments_wide")

        def today(i):
            t = cols[i % len(cols)]
            segments.count_segments_torch(t.to(torch.int16), off, out=today_rows, store=True)

        # parity of what is measured, on every column
        for b in range(len(cols)):
            mine(b)
            today(b)
            wide(b, 1)
            torch.cuda.synchronize()
            assert torch.equal(rows, today_rows), "rows differ from .to(int16) + count_segments_torch"
            assert torch.equal(rows.sum(dim=0), wide_out[:32]) and not bool(high.any()) and int(wide_out[32]) == 0, "rows do not sum to the wide counters"
        print("W = %d, %s: %d segments; rows equal .to(int16) + count_segments_torch's and sum to fsk_launch_wide's on every column, masks 0"
              % (W, name, nseg), flush=True)
        if args.quick:
            continue
        ks, ws, cs = [], [], []
        for _ in range(args.rounds):
            ks.append(timed(wide, args.reps))
            ws.append(timed(mine, args.reps))
            cs.append(timed(today, max(2, args.reps // 5)))
        km, wm, cm = (statistics.median(x) for x in (ks, ws, cs))
        print("W = %d, %-26s: (a) wide %s = %.3f TB/s   (b) segments wide %s = %.3f TB/s   (b)/(a) time %.4f   (c) .to(int16) + "
              "count_segments_torch %s   (c)/(b) %.2f x" % (W, name, med(ks), W * n / km / 1e9, med(ws), W * n / wm / 1e9, wm / km, med(cs), cm / wm),
              flush=True)
        if name.startswith("512,000") or name.startswith("5,000"):
            per = {mu: [] for mu in (1, 2, 3, 4, 8)}
            try:
                for _ in range(args.rounds):
                    for mu in per:
                        lib.fsk_set_segments_policy(mu, seg_bpc.value)
                        mine(0)
                        per[mu].append(timed(mine, args.reps))
            finally:
                lib.fsk_set_segments_policy(mu0.value, seg_bpc.value)
            print("W = %d, %-26s: min_units " % (W, name) + "   ".join("%d: %s" % (mu, med(v)) for mu, v in per.items()), flush=True)
        del words, rows, high, today_rows
    del cols
    torch.cuda.empty_cache()
