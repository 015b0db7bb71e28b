#!/usr/bin/env python3
"""Filtered and selected segmented flagstat on int32 / int64 columns at full size: `python3
tests/perf/segments_wide_filter_where_sweep.py [--bytes N] [--rounds R] [--reps K] [--buffers B] [--density D] [--quick]` -- per
width, B (default 2) device-resident columns of N bytes (default 8 GiB: every pass reads 32 times the 256 MiB cache) of int32 /
int64 elements whose low halves are NA12878-like flags (filled on the device), a uint8 MAPQ column uniform in 0..60 and a mask of
density D (default 0.9) held three ways: an LSB-first bitmap at bit offset 0 (plain), the same mask at bit offset 3 (funnelled) and
one byte per element; timed with hipEvents after warm-up; the calls of a timed window rotate over the B columns.  Layouts: one
segment; segments of 1,048,576 elements; segments of ~1,000 elements (uniform in 500..1500).  Predicates: -F 0x904 and
-F 0x904 -q 30.  Per width, predicate and layout everything is timed in the same run, ALTERNATING:

  this kernel  the launcher of flagstat_segments_wide_filter_where.h: bitmap plain, bitmap funnelled, bytes (store form)
  (a) fsk_launch_segments_wide_filter on the same layout under the same predicate (the parent without a selection, store form)

Printed: median ms per call over the rounds with the spread (min .. max), the ratio to (a) and the yardstick: (a) x the ratio of
bytes moved x 1.03 -- the bitmap adds 1/8 byte per element, the byte form 1 byte per element, to the parent's W (W + 1 with MAPQ).
A figure to report against, not a gate.  Before anything is timed the rows, counts and masks of the three forms are compared with
each other on every column, and with (a)'s under an all-ones byte mask.  --quick: parity only."""
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
ap.add_argument("--buffers", type=int, default=2)
ap.add_argument("--density", type=float, default=0.9)
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()

import torch  # noqa: E402

lib = _lib.lib()
_lib.check(lib.FLAGSTATS_hip_init(0), "init")
lib.fsk_segments_policy.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
lib.fsk_segments_policy.restype = None
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
cus = lib.FLAGSTATS_hip_compute_units()
mu0, seg_bpc = ctypes.c_uint32(), ctypes.c_uint32()
lib.fsk_segments_policy(ctypes.byref(mu0), ctypes.byref(seg_bpc))
seg_grid = cus * seg_bpc.value                          # the segmented entries' grid
nbytes = args.bytes // 32768 * 32768
FUNNEL_OFFSET = 3
EXCLUDE = 0x904
print("segments_wide_filter_where_sweep: %d bytes (%.2f GiB) per column, %d columns per width, NA12878-like low halves, MAPQ uniform 0..60, "
      "mask density %.2f; rounds %d x reps %d; segments grid %d, min_units %d; K1 code object %s"
      % (nbytes, nbytes / 2 ** 30, args.buffers, args.density, args.rounds, args.reps, seg_grid, mu0.value, kernel_id.kernel_id()), flush=True)


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
            ("1,048,576-element segments", csr(torch.arange(1 << 20, n, 1 << 20, dtype=torch.int64, device="cuda"))),
            ("~1,000-element segments", csr(short)))


def packed(bits, lead):
    """the bool tensor as an LSB-first bitmap whose bit lead + i is bits[i] (the unused bits of the first and last byte set)"""
    n = bits.numel()
    total = (lead + n + 7) // 8 * 8
    padded = torch.ones(total, dtype=torch.uint8, device="cuda")
    padded[lead:lead + n] = bits
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device="cuda")
    out = torch.empty(total // 8, dtype=torch.uint8, device="cuda")
    step = 1 << 27
    for i in range(0, total // 8, step):
        out[i:i + step] = (padded[8 * i:8 * (i + step)].view(-1, 8).to(torch.int32) * weights).sum(dim=1).to(torch.uint8)
    return out


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
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    byte_col = torch.empty(n, dtype=torch.uint8, device="cuda")
    mapq = torch.empty(n, dtype=torch.uint8, device="cuda")
    for i in range(0, n, step):
        byte_col[i:i + step] = (torch.rand(min(step, n - i), device="cuda", generator=gen) < args.density).to(torch.uint8)
        mapq[i:i + step] = torch.randint(0, 61, (min(step, n - i),), device="cuda", generator=gen, dtype=torch.uint8)
    bits0, bits3 = packed(byte_col, 0), packed(byte_col, FUNNEL_OFFSET)
    ones = torch.ones(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    forms = (("bitmap", bits0, 0, 1, 0.125), ("bitmap, funnelled", bits3, FUNNEL_OFFSET, 1, 0.125), ("bytes", byte_col, 0, 8, 1.0))

    for min_mapq in (0, 30):
        for name, off in layouts(n):
            nseg = off.numel() - 1
            words = [torch.zeros(nseg * 34, dtype=torch.int64, device="cuda") for _ in forms]
            filt = torch.zeros(nseg * 34, dtype=torch.int64, device="cuda")

            def parent(i):
                t = cols[i % len(cols)]
                check_hip(lib.fsk_launch_segments_wide_filter(t.data_ptr(), W, mapq.data_ptr() if min_mapq else None, 0, n, off.data_ptr(), nseg,
                                                              0, EXCLUDE, min_mapq, filt.data_ptr(), filt.data_ptr() + nseg * 256,
                                                              filt.data_ptr() + nseg * 264, 1, seg_grid, stream), "fsk_launch_segments_wide_filter")

            def mine_of(s, so, sb, w):
                def mine(i):
                    t = cols[i % len(cols)]
                    check_hip(lib.fsk_launch_segments_wide_masked_filter(t.data_ptr(), W, mapq.data_ptr() if min_mapq else None, s.data_ptr(), so,
                                                                         sb, 0, n, off.data_ptr(), nseg, 0, EXCLUDE, min_mapq, w.data_ptr(),
                                                                         w.data_ptr() + nseg * 256, w.data_ptr() + nseg * 264, 1, seg_grid,
                                                                         stream), "fsk_launch_segments_wide_masked_filter")
                return mine

            mine = [mine_of(s, so, sb, words[k]) for k, (_, s, so, sb, _) in enumerate(forms)]
            all_ones = mine_of(ones, 0, 8, words[0])
            # parity of what is measured, on every column
            for b in range(len(cols)):
                parent(b)
                all_ones(b)
                torch.cuda.synchronize()
                assert torch.equal(words[0], filt), "an all-ones mask differs from fsk_launch_segments_wide_filter"
                for f in mine:
                    f(b)
                torch.cuda.synchronize()
                assert torch.equal(words[0], words[1]) and torch.equal(words[0], words[2]), "the three forms of the same mask differ"
                counted, passing = int(words[0][nseg * 32:nseg * 33].sum()), int(filt[nseg * 32:nseg * 33].sum())
                assert 0 < counted < passing < n, "a part must pass and a part of that must be selected"
            print("W = %d, -F 0x904%s, %s: %d segments; the three forms agree on every column and an all-ones mask gives "
                  "fsk_launch_segments_wide_filter's words" % (W, " -q 30" if min_mapq else "", name, nseg), flush=True)
            if args.quick:
                continue
            fns = [parent] + mine
            for fn in fns:                                   # warm-up: every call once more, untimed
                fn(0)
            torch.cuda.synchronize()
            ts = [[] for _ in fns]
            for _ in range(args.rounds):
                for k, fn in enumerate(fns):
                    ts[k].append(timed(fn, args.reps))
            m = [statistics.median(x) for x in ts]
            moved = W + (1 if min_mapq else 0)               # the parent's bytes per element
            pred = "-F 0x904 -q 30" if min_mapq else "-F 0x904      "
            print("W = %d, %s, %-26s: (a) segments_wide_filter %s = %.3f TB/s" % (W, pred, name, med(ts[0]), moved * n / m[0] / 1e9), flush=True)
            for k, (label, _, _, _, extra) in enumerate(forms, 1):
                bound = m[0] * (moved + extra) / moved * 1.03
                print("W = %d, %s, %-26s: %-18s %s = %.3f TB/s   / (a) %.4f   yardstick (a) x %.4f x 1.03 = %.4f ms: %s (%+.1f %%)"
                      % (W, pred, name, label, med(ts[k]), (moved + extra) * n / m[k] / 1e9, m[k] / m[0], (moved + extra) / moved, bound,
                         "met" if m[k] <= bound else "MISSED", 100 * (m[k] / bound - 1)), flush=True)
            del words, filt
    del cols, byte_col, mapq, bits0, bits3, ones
    torch.cuda.empty_cache()
