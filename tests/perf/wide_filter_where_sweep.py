#!/usr/bin/env python3
"""Filtered and selected flagstat of int32 / int64 columns at full size: `python3 tests/perf/wide_filter_where_sweep.py
[--bytes N] [--rounds R] [--reps K] [--buffers B] [--quick]` -- per width, B (default 2) device-resident columns of N bytes
(default 8 GiB: every pass reads 32 times the 256 MiB cache) of int32 / int64 elements whose low halves are NA12878-like flags
(filled on the device), one uint8 MAPQ column uniform over 0..60, and per mask density (0.01, 0.5, 0.99) one boolean mask as bytes,
as an LSB-first bitmap and as the same bitmap 3 bits into its first byte.  Timed with hipEvents after warm-up; the calls of a
timed window rotate over the B columns.  In one run, ALTERNATING, under -F 0x904 (no MAPQ column, Q = 0) and under -F 0x904 -q 30
(Q = 1):

  (f)  fsk_launch_wide_filter with the same predicate (the parent kernel of this build)            W + Q bytes per element
  (w1) fsk_launch_wide_filter_where, bitmap at bit offset 0 (one selection byte per lane, vector)  W + Q + 1/8 bytes per element
  (w3) ... the bitmap at bit offset 3 (the funnelled form: two selection bytes)                    W + Q + 1/8 bytes per element
  (w8) ... the byte form                                                                           W + Q + 1 bytes per element

and at density 0.5 under -F 0x904 -q 30, over the first 2^30 elements (all of them where the column is shorter), the two routes
a caller had without this kernel, on the same tensors:

  (c1) the filter as a torch expression ANDed with the mask, then wide_where.count_torch_ints_where
  (c2) t.to(torch.int16) followed by filter_where.count_torch_filter_where

Printed per width, predicate and density: median ms per call over the rounds with the spread, the time ratios (w1) / (f),
(w3) / (f) and (w8) / (f) beside their yardsticks (the ratio of bytes moved plus 3 %), and (c1), (c2) over (w8) on the same
elements.  Before anything is timed the counters and `selected` of (w1), (w3) and (w8) are compared, on the first column, with
fsk_launch_wide_where under the combined mask built by torch, and `high` with 0.  --quick: one call of each after one warm-up."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from libflagstats_amd import _lib, device, filter_where, kernel_id, wide_where  # noqa: E402

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
print("wide_filter_where_sweep: %d bytes (%.2f GiB) per column, %d columns per width, NA12878-like low halves, MAPQ uniform 0..60; "
      "rounds %d x reps %d; launcher grid %d; K1 code object %s"
      % (nbytes, nbytes / 2 ** 30, args.buffers, args.rounds, args.reps, grid, kernel_id.kernel_id()), flush=True)

EXCLUDE, MIN_MAPQ = 0x904, 30
PREDS = (("-F 0x904", 0), ("-F 0x904 -q 30", MIN_MAPQ))


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


STEP = 1 << 26
WEIGHTS = None


def pack_bits(m):
    """a bool tensor of a multiple of 8 elements as an LSB-first bitmap"""
    global WEIGHTS
    if WEIGHTS is None:
        WEIGHTS = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device="cuda")
    out = torch.empty(m.numel() // 8, dtype=torch.uint8, device="cuda")
    for i in range(0, m.numel(), STEP):
        c = m[i:i + STEP].view(-1, 8).to(torch.uint8) * WEIGHTS
        out[i // 8:i // 8 + c.shape[0]] = c.sum(1, dtype=torch.uint8)
    return out


flt_out = torch.zeros(34, dtype=torch.int64, device="cuda")
ref_out = torch.zeros(34, dtype=torch.int64, device="cuda")
out = torch.zeros(34, dtype=torch.int64, device="cuda")
pad3, pad5 = torch.zeros(3, dtype=torch.bool, device="cuda"), torch.zeros(5, dtype=torch.bool, device="cuda")

for W, dt in ((4, torch.int32), (8, torch.int64)):
    n = nbytes // W
    flags16 = torch.empty(n, dtype=torch.int16, device="cuda")
    cols = []
    for b in range(args.buffers):
        device.generate_torch(flags16, device.GEN_NA12878, seed=11 + b, mask=0)
        t = torch.empty(n, dtype=dt, device="cuda")
        for i in range(0, n, STEP):
            t[i:i + STEP] = flags16[i:i + STEP].to(dt) & 0xFFFF
        cols.append(t)
    del flags16
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    mapq = torch.empty(n, dtype=torch.uint8, device="cuda")
    for i in range(0, n, STEP):
        c = min(STEP, n - i)
        mapq[i:i + c] = torch.randint(0, 61, (c,), device="cuda", generator=gen, dtype=torch.uint8)

    for density in (0.01, 0.5, 0.99):
        m = torch.empty(n, dtype=torch.bool, device="cuda")
        for i in range(0, n, STEP):
            c = min(STEP, n - i)
            m[i:i + c] = torch.rand(c, device="cuda", generator=gen) < density
        bits0 = pack_bits(m)
        bits3 = pack_bits(torch.cat([pad3, m, pad5]))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()

        for pname, mn in PREDS:
            Q = 1 if mn else 0
            mq = mapq.data_ptr() if mn else None

            def parent(i, mode=0):
                t = cols[i % len(cols)]
                check_hip(lib.fsk_launch_wide_filter(t.data_ptr(), n, W, 0, EXCLUDE, mq, mn, flt_out.data_ptr(), flt_out.data_ptr() + 256,
                                                     flt_out.data_ptr() + 264, mode, grid, stream), "fsk_launch_wide_filter")

            def mine(sel, off, sel_bits):
                def run(i, mode=0):
                    t = cols[i % len(cols)]
                    check_hip(lib.fsk_launch_wide_filter_where(t.data_ptr(), n, W, 0, EXCLUDE, mq, mn, sel.data_ptr(), off, sel_bits,
                                                               out.data_ptr(), out.data_ptr() + 256, out.data_ptr() + 264, mode, grid, stream),
                              "fsk_launch_wide_filter_where")
                return run

            forms = (("w1", mine(bits0, 0, 1)), ("w3", mine(bits3, 3, 1)), ("w8", mine(m, 0, 8)))
            # parity of what is measured, on the first column: the three forms == the selected wide kernel under the combined mask
            cm = torch.empty(n, dtype=torch.bool, device="cuda")
            for i in range(0, n, STEP):
                c = (cols[0][i:i + STEP] & EXCLUDE) == 0
                if mn:
                    c &= mapq[i:i + STEP] >= mn
                cm[i:i + STEP] = c & m[i:i + STEP]
            check_hip(lib.fsk_launch_wide_where(cols[0].data_ptr(), n, W, cm.data_ptr(), 0, 8, ref_out.data_ptr(), ref_out.data_ptr() + 256,
                                                ref_out.data_ptr() + 264, 1, grid, stream), "fsk_launch_wide_where")
            for name, fn in forms:
                fn(0, 1)
                torch.cuda.synchronize()
                assert torch.equal(out[:33], ref_out[:33]) and int(out[33]) == 0, "%s differs from wide_where under the combined mask" % name
            del cm
            print("W = %d %s density %.2f: %d of %d elements counted in the first column; counters and selected of (w1), (w3), (w8) equal "
                  "wide_where's under the combined mask, high == 0" % (W, pname, density, int(out[32]), n), flush=True)
            parent(0)
            torch.cuda.synchronize()
            if args.quick:
                continue
            times = {k: [] for k in ("f", "w1", "w3", "w8")}
            for _ in range(args.rounds):
                times["f"].append(timed(parent, args.reps))
                for name, fn in forms:
                    times[name].append(timed(fn, args.reps))
            med = {k: statistics.median(v) for k, v in times.items()}
            per_elem = {"f": W + Q, "w1": W + Q + 0.125, "w3": W + Q + 0.125, "w8": W + Q + 1}
            for k in ("f", "w1", "w3", "w8"):
                print("W = %d %s density %.2f (%-2s): %.4f ms [%.4f .. %.4f] = %.3f TB/s at %.3f B/element, %.1f Gelements/s"
                      % (W, pname, density, k, med[k], min(times[k]), max(times[k]), per_elem[k] * n / med[k] / 1e9, per_elem[k],
                         n / med[k] / 1e6), flush=True)
            for k in ("w1", "w3", "w8"):
                moved = per_elem[k] / per_elem["f"]
                r = med[k] / med["f"]
                print("W = %d %s density %.2f: (%s)/(f) time %.4f, yardstick %.4f (bytes moved %.5f + 3 %%): %s"
                      % (W, pname, density, k, r, moved + 0.03, moved, "met" if r <= moved + 0.03 else "MISSED"), flush=True)
            if density == 0.5 and mn:
                # the two routes a caller had, over at most 2^30 elements of the same tensors
                n30 = min(n, 1 << 30)
                sub, subm, subq = [t[:n30] for t in cols], m[:n30], mapq[:n30]
                o32, o1, o1b, o1c = (torch.zeros(k, dtype=torch.int64, device="cuda") for k in (32, 1, 1, 1))

                def expression(i):
                    t = sub[i % len(sub)]
                    wide_where.count_torch_ints_where(t, ((t & EXCLUDE) == 0) & (subq >= mn) & subm, out=o32, selected=o1, high=o1c, store=True)

                def narrow(i):
                    filter_where.count_torch_filter_where(sub[i % len(sub)].to(torch.int16), subm, exclude=EXCLUDE, mapq=subq, min_mapq=mn,
                                                          out=o32, selected=o1b, store=True)

                def mine30(i):
                    t = sub[i % len(sub)]
                    check_hip(lib.fsk_launch_wide_filter_where(t.data_ptr(), n30, W, 0, EXCLUDE, subq.data_ptr(), mn, subm.data_ptr(), 0, 8,
                                                               out.data_ptr(), out.data_ptr() + 256, out.data_ptr() + 264, 1, grid, stream),
                              "fsk_launch_wide_filter_where")

                mine30(0)
                expression(0)
                torch.cuda.synchronize()
                assert torch.equal(out[:32], o32) and int(out[32]) == int(o1[0]), "the torch expression + count_torch_ints_where differs"
                narrow(0)
                torch.cuda.synchronize()
                assert torch.equal(out[:32], o32) and int(out[32]) == int(o1b[0]), ".to(int16) + count_torch_filter_where differs"
                c1, c2, w = [], [], []
                for _ in range(max(2, args.rounds // 2)):
                    w.append(timed(mine30, args.reps))
                    c1.append(timed(expression, 2))
                    c2.append(timed(narrow, 2))
                wm, c1m, c2m = (statistics.median(x) for x in (w, c1, c2))
                print("W = %d %s density 0.50, %d elements: (w8) %.4f ms   (c1) torch expression & mask + count_torch_ints_where %.4f ms = "
                      "%.1f x   (c2) .to(int16) + count_torch_filter_where %.4f ms = %.1f x" % (W, pname, n30, wm, c1m, c1m / wm, c2m, c2m / wm),
                      flush=True)
                del sub, subm, subq
        del m, bits0, bits3
        torch.cuda.empty_cache()
    del cols, mapq
    torch.cuda.empty_cache()
