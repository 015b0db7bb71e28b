#!/usr/bin/env python3
"""Filtered flagstat under a selection at full size: `python3 tests/perf/filter_where_sweep.py [--flags N] [--rounds R]
[--reps K] [--today-flags N] [--densities d,d,d] [--quick]` -- N (default 2^32) device-resident NA12878-like uint16 flags (filled
on the device), a uint8 MAPQ column beside them (three quarters 60, the rest uniform in 0..59) and a random selection of every
density given (default 0.01, 0.5, 0.99) as a boolean mask and as an LSB-first bitmap, timed with hipEvents after warm-up.  In one
run, per density and per predicate (-F 0x904; -F 0x904 -q 30), ALTERNATING:

  (a)  FLAGSTATS_hip_device_u16_filter with the predicate: flagstat_count_filter, 2 or 3 B per flag -- the yardstick's base
  (b1) FLAGSTATS_hip_device_u16_filter_where, bitmap at bit offset 0            2.125 or 3.125 B per flag
  (b2) ... bitmap at bit offset 3 (two bytes funnelled per vector)              2.125 or 3.125 B per flag
  (b3) ... boolean mask                                                         3 or 4 B per flag
  (c)  what a torch caller does today, over the first --today-flags flags (default 2^30): the torch expression for the filter's
       mask, ANDed with the boolean mask, followed by where.count_torch_where -- beside (b3) over the same slice

Yardstick of a form: the time of (a) in the same run, times the ratio of the bytes moved, plus 3 %.  Printed: median ms per call
over the rounds with the spread, (b) / (a), the yardstick's ratio and MEETS or MISSES, and (c) / (b3).  Before anything is timed
the counters and `selected` of every form over the slice are compared with (c)'s.  --quick: one call of each after one warm-up."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from libflagstats_amd import _lib, device, kernel_id, where  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--flags", type=int, default=1 << 32)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--today-flags", type=int, default=1 << 30)
ap.add_argument("--densities", default="0.01,0.5,0.99")
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()

import torch  # noqa: E402

lib = _lib.lib()
_lib.check(lib.FLAGSTATS_hip_init(0), "init")
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
n = args.flags // 16384 * 16384
n_today = min(n, args.today_flags) // 16384 * 16384
PAD = 64                                          # selection elements behind the n-th: the bitmap at bit offset 3 reaches into them
print("filter_where_sweep: %d flags (%.2f GiB) + %d MAPQ bytes + a selection, NA12878-like; rounds %d x reps %d; (c) over %d flags; "
      "K1 code object %s" % (n, 2 * n / 2 ** 30, n, args.rounds, args.reps, n_today, kernel_id.kernel_id()), flush=True)


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
mask = torch.empty(n + PAD, dtype=torch.bool, device="cuda")
bitmap = torch.empty((n + PAD) // 8, dtype=torch.uint8, device="cuda")
gen = torch.Generator(device="cuda")
gen.manual_seed(5)
step = 1 << 26
for i in range(0, n, step):
    c = min(step, n - i)
    low = torch.randint(0, 60, (c,), device="cuda", generator=gen, dtype=torch.uint8)
    keep = torch.rand(c, device="cuda", generator=gen) < 0.25
    mapq[i:i + c] = torch.where(keep, low, torch.full_like(low, 60))
del low, keep
weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device="cuda")


def fill_selection(density):
    """a fresh random mask of this density, and the same as an LSB-first bitmap"""
    for i in range(0, n + PAD, step):
        c = min(step, n + PAD - i)
        m = torch.rand(c, device="cuda", generator=gen) < density
        mask[i:i + c] = m
        bitmap[i // 8:(i + c) // 8] = (m.view(-1, 8).to(torch.uint8) * weights).sum(dim=1, dtype=torch.uint8)
    torch.cuda.synchronize()


out = torch.zeros(33, dtype=torch.int64, device="cuda")
base_out = torch.zeros(33, dtype=torch.int64, device="cuda")
today_out = torch.zeros(32, dtype=torch.int64, device="cuda")
today_sel = torch.zeros(1, dtype=torch.int64, device="cuda")
ts, qs = t[:n_today], mapq[:n_today]

PREDICATES = (("-F 0x904", 0, 0x904, 0), ("-F 0x904 -q 30", 0, 0x904, 30))
# name, text, selection pointer, sel_offset, sel_bits, selection bytes per flag
FORMS = (("b1", "bitmap", bitmap, 0, 1, 0.125), ("b2", "bitmap funnelled", bitmap, 3, 1, 0.125), ("b3", "boolean mask", mask, 0, 8, 1.0))


def run_filter(count, require, exclude, min_mapq, flags):
    _lib.check(lib.FLAGSTATS_hip_device_u16_filter(t.data_ptr(), count, require, exclude, mapq.data_ptr() if min_mapq else None, min_mapq,
                                                   base_out.data_ptr(), base_out.data_ptr() + 256, flags, stream),
               "FLAGSTATS_hip_device_u16_filter")


def run_both(count, require, exclude, min_mapq, sel, sel_offset, sel_bits, flags):
    _lib.check(lib.FLAGSTATS_hip_device_u16_filter_where(t.data_ptr(), count, require, exclude, mapq.data_ptr() if min_mapq else None,
                                                         min_mapq, sel.data_ptr(), sel_offset, sel_bits, out.data_ptr(),
                                                         out.data_ptr() + 256, flags, stream), "FLAGSTATS_hip_device_u16_filter_where")


def today_mask(require, exclude, min_mapq, shift):
    m = (ts & exclude) == 0
    if require:
        m = m & ((ts & require) == require)
    if min_mapq:
        m = m & (qs >= min_mapq)
    return m & mask[shift:shift + n_today]


def run_today(require, exclude, min_mapq, shift=0, store=False):
    where.count_torch_where(ts, today_mask(require, exclude, min_mapq, shift), out=today_out, selected=today_sel, store=store)


for density in (float(x) for x in args.densities.split(",")):
    fill_selection(density)
    for text, require, exclude, min_mapq in PREDICATES:
        base_bytes = 3.0 if min_mapq else 2.0
        # parity of what is measured, over the slice (c) takes: every form == where under torch's combined mask
        for name, form, sel, sel_offset, sel_bits, sel_bytes in FORMS:
            run_both(n_today, require, exclude, min_mapq, sel, sel_offset, sel_bits, 1)
            run_today(require, exclude, min_mapq, shift=sel_offset, store=True)
            torch.cuda.synchronize()
            assert torch.equal(out[:32], today_out) and int(out[32]) == int(today_sel[0]), \
                "filter_where counters (%s) differ from where's under torch's combined mask" % form
        run_both(n, require, exclude, min_mapq, mask, 0, 8, 1)
        torch.cuda.synchronize()
        print("density %.2f, %s: %d of %d flags counted; counters and selected of the three forms over the first %d flags equal "
              "count_torch_where's under torch's combined mask" % (density, text, int(out[32]), n, n_today), flush=True)

        def base():
            run_filter(n, require, exclude, min_mapq, 0)

        def part():
            run_both(n_today, require, exclude, min_mapq, mask, 0, 8, 0)

        def today():
            run_today(require, exclude, min_mapq)

        fulls = [(lambda f=f: run_both(n, require, exclude, min_mapq, f[2], f[3], f[4], 0)) for f in FORMS]
        for fn in [base, part, today] + fulls:
            fn()
        torch.cuda.synchronize()
        if args.quick:
            continue
        bs, ss, cs, ws = [], [], [], [[] for _ in FORMS]
        for _ in range(args.rounds):
            bs.append(timed(base, args.reps))
            for k, fn in enumerate(fulls):
                ws[k].append(timed(fn, args.reps))
            ss.append(timed(part, args.reps))
            cs.append(timed(today, max(1, args.reps // 5)))
        bm, sm, cm = (statistics.median(x) for x in (bs, ss, cs))
        print("density %.2f, %-14s: (a) filter %.4f ms = %.3f TB/s at %.0f B/flag [%.4f .. %.4f ms]" %
              (density, text, bm, base_bytes * n / bm / 1e9, base_bytes, min(bs), max(bs)), flush=True)
        for (name, form, sel, sel_offset, sel_bits, sel_bytes), w in zip(FORMS, ws):
            wm = statistics.median(w)
            per_flag = base_bytes + sel_bytes
            bound = per_flag / base_bytes * 1.03
            print("density %.2f, %-14s: (%s) %-16s %.4f ms = %.3f TB/s at %.3f B/flag [%.4f .. %.4f ms], %.1f Gflags/s   (%s)/(a) time "
                  "%.4f against the yardstick %.4f (= %.3f / %.0f + 3 %%): %s"
                  % (density, text, name, form, wm, per_flag * n / wm / 1e9, per_flag, min(w), max(w), n / wm / 1e6, name, wm / bm, bound,
                     per_flag, base_bytes, "MEETS" if wm / bm <= bound else "MISSES"), flush=True)
        print("density %.2f, %-14s: over %d flags: (b3) %.4f ms, (c) torch masks ANDed + count_torch_where %.4f ms   (c)/(b3) %.2f x"
              % (density, text, n_today, sm, cm, cm / sm), flush=True)
        if sm >= cm:
            print("FINDING: (b3) is not faster than (c) over the same %d flags" % n_today, flush=True)
