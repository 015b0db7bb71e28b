#!/usr/bin/env python3
"""Filtered and selected segmented flagstat at full size: `python3 tests/perf/segments_filter_where_sweep.py [--flags N]
[--rounds R] [--reps K] [--today-flags N] [--oracle-flags N] [--densities d,d,d] [--quick]` -- N (default 2^32) device-resident
NA12878-like uint16 flags (filled on the device), a uint8 MAPQ column beside them (three quarters 60, the rest uniform in 0..59)
and a random selection of every density given (default 0.01, 0.5, 0.99) as a boolean mask and as an LSB-first bitmap, timed with
hipEvents after warm-up.  The layouts of tests/perf/segments_sweep.py:

  P1  one segment over the whole array
  P2  512,000-flag segments (the column store's block)
  P3  random lengths 0..2000 (mean 1000)

In one run, per density, per predicate (-F 0x904; -F 0x904 -q 30) and per layout, ALTERNATING:

  (a)  FLAGSTATS_hip_device_u16_segments_filter, same predicate, same layout       2 or 3 B per flag -- the yardstick's base
  (w)  FLAGSTATS_hip_device_u16_filter_where over the whole column, bitmap         2.125 or 3.125 B per flag, one row
  (b1) FLAGSTATS_hip_device_u16_segments_filter_where, bitmap at bit offset 0      2.125 or 3.125 B per flag
  (b2) ... bitmap at bit offset 3 (two bytes funnelled per vector)                 2.125 or 3.125 B per flag
  (b3) ... boolean mask (without -q: flagstat_segments_filter<true> on the mask)   3 or 4 B per flag
  (c)  what a torch caller does today, over the first --today-flags flags (default 2^30: the limit of torch's mask indexing):
       the torch expression for the filter's mask ANDed with the boolean mask, t[m], a cumulative sum of m read at the offsets,
       segments.count_segments_torch on the compacted copy; beside (b3) over the same slice

Yardstick of a form on P1 and P2: the time of (a) in the same run, times the ratio of the bytes moved, plus 3 %.  P3 is
instruction-bound and only reported.  Printed: median ms per call over the rounds with the spread, (b) / (a), the yardstick's
ratio and MEETS or MISSES (P3: REPORTED), (b1) / (w), and (c) / (b3).  Before anything is timed, in the measured configuration:
over the first --oracle-flags flags (default 2^22) rows and `selected` of the three forms equal
tests/segments_filter_where_oracle.want exactly; over the whole array the rows of (b1) sum to (w)'s counters and `selected` to its
count and (b3) equals (b1); over the (c) slice rows and `selected` of (b3) equal (c)'s.
--quick: one call of each after one warm-up (for rocprofv3 runs: --kernel-trace --stats, or --pmc on its own)."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import segments_filter_where_oracle as sfwo  # noqa: E402
from libflagstats_amd import _lib, device, kernel_id, segments  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--flags", type=int, default=1 << 32)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--today-flags", type=int, default=1 << 30)
ap.add_argument("--oracle-flags", type=int, default=1 << 22)
ap.add_argument("--densities", default="0.01,0.5,0.99")
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()

import torch  # noqa: E402

lib = _lib.lib()
_lib.check(lib.FLAGSTATS_hip_init(0), "init")
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
n = args.flags // 16384 * 16384
n_today = min(n, args.today_flags) // 16384 * 16384
n_oracle = min(n, args.oracle_flags)
PAD = 64                                          # selection elements behind the n-th: the bitmap at bit offset 3 reaches into them
print("segments_filter_where_sweep: %d flags (%.2f GiB) + %d MAPQ bytes + a selection, NA12878-like; rounds %d x reps %d; (c) over %d "
      "flags; oracle over %d flags; K1 code object %s" % (n, 2 * n / 2 ** 30, n, args.rounds, args.reps, n_today, n_oracle,
                                                          kernel_id.kernel_id()), flush=True)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def u64(x):
    return x.cpu().numpy().view(np.uint64)


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


rng = np.random.RandomState(7)
lengths = rng.randint(0, 2001, n // 1000 + 1000)
o3 = np.concatenate([[0], np.cumsum(lengths)])
LAYOUTS = (("P1 one segment", np.array([0, n], dtype=np.int64), True),
           ("P2 512,000-flag blocks", np.append(np.arange(0, n, 512_000, dtype=np.int64), n), True),
           ("P3 random lengths, mean 1000", np.append(o3[o3 < n], n).astype(np.int64), False))
PREDICATES = (("-F 0x904", 0, 0x904, 0), ("-F 0x904 -q 30", 0, 0x904, 30))
# name, text, selection, sel_offset, sel_bits, selection bytes per flag
FORMS = (("b1", "bitmap", bitmap, 0, 1, 0.125), ("b2", "bitmap funnelled", bitmap, 3, 1, 0.125), ("b3", "boolean mask", mask, 0, 8, 1.0))

host_t = t[:n_oracle].cpu().numpy().view(np.uint16)
host_q = mapq[:n_oracle].cpu().numpy()
whole = torch.zeros(33, dtype=torch.int64, device="cuda")
ts, qs = t[:n_today], mapq[:n_today]


def run_base(count, offs, nseg, pred, rows, cnt):
    _lib.check(lib.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), count, offs.data_ptr(), nseg, pred[1], pred[2],
                                                            mapq.data_ptr() if pred[3] else None, pred[3], rows.data_ptr(), cnt.data_ptr(), 1,
                                                            stream), "FLAGSTATS_hip_device_u16_segments_filter")


def run_whole(count, pred):
    _lib.check(lib.FLAGSTATS_hip_device_u16_filter_where(t.data_ptr(), count, pred[1], pred[2], mapq.data_ptr() if pred[3] else None, pred[3],
                                                         bitmap.data_ptr(), 0, 1, whole.data_ptr(), whole.data_ptr() + 256, 1, stream),
               "FLAGSTATS_hip_device_u16_filter_where")


def run_both(count, offs, nseg, pred, form, rows, cnt):
    _lib.check(lib.FLAGSTATS_hip_device_u16_segments_filter_where(t.data_ptr(), count, offs.data_ptr(), nseg, pred[1], pred[2],
                                                                  mapq.data_ptr() if pred[3] else None, pred[3], form[2].data_ptr(), form[3],
                                                                  form[4], rows.data_ptr(), cnt.data_ptr(), 1, stream),
               "FLAGSTATS_hip_device_u16_segments_filter_where")


def today_mask(pred):
    m = (ts & pred[2]) == 0
    if pred[1]:
        m = m & ((ts & pred[1]) == pred[1])
    if pred[3]:
        m = m & (qs >= pred[3])
    return m & mask[:n_today]


for density in (float(x) for x in args.densities.split(",")):
    fill_selection(density)
    host_m = mask[:n_oracle + PAD].cpu().numpy()
    for pred in PREDICATES:
        text = pred[0]
        base_bytes = 3.0 if pred[3] else 2.0
        for name, o, judged in LAYOUTS:
            nseg = o.size - 1
            offs = torch.from_numpy(o).cuda()
            rows = [torch.empty((nseg, 32), dtype=torch.int64, device="cuda") for _ in FORMS]
            cnt = [torch.empty(nseg, dtype=torch.int64, device="cuda") for _ in FORMS]
            base_rows = torch.empty((nseg, 32), dtype=torch.int64, device="cuda")
            base_cnt = torch.empty(nseg, dtype=torch.int64, device="cuda")
            o_today = np.unique(np.clip(o, 0, n_today)) if n_today < n else o
            offs_today = torch.from_numpy(o_today).cuda()
            nseg_today = o_today.size - 1
            o_small = np.unique(np.clip(o, 0, n_oracle))
            offs_small = torch.from_numpy(o_small).cuda()

            def base():
                run_base(n, offs, nseg, pred, base_rows, base_cnt)

            def whole_column():
                run_whole(n, pred)

            def part():
                run_both(n_today, offs_today, nseg_today, pred, FORMS[2], rows[2][:nseg_today], cnt[2][:nseg_today])

            def today():
                m = today_mask(pred)
                pre = torch.zeros(n_today + 1, dtype=torch.int64, device=ts.device)
                torch.cumsum(m, 0, out=pre[1:])
                compact = pre[offs_today]
                return segments.count_segments_torch(ts[m], compact), compact[1:] - compact[:-1]

            fulls = [(lambda k=k: run_both(n, offs, nseg, pred, FORMS[k], rows[k], cnt[k])) for k in range(len(FORMS))]
            # parity of what is measured: the oracle over a prefix (three forms), (c) over its slice, the whole-column kernel over all
            ns = o_small.size - 1
            for k, form in enumerate(FORMS):
                want_rows, want_sel = sfwo.want(host_t, o_small, host_m[form[3]:form[3] + n_oracle], pred[1], pred[2], host_q, pred[3])
                run_both(n_oracle, offs_small, ns, pred, form, rows[k][:ns], cnt[k][:ns])
                torch.cuda.synchronize()
                assert np.array_equal(u64(rows[k][:ns]), want_rows) and np.array_equal(u64(cnt[k][:ns]), want_sel), (density, text, name, form[1])
            part()
            r_today, s_today = today()
            torch.cuda.synchronize()
            assert torch.equal(rows[2][:nseg_today], r_today) and torch.equal(cnt[2][:nseg_today], s_today), (density, text, name, "today")
            del r_today, s_today
            for fn in [base, whole_column] + fulls:
                fn()
            torch.cuda.synchronize()
            assert torch.equal(rows[0].sum(dim=0), whole[:32]) and int(cnt[0].sum()) == int(whole[32]), (density, text, name, "whole column")
            assert torch.equal(rows[0], rows[2]) and torch.equal(cnt[0], cnt[2]), (density, text, name, "byte form")
            print("density %.2f, %-14s %-30s nseg %9d: %d of %d flags counted; rows and selected equal the oracle's over the first %d flags "
                  "(three forms), (c)'s over the first %d, and sum to the whole-column kernel's over all"
                  % (density, text, name, nseg, int(whole[32]), n, n_oracle, n_today), flush=True)
            part(), today()
            torch.cuda.synchronize()
            if args.quick:
                continue
            bs, hs, ss, cs, ws = [], [], [], [], [[] for _ in FORMS]
            for _ in range(args.rounds):
                bs.append(timed(base, args.reps))
                for k, fn in enumerate(fulls):
                    ws[k].append(timed(fn, args.reps))
                hs.append(timed(whole_column, args.reps))
                ss.append(timed(part, args.reps))
                cs.append(timed(today, max(1, args.reps // 5)))
            bm, hm, sm, cm = (statistics.median(x) for x in (bs, hs, ss, cs))
            head = "density %.2f, %-14s %-30s" % (density, text, name)
            print("%s: (a) segments_filter %.4f ms = %.3f TB/s at %.0f B/flag [%.4f .. %.4f ms]   (w) whole-column filter_where, bitmap "
                  "%.4f ms [%.4f .. %.4f ms]" % (head, bm, base_bytes * n / bm / 1e9, base_bytes, min(bs), max(bs), hm, min(hs), max(hs)),
                  flush=True)
            for (fname, form, sel, sel_offset, sel_bits, sel_bytes), w in zip(FORMS, ws):
                wm = statistics.median(w)
                per_flag = base_bytes + sel_bytes
                bound = per_flag / base_bytes * 1.03
                verdict = ("MEETS" if wm / bm <= bound else "MISSES") if judged else "REPORTED (instruction-bound layout, not judged)"
                print("%s: (%s) %-16s %.4f ms = %.3f TB/s at %.3f B/flag [%.4f .. %.4f ms], %.1f Gflags/s   (%s)/(a) time %.4f against the "
                      "yardstick %.4f (= %.3f / %.0f + 3 %%): %s   (%s)/(w) %.4f"
                      % (head, fname, form, wm, per_flag * n / wm / 1e9, per_flag, min(w), max(w), n / wm / 1e6, fname, wm / bm, bound, per_flag,
                         base_bytes, verdict, fname, wm / hm), flush=True)
            print("%s: over %d flags: (b3) %.4f ms, (c) torch masks ANDed + t[m] + cumsum at the offsets + count_segments_torch %.4f ms   "
                  "(c)/(b3) %.2f x" % (head, n_today, sm, cm, cm / sm), flush=True)
            del rows, cnt, base_rows, base_cnt, offs
            torch.cuda.empty_cache()
