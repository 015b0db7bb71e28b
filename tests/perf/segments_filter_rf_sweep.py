#!/usr/bin/env python3
"""Filtered segmented flagstat under samtools' whole FLAG predicate at full size: `python3 tests/perf/segments_filter_rf_sweep.py
[--flags N] [--rounds R] [--reps K] [--buffers B] [--check-flags N] [--quick]` -- B (default 2) device-resident uint16 arrays of N
flags (default 2^32: every pass reads 32 times the 256 MiB cache), NA12878-like, filled on the device, and one uint8 MAPQ column
beside them (three quarters 60, the rest uniform in 0..59), timed with hipEvents after warm-up.  The calls of a timed window
rotate over the B arrays.  The layouts of tests/perf/segments_filter_sweep.py:

  P1  one segment over the whole array
  P2  512,000-flag segments (the column store's block)
  P3  random lengths 0..2000 (mean 1000)

Every arm is -F 0x904 plus what it names, without and with -q 30, and runs ALTERNATING with its yardstick in the same process:

  (a)  FLAGSTATS_hip_device_u16_segments_filter with -F 0x904 [-q 30]: fsk::flagstat_segments_filter, the parent's kernel
  (b1) FLAGSTATS_hip_device_u16_segments_filter_rf with --rf 0x50    the any-of test alone      flagstat_segments_filter_rf<., 1, 0>
  (b2) ... with -G 0x420                                             the all-of test alone      <., 0, 1>
  (b3) ... with --rf 0x210 -G 0x480                                  both, across byte planes   <., 1, 1>
  (b4) ... with --rf 0x40                                            reduced to -f 0x40 -F 0x904: flagstat_segments_filter itself
  (c)  FLAGSTATS_hip_device_u16_filter over the whole array, -F 0x904 [-q 30]
  (d)  FLAGSTATS_hip_device_u16_filter_rf over the whole array, for (b1) .. (b3): (d)/(c) is what the tests cost a whole column

Yardsticks, none a time fixed in advance: (b4) is (a)'s time in the same rounds plus 3 % (the same kernel, the same bytes);
(b1) .. (b3) on P1 and P2 are (a)'s time times (d)/(c) of the same arm in the same run, plus 3 % -- the segmented form is not
asked to beat the whole-column cost of the tests, only not to add to it; on P3 the same product times 1.07, what the shared walk
cost the parent on such segments (profiles/r18/ab_flagstat_segments_filter.log), plus 3 %.  Printed: median ms per call over the
rounds with the spread, the ratio, the yardstick, MET or MISSED.  Before anything is timed, rows and `selected` of (b) over the
first --check-flags flags (default 2^28) of every array are compared, on a handful of segments of the layout, with
filter_rf.count_torch_filter_rf over each segment's slice.  --quick: one call of each after one warm-up."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from libflagstats_amd import _lib, device, filter_rf, kernel_id  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--flags", type=int, default=2 ** 32)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--buffers", type=int, default=2)
ap.add_argument("--check-flags", type=int, default=1 << 28)
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()

import torch  # noqa: E402

lib = _lib.lib()
_lib.check(lib.FLAGSTATS_hip_init(0), "init")
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
n = args.flags
n_check = min(n, args.check_flags)
print("segments_filter_rf_sweep: %d flags (%.2f GiB) per array, %d arrays, + %d MAPQ bytes, NA12878-like; rounds %d x reps %d; check over "
      "%d flags; K1 code object %s" % (n, 2 * n / 2 ** 30, args.buffers, n, args.rounds, args.reps, n_check, kernel_id.kernel_id()), flush=True)

arrays = []
for b in range(args.buffers):
    t = torch.empty(n, dtype=torch.int16, device="cuda")
    device.generate_torch(t, device.GEN_NA12878, seed=11 + b, mask=0)
    arrays.append(t)
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
torch.cuda.empty_cache()

rng = np.random.RandomState(7)
lengths = rng.randint(0, 2001, n // 1000 + 1000)
o3 = np.concatenate([[0], np.cumsum(lengths)])
# name, offsets, what the shared walk may cost on top (1.07: the r18 figure for ~1,000-flag segments)
LAYOUTS = (("P1 one segment", np.array([0, n], dtype=np.int64), 1.0),
           ("P2 512,000-flag blocks", np.append(np.arange(0, n, 512_000, dtype=np.int64), n), 1.0),
           ("P3 random lengths, mean 1000", np.append(o3[o3 < n], n).astype(np.int64), 1.07))
EXCLUDE = 0x904
# name, text, include_any, exclude_all, what fsk_filter_rf_reduce answers
ARMS = (("b1", "--rf 0x50", 0x0050, 0, 2), ("b2", "-G 0x420", 0, 0x0420, 2), ("b3", "--rf 0x210 -G 0x480", 0x0210, 0x0480, 2),
        ("b4", "--rf 0x40 (reduced)", 0x0040, 0, 1))
reduced = (ctypes.c_uint32 * 4)()
for name, text, include_any, exclude_all, kind in ARMS:
    assert lib.fsk_filter_rf_reduce(0, EXCLUDE, include_any, exclude_all, reduced) == kind, (name, tuple(reduced))


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(base, mine):
    """median ms of both, and the ratios round by round"""
    bs, ws = [], []
    for _ in range(args.rounds):
        bs.append(timed(base, args.reps))
        ws.append(timed(mine, args.reps))
    return statistics.median(bs), statistics.median(ws), bs, ws


# ---- (c), (d): what the tests cost a whole column, per arm and threshold
whole_out = torch.zeros(33, dtype=torch.int64, device="cuda")
whole_ratio = {}
for min_mapq in (0, 30):
    q = mapq.data_ptr() if min_mapq else None

    def whole_base(i):
        _lib.check(lib.FLAGSTATS_hip_device_u16_filter(arrays[i % len(arrays)].data_ptr(), n, 0, EXCLUDE, q, min_mapq, whole_out.data_ptr(),
                                                       whole_out.data_ptr() + 256, 0, stream), "FLAGSTATS_hip_device_u16_filter")

    for name, text, include_any, exclude_all, kind in ARMS[:3]:
        def whole_mine(i):
            _lib.check(lib.FLAGSTATS_hip_device_u16_filter_rf(arrays[i % len(arrays)].data_ptr(), n, 0, EXCLUDE, include_any, exclude_all, q,
                                                              min_mapq, whole_out.data_ptr(), whole_out.data_ptr() + 256, 0, stream),
                       "FLAGSTATS_hip_device_u16_filter_rf")

        whole_base(0)
        whole_mine(1)
        torch.cuda.synchronize()
        if args.quick:
            whole_ratio[name, min_mapq] = 1.0
            continue
        cm, dm, cs, ds = alternate(whole_base, whole_mine)
        whole_ratio[name, min_mapq] = dm / cm
        per_flag = 3 if min_mapq else 2
        print("whole column (%s) -F 0x904 %s%s: (c) filter %.4f ms = %.3f TB/s [%.4f .. %.4f ms]   (d) filter_rf %.4f ms = %.3f TB/s at %d B/flag "
              "[%.4f .. %.4f ms]   (d)/(c) %.4f" % (name, text, " -q 30" if min_mapq else "", cm, per_flag * n / cm / 1e9, min(cs), max(cs), dm,
                                                   per_flag * n / dm / 1e9, per_flag, min(ds), max(ds), dm / cm), flush=True)

# ---- (a), (b): the segmented entries per layout
met = missed = 0
for lname, o, walk in LAYOUTS:
    nseg = o.size - 1
    offs = torch.from_numpy(o).cuda()
    rows = torch.empty((nseg, 32), dtype=torch.int64, device="cuda")
    sel = torch.empty(nseg, dtype=torch.int64, device="cuda")
    base_rows = torch.empty((nseg, 32), dtype=torch.int64, device="cuda")
    base_sel = torch.empty(nseg, dtype=torch.int64, device="cuda")
    # a handful of segments of the layout cut to the check slice: the first, some in the middle, the last
    o_small = np.unique(np.clip(o, 0, n_check))
    ns = o_small.size - 1
    offs_small = torch.from_numpy(o_small).cuda()
    picks = sorted({0, 1, ns // 3, ns // 2, ns - 2, ns - 1} & set(range(ns)))
    ref_rows = torch.zeros(32, dtype=torch.int64, device="cuda")
    ref_sel = torch.zeros(1, dtype=torch.int64, device="cuda")
    for name, text, include_any, exclude_all, kind in ARMS:
        for min_mapq in (0, 30):
            label = "-F 0x904 %s%s" % (text, " -q 30" if min_mapq else "")
            q = mapq.data_ptr() if min_mapq else None

            def base(i, count=n, d_o=offs, k=nseg):
                _lib.check(lib.FLAGSTATS_hip_device_u16_segments_filter(arrays[i % len(arrays)].data_ptr(), count, d_o.data_ptr(), k, 0, EXCLUDE,
                                                                        q, min_mapq, base_rows.data_ptr(), base_sel.data_ptr(), 1, stream),
                           "FLAGSTATS_hip_device_u16_segments_filter")

            def mine(i, count=n, d_o=offs, k=nseg):
                _lib.check(lib.FLAGSTATS_hip_device_u16_segments_filter_rf(arrays[i % len(arrays)].data_ptr(), count, d_o.data_ptr(), k, 0,
                                                                           EXCLUDE, include_any, exclude_all, q, min_mapq, rows.data_ptr(),
                                                                           sel.data_ptr(), 1, stream),
                           "FLAGSTATS_hip_device_u16_segments_filter_rf")

            # parity of what is measured: per picked segment, the whole-column entry over the segment's slice
            for b in range(len(arrays)):
                mine(b, n_check, offs_small, ns)
                torch.cuda.synchronize()
                for s in picks:
                    lo, hi = int(o_small[s]), int(o_small[s + 1])
                    filter_rf.count_torch_filter_rf(arrays[b][lo:hi], exclude=EXCLUDE, include_any=include_any, exclude_all=exclude_all,
                                                    mapq=mapq[lo:hi] if min_mapq else None, min_mapq=min_mapq, out=ref_rows, selected=ref_sel,
                                                    store=True)
                    torch.cuda.synchronize()
                    assert torch.equal(rows[s], ref_rows) and int(sel[s]) == int(ref_sel[0]), (lname, label, b, s, "!= count_torch_filter_rf")
            mine(0)
            torch.cuda.synchronize()
            print("%-30s (%s) %-39s nseg %9d: %d of %d flags pass in the first array; rows and selected of %d segments within the first %d "
                  "flags of every array equal count_torch_filter_rf's over their slices"
                  % (lname, name, label, nseg, int(sel.sum()), n, len(picks), n_check), flush=True)
            base(0)
            mine(1)
            torch.cuda.synchronize()
            if args.quick:
                continue
            am, bm, As, Bs = alternate(base, mine)
            ratio = bm / am
            if kind == 1:
                yard, how = 1.03, "1.030 (the same kernel)"
            else:
                w = whole_ratio[name, min_mapq]
                yard = w * walk * 1.03
                how = "%.4f = (d)/(c) %.4f%s x 1.03" % (yard, w, " x 1.07" if walk != 1.0 else "")
            ok = ratio <= yard
            met += ok
            missed += not ok
            per_flag = 3 if min_mapq else 2
            print("%-30s (%s) %-39s: (a) segments_filter -F 0x904%s %.4f ms = %.3f TB/s [%.4f .. %.4f ms]   (b) segments_filter_rf %.4f ms = "
                  "%.3f TB/s at %d B/flag [%.4f .. %.4f ms]   (b)/(a) time %.4f [%.4f .. %.4f], yardstick %s: %s"
                  % (lname, name, label, " -q 30" if min_mapq else "", am, per_flag * n / am / 1e9, min(As), max(As), bm, per_flag * n / bm / 1e9,
                     per_flag, min(Bs), max(Bs), ratio, min(y / x for x, y in zip(As, Bs)), max(y / x for x, y in zip(As, Bs)), how,
                     "MET" if ok else "MISSED"), flush=True)
    del rows, sel, base_rows, base_sel, offs, offs_small
    torch.cuda.empty_cache()
if not args.quick:
    print("segments_filter_rf_sweep: %d arms MET, %d MISSED" % (met, missed), flush=True)
