#!/usr/bin/env python3
"""Filtered segmented flagstat on int32 / int64 columns at full size: `python3 tests/perf/segments_wide_filter_sweep.py [--bytes N]
[--rounds R] [--reps K] [--buffers B] [--quick]` -- per width, B (default 2) device-resident columns of N bytes (default 8 GiB:
every pass reads 32 times the 256 MiB cache) of int32 / int64 elements whose low halves are NA12878-like flags (filled on the
device) and one uniform random MAPQ column, timed with hipEvents after warm-up; the calls of a timed window rotate over the B
columns.  Layouts: one segment; blocks of 512,000 elements; segments of ~1,000 elements (uniform in 500..1500).  Per layout the
predicates -F 0x904, -f 0x2 -F 0x904 and -F 0x904 -q 30, each timed in the same run, ALTERNATING, beside

  (a) fsk_launch_segments_wide on the same layout (the unfiltered segmented kernel of this build, store form)
  (b) fsk_launch_wide_filter over the whole column under the same predicate (the filtered kernel without segments, store form)
  (c) the route a caller had without this kernel: t.to(torch.int16) followed by segments_filter.count_segments_torch_filter

Printed per width, layout and predicate: median ms per call over the rounds with the spread (min .. max), and the ratios in time
mine / (a), mine / (b) and (c) / mine.  Before anything is timed the rows and counts of the new kernel are compared with (c)'s, their
sums with (b)'s counters and count, and the masks with 0, on every column.  --quick: parity only."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from libflagstats_amd import _lib, device, kernel_id, segments_filter  # noqa: E402

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
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
bpc = lib.FLAGSTATS_hip_get(b"blocks_per_cu")
cus = lib.FLAGSTATS_hip_compute_units()
wide_grid = cus * (bpc if bpc else 1)                   # the wide entries' grid
mu0, seg_bpc = ctypes.c_uint32(), ctypes.c_uint32()
lib.fsk_segments_policy(ctypes.byref(mu0), ctypes.byref(seg_bpc))
seg_grid = cus * seg_bpc.value                          # the segmented entries' grid
nbytes = args.bytes // 32768 * 32768
PREDICATES = (("-F 0x904", 0, 0x904, 0), ("-f 0x2 -F 0x904", 2, 0x904, 0), ("-F 0x904 -q 30", 0, 0x904, 30))
print("segments_wide_filter_sweep: %d bytes (%.2f GiB) per column, %d columns per width, NA12878-like low halves, uniform MAPQ; rounds %d x "
      "reps %d; wide grid %d, segments grid %d, min_units %d; K1 code object %s"
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
            ("~1,000-element segments", csr(short)))


whole = torch.zeros(34, dtype=torch.int64, device="cuda")

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
    gen.manual_seed(5)
    mapq = torch.empty(n, dtype=torch.uint8, device="cuda")
    for i in range(0, n, step):
        mapq[i:i + step] = torch.randint(0, 256, (min(step, n - i),), device="cuda", generator=gen, dtype=torch.int16).to(torch.uint8)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

    for name, off in layouts(n):
        nseg = off.numel() - 1
        words = torch.zeros(nseg * 34, dtype=torch.int64, device="cuda")
        rows, sel, high = words[:nseg * 32].view(nseg, 32), words[nseg * 32:nseg * 33], words[nseg * 33:]
        plain = torch.zeros(nseg * 33, dtype=torch.int64, device="cuda")
        today_rows = torch.zeros((nseg, 32), dtype=torch.int64, device="cuda")
        today_sel = torch.zeros(nseg, dtype=torch.int64, device="cuda")

        def unfiltered(i):
            t = cols[i % len(cols)]
            check_hip(lib.fsk_launch_segments_wide(t.data_ptr(), W, 0, n, off.data_ptr(), nseg, plain.data_ptr(),
                                                   plain.data_ptr() + nseg * 256, 1, seg_grid, stream), "fsk_launch_segments_wide")

        def calls(req, exc, mq):
            qp = mapq.data_ptr() if mq else None

            def mine(i):
                t = cols[i % len(cols)]
                check_hip(lib.fsk_launch_segments_wide_filter(t.data_ptr(), W, qp, 0, n, off.data_ptr(), nseg, req, exc, mq, rows.data_ptr(),
                                                              sel.data_ptr(), high.data_ptr(), 1, seg_grid, stream),
                          "fsk_launch_segments_wide_filter")

            def whole_column(i):
                t = cols[i % len(cols)]
                check_hip(lib.fsk_launch_wide_filter(t.data_ptr(), n, W, req, exc, qp, mq, whole.data_ptr(), whole.data_ptr() + 256,
                                                     whole.data_ptr() + 264, 1, wide_grid, stream), "fsk_launch_wide_filter")

            def today(i):
                t = cols[i % len(cols)]
                segments_filter.count_segments_torch_filter(t.to(torch.int16), off, require=req, exclude=exc, mapq=mapq if mq else None,
                                                            min_mapq=mq, out=today_rows, selected=today_sel, store=True)

            return mine, whole_column, today

        fns = {p[0]: calls(*p[1:]) for p in PREDICATES}
        # parity of what is measured, on every column
        for pname, (mine, whole_column, today) in fns.items():
            for b in range(len(cols)):
                mine(b)
                today(b)
                whole_column(b)
                torch.cuda.synchronize()
                assert torch.equal(rows, today_rows) and torch.equal(sel, today_sel), "rows or counts differ from .to(int16) + count_segments_torch_filter"
                assert torch.equal(rows.sum(dim=0), whole[:32]) and int(sel.sum()) == int(whole[32]), "rows do not sum to the wide filter's counters"
                assert not bool(high.any()) and int(whole[33]) == 0 and 0 < int(whole[32]) < n, "masks must be 0, the predicate must select a part"
        print("W = %d, %s: %d segments; rows and counts equal .to(int16) + count_segments_torch_filter's and sum to fsk_launch_wide_filter's on "
              "every column and predicate, masks 0" % (W, name, nseg), flush=True)
        if args.quick:
            continue
        for fn in (unfiltered,) + tuple(f for fs in fns.values() for f in fs):     # warm-up: every call once more, untimed
            fn(0)
        torch.cuda.synchronize()
        ua = []
        per = {p[0]: ([], [], []) for p in PREDICATES}
        for _ in range(args.rounds):
            ua.append(timed(unfiltered, args.reps))
            for pname, (mine, whole_column, today) in fns.items():
                per[pname][0].append(timed(mine, args.reps))
                per[pname][1].append(timed(whole_column, args.reps))
                per[pname][2].append(timed(today, max(2, args.reps // 5)))
        am = statistics.median(ua)
        print("W = %d, %-26s: (a) segments wide, no filter %s = %.3f TB/s" % (W, name, med(ua), W * n / am / 1e9), flush=True)
        for pname, (ms, bs, cs) in per.items():
            mm, bm, cm = (statistics.median(x) for x in (ms, bs, cs))
            print("W = %d, %-26s: %-16s segments wide filter %s = %.3f TB/s of elements   / (a) %.4f   (b) wide filter, whole column %s   / (b) "
                  "%.4f   (c) .to(int16) + count_segments_torch_filter %s   (c) / this %.2f x"
                  % (W, name, pname, med(ms), W * n / mm / 1e9, mm / am, med(bs), mm / bm, med(cs), cm / mm), flush=True)
        del words, rows, sel, high, plain, today_rows, today_sel
    del cols, mapq
    torch.cuda.empty_cache()
