#!/usr/bin/env python3
"""Selected-elements segmented flagstat on int32 / int64 columns at full size: `python3 tests/perf/segments_wide_where_sweep.py
[--bytes N] [--rounds R] [--reps K] [--buffers B] [--quick]` -- per width, B (default 2) device-resident columns of N bytes (default
8 GiB: every pass reads 32 times the 256 MiB cache) of int32 / int64 elements whose low halves are NA12878-like flags (filled on
the device), under masks of density 0.01, 0.5 and 0.99 held three ways: an LSB-first bitmap at bit offset 0 (plain), the same mask
at bit offset 3 (funnelled) and one byte per element; timed with hipEvents after warm-up; the calls of a timed window rotate over
the B columns.  Layouts: one segment; blocks of 512,000 elements; segments of ~1,000 elements (uniform in 500..1500).  Per layout
and density everything is timed in the same run, ALTERNATING:

  this kernel  fsk_launch_segments_wide_where: bitmap plain, bitmap funnelled, bytes (store form)
  (a) fsk_launch_segments_wide on the same layout (the unmasked segmented kernel, store form)
  (b) fsk_launch_wide_where over the whole column under the same bitmap / the same bytes (the masked kernel without segments)
  (c) fsk_launch_segments_wide_filter under -q 1 with the same byte column as its MAPQ column (same rows and counts, other `high`)

Printed per width, layout and density: median ms per call over the rounds with the spread (min .. max), the ratios in time and
the two yardsticks: bitmap form <= (a) x (W + 1/8) / W x 1.03 (the ratio of bytes moved, plus 3 %) on the two long layouts, byte
form <= 1.03 x (c).  Before anything is timed the rows, counts and masks of the three forms of this kernel are compared with each
other, their sums with (b)'s counters, count and mask, and rows and counts with (c)'s, on every column.  --quick: parity only."""
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
DENSITIES = (0.01, 0.5, 0.99)
FUNNEL_OFFSET = 3
print("segments_wide_where_sweep: %d bytes (%.2f GiB) per column, %d columns per width, NA12878-like low halves; rounds %d x reps %d; wide "
      "grid %d, segments grid %d, min_units %d; K1 code object %s"
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

    return (("one segment", True, csr(torch.zeros(0, dtype=torch.int64, device="cuda"))),
            ("512,000-element blocks", True, csr(torch.arange(512_000, n, 512_000, dtype=torch.int64, device="cuda"))),
            ("~1,000-element segments", False, csr(short)))


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
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    the_layouts = layouts(n)

    for density in DENSITIES:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7)
        byte_col = torch.empty(n, dtype=torch.uint8, device="cuda")
        for i in range(0, n, step):
            byte_col[i:i + step] = (torch.rand(min(step, n - i), device="cuda", generator=gen) < density).to(torch.uint8)
        bits0, bits3 = packed(byte_col, 0), packed(byte_col, FUNNEL_OFFSET)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        forms = (("bitmap", bits0, 0, 1), ("bitmap, funnelled", bits3, FUNNEL_OFFSET, 1), ("bytes", byte_col, 0, 8))

        for name, long_layout, off in the_layouts:
            nseg = off.numel() - 1
            words = [torch.zeros(nseg * 34, dtype=torch.int64, device="cuda") for _ in forms]
            plain = torch.zeros(nseg * 33, dtype=torch.int64, device="cuda")
            filt = torch.zeros(nseg * 34, dtype=torch.int64, device="cuda")

            def unmasked(i):
                t = cols[i % len(cols)]
                check_hip(lib.fsk_launch_segments_wide(t.data_ptr(), W, 0, n, off.data_ptr(), nseg, plain.data_ptr(),
                                                       plain.data_ptr() + nseg * 256, 1, seg_grid, stream), "fsk_launch_segments_wide")

            def mine_of(k):
                _, s, so, sb = forms[k]
                w = words[k]

                def mine(i):
                    t = cols[i % len(cols)]
                    check_hip(lib.fsk_launch_segments_wide_where(t.data_ptr(), W, s.data_ptr(), so, sb, 0, n, off.data_ptr(), nseg, w.data_ptr(),
                                                                 w.data_ptr() + nseg * 256, w.data_ptr() + nseg * 264, 1, seg_grid, stream),
                              "fsk_launch_segments_wide_where")
                return mine

            def whole_of(k):
                _, s, so, sb = forms[k]

                def whole_column(i):
                    t = cols[i % len(cols)]
                    check_hip(lib.fsk_launch_wide_where(t.data_ptr(), n, W, s.data_ptr(), so, sb, whole.data_ptr(), whole.data_ptr() + 256,
                                                        whole.data_ptr() + 264, 1, wide_grid, stream), "fsk_launch_wide_where")
                return whole_column

            def filtered(i):
                t = cols[i % len(cols)]
                check_hip(lib.fsk_launch_segments_wide_filter(t.data_ptr(), W, byte_col.data_ptr(), 0, n, off.data_ptr(), nseg, 0, 0, 1,
                                                              filt.data_ptr(), filt.data_ptr() + nseg * 256, filt.data_ptr() + nseg * 264, 1,
                                                              seg_grid, stream), "fsk_launch_segments_wide_filter")

            mine = [mine_of(k) for k in range(3)]
            wholes = [whole_of(0), whole_of(2)]
            # parity of what is measured, on every column
            for b in range(len(cols)):
                for f in mine:
                    f(b)
                filtered(b)
                torch.cuda.synchronize()
                assert torch.equal(words[0], words[1]) and torch.equal(words[0], words[2]), "the three forms of the same mask differ"
                assert torch.equal(words[0][:nseg * 33], filt[:nseg * 33]), "rows or counts differ from segments_wide_filter under -q 1"
                rows, sel, high = words[0][:nseg * 32].view(nseg, 32), words[0][nseg * 32:nseg * 33], words[0][nseg * 33:]
                for wc in wholes:
                    wc(b)
                    torch.cuda.synchronize()
                    assert torch.equal(rows.sum(dim=0), whole[:32]) and int(sel.sum()) == int(whole[32]), "rows do not sum to wide_where's"
                    assert not bool(high.any()) and int(whole[33]) == 0 and 0 < int(whole[32]) < n, "masks must be 0, a part must be selected"
            print("W = %d, density %.2f, %s: %d segments; the three forms agree, sum to fsk_launch_wide_where's on every column and equal "
                  "fsk_launch_segments_wide_filter -q 1 in rows and counts; masks 0" % (W, density, name, nseg), flush=True)
            if args.quick:
                continue
            fns = [unmasked] + mine + wholes + [filtered]
            for fn in fns:                                   # warm-up: every call once more, untimed
                fn(0)
            torch.cuda.synchronize()
            ts = [[] for _ in fns]
            for _ in range(args.rounds):
                for k, fn in enumerate(fns):
                    ts[k].append(timed(fn, args.reps))
            m = [statistics.median(x) for x in ts]
            a, bm, bf, by, wb, wy, c = m
            bound = a * (W + 0.125) / W * 1.03
            print("W = %d, d %.2f, %-26s: (a) segments wide, unmasked %s = %.3f TB/s of elements" % (W, density, name, med(ts[0]), W * n / a / 1e9),
                  flush=True)
            for label, k, mk, wk in (("bitmap", 1, bm, wb), ("bitmap, funnelled", 2, bf, wb)):
                verdict = ("yardstick (a) x %.4f x 1.03 = %.4f ms: %s" % ((W + 0.125) / W, bound, "met" if mk <= bound else "MISSED")) if long_layout \
                    else "(no yardstick on this layout)"
                print("W = %d, d %.2f, %-26s: %-18s %s = %.3f TB/s of elements + bits   / (a) %.4f   (b) wide_where, whole column %s   / (b) "
                      "%.4f   %s" % (W, density, name, label, med(ts[k]), (W + 0.125) * n / mk / 1e9, mk / a, med(ts[4]), mk / wk, verdict),
                      flush=True)
            print("W = %d, d %.2f, %-26s: %-18s %s = %.3f TB/s of elements + bytes   / (a) %.4f   (b) wide_where, whole column %s   / (b) %.4f   "
                  "(c) segments_wide_filter -q 1 %s   / (c) %.4f   yardstick 1.03 x (c) = %.4f ms: %s"
                  % (W, density, name, "bytes", med(ts[3]), (W + 1) * n / by / 1e9, by / a, med(ts[5]), by / wy, med(ts[6]), by / c, 1.03 * c,
                     "met" if by <= 1.03 * c else "MISSED"), flush=True)
            del words, plain, filt
        del byte_col, bits0, bits3
        torch.cuda.empty_cache()
    del cols
    torch.cuda.empty_cache()
