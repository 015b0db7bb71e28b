#!/usr/bin/env python3
"""Selected-elements segmented flagstat at full size: `python3 tests/perf/segments_where_sweep.py [--flags N] [--rounds R] [--reps K]
[--today-flags N] [--oracle-flags N] [--quick]` -- a device-resident uint16 array (torch memory, NA12878-like, filled on the
device), a random mask over it as torch.bool (1 B per flag) and the same mask as an LSB-first bitmap (0.125 B per flag), timed
with hipEvents after warm-up.  Mask densities 0.01, 0.5 and 0.99; the layouts of tests/perf/segments_sweep.py:

  P1  one segment over the whole array
  P2  512,000-flag segments (the column store's block)
  P3  random lengths 0..2000 (mean 1000)

Per density and layout, ALTERNATING in one run:

  (k) FLAGSTATS_hip_device_u16                  K1 over the whole array
  (w) FLAGSTATS_hip_device_u16_where            flagstat_count_where<1> over the whole array under the bitmap
  (a) FLAGSTATS_hip_device_u16_segments         the unfiltered segmented kernel on the same layout
  (b) FLAGSTATS_hip_device_u16_segments_where   the bitmap form, store form, rows and selected (2.125 B per flag)
  (y) the same entry in the byte form of the same mask (3 B per flag)
  (c) what a torch caller does today, over the first --today-flags flags (default 2^30: the limit of torch's mask indexing):
      t[m], a cumulative sum of the mask read at the offsets, segments.count_segments_torch on the compacted copy; beside (b) over
      the same slice

Printed: median ms per call over the rounds with min / max; (w)/(k), (a)/(k), their product + 3 % as the bound, (b)/(k) against
it; (y)/(b); (b)/(a); (c)/(b).  Before anything is timed, in the measured configuration: over the first --oracle-flags flags
(default 2^22) rows and `selected` of both forms equal tests/segments_where_oracle.want exactly; over the whole array the rows sum
to the where kernel's counters and `selected` to its count; over the (c) slice rows and `selected` equal (c)'s.
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
import segments_where_oracle as swo  # noqa: E402
from libflagstats_amd import _lib, device, kernel_id, segments  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--flags", type=int, default=2 ** 32)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--today-flags", type=int, default=2 ** 30)
ap.add_argument("--oracle-flags", type=int, default=2 ** 22)
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()

import torch  # noqa: E402

lib = _lib.lib()
_lib.check(lib.FLAGSTATS_hip_init(0), "init")
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
n = args.flags // 8 * 8
n_today = min(n, args.today_flags)
n_oracle = min(n, args.oracle_flags)
print("segments_where_sweep: %d flags (%.2f GiB), NA12878-like, + a mask as %d bytes and as %d bitmap bytes; rounds %d x reps %d; (c) over "
      "%d flags; oracle over %d flags; K1 code object %s" % (n, 2 * n / 2 ** 30, n, n // 8, args.rounds, args.reps, n_today, n_oracle,
                                                             kernel_id.kernel_id()), flush=True)

t = torch.empty(n, dtype=torch.int16, device="cuda")
device.generate_torch(t, device.GEN_NA12878, seed=11, mask=0)
mask = torch.empty(n, dtype=torch.bool, device="cuda")
bitmap = torch.empty(n // 8, dtype=torch.uint8, device="cuda")
gen = torch.Generator(device="cuda")
weights = (1 << torch.arange(8, device="cuda", dtype=torch.int32))


def make_mask(density, seed):
    gen.manual_seed(seed)
    step = 1 << 26
    for i in range(0, n, step):
        c = min(step, n - i)
        m = torch.rand(c, device="cuda", generator=gen) < density
        mask[i:i + c] = m
        bitmap[i // 8:(i + c) // 8] = (m.view(-1, 8).to(torch.int32) * weights).sum(dim=1).to(torch.uint8)
    torch.cuda.synchronize()


rng = np.random.RandomState(7)
lengths = rng.randint(0, 2001, n // 1000 + 1000)
o3 = np.concatenate([[0], np.cumsum(lengths)])
LAYOUTS = (("P1 one segment", np.array([0, n], dtype=np.int64)),
           ("P2 512,000-flag blocks", np.append(np.arange(0, n, 512_000, dtype=np.int64), n)),
           ("P3 random lengths, mean 1000", np.append(o3[o3 < n], n).astype(np.int64)))
DENSITIES = (0.01, 0.5, 0.99)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def run_where(count, offs, nseg, sel, sel_bits, rows, cnt, flags=1):
    _lib.check(lib.FLAGSTATS_hip_device_u16_segments_where(t.data_ptr(), count, offs.data_ptr(), nseg, sel.data_ptr(), 0, sel_bits,
                                                           rows.data_ptr(), cnt.data_ptr(), flags, stream),
               "FLAGSTATS_hip_device_u16_segments_where")


def u64(x):
    return x.cpu().numpy().view(np.uint64)


host_t = t[:n_oracle].cpu().numpy().view(np.uint16)
whole = torch.zeros(33, dtype=torch.int64, device="cuda")
k1_out = torch.zeros(32, dtype=torch.int64, device="cuda")
for di, density in enumerate(DENSITIES):
    make_mask(density, 5 + di)
    host_m = mask[:n_oracle].cpu().numpy()
    for name, o in LAYOUTS:
        nseg = o.size - 1
        offs = torch.from_numpy(o).cuda()
        rows = torch.empty((nseg, 32), dtype=torch.int64, device="cuda")
        cnt = torch.empty(nseg, dtype=torch.int64, device="cuda")
        rows8 = torch.empty((nseg, 32), dtype=torch.int64, device="cuda")
        cnt8 = torch.empty(nseg, dtype=torch.int64, device="cuda")
        plain = torch.empty((nseg, 32), dtype=torch.int64, device="cuda")
        o_today = np.unique(np.clip(o, 0, n_today)) if n_today < n else o
        offs_today = torch.from_numpy(o_today).cuda()
        nseg_today = o_today.size - 1
        o_small = np.unique(np.clip(o, 0, n_oracle))
        offs_small = torch.from_numpy(o_small).cuda()
        ts, ms = t[:n_today], mask[:n_today]

        def k1():
            _lib.check(lib.FLAGSTATS_hip_device_u16(t.data_ptr(), n, k1_out.data_ptr(), stream), "FLAGSTATS_hip_device_u16")

        def where():
            _lib.check(lib.FLAGSTATS_hip_device_u16_where(t.data_ptr(), n, bitmap.data_ptr(), 0, 1, whole.data_ptr(), whole.data_ptr() + 256,
                                                          1, stream), "FLAGSTATS_hip_device_u16_where")

        def unfiltered():
            _lib.check(lib.FLAGSTATS_hip_device_u16_segments(t.data_ptr(), n, offs.data_ptr(), nseg, plain.data_ptr(), 1, stream),
                       "FLAGSTATS_hip_device_u16_segments")

        def bits():
            run_where(n, offs, nseg, bitmap, 1, rows, cnt)

        def bytes_():
            run_where(n, offs, nseg, mask, 8, rows8, cnt8)

        def part():
            run_where(n_today, offs_today, nseg_today, bitmap, 1, rows[:nseg_today], cnt[:nseg_today])

        def today():
            pre = torch.zeros(n_today + 1, dtype=torch.int64, device=ts.device)
            torch.cumsum(ms, 0, out=pre[1:])
            compact = pre[offs_today]
            return segments.count_segments_torch(ts[ms], compact), compact[1:] - compact[:-1]

        # parity of what is measured: the oracle over a prefix (both forms), the where kernel over everything, (c) over its slice
        ns = o_small.size - 1
        want_rows, want_sel = swo.want(host_t, o_small, host_m)
        for sel, sel_bits in ((bitmap, 1), (mask, 8)):
            run_where(n_oracle, offs_small, ns, sel, sel_bits, rows[:ns], cnt[:ns])
            torch.cuda.synchronize()
            assert np.array_equal(u64(rows[:ns]), want_rows) and np.array_equal(u64(cnt[:ns]), want_sel), (density, name, sel_bits, "oracle")
        part()
        r_today, s_today = today()
        torch.cuda.synchronize()
        assert torch.equal(rows[:nseg_today], r_today) and torch.equal(cnt[:nseg_today], s_today), (density, name, "today")
        del r_today, s_today
        bits(), bytes_(), where(), unfiltered(), k1()
        torch.cuda.synchronize()
        assert torch.equal(rows.sum(dim=0), whole[:32]) and int(cnt.sum()) == int(whole[32]), (density, name, "where kernel")
        assert torch.equal(rows, rows8) and torch.equal(cnt, cnt8), (density, name, "byte form")
        print("density %.2f %-30s nseg %9d: %d of %d flags selected; rows and selected equal the oracle's over the first %d flags (both "
              "forms), (c)'s over the first %d, and sum to the where kernel's over all" % (density, name, nseg, int(whole[32]), n, n_oracle,
                                                                                         n_today), flush=True)
        part(), today()
        torch.cuda.synchronize()
        if args.quick:
            continue
        acc = {key: [] for key in "kwabypc"}
        for _ in range(args.rounds):
            for key, fn in (("k", k1), ("w", where), ("a", unfiltered), ("b", bits), ("y", bytes_), ("p", part)):
                acc[key].append(timed(fn, args.reps))
            acc["c"].append(timed(today, max(1, args.reps // 5)))
        med = {key: statistics.median(v) for key, v in acc.items()}
        ratio = lambda x, y: [p / q for p, q in zip(acc[x], acc[y])]  # noqa: E731
        bound = med["w"] / med["k"] * med["a"] / med["k"] * 1.03
        print("density %.2f %-30s: (k) K1 %.4f ms [%.4f .. %.4f]  (w) where<1> %.4f ms [%.4f .. %.4f]  (a) segments %.4f ms [%.4f .. %.4f]  "
              "(b) bitmap %.4f ms [%.4f .. %.4f] = %.3f TB/s at 2.125 B/flag  (y) bytes %.4f ms [%.4f .. %.4f] = %.3f TB/s at 3 B/flag   "
              "(w)/(k) %.4f  (a)/(k) %.4f  bound (w)/(k) x (a)/(k) x 1.03 = %.4f  (b)/(k) %.4f [%.4f .. %.4f]  (y)/(b) %.4f [%.4f .. %.4f]  "
              "(b)/(a) %.4f   over %d flags: (b) %.4f ms, (c) t[m] + cumsum at the offsets + count_segments_torch %.4f ms  (c)/(b) %.2f x"
              % (density, name, med["k"], min(acc["k"]), max(acc["k"]), med["w"], min(acc["w"]), max(acc["w"]), med["a"], min(acc["a"]),
                 max(acc["a"]), med["b"], min(acc["b"]), max(acc["b"]), 2.125 * n / med["b"] / 1e9, med["y"], min(acc["y"]), max(acc["y"]),
                 3 * n / med["y"] / 1e9, med["w"] / med["k"], med["a"] / med["k"], bound, med["b"] / med["k"], min(ratio("b", "k")),
                 max(ratio("b", "k")), med["y"] / med["b"], min(ratio("y", "b")), max(ratio("y", "b")), med["b"] / med["a"], n_today, med["p"],
                 med["c"], med["c"] / med["p"]), flush=True)
        del rows, cnt, rows8, cnt8, plain, offs
        torch.cuda.empty_cache()
