#!/usr/bin/env python3
"""Filtered segmented flagstat at full size: `python3 tests/perf/segments_filter_sweep.py [--flags N] [--rounds R] [--reps K]
[--today-flags N] [--host-flags N] [--oracle-flags N] [--quick]` -- a device-resident uint16 array (torch memory, NA12878-like,
filled on the device) and a uint8 MAPQ column beside it (three quarters 60, the rest uniform in 0..59), timed with hipEvents
after warm-up.  The layouts of tests/perf/segments_sweep.py:

  P1  one segment over the whole array
  P2  512,000-flag segments (the column store's block)
  P3  random lengths 0..2000 (mean 1000)

under the predicates of tests/perf/filter_sweep.py: -F 0x904, -f 0x2 -F 0x904 (2 B per flag) and -F 0x904 -q 30 (3 B per flag).
Per layout and predicate, ALTERNATING in one run:

  (a) FLAGSTATS_hip_device_u16_segments          the unfiltered segmented kernel on the same layout
  (b) FLAGSTATS_hip_device_u16_segments_filter   store form, rows and selected
  (c) what a torch caller does today, over the first --today-flags flags (default 2^30): the torch expression for the mask,
      torch.where(mask, t, 0), segments.count_segments_torch on the zeroed copy and a prefix-sum difference of the mask for
      `selected`; beside (b) over the same slice

Printed: median ms per call over the rounds with min / max, (b) / (a), and (c) / (b).  Before anything is timed, in the measured
configuration: over the first --oracle-flags flags (default 2^22) rows and `selected` equal tests/segments_filter_oracle.want
exactly; over the whole array the rows sum to FLAGSTATS_hip_device_u16_filter's counters and `selected` to its count; over the
(c) slice rows and `selected` equal (c)'s.
--host-flags N (default 2^30; 0: off): FLAGSTATS_hip_u16_x64_segments_filter over N flags in page-locked memory at the default
chunk size, P2 and P3, host clock around each call, alternating with FLAGSTATS_hip_u16_x64_segments over the same array.
--quick: one call of each after one warm-up (for rocprofv3 runs: --kernel-trace --stats, or --pmc on its own)."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import segments_filter_oracle as sfo  # noqa: E402
from libflagstats_amd import _lib, device, kernel_id, segments  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--flags", type=int, default=2 ** 32)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--today-flags", type=int, default=2 ** 30)
ap.add_argument("--host-flags", type=int, default=2 ** 30)
ap.add_argument("--oracle-flags", type=int, default=2 ** 22)
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()

import torch  # noqa: E402

lib = _lib.lib()
_lib.check(lib.FLAGSTATS_hip_init(0), "init")
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
n = args.flags
n_today = min(n, args.today_flags)
n_oracle = min(n, args.oracle_flags)
print("segments_filter_sweep: %d flags (%.2f GiB) + %d MAPQ bytes, NA12878-like; rounds %d x reps %d; (c) over %d flags; oracle over %d "
      "flags; K1 code object %s" % (n, 2 * n / 2 ** 30, n, args.rounds, args.reps, n_today, n_oracle, kernel_id.kernel_id()), flush=True)

t = torch.empty(n, dtype=torch.int16, device="cuda")
device.generate_torch(t, device.GEN_NA12878, seed=11, mask=0)
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

rng = np.random.RandomState(7)
lengths = rng.randint(0, 2001, n // 1000 + 1000)
o3 = np.concatenate([[0], np.cumsum(lengths)])
LAYOUTS = (("P1 one segment", np.array([0, n], dtype=np.int64)),
           ("P2 512,000-flag blocks", np.append(np.arange(0, n, 512_000, dtype=np.int64), n)),
           ("P3 random lengths, mean 1000", np.append(o3[o3 < n], n).astype(np.int64)))
CASES = (("-F 0x904", 0, 0x904, 0), ("-f 0x2 -F 0x904", 0x2, 0x904, 0), ("-F 0x904 -q 30", 0, 0x904, 30))


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def run_filter(count, offs, nseg, require, exclude, min_mapq, rows, sel, flags=1):
    _lib.check(lib.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), count, offs.data_ptr(), nseg, require, exclude,
                                                            mapq.data_ptr() if min_mapq else None, min_mapq, rows.data_ptr(),
                                                            sel.data_ptr(), flags, stream), "FLAGSTATS_hip_device_u16_segments_filter")


def u64(x):
    return x.cpu().numpy().view(np.uint64)


host_t = t[:n_oracle].cpu().numpy().view(np.uint16)
host_q = mapq[:n_oracle].cpu().numpy()
whole = torch.zeros(33, dtype=torch.int64, device="cuda")
for name, o in LAYOUTS:
    nseg = o.size - 1
    offs = torch.from_numpy(o).cuda()
    rows = torch.empty((nseg, 32), dtype=torch.int64, device="cuda")
    sel = torch.empty(nseg, dtype=torch.int64, device="cuda")
    plain = torch.empty((nseg, 32), dtype=torch.int64, device="cuda")
    # the layout cut to the (c) slice and to the oracle's slice
    o_today = np.unique(np.clip(o, 0, n_today)) if n_today < n else o
    offs_today = torch.from_numpy(o_today).cuda()
    nseg_today = o_today.size - 1
    o_small = np.unique(np.clip(o, 0, n_oracle))
    offs_small = torch.from_numpy(o_small).cuda()

    def unfiltered():
        _lib.check(lib.FLAGSTATS_hip_device_u16_segments(t.data_ptr(), n, offs.data_ptr(), nseg, plain.data_ptr(), 1, stream),
                   "FLAGSTATS_hip_device_u16_segments")

    for text, require, exclude, min_mapq in CASES:
        ts, qs = t[:n_today], mapq[:n_today]

        def today():
            m = (ts & exclude) == 0
            if require:
                m = m & ((ts & require) == require)
            if min_mapq:
                m = m & (qs >= min_mapq)
            z = torch.where(m, ts, torch.zeros((), dtype=ts.dtype, device=ts.device))
            r = segments.count_segments_torch(z, offs_today)
            pre = torch.zeros(n_today + 1, dtype=torch.int64, device=ts.device)
            torch.cumsum(m, 0, out=pre[1:])
            return r, pre[offs_today[1:]] - pre[offs_today[:-1]]

        # parity of what is measured: the oracle over a prefix, the filter kernel over everything, (c) over its slice
        ns = o_small.size - 1
        run_filter(n_oracle, offs_small, ns, require, exclude, min_mapq, rows[:ns], sel[:ns])
        torch.cuda.synchronize()
        want_rows, want_sel = sfo.want(host_t, o_small, require, exclude, host_q, min_mapq)
        assert np.array_equal(u64(rows[:ns]), want_rows) and np.array_equal(u64(sel[:ns]), want_sel), (name, text, "oracle")
        run_filter(n_today, offs_today, nseg_today, require, exclude, min_mapq, rows[:nseg_today], sel[:nseg_today])
        r_today, s_today = today()
        torch.cuda.synchronize()
        assert torch.equal(rows[:nseg_today], r_today) and torch.equal(sel[:nseg_today], s_today), (name, text, "today")
        del r_today, s_today
        run_filter(n, offs, nseg, require, exclude, min_mapq, rows, sel)
        _lib.check(lib.FLAGSTATS_hip_device_u16_filter(t.data_ptr(), n, require, exclude, mapq.data_ptr() if min_mapq else None, min_mapq,
                                                       whole.data_ptr(), whole.data_ptr() + 256, 1, stream), "FLAGSTATS_hip_device_u16_filter")
        torch.cuda.synchronize()
        assert torch.equal(rows.sum(dim=0), whole[:32]) and int(sel.sum()) == int(whole[32]), (name, text, "filter kernel")
        print("%-30s %-16s nseg %9d: %d of %d flags pass; rows and selected equal the oracle's over the first %d flags, (c)'s over the "
              "first %d, and sum to the filter kernel's over all" % (name, text, nseg, int(whole[32]), n, n_oracle, n_today), flush=True)

        def full():
            run_filter(n, offs, nseg, require, exclude, min_mapq, rows, sel)

        def part():
            run_filter(n_today, offs_today, nseg_today, require, exclude, min_mapq, rows[:nseg_today], sel[:nseg_today])

        full()
        unfiltered()
        part()
        today()
        torch.cuda.synchronize()
        if args.quick:
            continue
        us, fs, ps, cs = [], [], [], []
        for _ in range(args.rounds):
            us.append(timed(unfiltered, args.reps))
            fs.append(timed(full, args.reps))
            ps.append(timed(part, args.reps))
            cs.append(timed(today, max(1, args.reps // 5)))
        um, fm, pm, cm = (statistics.median(x) for x in (us, fs, ps, cs))
        per_flag = 3.0 if min_mapq else 2.0
        print("%-30s %-16s: (a) segments %.4f ms [%.4f .. %.4f] = %.3f TB/s   (b) filtered %.4f ms [%.4f .. %.4f] = %.3f TB/s at %.0f B/flag   "
              "(b)/(a) time %.4f [%.4f .. %.4f]   over %d flags: (b) %.4f ms, (c) torch mask + where + count_segments_torch + prefix sums "
              "%.4f ms   (c)/(b) %.2f x"
              % (name, text, um, min(us), max(us), 2 * n / um / 1e9, fm, min(fs), max(fs), per_flag * n / fm / 1e9, per_flag, fm / um,
                 min(f / u for f, u in zip(fs, us)), max(f / u for f, u in zip(fs, us)), n_today, pm, cm, cm / pm), flush=True)
    del rows, sel, plain, offs
    torch.cuda.empty_cache()

# ---- the host-array form beside the unfiltered host form over the same array
if args.host_flags and not args.quick:
    hn = min(args.host_flags, n)
    hp = lib.FLAGSTATS_hip_host_alloc(2 * hn)
    hq = lib.FLAGSTATS_hip_host_alloc(hn)
    assert hp and hq, "host_alloc"
    torch.cuda.synchronize()
    _lib.check(lib.FLAGSTATS_hip_memcpy_d2h(hp, t.data_ptr(), 2 * hn), "d2h")
    _lib.check(lib.FLAGSTATS_hip_memcpy_d2h(hq, mapq.data_ptr(), hn), "d2h")
    print("host form: %d flags (%.2f GiB) + MAPQ in page-locked memory, chunk_flags %d" % (hn, 2 * hn / 2 ** 30, lib.FLAGSTATS_hip_get(b"chunk_flags")),
          flush=True)
    oh = np.concatenate([[0], np.cumsum(rng.randint(0, 2001, hn // 1000 + 1000))])
    for name, o in (("H2 512,000-flag blocks", np.append(np.arange(0, hn, 512_000, dtype=np.int64), hn)),
                    ("H3 random lengths, mean 1000", np.append(oh[oh < hn], hn))):
        o = o.astype(np.uint64)
        nseg = o.size - 1
        rows = np.zeros((nseg, 32), dtype=np.uint64)
        sel = np.zeros(nseg, dtype=np.uint64)
        plain = np.zeros((nseg, 32), dtype=np.uint64)
        d_o = torch.from_numpy(o.astype(np.int64)).cuda()
        d_rows = torch.empty((nseg, 32), dtype=torch.int64, device="cuda")
        d_sel = torch.empty(nseg, dtype=torch.int64, device="cuda")

        def host_plain():
            _lib.check(lib.FLAGSTATS_hip_u16_x64_segments(hp, hn, o.ctypes.data, nseg, plain.ctypes.data, 1), "FLAGSTATS_hip_u16_x64_segments")

        for text, require, exclude, min_mapq in CASES:
            def host_filter():
                _lib.check(lib.FLAGSTATS_hip_u16_x64_segments_filter(hp, hn, o.ctypes.data, nseg, require, exclude, hq if min_mapq else None,
                                                                     min_mapq, rows.ctypes.data, sel.ctypes.data, 1),
                           "FLAGSTATS_hip_u16_x64_segments_filter")

            host_filter()
            host_plain()
            run_filter(hn, d_o, nseg, require, exclude, min_mapq, d_rows, d_sel)     # (checked against the oracle above)
            torch.cuda.synchronize()
            assert np.array_equal(rows, u64(d_rows)) and np.array_equal(sel, u64(d_sel)), (name, text, "host form != device form")
            ws, ss = [], []
            for _ in range(args.rounds):
                for fn, acc in ((host_plain, ws), (host_filter, ss)):
                    t0 = time.perf_counter()
                    fn()
                    acc.append((time.perf_counter() - t0) * 1e3)
            wm, sm = statistics.median(ws), statistics.median(ss)
            per_flag = 3 if min_mapq else 2
            print("%-30s %-16s nseg %8d: filtered %.2f ms [%.2f .. %.2f] (%.1f GB/s over %d B/flag)  FLAGSTATS_hip_u16_x64_segments %.2f ms "
                  "[%.2f .. %.2f] (%.1f GB/s)  time ratio %.3f; rows and selected equal the device form's"
                  % (name, text, nseg, sm, min(ss), max(ss), per_flag * hn / sm / 1e6, per_flag, wm, min(ws), max(ws), 2 * hn / wm / 1e6, sm / wm),
                  flush=True)
    lib.FLAGSTATS_hip_host_free(hp)
    lib.FLAGSTATS_hip_host_free(hq)
