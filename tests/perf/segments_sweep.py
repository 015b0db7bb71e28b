#!/usr/bin/env python3
"""Segmented flagstat at full size: `python3 tests/perf/segments_sweep.py [--flags N] [--rounds R] [--reps K] [--units 1,2,4,8]
[--quick]` -- a device-resident uint16 array (torch memory, filled on the device), timed with hipEvents after warm-up, each
layout's segmented calls ALTERNATING with FLAGSTATS_hip_device_u16 (K1) over the same array in the same run:

  P1  one segment over the whole array           gate: <= 1.03 x the time of FLAGSTATS_hip_device_u16
  P2  512,000-flag segments (the column store's block)   gate: >= 0.85 x K1's input rate
  P3  random lengths 0..2000 (mean 1000)                  reported: rate over input + output bytes, target 50 % of 8 TB/s

Printed per layout and form (store: `flags` bit 0, with its memset; +=: atomics only): median ms per call over the rounds, the
input rate (array bytes) and the input + output rate (array + offsets + nseg * 256 counter bytes).
--host-flags N (default 2^30; 0: off): the HOST-array form FLAGSTATS_hip_u16_x64_segments over N flags in page-locked memory at
the default chunk size (32 Mi flags), 512,000-flag blocks and random lengths of mean 1,000, host clock around each call, alternating
with FLAGSTATS_u16_x64 over the same array (the same bytes cross the bus); --host-only skips the device layouts.  --units sweeps the
smallest run of whole 4096-flag units inside one segment that goes through K1's carry-save chain (fsk_set_segments_policy).
--quick: one call per layout and form after one warm-up (for rocprofv3 runs: --kernel-trace --stats, or --pmc on its own)."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from libflagstats_amd import _lib, device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--flags", type=int, default=2 ** 32)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--units", default="")
ap.add_argument("--quick", action="store_true")
ap.add_argument("--host-flags", type=int, default=2 ** 30)
ap.add_argument("--host-only", action="store_true")
args = ap.parse_args()

import torch  # noqa: E402

lib = _lib.lib()
_lib.check(lib.FLAGSTATS_hip_init(0), "init")
lib.fsk_segments_policy.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
lib.fsk_set_segments_policy.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
mu, bpc = ctypes.c_uint32(), ctypes.c_uint32()
lib.fsk_segments_policy(ctypes.byref(mu), ctypes.byref(bpc))
default_units = mu.value

n = args.flags
t = torch.empty(n, dtype=torch.int16, device="cuda")
device.generate_torch(t, device.GEN_NA12878, seed=11, mask=0)
rng = np.random.RandomState(7)
layouts = {
    "P1 one segment": np.array([0, n], dtype=np.int64),
    "P2 512,000-flag blocks": np.append(np.arange(0, n, 512_000, dtype=np.int64), n),
}
lengths = rng.randint(0, 2001, n // 1000 + 1000)
o3 = np.concatenate([[0], np.cumsum(lengths)])
layouts["P3 random lengths, mean 1000"] = np.append(o3[o3 < n], n).astype(np.int64)
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
k1_out = torch.zeros(32, dtype=torch.int64, device="cuda")


def k1():
    _lib.check(lib.FLAGSTATS_hip_device_u16(t.data_ptr(), n, k1_out.data_ptr(), stream), "FLAGSTATS_hip_device_u16")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


units = [int(u) for u in args.units.split(",") if u] or [default_units]
print("segments_sweep: %d flags (%.2f GiB), NA12878-like; chain from %s whole units (default %d); rounds %d x reps %d"
      % (n, 2 * n / 2 ** 30, units, default_units, args.rounds, args.reps), flush=True)
for name, o in ({} if args.host_only else layouts).items():
    nseg = o.size - 1
    offs = torch.from_numpy(o).cuda()
    out = torch.empty((nseg, 32), dtype=torch.int64, device="cuda")
    io = 2 * n + 8 * (nseg + 1) + 256 * nseg
    for u in (units if not name.startswith("P1") else units[:1]):
        lib.fsk_set_segments_policy(u, bpc.value)
        for flags, form in ((1, "store"), (0, "+=")):
            def seg():
                _lib.check(lib.FLAGSTATS_hip_device_u16_segments(t.data_ptr(), n, offs.data_ptr(), nseg, out.data_ptr(), flags, stream),
                           "FLAGSTATS_hip_device_u16_segments")
            if args.quick:
                seg()
                torch.cuda.synchronize()
                seg()
                k1()
                torch.cuda.synchronize()
                continue
            seg()
            k1()
            torch.cuda.synchronize()
            ks, ss = [], []
            for _ in range(args.rounds):
                ks.append(timed(k1, args.reps))
                ss.append(timed(seg, args.reps))
            km, sm = statistics.median(ks), statistics.median(ss)
            print("%-30s units>=%-2d %-5s nseg %9d: segments %.4f ms (%.3f TB/s input, %.3f TB/s in+out = %.1f %% of 8)  "
                  "K1 %.4f ms (%.3f TB/s)  time ratio %.4f  rate ratio %.4f  [seg min %.4f max %.4f]"
                  % (name, u, form, nseg, sm, 2 * n / sm / 1e9, io / sm / 1e9, 100 * io / sm / 1e9 / 8, km, 2 * n / km / 1e9,
                     sm / km, km / sm, min(ss), max(ss)), flush=True)
    # parity of the measured configuration: the rows sum to K1's count of the covered range
    lib.fsk_set_segments_policy(default_units, bpc.value)
    _lib.check(lib.FLAGSTATS_hip_device_u16_segments(t.data_ptr(), n, offs.data_ptr(), nseg, out.data_ptr(), 1, stream), "segments")
    k1_out.zero_()
    _lib.check(lib.FLAGSTATS_hip_device_u16(t.data_ptr() + 2 * int(o[0]), int(o[-1] - o[0]), k1_out.data_ptr(), stream), "K1")
    torch.cuda.synchronize()
    assert torch.equal(out.sum(dim=0), k1_out), name
    print("%s: rows sum to K1's counters" % name, flush=True)
    del out, offs
    torch.cuda.empty_cache()

# ---- the host-array form: chunks of the engine's default size, every chunk's launch walks the offsets
if args.host_flags and not args.quick:
    import time
    hn = min(args.host_flags, n)
    hp = lib.FLAGSTATS_hip_host_alloc(2 * hn)
    assert hp, "host_alloc"
    torch.cuda.synchronize()
    _lib.check(lib.FLAGSTATS_hip_memcpy_d2h(hp, t.data_ptr(), 2 * hn), "d2h")
    print("host form: %d flags (%.2f GiB) in page-locked memory, chunk_flags %d" % (hn, 2 * hn / 2 ** 30, lib.FLAGSTATS_hip_get(b"chunk_flags")),
          flush=True)
    lengths = rng.randint(0, 2001, hn // 1000 + 1000)
    oh = np.concatenate([[0], np.cumsum(lengths)])
    host_layouts = {"H2 512,000-flag blocks": np.append(np.arange(0, hn, 512_000, dtype=np.int64), hn),
                    "H3 random lengths, mean 1000": np.append(oh[oh < hn], hn)}
    whole = np.zeros(32, dtype=np.uint64)

    def host_whole():
        whole[:] = 0
        _lib.check(lib.FLAGSTATS_u16_x64(hp, hn, whole.ctypes.data), "FLAGSTATS_u16_x64")

    for name, o in host_layouts.items():
        o = o.astype(np.uint64)
        nseg = o.size - 1
        rows = np.zeros((nseg, 32), dtype=np.uint64)

        def host_seg():
            _lib.check(lib.FLAGSTATS_hip_u16_x64_segments(hp, hn, o.ctypes.data, nseg, rows.ctypes.data, 1),
                       "FLAGSTATS_hip_u16_x64_segments")

        host_seg()
        host_whole()
        ws, ss = [], []
        for _ in range(args.rounds):
            for fn, acc in ((host_whole, ws), (host_seg, ss)):
                t0 = time.perf_counter()
                fn()
                acc.append((time.perf_counter() - t0) * 1e3)
        wm, sm = statistics.median(ws), statistics.median(ss)
        print("%-30s nseg %8d: segments %.2f ms (%.1f GB/s of input)  FLAGSTATS_u16_x64 %.2f ms (%.1f GB/s)  time ratio %.3f"
              "  [seg min %.2f max %.2f]" % (name, nseg, sm, 2 * hn / sm / 1e6, wm, 2 * hn / wm / 1e6, sm / wm, min(ss), max(ss)),
              flush=True)
        assert np.array_equal(rows.sum(axis=0), whole), name
        print("%s: rows sum to FLAGSTATS_u16_x64's counters" % name, flush=True)
    lib.FLAGSTATS_hip_host_free(hp)
