"""GPU: the eight kernels derived from K1's step tree (where, filter, segments, segments_filter, wide, wide_filter, wide_segments,
wide_segments_filter) under a randomized sweep, one after another over the engine's staging slots, and from several threads at
once.  Cases, reference and the poisoned input / output images come from tests/derived_plan.py (checked on the CPU by
tests/test_derived_plan_host.py); every comparison is exact, and every call is one the header documents as legal.

To run one case of the sweep again: ``derived_plan.plan(SEED, index + 1)[index]`` -- a failure names the index and the drawn
parameters."""
import ctypes
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import derived_plan as dp  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 20261019     # tests/test_derived_plan_host.py checks this plan's coverage

# arguments of every entry, by name: A array, N n, W elem_bytes, S / SO / SB selection, its offset and encoding, R / X / Q / MQ
# require, exclude, MAPQ column, min_mapq, O / NS offsets and nseg, OUT / SEL / HIGH outputs, Z a zero (the launchers' `base`)
PUBLIC = {"where": "A N S SO SB OUT SEL MODE", "filter": "A N R X Q MQ OUT SEL MODE", "segments": "A N O NS OUT MODE",
          "segments_filter": "A N O NS R X Q MQ OUT SEL MODE", "wide": "A N W OUT HIGH MODE", "wide_filter": "A N W R X Q MQ OUT SEL HIGH MODE",
          "wide_segments": "A N W O NS OUT HIGH MODE", "wide_segments_filter": "A N W O NS R X Q MQ OUT SEL HIGH MODE"}
LAUNCHER = {"where": ("fsk_launch_where", "A N S SO SB OUT SEL MODE GRID"), "filter": ("fsk_launch_filter", "A N R X Q MQ OUT SEL MODE GRID"),
            "segments": ("fsk_launch_segments", "A Z N O NS OUT MODE GRID"),
            "segments_filter": ("fsk_launch_segments_filter", "A Q Z N O NS R X MQ OUT SEL MODE GRID"),
            "wide": ("fsk_launch_wide", "A N W OUT HIGH MODE GRID"), "wide_filter": ("fsk_launch_wide_filter", "A N W R X Q MQ OUT SEL HIGH MODE GRID"),
            "wide_segments": ("fsk_launch_segments_wide", "A W Z N O NS OUT HIGH MODE GRID"),
            "wide_segments_filter": ("fsk_launch_segments_wide_filter", "A W Q Z N O NS R X MQ OUT SEL HIGH MODE GRID")}
STEM = {"where": "u16_where", "filter": "u16_filter", "segments": "u16_segments", "segments_filter": "u16_segments_filter", "wide": "wide",
        "wide_filter": "wide_filter", "wide_segments": "wide_segments", "wide_segments_filter": "wide_segments_filter"}
HOST = {"where": "FLAGSTATS_hip_u16_x64_where", "filter": "FLAGSTATS_hip_u16_x64_filter", "segments": "FLAGSTATS_hip_u16_x64_segments",
        "segments_filter": "FLAGSTATS_hip_u16_x64_segments_filter", "wide": "FLAGSTATS_hip_wide_x64", "wide_filter": "FLAGSTATS_hip_wide_x64_filter",
        "wide_segments": "FLAGSTATS_hip_wide_x64_segments", "wide_segments_filter": "FLAGSTATS_hip_wide_x64_segments_filter"}


def entry_name(case):
    fam, form = case["family"], case["form"]
    if form == "launcher":
        return LAUNCHER[fam][0]
    if form == "host":
        return HOST[fam]
    return "FLAGSTATS_hip_device_" + STEM[fam] + ("_sync" if form == "sync" else "")


@pytest.fixture(scope="module")
def lib(hip):
    f = hip.fsk_launch_segments       # the one launcher _lib.lib() attaches no prototype to
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                  ctypes.c_uint32, ctypes.c_void_p]
    hip.fsk_segments_policy.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    hip.fsk_segments_policy.restype = None
    hip.fsk_set_segments_policy.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    hip.fsk_set_segments_policy.restype = None
    return hip


def get_policy(hip):
    mu, bpc = ctypes.c_uint32(), ctypes.c_uint32()
    hip.fsk_segments_policy(ctypes.byref(mu), ctypes.byref(bpc))
    return mu.value, bpc.value


def err(hip):
    return hip.FLAGSTATS_hip_last_error().decode(errors="replace")


def host_at_16(image):
    """(owner, address): a copy of the byte image in host memory, at a 16-byte boundary"""
    buf = np.empty(image.size + 16, dtype=np.uint8)
    off = -buf.ctypes.data % 16
    view = buf[off:off + image.size]
    view[:] = image
    return buf, view.ctypes.data


def device_at_16(image):
    import torch
    t = torch.from_numpy(image).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr()


class Call:
    """one case made ready: its inputs in poisoned slabs where the form wants them (device memory, or host memory for the host form),
    and the entry's argument list but for the outputs"""

    def __init__(self, case):
        self.case = case
        self.keep = []
        form = case["form"]
        put = host_at_16 if form == "host" else device_at_16
        a = {"N": case["n"], "W": case["W"], "Z": 0, "R": case["require"], "X": case["exclude"], "MQ": case["min_mapq"], "NS": case["nseg"],
             "MODE": case["mode"], "GRID": case["grid"], "S": None, "SO": case["sel_offset"], "SB": 1 if case["kind"] == "where_bitmap" else 8,
             "Q": None, "O": None}
        img, at = dp.array_image(case)
        owner, base = put(img)
        self.keep.append(owner)
        a["A"] = base + at
        assert a["A"] % 16 == case["phase"]
        if case["mapq"] is not None and not case["mapq_null"]:
            img, at = dp.bytes_image(case["mapq"], case["mapq_align"])
            owner, base = put(img)
            self.keep.append(owner)
            a["Q"] = base + at
        if case["kind"] == "where_bytes":
            img, at = dp.bytes_image(case["mask"].astype(np.uint8) * np.uint8(1 + case["n"] % 255), case["sel_align"])
            owner, base = put(img)
            self.keep.append(owner)
            a["S"] = base + at
        elif case["kind"] == "where_bitmap":
            img, at, back = dp.bitmap_image(case)
            owner, base = put(img)
            self.keep.append(owner)
            a["S"] = base + at - back
        if case["offsets"] is not None:
            if form in ("sync", "host"):
                o = np.ascontiguousarray(case["offsets"], dtype=np.uint64)
                self.keep.append(o)
                a["O"] = o.ctypes.data
            else:
                owner, a["O"] = device_at_16(np.ascontiguousarray(case["offsets"], dtype=np.int64))
                self.keep.append(owner)
        self.args = a
        self.device_outputs = form in ("launcher", "device")
        self.outputs = None

    def fresh_outputs(self):
        """prefilled output allocations with their spare rows; their addresses go into the argument list"""
        import torch
        allocs, where = dp.output_layout(self.case)
        if self.device_outputs:
            self.outputs = [torch.from_numpy(w.view(np.int64)).cuda() for w in allocs]
            bases = [t.data_ptr() for t in self.outputs]
        else:
            self.outputs = allocs
            bases = [w.ctypes.data for w in allocs]
        for name, key in (("rows", "OUT"), ("selected", "SEL"), ("high", "HIGH")):
            self.args[key] = bases[where[name][0]] + 8 * where[name][1] if name in where else None

    def __call__(self, hip, stream=None, out=None):
        """the call itself: its return value.  `out`: (d_out, d_selected, d_high) in place of outputs of its own."""
        case, a = self.case, dict(self.args)
        if out is not None:
            a["OUT"], a["SEL"], a["HIGH"] = out
        fam, form = case["family"], case["form"]
        name = entry_name(case)
        order = LAUNCHER[fam][1] if form == "launcher" else PUBLIC[fam]
        argv = [a[k] for k in order.split()]
        if form in ("launcher", "device"):
            argv.append(stream)
        return getattr(hip, name)(*argv)

    def read(self):
        if self.device_outputs:
            return [t.cpu().numpy().view(np.uint64) for t in self.outputs]
        return self.outputs


def mismatch(case, got, want):
    """None, or what differs: the allocation, its first differing words and what they hold"""
    allocs, where = dp.output_layout(case)
    for k, (g, w) in enumerate(zip(got, want)):
        if np.array_equal(g, w):
            continue
        bad = np.nonzero(g != w)[0]
        names = []
        for i in bad[:6]:
            owner = [n for n, (kk, at, count) in where.items() if kk == k and at <= i < at + count]
            names.append((owner[0], int(i - where[owner[0]][1])) if owner else ("spare word", int(i)))
        return {"allocation": k, "differing words": int(bad.size), "first": names, "got": [hex(int(v)) for v in g[bad[:6]]],
                "want": [hex(int(v)) for v in w[bad[:6]]]}
    return None


def run_case(hip, case, ref, stream=None):
    """the case through its form, knobs set and restored around it; None, or what differs from the expected images"""
    import torch
    old_chunk, old_policy = hip.FLAGSTATS_hip_get(b"chunk_flags"), get_policy(hip)
    try:
        if case["chunk_flags"] is not None:
            assert hip.FLAGSTATS_hip_set(b"chunk_flags", case["chunk_flags"]) == 0, err(hip)
        if case["policy"] is not None:
            hip.fsk_set_segments_policy(*case["policy"])
            assert get_policy(hip) == case["policy"]
        call = Call(case)
        call.fresh_outputs()
        torch.cuda.synchronize()
        rc = call(hip, stream)
        assert rc == 0, "case %d: %r %s rc %d: %s" % (case["index"], dp.describe(case), entry_name(case), rc, err(hip))
        torch.cuda.synchronize()
        got = call.read()
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old_chunk)
        hip.fsk_set_segments_policy(*old_policy)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old_chunk and get_policy(hip) == old_policy
    return mismatch(case, got, dp.expected_images(case, ref))


# ------------------------------------------------------------------ 1. the randomized sweep
def test_random_cases_every_derived_family(lib, oracle_mod):
    import torch
    hip = lib
    iters = int(os.environ.get("FLAGSTATS_FUZZ_ITERS_DERIVED", "240"))   # a soak run sets thousands
    cases = dp.plan(SEED, iters)
    assert dp.skip_reasons(cases) == []
    side = torch.cuda.Stream()
    stream = ctypes.c_void_p(side.cuda_stream)
    assert side.cuda_stream != 0
    knobs = (hip.FLAGSTATS_hip_get(b"chunk_flags"), get_policy(hip))
    for case in cases:
        ref = dp.reference(case)
        bad = run_case(hip, case, ref, stream if case["form"] == "device" else None)
        assert bad is None, "case %d: %r %s %r" % (case["index"], dp.describe(case), entry_name(case), bad)   # a str: shown whole
    assert (hip.FLAGSTATS_hip_get(b"chunk_flags"), get_policy(hip)) == knobs


# ------------------------------------------------------------------ 2. the kinds one after another over the two staging slots
CHUNK_WALK = (65544, 8192, 1000, 8)     # ... and 65544 again


def widened(low, dtype, rng, every):
    """low (uint16) as dtype with random bits above bit 15 (the sign bit among them) on one element in `every`"""
    W = np.dtype(dtype).itemsize
    hi = (rng.randint(0, 1 << 16, low.size).astype(np.uint64) << np.uint64(16)) | (rng.randint(0, 1 << 32, low.size).astype(np.uint64) << np.uint64(32))
    u = low.astype(np.uint64) | np.where(rng.randint(0, every, low.size) == 0, hi, np.uint64(0))
    return u.astype(dp.UNSIGNED[W]).view(dtype)


def interleaved_round(rng):
    """the ten derived calls of one round, in order (the K1 calls around them are made by the test): sizes chosen so that the calls
    at positions 0, 4 and 8 of a round, which never meet chunk_flags 8 in the three rounds, are the large ones"""
    u16 = lambda n: rng.randint(0, 65536, n).astype(np.uint16)  # noqa: E731
    q = lambda n: rng.randint(0, 256, n).astype(np.uint8)  # noqa: E731
    cuts = lambda n, first, k: np.concatenate([[first], np.sort(rng.randint(first, n - 3, k)), [n - 3]])  # noqa: E731
    F = "host"
    n = 3001
    calls = [dp.fixed_case("where_bitmap", F, u16(n), 3, mask=rng.randint(0, 2, n), sel_offset=5, phase=2, sel_align=3)]
    n = 1203
    calls.append(dp.fixed_case("wide", F, widened(u16(n), np.int64, rng, 300), 1, phase=8, high_at="apart"))
    n = 4099
    calls.append(dp.fixed_case("filter", F, u16(n), 0, require=1, exclude=0x904, mapq=q(n), min_mapq=30, mapq_align=1))
    n = 150_001
    calls.append(dp.fixed_case("wide_filter", F, widened(u16(n), np.uint32, rng, 5000), 2, exclude=0x704, mapq=q(n), min_mapq=20, phase=4,
                               mapq_align=7, selected_at="apart"))
    n = 2500
    calls.append(dp.fixed_case("segments", F, u16(n), 3, offsets=cuts(n, 7, 9)))
    n = 3777
    calls.append(dp.fixed_case("segments_filter", F, u16(n), 1, require=2, exclude=0x100, mapq=q(n), min_mapq=100, offsets=cuts(n, 0, 30),
                               mapq_align=5))
    n = 1999
    calls.append(dp.fixed_case("wide_segments", F, widened(u16(n), np.int32, rng, 100), 0, offsets=cuts(n, 1, 5), phase=12))
    n = 120_003
    calls.append(dp.fixed_case("wide_segments_filter", F, widened(u16(n), np.uint64, rng, 9000), 3, require=0x40, exclude=0x800, mapq=q(n),
                               min_mapq=1, offsets=cuts(n, 11, 16), mapq_align=9, high_at="apart"))
    n = 100
    calls.append(dp.fixed_case("where_bytes", F, u16(n), 2, mask=rng.randint(0, 3, n) == 0, sel_align=15, selected_at="apart"))
    return calls


def test_entry_kinds_interleaved_over_the_staging_slots(lib, oracle_mod):
    hip = lib
    rng = np.random.RandomState(77)
    derived = interleaved_round(rng)
    refs = [dp.reference(c) for c in derived]
    for c, r in zip(derived, refs):
        assert 100 <= c["n"] <= 200_000 and r["selected"].any() and (c["kind"] not in dp.WIDE or r["high"].any())
    first, last = rng.randint(0, 65536, 200_000).astype(np.uint16), rng.randint(0, 65536, 5000).astype(np.uint16)
    k1 = [(first, oracle_mod.flagstat_c(first)), (last, oracle_mod.flagstat_c(last))]
    old_chunk, old_small = hip.FLAGSTATS_hip_get(b"chunk_flags"), hip.FLAGSTATS_hip_get(b"small_flags")
    slots = set()
    try:
        assert hip.FLAGSTATS_hip_set(b"small_flags", 0) == 0, err(hip)        # always stage: K1's host path uses the slots too
        for start in range(3):
            step = start

            def next_chunk():
                nonlocal step
                chunk = CHUNK_WALK[step % 4]
                assert hip.FLAGSTATS_hip_set(b"chunk_flags", chunk) == 0, err(hip)
                step += 1
                return chunk

            for position in range(11):
                chunk = next_chunk()
                if position in (0, 10):
                    x, want = k1[position // 10]
                    out = np.full(32, dp.BIAS, dtype=np.uint64)
                    assert hip.FLAGSTATS_u16_x64(x.ctypes.data, x.size, out.ctypes.data) == 0, err(hip)
                    assert np.array_equal(out, want + np.uint64(dp.BIAS)), (start, position, chunk, "FLAGSTATS_u16_x64")
                    slots.add((start, 2 if x.size > chunk else 1))
                    continue
                case, ref = derived[position - 1], refs[position - 1]
                assert chunk != 8 or case["n"] <= 5000
                bad = run_case(hip, case, ref)
                assert bad is None, "round %d call %d chunk_flags %d: %r %s %r" % (start, position, chunk, dp.describe(case), entry_name(case), bad)
                covered = case["n"] if case["offsets"] is None else int(case["offsets"][-1] - case["offsets"][0])
                slots.add((start, 2 if covered > chunk * 2 // case["W"] else 1))
            assert (start, 1) in slots and (start, 2) in slots, (start, slots)     # some calls of the round took one slot, some two
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old_chunk)
        hip.FLAGSTATS_hip_set(b"small_flags", old_small)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old_chunk and hip.FLAGSTATS_hip_get(b"small_flags") == old_small


# ------------------------------------------------------------------ 3. callers of different kinds at once
CALLS_PER_THREAD = 30
JOIN_SECONDS = 120


def test_concurrent_callers_of_different_kinds(lib, oracle_mod):
    import torch
    hip = lib
    rng = np.random.RandomState(91)
    u16 = lambda n: rng.randint(0, 65536, n).astype(np.uint16)  # noqa: E731
    q = lambda n: rng.randint(0, 256, n).astype(np.uint8)  # noqa: E731
    cuts = lambda n, first, k: np.concatenate([[first], np.sort(rng.randint(first, n - 3, k)), [n - 3]])  # noqa: E731
    problems = []         # (thread, call number, entry, got, want): list.append is atomic

    def three(form, modes, sizes):
        """where / filter / wide_filter cases of one form"""
        n0, n1, n2 = sizes
        return [dp.fixed_case("where_bitmap", form, u16(n0), modes[0], mask=rng.randint(0, 2, n0), sel_offset=3, phase=6),
                dp.fixed_case("filter", form, u16(n1), modes[1], require=1, exclude=0x904, mapq=q(n1), min_mapq=30, mapq_align=3),
                dp.fixed_case("wide_filter", form, widened(u16(n2), np.int64, rng, 700), modes[2], exclude=0x104, mapq=q(n2), min_mapq=9,
                              phase=8, mapq_align=2)]

    def checked(cases):
        pairs = [(Call(c), dp.expected_images(c, dp.reference(c))) for c in cases]
        assert all(2000 <= c["n"] <= 200_000 for c in cases)
        return pairs

    # A: host forms, several chunks each at chunk_flags 8192
    thread_a = checked(three("host", (1, 0, 3), (200_000, 61_003, 90_001)))
    # B: the _sync forms of the four segment families
    nb = (150_000, 70_001, 40_003, 33_333)
    thread_b = checked([
        dp.fixed_case("segments", "sync", u16(nb[0]), 3, offsets=cuts(nb[0], 5, 40)),
        dp.fixed_case("segments_filter", "sync", u16(nb[1]), 0, require=1, exclude=0x900, mapq=q(nb[1]), min_mapq=40, offsets=cuts(nb[1], 0, 7)),
        dp.fixed_case("wide_segments", "sync", widened(u16(nb[2]), np.int32, rng, 900), 1, offsets=cuts(nb[2], 9, 12), phase=4),
        dp.fixed_case("wide_segments_filter", "sync", widened(u16(nb[3]), np.uint64, rng, 900), 2, exclude=0x4, mapq=q(nb[3]), min_mapq=200,
                      offsets=cuts(nb[3], 1, 3), mapq_align=11)])
    # C and D: device forms, each thread on its own stream, all of them += into the same 34 words
    shared = torch.zeros(34, dtype=torch.int64, device="cuda")
    shared_out = (shared.data_ptr(), shared.data_ptr() + 256, shared.data_ptr() + 264)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    adders = []
    for sizes in ((180_000, 2000, 77_777), (3001, 199_999, 50_000)):
        cases = three("device", (0, 2, 2), sizes)
        adders.append([(Call(c), dp.reference(c)) for c in cases])
    want_shared = np.zeros(34, dtype=np.uint64)
    for pairs in adders:
        for k in range(CALLS_PER_THREAD):
            call, ref = pairs[k % len(pairs)]
            rows = ref["rows"][0].copy()
            if not call.case["mode"] & dp.SUPERSET:
                rows[[0, 9, 16]] = 0
            want_shared[:32] += rows
            want_shared[32] += ref["selected"][0]
            if call.case["kind"] in dp.WIDE:
                want_shared[33] |= ref["high"][0]
    assert want_shared[33] and want_shared[0] and want_shared[32]
    # E: K1's host entries (they move to a side engine when the default engine's lock is taken)
    e_arrays = [u16(1000), u16(300_000), u16(123_457)]
    e_wants = [oracle_mod.flagstat_c(x) for x in e_arrays]
    # F: K1's _sync entry and the wide _sync entry on device arrays
    f_low, f_wide = u16(99_999), widened(u16(64_000), np.int32, rng, 800)
    f_owner16, f_ptr16 = device_at_16(f_low.view(np.uint8))
    f_wide_case = dp.fixed_case("wide", "sync", f_wide, 3, phase=4)
    f_pairs = checked([f_wide_case])
    f_want16 = oracle_mod.flagstat_c(f_low)
    torch.cuda.synchronize()

    def record(who, k, entry, got, want):
        problems.append((who, k, entry, got, want))

    def run_checked(who, pairs, k):
        call, want = pairs[k % len(pairs)]
        call.fresh_outputs()
        entry = entry_name(call.case)
        rc = call(hip)
        if rc != 0:
            return record(who, k, entry, "rc %d: %s" % (rc, err(hip)), "0")
        bad = mismatch(call.case, call.read(), want)
        if bad is not None:
            record(who, k, entry, bad, "the reference")

    def body_a(k):
        run_checked("A", thread_a, k)

    def body_b(k):
        run_checked("B", thread_b, k)

    def adder(who, pairs, stream):
        def body(k):
            call = pairs[k % len(pairs)][0]
            rc = call(hip, ctypes.c_void_p(stream.cuda_stream), out=shared_out if call.case["kind"] in dp.WIDE else shared_out[:2] + (None,))
            if rc != 0:
                record(who, k, entry_name(call.case), "rc %d: %s" % (rc, err(hip)), "0")
        return body

    def body_e(k):
        x, want = e_arrays[k % 3], e_wants[k % 3]
        if k % 3 < 2:
            out = np.full(32, dp.BIAS, dtype=np.uint32)
            rc, entry = hip.FLAGSTATS_u16(x.ctypes.data, x.size, out.ctypes.data), "FLAGSTATS_u16"
        else:
            out = np.full(32, dp.BIAS, dtype=np.uint64)
            rc, entry = hip.FLAGSTATS_u16_x64(x.ctypes.data, x.size, out.ctypes.data), "FLAGSTATS_u16_x64"
        if rc != 0:
            return record("E", k, entry, "rc %d: %s" % (rc, err(hip)), "0")
        if not np.array_equal(out.astype(np.uint64), want + np.uint64(dp.BIAS)):
            record("E", k, entry, out.tolist(), (want + np.uint64(dp.BIAS)).tolist())

    def body_f(k):
        if k % 2:
            return run_checked("F", f_pairs, k)
        out = np.full(32, dp.BIAS, dtype=np.uint64)
        rc = hip.FLAGSTATS_hip_device_u16_sync(f_ptr16, f_low.size, out.ctypes.data)
        if rc != 0:
            return record("F", k, "FLAGSTATS_hip_device_u16_sync", "rc %d: %s" % (rc, err(hip)), "0")
        if not np.array_equal(out, f_want16 + np.uint64(dp.BIAS)):
            record("F", k, "FLAGSTATS_hip_device_u16_sync", out.tolist(), (f_want16 + np.uint64(dp.BIAS)).tolist())

    bodies = {"A": body_a, "B": body_b, "C": adder("C", adders[0], streams[0]), "D": adder("D", adders[1], streams[1]), "E": body_e,
              "F": body_f}
    barrier = threading.Barrier(len(bodies))

    def worker(who, body):
        try:
            barrier.wait(timeout=JOIN_SECONDS)
            for k in range(CALLS_PER_THREAD):
                body(k)
        except BaseException as exc:                       # nothing is raised across the thread boundary
            record(who, -1, "the thread itself", repr(exc), "no exception")

    old_chunk = hip.FLAGSTATS_hip_get(b"chunk_flags")
    assert hip.FLAGSTATS_hip_set(b"chunk_flags", 8192) == 0, err(hip)   # knobs are global: set before the threads, restored after
    try:
        threads = {who: threading.Thread(target=worker, args=(who, body), name="caller-" + who, daemon=True) for who, body in bodies.items()}
        for t in threads.values():
            t.start()
        for t in threads.values():
            t.join(JOIN_SECONDS)
        stuck = [who for who, t in threads.items() if t.is_alive()]
        assert not stuck, ("still running after %d s" % JOIN_SECONDS, stuck)
        assert hip.FLAGSTATS_hip_get(b"chunk_flags") == 8192
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old_chunk)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old_chunk
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    assert problems == [], "%d mismatches, the first: %r" % (len(problems), problems[:4])
    got_shared = shared.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_shared, want_shared), ([hex(int(v)) for v in got_shared], [hex(int(v)) for v in want_shared])
    del f_owner16
