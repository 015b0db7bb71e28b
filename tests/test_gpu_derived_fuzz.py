"""GPU: the eighteen kernels derived from K1's step tree under a randomized sweep, one after another over the engine's staging
slots, and from several threads at once -- the eight of the first family (where, filter, segments, segments_filter, wide,
wide_filter, wide_segments, wide_segments_filter), the nine derived later (derived_plan.LATER_KINDS: the masked kinds and the
two of the whole predicate, --rf / -G) and the segmented unit of the whole predicate (derived_plan.RF_SEGMENTED_KINDS), each
family in tests of its own.  Cases, reference and the poisoned input / output images
come from tests/derived_plan.py (checked on the CPU by tests/test_derived_plan_host.py); every comparison is exact, and every
call is one the header documents as legal.

To run one case of a sweep again: ``derived_plan.plan(SEED, index + 1)[index]``, ``plan_later(LATER_SEED, index + 1)[index]`` or
``plan_rf_segmented(RF_SEGMENTED_SEED, index + 1)[index]`` -- a failure names the index and the drawn parameters."""
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
LATER_SEED = 20261021   # ... and that of dp.plan_later(LATER_SEED, ...), the nine later units
RF_SEGMENTED_SEED = 20261024    # ... and that of dp.plan_rf_segmented(RF_SEGMENTED_SEED, ...), fixed there before any GPU run

# arguments of every entry, by name: A array, N n, W elem_bytes, S / SO / SB selection, its offset and encoding, R / X / Q / MQ
# require, exclude, MAPQ column, min_mapq, O / NS offsets and nseg, OUT / SEL / HIGH outputs, Z a zero (the launchers' `base`)
PUBLIC = {"where": "A N S SO SB OUT SEL MODE", "filter": "A N R X Q MQ OUT SEL MODE", "segments": "A N O NS OUT MODE",
          "segments_filter": "A N O NS R X Q MQ OUT SEL MODE", "wide": "A N W OUT HIGH MODE", "wide_filter": "A N W R X Q MQ OUT SEL HIGH MODE",
          "wide_segments": "A N W O NS OUT HIGH MODE", "wide_segments_filter": "A N W O NS R X Q MQ OUT SEL HIGH MODE",
          # the nine later units: IA / XA include_any and exclude_all
          "segments_where": "A N O NS S SO SB OUT SEL MODE", "wide_where": "A N W S SO SB OUT SEL HIGH MODE",
          "wide_segments_where": "A N W O NS S SO SB OUT SEL HIGH MODE", "filter_where": "A N R X Q MQ S SO SB OUT SEL MODE",
          "segments_filter_where": "A N O NS R X Q MQ S SO SB OUT SEL MODE", "wide_filter_where": "A N W R X Q MQ S SO SB OUT SEL HIGH MODE",
          "wide_segments_filter_where": "A N W O NS R X Q MQ S SO SB OUT SEL HIGH MODE", "filter_rf": "A N R X IA XA Q MQ OUT SEL MODE",
          "wide_filter_rf": "A N W R X IA XA Q MQ OUT SEL HIGH MODE", "segments_filter_rf": "A N O NS R X IA XA Q MQ OUT SEL MODE"}
LAUNCHER = {"where": ("fsk_launch_where", "A N S SO SB OUT SEL MODE GRID"), "filter": ("fsk_launch_filter", "A N R X Q MQ OUT SEL MODE GRID"),
            "segments": ("fsk_launch_segments", "A Z N O NS OUT MODE GRID"),
            "segments_filter": ("fsk_launch_segments_filter", "A Q Z N O NS R X MQ OUT SEL MODE GRID"),
            "wide": ("fsk_launch_wide", "A N W OUT HIGH MODE GRID"), "wide_filter": ("fsk_launch_wide_filter", "A N W R X Q MQ OUT SEL HIGH MODE GRID"),
            "wide_segments": ("fsk_launch_segments_wide", "A W Z N O NS OUT HIGH MODE GRID"),
            "wide_segments_filter": ("fsk_launch_segments_wide_filter", "A W Q Z N O NS R X MQ OUT SEL HIGH MODE GRID"),
            "segments_where": ("fsk_launch_segments_where", "A S SO SB Z N O NS OUT SEL MODE GRID"),
            "wide_where": ("fsk_launch_wide_where", "A N W S SO SB OUT SEL HIGH MODE GRID"),
            "wide_segments_where": ("fsk_launch_segments_wide_where", "A W S SO SB Z N O NS OUT SEL HIGH MODE GRID"),
            "filter_where": ("fsk_launch_filter_where", "A N R X Q MQ S SO SB OUT SEL MODE GRID"),
            "segments_filter_where": ("fsk_launch_segments_filter_where", "A Q S SO SB Z N O NS R X MQ OUT SEL MODE GRID"),
            "wide_filter_where": ("fsk_launch_wide_filter_where", "A N W R X Q MQ S SO SB OUT SEL HIGH MODE GRID"),
            "wide_segments_filter_where": ("fsk_launch_segments_wide_masked_filter", "A W Q S SO SB Z N O NS R X MQ OUT SEL HIGH MODE GRID"),
            "filter_rf": ("fsk_launch_filter_rf", "A N R X IA XA Q MQ OUT SEL MODE GRID"),
            "wide_filter_rf": ("fsk_launch_wide_filter_rf", "A N W R X IA XA Q MQ OUT SEL HIGH MODE GRID"),
            "segments_filter_rf": ("fsk_launch_segments_filter_rf", "A Q Z N O NS R X IA XA MQ OUT SEL MODE GRID")}
STEM = {"where": "u16_where", "filter": "u16_filter", "segments": "u16_segments", "segments_filter": "u16_segments_filter", "wide": "wide",
        "wide_filter": "wide_filter", "wide_segments": "wide_segments", "wide_segments_filter": "wide_segments_filter",
        "segments_where": "u16_segments_where", "wide_where": "wide_where", "wide_segments_where": "wide_segments_where",
        "filter_where": "u16_filter_where", "segments_filter_where": "u16_segments_filter_where", "wide_filter_where": "wide_filter_where",
        "wide_segments_filter_where": "wide_segments_filter_where", "filter_rf": "u16_filter_rf", "wide_filter_rf": "wide_filter_rf",
        "segments_filter_rf": "u16_segments_filter_rf"}
HOST = {"where": "FLAGSTATS_hip_u16_x64_where", "filter": "FLAGSTATS_hip_u16_x64_filter", "segments": "FLAGSTATS_hip_u16_x64_segments",
        "segments_filter": "FLAGSTATS_hip_u16_x64_segments_filter", "wide": "FLAGSTATS_hip_wide_x64", "wide_filter": "FLAGSTATS_hip_wide_x64_filter",
        "wide_segments": "FLAGSTATS_hip_wide_x64_segments", "wide_segments_filter": "FLAGSTATS_hip_wide_x64_segments_filter",
        "segments_where": "FLAGSTATS_hip_u16_x64_segments_where", "wide_where": "FLAGSTATS_hip_wide_x64_where",
        "wide_segments_where": "FLAGSTATS_hip_wide_x64_segments_where", "filter_where": "FLAGSTATS_hip_u16_x64_filter_where",
        "segments_filter_where": "FLAGSTATS_hip_u16_x64_segments_filter_where", "wide_filter_where": "FLAGSTATS_hip_wide_x64_filter_where",
        "wide_segments_filter_where": "FLAGSTATS_hip_wide_x64_segments_filter_where", "filter_rf": "FLAGSTATS_hip_u16_x64_filter_rf",
        "wide_filter_rf": "FLAGSTATS_hip_wide_x64_filter_rf", "segments_filter_rf": "FLAGSTATS_hip_u16_x64_segments_filter_rf"}
assert set(PUBLIC) == set(LAUNCHER) == set(STEM) == set(HOST) == ({dp.family(k) for k in dp.KINDS} | set(dp.LATER_KINDS)
                                                                    | set(dp.RF_SEGMENTED_KINDS)) and len(PUBLIC) == 18


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
             "MODE": case["mode"], "GRID": case["grid"], "S": None, "SO": case["sel_offset"], "SB": dp.sel_bits_of(case) or 0,
             "Q": None, "O": None, "IA": case.get("include_any", 0), "XA": case.get("exclude_all", 0)}
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
        if case["mask"] is not None:
            img, at = dp.selection_image(case)      # `at` is negative where a bitmap offset of 2^33 + k moves the pointer back
            owner, base = put(img)
            self.keep.append(owner)
            a["S"] = base + at
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
    sweep(lib, dp.plan(SEED, int(os.environ.get("FLAGSTATS_FUZZ_ITERS_DERIVED", "240"))))   # a soak run sets thousands


def test_random_cases_every_later_family(lib, oracle_mod):
    """the nine units derived after the sweep was written (dp.LATER_KINDS), under the same knob"""
    sweep(lib, dp.plan_later(LATER_SEED, int(os.environ.get("FLAGSTATS_FUZZ_ITERS_DERIVED", "240"))))


def test_random_cases_every_rf_segmented_family(lib, oracle_mod):
    """the segmented unit of the whole predicate (dp.RF_SEGMENTED_KINDS), the dealt zero-fill cases among them, under the same knob"""
    sweep(lib, dp.plan_rf_segmented(RF_SEGMENTED_SEED, int(os.environ.get("FLAGSTATS_FUZZ_ITERS_DERIVED", "240"))))


def sweep(hip, cases):
    import torch
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
    """the nine derived calls of one round, in order (the K1 calls around them are made by the test): sizes chosen so that the calls
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
    rng = np.random.RandomState(77)
    derived = interleaved_round(rng)
    refs = [dp.reference(c) for c in derived]
    for c, r in zip(derived, refs):
        assert 100 <= c["n"] <= 200_000 and r["selected"].any() and (c["kind"] not in dp.WIDE or r["high"].any())
    walk_the_slots(lib, oracle_mod, rng, derived, refs)


def walk_the_slots(hip, oracle_mod, rng, derived, refs):
    """three rounds of: a K1 host call, the derived host calls, a K1 host call -- chunk_flags advancing along CHUNK_WALK at every
    call, a round later each time, so that every call but those a multiple of 4 from the round's first meets every chunk size"""
    last_position = len(derived) + 1
    first, last = rng.randint(0, 65536, 200_000).astype(np.uint16), rng.randint(0, 65536, 5000).astype(np.uint16)
    k1 = {0: (first, oracle_mod.flagstat_c(first)), last_position: (last, oracle_mod.flagstat_c(last))}
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

            for position in range(last_position + 1):
                chunk = next_chunk()
                if position in k1:
                    x, want = k1[position]
                    assert chunk != 8 or x.size <= 5000
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


def later_round(rng):
    """the thirteen derived calls of one round of the later kinds, in order: the host forms of the nine later kinds with `filter`
    and `wide` of the old family in between, then two of the segmented unit of the whole predicate.  With a K1 call at positions
    0 and 14, positions 4, 8 and 12 (calls 3, 7 and 11 here) never meet chunk_flags 8: the first two are the large ones, the
    third is the call that can pass nothing and moves nothing."""
    u16 = lambda n: rng.randint(0, 65536, n).astype(np.uint16)  # noqa: E731
    q = lambda n: rng.randint(0, 256, n).astype(np.uint8)  # noqa: E731
    half = lambda n: rng.randint(0, 2, n).astype(bool)  # noqa: E731
    cuts = lambda n, first, k: np.concatenate([[first], np.sort(rng.randint(first, n - 3, k)), [n - 3]])  # noqa: E731
    F = "host"
    n = 3001
    calls = [dp.fixed_case("segments_where", F, u16(n), 3, mask=half(n), sel_bits=1, sel_offset=5, offsets=cuts(n, 7, 9), phase=2, sel_align=3)]
    n = 2203
    calls.append(dp.fixed_case("wide_where", F, widened(u16(n), np.int64, rng, 300), 1, mask=half(n), sel_bits=8, sel_offset=3, phase=8,
                               sel_align=7, high_at="apart"))
    n = 4099
    calls.append(dp.fixed_case("filter", F, u16(n), 0, require=1, exclude=0x904, mapq=q(n), min_mapq=30, mapq_align=1))
    n = 150_001
    calls.append(dp.fixed_case("wide_filter_where", F, widened(u16(n), np.uint32, rng, 5000), 2, exclude=0x704, mapq=q(n), min_mapq=20,
                               mask=half(n), sel_bits=1, sel_offset=11, phase=4, mapq_align=7, sel_align=5, selected_at="apart"))
    n = 2500      # --rf 0x50 -G 0xC beside -f 1 -F 0x900: the reduction leaves both tests
    calls.append(dp.fixed_case("filter_rf", F, u16(n) & np.uint16(0x0FFF), 3, require=1, exclude=0x900, include_any=0x50, exclude_all=0xC,
                               mapq=q(n), min_mapq=30, mapq_align=1))
    n = 2999
    calls.append(dp.fixed_case("wide_segments_where", F, widened(u16(n), np.int32, rng, 100), 0, mask=half(n), sel_bits=1, sel_offset=3,
                               offsets=cuts(n, 1, 5), phase=12, sel_align=9))
    n = 2203
    calls.append(dp.fixed_case("wide", F, widened(u16(n), np.int64, rng, 300), 1, phase=8, high_at="apart"))
    n = 120_003
    calls.append(dp.fixed_case("wide_segments_filter_where", F, widened(u16(n), np.uint64, rng, 9000), 3, require=0x40, exclude=0x800,
                               mapq=q(n), min_mapq=1, mask=half(n), sel_bits=8, offsets=cuts(n, 11, 16), mapq_align=9, sel_align=1,
                               high_at="apart"))
    n = 3777
    calls.append(dp.fixed_case("segments_filter_where", F, u16(n), 1, require=2, exclude=0x100, mapq=q(n), min_mapq=100, mask=half(n),
                               sel_bits=8, sel_offset=1, offsets=cuts(n, 0, 30), mapq_align=5, sel_align=15))
    n = 2001      # every --rf bit is excluded: nothing can pass, nothing is read
    calls.append(dp.fixed_case("wide_filter_rf", F, widened(u16(n), np.uint32, rng, 50), 1, exclude=0x30, include_any=0x30, mapq=q(n),
                               min_mapq=5, phase=4, mapq_align=3))
    n = 2100
    calls.append(dp.fixed_case("filter_where", F, u16(n), 2, require=1, exclude=0x904, mapq=q(n), min_mapq=30, mask=half(n), sel_bits=1,
                               sel_offset=9, mapq_align=11, sel_align=13, selected_at="apart"))
    n = 2801      # every -G bit is required: nothing can pass, nothing is read, the store form still zeroes
    calls.append(dp.fixed_case("segments_filter_rf", F, u16(n), 1, require=0x41, exclude_all=0x41, mapq=q(n), min_mapq=5,
                               offsets=cuts(n, 3, 12), mapq_align=3))
    n = 3333      # --rf 0x50 -G 0xC beside -f 1 -F 0x900 -q 30: both tests are left; the MAPQ slice rides behind a chunk's flags
    calls.append(dp.fixed_case("segments_filter_rf", F, u16(n) & np.uint16(0x0FFF), 2, require=1, exclude=0x900, include_any=0x50,
                               exclude_all=0xC, mapq=q(n), min_mapq=30, offsets=cuts(n, 5, 20), phase=6, mapq_align=7,
                               selected_at="apart"))
    return calls


def test_later_entry_kinds_interleaved_over_the_staging_slots(lib, oracle_mod):
    rng = np.random.RandomState(78)
    derived = later_round(rng)
    refs = [dp.reference(c) for c in derived]
    assert {c["kind"] for c in derived} == set(dp.LATER_KINDS) | set(dp.RF_SEGMENTED_KINDS) | {"filter", "wide"}
    empties = [i for i, c in enumerate(derived) if not dp.Definition().reads(c)]
    assert [derived[i]["kind"] for i in empties] == ["wide_filter_rf", "segments_filter_rf"]
    for i, (c, r) in enumerate(zip(derived, refs)):
        empty = i in empties
        assert 2000 <= c["n"] <= 200_000 and r["selected"].any() != empty, c["kind"]
        assert c["kind"] not in dp.WIDE + dp.LATER_WIDE or r["high"].any() != empty, c["kind"]
    # positions 4, 8 and 12 of a round never meet chunk_flags 8: the two large calls and the empty segmented one
    assert len(derived) == 13 and [i for i, c in enumerate(derived) if c["n"] > 5000] == [3, 7] and empties[1] == 11
    reduced = (ctypes.c_uint32 * 4)()
    nothing, residue = derived[11], derived[12]          # the segmented unit of the whole predicate: an empty call, a residue of both
    assert lib.fsk_filter_rf_reduce(nothing["require"], nothing["exclude"], nothing["include_any"], nothing["exclude_all"], reduced) == 0
    assert lib.fsk_filter_rf_reduce(residue["require"], residue["exclude"], residue["include_any"], residue["exclude_all"], reduced) == 2
    assert reduced[2] and reduced[3] and residue["min_mapq"] > 0 and residue["mapq_align"] & 1 and 2000 <= residue["n"] <= 5000
    assert (refs[12]["selected"] > 0).sum() >= 10 and refs[12]["selected"].sum() < refs[12]["length"].sum() // 4
    rf = {c["kind"]: c for c in derived if c["kind"] in dp.RF}
    assert dp.Definition().reads(rf["filter_rf"]) and not dp.Definition().reads(rf["wide_filter_rf"])       # one counts, one is empty
    both = rf["filter_rf"]                               # residue-both: no bit of --rf or -G is decided by -f / -F
    assert bin(both["include_any"]).count("1") >= 2 and bin(both["exclude_all"]).count("1") >= 2
    assert not (both["include_any"] | both["exclude_all"]) & (both["require"] | both["exclude"])
    masked = [c for c in derived if c["mask"] is not None]
    assert {c["sel_bits"] for c in masked} == {1, 8} and any(c["sel_offset"] & 1 for c in masked)
    assert any(c["sel_align"] & 1 for c in masked) and any(c["mapq_align"] & 1 for c in derived if c["mapq"] is not None)
    walk_the_slots(lib, oracle_mod, rng, derived, refs)


# ------------------------------------------------------------------ 3. callers of different kinds at once
CALLS_PER_THREAD = 30
JOIN_SECONDS = 120


def run_callers(hip, problems, bodies):
    """one thread per body behind one barrier, CALLS_PER_THREAD calls each, at chunk_flags 8192 (knobs are global: set before the
    threads, restored after); nothing is raised across the thread boundary: what goes wrong is appended to `problems`"""
    barrier = threading.Barrier(len(bodies))

    def worker(who, body):
        try:
            barrier.wait(timeout=JOIN_SECONDS)
            for k in range(CALLS_PER_THREAD):
                body(k)
        except BaseException as exc:                       # nothing is raised across the thread boundary
            problems.append((who, -1, "the thread itself", repr(exc), "no exception"))

    old_chunk = hip.FLAGSTATS_hip_get(b"chunk_flags")
    assert hip.FLAGSTATS_hip_set(b"chunk_flags", 8192) == 0, err(hip)
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


def checked_body(hip, problems, who, pairs):
    """body of a thread that makes the calls of `pairs` [(Call, expected images)] in turn and compares each"""
    def body(k):
        call, want = pairs[k % len(pairs)]
        call.fresh_outputs()
        entry = entry_name(call.case)
        rc = call(hip)
        if rc != 0:
            return problems.append((who, k, entry, "rc %d: %s" % (rc, err(hip)), "0"))
        bad = mismatch(call.case, call.read(), want)
        if bad is not None:
            problems.append((who, k, entry, bad, "the reference"))
    return body


def adder_body(hip, problems, who, pairs, stream, shared_out):
    """body of a thread that += the device-form calls of `pairs` into the shared words on its own stream"""
    def body(k):
        call = pairs[k % len(pairs)][0]
        out = shared_out if call.case["high_at"] is not None else shared_out[:2] + (None,)
        rc = call(hip, ctypes.c_void_p(stream.cuda_stream), out=out)
        if rc != 0:
            problems.append((who, k, entry_name(call.case), "rc %d: %s" % (rc, err(hip)), "0"))
    return body


def shared_sum(adders):
    """the 34 words that the adder threads must leave: the sum of the rows, the sum of `selected`, the OR of `high`"""
    want = np.zeros(34, dtype=np.uint64)
    for pairs in adders:
        for k in range(CALLS_PER_THREAD):
            call, ref = pairs[k % len(pairs)]
            rows = ref["rows"][0].copy()
            if not call.case["mode"] & dp.SUPERSET:
                rows[[0, 9, 16]] = 0
            want[:32] += rows
            want[32] += ref["selected"][0]
            if call.case["high_at"] is not None:
                want[33] |= ref["high"][0]
    return want


def k1_body(hip, problems, who, arrays, wants):
    """body of a thread on K1's host entries (they move to a side engine when the default engine's lock is taken)"""
    def body(k):
        x, want = arrays[k % 3], wants[k % 3]
        if k % 3 < 2:
            out = np.full(32, dp.BIAS, dtype=np.uint32)
            rc, entry = hip.FLAGSTATS_u16(x.ctypes.data, x.size, out.ctypes.data), "FLAGSTATS_u16"
        else:
            out = np.full(32, dp.BIAS, dtype=np.uint64)
            rc, entry = hip.FLAGSTATS_u16_x64(x.ctypes.data, x.size, out.ctypes.data), "FLAGSTATS_u16_x64"
        if rc != 0:
            return problems.append((who, k, entry, "rc %d: %s" % (rc, err(hip)), "0"))
        if not np.array_equal(out.astype(np.uint64), want + np.uint64(dp.BIAS)):
            problems.append((who, k, entry, out.tolist(), (want + np.uint64(dp.BIAS)).tolist()))
    return body


def test_concurrent_callers_of_the_later_kinds(lib, oracle_mod):
    import torch
    hip = lib
    rng = np.random.RandomState(92)
    u16 = lambda n: rng.randint(0, 65536, n).astype(np.uint16)  # noqa: E731
    q = lambda n: rng.randint(0, 256, n).astype(np.uint8)  # noqa: E731
    half = lambda n: rng.randint(0, 2, n).astype(bool)  # noqa: E731
    cuts = lambda n, first, k: np.concatenate([[first], np.sort(rng.randint(first, n - 3, k)), [n - 3]])  # noqa: E731
    problems = []         # (thread, call number, entry, got, want): list.append is atomic

    def checked(cases):
        assert all(2000 <= c["n"] <= 200_000 for c in cases)
        return [(Call(c), dp.expected_images(c, dp.reference(c))) for c in cases]

    # A: host forms, several chunks each at chunk_flags 8192
    na = (200_000, 90_001, 61_003, 70_007)
    thread_a = checked([
        dp.fixed_case("filter_where", "host", u16(na[0]), 1, require=1, exclude=0x904, mapq=q(na[0]), min_mapq=30, mask=half(na[0]), sel_bits=1,
                      sel_offset=3, phase=6, mapq_align=3, sel_align=5),
        dp.fixed_case("wide_filter_where", "host", widened(u16(na[1]), np.int64, rng, 700), 3, exclude=0x104, mapq=q(na[1]), min_mapq=9,
                      mask=half(na[1]), sel_bits=8, sel_offset=1, phase=8, mapq_align=2, sel_align=7),
        dp.fixed_case("filter_rf", "host", u16(na[2]), 0, require=1, exclude=0x900, include_any=0x50, exclude_all=0xC, mapq=q(na[2]),
                      min_mapq=30, mapq_align=1),
        dp.fixed_case("segments_filter_rf", "host", u16(na[3]), 2, exclude=0x904, include_any=0x210, exclude_all=0x480, mapq=q(na[3]),
                      min_mapq=20, offsets=cuts(na[3], 3, 25), phase=10, mapq_align=9)])
    # B: the _sync forms of the four segmented masked kinds and of the segmented unit of the whole predicate
    nb = (150_000, 70_001, 40_003, 33_333, 55_555)
    thread_b = checked([
        dp.fixed_case("segments_filter_rf", "sync", u16(nb[4]), 1, require=1, exclude=0x804, include_any=0x110, exclude_all=0x2200,
                      mapq=q(nb[4]), min_mapq=10, offsets=cuts(nb[4], 2, 30), phase=4, mapq_align=5, selected_at="apart"),
        dp.fixed_case("segments_where", "sync", u16(nb[0]), 3, mask=half(nb[0]), sel_bits=1, sel_offset=7, offsets=cuts(nb[0], 5, 40)),
        dp.fixed_case("segments_filter_where", "sync", u16(nb[1]), 0, require=1, exclude=0x900, mapq=q(nb[1]), min_mapq=40, mask=half(nb[1]),
                      sel_bits=8, offsets=cuts(nb[1], 0, 7), sel_align=3),
        dp.fixed_case("wide_segments_where", "sync", widened(u16(nb[2]), np.int32, rng, 900), 1, mask=half(nb[2]), sel_bits=8, sel_offset=2,
                      offsets=cuts(nb[2], 9, 12), phase=4),
        dp.fixed_case("wide_segments_filter_where", "sync", widened(u16(nb[3]), np.uint64, rng, 900), 2, exclude=0x4, mapq=q(nb[3]),
                      min_mapq=200, mask=half(nb[3]), sel_bits=1, sel_offset=13, offsets=cuts(nb[3], 1, 3), mapq_align=11)])
    # C and D: device forms, each thread on its own stream, all of them += into the same 34 words
    shared = torch.zeros(34, dtype=torch.int64, device="cuda")
    shared_out = (shared.data_ptr(), shared.data_ptr() + 256, shared.data_ptr() + 264)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    adders = []
    for (n0, n1, n2), bits in (((180_000, 2000, 77_777), (1, 8)), ((3001, 199_999, 50_000), (8, 1))):
        cases = [dp.fixed_case("wide_where", "device", widened(u16(n0), np.int32, rng, 700), 0, mask=half(n0), sel_bits=bits[0], sel_offset=3,
                               phase=4),
                 dp.fixed_case("wide_filter_where", "device", widened(u16(n1), np.int64, rng, 700), 2, exclude=0x104, mapq=q(n1), min_mapq=9,
                               mask=half(n1), sel_bits=bits[1], sel_offset=6, phase=8, mapq_align=2),
                 dp.fixed_case("wide_filter_rf", "device", widened(u16(n2), np.uint32, rng, 700), 2, exclude=0x800, include_any=0x1C1,
                               exclude_all=0x30, mapq=q(n2), min_mapq=20, mapq_align=5)]
        if not adders:      # one segment, so that its row and its count += into the shared words like a flat call's
            n3 = 66_001
            cases.append(dp.fixed_case("segments_filter_rf", "device", u16(n3), 2, exclude=0x904, include_any=0x50, mapq=q(n3), min_mapq=15,
                                       offsets=[9, n3 - 5], phase=2, mapq_align=3))
        assert all(2000 <= c["n"] <= 200_000 for c in cases)
        adders.append([(Call(c), dp.reference(c)) for c in cases])
    want_shared = shared_sum(adders)
    assert want_shared[33] and want_shared[0] and want_shared[32]
    # E: K1's host entries
    e_arrays = [u16(2000), u16(200_000), u16(123_457)]
    e_wants = [oracle_mod.flagstat_c(x) for x in e_arrays]
    torch.cuda.synchronize()
    run_callers(hip, problems, {"A": checked_body(hip, problems, "A", thread_a), "B": checked_body(hip, problems, "B", thread_b),
                                "C": adder_body(hip, problems, "C", adders[0], streams[0], shared_out),
                                "D": adder_body(hip, problems, "D", adders[1], streams[1], shared_out),
                                "E": k1_body(hip, problems, "E", e_arrays, e_wants)})
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    assert problems == [], "%d mismatches, the first: %r" % (len(problems), problems[:4])
    got_shared = shared.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_shared, want_shared), ([hex(int(v)) for v in got_shared], [hex(int(v)) for v in want_shared])


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
    want_shared = shared_sum(adders)
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

    record = lambda *what: problems.append(what)  # noqa: E731
    wide_sync = checked_body(hip, problems, "F", f_pairs)

    def body_f(k):
        if k % 2:
            return wide_sync(k)
        out = np.full(32, dp.BIAS, dtype=np.uint64)
        rc = hip.FLAGSTATS_hip_device_u16_sync(f_ptr16, f_low.size, out.ctypes.data)
        if rc != 0:
            return record("F", k, "FLAGSTATS_hip_device_u16_sync", "rc %d: %s" % (rc, err(hip)), "0")
        if not np.array_equal(out, f_want16 + np.uint64(dp.BIAS)):
            record("F", k, "FLAGSTATS_hip_device_u16_sync", out.tolist(), (f_want16 + np.uint64(dp.BIAS)).tolist())

    run_callers(hip, problems, {"A": checked_body(hip, problems, "A", thread_a), "B": checked_body(hip, problems, "B", thread_b),
                                "C": adder_body(hip, problems, "C", adders[0], streams[0], shared_out),
                                "D": adder_body(hip, problems, "D", adders[1], streams[1], shared_out),
                                "E": k1_body(hip, problems, "E", e_arrays, e_wants), "F": body_f})
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    assert problems == [], "%d mismatches, the first: %r" % (len(problems), problems[:4])
    got_shared = shared.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_shared, want_shared), ([hex(int(v)) for v in got_shared], [hex(int(v)) for v in want_shared])
    del f_owner16
