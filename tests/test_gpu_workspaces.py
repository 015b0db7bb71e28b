"""GPU: the state that outlives a launch and is shared between launches -- the per-caller-stream workspaces of the device
entries (flagstat_engine.hip count_on_user_stream: one per stream, most recently used first, at most 64), their regrowth when
"blocks_per_cu" is raised (ensure_ws), and the 8 KiB ticket-and-copies block behind the partials that every launch must leave
zero (flagstat_kernels.hip fsk_launch) -- pushed where no other test goes: more streams than the engine keeps, regrowth with
work still queued, a grid smaller than the one the workspace was made for, every asynchronous entry family interleaved on one
stream with the launch knobs flipped between launches and no host wait, caller threads of different entry families at once;
and the three public entries no other GPU test calls.  Counters are integers: every comparison is exact.

One case is deliberately NOT tested (include/libflagstats_hip.h, INTEGRATION.md "Error behaviour"): a captured graph holds its
stream's workspace pointer, so replaying it after its stream was evicted or "blocks_per_cu" was raised touches freed memory;
a test of that could only pass by provoking a fault."""
import ctypes
import os
import sys
import threading
import time

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import blockfile_tool as bt  # noqa: E402

pytestmark = pytest.mark.gpu

U64 = np.uint64
KIND, SEED, MASK = 0, 20261, 0xFFFF     # GEN_UNIFORM: every flag bit, every slot live
STEP = 16384                            # flags per K1 step
KEPT = 64                               # kMaxUserStreams


def _steps(a, m):
    """K1 steps of the slice [a, a + m) of a 16-byte aligned array (fsk_launch: lo = a, hi = a + m, 8 flags per vector)."""
    return ((a + m + 7) // 8 + 2047) // 2048


def two_level_expected(grid_knob, a, m, max_steps, min_grid=64):
    """fsk_launch's rule for the accumulate form into device memory with the atomic epilogue."""
    if m == 0:
        return None                                            # no launch
    grid = min(grid_knob, _steps(a, m))
    return int(grid >= min_grid and -(-_steps(a, m) // grid) <= max_steps)


class Data:
    """One device array of n3 + 64 generated flags for every test here, and the oracle's counters of its slices (each computed
    once).  The plain counters come from oracle.flagstat_generated; the superset slots and the bit counts, which the generated
    form does not give, from the host twin of the array."""

    def __init__(self, hip):
        import torch

        import oracle
        from libflagstats_amd import device
        self.cus = hip.FLAGSTATS_hip_compute_units()
        assert self.cus >= 64, self.cus
        self.n1 = 70_001
        self.n2 = STEP * self.cus * 2 + 4321
        self.n3 = STEP * self.cus * 3 + 77
        self.total = self.n3 + 64
        self.t = torch.empty(self.total, dtype=torch.int16, device="cuda:0")
        device.generate_torch(self.t, KIND, SEED, MASK)
        torch.cuda.synchronize()
        assert self.t.data_ptr() % 16 == 0
        self.host = oracle.generate(KIND, SEED, MASK, 0, self.total)
        a = self.host
        pp = ((a & 0x100) == 0) & ((a & 0x800) == 0) & ((a & 1) == 1)
        fail = (a & 0x200) != 0
        self._pp_pass = np.concatenate(([0], np.cumsum(pp & ~fail, dtype=np.int64)))
        self._pp_fail = np.concatenate(([0], np.cumsum(pp & fail, dtype=np.int64)))
        self._cache = {}
        self._oracle = oracle

    def ptr(self, a):
        return self.t.data_ptr() + 2 * a

    def want(self, a, m, form="plain"):
        """uint64[32] of slice [a, a + m): 'plain' the 19 counters, 'superset' plus slots 0 / 16 / 9; 'pos': uint64[16] bit counts."""
        assert 0 <= a and a + m <= self.total
        key = (a, m, form)
        if key not in self._cache:
            if form == "pos":
                w = self._oracle.pospopcnt(self.host[a:a + m])
            else:
                w = self._oracle.flagstat_generated(KIND, SEED, MASK, a, m, threads=8).copy()
                if form == "superset":
                    w[0] = self._pp_pass[a + m] - self._pp_pass[a]
                    w[16] = self._pp_fail[a + m] - self._pp_fail[a]
                    w[9] = m - int(w[25])
            self._cache[key] = w
        return self._cache[key]


@pytest.fixture(scope="module")
def data(hip):
    return Data(hip)


class Runtime:
    """The HIP runtime this process has already loaded, for streams of the test's own: torch.cuda.Stream() hands out streams
    from a small pool, far fewer distinct ones than the engine keeps workspaces for."""

    def __init__(self):
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        assert path, "libamdhip64 is not loaded"
        self.rt = ctypes.CDLL(path)
        self.rt.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
        self.rt.hipStreamCreateWithFlags.restype = ctypes.c_int
        self.rt.hipStreamDestroy.argtypes = [ctypes.c_void_p]
        self.rt.hipStreamDestroy.restype = ctypes.c_int
        self.made = []

    def streams(self, count):
        out = []
        for _ in range(count):
            h = ctypes.c_void_p()
            assert self.rt.hipStreamCreateWithFlags(ctypes.byref(h), 1) == 0      # hipStreamNonBlocking
            assert h.value
            out.append(h.value)
            self.made.append(h.value)
        return out

    def destroy(self):
        for h in self.made:
            assert self.rt.hipStreamDestroy(ctypes.c_void_p(h)) == 0
        self.made = []


@pytest.fixture()
def runtime(hip):
    import torch
    torch.cuda.set_device(0)
    rt = Runtime()
    yield rt
    torch.cuda.synchronize()
    rt.destroy()


@pytest.fixture()
def knobs(hip):
    """Set knobs through this; every one touched is put back afterwards."""
    old = {}

    def set_knob(key, value):
        k = key.encode()
        if k not in old:
            old[k] = hip.FLAGSTATS_hip_get(k)
        assert hip.FLAGSTATS_hip_set(k, value) == 0, key

    yield set_knob
    for k, v in old.items():
        hip.FLAGSTATS_hip_set(k, v)


def _sp(stream):
    return ctypes.c_void_p(stream) if stream else None


class Calls:
    """The asynchronous device entries on raw stream handles, each checked for its return code."""

    def __init__(self, hip, data):
        from libflagstats_amd import _lib
        self.hip, self.data, self.check = hip, data, _lib.check

    def acc(self, a, m, out, stream):
        self.check(self.hip.FLAGSTATS_hip_device_u16(self.data.ptr(a), m, out, _sp(stream)), "device_u16")

    def store(self, a, m, out, stream):
        self.check(self.hip.FLAGSTATS_hip_device_u16_store(self.data.ptr(a), m, out, _sp(stream)), "device_u16_store")

    def superset(self, a, m, out, stream):
        self.check(self.hip.FLAGSTATS_hip_device_u16_superset(self.data.ptr(a), m, out, _sp(stream)), "device_u16_superset")

    def pos(self, a, m, out, stream):
        self.check(self.hip.FLAGSTATS_hip_device_pospopcnt_u16(self.data.ptr(a), m, out, _sp(stream)), "device_pospopcnt_u16")

    def allreduce(self, a, m, out, comm, stream):
        self.check(self.hip.FLAGSTATS_hip_device_u16_allreduce(self.data.ptr(a), m, out, comm, _sp(stream)), "device_u16_allreduce")


def _dirty_the_allocator(hip, grids, copies=24):
    """Allocate, fill with non-zero flags and free buffers of exactly the sizes a workspace has (21 x 8 bytes per workgroup +
    the 8 KiB block), so that a fresh workspace is likely to be handed memory that is not zero: the library zeroes it itself."""
    from libflagstats_amd import _lib
    ptrs = []
    for g in grids:
        nbytes = g * 21 * 8 + 8192
        for _ in range(copies):
            p = hip.FLAGSTATS_hip_device_alloc(nbytes)
            assert p, hip.FLAGSTATS_hip_last_error()
            ptrs.append(p)
            _lib.check(hip.FLAGSTATS_hip_generate_u16(p, nbytes // 2, 0, 99, 0xFFFF, 0, None), "generate")
    _lib.check(hip.FLAGSTATS_hip_synchronize(), "sync")
    for p in ptrs:
        hip.FLAGSTATS_hip_device_free(p)


def _u64(t):
    return t.cpu().numpy().view(U64)


# ------------------------------------------------------------------ 1. more caller streams than the engine keeps
def test_more_caller_streams_than_the_engine_keeps(hip, data, runtime, knobs):
    """70 streams of the test's own and the NULL stream, visited in the same order for three rounds: with 71 > 64 streams in
    least-recently-used order every call from the 65th on evicts a workspace (device-wide wait, free) and every stream comes
    back after having been evicted.  Round 1 and 2 accumulate, round 3 is the store form on even streams and the superset
    accumulate on odd ones; slices cycle through the two-level size, a small one-level size, one step minus a flag and one
    flag.  No host wait between the calls.  Then a stream is evicted while its own launches are still queued, and returns."""
    import torch
    d, c = data, Calls(hip, data)
    knobs("blocks_per_cu", 1)
    knobs("epilogue", 1)
    knobs("group_min_grid", 64)
    knobs("group_max_steps", 40)
    held0 = hip.FLAGSTATS_hip_get(b"user_workspaces")
    assert held0 <= KEPT, held0
    _dirty_the_allocator(hip, [d.cus], copies=80)
    streams = runtime.streams(70)
    assert len(set(streams)) == 70 and 0 not in streams
    streams.append(0)                                                      # HIP's NULL stream is a caller stream like any other
    nslots = len(streams)
    outs = torch.zeros((nslots, 32), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    want = np.zeros((nslots, 32), dtype=U64)
    sizes = [d.n2, d.n1, STEP - 1, 1]
    most, forms = held0, []

    def after_call(expect_form=None):
        nonlocal most
        held = hip.FLAGSTATS_hip_get(b"user_workspaces")
        assert held <= KEPT, held
        most = max(most, held)
        if expect_form is not None:
            assert hip.FLAGSTATS_hip_get(b"last_k1_two_level") == expect_form
            forms[-1][expect_form] += 1

    t0 = time.perf_counter()
    for rnd in range(3):
        forms.append([0, 0])
        for i, s in enumerate(streams):
            a = (i + rnd) % 8
            m = sizes[i % 4] if rnd < 2 else sizes[(i // 2) % 4]           # (round 3: both parities see every size)
            o = outs[i].data_ptr()
            if rnd < 2:
                c.acc(a, m, o, s)
                want[i] += d.want(a, m)
            elif i % 2 == 0:
                c.store(a, m, o, s)
                want[i] = d.want(a, m)
            else:
                c.superset(a, m, o, s)
                want[i] += d.want(a, m, "superset")
            direct = rnd < 2 or i % 2 == 1
            after_call(two_level_expected(d.cus, a, m, 40) if direct else None)
        # 71 distinct streams have called: the engine holds 64 workspaces whatever it held before, and never more
        assert hip.FLAGSTATS_hip_get(b"user_workspaces") == KEPT
        assert forms[-1][0] >= 1 and forms[-1][1] >= 1, forms
    # An evicted stream with work in flight.  The engine now holds the NULL stream and streams 7..69 (the last 64 callers).
    # 24 launches of n3 are queued on the NULL stream; streams 7..69 then call with one flag each (63 hits: a splice, no wait),
    # which leaves the NULL stream least recently used; stream 0's call is a miss and evicts it, with its launches still
    # queued or running; the NULL stream's return is another miss.
    null = nslots - 1
    for k in range(24):
        c.acc(k % 8, d.n3, outs[null].data_ptr(), 0)
        want[null] += d.want(k % 8, d.n3)
        after_call(1)
    for i in range(7, 70):
        c.acc(3, 1, outs[i].data_ptr(), streams[i])
        want[i] += d.want(3, 1)
        after_call(0)
    c.acc(1, d.n2, outs[0].data_ptr(), streams[0])
    want[0] += d.want(1, d.n2)
    after_call(1)
    for k in range(4):
        c.acc(k, d.n2, outs[null].data_ptr(), 0)
        want[null] += d.want(k, d.n2)
        after_call(1)
    c.pos(5, d.n2, outs[null].data_ptr() + 128, 0)                          # (slots 16..31 of the NULL stream's row take the bit counts too)
    want[null][16:] += d.want(5, d.n2, "pos")
    after_call()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    got = _u64(outs)
    bad = [i for i in range(nslots) if not np.array_equal(got[i], want[i])]
    print("caller streams: %d distinct + NULL, workspaces held before %d, most %d, after %d; forms per round [one-level, two-level] %s; %.2f s"
          % (70, held0, most, hip.FLAGSTATS_hip_get(b"user_workspaces"), forms, wall))
    assert not bad, bad
    assert most == KEPT and hip.FLAGSTATS_hip_get(b"user_workspaces") == KEPT


# ------------------------------------------------------------------ 2. regrowth while others are busy, and the shrunken grid
def test_regrowth_with_work_queued_and_a_grid_below_the_workspaces(hip, data, runtime, knobs):
    """"blocks_per_cu" raised 1 -> 2 -> 5 while launches are still queued on a caller stream: the next call on each stream --
    two caller streams and an open session, which has workspaces of its own -- frees its workspace, makes a larger one and zeroes
    it on its stream.  Then the knob goes back to 1: the grid is smaller than the one the workspaces were made for and the block
    stays where the larger partials put it; the two-level form, the store form and pospopcnt in both epilogues run there."""
    import torch

    import oracle
    from libflagstats_amd.session import StreamSession
    d, c = data, Calls(hip, data)
    knobs("epilogue", 1)
    knobs("group_min_grid", 64)
    knobs("group_max_steps", 40)
    knobs("blocks_per_cu", 1)
    knobs("chunk_flags", 1 << 19)                                          # session chunks of 1 MiB: every second push below submits one
    _dirty_the_allocator(hip, [d.cus, 2 * d.cus, 5 * d.cus])
    sa, sb = runtime.streams(2)
    acc = torch.zeros((2, 32), dtype=torch.int64, device="cuda:0")
    sto = torch.full((2, 32), 77, dtype=torch.int64, device="cuda:0")
    pos = torch.zeros((2, 16), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    want_acc = np.zeros((2, 32), dtype=U64)
    want_pos = np.zeros((2, 16), dtype=U64)
    block = oracle.generate(oracle.GEN_NA12878, 41, 1, 0, 300_000)
    want_block, pushes = oracle.flagstat_hist(block), 0
    forms = [0, 0]

    def call(which, a, m):
        c.acc(a, m, acc[which].data_ptr(), (sa, sb)[which])
        want_acc[which] += d.want(a, m)
        exp = two_level_expected(hip.FLAGSTATS_hip_get(b"grid"), a, m, 40)
        assert hip.FLAGSTATS_hip_get(b"last_k1_two_level") == exp
        forms[exp] += 1

    with StreamSession() as ses:
        def push_twice():
            nonlocal pushes
            ses.push(block)
            ses.push(block)
            pushes += 2

        call(0, 0, d.n2)
        call(1, 1, d.n1)
        push_twice()
        for bpc in (2, 5):
            for k in range(6):                                             # still queued on A when the knob goes up
                call(0, k, d.n2 if k % 2 else d.n3)
            knobs("blocks_per_cu", bpc)
            assert hip.FLAGSTATS_hip_get(b"grid") == bpc * d.cus
            call(1, 2, d.n2)
            call(0, 3, d.n3)
            call(1, 4, d.n1)
            push_twice()
        knobs("blocks_per_cu", 1)                                          # grid < grid_cap: the block stays behind 5 x CUs partials
        assert hip.FLAGSTATS_hip_get(b"grid") == d.cus
        for k in range(10):
            call(0, k % 8, d.n2)
            call(1, (k + 3) % 8, d.n2)
        push_twice()
        for which, s in enumerate((sa, sb)):
            c.store(which + 1, d.n2, sto[which].data_ptr(), s)
            for epilogue in (1, 0):
                knobs("epilogue", epilogue)
                c.pos(which + 2, d.n3, pos[which].data_ptr(), s)
                want_pos[which] += d.want(which + 2, d.n3, "pos")
            knobs("epilogue", 1)
            call(which, 6, d.n2)                                           # the two-level form again, behind the K2 forms
        got_ses = ses.finish()
    torch.cuda.synchronize()
    print("regrowth: forms [one-level, two-level] %s, %d session pushes" % (forms, pushes))
    assert np.array_equal(_u64(acc), want_acc)
    assert np.array_equal(_u64(sto), np.stack([d.want(1, d.n2), d.want(2, d.n2)]))
    assert np.array_equal(_u64(pos), want_pos)
    assert np.array_equal(got_ses, want_block * U64(pushes))
    assert forms[1] >= 20 and forms[0] >= 1, forms


# ------------------------------------------------------------------ 3. every async entry on one workspace, knobs flipped between launches
FAMILIES = ("acc", "store", "superset", "superset_host", "pos0", "pos1", "acc_k2", "allreduce")


def launch_plan(cus, n1, n2, n3, count=300, seed=20261017):
    """The fixed sequence of test 3: (family, start offset, flags, variant, epoch_stagger, group_max_steps) per launch."""
    rs = np.random.RandomState(seed)
    edge = [n1, n2, n3, 0, 1, 7, STEP - 1]
    plan = []
    for _ in range(count):
        fam = FAMILIES[rs.randint(len(FAMILIES))]
        if rs.randint(3) == 0:
            fam = "acc"                                                    # (the family whose form matters gets a third of the launches)
        m = [n1, n2, n3][rs.randint(3)] if fam == "acc" else edge[rs.randint(len(edge))]
        plan.append((fam, int(rs.randint(8)), int(m), int([9, 25, 71][rs.randint(3)]), int(rs.randint(2)), int([2, 40][rs.randint(2)])))
    return plan


def plan_forms(plan, cus):
    """[small one-level, large one-level, two-level] launches of the plan's direct-epilogue families."""
    forms = [0, 0, 0]
    for fam, a, m, _, _, gms in plan:
        if fam in ("acc", "superset") and m:
            two = two_level_expected(cus, a, m, gms)
            forms[2 if two else (1 if min(cus, _steps(a, m)) >= 64 else 0)] += 1
    return forms


def test_every_async_entry_on_one_workspace_with_knobs_flipped_between_launches(hip, data, runtime, knobs):
    """300 launches on ONE caller stream -- one workspace, one ticket-and-copies block -- with no host wait: accumulate through
    the small one-level, the large one-level and the two-level epilogue, the store form (K1 + K2), superset into device and into
    pinned-host counters (K2), pospopcnt in both epilogues, accumulate through K1 + K2, and the all-reduce store form on a
    communicator of one rank; before every launch the K1 schedule, the epoch stagger and the step limit of the two-level form are
    drawn anew.  Accumulate families are checked against the running sum, store families against their last launch."""
    import torch
    from libflagstats_amd import _lib
    d, c = data, Calls(hip, data)
    plan = launch_plan(d.cus, d.n1, d.n2, d.n3)
    want_forms = plan_forms(plan, d.cus)
    assert min(want_forms) >= 20, want_forms
    for key, value in (("blocks_per_cu", 1), ("epilogue", 1), ("group_min_grid", 64), ("group_max_steps", 40), ("variant", 71),
                       ("epoch_stagger", 1)):
        knobs(key, value)
    (s,) = runtime.streams(1)
    ident = (ctypes.c_char * 128)()
    comm = None
    if hip.FLAGSTATS_hip_comm_unique_id(ident) == 0:
        comm = hip.FLAGSTATS_hip_comm_init_rank(ident, 1, 0, 0)
    if not comm:
        print("NOTE: RCCL cannot be loaded (%s): the all-reduce family is left out, its launches go to the store form"
              % hip.FLAGSTATS_hip_last_error().decode(errors="replace"))
    hp = hip.FLAGSTATS_hip_host_alloc(256)
    assert hp
    try:
        host = np.ctypeslib.as_array(ctypes.cast(hp, ctypes.POINTER(ctypes.c_uint64)), shape=(32,))
        host[:] = 5
        names = ("acc", "store", "superset", "pos", "acc_k2", "allreduce")
        outs = {k: torch.full((32,), 9, dtype=torch.int64, device="cuda:0") for k in names}
        want = {k: np.full(32, 9, dtype=U64) for k in names}
        want_host = np.full(32, 5, dtype=U64)
        torch.cuda.synchronize()
        forms, ran = [0, 0, 0], {k: 0 for k in FAMILIES}
        for fam, a, m, variant, stagger, gms in plan:
            knobs("variant", variant)
            knobs("epoch_stagger", stagger)
            knobs("group_max_steps", gms)
            if fam == "allreduce" and not comm:
                fam = "store"
            ran[fam] += 1
            if fam in ("acc", "superset"):
                (c.acc if fam == "acc" else c.superset)(a, m, outs[fam].data_ptr(), s)
                want[fam] += d.want(a, m, "plain" if fam == "acc" else "superset")
                if m:
                    two = two_level_expected(d.cus, a, m, gms)
                    assert hip.FLAGSTATS_hip_get(b"last_k1_two_level") == two, (fam, a, m, gms)
                    forms[2 if two else (1 if min(d.cus, _steps(a, m)) >= 64 else 0)] += 1
            elif fam == "store":
                c.store(a, m, outs["store"].data_ptr(), s)
                want["store"] = d.want(a, m).copy()
            elif fam == "superset_host":
                c.check(hip.FLAGSTATS_hip_device_u16_superset(d.ptr(a), m, hp, _sp(s)), "superset into pinned-host counters")
                want_host += d.want(a, m, "superset")
            elif fam in ("pos0", "pos1"):
                knobs("epilogue", int(fam[-1]))
                c.pos(a, m, outs["pos"].data_ptr(), s)
                knobs("epilogue", 1)
                want["pos"][:16] += d.want(a, m, "pos")
            elif fam == "acc_k2":
                knobs("epilogue", 0)
                c.acc(a, m, outs["acc_k2"].data_ptr(), s)
                knobs("epilogue", 1)
                want["acc_k2"] += d.want(a, m)
                if m:
                    assert hip.FLAGSTATS_hip_get(b"last_k1_two_level") == 0
            else:
                c.allreduce(a, m, outs["allreduce"].data_ptr(), comm, s)
                want["allreduce"] = d.want(a, m).copy()
        torch.cuda.synchronize()
        print("one workspace, 300 launches: forms [small one-level, large one-level, two-level] %s, launches per family %s" % (forms, ran))
        for k in names:
            assert np.array_equal(_u64(outs[k]), want[k]), k
        assert np.array_equal(host, want_host)
        assert forms == want_forms and min(forms) >= 20, (forms, want_forms)
    finally:
        torch.cuda.synchronize()
        hip.FLAGSTATS_hip_host_free(hp)
        if comm:
            _lib.check(hip.FLAGSTATS_hip_comm_destroy(comm), "comm destroy")


# ------------------------------------------------------------------ 4. mixed caller threads, fixed work
def test_caller_threads_of_different_entry_families(hip, data, knobs):
    """Five threads behind a barrier, 20 iterations each, nothing timed: (a) an LZ4 block image through the GPU decoder, which holds
    the default engine for the whole file, (b) the same as Zstandard, (c) the reference-shaped host entry at three sizes (side
    engines while (a) / (b) hold the default one; every such call also ages the decoder's kept buffers), (d) a session on its
    own streams, (e) the device entry and the segmented entry on a caller stream.  Every result is checked in its thread."""
    import torch

    import oracle
    from libflagstats_amd import blockfile, device, segments
    from libflagstats_amd.session import StreamSession
    d = data
    iters = 20
    knobs("lz4_gpu_min_bytes", 1)
    knobs("zstd_gpu_min_bytes", 1)
    for key, value in (("blocks_per_cu", 1), ("epilogue", 1), ("group_max_steps", 40), ("variant", 71), ("epoch_stagger", 1)):
        knobs(key, value)
    flags = oracle.generate(oracle.GEN_NA12878, 17, 1, 0, 4 * 512000)
    want_file = oracle.flagstat_hist(flags)
    img_lz4 = bt.block_file_image(flags)
    have_zstd = hip.FLAGSTATS_hip_zstd_available() == 1
    img_zstd = bt.block_file_image(flags, mode="zstd", level=1) if have_zstd else None
    if not have_zstd:
        print("NOTE: libzstd cannot be loaded: the Zstandard thread is left out")
    host_arrays = [oracle.generate(oracle.GEN_UNIFORM, 60 + k, 0xFFFF, 0, n) for k, n in enumerate((1000, 1 << 18, 1 << 22))]
    want_host = [oracle.flagstat_hist(a) for a in host_arrays]
    block = flags[:512000]
    want_block = oracle.flagstat_hist(block)
    seg_offsets = np.array([0, 1000, 70_001, 70_001, 200_000, 200_007], dtype=np.int64)
    want_seg = np.stack([d.want(int(lo), int(hi - lo)) for lo, hi in zip(seg_offsets[:-1], seg_offsets[1:])])
    offsets_dev = torch.from_numpy(seg_offsets).to("cuda:0")
    device_out = torch.zeros(32, dtype=torch.int64, device="cuda:0")       # (zeroed here: thread (e) has a stream of its own)
    torch.cuda.synchronize()
    errors, done = [], {}
    names = ["lz4", "zstd", "host", "session", "device"] if have_zstd else ["lz4", "host", "session", "device"]
    barrier = threading.Barrier(len(names))

    def decoder(name, entry, img):
        for it in range(iters):
            got, st = entry(img, 0)
            assert st["gpu_decode"] == 1 and st["n_flags"] == flags.size, (name, it, st)
            assert np.array_equal(got, want_file), (name, it)
            done[name] = it + 1

    def host_calls():
        for it in range(iters):
            k = it % 3
            got = np.zeros(32, dtype=np.uint32)
            assert hip.FLAGSTATS_u16(host_arrays[k].ctypes.data, host_arrays[k].size, got.ctypes.data) == 0, it
            assert np.array_equal(got.astype(U64), want_host[k]), (it, k)
            done["host"] = it + 1

    def session():
        with StreamSession() as ses:
            pending = 0
            for it in range(iters):
                ses.push(block)
                pending += 1
                if it % 5 == 4:
                    assert ses.pending_flags == pending * block.size
                    assert np.array_equal(ses.finish(), want_block * U64(pending)), it
                    pending = 0
                done["session"] = it + 1

    def device_calls():
        s = torch.cuda.Stream()
        out = device_out
        total = np.zeros(32, dtype=U64)
        with torch.cuda.stream(s):
            for it in range(iters):
                a, m = it % 8, (d.n2, d.n1, d.n3, 7)[it % 4]
                device.count_torch(d.t[a:a + m], out)
                total += d.want(a, m)
                seg = segments.count_segments_torch(d.t[:200_064], offsets_dev)
                s.synchronize()
                assert np.array_equal(_u64(out), total), it
                assert np.array_equal(_u64(seg), want_seg), it
                done["device"] = it + 1

    work = {"lz4": lambda: decoder("lz4", blockfile.flagstat_lz4_image, img_lz4),
            "zstd": lambda: decoder("zstd", blockfile.flagstat_zstd_image, img_zstd),
            "host": host_calls, "session": session, "device": device_calls}

    def run(name):
        try:
            barrier.wait(timeout=60)
            work[name]()
        except BaseException as e:  # noqa: BLE001
            errors.append((name, done.get(name, 0), repr(e)))

    threads = [threading.Thread(target=run, args=(n,), name=n, daemon=True) for n in names]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)             # a cap, not a measurement: the work is a few seconds
    stuck = [t.name for t in threads if t.is_alive()]
    if stuck:
        pytest.exit("caller threads %s are still inside the library after 120 s (iterations done: %s): the engine is wedged, "
                    "no further GPU test may start behind it" % (stuck, done), returncode=1)
    print("mixed caller threads %s: iterations done %s in %.2f s" % (names, done, time.perf_counter() - t0))
    assert not errors, errors
    assert all(done.get(n) == iters for n in names), done


# ------------------------------------------------------------------ 5. the entries no other GPU test calls
READ_ONLY = (b"user_workspaces", b"staged_calls", b"host_chunks", b"host_overlapped", b"lz4_gpu_kept_bytes")


def test_ctx_device_u16_sync(hip, data):
    """FLAGSTATS_hip_ctx_device_u16_sync: a device array through a private engine, out[32] += counters, synchronous; a host
    pointer and a NULL out are refused with a message; the default engine is not involved."""
    d = data
    ctx = hip.FLAGSTATS_hip_ctx_create(0)
    assert ctx, hip.FLAGSTATS_hip_last_error()
    try:
        assert hip.FLAGSTATS_hip_ctx_device(ctx) == 0
        before = [hip.FLAGSTATS_hip_get(k) for k in READ_ONLY]
        out = np.arange(500, 532, dtype=U64)
        want = out.copy()
        for off in (0, 3):
            for n in (0, 1, STEP - 1, STEP * 3 + 5, 5_000_011):
                assert hip.FLAGSTATS_hip_ctx_device_u16_sync(ctx, d.ptr(off), n, out.ctypes.data) == 0, (off, n)
                want += d.want(off, n)
                assert np.array_equal(out, want), (off, n)
        assert hip.FLAGSTATS_hip_ctx_device_u16_sync(ctx, None, 0, out.ctypes.data) == 0 and np.array_equal(out, want)
        pageable = np.arange(4096, dtype=np.uint16)
        assert hip.FLAGSTATS_hip_ctx_device_u16_sync(ctx, pageable.ctypes.data, pageable.size, out.ctypes.data) != 0
        assert b"d_array" in hip.FLAGSTATS_hip_last_error()
        assert hip.FLAGSTATS_hip_ctx_device_u16_sync(ctx, d.ptr(0), 100, None) != 0
        assert b"out" in hip.FLAGSTATS_hip_last_error()
        assert hip.FLAGSTATS_hip_ctx_device_u16_sync(None, d.ptr(0), 100, out.ctypes.data) != 0
        assert np.array_equal(out, want)                                   # the refused calls left the counters alone
        assert [hip.FLAGSTATS_hip_get(k) for k in READ_ONLY] == before
    finally:
        hip.FLAGSTATS_hip_ctx_destroy(ctx)


def test_host_staged_u16_threads_sizes_and_stats(hip, knobs):
    """FLAGSTATS_hip_host_staged_u16 called directly: worker counts 0 (automatic), 1, 3 and 8, arrays of 0, 1, 2^20 + 7 and
    6,000,013 flags from an even and an odd element, the default chunk size and the smallest the pipeline makes, with and without
    statistics; a page-locked array is taken like a pageable one; a NULL array is refused and leaves out[] alone.  The explicit
    entry does not count as a call the size rule has staged ("staged_calls": flagstat_engine.hip count_host_shared only)."""
    import oracle
    from libflagstats_amd import _lib
    nmax = 6_000_013
    src = oracle.generate(oracle.GEN_NA12878, 23, 1, 0, nmax + 1)
    want = {(start, n): oracle.flagstat_hist(src[start:start + n]) for start in (0, 1) for n in (0, 1, (1 << 20) + 7, nmax)}
    staged0 = hip.FLAGSTATS_hip_get(b"staged_calls")
    for chunk in (None, 70_000):
        if chunk:
            knobs("chunk_flags", chunk)
        for threads in (0, 1, 3, 8):
            for (start, n), w in want.items():
                for with_stats in (False, True):
                    out = np.full(32, 7, dtype=U64)
                    st = _lib.BlockfileStats()
                    rc = hip.FLAGSTATS_hip_host_staged_u16(src.ctypes.data + 2 * start, n, threads, out.ctypes.data,
                                                           ctypes.byref(st) if with_stats else None)
                    assert rc == 0, (chunk, threads, start, n, hip.FLAGSTATS_hip_last_error())
                    assert np.array_equal(out, w + U64(7)), (chunk, threads, start, n)
                    if with_stats:
                        # (an empty array has nothing to put into a chunk: 0 chunks; every other array at least one)
                        assert st.n_flags == n and (st.chunks >= 1 if n else st.chunks == 0) and st.gpu_decode == 0, (chunk, threads, start, n, st.chunks)
                        assert 1 <= st.threads <= (threads if threads else 24), (threads, st.threads)
                        if chunk and n == nmax:
                            assert st.chunks >= 3, st.chunks               # 12 MB in chunks of 1, 2 and 4 MiB
    n = (1 << 20) + 7
    hp = hip.FLAGSTATS_hip_host_alloc(2 * n + 2)
    assert hp
    try:
        pinned = np.ctypeslib.as_array(ctypes.cast(hp, ctypes.POINTER(ctypes.c_uint16)), shape=(n + 1,))
        pinned[:] = src[:n + 1]
        for start in (0, 1):
            out = np.zeros(32, dtype=U64)
            assert hip.FLAGSTATS_hip_host_staged_u16(hp + 2 * start, n, 3, out.ctypes.data, None) == 0
            assert np.array_equal(out, want[(start, n)]), start
    finally:
        hip.FLAGSTATS_hip_host_free(hp)
    out = np.full(32, 7, dtype=U64)
    assert hip.FLAGSTATS_hip_host_staged_u16(None, 100, 3, out.ctypes.data, None) != 0
    assert b"NULL array" in hip.FLAGSTATS_hip_last_error() and (out == 7).all()
    assert hip.FLAGSTATS_hip_host_staged_u16(src.ctypes.data, 100, 3, None, None) != 0
    assert hip.FLAGSTATS_hip_get(b"staged_calls") == staged0


def test_stream_flags_after_a_refused_acquire(hip, knobs):
    """FLAGSTATS_hip_stream_flags counts committed flags only: an acquire refused for exceeding the chunk and an acquire that is
    never committed leave it -- and what finish() returns -- as they were."""
    import oracle
    from libflagstats_amd import _lib
    from libflagstats_amd.session import StreamSession
    knobs("chunk_flags", 1 << 19)                                          # 1 MiB chunks
    a = oracle.generate(oracle.GEN_UNIFORM, 3, 0xFFFF, 0, 1300)
    with StreamSession() as ses:
        assert ses.pending_flags == 0
        ses.push(a[:1000])
        assert ses.pending_flags == 1000
        with pytest.raises(_lib.FlagstatsHipError, match="chunk"):
            ses.acquire((1 << 19) + 64)
        assert ses.pending_flags == 1000
        view = ses.acquire(500)                                            # handed out, never committed
        view[:] = 0xFFFF
        assert ses.pending_flags == 1000
        view = ses.acquire(300)
        view[:] = a[1000:]
        ses.commit(300)
        assert ses.pending_flags == 1300
        assert np.array_equal(ses.finish(), oracle.flagstat_hist(a))
        assert ses.pending_flags == 0
