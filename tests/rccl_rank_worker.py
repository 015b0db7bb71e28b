"""One RANK of the multi-rank tests (tests/test_gpu_multi_ranks.py, tests/test_rccl_stub_host.py); not collected by pytest.

    python tests/rccl_rank_worker.py RANK WORLD ID_HEX[,ID_HEX] SCENARIO SEED OUT_PREFIX

The ranks are fresh processes that share one GPU.  The parent sets FLAGSTATS_HIP_RCCL to the RCCL stand-in
(tests/hoststub/rccl_stub.cpp) in the child's environment only, so the product library binds it instead of RCCL, and ships the
128-byte id that it got from the stand-in's ncclGetUniqueId.  The worker runs one scenario through the product's C ABI, keeps
every step's reduced counters in a device log (row j is copied behind step j's all-reduce, in stream order, and read once at the
end), writes OUT_PREFIX.npy (uint64 [steps, 32]) and OUT_PREFIX.json, and exits 0; on an error of the library it prints the
library's last error and exits non-zero.  torch gives streams and tensors only; torch.distributed is not used.

`plan(scenario, world, seed)` is the one description of what every rank does in every step; the tests build their expectation
from it with the oracle, never from a run of the library.  The scenarios whose name starts with `host` drive the stand-in's
summing protocol alone (rccl_stub_host_allreduce through ctypes): no GPU, no torch, no product library.
"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STUB = os.path.join(ROOT, "tests", "hoststub", "build", "librccl_stub.so")
GEN_UNIFORM, GEN_NA12878 = 0, 1
K1_STEP = 16384                      # flags per K1 step: lengths sit on both sides of it
SHARD = 6_000_000 + 4 * K1_STEP      # flags in every rank's shard (weak-scaling scenarios)
BIG_TOTAL = 2 ** 30                  # `overlapped`: flags of all shards together, so that its LONG windows keep K1 busy for longer
                                     # than a collective takes (2 GiB over the chip, whatever the world) -- see shard_flags
STRONG_N = 20_000_003                # the global array of `strong`: leaves a remainder to the last rank at world 3 and 8
POISON = 0xFFFFFFFFFFFFFFFF         # what the stand-in delivers when a wait ran out or a rank was lost
NCCL_SYSTEM_ERROR, NCCL_INVALID_ARGUMENT = 2, 4
SCENARIOS = ("inline", "overlapped", "skew", "switch", "strong", "counters")


def stub_path():
    """The stand-in, built by `make rcclstub` (part of `all`); made here if a tree was built without it."""
    if not os.path.exists(STUB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "libflagstats_amd", "csrc"), "rcclstub"], check=True,
                       capture_output=True, timeout=600)
    return STUB


class UniqueId(ctypes.Structure):
    """ncclUniqueId: 128 bytes, passed to ncclCommInitRank BY VALUE."""
    _fields_ = [("internal", ctypes.c_char * 128)]


def as_id(raw):
    return UniqueId.from_buffer_copy(raw if isinstance(raw, bytes) else bytes.fromhex(raw))


def load_stub():
    lib = ctypes.CDLL(stub_path())
    lib.ncclGetUniqueId.argtypes = [ctypes.c_void_p]
    lib.ncclCommInitRank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, UniqueId, ctypes.c_int]
    lib.ncclCommCount.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    lib.ncclCommDestroy.argtypes = [ctypes.c_void_p]
    lib.ncclGetVersion.argtypes = [ctypes.POINTER(ctypes.c_int)]
    lib.rccl_stub_host_allreduce.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.rccl_stub_uses_wait_value.argtypes = [ctypes.c_void_p]
    return lib


def new_id(stub):
    """A fresh 128-byte id (its shared-memory segment exists from here on) as (hex, segment name)."""
    buf = (ctypes.c_char * 128)()
    rc = stub.ncclGetUniqueId(buf)
    assert rc == 0, rc
    raw = buf.raw
    assert raw[:8] == b"RCCLSTUB"
    return raw.hex(), raw[8:].split(b"\0")[0].decode()


def shard_of(rank, seed):
    """(kind, seed, mask) of a rank's shard: both generators are in every world."""
    return (GEN_UNIFORM, seed + rank, 0xFFFF) if rank % 2 == 0 else (GEN_NA12878, seed + rank, 1)


def vector(seed, comm, rank, step):
    """The uint64[32] a rank contributes in `counters` and in the host scenarios: depends on everything, and half of the slots
    sit at or above 2^63, so that the sum over two or more ranks wraps."""
    v = np.random.default_rng([seed, comm, rank, step]).integers(0, 2 ** 64, 32, dtype=np.uint64)
    v[::2] |= np.uint64(1 << 63)
    v[5] = np.uint64(1 << 63)
    v[7] = np.uint64(POISON - rank)
    return v


_LENGTHS = (K1_STEP - 1, K1_STEP, K1_STEP + 1, 1, 3_000_017, 5, 3 * K1_STEP + 7, 100_003, 2 * K1_STEP, 1_000_001, 5_000_001,
            K1_STEP // 2, 7 * K1_STEP - 1, 250_000, 4_500_003, 33)


def shard_flags(scenario, world):
    """Flags in every rank's shard.  `overlapped` has big shards: with the ordering event missing, the side stream reads a
    counter buffer early only if K1 + K2 of that step are still running, and the side stream lags by one collective per step, so
    runs of its steps count most of a shard that takes K1 several collectives' time (the ranks share the chip, so the sum over
    ranks is what counts, and it is the same in every world)."""
    return BIG_TOTAL // world + 12_345 if scenario == "overlapped" else SHARD


def _windows(rng, world, steps, first=0, shard=SHARD, long_steps=()):
    """Step j of rank r counts [off, off + len) of its shard: every step other flags, offsets at all 2-byte alignments of a
    16-byte line, lengths on both sides of the K1 step, a few of millions, and n == 0 on one rank in every fifth step; in
    `long_steps` (indices into this phase) 70-98 % of the shard."""
    out = []
    for j in range(first, first + steps):
        row = []
        for r in range(world):
            n = _LENGTHS[(j + 3 * r) % len(_LENGTHS)]
            if j - first in long_steps:
                n = int(shard * (0.70 + 0.28 * float(rng.random())))
            if j % 5 == 2 and r == (j // 5) % world:
                n = 0
            off = int(rng.integers(0, (shard - n) // 8)) * 8 + (j + r) % 8
            row.append((min(off, shard - n), n))
        out.append(row)
    return out


def plan(scenario, world, seed):
    """List of phases; a phase is a dict with `form` ("inline" | "overlapped" | "counters"), `ring`, `null_launch` (the launch
    stream is the null stream, as in bench.py) and `steps`; a step is a dict with `win` (per rank (offset, length)) and, in
    `skew`, `late` = (rank, "gpu" | "host").  `strong` windows are (offset, length) in the GLOBAL array."""
    rng = np.random.default_rng([seed, world, (SCENARIOS + ("badargs",)).index(scenario)])
    phases = []

    def phase(form, steps, ring=1, null_launch=False, late=None, long_steps=()):
        first = sum(len(p["steps"]) for p in phases)
        st = [{"win": w} for w in _windows(rng, world, steps, first, shard_flags(scenario, world), long_steps)]
        for k, who_how in (late or {}).items():
            st[k]["late"] = who_how
        phases.append({"form": form, "ring": ring, "null_launch": null_launch, "steps": st})

    if scenario == "inline":
        phase("inline", 26, null_launch=True)
    elif scenario == "overlapped":
        phase("overlapped", 13, ring=3, null_launch=True, long_steps=range(4, 10))    # 4 passes and one step
        phase("overlapped", 27, ring=8, long_steps=range(6, 20))                      # 3 passes and three steps
    elif scenario == "skew":
        for third in range(3):               # a different rank is late in each third
            who = (third + 1) % world
            phase("overlapped", 10, ring=3, late={2: (who, "gpu"), 6: (who, "host")})
        for third in range(3):
            who = (third + 2) % world
            phase("inline", 5, late={1: (who, "gpu"), 3: (who, "host")})
    elif scenario == "switch":
        phase("inline", 8, null_launch=True)
        phase("overlapped", 19, ring=8, null_launch=True)
        phase("inline", 8, null_launch=True)
    elif scenario == "strong":
        wins = [(0, STRONG_N)]
        for j in range(1, 8):
            n = int(rng.integers(1, STRONG_N // 2)) if j % 3 else _LENGTHS[j]
            wins.append((int(rng.integers(0, STRONG_N - n)), n))
        phases.append({"form": "inline", "ring": 1, "null_launch": True, "steps": [{"win": w} for w in wins[:4]]})
        phases.append({"form": "overlapped", "ring": 3, "null_launch": False, "steps": [{"win": w} for w in wins[4:]]})
    elif scenario == "counters":
        phases.append({"form": "counters", "ring": 1, "null_launch": False, "steps": [{} for _ in range(20)]})
    elif scenario == "badargs":
        phase("inline", 3)
    else:
        raise ValueError(scenario)
    return phases


def strong_cut(win, b, e):
    """The part of the global window `win` that lies in the shard [b, e): (offset inside the shard, length)."""
    lo, hi = max(win[0], b), min(win[0] + win[1], e)
    return (lo - b, hi - lo) if hi > lo else (0, 0)


# ------------------------------------------------------------------------------------------------ host scenarios (no GPU)
def run_host(rank, world, ids, scenario, seed, out_prefix):
    """host:STEPS[:LEAVE_AFTER]  every communicator of `ids`, STEPS collectives each, random sleeps in between; the LAST rank
    leaves (exits without ncclCommDestroy) after LEAVE_AFTER steps if that is given."""
    parts = scenario.split(":")
    steps = int(parts[1])
    leave_after = int(parts[2]) if len(parts) > 2 else None
    stub = load_stub()
    info = {"rank": rank, "init_rc": [], "rc": [], "count": [], "destroy_rc": []}
    comms = []
    t0 = time.monotonic()
    for raw in ids:
        c = ctypes.c_void_p()
        rc = stub.ncclCommInitRank(ctypes.byref(c), world, as_id(raw), rank)
        info["init_rc"].append(rc)
        comms.append(c if rc == 0 else None)
    info["init_s"] = time.monotonic() - t0
    got = np.zeros((len(ids), steps, 32), dtype=np.uint64)
    if all(comms):
        for c in comms:
            n = ctypes.c_int(-1)
            stub.ncclCommCount(c, ctypes.byref(n))
            info["count"].append(n.value)
        rng = np.random.default_rng([seed, rank, 99])
        order = list(range(len(comms)))
        for j in range(steps):
            if leave_after is not None and rank == world - 1 and j == leave_after:
                np.save(out_prefix + ".npy", got)
                with open(out_prefix + ".json", "w") as f:
                    json.dump(info, f)
                sys.exit(0)            # leaves without a word: the stand-in's exit handler marks the rank as gone
            rcs = [None] * len(comms)
            for ci in order:   # the host form is synchronous: every rank keeps the same order of communicators
                time.sleep(float(rng.random()) * 0.003 if rng.random() < 0.5 else 0.0)
                v = vector(seed, ci, rank, j)
                t1 = time.monotonic()
                rcs[ci] = stub.rccl_stub_host_allreduce(comms[ci], v.ctypes.data, 32)
                info["slowest_call_s"] = max(info.get("slowest_call_s", 0.0), time.monotonic() - t1)
                got[ci, j] = v
            info["rc"].append(rcs)
        for c in comms:
            info["destroy_rc"].append(stub.ncclCommDestroy(c))
    np.save(out_prefix + ".npy", got)
    with open(out_prefix + ".json", "w") as f:
        json.dump(info, f)


# ------------------------------------------------------------------------------------------------ GPU scenarios
def independent_side_stream(torch, dev, launches):
    """(side stream, verdict).  The runtime maps streams onto a few hardware queues, and two streams that share one run in
    order: a launch stream could then never overtake a side stream that waits for another rank, and the scenarios would pass
    whatever the ordering calls were.  So the side stream is chosen by trial: hold a candidate the way a waiting collective
    does and see whether work queued afterwards on each launch stream completes meanwhile.  Verdict True: it did, on every
    launch stream; False: no candidate of 12 was independent; None: the runtime has no wait-value operation to hold with."""
    stub = ctypes.CDLL(stub_path())
    stub.rccl_stub_hold_stream.restype = ctypes.c_void_p
    stub.rccl_stub_hold_stream.argtypes = [ctypes.c_void_p]
    stub.rccl_stub_release.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    probe = torch.zeros(64, device=dev)
    torch.cuda.synchronize()
    side = None
    for _ in range(12):
        side = torch.cuda.Stream(device=dev)
        if any(side.cuda_stream == s.cuda_stream for s in launches):
            continue
        hold = stub.rccl_stub_hold_stream(ctypes.c_void_p(side.cuda_stream))
        if not hold:
            return side, None
        free = True
        for s in launches:
            with torch.cuda.stream(s):
                probe.add_(1)
                ev = torch.cuda.Event()
                ev.record(s)
            t0 = time.monotonic()
            while not ev.query() and time.monotonic() - t0 < 0.05:
                time.sleep(0.0005)
            free = free and ev.query()
        stub.rccl_stub_release(ctypes.c_void_p(hold), ctypes.c_void_p(side.cuda_stream))
        torch.cuda.synchronize()
        if free:
            return side, True
    return side, False


def run_gpu(rank, world, raw_id, scenario, seed, out_prefix):
    import torch

    from libflagstats_amd import _lib, device

    lib = _lib.lib()
    lib.FLAGSTATS_hip_set(b"on_error", 0)
    _lib.check(lib.FLAGSTATS_hip_init(0), "FLAGSTATS_hip_init")
    dev = torch.device("cuda", 0)
    info = {"rank": rank, "world": world, "scenario": scenario, "bad": {}}

    if scenario == "badargs":
        # the same bad calls on every rank BEFORE the first collective: nobody waits for a rank that failed
        info["bad"]["rank_ge_nranks"] = [bool(lib.FLAGSTATS_hip_comm_init_rank(raw_id, world, world, 0)),
                                         lib.FLAGSTATS_hip_last_error().decode(errors="replace")]
        info["bad"]["null_id"] = [bool(lib.FLAGSTATS_hip_comm_init_rank(None, world, rank, 0)),
                                  lib.FLAGSTATS_hip_last_error().decode(errors="replace")]
    comm = lib.FLAGSTATS_hip_comm_init_rank(raw_id, world, rank, 0)
    if not comm:
        _lib.check(-1, "FLAGSTATS_hip_comm_init_rank")
    info["comm_count"] = int(lib.FLAGSTATS_hip_comm_count(comm))
    buf, ver = ctypes.create_string_buffer(1024), ctypes.c_int(-1)
    _lib.check(lib.FLAGSTATS_hip_comm_library(buf, len(buf), ctypes.byref(ver)), "FLAGSTATS_hip_comm_library")
    info["library"], info["version"] = buf.value.decode(errors="replace"), int(ver.value)

    phases = plan(scenario, world, seed)
    nsteps = sum(len(p["steps"]) for p in phases)
    strong = scenario == "strong"
    if strong:
        b, e = ctypes.c_uint64(), ctypes.c_uint64()
        lib.FLAGSTATS_hip_shard_range(STRONG_N, rank, world, ctypes.byref(b), ctypes.byref(e))
        info["shard"] = [b.value, e.value]
        flags = torch.empty(e.value - b.value, dtype=torch.int16, device=dev)
        device.generate_torch(flags, GEN_UNIFORM, seed=seed, mask=0xFFFF, first_index=b.value)
    else:
        kind, sd, mask = shard_of(rank, seed)
        flags = torch.empty(shard_flags(scenario, world), dtype=torch.int16, device=dev)
        device.generate_torch(flags, kind, seed=sd, mask=mask)
    log = torch.full((nsteps, 32), -7, dtype=torch.int64, device=dev)
    scratch = torch.zeros(32, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    if scenario == "badargs":
        host = np.zeros(32, dtype=np.uint64)
        null = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        info["bad"]["host_counters"] = [lib.FLAGSTATS_hip_allreduce_counters(host.ctypes.data, comm, null),
                                        lib.FLAGSTATS_hip_last_error().decode(errors="replace")]
        for name, obj in (("stream_is_a_communicator", comm), ("stream_is_no_object", 0x1234)):
            info["bad"][name] = [lib.FLAGSTATS_hip_stream_wait_stream(null, ctypes.c_void_p(obj), 0),
                                 lib.FLAGSTATS_hip_last_error().decode(errors="replace")]

    null_stream = torch.cuda.current_stream(dev)
    own_launch = torch.cuda.Stream(device=dev)
    side, info["independent_streams"] = independent_side_stream(torch, dev, (null_stream, own_launch))
    side_p = ctypes.c_void_p(side.cuda_stream)
    # `skew`: what the late rank's extra K1 launches read, 2 GiB each (its content does not matter)
    ballast = torch.empty(2 ** 30, dtype=torch.int16, device=dev) if scenario == "skew" else None
    keep = []
    j = 0
    for ph in phases:
        launch = null_stream if ph["null_launch"] else own_launch
        launch_p = ctypes.c_void_p(launch.cuda_stream)
        ring = [torch.full((32,), -9, dtype=torch.int64, device=dev) for _ in range(ph["ring"])]
        keep.extend(ring)
        for s in (own_launch, side):     # torch filled the buffers on the null stream: the phase's streams start behind that
            s.wait_stream(null_stream)
        for i, st in enumerate(ph["steps"]):
            if ph["form"] == "counters":
                # alternately on the two streams; each waits for the other first, so the calls are in stream order
                stream, other = (launch, side) if i % 2 == 0 else (side, launch)
                d = torch.from_numpy(vector(seed, 0, rank, j).view(np.int64)).to(dev)
                keep.append(d)
                stream.wait_stream(null_stream)
                stream.wait_stream(other)
                _lib.check(lib.FLAGSTATS_hip_allreduce_counters(d.data_ptr(), comm, ctypes.c_void_p(stream.cuda_stream)),
                           "FLAGSTATS_hip_allreduce_counters")
                with torch.cuda.stream(stream):
                    log[j].copy_(d, non_blocking=True)
                j += 1
                continue
            off, n = strong_cut(st["win"], *info["shard"]) if strong else st["win"][rank]
            late = st.get("late")
            if late and late[0] == rank:
                if late[1] == "gpu":     # a few long K1 launches queued in front on this rank's launch stream
                    for _ in range(8):
                        _lib.check(lib.FLAGSTATS_hip_device_u16(ballast.data_ptr(), ballast.numel(), scratch.data_ptr(), launch_p),
                                   "late K1")
                else:
                    time.sleep(0.05)
            ptr = flags.data_ptr() + 2 * off
            if ph["form"] == "inline":
                _lib.check(lib.FLAGSTATS_hip_device_u16_allreduce(ptr, n, ring[0].data_ptr(), comm, launch_p), "allreduce")
                with torch.cuda.stream(launch):
                    log[j].copy_(ring[0], non_blocking=True)
            else:
                k = i % len(ring)
                if k == 0 and i:   # once per ring pass, as include/libflagstats_hip.h prescribes
                    _lib.check(lib.FLAGSTATS_hip_stream_wait_stream(launch_p, side_p, 0), "stream_wait_stream")
                _lib.check(lib.FLAGSTATS_hip_device_u16_allreduce_overlapped(ptr, n, ring[k].data_ptr(), comm, launch_p, side_p),
                           "allreduce overlapped")
                with torch.cuda.stream(side):
                    log[j].copy_(ring[k], non_blocking=True)
            j += 1
        # between forms: the side stream drains into the launch streams (bench.py's drain()), and the next phase's buffers
        # and launch stream start behind everything of this one
        for s in (null_stream, own_launch):
            s.wait_stream(side)
        own_launch.wait_stream(null_stream)
        null_stream.wait_stream(own_launch)
    torch.cuda.synchronize()
    got = log.cpu().numpy().view(np.uint64)
    stub = ctypes.CDLL(info["library"])   # the copy the product bound: already loaded, this only names it
    stub.rccl_stub_uses_wait_value.argtypes = [ctypes.c_void_p]
    info["wait_value"] = int(stub.rccl_stub_uses_wait_value(ctypes.c_void_p(comm)))
    info["destroy_rc"] = int(lib.FLAGSTATS_hip_comm_destroy(comm))
    np.save(out_prefix + ".npy", got)
    with open(out_prefix + ".json", "w") as f:
        json.dump(info, f)


def main(argv):
    rank, world, ids, scenario, seed, out_prefix = int(argv[1]), int(argv[2]), argv[3], argv[4], int(argv[5]), argv[6]
    raws = [bytes.fromhex(h) for h in ids.split(",")]
    assert all(len(r) == 128 for r in raws)
    if scenario.startswith("host"):
        run_host(rank, world, raws, scenario, seed, out_prefix)
        return 0
    assert os.environ.get("FLAGSTATS_HIP_RCCL"), "the parent names the stand-in in FLAGSTATS_HIP_RCCL"
    try:
        run_gpu(rank, world, raws[0], scenario, seed, out_prefix)
    except Exception as e:  # noqa: BLE001 -- the text is what the parent shows
        print("rank %d: %s: %s" % (rank, type(e).__name__, e), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
