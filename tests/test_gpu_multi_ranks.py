"""GPU: the one-process-per-device step (FLAGSTATS_hip_device_u16_allreduce / _allreduce_overlapped, flagstat_multi.hip) at
world sizes 2, 3 and 8 on ONE GPU, over a stand-in for RCCL.

Real RCCL refuses two ranks on one device, and at one rank it launches nothing for an in-place all-reduce, so
test_gpu_multi.py::test_rccl_allreduce_world_of_one passes whatever the ordering between K2, the collective and the ring of
counter buffers is.  Here the ranks are fresh processes (tests/rccl_rank_worker.py) that bind tests/hoststub/rccl_stub.cpp through
the product's own knob FLAGSTATS_HIP_RCCL: its ncclAllReduce reads the contribution from device memory in stream order, waits
on the device for the other ranks and writes the sum back in stream order, so a missing ordering event, a buffer read before K2
wrote it or a buffer rewritten while its all-reduce is pending changes the numbers.  Every step counts OTHER flags, and row j of
every rank's log must equal the sum over ranks of the oracle's counters of that rank's window of step j, all 32 slots, bit for bit.
The expectation comes from the oracle alone.

What this covers: the call sequence, stream ordering, the ring rule and rank skew at 2-8 ranks.  What it does not: RCCL itself,
xGMI, any timing (nothing here is timed; the limits below are caps that turn a lost rank into a failed test).

That the tests can fail was shown once, at world 2, on copies that are not kept: with the ordering event dropped from
FLAGSTATS_hip_device_u16_allreduce_overlapped, `overlapped` differed from the oracle in 31 of 40 steps and `skew` in 23 of 45; with
the worker's once-per-ring FLAGSTATS_hip_stream_wait_stream dropped, in 32 of 40 and in 26 of 45.  Both need a side stream that the
launch stream can overtake: two streams that share a hardware queue run in order and hide either fault (the first version of
these tests stayed green for that reason), so every rank picks its side stream by trial and reports it, and the tests assert it.

The pytest process must not bind RCCL through the library (it binds once per process); it gets the id from the stand-in through
ctypes.  No test starts more than 8 ranks, and no two groups run at once."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import rccl_rank_worker as rw
from conftest import ROOT

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "rccl_rank_worker.py")
U64 = np.uint64
RANK_LIMIT_S = 120     # a cap on a scenario that takes seconds, not a measurement
SEED = 20261016


def run_group(tmp_path, world, scenario, seed, worker=WORKER, extra_env=None):
    """One group of `world` rank processes; returns [(info, rows)] by rank.  When a rank exits non-zero or runs out of time the
    rest of the group is killed and the test fails with every rank's stderr tail; nothing is tried again."""
    assert world <= 8
    stub = rw.load_stub()
    hexid, name = rw.new_id(stub)
    env = {k: v for k, v in os.environ.items() if not k.startswith("FLAGSTATS_HIP_")}
    env["FLAGSTATS_HIP_RCCL"] = rw.stub_path()          # in the children only
    env.update(extra_env or {})
    procs, errs = [], []
    try:
        for r in range(world):
            out = str(tmp_path / ("%s_w%d_r%d" % (scenario, world, r)))
            errs.append(open(out + ".stderr", "w+"))
            procs.append((subprocess.Popen([sys.executable, worker, str(r), str(world), hexid, scenario, str(seed), out],
                                           stdout=subprocess.DEVNULL, stderr=errs[-1], env=env, cwd=ROOT), out))
        deadline = time.monotonic() + RANK_LIMIT_S
        why = None
        while why is None and any(p.poll() is None for p, _ in procs):
            bad = [r for r, (p, _) in enumerate(procs) if p.poll() not in (None, 0)]
            if bad:
                why = "rank %s exited with %s" % (bad, [procs[r][0].returncode for r in bad])
            elif time.monotonic() > deadline:
                why = "ranks %s ran out of time (%d s)" % ([r for r, (p, _) in enumerate(procs) if p.poll() is None], RANK_LIMIT_S)
            else:
                time.sleep(0.05)
        bad = [r for r, (p, _) in enumerate(procs) if p.poll() not in (None, 0)]
        if why is None and bad:
            why = "rank %s exited with %s" % (bad, [procs[r][0].returncode for r in bad])
    finally:
        for p, _ in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
        tails = []
        for r, f in enumerate(errs):
            f.seek(0)
            tails.append("--- rank %d stderr ---\n%s" % (r, f.read()[-1500:]))
            f.close()
        left_behind = os.path.exists("/dev/shm" + name)
        if left_behind:
            os.unlink("/dev/shm" + name)
    if why:
        pytest.fail("%s, world %d: %s\n%s" % (scenario, world, why, "\n".join(tails)), pytrace=False)
    assert not left_behind, "the last ncclCommDestroy did not unlink " + name
    res = []
    for r, (_, out) in enumerate(procs):
        res.append((json.load(open(out + ".json")), np.load(out + ".npy")))
    return res


CHUNK = 2 ** 20


class WindowOracle:
    """The oracle's counters of windows of generated arrays.  The counters are sums over flags, so a long window is the oracle's
    whole chunks inside it (each chunk is asked for once and kept) plus the oracle's counters of its two ragged ends: long
    windows that overlap cost the oracle one pass over the shard, which is what keeps a test within about 2^31 flags."""

    def __init__(self):
        import oracle
        self.oracle, self.chunks, self.asked = oracle, {}, 0

    def direct(self, kind, sd, mask, first, n):
        self.asked += n
        return self.oracle.flagstat_generated(kind, sd, mask, first, n, threads=8 if n >= 2 ** 19 else 1)

    def __call__(self, kind, sd, mask, first, n):
        k1, k2 = -(-first // CHUNK), (first + n) // CHUNK
        if k2 - k1 < 2:
            return self.direct(kind, sd, mask, first, n)
        want = self.direct(kind, sd, mask, first, k1 * CHUNK - first) + self.direct(kind, sd, mask, k2 * CHUNK, first + n - k2 * CHUNK)
        for k in range(k1, k2):
            key = (kind, sd, mask, k)
            if key not in self.chunks:
                self.chunks[key] = self.direct(kind, sd, mask, k * CHUNK, CHUNK)
            want += self.chunks[key]
        return want


def expected(scenario, world, seed):
    """uint64 [steps, 32] from the oracle (or, for `counters`, numpy's sum modulo 2^64 of the contributed vectors)."""
    rows = []
    gen = WindowOracle()

    j = 0
    for ph in rw.plan(scenario, world, seed):
        for st in ph["steps"]:
            want = np.zeros(32, dtype=U64)
            if ph["form"] == "counters":
                for r in range(world):
                    want += rw.vector(seed, 0, r, j)
            elif scenario == "strong":
                want = gen(rw.GEN_UNIFORM, seed, 0xFFFF, st["win"][0], st["win"][1])    # the window of the WHOLE array
            else:
                for r in range(world):
                    kind, sd, mask = rw.shard_of(r, seed)
                    want += gen(kind, sd, mask, st["win"][r][0], st["win"][r][1])
            rows.append(want)
            j += 1
    assert gen.asked <= 2 ** 31, gen.asked      # the oracle's share of one test (a budget for its run time)
    return np.stack(rows)


def check_group(res, want, world):
    for r, (info, rows) in enumerate(res):
        assert info["comm_count"] == world, (r, info)
        assert os.path.samefile(info["library"], rw.stub_path()) and info["version"] == 1, (r, info)   # not RCCL, and says so
        assert info["destroy_rc"] == 0, (r, info)
        # the precondition of every verdict below: this rank's launch streams CAN overtake its side stream while that waits
        # for another rank (None: the runtime has no wait-value operation to try it with; the stand-in then carries the
        # collectives with its blocking host function, wait_value == 0)
        assert info["wait_value"] in (0, 1) and info["independent_streams"] is not False, (r, info)
        assert info["independent_streams"] is True or info["wait_value"] == 0, (r, info)
        assert rows.shape == want.shape, (r, rows.shape, want.shape)
        wrong = sorted(set(int(j) for j in np.argwhere(rows != want)[:, 0]))
        assert not wrong, "rank %d: steps %s differ from the oracle; first: got %s want %s" % (r, wrong, rows[wrong[0]], want[wrong[0]])
    for r in range(1, world):
        assert np.array_equal(res[r][1], res[0][1]), r


@pytest.mark.parametrize("scenario", rw.SCENARIOS)
@pytest.mark.parametrize("world", [2, 3, 8])
def test_every_step_of_every_rank_equals_the_oracle_sum(hip, tmp_path, world, scenario):
    """inline: >= 24 in-line steps on one stream.  overlapped: rings of 3 and of 8 buffers, >= 3 passes each, the launch stream
    waiting for the side stream once per pass as include/libflagstats_hip.h prescribes; every step is checked, not only a buffer's
    last user.  skew: both forms while one rank -- another one in each third -- is late, once by long K1 launches queued in front
    on its launch stream and once by a host-side sleep, so that the collective really waits and the side stream really lags.
    switch: in line, overlapped, in line on one communicator (bench.py --calibrate).  strong: one array cut with
    FLAGSTATS_hip_shard_range, remainder on the last rank, first_index = the shard's begin.  counters:
    FLAGSTATS_hip_allreduce_counters alone, values at and above 2^63, alternating streams."""
    seed = SEED + 100 * world
    want = expected(scenario, world, seed)
    if scenario != "counters":
        assert len(set(w.tobytes() for w in want)) == len(want)      # every step has numbers of its own
    res = run_group(tmp_path, world, scenario, seed)
    check_group(res, want, world)
    if scenario == "strong":
        import oracle
        from libflagstats_amd.dist import shard_range
        for r, (info, rows) in enumerate(res):
            assert tuple(info["shard"]) == shard_range(rw.STRONG_N, r, world)
        assert rw.STRONG_N % world != 0
        assert np.array_equal(res[0][1][0], oracle.flagstat_generated(rw.GEN_UNIFORM, seed, 0xFFFF, 0, rw.STRONG_N, threads=8))


def test_argument_errors_stay_loud_and_leave_nobody_waiting(hip, tmp_path):
    """World 2, through the C ABI, on every rank BEFORE its first collective: comm_init_rank with rank >= nranks and with a NULL
    id, allreduce_counters with host memory for d_counters, stream_wait_stream with a stream that is another kind of object.
    Each is refused with a message; the communicator then carries three right steps."""
    world, seed = 2, SEED + 7
    res = run_group(tmp_path, world, "badargs", seed)
    check_group(res, expected("badargs", world, seed), world)
    for info, _ in res:
        bad = info["bad"]
        assert bad["rank_ge_nranks"][0] is False and "communicator arguments" in bad["rank_ge_nranks"][1], bad
        assert bad["null_id"][0] is False and "communicator arguments" in bad["null_id"][1], bad
        assert bad["host_counters"][0] != 0 and "d_counters" in bad["host_counters"][1], bad
        assert bad["stream_is_a_communicator"][0] != 0 and bad["stream_is_a_communicator"][1], bad
        assert bad["stream_is_no_object"][0] != 0 and bad["stream_is_no_object"][1], bad
