"""CPU: the summing protocol of the RCCL stand-in (tests/hoststub/rccl_stub.cpp) on its own.

Every verdict of tests/test_gpu_multi_ranks.py on the multi-rank step leans on the stand-in, so its shared-memory part (join,
contribute, sum, bounded wait, poison) is checked here without a GPU, through rccl_stub_host_allreduce and ctypes, with ranks as
fresh child processes (tests/rccl_rank_worker.py, scenarios `host:...`).  The expectation is numpy's sum modulo 2^64 of the
vectors that `rccl_rank_worker.vector` defines.  /dev/shm is all this needs."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import rccl_rank_worker as rw
from conftest import ROOT

WORKER = os.path.join(ROOT, "tests", "rccl_rank_worker.py")
U64 = np.uint64


def _run_ranks(tmp_path, ranks, world, ids, scenario, seed, timeout_s=None, limit=120):
    """Starts the given ranks, waits for all; returns {rank: (returncode, info, rows, stderr)}."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("FLAGSTATS_HIP_") and k != "RCCL_STUB_TIMEOUT_S"}
    if timeout_s is not None:
        env["RCCL_STUB_TIMEOUT_S"] = str(timeout_s)
    procs = {}
    for r in ranks:
        out = str(tmp_path / ("w%d_r%d" % (world, r)))
        procs[r] = (subprocess.Popen([sys.executable, WORKER, str(r), str(world), ",".join(ids), scenario, str(seed), out],
                                     stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env), out)
    res = {}
    deadline = time.monotonic() + limit
    try:
        for r, (p, out) in procs.items():
            _, err = p.communicate(timeout=max(1.0, deadline - time.monotonic()))
            info = json.load(open(out + ".json")) if os.path.exists(out + ".json") else None
            rows = np.load(out + ".npy") if os.path.exists(out + ".npy") else None
            res[r] = (p.returncode, info, rows, err)
    finally:
        for p, _ in procs.values():
            if p.poll() is None:
                p.kill()
                p.wait()
    return res


def _want(seed, ncomm, world, steps):
    want = np.zeros((ncomm, steps, 32), dtype=U64)
    for ci in range(ncomm):
        for j in range(steps):
            for r in range(world):
                want[ci, j] += rw.vector(seed, ci, r, j)     # uint64 addition wraps modulo 2^64
    return want


def _gone(names):
    for n in names:
        assert not os.path.exists("/dev/shm" + n), "segment %s was left behind" % n


@pytest.fixture
def stub():
    assert os.path.isdir("/dev/shm")
    return rw.load_stub()


def test_version_and_id(stub):
    v = rw.ctypes.c_int(-1)
    assert stub.ncclGetVersion(rw.ctypes.byref(v)) == 0 and v.value == 1    # nothing that ran on it passes for RCCL
    _, name = rw.new_id(stub)
    assert os.path.exists("/dev/shm" + name)
    os.unlink("/dev/shm" + name)                                            # an id nobody joined: the maker tidies up


@pytest.mark.parametrize("world", [2, 3, 8])
def test_sums_wrap_and_match_in_every_step(stub, tmp_path, world):
    """300 collectives of rank- and step-dependent uint64[32] with random sleeps of up to 3 ms, so that the ranks arrive in
    every order; the sum wraps in half of the slots."""
    steps, seed = 300, 1000 + world
    hexid, name = rw.new_id(stub)
    res = _run_ranks(tmp_path, range(world), world, [hexid], "host:%d" % steps, seed)
    want = _want(seed, 1, world, steps)
    exact = [sum(int(rw.vector(seed, 0, r, 0)[k]) for r in range(world)) for k in range(32)]
    assert sum(x >= 2 ** 64 for x in exact) >= 16 and [x % 2 ** 64 for x in exact] == [int(x) for x in want[0, 0]]   # it wraps
    for r in range(world):
        rc, info, rows, err = res[r]
        assert rc == 0 and info and info["init_rc"] == [0], (r, rc, err[-2000:])
        assert info["count"] == [world] and info["destroy_rc"] == [0]
        assert all(x == [0] for x in info["rc"]) and len(info["rc"]) == steps
        assert np.array_equal(rows, want), (r, np.argwhere(rows != want)[:5])
    _gone([name])


def test_two_communicators_in_the_same_processes_do_not_mix(stub, tmp_path):
    world, steps, seed = 3, 120, 77
    ids = [rw.new_id(stub) for _ in range(2)]
    res = _run_ranks(tmp_path, range(world), world, [h for h, _ in ids], "host:%d" % steps, seed)
    want = _want(seed, 2, world, steps)
    assert not np.array_equal(want[0], want[1])
    for r in range(world):
        rc, info, rows, err = res[r]
        assert rc == 0 and info["init_rc"] == [0, 0] and info["count"] == [world, world], (r, rc, err[-2000:])
        assert np.array_equal(rows, want), r
    _gone([n for _, n in ids])


def test_a_rank_that_never_joins_fails_the_others_within_the_bound(stub, tmp_path):
    world = 3
    hexid, name = rw.new_id(stub)
    t0 = time.monotonic()
    res = _run_ranks(tmp_path, [0, 2], world, [hexid], "host:5", 5, timeout_s=2, limit=60)
    assert time.monotonic() - t0 < 30
    for r in (0, 2):
        rc, info, rows, err = res[r]
        assert rc == 0 and info["init_rc"] == [rw.NCCL_SYSTEM_ERROR], (r, rc, info, err[-2000:])
        assert info["init_s"] < 10 and not info["rc"]
    assert max(res[r][1]["init_s"] for r in (0, 2)) > 1.5   # they did wait for the third rank, up to the bound
    assert "rccl_stub" in res[0][3] + res[2][3]              # one loud line
    _gone([name])


def test_a_rank_that_leaves_poisons_the_others(stub, tmp_path):
    """The last rank exits after step 4 without a word.  The others: steps 0..3 right, step 4 all-ones and ncclSystemError, every
    later call ncclSystemError, all within the bound; nothing stays in /dev/shm."""
    world, steps, leave, seed = 3, 8, 4, 9
    hexid, name = rw.new_id(stub)
    t0 = time.monotonic()
    res = _run_ranks(tmp_path, range(world), world, [hexid], "host:%d:%d" % (steps, leave), seed, timeout_s=2, limit=60)
    assert time.monotonic() - t0 < 30
    want = _want(seed, 1, world, steps)
    assert res[world - 1][0] == 0
    for r in range(world - 1):
        rc, info, rows, err = res[r]
        assert rc == 0 and info["init_rc"] == [0], (r, rc, err[-2000:])
        assert np.array_equal(rows[0, :leave], want[0, :leave]), r
        assert info["rc"][:leave] == [[0]] * leave
        assert info["rc"][leave:] == [[rw.NCCL_SYSTEM_ERROR]] * (steps - leave), info["rc"]
        assert np.all(rows[0, leave] == U64(rw.POISON)), rows[0, leave]
        for j in range(leave + 1, steps):                    # refused calls leave the caller's vector alone
            assert np.array_equal(rows[0, j], rw.vector(seed, 0, r, j))
        assert info["slowest_call_s"] < 10
        assert info["destroy_rc"] == [rw.NCCL_SYSTEM_ERROR]
    _gone([name])


def test_a_rank_taken_twice_and_a_world_that_disagrees_are_errors(stub):
    ct = rw.ctypes
    hexid, name = rw.new_id(stub)
    raw = rw.as_id(hexid)
    c = ct.c_void_p()
    assert stub.ncclCommInitRank(ct.byref(c), 1, raw, 0) == 0                # a world of one joins at once
    n = ct.c_int(-1)
    assert stub.ncclCommCount(c, ct.byref(n)) == 0 and n.value == 1
    v = rw.vector(1, 0, 0, 0)
    keep = v.copy()
    assert stub.rccl_stub_host_allreduce(c, v.ctypes.data, 32) == 0 and np.array_equal(v, keep)
    assert stub.rccl_stub_host_allreduce(c, v.ctypes.data, 33) == rw.NCCL_INVALID_ARGUMENT
    c2 = ct.c_void_p()
    assert stub.ncclCommInitRank(ct.byref(c2), 2, raw, 1) == rw.NCCL_INVALID_ARGUMENT     # the world disagrees
    assert stub.rccl_stub_host_allreduce(c, v.ctypes.data, 32) == rw.NCCL_SYSTEM_ERROR    # ... and that is sticky
    stub.ncclCommDestroy(c)
    _gone([name])
    hexid, name = rw.new_id(stub)
    raw = rw.as_id(hexid)
    assert stub.ncclCommInitRank(ct.byref(c), 1, raw, 0) == 0
    assert stub.ncclCommInitRank(ct.byref(c2), 1, raw, 0) == rw.NCCL_INVALID_ARGUMENT     # rank 0 is taken
    stub.ncclCommDestroy(c)
    _gone([name])
    bad = rw.UniqueId()
    assert stub.ncclCommInitRank(ct.byref(c2), 1, bad, 0) == rw.NCCL_INVALID_ARGUMENT     # not an id of the stand-in
