"""The filtered and selected flagstat of int32 / int64 columns under graph capture: FLAGSTATS_hip_device_wide_filter_where and
wide_filter_where.count_torch_ints_filter_where captured with torch.cuda.graph in the store and the accumulate form, replayed,
then replayed again after the array, the MAPQ column, the selection and the result words have been rewritten in place -- a replay
counts what the buffers hold then.  The entry keeps no workspace, so a graph holds no pointer of the library's."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_filter_where_oracle as wfwo  # noqa: E402
from test_gpu_wide_filter import (ALL_HIGH, BIAS, GARBAGE, HIGH_BIAS, SEL_BIAS, STEP, UNSIGNED, dev8, err, expect_triple, to_device,  # noqa: E402
                                  u64)
from wide_where_oracle import BITMAP, BYTES, pack  # noqa: E402

pytestmark = pytest.mark.gpu

STORE, SUPERSET = 1, 2
REQUIRE, EXCLUDE, MIN_MAPQ = 0x0002, 0x0904, 30


@pytest.mark.parametrize("error_mode", ["global", "thread_local"])
@pytest.mark.parametrize("layer", ["entry", "torch"])
@pytest.mark.parametrize("mode", [STORE | SUPERSET, 0])
@pytest.mark.parametrize("W", [4, 8])
def test_graph_capture_and_replay(hip, oracle_mod, W, mode, layer, error_mode):
    """one plain call, then the bitmap and the byte form captured in one graph (the store form's zeroes are part of it), replayed
    over fresh result words, the buffers rewritten, replayed again.  Elements that are not selected pass the predicate and carry
    every high bit; one selected element that fails carries a high bit of its own"""
    import torch
    from libflagstats_amd import wide_filter_where
    rng = np.random.RandomState(89 + W)
    n = 3 * STEP[W] + 7
    sets = []
    for k in range(2):
        mask = rng.randint(0, 100, n) < 30 + 40 * k
        column = rng.randint(0, 65536, n).astype(UNSIGNED[W])
        mapq = rng.randint(20, 41, n).astype(np.uint8)
        failing = np.flatnonzero(mask & ((column & UNSIGNED[W](EXCLUDE)) != 0))[17]
        column[failing] |= UNSIGNED[W](1 << (20 + 9 * k))
        column[~mask] = UNSIGNED[W](ALL_HIGH[W] | 0x0043)
        mapq[~mask] = 255
        sets.append((column, mask, mapq, wfwo.want(oracle_mod, column, mask, REQUIRE, EXCLUDE, mapq, MIN_MAPQ, superset=True)))
    assert sets[0][3][1] != sets[1][3][1] and sets[0][3][2] != sets[1][3][2] and 0 < sets[0][3][1] < int(sets[0][1].sum())
    t = to_device(sets[0][0])
    d_mapq = dev8(sets[0][2])
    d_bits, d_mask = dev8(pack(sets[0][1], 3, fill=1)), torch.from_numpy(sets[0][1]).cuda()
    words = torch.zeros((2, 34), dtype=torch.int64, device="cuda")      # per encoding: out[32], selected, high
    store, superset = bool(mode & STORE), bool(mode & SUPERSET)
    s = torch.cuda.Stream()
    stream = ctypes.c_void_p(s.cuda_stream)

    def call():
        if layer == "torch":
            for k, (where, kw) in enumerate(((d_bits, {"packed": True, "bit_offset": 3}), (d_mask, {}))):
                wide_filter_where.count_torch_ints_filter_where(t, where, require=REQUIRE, exclude=EXCLUDE, mapq=d_mapq, min_mapq=MIN_MAPQ,
                                                                out=words[k, :32], selected=words[k, 32:33], high=words[k, 33:34],
                                                                store=store, superset=superset, **kw)
            return 0
        p0, p1 = words[0].data_ptr(), words[1].data_ptr()
        f = hip.FLAGSTATS_hip_device_wide_filter_where
        rc = f(t.data_ptr(), n, W, REQUIRE, EXCLUDE, d_mapq.data_ptr(), MIN_MAPQ, d_bits.data_ptr(), 3, BITMAP, p0, p0 + 256, p0 + 264, mode,
               stream)
        return rc or f(t.data_ptr(), n, W, REQUIRE, EXCLUDE, d_mapq.data_ptr(), MIN_MAPQ, d_mask.data_ptr(), 0, BYTES, p1, p1 + 256, p1 + 264,
                       mode, stream)

    def refill():
        words[:, :32] = GARBAGE if store else BIAS
        words[:, 32] = GARBAGE if store else SEL_BIAS
        words[:, 33] = GARBAGE if store else HIGH_BIAS

    def same(want, what):
        for enc in range(2):
            assert np.array_equal(u64(words[enc]), expect_triple(want[0], want[1], want[2], mode)), (W, mode, layer, error_mode, what, enc)

    refill()
    torch.cuda.synchronize()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert call() == 0, err(hip)
    torch.cuda.synchronize()
    same(sets[0][3], "plain")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode=error_mode):
        rc = call()
    assert rc == 0, err(hip)
    torch.cuda.synchronize()
    for column, mask, mapq, want in (sets[0], sets[1], sets[0]):
        t.copy_(to_device(column))
        d_mapq.copy_(dev8(mapq))
        d_bits.copy_(dev8(pack(mask, 3, fill=1)))
        d_mask.copy_(torch.from_numpy(mask).cuda())
        refill()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        same(want, "replay")
    del g
