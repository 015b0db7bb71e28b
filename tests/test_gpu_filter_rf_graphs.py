"""The filtered flagstat under samtools' whole FLAG predicate under graph capture: FLAGSTATS_hip_device_u16_filter_rf and
filter_rf.count_torch_filter_rf captured with torch.cuda.graph in the store and the accumulate form, with a predicate that leaves
a residue (fsk::flagstat_count_filter_rf) and one the launcher reduces to a pair (fsk::flagstat_count_filter), replayed, then
replayed again after the flags, the MAPQ column and the result words have been rewritten in place -- a replay counts what the
buffers hold then.  The entry keeps no workspace, so a graph holds no pointer of the library's; the store form's zeroes are part of
the graph."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from filter_rf_oracle import want_counters  # noqa: E402
from test_gpu_where import BIAS, GARBAGE, SEL_BIAS, S, dev8, dev16, err, expect_row, u64  # noqa: E402

pytestmark = pytest.mark.gpu

STORE, SUPERSET = 1, 2
# (require, exclude, include_any, exclude_all) and what fsk_filter_rf_reduce answers
PREDICATES = {"residual": ((0x0001, 0x0904, 0x0050, 0x0420), 2), "reduced": ((0x0001, 0x0904, 0x0040, 0x000C), 1)}


@pytest.mark.parametrize("layer", ["entry", "torch"])
@pytest.mark.parametrize("mode", [STORE | SUPERSET, 0])
@pytest.mark.parametrize("mq", [False, True])
@pytest.mark.parametrize("predicate", sorted(PREDICATES))
def test_graph_capture_and_replay(hip, oracle_mod, predicate, mq, mode, layer):
    """one plain call, then the call captured in a graph, replayed over fresh result words, the buffers rewritten, replayed again"""
    import torch
    from libflagstats_amd import filter_rf as rf
    p, kind = PREDICATES[predicate]
    reduced = (ctypes.c_uint32 * 4)()
    assert hip.fsk_filter_rf_reduce(p[0], p[1], p[2], p[3], reduced) == kind
    rng = np.random.RandomState(87 + mq)
    n = 3 * S + 7
    mn = 30 if mq else 0
    sets = []
    for k in range(2):
        values = rng.randint(0, 65536, n).astype(np.uint16)
        values[rng.randint(0, 100, n) < 20 + 40 * k] &= np.uint16(~p[1] & 0xFFFF)      # more of B's flags pass than of A's
        mapq = rng.randint(0, 61, n).astype(np.uint8)
        sets.append((values, mapq, want_counters(oracle_mod, values, *p, mapq, mn, superset=True)))
    assert sets[0][2][1] != sets[1][2][1] and sets[0][2][1] > 0
    t, q = dev16(sets[0][0]), dev8(sets[0][1])
    assert t.data_ptr() % 16 == 0
    words = torch.zeros(33, dtype=torch.int64, device="cuda")      # out[32], selected
    store, superset = bool(mode & STORE), bool(mode & SUPERSET)
    s = torch.cuda.Stream()
    stream = ctypes.c_void_p(s.cuda_stream)

    def call():
        if layer == "torch":
            rf.count_torch_filter_rf(t, require=p[0], exclude=p[1], include_any=p[2], exclude_all=p[3], mapq=q if mq else None, min_mapq=mn,
                                     out=words[:32], selected=words[32:33], store=store, superset=superset)
            return 0
        w = words.data_ptr()
        return hip.FLAGSTATS_hip_device_u16_filter_rf(t.data_ptr(), n, p[0], p[1], p[2], p[3], q.data_ptr() if mq else None, mn, w, w + 256,
                                                      mode, stream)

    def refill():
        words[:32] = GARBAGE if store else BIAS
        words[32] = GARBAGE if store else SEL_BIAS

    def same(want, what):
        got = u64(words)
        assert np.array_equal(got[:32], expect_row(want[0], mode)), (predicate, mq, mode, layer, what)
        assert int(got[32]) == want[1] + (0 if store else SEL_BIAS), (predicate, mq, mode, layer, what)

    refill()
    torch.cuda.synchronize()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert call() == 0, err(hip)
    torch.cuda.synchronize()
    same(sets[0][2], "plain")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc = call()
    assert rc == 0, err(hip)
    torch.cuda.synchronize()
    for values, mapq, want in (sets[0], sets[1], sets[0]):
        t.copy_(dev16(values))
        q.copy_(dev8(mapq))
        refill()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        same(want, "replay")
    del g
