"""The filtered segmented flagstat under samtools' whole FLAG predicate under graph capture: FLAGSTATS_hip_device_u16_segments_filter_rf
captured with torch.cuda.graph on a stream of its own, for a predicate that nothing can pass (no kernel: the store form's zeroes
alone, nothing at all in the += form), one that reduces to a plain pair (the parent's kernel) and one that leaves a residue
(fsk::flagstat_segments_filter_rf), in the store and the += form -- replayed, then replayed again after the array, the MAPQ bytes
and the result words have been rewritten in place: a replay counts what the buffers hold then.  The entry keeps no workspace, so a
graph holds no pointer of the library's.

The captured work is one chain on one stream: a one-element add in front of the entry's call, so that the graph of the call that
queues nothing still has a node, and whatever the entry queues behind it.  Expected values are segments_filter_rf_oracle's."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_filter_rf_oracle as sfro  # noqa: E402
from segments_oracle import SEG_UNIT  # noqa: E402
from test_gpu_segments_filter import BIAS, GARBAGE, SEL_BIAS, dev8, dev16, dev64, err, expect  # noqa: E402

pytestmark = pytest.mark.gpu

U = SEG_UNIT
STORE, SUPERSET = 1, 2
MIN_MAPQ = 30
# (require, exclude, include_any, exclude_all) and the reduction's answer (pinned by tests/test_segments_filter_rf_host.py)
PREDICATES = {"nothing passes": ((0, 0x904, 0x900, 0), 0), "plain pair": ((0, 0x904, 0x40, 0), 1), "residue": ((0x1, 0x804, 0x110, 0x2200), 2)}


@pytest.mark.parametrize("mode", [STORE | SUPERSET, 0])
@pytest.mark.parametrize("predicate", list(PREDICATES))
def test_graph_capture_and_replay(hip, predicate, mode):
    """one plain call, then the call captured in a graph, replayed over fresh result words, the buffers rewritten, replayed again"""
    import torch
    p, kind = PREDICATES[predicate]
    reduced = (ctypes.c_uint32 * 4)()
    assert hip.fsk_filter_rf_reduce(p[0], p[1], p[2], p[3], reduced) == kind
    n = 7 * U + 77                            # chain runs and per-flag units, the array one flag into a 16-byte line
    o = np.array([3, 3, 500, U + 9, 5 * U - 1, 6 * U, n - 2], dtype=np.int64)
    nseg = o.size - 1
    data, wants = {}, {}
    for ds, seed in (("A", 61), ("B", 62)):
        rng = np.random.RandomState(seed)
        values = rng.randint(0, 65536, n).astype(np.uint16)
        mapq = rng.randint(0, 61, n).astype(np.uint8)
        data[ds] = (dev16(values), dev8(mapq))
        wants[ds] = sfro.want(values, o, *p, mapq, MIN_MAPQ, superset=True)
    if kind:
        assert wants["A"][1][0] == 0 and (wants["A"][1][1:] > 0).all()        # (the first segment is empty)
        assert (wants["A"][1] != wants["B"][1]).any()
    else:
        assert not any(w[0].any() or w[1].any() for w in wants.values())
    t_slab = torch.zeros(8 + n + 8, dtype=torch.int16, device="cuda")
    q_slab = torch.zeros(16 + n + 16, dtype=torch.uint8, device="cuda")
    t, q = t_slab[1:1 + n], q_slab[3:3 + n]
    assert t.data_ptr() % 16 == 2 and q.data_ptr() % 16 == 3
    d_off = dev64(o)
    words = torch.zeros(nseg * 33, dtype=torch.int64, device="cuda")
    ticks = torch.zeros(1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    stream = ctypes.c_void_p(s.cuda_stream)

    def call():
        ticks.add_(1)
        w = words.data_ptr()
        return hip.FLAGSTATS_hip_device_u16_segments_filter_rf(t.data_ptr(), n, d_off.data_ptr(), nseg, p[0], p[1], p[2], p[3], q.data_ptr(),
                                                               MIN_MAPQ, w, w + nseg * 256, mode, stream)

    def refill(ds):
        t.copy_(data[ds][0])
        q.copy_(data[ds][1])
        words[:nseg * 32] = GARBAGE if mode & STORE else BIAS
        words[nseg * 32:] = GARBAGE if mode & STORE else SEL_BIAS

    def same(ds, what):
        rows, sel = expect(wants[ds][0], wants[ds][1], mode)
        got = words.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:nseg * 32].reshape(nseg, 32), rows) and np.array_equal(got[nseg * 32:], sel), (predicate, mode, what)

    refill("A")
    torch.cuda.synchronize()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert call() == 0, err(hip)
    torch.cuda.synchronize()
    same("A", "plain")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc = call()
    assert rc == 0, err(hip)
    torch.cuda.synchronize()
    assert int(ticks[0]) == 1                 # a captured call runs nothing
    for i, ds in enumerate(("A", "B", "A")):
        refill(ds)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        assert int(ticks[0]) == 2 + i
        same(ds, "replay " + ds)
    del g
