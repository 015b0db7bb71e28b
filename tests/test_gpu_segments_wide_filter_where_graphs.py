"""The filtered and selected segmented flagstat of int32 / int64 columns under graph capture:
FLAGSTATS_hip_device_wide_segments_filter_where and segments_wide_filter_where.count_segments_torch_ints_filter_where captured with
torch.cuda.graph on one stream in the store and the accumulate form, replayed, then replayed again after the array, the MAPQ
column, the selection, the offsets and the result words have been rewritten in place -- a replay counts what the buffers hold
then.  The entry keeps no workspace, so a graph holds no pointer of the library's."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_wide_filter_where_oracle as swfwo  # noqa: E402
from segments_wide_where_oracle import BITMAP, BYTES, pack  # noqa: E402
from test_gpu_segments_wide_filter_where import F904Q30, scene  # noqa: E402
from test_gpu_segments_wide_where import BIAS, GARBAGE, MASK_BIAS, SEL_BIAS, dev, dev64, err, expect, same, u64  # noqa: E402

pytestmark = pytest.mark.gpu

STORE, SUPERSET = 1, 2


@pytest.mark.parametrize("layer", ["entry", "torch"])
@pytest.mark.parametrize("mode", [STORE | SUPERSET, 0])
@pytest.mark.parametrize("W", [4, 8])
def test_graph_capture_and_replay(hip, W, mode, layer):
    """one plain call, then the bitmap and the byte form captured in one graph on one stream (the store form's zeroing is part of
    it); the replay's results equal the eager ones; array / MAPQ / selection / offsets rewritten in place, replayed again: the
    oracle's"""
    import torch
    from libflagstats_amd import segments_wide_filter_where as swfw
    rng = np.random.RandomState(89 + W)
    U = 8192 // W
    n = 30 * U + 7
    nseg = 6
    req, exc, mq = F904Q30
    sets = []
    for k in range(2):
        mask = rng.randint(0, 100, n) < 30 + 40 * k
        o = np.sort(np.concatenate([[3 + k], rng.randint(4, n - 5, nseg - 1), [n - 2 - k]])).astype(np.int64)
        x, sel_set, q = scene(rng, n, W, o, mask, F904Q30, hot_every=5 + 900 * k)
        sets.append((x, sel_set, q, o, swfwo.want(x, o, mask, req, exc, q, mq, True)))
    assert not np.array_equal(sets[0][4][1], sets[1][4][1]) and not np.array_equal(sets[0][4][2], sets[1][4][2])
    t, d_q, d_off = dev(sets[0][0]), dev(sets[0][2]), dev64(sets[0][3])
    d_bits, d_mask = dev(pack(sets[0][1], 3, fill=1)), dev(sets[0][1])
    words = torch.zeros((2, nseg * 34), dtype=torch.int64, device="cuda")      # per encoding: rows, counts, masks
    rows = [words[e, :nseg * 32].view(nseg, 32) for e in range(2)]
    sel = [words[e, nseg * 32:nseg * 33] for e in range(2)]
    high = [words[e, nseg * 33:] for e in range(2)]
    store, superset = bool(mode & STORE), bool(mode & SUPERSET)
    s = torch.cuda.Stream()
    stream = ctypes.c_void_p(s.cuda_stream)

    def call():
        if layer == "torch":
            kw = dict(require=req, exclude=exc, mapq=d_q, min_mapq=mq, store=store, superset=superset)
            swfw.count_segments_torch_ints_filter_where(t, d_off, d_bits, packed=True, bit_offset=3, out=rows[0], selected=sel[0], high=high[0], **kw)
            swfw.count_segments_torch_ints_filter_where(t, d_off, d_mask, out=rows[1], selected=sel[1], high=high[1], **kw)
            return 0
        f = hip.FLAGSTATS_hip_device_wide_segments_filter_where
        rc = f(t.data_ptr(), n, W, d_off.data_ptr(), nseg, req, exc, d_q.data_ptr(), mq, d_bits.data_ptr(), 3, BITMAP, rows[0].data_ptr(),
               sel[0].data_ptr(), high[0].data_ptr(), mode, stream)
        return rc or f(t.data_ptr(), n, W, d_off.data_ptr(), nseg, req, exc, d_q.data_ptr(), mq, d_mask.data_ptr(), 0, BYTES, rows[1].data_ptr(),
                       sel[1].data_ptr(), high[1].data_ptr(), mode, stream)

    def refill():
        words[:, :nseg * 32] = GARBAGE if store else BIAS
        words[:, nseg * 32:nseg * 33] = GARBAGE if store else SEL_BIAS
        words[:, nseg * 33:] = GARBAGE if store else MASK_BIAS

    def check(want, what):
        for e in range(2):
            same((u64(rows[e]), u64(sel[e]), u64(high[e])), expect(want, mode), (W, mode, layer, what, e))

    refill()
    torch.cuda.synchronize()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert call() == 0, err(hip)
    torch.cuda.synchronize()
    check(sets[0][4], "plain")
    eager = words.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc = call()
    assert rc == 0, err(hip)
    torch.cuda.synchronize()
    for i, (x, sel_set, q, o, want) in enumerate((sets[0], sets[1], sets[0])):
        t.copy_(dev(x))
        d_q.copy_(dev(q))
        d_bits.copy_(dev(pack(sel_set, 3, fill=1)))
        d_mask.copy_(dev(sel_set))
        d_off.copy_(dev64(o))
        refill()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        if i == 0:
            assert torch.equal(words, eager)             # the replay's results equal the eager ones
        check(want, "replay")
    del g
