"""The filtered and selected segmented flagstat under graph capture: FLAGSTATS_hip_device_u16_segments_filter_where and
segments_filter_where.count_segments_torch_filter_where captured with torch.cuda.graph in the store and the accumulate form, in
the five kernel forms and the dispatched one (a byte mask without -q), replayed, then replayed again after the flags, the MAPQ
column, the selection, the offsets and the result words have been rewritten in place -- a replay counts what the buffers hold
then.  The entry keeps no workspace, so a graph holds no pointer of the library's; the store form's zeroes are part of the graph.
The launches of a graph follow one another on one stream: its branches are sequential."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_filter_where_oracle as sfwo  # noqa: E402
from segments_where_oracle import BITMAP, BYTES, pack  # noqa: E402
from test_gpu_segments_where import BIAS, GARBAGE, SEL_BIAS, STORE, SUPERSET, U, dev8, dev16, dev64, err, expect, u64  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = ("bitmap", "funnel", "bytes")             # the array starts on a 16-byte boundary: bit offset 0 is not funnelled, 3 is
BIT_OFFSET = {"bitmap": 0, "funnel": 3}


@pytest.mark.parametrize("layer", ["entry", "torch"])
@pytest.mark.parametrize("mode", [STORE | SUPERSET, 0])
@pytest.mark.parametrize("mq", [False, True])
def test_graph_capture_and_replay(hip, mq, mode, layer):
    """one plain call of the three selection forms (with -q: the unit's three kernels with the column; without: its two bitmap
    kernels and the dispatched byte form), then the three captured in one graph, replayed over fresh result words, the buffers
    rewritten, replayed again.  30 units and six segments: per-flag pieces and chain runs"""
    import torch
    from libflagstats_amd import segments_filter_where as sfw
    rng = np.random.RandomState(91 + mq)
    n = 30 * U + 7
    nseg = 6
    require, exclude, mn = 0x1, 0x904, (30 if mq else 0)
    sets = []
    for k in range(2):
        values = rng.randint(0, 65536, n).astype(np.uint16)
        values[::2] &= np.uint16(0xF6FB)
        mapq = rng.randint(0, 61, n).astype(np.uint8)
        mask = rng.randint(0, 100, n) < 30 + 40 * k
        o = np.sort(np.concatenate([[3 + k], rng.randint(4, n - 5, nseg - 1), [n - 2 - k]])).astype(np.int64)
        sets.append((values, mapq, mask, o, sfwo.want(values, o, mask, require, exclude, mapq, mn, superset=True)))
    assert not np.array_equal(sets[0][4][1], sets[1][4][1]) and sets[0][4][1].any()
    t, q, d_off = dev16(sets[0][0]), dev8(sets[0][1]), dev64(sets[0][3])
    assert t.data_ptr() % 16 == 0
    d_sel = {"bitmap": dev8(pack(sets[0][2], 0, fill=1)), "funnel": dev8(pack(sets[0][2], 3, fill=1)),
             "bytes": torch.from_numpy(sets[0][2]).cuda()}
    rows = torch.zeros((3, nseg, 32), dtype=torch.int64, device="cuda")
    cnt = torch.zeros((3, nseg), dtype=torch.int64, device="cuda")
    store, superset = bool(mode & STORE), bool(mode & SUPERSET)
    s = torch.cuda.Stream()
    stream = ctypes.c_void_p(s.cuda_stream)

    def call():
        for i, form in enumerate(FORMS):
            if layer == "torch":
                sfw.count_segments_torch_filter_where(t, d_off, d_sel[form], require=require, exclude=exclude, mapq=q if mq else None,
                                                      min_mapq=mn, packed=form != "bytes", bit_offset=BIT_OFFSET.get(form, 0), out=rows[i],
                                                      selected=cnt[i], store=store, superset=superset)
                continue
            rc = hip.FLAGSTATS_hip_device_u16_segments_filter_where(t.data_ptr(), n, d_off.data_ptr(), nseg, require, exclude,
                                                                    q.data_ptr() if mq else None, mn, d_sel[form].data_ptr(),
                                                                    BIT_OFFSET.get(form, 0), BYTES if form == "bytes" else BITMAP,
                                                                    rows[i].data_ptr(), cnt[i].data_ptr(), mode, stream)
            if rc:
                return rc
        return 0

    def refill():
        rows.fill_(GARBAGE if store else BIAS)
        cnt.fill_(GARBAGE if store else SEL_BIAS)

    def same(want, what):
        w_rows, w_sel = expect(want[0], want[1], mode)
        for i, form in enumerate(FORMS):
            assert np.array_equal(u64(rows[i]), w_rows) and np.array_equal(u64(cnt[i]), w_sel), (mq, mode, layer, what, form)

    refill()
    torch.cuda.synchronize()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert call() == 0, err(hip)
    torch.cuda.synchronize()
    same(sets[0][4], "plain")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc = call()
    assert rc == 0, err(hip)
    torch.cuda.synchronize()
    for values, mapq, mask, o, want in (sets[0], sets[1], sets[0]):
        t.copy_(dev16(values))
        q.copy_(dev8(mapq))
        d_off.copy_(dev64(o))
        d_sel["bitmap"].copy_(dev8(pack(mask, 0, fill=1)))
        d_sel["funnel"].copy_(dev8(pack(mask, 3, fill=1)))
        d_sel["bytes"].copy_(torch.from_numpy(mask).cuda())
        refill()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        same(want, "replay")
    del g
