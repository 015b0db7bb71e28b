"""The filtered flagstat under a selection under graph capture: FLAGSTATS_hip_device_u16_filter_where and
filter_where.count_torch_filter_where captured with torch.cuda.graph in the store and the accumulate form, in each of the six
kernel forms, replayed, then replayed again after the flags, the MAPQ column, the selection and the result words have been
rewritten in place -- a replay counts what the buffers hold then.  The entry keeps no workspace, so a graph holds no pointer of
the library's; the store form's zeroes are part of the graph."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from filter_where_oracle import want_counters  # noqa: E402
from test_gpu_where import BIAS, GARBAGE, SEL_BIAS, S, dev8, dev16, err, expect_row, u64  # noqa: E402
from where_oracle import BITMAP, BYTES, pack  # noqa: E402

pytestmark = pytest.mark.gpu

STORE, SUPERSET = 1, 2
FORMS = ("bitmap", "funnel", "bytes")             # the array starts on a 16-byte boundary: bit offset 0 is not funnelled, 3 is
BIT_OFFSET = {"bitmap": 0, "funnel": 3}


@pytest.mark.parametrize("layer", ["entry", "torch"])
@pytest.mark.parametrize("mode", [STORE | SUPERSET, 0])
@pytest.mark.parametrize("mq", [False, True])
def test_graph_capture_and_replay(hip, oracle_mod, mq, mode, layer):
    """one plain call of the three selection forms, then the three captured in one graph, replayed over fresh result words, the
    buffers rewritten, replayed again"""
    import torch
    from libflagstats_amd import filter_where as fw
    rng = np.random.RandomState(83 + mq)
    n = 3 * S + 7
    require, exclude, mn = 0x1, 0x904, (30 if mq else 0)
    sets = []
    for k in range(2):
        values = rng.randint(0, 65536, n).astype(np.uint16)
        mapq = rng.randint(0, 61, n).astype(np.uint8)
        mask = rng.randint(0, 100, n) < 30 + 40 * k
        sets.append((values, mapq, mask, want_counters(oracle_mod, values, mask, require, exclude, mapq, mn, superset=True)))
    assert sets[0][3][1] != sets[1][3][1] and sets[0][3][1] > 0
    t, q = dev16(sets[0][0]), dev8(sets[0][1])
    assert t.data_ptr() % 16 == 0
    d_sel = {"bitmap": dev8(pack(sets[0][2], 0, fill=1)), "funnel": dev8(pack(sets[0][2], 3, fill=1)),
             "bytes": torch.from_numpy(sets[0][2]).cuda()}
    words = torch.zeros((3, 33), dtype=torch.int64, device="cuda")      # per form: out[32], selected
    store, superset = bool(mode & STORE), bool(mode & SUPERSET)
    s = torch.cuda.Stream()
    stream = ctypes.c_void_p(s.cuda_stream)

    def call():
        for i, form in enumerate(FORMS):
            if layer == "torch":
                fw.count_torch_filter_where(t, d_sel[form], require=require, exclude=exclude, mapq=q if mq else None, min_mapq=mn,
                                            packed=form != "bytes", bit_offset=BIT_OFFSET.get(form, 0), out=words[i, :32],
                                            selected=words[i, 32:33], store=store, superset=superset)
                continue
            p = words[i].data_ptr()
            rc = hip.FLAGSTATS_hip_device_u16_filter_where(t.data_ptr(), n, require, exclude, q.data_ptr() if mq else None, mn,
                                                           d_sel[form].data_ptr(), BIT_OFFSET.get(form, 0), BYTES if form == "bytes" else BITMAP,
                                                           p, p + 256, mode, stream)
            if rc:
                return rc
        return 0

    def refill():
        words[:, :32] = GARBAGE if store else BIAS
        words[:, 32] = GARBAGE if store else SEL_BIAS

    def same(want, what):
        for i, form in enumerate(FORMS):
            got = u64(words[i])
            assert np.array_equal(got[:32], expect_row(want[0], mode)), (mq, mode, layer, what, form)
            assert int(got[32]) == want[1] + (0 if store else SEL_BIAS), (mq, mode, layer, what, form)

    refill()
    torch.cuda.synchronize()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert call() == 0, err(hip)
    torch.cuda.synchronize()
    same(sets[0][3], "plain")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc = call()
    assert rc == 0, err(hip)
    torch.cuda.synchronize()
    for values, mapq, mask, want in (sets[0], sets[1], sets[0]):
        t.copy_(dev16(values))
        q.copy_(dev8(mapq))
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
