"""The selected-elements segmented flagstat of int32 / int64 columns under graph capture: FLAGSTATS_hip_device_wide_segments_where
and segments_wide_where.count_segments_torch_ints_where captured with torch.cuda.graph in the store and the accumulate form,
replayed, then replayed again after the array, the selection, the offsets and the result words have been rewritten in place -- a
replay counts what the buffers hold then.  The entry keeps no workspace, so a graph holds no pointer of the library's."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_wide_where_oracle as swwo  # noqa: E402
from segments_wide_where_oracle import BITMAP, BYTES, pack, poison  # noqa: E402
from test_gpu_segments_wide_where import BIAS, GARBAGE, MASK_BIAS, SEL_BIAS, UNSIGNED, dev, dev64, err, expect, same, u64  # noqa: E402

pytestmark = pytest.mark.gpu

STORE, SUPERSET = 1, 2


@pytest.mark.parametrize("error_mode", ["global", "thread_local"])
@pytest.mark.parametrize("layer", ["entry", "torch"])
@pytest.mark.parametrize("mode", [STORE | SUPERSET, 0])
@pytest.mark.parametrize("W", [4, 8])
def test_graph_capture_and_replay(hip, W, mode, layer, error_mode):
    """one plain call, then the bitmap and the byte form captured in one graph (the store form's zeroing is part of it), replayed
    over fresh result words, array / selection / offsets rewritten, replayed again"""
    import torch
    from libflagstats_amd import segments_wide_where as sww
    rng = np.random.RandomState(83 + W)
    U = 8192 // W
    n = 30 * U + 7
    nseg = 6
    sets = []
    for k in range(2):
        mask = rng.randint(0, 100, n) < 30 + 40 * k
        x = rng.randint(0, 65536, n).astype(UNSIGNED[W])
        o = np.sort(np.concatenate([[3 + k], rng.randint(4, n - 5, nseg - 1), [n - 2 - k]])).astype(np.int64)
        picked = np.flatnonzero(mask)
        x[picked[picked > o[2]][17]] |= UNSIGNED[W](1 << (20 + 9 * k))
        x[~mask] = poison(W)
        sets.append((x, mask, o, swwo.want(x, o, mask, True)))
    assert not np.array_equal(sets[0][3][1], sets[1][3][1]) and not np.array_equal(sets[0][3][2], sets[1][3][2])
    t, d_off = dev(sets[0][0]), dev64(sets[0][2])
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
            sww.count_segments_torch_ints_where(t, d_off, d_bits, packed=True, bit_offset=3, out=rows[0], selected=sel[0], high=high[0],
                                                store=store, superset=superset)
            sww.count_segments_torch_ints_where(t, d_off, d_mask, out=rows[1], selected=sel[1], high=high[1], store=store, superset=superset)
            return 0
        rc = hip.FLAGSTATS_hip_device_wide_segments_where(t.data_ptr(), n, W, d_off.data_ptr(), nseg, d_bits.data_ptr(), 3, BITMAP,
                                                          rows[0].data_ptr(), sel[0].data_ptr(), high[0].data_ptr(), mode, stream)
        return rc or hip.FLAGSTATS_hip_device_wide_segments_where(t.data_ptr(), n, W, d_off.data_ptr(), nseg, d_mask.data_ptr(), 0, BYTES,
                                                                  rows[1].data_ptr(), sel[1].data_ptr(), high[1].data_ptr(), mode, stream)

    def refill():
        words[:, :nseg * 32] = GARBAGE if store else BIAS
        words[:, nseg * 32:nseg * 33] = GARBAGE if store else SEL_BIAS
        words[:, nseg * 33:] = GARBAGE if store else MASK_BIAS

    def check(want, what):
        for e in range(2):
            same((u64(rows[e]), u64(sel[e]), u64(high[e])), expect(want, mode), (W, mode, layer, error_mode, what, e))

    refill()
    torch.cuda.synchronize()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert call() == 0, err(hip)
    torch.cuda.synchronize()
    check(sets[0][3], "plain")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode=error_mode):
        rc = call()
    assert rc == 0, err(hip)
    torch.cuda.synchronize()
    for x, mask, o, want in (sets[0], sets[1], sets[0]):
        t.copy_(dev(x))
        d_bits.copy_(dev(pack(mask, 3, fill=1)))
        d_mask.copy_(dev(mask))
        d_off.copy_(dev64(o))
        refill()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        check(want, "replay")
    del g
