"""The filtered wide-input flagstat under samtools' whole FLAG predicate under graph capture: FLAGSTATS_hip_device_wide_filter_rf and
wide_filter_rf.count_torch_ints_filter_rf captured with torch.cuda.graph in the store and the accumulate form, with a predicate
that leaves a residue (fsk::flagstat_count_wide_filter_rf) and, in the store form, one that nothing can pass (no kernel is launched:
the graph holds the store form's zeroes alone; its += form queues nothing at all, and a graph without a node would test torch, not
this library), replayed, then replayed again after the column, the MAPQ bytes and the result words have
been rewritten in place -- a replay counts what the buffers hold then.  The entry keeps no workspace, so a graph holds no pointer of
the library's.

The columns are graphs_plan's wide slabs (data sets A and B of one size at one address: the edge shape's flags one element past a
16-byte line, high bits in the head edge step, the fast step and the tail edge step, surrounded by elements that pass everything
and carry every high bit) and its MAPQ slab; the expected values are wide_filter_rf_oracle's over the bodies."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphs_plan  # noqa: E402
import wide_filter_rf_oracle as wro  # noqa: E402
from test_gpu_wide_filter import BIAS, GARBAGE, HIGH_BIAS, SEL_BIAS, WIDTHS, err, expect_triple, u64  # noqa: E402

pytestmark = pytest.mark.gpu

STORE, SUPERSET = 1, 2
# (require, exclude, include_any, exclude_all) and what fsk_filter_rf_reduce answers
PREDICATES = {"residual": ((0x0001, 0x0900, 0x0050, 0x0420), 2), "empty": ((0x0001, 0x0950, 0x0050, 0x0420), 0)}


@pytest.mark.parametrize("layer", ["entry", "torch"])
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("predicate,mode", [("residual", STORE | SUPERSET), ("residual", 0), ("empty", STORE | SUPERSET)])
def test_graph_capture_and_replay(hip, oracle_mod, predicate, W, mode, layer):
    """one plain call, then the call captured in a graph, replayed over fresh result words, the buffers rewritten, replayed again"""
    import torch
    from libflagstats_amd import wide_filter_rf as wrf
    p, kind = PREDICATES[predicate]
    reduced = (ctypes.c_uint32 * 4)()
    assert hip.fsk_filter_rf_reduce(p[0], p[1], p[2], p[3], reduced) == kind
    plan = graphs_plan.plan(oracle_mod)
    column, mapq = plan.slabs["wide", W], plan.slabs["mapq"]
    n, mn = column.n, graphs_plan.MIN_MAPQ
    assert mapq.n == n and column.phase_bytes() == W
    wants = {ds: wro.want(oracle_mod, column.body(ds), *p, mapq.body(ds), mn, superset=True) for ds in graphs_plan.DATA_SETS}
    if kind:
        assert wants["A"][1] != wants["B"][1] and wants["A"][1] > 0 and wants["A"][2] != wants["B"][2] and wants["A"][2] and wants["B"][2]
    else:
        assert all(w[1] == 0 and w[2] == 0 and not w[0].any() for w in wants.values())
    dev = {ds: (torch.from_numpy(column.host(ds)).cuda(), torch.from_numpy(mapq.host(ds)).cuda()) for ds in graphs_plan.DATA_SETS}
    t_slab, q_slab = dev["A"][0].clone(), dev["A"][1].clone()
    t, q = t_slab[column.at:column.at + n], q_slab[mapq.at:mapq.at + n]
    assert t_slab.data_ptr() % 16 == 0 and t.data_ptr() % 16 == W and q.data_ptr() % 16 == graphs_plan.MAPQ_ALIGN
    words = torch.zeros(34, dtype=torch.int64, device="cuda")      # out[32], selected, high
    store, superset = bool(mode & STORE), bool(mode & SUPERSET)
    s = torch.cuda.Stream()
    stream = ctypes.c_void_p(s.cuda_stream)

    def call():
        if layer == "torch":
            wrf.count_torch_ints_filter_rf(t, require=p[0], exclude=p[1], include_any=p[2], exclude_all=p[3], mapq=q, min_mapq=mn,
                                           out=words[:32], selected=words[32:33], high=words[33:34], store=store, superset=superset)
            return 0
        w = words.data_ptr()
        return hip.FLAGSTATS_hip_device_wide_filter_rf(t.data_ptr(), n, W, p[0], p[1], p[2], p[3], q.data_ptr(), mn, w, w + 256, w + 264, mode,
                                                       stream)

    def refill():
        words[:32] = GARBAGE if store else BIAS
        words[32] = GARBAGE if store else SEL_BIAS
        words[33] = GARBAGE if store else HIGH_BIAS

    def same(want, what):
        assert np.array_equal(u64(words), expect_triple(want[0], want[1], want[2], mode)), (predicate, W, mode, layer, what, u64(words))

    refill()
    torch.cuda.synchronize()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert call() == 0, err(hip)
    torch.cuda.synchronize()
    same(wants["A"], "plain")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc = call()
    assert rc == 0, err(hip)
    torch.cuda.synchronize()
    for ds in ("A", "B", "A"):
        t_slab.copy_(dev[ds][0])
        q_slab.copy_(dev[ds][1])
        refill()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        same(wants[ds], "replay " + ds)
    del g
