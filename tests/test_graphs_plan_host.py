"""No GPU: what tests/test_gpu_graphs.py relies on in its inputs and expected values (tests/graphs_plan.py) -- the step geometry
of its two shapes, the alignments, that every predicate and selection passes between a quarter and three quarters of the elements
in both data sets, that the segment layouts hold what they are there for, and that the two data sets differ in every expected
row, so that a replay over data set B cannot pass with data set A's values."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphs_plan as gp  # noqa: E402
from segments_oracle import SEG_MIN_UNITS, SEG_UNIT  # noqa: E402


def test_plan_layout_fractions_and_differences(oracle_mod):
    p = gp.plan(oracle_mod)
    assert gp.plan(oracle_mod) is p                                  # built once, shared by every test of the process
    S = gp.S
    # --- the two shapes
    edge, grouped = gp.step_split("edge"), gp.step_split("grouped")
    assert (edge.n, edge.lo) == (2 * S + 100, 1) and edge.nsteps == 3 and edge.grid == 3
    assert edge.head_edge and edge.tail_edge and (edge.fast_begin, edge.fast_end) == (1, 2)
    assert [edge.pushes(b) for b in range(3)] == [[0], [1], [2]]
    assert (grouped.n, grouped.lo) == (100 * S + 77, 0) and grouped.nsteps == 101 and grouped.grid == 101
    assert not grouped.head_edge and grouped.tail_edge and (grouped.fast_begin, grouped.fast_end) == (0, 100)
    # the two-level epilogue's rule (fsk_launch): grid >= group_min_grid = 64, steps per workgroup <= group_max_steps = 40
    assert grouped.grid >= 64 and int(grouped.counts().max()) == 1 and edge.grid < 64
    assert 2 * (gp.PAD + 8 + grouped.n + gp.PAD) < 3.4e6            # the largest array, in bytes
    # --- alignments and surroundings
    for shape, (n, phase) in gp.SHAPES.items():
        for name in ("flags", "periodic"):
            slab = p.slabs[name, shape]
            assert slab.n == n and slab.phase_bytes() == 2 * phase and slab.a.size % 8 == 0
    assert p.slabs["mapq"].phase_bytes() == gp.MAPQ_ALIGN == 3 and p.slabs["sel", "bytes"].phase_bytes() == gp.SEL_ALIGN
    assert gp.BIT_OFFSET == 5 and p.slabs["sel", "bitmap"].n == (gp.BIT_OFFSET + edge.n + 7) // 8
    for W in gp.WIDTHS:
        assert p.slabs["wide", W].phase_bytes() == W and p.slabs["wide", W].n == edge.n
    for key, slab in p.slabs.items():
        if key == "offsets":
            continue
        for ds in gp.DATA_SETS:
            around = np.concatenate([slab.host(ds)[:slab.at], slab.host(ds)[slab.at + slab.n:]])
            assert slab.at >= gp.PAD and around.size >= 2 * gp.PAD and (around == around[0]).all(), key
            if slab.a.dtype == np.uint8:
                assert around[0] == 0xFF, key
            elif key[0] == "wide":
                assert gp.wfo.low16(around[:1])[0] == gp.BACKGROUND and gp.wfo.want_high(around[:1]) == gp.wfo.ALL_HIGH[key[1]], key
            else:
                assert around[0] in (gp.BACKGROUND, 0xFFFF), key
        assert not np.array_equal(slab.a, slab.b), key
    # the background passes the predicate and counts: one flag read outside [0, n) changes `selected` and several counters
    bg = np.array([gp.BACKGROUND], dtype=np.uint16)
    assert gp.filter_oracle.filter_mask(bg, gp.REQUIRE, gp.EXCLUDE).all() and oracle_mod.flagstat_c(bg).sum() >= 3
    # the bitmap's unused bits (below bit 5 of its first byte, above the last element's bit) are ones
    for ds in gp.DATA_SETS:
        bits = np.unpackbits(p.slabs["sel", "bitmap"].body(ds), bitorder="little")
        assert bits[:gp.BIT_OFFSET].all() and bits[gp.BIT_OFFSET + edge.n:].all()
        assert np.array_equal(bits[gp.BIT_OFFSET:gp.BIT_OFFSET + edge.n].astype(bool), p.masks["where"][ds])
        assert np.array_equal(p.slabs["sel", "bytes"].body(ds) != 0, p.masks["where"][ds])
        assert {0x00, 0x01, 0x02, 0x80, 0xFF} == set(p.slabs["sel", "bytes"].body(ds).tolist())
    # --- every predicate and selection passes between a quarter and three quarters, in both data sets -- overall and within
    # each of the three steps of the edge shape
    bounds = [0, S - 1, 2 * S - 1, edge.n]
    for key, masks in p.masks.items():
        for ds in gp.DATA_SETS:
            m = masks[ds]
            assert m.size == edge.n and 0.25 <= m.mean() <= 0.75, (key, ds, m.mean())
            for b, e in zip(bounds, bounds[1:]):
                assert 0.25 <= m[b:e].mean() <= 0.75, (key, ds, b, e)
            assert int(m.sum()) == int(p.want[key][ds]["selected"][0])
    assert not np.array_equal(p.masks["filter"]["A"], p.masks["filter_mapq"]["A"])
    # --- segments
    for ds in gp.DATA_SETS:
        o = p.slabs["offsets"].body(ds).astype(np.int64)
        lengths = np.diff(o)
        assert o.size == gp.NSEG + 1 == 41 and (lengths >= 0).all() and 0 < o[0] and o[-1] < edge.n
        assert (lengths == 0).sum() == 2 and {1, 2, 7, 63, 65} <= set(lengths.tolist())
        assert lengths.max() == gp.LONG_SEGMENT >= 3 * SEG_UNIT == 3 * 4096
        # at 32,868 flags every writer (wave) of the launch owns one unit at most, so the shipped policy (runs of at least two
        # whole units) never reaches the chain: the GPU tests capture under min_units = 1, where the long segment's whole units do
        assert SEG_MIN_UNITS == 2 and gp.chain_units(o, SEG_MIN_UNITS) == 0
        assert gp.chain_units(o, 1) >= 2           # a run of 3 * 4096 + 123 flags holds two or three whole units
        rows = p.want["segments"][ds]["out"]
        assert rows.shape == (gp.NSEG, 32) and not rows[lengths == 0].any() and rows[lengths >= 63].any(axis=1).all()
        frows, fsel = p.want["segments_filter"][ds]["out"], p.want["segments_filter"][ds]["selected"]
        assert frows.shape == (gp.NSEG, 32) and fsel.shape == (gp.NSEG,) and frows[lengths >= 63].any(axis=1).all()
        assert 0.25 * lengths.sum() <= fsel.sum() <= 0.75 * lengths.sum() and (fsel <= lengths).all()
    oa, ob = (p.slabs["offsets"].body(ds).astype(np.int64) for ds in gp.DATA_SETS)
    assert (oa != ob)[1:].all() and int(np.argmax(np.diff(oa))) != int(np.argmax(np.diff(ob)))
    assert set(np.nonzero(np.diff(oa) == 0)[0]).isdisjoint(np.nonzero(np.diff(ob) == 0)[0])
    # --- wide columns: a few elements above bit 15, one of them negative; `high` non-zero in A, another non-zero value in B
    for W in gp.WIDTHS:
        ha, hb = (int(p.want["wide", W][ds]["high"][0]) for ds in gp.DATA_SETS)
        assert ha and hb and ha != hb and ha >> (8 * W - 1) == 1 and hb >> (8 * W - 1) == 1
        for ds in gp.DATA_SETS:
            col = p.slabs["wide", W].body(ds)
            assert (col < 0).sum() == 1 and (gp.wfo.low16(col) == p.slabs["flags", "edge"].body(ds)).all()
            assert ((col >> 16) != 0).sum() == len(gp.HIGH_BITS[W, ds]) == 3
            assert int(p.want["wide_filter", W][ds]["high"][0]) == int(p.want["wide", W][ds]["high"][0])
            # the elements with high bits lie in the head edge step, the fast step and the tail edge step
            assert [int(np.searchsorted(bounds, at, side="right")) for at, _ in gp.HIGH_BITS[W, ds]] == [1, 2, 3]
    # --- expected values: no all-zero row, A and B differ in every row, the plain K1 row is oracle.flagstat_hist's
    for key, by_ds in p.want.items():
        for name in by_ds["A"]:
            a, b = by_ds["A"][name], by_ds["B"][name]
            assert a.dtype == np.uint64 and a.shape == b.shape, (key, name)
            for w in (a, b, gp.cut(a, False) if name == "out" and a.shape[-1] == 32 else a):
                assert w.any(), (key, name)
            if a.ndim == 2:
                assert (a != b).any(axis=1).all(), (key, name)
            elif a.size > 1:
                live = a.astype(bool) | b.astype(bool)
                assert live.sum() >= 16 and (a != b)[live].sum() >= live.sum() - 2, (key, name)
            else:
                assert a[0] != b[0], (key, name)
    for shape in gp.SHAPES:
        for ds in gp.DATA_SETS:
            assert np.array_equal(gp.cut(p.want["k1", shape][ds]["out"], False), p.want["hist", shape][ds]["out"])
            assert p.want["pospopcnt", shape][ds]["out"].shape == (16,)
            body = p.slabs["periodic", shape].body(ds)
            assert np.array_equal(p.want["pospopcnt", shape][ds]["out"], oracle_mod.pospopcnt_numpy(body).astype(np.uint64))
    # selected counts of the segments sum to the filtered count of the flags inside the segments
    for ds in gp.DATA_SETS:
        o = p.slabs["offsets"].body(ds).astype(np.int64)
        assert int(p.want["segments_filter"][ds]["selected"].sum()) == int(p.masks["filter_mapq"][ds][o[0]:o[-1]].sum())
