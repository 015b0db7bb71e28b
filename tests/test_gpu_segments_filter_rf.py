"""The filtered segmented flagstat under samtools' whole FLAG predicate on the MI355X: fsk::flagstat_segments_filter_rf in its six
instantiations, the launcher's three kinds of call, the three C entries and libflagstats_amd/segments_filter_rf.py.  Every
comparison is exact.

Expected rows never come from the code under test: segments_filter_rf_oracle.want is segments_oracle.segmented_counters of the
array with the failing flags zeroed (filter_rf_oracle.view_mask), slot 9 from the definition; the expected `selected` is the
per-segment sum of the mask.  Large inputs are periodic (one prime period for flags and MAPQ) and use the oracle's periodic form.
Layouts are placed with segments_oracle.WriterSplit, the launcher's work split mirrored, and checked to contain the runs they are
for.  The helpers (Batch: rows and counts prefilled with garbage or a bias, one upload and one read-back) are the parent's test's."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_filter_oracle as sfo  # noqa: E402
import segments_filter_rf_oracle as sfro  # noqa: E402
from filter_rf_oracle import view_mask  # noqa: E402
from segments_oracle import SEG_EPOCH, SEG_UNIT, writer_ranges  # noqa: E402
from test_gpu_segments_filter import (BIAS, EVERY_MIN_UNITS, GARBAGE, LENGTHS, MODES, N_EPOCHS, SEL_BIAS, Batch, P, dev8, dev16,  # noqa: E402
                                      dev64, epochs_layout, err, expect, geometry_offsets, get_policy, periodic_tensors, policy)

pytestmark = pytest.mark.gpu

U = SEG_UNIT
STORE, SUPERSET = 1, 2
P_ANY, P_ALL, P_BOTH = (0, 0x0904, 0x0050, 0), (0, 0x0904, 0, 0x0420), (0x0001, 0x0804, 0x0110, 0x2200)   # residues (the host test pins them)
AROUND = 0xFFFF & ~0x0904 & ~0x0020           # a flag that passes P_ANY and P_ALL: what lies around the arrays


@pytest.fixture(scope="module")
def launcher(hip):
    hip.fsk_segments_policy.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    hip.fsk_segments_policy.restype = None
    hip.fsk_set_segments_policy.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    hip.fsk_set_segments_policy.restype = None
    return hip.fsk_launch_segments_filter_rf


def kind_of(hip, p):
    out = (ctypes.c_uint32 * 4)()
    return hip.fsk_filter_rf_reduce(p[0], p[1], p[2], p[3], out), tuple(out)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------ 1. every value under every kind of predicate
_EVERY = {}


def every_value_case():
    """the input, its device copies and the expected rows and counts of every predicate: made once, shared, left unchanged"""
    if not _EVERY:
        values, o = sfro.every_value_input()
        _EVERY.update(values=values, o=o, t=dev16(values), d_off=dev64(o),
                      wants={p: sfro.want(values, o, *p, superset=True) for p in sfro.PREDICATES})
    return _EVERY["values"], _EVERY["o"], _EVERY["t"], _EVERY["d_off"], _EVERY["wants"]


@pytest.mark.parametrize("form", ["device", "sync", "host"])
def test_every_value_under_every_kind_of_predicate(hip, launcher, form):
    """0..65535 once each, shuffled (16 units), cut into segments of coprime lengths with empty ones, under every two-bit
    include_any and every two-bit exclude_all (both bits in one byte plane, one in each) and the eleven named predicates (residues,
    plain pairs, nothing passes) -- through the device entry, the _sync form and the host form, with and without `selected`, in
    the store + superset form and the += form"""
    values, o, t, d_off, wants = every_value_case()
    n, nseg = values.size, o.size - 1
    named = [q for q, _, _ in sfro.TABLE]
    for p, kind, _ in sfro.TABLE:
        assert kind_of(hip, p)[0] == kind and bool(wants[p][1].any()) == (kind != 0), p
    if form == "device":
        batch = Batch()
        plan = []
        for i, p in enumerate(sfro.PREDICATES):
            plan.append((p, STORE | SUPERSET, batch.add(STORE | SUPERSET, *wants[p], ("device", p, "store"), with_selected=i % 2 == 0)))
            plan.append((p, 0, batch.add(0, *wants[p], ("device", p, "+="), with_selected=i % 2 == 1)))
        batch.upload()
        for p, mode, k in plan:
            rc = hip.FLAGSTATS_hip_device_u16_segments_filter_rf(t.data_ptr(), n, d_off.data_ptr(), nseg, p[0], p[1], p[2], p[3], None, 0,
                                                                 batch.out(k), batch.selected(k), mode, None)
            assert rc == 0, (p, mode, err(hip))
        batch.check()
        return
    entry, src = ((hip.FLAGSTATS_hip_device_u16_segments_filter_rf_sync, t.data_ptr()) if form == "sync" else
                  (hip.FLAGSTATS_hip_u16_x64_segments_filter_rf, values.ctypes.data))
    for i, p in enumerate(sfro.PREDICATES):
        for mode in ((STORE | SUPERSET, 0) if p in named else ((STORE | SUPERSET, 0)[i % 2],)):
            rows = np.full((nseg, 32), GARBAGE if mode & STORE else BIAS, dtype=np.uint64)
            sel = np.full(nseg, GARBAGE if mode & STORE else SEL_BIAS, dtype=np.uint64)
            with_selected = p in named or i % 3 != 0
            rc = entry(src, n, o.ctypes.data, nseg, p[0], p[1], p[2], p[3], None, 0, rows.ctypes.data,
                       sel.ctypes.data if with_selected else None, mode)
            assert rc == 0, (form, p, mode, err(hip))
            want_rows, want_sel = expect(wants[p][0], wants[p][1], mode)
            assert np.array_equal(rows, want_rows), (form, p, mode)
            if with_selected:
                assert np.array_equal(sel, want_sel), (form, p, mode)
            else:
                assert (sel == (GARBAGE if mode & STORE else SEL_BIAS)).all()


def test_the_python_layer(hip):
    import torch
    from libflagstats_amd import segments_filter_rf as sfr
    values, o, t, d_off, _ = every_value_case()
    n, nseg = values.size, o.size - 1
    p = P_BOTH
    want_rows, want_sel = sfro.want(values, o, *p)
    kw = dict(require=p[0], exclude=p[1], include_any=p[2], exclude_all=p[3])
    for got_rows, got_sel in (sfr.flagstats_segments_filter_rf(values, o, **kw),
                              sfr.count_segments_device_ptr_filter_rf(t.data_ptr(), n, o, **kw)):
        assert got_rows.dtype == np.uint64 and got_sel.dtype == np.uint64
        assert np.array_equal(got_rows, want_rows) and np.array_equal(got_sel, want_sel)
    rows_t, sel_t = sfr.count_segments_torch_filter_rf(t, d_off, **kw)
    torch.cuda.synchronize()
    assert rows_t.dtype == torch.int64 and tuple(rows_t.shape) == (nseg, 32) and tuple(sel_t.shape) == (nseg,) and rows_t.device == t.device
    assert np.array_equal(u64(rows_t), want_rows) and np.array_equal(u64(sel_t), want_sel)
    dicts = sfr.segment_filter_dicts(got_rows, got_sel)
    assert [d["n_values"] for d in dicts] == [int(x) for x in want_sel]
    i = int(np.argmax(want_sel))
    assert int(dicts[i]["passed"]["mapped"]) == int(want_sel[i]) - int(want_rows[i, 2]) - int(want_rows[i, 18])


# ------------------------------------------------------------------ 2. geometry
PHASES = (0, 1, 3, 7)                         # the array 0, 2, 6 and 14 bytes into a 16-byte line
ALIGNMENTS = (None, 0, 3, 15)                 # of the MAPQ column


def test_geometry_direct_launches(hip, launcher):
    """fsk_launch_segments_filter_rf on grids 1 and 3: the array 0, 2, 6 and 14 bytes into a 16-byte line (ragged first and last
    units), lengths from one flag to nine units, boundaries inside a vector, at a row, at unit and writer seams +-1, empty
    segments, gaps in front of and behind the segments, under a residue of each instantiation.  The flags around the array pass
    P_ANY and P_ALL and carry MAPQ 0xFF, and a zero-filled position passes P_ALL, so `selected` shows any position counted outside
    its segment.  Segments that span two writers (added atomically) stand next to segments inside one (stored plainly).  Also
    one chunk of a longer array (base != 0) that holds only part of some segments, nseg == 0 and m == 0."""
    rng = np.random.RandomState(48)
    nmax = LENGTHS[-1]
    body = rng.randint(0, 65536, nmax).astype(np.uint16)
    forced = rng.randint(0, 100, nmax) < 55       # these pass all three predicates
    body[forced] = (body[forced] & np.uint16(~0x2D24 & 0xFFFF)) | np.uint16(0x0051)
    for p in (P_ANY, P_ALL, P_BOTH):
        assert view_mask(body[forced], *p).all() and not view_mask(body, *p).all()
        assert kind_of(hip, p) == (2, p)
    assert view_mask(np.array([AROUND], dtype=np.uint16), *P_ANY).all() and view_mask(np.array([AROUND, 0], dtype=np.uint16), *P_ALL).all()
    mapq = rng.randint(15, 60, nmax).astype(np.uint8)
    slabs, at = [], {}
    pos = 0
    for n in LENGTHS:
        for phase in PHASES:
            region = np.full((64 + 8 + n + 64 + 7) // 8 * 8, AROUND, dtype=np.uint16)
            region[64 + phase:64 + phase + n] = body[:n]
            at[n, phase] = pos + 64 + phase
            slabs.append(region)
            pos += region.size
    cols, q_at = [], {}
    pos = 0
    for n in LENGTHS:
        for align in ALIGNMENTS[1:]:
            region = np.full((16 + 16 + n + 16 + 15) // 16 * 16, 0xFF, dtype=np.uint8)
            region[16 + align:16 + align + n] = mapq[:n]
            q_at[n, align] = pos + 16 + align
            cols.append(region)
            pos += region.size
    d_arrays, d_cols = dev16(np.concatenate(slabs)), dev8(np.concatenate(cols))
    assert d_arrays.data_ptr() % 16 == 0 and d_cols.data_ptr() % 16 == 0
    batch, calls, offs = Batch(), [], []
    i = 0
    plain_seen, added_seen, seen = False, False, set()
    for n in LENGTHS:
        for phase in PHASES:
            ptr = d_arrays.data_ptr() + 2 * at[n, phase]
            assert ptr % 16 == 2 * phase
            for grid in (1, 3):
                w = writer_ranges(ptr % 16, n, grid)
                for p in (P_ANY, P_ALL, P_BOTH):
                    align = ALIGNMENTS[(i + i // 6) % 4]
                    mode = MODES[i % 4]
                    o = geometry_offsets(w, n, i % 3)
                    i += 1
                    seen.add((p, align is None, grid))
                    pieces = w.pieces(o)
                    plain_seen |= bool(pieces["plain"].any())
                    added_seen |= bool((~pieces["plain"]).any())
                    mn = 0 if align is None else 30
                    qptr = None if align is None else d_cols.data_ptr() + q_at[n, align]
                    want_rows, want_sel = sfro.want(body[:n], o, *p, mapq[:n], mn, superset=True)
                    k = batch.add(mode, want_rows, want_sel, (n, phase, grid, p, align, mode, o.tolist()))
                    offs.append(o)
                    calls.append((k, ptr, qptr, 0, n, len(offs) - 1, o.size - 1, p, mn, mode, grid))
    assert len(seen) == 12 and plain_seen and added_seen
    # one chunk [c0, c0 + m) of the longest array, global offsets over the whole of it
    n = LENGTHS[-1]
    o_all = np.array([0, 3, U + 1, 2 * U, 2 * U, 4 * U - 3, 6 * U + 9, 8 * U, n - 2], dtype=np.int64)
    for phase, c0, m in ((0, U + 3, 3 * U), (3, 2 * U - 5, 4 * U + 11), (7, 7, U)):
        for align, p in ((None, P_ANY), (3, P_ALL), (3, P_BOTH)):
            mn = 0 if align is None else 30
            clipped = np.clip(o_all, c0, c0 + m)
            want_rows, want_sel = sfro.want(body[:n], clipped, *p, mapq[:n], mn, superset=True)
            assert (o_all < c0).any() and (o_all > c0 + m).any() and want_sel.any() and not want_sel.all()
            ptr = d_arrays.data_ptr() + 2 * (at[n, phase] + c0)
            qptr = None if align is None else d_cols.data_ptr() + q_at[n, align] + c0
            for mode in (3, 0):
                k = batch.add(mode, want_rows, want_sel, ("chunk", phase, c0, m, align, p, mode))
                offs.append(o_all)
                calls.append((k, ptr, qptr, c0, m, len(offs) - 1, o_all.size - 1, p, mn, mode, 2))
    # m == 0: the store form zeroes, the += form leaves the bias; nseg == 0: nothing is touched
    nothing = (np.zeros((3, 32), dtype=np.uint64), np.zeros(3, dtype=np.uint64))
    for mode in MODES:
        k = batch.add(mode, *nothing, ("m == 0", mode))
        offs.append(np.array([0, 0, 0, 0], dtype=np.int64))
        calls.append((k, d_arrays.data_ptr(), None, 0, 0, len(offs) - 1, 3, P_BOTH, 0, mode, 2))
    k_none = batch.add(0, *nothing, "nseg == 0")
    lens = np.array([0] + [x.size for x in offs], dtype=np.int64)
    starts = np.cumsum(lens)
    d_off = dev64(np.concatenate(offs))
    batch.upload()
    for k, ptr, qptr, base, m, oi, nseg, p, mn, mode, grid in calls:
        rc = launcher(ptr, qptr, base, m, d_off.data_ptr() + 8 * int(starts[oi]), nseg, p[0], p[1], p[2], p[3], mn, batch.out(k),
                      batch.selected(k), mode, grid, None)
        assert rc == 0, (batch.items[k][5], rc)
    assert launcher(d_arrays.data_ptr(), None, 0, 100, None, 0, *P_BOTH, 0, batch.out(k_none), batch.selected(k_none), STORE, 2, None) == 0
    batch.check()


# ------------------------------------------------------------------ 3. which MAPQ byte belongs to which flag
@pytest.mark.parametrize("phase,align", [(0, 0), (5, 3), (0, 5)])
def test_which_mapq_byte_belongs_to_which_flag(hip, launcher, phase, align):
    """the parent's test under a residue: 16 units at grid 1; every flag passes the FLAG test and differs from its neighbours.
    MAPQ 60 at one position p and 0 elsewhere: `selected` is 1 in p's segment and 0 in the others and the row is that of array[p]
    alone; then 0 at p and 60 elsewhere.  p sweeps lanes, rows and units of a per-flag unit, of a chain run, and of their joints."""
    import torch
    n = 16 * U
    p4 = P_BOTH
    values = np.array([0x0111, 0x0091, 0x0011], dtype=np.uint16)[np.arange(n) % 3]
    assert view_mask(values[:3], *p4).all()
    slab = torch.full((64 + 8 + n + 64,), 0x00D1, dtype=torch.int16, device="cuda")
    slab[64 + phase:64 + phase + n] = dev16(values)
    arr = slab[64 + phase:64 + phase + n]
    assert arr.data_ptr() % 16 == 2 * phase
    col = torch.full((16 + 16 + n + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    q = col[16 + align:16 + align + n]
    assert q.data_ptr() % 16 == align
    w = writer_ranges(arr.data_ptr() % 16, n, 1)
    g = lambda k: k * U - w.lo0                                  # array index of unit boundary k  # noqa: E731
    o = np.array([0, 100, g(1) + 9, g(2) - 1, g(4) + 300, g(8) + 5, g(9) + 5, g(10), g(15) - 3, n], dtype=np.int64)
    pieces = w.pieces(o)
    assert {2, 3}.issubset(set(pieces["chain"].tolist())) and (pieces["chain"] == 0).any() and (pieces["head"] > 0).any()
    positions = sorted({min(max(g(k) + d, 0), n - 1) for k in (0, 1, 4, 5, 8, 10, 15)
                        for d in (-1, 0, 1, 7, 8, 300, 511, 512, 2048 + 77, U - 9)} | {0, n - 1})
    d_off = dev64(o)
    nseg = o.size - 1
    batch, plan = Batch(), []
    mq = np.zeros(n, dtype=np.uint8)
    for pos in positions:
        mq[:] = 0
        mq[pos] = 60
        alone = sfro.want(values, o, *p4, mq, 30, superset=True)
        assert int(alone[1].sum()) == 1
        rest = sfro.want(values, o, *p4, 60 - mq, 30, superset=True)
        assert int(rest[1].sum()) == n - 1
        # an off-by-one between column and array changes `selected`: the neighbours of pos lie in other vectors, rows or segments
        plan.append((pos, batch.add(STORE | SUPERSET, alone[0], alone[1], ("alone", phase, align, pos)),
                     batch.add(SUPERSET, rest[0], rest[1], ("all but", phase, align, pos))))
    batch.upload()
    for pos, k_alone, k_rest in plan:
        for k, everywhere, at_p in ((k_alone, 0, 60), (k_rest, 60, 0)):
            q.fill_(everywhere)
            q[pos] = at_p
            rc = launcher(arr.data_ptr(), q.data_ptr(), 0, n, d_off.data_ptr(), nseg, *p4, 30, batch.out(k), batch.selected(k),
                          batch.items[k][2], 1, None)
            assert rc == 0, rc
    batch.check()


# ------------------------------------------------------------------ 4. chain and epochs
@pytest.mark.parametrize("min_mapq", [0, 30])
def test_chain_and_epochs(hip, launcher, min_mapq):
    """grid 1 over the parent's 2,100 units of periodic input under (0x1, 0x804, 0x110, 0x2200): chain runs of 2, 254, 255, 256
    and 511 whole units -- below, at and past the epoch of 255, and two epochs and one unit -- with ragged heads and tails, rows
    stored plainly and rows added by two writers; all four modes over garbage / bias in rows and counts"""
    n = N_EPOCHS
    pattern = np.random.RandomState(405).randint(0, 65536, P).astype(np.uint16)
    mq_pattern = np.random.RandomState(406).randint(0, 61, P).astype(np.uint8)
    t, q = periodic_tensors(pattern, mq_pattern, n)
    ptr, qptr = t.data_ptr() + 2 * 3, q.data_ptr() + 3         # phase 3 of the array, MAPQ alignment 3
    w = writer_ranges(ptr % 16, n, 1)
    assert w.waves == 4 and w.lo0 == 3
    o = epochs_layout(w, n)
    pieces = w.pieces(o)
    chains = set(pieces["chain"].tolist())
    assert {2, 254, 255, 256, 511, 100, 300}.issubset(chains), chains
    assert ((pieces["chain"] > SEG_EPOCH) & pieces["plain"]).any() and ((pieces["chain"] > SEG_EPOCH) & ~pieces["plain"]).any()
    assert ((pieces["chain"] > 0) & (pieces["head"] > 0) & (pieces["tail"] > 0)).any()
    want_rows, want_sel = sfro.periodic_want(pattern, o, *P_BOTH, mq_pattern, min_mapq, superset=True, phase=3)
    parent_sel = sfo.periodic_want(pattern, o, P_BOTH[0], P_BOTH[1], mq_pattern, min_mapq, superset=True, phase=3)[1]
    assert (want_sel[np.diff(o) > 0] > 0).all() and (want_sel[np.diff(o) > 0] < parent_sel[np.diff(o) > 0]).all()
    d_off = dev64(o)
    batch = Batch()
    ks = [batch.add(mode, want_rows, want_sel, (min_mapq, mode)) for mode in MODES]
    batch.upload()
    for k in ks:
        rc = launcher(ptr, qptr if min_mapq else None, 0, n, d_off.data_ptr(), o.size - 1, *P_BOTH, min_mapq, batch.out(k),
                      batch.selected(k), batch.items[k][2], 1, None)
        assert rc == 0, rc
    batch.check()
    del t, q


# ------------------------------------------------------------------ 5. every min_units
def test_every_min_units_through_the_public_entries(hip, launcher):
    """the segments policy's chain threshold 0, 1, 2, 3, 255, 256 and 0xFFFFFFFF (per flag everywhere) under the device entry, the
    _sync form and the host form: the same rows and counts under every one; the policy is restored"""
    import torch
    from libflagstats_amd import segments_filter_rf as sfr
    n = (1 << 24) + 4099          # four units per writer at one workgroup per CU of 256 CUs
    pattern = np.random.RandomState(407).randint(0, 65536, P).astype(np.uint16)
    mq_pattern = np.random.RandomState(408).randint(0, 61, P).astype(np.uint8)
    t, q = periodic_tensors(pattern, mq_pattern, n)
    t, q = t[:n], q[:n]
    x, xq = np.resize(pattern, n), np.resize(mq_pattern, n)
    rng = np.random.RandomState(19)
    lengths = rng.choice([3, 100, 4095, 4097, 2 * U + 5, 3 * U, 17 * U - 1, 300_007, 1_000_003], 40)
    o = np.concatenate([[13], 13 + np.cumsum(lengths)])
    o = np.append(o[o < n - 7], n - 7).astype(np.int64)
    d_off = dev64(o)
    cus = hip.FLAGSTATS_hip_compute_units()
    saved = get_policy(hip)
    residues = (P_BOTH, P_ANY, P_ALL)
    for i, mu in enumerate(EVERY_MIN_UNITS):
        sup = bool(i % 2)
        mn = 30 if i % 3 else 0
        p = residues[i % 3]
        kw = dict(require=p[0], exclude=p[1], include_any=p[2], exclude_all=p[3])
        want_rows, want_sel = sfro.periodic_want(pattern, o, *p, mq_pattern, mn, superset=sup)
        chain = writer_ranges(t.data_ptr() % 16, n, cus).pieces(o, mu)["chain"]
        assert (chain.max() > 0) == (mu <= 3), (mu, chain.max())
        with policy(hip, mu):
            for store in (True, False):
                rows = torch.full((o.size - 1, 32), GARBAGE if store else BIAS, dtype=torch.int64, device="cuda")
                sel = torch.full((o.size - 1,), GARBAGE if store else SEL_BIAS, dtype=torch.int64, device="cuda")
                sfr.count_segments_torch_filter_rf(t, d_off, mapq=q if mn else None, min_mapq=mn, out=rows, selected=sel, store=store,
                                                   superset=sup, **kw)
                torch.cuda.synchronize()
                w_rows, w_sel = expect(want_rows, want_sel, (STORE if store else 0) | SUPERSET)   # (want_rows has no superset slots unless sup)
                assert np.array_equal(u64(rows), w_rows), ("device", mu, store)
                assert np.array_equal(u64(sel), w_sel), ("device", mu, store)
            got = sfr.count_segments_device_ptr_filter_rf(t.data_ptr(), n, o, mapq_ptr=q.data_ptr() if mn else 0, min_mapq=mn, superset=sup, **kw)
            assert np.array_equal(got[0], want_rows) and np.array_equal(got[1], want_sel), ("sync", mu)
            got = sfr.flagstats_segments_filter_rf(x, o, mapq=xq if mn else None, min_mapq=mn, superset=sup, **kw)
            assert np.array_equal(got[0], want_rows) and np.array_equal(got[1], want_sel), ("host", mu)
    assert get_policy(hip) == saved


# ------------------------------------------------------------------ 6. the three kinds of call
def test_the_three_kinds_of_call(hip, launcher):
    """nothing can pass: the store form zeroes rows and counts and the += form leaves the bias, through the three entries and
    through the launcher with a MAPQ column of one byte (the entries check the column's extent before they know the predicate, so
    only the launcher takes such a column; every pointer handed in is a valid one); a plain pair: bit for bit segments_filter's
    result under the reduced pair; a residue: the oracle"""
    import torch
    from libflagstats_amd import segments_filter as sf
    from libflagstats_amd import segments_filter_rf as sfr
    n = 5 * U + 77
    rng = np.random.RandomState(54)
    values = rng.randint(0, 65536, n).astype(np.uint16)
    mapq = rng.randint(0, 60, n).astype(np.uint8)
    t, q = dev16(values), dev8(mapq)
    o = np.array([5, 5, 300, U + 1, 4 * U, n - 3], dtype=np.int64)
    d_off = dev64(o)
    nseg = o.size - 1
    nothing = (np.zeros((nseg, 32), dtype=np.uint64), np.zeros(nseg, dtype=np.uint64))
    batch, calls = Batch(), []
    for p, kind, pair in sfro.TABLE:
        assert kind_of(hip, p)[0] == kind
        for mn in (0, 30):
            want = nothing if kind == 0 else sfro.want(values, o, *p, mapq, mn, superset=True)
            if kind == 1:
                again = sfo.want(values, o, pair[0], pair[1], mapq, mn, superset=True)
                assert np.array_equal(want[0], again[0]) and np.array_equal(want[1], again[1])
            if kind:
                assert want[1].any()
            for mode in MODES:
                calls.append((batch.add(mode, *want, (p, kind, mn, mode)), p, mn, mode))
    batch.upload()
    for k, p, mn, mode in calls:
        rc = hip.FLAGSTATS_hip_device_u16_segments_filter_rf(t.data_ptr(), n, d_off.data_ptr(), nseg, *p, q.data_ptr() if mn else None, mn,
                                                             batch.out(k), batch.selected(k), mode, None)
        assert rc == 0, (p, mn, mode, err(hip))
    batch.check()
    # nothing can pass, through the launcher with a one-byte column under min_mapq = 30: such a call launches nothing, so the
    # column's length does not matter to it; the result is what is asserted
    one = torch.zeros(1, dtype=torch.uint8, device="cuda")
    batch = Batch()
    ks = [(batch.add(mode, *nothing, ("launcher, nothing passes", p, mode)), p, mode) for p, kind, _ in sfro.TABLE if kind == 0 for mode in MODES]
    batch.upload()
    for k, p, mode in ks:
        assert launcher(t.data_ptr(), one.data_ptr(), 0, n, d_off.data_ptr(), nseg, *p, 30, batch.out(k), batch.selected(k), mode, 2, None) == 0
    batch.check()
    # the host form moves nothing for such a predicate and still answers
    for p, kind, _ in sfro.TABLE:
        if kind:
            continue
        for mode in MODES:
            rows = np.full((nseg, 32), GARBAGE if mode & 1 else BIAS, dtype=np.uint64)
            sel = np.full(nseg, GARBAGE if mode & 1 else SEL_BIAS, dtype=np.uint64)
            for entry, src, qsrc in ((hip.FLAGSTATS_hip_device_u16_segments_filter_rf_sync, t.data_ptr(), q.data_ptr()),
                                     (hip.FLAGSTATS_hip_u16_x64_segments_filter_rf, values.ctypes.data, mapq.ctypes.data)):
                rows[:] = GARBAGE if mode & 1 else BIAS
                sel[:] = GARBAGE if mode & 1 else SEL_BIAS
                assert entry(src, n, o.ctypes.data, nseg, *p, qsrc, 30, rows.ctypes.data, sel.ctypes.data, mode) == 0, err(hip)
                want = expect(*nothing, mode)
                assert np.array_equal(rows, want[0]) and np.array_equal(sel, want[1]), (p, mode)
    # a plain pair is the parent's entry, bit for bit, in every mode
    for p, kind, pair in sfro.TABLE:
        if kind != 1:
            continue
        for mn in (0, 30):
            for store in (True, False):
                for sup in (False, True):
                    a = [torch.full((nseg, 32), BIAS, dtype=torch.int64, device="cuda"), torch.full((nseg,), SEL_BIAS, dtype=torch.int64, device="cuda")]
                    b = [x.clone() for x in a]
                    sf.count_segments_torch_filter(t, d_off, require=pair[0], exclude=pair[1], mapq=q if mn else None, min_mapq=mn, out=a[0],
                                                   selected=a[1], store=store, superset=sup)
                    sfr.count_segments_torch_filter_rf(t, d_off, require=p[0], exclude=p[1], include_any=p[2], exclude_all=p[3],
                                                       mapq=q if mn else None, min_mapq=mn, out=b[0], selected=b[1], store=store, superset=sup)
                    torch.cuda.synchronize()
                    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int(b[1].sum()) != nseg * SEL_BIAS, (p, mn, store, sup)


# ------------------------------------------------------------------ 7. equivalences
def test_equivalences(hip, launcher):
    """include_any = exclude_all = 0 is the parent entry (device offsets that run past the array are clamped); one segment [0, n) is
    filter_rf.count_torch_filter_rf; the sum over segments that tile the array is the whole-column call"""
    import torch
    from libflagstats_amd import filter_rf
    from libflagstats_amd import segments_filter_rf as sfr
    n = 5 * U + 77
    rng = np.random.RandomState(55)
    values = rng.randint(0, 65536, n).astype(np.uint16)
    mapq = rng.randint(0, 60, n).astype(np.uint8)
    t, q = dev16(values), dev8(mapq)
    o = np.array([5, 5, 300, U + 1, 4 * U, n + 1000, n + 5000], dtype=np.int64)     # the last two run past the array
    d_off = dev64(o)
    nseg = o.size - 1
    for mode in MODES:
        for require, exclude, mn in ((0, 0, 0), (0x2, 0x904, 30)):
            a = torch.full((nseg * 33,), BIAS, dtype=torch.int64, device="cuda")
            b = torch.full((nseg * 33,), BIAS, dtype=torch.int64, device="cuda")
            assert hip.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), n, d_off.data_ptr(), nseg, require, exclude, q.data_ptr(), mn,
                                                                a.data_ptr(), a.data_ptr() + nseg * 256, mode, None) == 0, err(hip)
            assert hip.FLAGSTATS_hip_device_u16_segments_filter_rf(t.data_ptr(), n, d_off.data_ptr(), nseg, require, exclude, 0, 0, q.data_ptr(),
                                                                   mn, b.data_ptr(), b.data_ptr() + nseg * 256, mode, None) == 0, err(hip)
            torch.cuda.synchronize()
            assert torch.equal(a, b) and not (b[nseg * 32:] == BIAS).all(), (mode, require, exclude, mn)
    # one segment [0, n), and segments that tile [0, n), against the whole-column entry
    whole = dev64(np.array([0, n]))
    tiles = np.array([0, 1, 9, 600, U - 1, U, 2 * U + 5, 2 * U + 5, 4 * U + 1, n], dtype=np.int64)
    d_tiles = dev64(tiles)
    for p in (P_ANY, P_ALL, P_BOTH):
        kw = dict(require=p[0], exclude=p[1], include_any=p[2], exclude_all=p[3])
        for mn in (0, 30):
            for sup in (False, True):
                ref_rows, ref_sel = filter_rf.count_torch_filter_rf(t, mapq=q if mn else None, min_mapq=mn, store=True, superset=sup, **kw)
                rows1, sel1 = sfr.count_segments_torch_filter_rf(t, whole, mapq=q if mn else None, min_mapq=mn, superset=sup, **kw)
                rows9, sel9 = sfr.count_segments_torch_filter_rf(t, d_tiles, mapq=q if mn else None, min_mapq=mn, superset=sup, **kw)
                torch.cuda.synchronize()
                assert torch.equal(rows1[0], ref_rows) and int(sel1[0]) == int(ref_sel[0]) > 0, (p, mn, sup)
                assert torch.equal(rows9.sum(dim=0), ref_rows) and int(sel9.sum()) == int(ref_sel[0]), (p, mn, sup)
        # the whole-column reference itself against the oracle (both kernels could be wrong alike)
        assert int(ref_sel[0]) == int(view_mask(values, *p, mapq, 30).sum())
    # NULL d_selected through the launcher; nseg == 0 touches nothing
    want_rows, want_sel = sfro.want(values, tiles, *P_BOTH, mapq, 30, superset=True)
    batch = Batch()
    ks = [batch.add(mode, want_rows, want_sel, ("NULL d_selected", mode), with_selected=False) for mode in MODES]
    batch.upload()
    for k in ks:
        assert launcher(t.data_ptr(), q.data_ptr(), 0, n, d_tiles.data_ptr(), tiles.size - 1, *P_BOTH, 30, batch.out(k), None, batch.items[k][2], 2,
                        None) == 0
    batch.check()
    assert hip.FLAGSTATS_hip_device_u16_segments_filter_rf(t.data_ptr(), n, None, 0, 0, 0, 0x50, 0, None, 0, None, None, STORE, None) == 0
    assert hip.FLAGSTATS_hip_u16_x64_segments_filter_rf(values.ctypes.data, n, None, 0, 0, 0, 0, 0xC, None, 0, None, None, STORE) == 0


# ------------------------------------------------------------------ 8. atomics
def test_three_streams_add_into_one_set_of_rows(hip):
    import torch
    from libflagstats_amd import segments_filter_rf as sfr
    rng = np.random.RandomState(74)
    o = np.array([0, 50, 3 * U + 1, 3 * U + 1, 20 * U - 7, 36 * U], dtype=np.int64)
    nseg = o.size - 1
    d_off = dev64(o)
    rows = torch.zeros((nseg, 32), dtype=torch.int64, device="cuda")
    sel = torch.zeros(nseg, dtype=torch.int64, device="cuda")
    total_rows, total_sel = np.zeros((nseg, 32), dtype=np.uint64), np.zeros(nseg, dtype=np.uint64)
    inputs = []
    for n, p, mn in ((36 * U + 11, P_ANY, 30), (30 * U + 5, P_ALL, 0), (40 * U - 3, (0, 0, 0x0101, 0x8080), 200)):
        values = rng.randint(0, 65536, n).astype(np.uint16)
        mapq = rng.randint(0, 256, n).astype(np.uint8)
        w_rows, w_sel = sfro.want(values, np.clip(o, 0, n), *p, mapq, mn, superset=True)
        assert w_sel.any()
        total_rows += w_rows
        total_sel += w_sel
        inputs.append((dev16(values), p, dev8(mapq) if mn else None, mn))
    streams = [torch.cuda.Stream() for _ in inputs]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    for st, (t, p, q, mn) in zip(streams, inputs):
        with torch.cuda.stream(st):
            sfr.count_segments_torch_filter_rf(t, d_off, require=p[0], exclude=p[1], include_any=p[2], exclude_all=p[3], mapq=q, min_mapq=mn,
                                               out=rows, selected=sel, store=False, superset=True)
    for st in streams:
        st.synchronize()
    assert np.array_equal(u64(rows), total_rows) and np.array_equal(u64(sel), total_sel)


# ------------------------------------------------------------------ 9. host form across chunks
def test_host_form_across_chunks(hip):
    """chunks of 8,193 flags from offsets[0] = 3 on: segments straddle chunk seams, both staging slots are used, chunks start at odd
    and even elements of array and column, and the column's slice sits 16,386 bytes into the staging buffer"""
    from libflagstats_amd import _lib
    from libflagstats_amd import segments_filter_rf as sfr
    n = 6 * 8193 + 77
    rng = np.random.RandomState(90)
    values = rng.randint(0, 65536, n + 1).astype(np.uint16)[1:]
    mapq = rng.randint(0, 60, n + 1).astype(np.uint8)[1:]
    o = np.array([3, 10, 10, 8193 + 2, 3 * 8193 + 500, 3 * 8193 + 501, 5 * 8193 + 3, n - 20], dtype=np.int64)
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", 8193), "chunk_flags")
        for p in (P_BOTH, P_ANY, P_ALL):
            kw = dict(require=p[0], exclude=p[1], include_any=p[2], exclude_all=p[3])
            for q, mn in ((None, 0), (mapq, 30)):
                for sup in (False, True):
                    want_rows, want_sel = sfro.want(values, o, *p, q, mn, superset=sup)
                    assert want_sel.any() and (want_sel < np.diff(o).astype(np.uint64)).any()
                    got = sfr.flagstats_segments_filter_rf(values, o, mapq=q, min_mapq=mn, superset=sup, **kw)
                    assert np.array_equal(got[0], want_rows) and np.array_equal(got[1], want_sel), (p, mn, sup)
                want_rows, want_sel = sfro.want(values, o, *p, q, mn, superset=True)
                for flags in (0, SUPERSET):                  # += over bias words
                    rows = np.full((o.size - 1, 32), BIAS, dtype=np.uint64)
                    sel = np.full(o.size - 1, SEL_BIAS, dtype=np.uint64)
                    rc = hip.FLAGSTATS_hip_u16_x64_segments_filter_rf(values.ctypes.data, n, o.ctypes.data, o.size - 1, *p,
                                                                      q.ctypes.data if mn else None, mn, rows.ctypes.data, sel.ctypes.data, flags)
                    assert rc == 0, err(hip)
                    w = expect(want_rows, want_sel, flags)
                    assert np.array_equal(rows, w[0]) and np.array_equal(sel, w[1]), (p, mn, flags)
        # one chunk only (a single staging slot), and segments that cover nothing
        for oo in (np.array([1, 50, 99]), np.array([7, 7, 7]), np.array([n, n])):
            got = sfr.flagstats_segments_filter_rf(values, oo, *P_BOTH, mapq=mapq, min_mapq=30)
            want = sfro.want(values, oo, *P_BOTH, mapq, 30)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), oo
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old
    got = sfr.flagstats_segments_filter_rf(values[:0], [0, 0], 1, 4, 0x50, 0xC0, mapq=mapq[:0], min_mapq=30)
    assert got[0].shape == (1, 32) and not got[0].any() and not got[1].any()
    got = sfr.count_segments_device_ptr_filter_rf(0, 0, [0, 0, 0], 1, 4, 0x50, 0xC0)
    assert got[0].shape == (2, 32) and not got[0].any() and not got[1].any()


# ------------------------------------------------------------------ 10. refusals that need a device
def test_refusals_on_the_device(hip, launcher):
    """what only a device at hand can refuse: the launcher's own checks (nothing queued), the entry's extent checks with the two
    new masks in the call, and tensors on another device than `t` (on a box with a second GPU)"""
    import torch
    from libflagstats_amd import segments_filter_rf as sfr
    n, nseg = 4096, 3
    t = torch.zeros(n + 8, dtype=torch.int16, device="cuda")
    q = torch.full((n + 8,), 60, dtype=torch.uint8, device="cuda")
    d_off = dev64(np.array([0, 10, 2000, n]))
    words = torch.full((nseg * 33,), BIAS, dtype=torch.int64, device="cuda")
    p, ps = words.data_ptr(), words.data_ptr() + nseg * 256
    a, c, f = t.data_ptr(), q.data_ptr(), d_off.data_ptr()
    r = P_BOTH
    assert launcher(a, c, 0, 8, f, nseg, *r, 30, p, ps, 4, 1, None) != 0                                  # other mode bits
    assert launcher(a, c, 0, 8, f, nseg, *r, 30, p, ps, STORE, 0, None) != 0                              # no workgroups
    assert launcher(a, None, 0, 1 << 35, f, nseg, *r, 0, p, ps, STORE, 1, None) != 0                      # 2^33 flags per wave
    for k in range(4):
        bad = list(r)
        bad[k] = 0x10000
        assert launcher(a, None, 0, 8, f, nseg, *bad, 0, p, ps, STORE, 1, None) != 0
    assert launcher(a, c, 0, 8, f, nseg, *r, 256, p, ps, STORE, 1, None) != 0
    assert launcher(a, None, 0, 8, f, nseg, *r, 30, p, ps, STORE, 1, None) != 0                           # no column
    assert launcher(None, c, 0, 8, f, nseg, *r, 30, p, ps, STORE, 1, None) != 0
    assert launcher(a + 1, c, 0, 8, f, nseg, *r, 30, p, ps, STORE, 1, None) != 0
    assert launcher(a, c, 0, 8, None, nseg, *r, 30, p, ps, STORE, 1, None) != 0
    assert launcher(a, c, 0, 8, f, nseg, *r, 30, None, ps, STORE, 1, None) != 0
    # the entry: a column one byte short (an allocation of the library's own, whose size is exact), host rows as d_out
    rows, sel = words[:nseg * 32], words[nseg * 32:]
    nbytes = 2 << 20
    raw = hip.FLAGSTATS_hip_device_alloc(nbytes)
    assert raw
    try:
        big = torch.zeros(nbytes + 8, dtype=torch.int16, device="cuda")
        big_off = dev64(np.array([0, 5, 100, nbytes]))
        rc = hip.FLAGSTATS_hip_device_u16_segments_filter_rf(big.data_ptr(), nbytes + 1, big_off.data_ptr(), nseg, *r, raw, 30, rows.data_ptr(),
                                                             sel.data_ptr(), STORE, None)
        assert rc != 0 and "d_mapq" in err(hip) and "1 bytes short" in err(hip), err(hip)
    finally:
        hip.FLAGSTATS_hip_device_free(raw)
    h_out = np.full((nseg, 32), BIAS, dtype=np.uint64)
    rc = hip.FLAGSTATS_hip_device_u16_segments_filter_rf(a, n, f, nseg, *r, c, 30, h_out.ctypes.data, sel.data_ptr(), 0, None)
    assert rc != 0 and "d_out" in err(hip), err(hip)
    torch.cuda.synchronize()
    assert (words == BIAS).all() and (h_out == BIAS).all()
    cpu = {"offsets": torch.zeros(4, dtype=torch.int64), "mapq": torch.zeros(n + 8, dtype=torch.uint8),
           "out": torch.zeros((3, 32), dtype=torch.int64), "selected": torch.zeros(3, dtype=torch.int64)}
    for name, x in cpu.items():
        kw = {"mapq": q, "min_mapq": 30, "include_any": 0x50}
        args = [t, d_off]
        if name == "offsets":
            args[1] = x
        else:
            kw[name] = x
        with pytest.raises(ValueError, match=r"%s must live on t's device \(cuda:0\), not on cpu" % name):
            sfr.count_segments_torch_filter_rf(*args, **kw)
    if torch.cuda.device_count() < 2:
        return                                                                     # (the rest needs a second device)
    other = {"offsets": torch.zeros(4, dtype=torch.int64, device="cuda:1"), "mapq": torch.zeros(n + 8, dtype=torch.uint8, device="cuda:1"),
             "out": torch.zeros((3, 32), dtype=torch.int64, device="cuda:1"), "selected": torch.zeros(3, dtype=torch.int64, device="cuda:1")}
    for name, x in other.items():
        kw = {"mapq": q, "min_mapq": 30, "exclude_all": 0xC}
        args = [t, d_off]
        if name == "offsets":
            args[1] = x
        else:
            kw[name] = x
        with pytest.raises(ValueError, match=r"%s must live on t's device \(cuda:0\), not on cuda:1" % name):
            sfr.count_segments_torch_filter_rf(*args, **kw)
