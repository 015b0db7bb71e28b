"""GPU: the eighteen kernels derived from K1 -- flat and segmented, on uint16, int32 and int64 columns, under samtools' filter, a
selection, or both, and the three units of the whole predicate (--rf / -G) -- past 2^31 and 2^32 elements and bytes, against
tests/periodic_oracle.py: an exact reference that needs no host copy of the column.  Every comparison is exact.

The columns: 2^32 + 3 * 2^20 + 5 uint16 or int32 elements (8 and 16 GiB), 2^31 + 3 * 2^20 + 5 int64 elements (16 GiB), a MAPQ
column, a byte mask and bitmaps for the selection offsets 0, 5 and 2^32 + 13, all filled on the device from periods of 977, 61
and 13 elements, with needles at the elements and bytes around 2^31 and 2^32 and at the end.  One element slab is held at a
time; the MAPQ column and the selections are shared by the widths.  Every array lies between sentinels that count if touched
(flags 0xFFFF, MAPQ 255, selection ones), and a window or a segment is a view into it.

tests/test_periodic_oracle_host.py shows on the CPU that each call below tells an index held in 32 bits -- in the array's byte
offset, the selection index, the MAPQ index or the segment offsets -- from the truth."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import periodic_oracle as po  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 64                                        # sentinel elements / bytes in front of and behind every array
STORE, SUPERSET = 1, 2
GARBAGE, BIAS, SEL_BIAS, MASK_BIAS = 0x5EED_0000_0BAD, 3, 5, (1 << 48) | (1 << 29)
N_MAX = po.slab_n(2)
TORCH = {2: "int16", 4: "int32", 8: "int64"}
# (wide, segmented, filtered, masked): the fifteen derived units -- all sixteen combinations but K1 itself
FLAT = [(w, False, f, m) for w in (False, True) for f in (False, True) for m in (False, True) if w or f or m]
SEGMENTED = [(w, True, f, m) for w in (False, True) for f in (False, True) for m in (False, True)]
# u16_filter_rf and wide_filter_rf, flat, on whole columns; u16_segments_filter_rf, on uint16 columns only
RF = [(False, False, True, False, "rf"), (True, False, True, False, "rf"), po.RF_SEGMENTED_UNIT]
assert len(FLAT) + len(SEGMENTED) == 15 and len(FLAT) + len(SEGMENTED) + len(RF) == 18 and RF[2] == (False, True, True, False, "rf")


def stem(unit):
    wide, seg, filt, mask = unit[:4]
    return ("wide" if wide else "u16") + ("_segments" if seg else "") + ("_filter" if filt else "") + ("_where" if mask else "") + "_rf" * (len(unit) > 4)


def entry_name(unit, form):
    return "FLAGSTATS_hip_device_" + stem(unit) + ("_sync" if form == "sync" else "")


def arguments(unit, a, with_stream):
    """the argument list of a public entry of the unit: array, n, [elem_bytes], [offsets, nseg], [require, exclude, mapq,
    [include_any, exclude_all], mapq, min_mapq], [sel, sel_offset, sel_bits], out, [selected], [high], flags, [stream]"""
    wide, seg, filt, mask = unit[:4]
    pred = ["R", "X", "IA", "XA", "Q", "MQ"] if len(unit) > 4 else ["R", "X", "Q", "MQ"]
    names = ["A", "N"] + (["W"] if wide else []) + (["O", "NS"] if seg else []) + (pred if filt else [])
    names += (["S", "SO", "SB"] if mask else []) + ["OUT"] + (["SEL"] if filt or mask else []) + (["HIGH"] if wide else []) + ["FLAGS"]
    return [a[k] for k in names] + ([None] if with_stream else [])


def fill_periodic(body, pattern):
    """body[j] = pattern[j % len(pattern)], on the device, with no copy of the body's size"""
    p = pattern.numel()
    k = body.numel() // p
    if k:
        body[:k * p].view(k, p).copy_(pattern.unsqueeze(0).expand(k, p))
    body[k * p:] = pattern[:body.numel() - k * p]


class Shared:
    """the MAPQ column, the byte mask and the bitmaps: made once, for the longest column, and left unchanged"""

    def __init__(self):
        import torch
        F, H, S, Q = po.patterns(2)
        self.S = S
        needles = sorted(po.needle_positions(N_MAX))
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        self.mapq = torch.full((PAD + N_MAX + PAD,), 255, dtype=torch.uint8, device="cuda")
        fill_periodic(self.mapq[PAD:PAD + N_MAX], dev(Q))
        self.bytes = torch.full((PAD + N_MAX + PAD,), 255, dtype=torch.uint8, device="cuda")
        fill_periodic(self.bytes[PAD:PAD + N_MAX], dev(np.where(S, 1 + np.arange(po.LEN_S) % 250, 0).astype(np.uint8)))
        at = torch.tensor(needles, dtype=torch.int64, device="cuda") + PAD
        self.mapq[at] = po.NEEDLE_MAPQ
        self.bytes[at] = 1
        self.bitmaps = {so: self.bitmap(so, needles) for so in (0, 5, po.BIG_OFFSET)}
        torch.cuda.synchronize()

    def bitmap(self, so, needles, n=N_MAX, pattern=None):
        """uint8 tensor: PAD sentinel bytes, then the bitmap whose bit ``so + j`` is S[(so + j) % 61] for element j < n (1 at a
        needle), ones in every other bit; then sentinels"""
        import torch
        S = self.S if pattern is None else pattern
        nbytes = (so + n + 7) // 8
        t = torch.full((PAD + nbytes + PAD,), 255, dtype=torch.uint8, device="cuda")
        b0 = so // 8
        period = np.packbits(S[(8 * b0 + np.arange(8 * po.LEN_S)) % po.LEN_S], bitorder="little")      # 61 bytes, from byte b0 on
        fill_periodic(t[PAD + b0:PAD + nbytes], torch.from_numpy(period).cuda())
        for at, ones in ((b0, (1 << (so & 7)) - 1), (nbytes - 1, 0xFF & ~((1 << ((so + n - 1) & 7) + 1) - 1))):
            t[PAD + at] = int(t[PAD + at].item()) | ones
        for p in needles:
            self.set_bit(t, so + p, True)
        return t

    @staticmethod
    def set_bit(t, bit, value):
        at = PAD + (bit >> 3)
        old = int(t[at].item())
        t[at] = (old | 1 << (bit & 7)) if value else (old & ~(1 << (bit & 7)) & 0xFF)


class Slab:
    """the element slab of one width and its oracle"""

    def __init__(self, W):
        import torch
        self.W = W
        self.col = po.column(W)
        self.n = self.col.n
        dtype = getattr(torch, TORCH[W])
        self.t = torch.full((PAD + self.n + PAD,), -1, dtype=dtype, device="cuda")
        j = np.arange(po.LEN_F * po.LEN_H, dtype=np.int64)
        flag, hb, _, _ = self.col.background(j, j, j)
        period = (flag.astype(np.uint64) | hb).astype(po.UNSIGNED[W]).view(np.dtype(TORCH[W]))
        fill_periodic(self.body, torch.from_numpy(period).cuda())
        for p, (f, h, _, _) in self.col.needles.items():
            self.body[p] = int(np.array([f | h], dtype=np.uint64).astype(po.UNSIGNED[W]).view(np.dtype(TORCH[W]))[0])
        torch.cuda.synchronize()
        self.base = self.t.data_ptr() + PAD * W
        assert self.base % 16 == 0
        self._want = {}

    @property
    def body(self):
        return self.t[PAD:PAD + self.n]

    def want(self, call, filt, mask):
        """the oracle's result of a call for a kernel with / without a filter and a selection, computed once"""
        key = po.call_key(call, filt, mask)
        if key not in self._want:
            self._want[key] = self.col.expect(call["offsets"], superset=True, **po.reduced(call, filt, mask))
        return self._want[key]


@pytest.fixture(scope="module")
def shared(hip):
    import torch
    s = Shared()
    yield s
    del s
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", params=[2, 4, 8])
def slab(request, shared):
    import torch
    s = Slab(request.param)
    yield s
    s.t = None
    del s
    torch.cuda.empty_cache()


def selection(shared, call, first=0):
    """(pointer, sel_offset, sel_bits) of the call's selection for an array that begins at element ``first`` of the slab"""
    if call["form"] == "bytes":
        return shared.bytes.data_ptr() + PAD, first, 8
    return shared.bitmaps[call["sel_offset"]].data_ptr() + PAD, call["sel_offset"] + first, 1


def run_unit(hip, shared, slab, unit, form, store, call, first=None):
    """One call of a public entry against the oracle.  A flat unit takes the call's one segment as its array; a segmented unit
    takes the whole slab and the call's offsets -- or, with ``first``, the window from there on with the offsets relative to it.
    Returns None or what differs."""
    import torch
    wide, seg, filt, mask = unit[:4]
    W = slab.W
    assert wide == (W > 2) and (len(unit) > 4) == ("rf" in call)
    o_abs = np.asarray(call["offsets"], dtype=np.int64)
    want = slab.want(call, filt, mask)
    if seg and first is None:
        first, n, offs = 0, slab.n, o_abs
    elif seg:
        n, offs = int(o_abs[-1]) - first, o_abs - first
    else:
        assert o_abs.size == 2
        first, n, offs = int(o_abs[0]), int(o_abs[1] - o_abs[0]), None
    nseg = o_abs.size - 1
    require, exclude, min_mapq = call["pred"]
    S, SO, SB = selection(shared, call, first)
    a = {"A": slab.base + first * W, "N": n, "W": W, "NS": nseg, "R": require, "X": exclude, "MQ": min_mapq,
         "IA": call.get("rf", (0, 0))[0], "XA": call.get("rf", (0, 0))[1],
         "Q": shared.mapq.data_ptr() + PAD + first if min_mapq else None, "S": S, "SO": SO, "SB": SB,
         "FLAGS": (STORE if store else 0) | SUPERSET}
    fills = (GARBAGE, GARBAGE, GARBAGE) if store else (BIAS, SEL_BIAS, MASK_BIAS)
    shapes = ((nseg, 32), (nseg,), (nseg,))
    if form == "device":
        outs = [torch.full(shape, fill, dtype=torch.int64, device="cuda") for shape, fill in zip(shapes, fills)]
        ptrs = [t.data_ptr() for t in outs]
        if seg:
            d_off = torch.from_numpy(np.ascontiguousarray(offs)).cuda()
            a["O"] = d_off.data_ptr()
    else:
        outs = [np.full(shape, fill, dtype=np.uint64) for shape, fill in zip(shapes, fills)]
        ptrs = [x.ctypes.data for x in outs]
        if seg:
            h_off = np.ascontiguousarray(offs, dtype=np.uint64)
            a["O"] = h_off.ctypes.data
    a["OUT"], a["SEL"], a["HIGH"] = ptrs
    torch.cuda.synchronize()
    name = entry_name(unit, form)
    rc = getattr(hip, name)(*arguments(unit, a, form == "device"))
    assert rc == 0, (name, call["case"], rc, hip.FLAGSTATS_hip_last_error().decode(errors="replace"))
    torch.cuda.synchronize()
    rows, selected, high = (t.cpu().numpy().view(np.uint64) for t in outs) if form == "device" else outs
    w_rows, w_sel, w_high = want.rows, want.selected, want.high(mask)
    if not store:
        w_rows, w_sel, w_high = w_rows + np.uint64(BIAS), w_sel + np.uint64(SEL_BIAS), w_high | np.uint64(MASK_BIAS)
    bad = {}
    if not np.array_equal(rows, w_rows):
        i = np.argwhere(rows != w_rows)[:4]
        bad["rows"] = [(tuple(int(v) for v in ij), int(rows[tuple(ij)]), int(w_rows[tuple(ij)])) for ij in i]
    if (filt or mask) and not np.array_equal(selected, w_sel):
        i = np.nonzero(selected != w_sel)[0][:4]
        bad["selected"] = [(int(k), int(selected[k]), int(w_sel[k])) for k in i]
    if wide and not np.array_equal(high, w_high):
        i = np.nonzero(high != w_high)[0][:4]
        bad["high"] = [(int(k), hex(int(high[k])), hex(int(w_high[k]))) for k in i]
    return {"entry": name, "case": call["case"], "store": store, **bad} if bad else None


def units_of(slab, units):
    return [u for u in units if u[0] == (slab.W > 2)]


# ------------------------------------------------------------------ 1, 2: flat units, the whole slab and windows past the mark
def test_flat_units_whole_slab(hip, shared, slab):
    calls = [c for c in po.slab_calls(slab.W) if c["case"].startswith("whole")]
    assert len(calls) == 9                        # -F 0x904, -f 0x2 -F 0x904 -q 30 and no predicate, each under the three mask forms
    for call in calls:
        assert int(slab.want(call, True, True).selected[0]) > 0
        for unit in units_of(slab, FLAT):
            for store in (True, False):
                assert run_unit(hip, shared, slab, unit, "device", store, call) is None
            assert run_unit(hip, shared, slab, unit, "sync", False, call) is None


def test_windows_that_begin_past_the_mark(hip, shared, slab):
    """the base is 2, 4 or 8 bytes past a 16-byte boundary; the selection offset alone passes 2^32"""
    calls = [c for c in po.slab_calls(slab.W) if c["local"]]
    assert len(calls) == 2
    for call in calls:
        first = int(call["offsets"][0])
        assert first > po.MARK[slab.W] and (slab.base + first * slab.W) % 16 == slab.W
        for unit in units_of(slab, FLAT):
            for store in (True, False):
                assert run_unit(hip, shared, slab, unit, "device", store, call) is None
        for unit in units_of(slab, SEGMENTED):
            for form in ("device", "sync"):
                assert run_unit(hip, shared, slab, unit, form, True, call, first=first) is None


def test_rf_units_whole_slab_and_window(hip, shared, slab):
    """u16_filter_rf / wide_filter_rf under the two residue predicates: the whole slab in the device form (store and +=) and the
    _sync form, and the window that begins past the mark at a base 2, 4 or 8 bytes past a 16-byte boundary"""
    unit = units_of(slab, RF)[0]
    calls = po.rf_slab_calls(slab.W)
    assert [c["layout"] for c in calls] == ["whole", "whole", "window", "window"]
    for call in calls:
        want = slab.want(call, True, False)
        assert 0 < int(want.selected[0]) < int(call["offsets"][1] - call["offsets"][0])
        for store in (True, False):
            assert run_unit(hip, shared, slab, unit, "device", store, call) is None
        if call["layout"] == "whole":
            assert run_unit(hip, shared, slab, unit, "sync", False, call) is None
        else:
            first = int(call["offsets"][0])
            assert first > po.MARK[slab.W] and (slab.base + first * slab.W) % 16 == slab.W


def test_rf_units_needles_one_at_a_time(hip, shared, slab):
    """for every needle a residue predicate with -q 60 that this needle alone passes (po.needle_rf_predicate): counters and
    selected are those of exactly that element, wherever in the 8 or 16 GiB it lies; high is the whole column's"""
    unit = units_of(slab, RF)[0]
    col = slab.col
    for k, (flag, _, _, _) in sorted(col.needles.items()):
        call = po.rf_call(po.needle_rf_predicate(flag), (0, slab.n), "rf-needle-%d" % k, "whole")
        want, alone = slab.want(call, True, False), col.expect([k, k + 1], superset=True)
        assert int(want.selected[0]) == 1 and np.array_equal(want.rows, alone.rows)
        assert run_unit(hip, shared, slab, unit, "device", True, call) is None


# ------------------------------------------------------------------ 3: needles one at a time
def test_needles_one_at_a_time(hip, shared, slab):
    """a bitmap that selects needle k and 4,000 background elements far from it, and -q 60, which only a needle passes:
    counters, selected and high are those of exactly that element"""
    import torch
    W, col = slab.W, slab.col
    none = np.zeros(po.LEN_S, dtype=bool)
    bitmap = shared.bitmap(0, [], n=slab.n, pattern=none)
    block = bitmap[PAD + po.BLOCK_AT // 8 - 1:PAD + (po.BLOCK_AT + po.BLOCK_LEN) // 8 + 2]
    bits = np.zeros(block.numel() * 8, dtype=bool)
    lo = po.BLOCK_AT - 8 * (po.BLOCK_AT // 8 - 1)
    bits[lo:lo + po.BLOCK_LEN] = True
    block.copy_(torch.from_numpy(np.packbits(bits, bitorder="little")).cuda())
    whole = np.array([0, slab.n], dtype=np.int64)
    for k in sorted(col.needles):
        Shared.set_bit(bitmap, k, True)
        for filt in (False, True):
            pred = (0, 0, 60) if filt else (0, 0, 0)
            want = po.union_expect(col, po.one_needle_ranges(k), superset=True, min_mapq=pred[2])
            alone = col.expect([k, k + 1], superset=True)
            if filt:
                assert int(want.selected[0]) == 1 and np.array_equal(want.rows, alone.rows)
            else:
                assert int(want.selected[0]) == 1 + po.BLOCK_LEN
            assert int(want.high_read[0]) & int(alone.high_read[0]) == int(alone.high_read[0]) and (W == 2 or int(alone.high_read[0]))
            unit = (W > 2, False, filt, True)
            a = {"A": slab.base, "N": slab.n, "W": W, "R": 0, "X": 0, "MQ": pred[2], "Q": shared.mapq.data_ptr() + PAD if filt else None,
                 "S": bitmap.data_ptr() + PAD, "SO": 0, "SB": 1, "FLAGS": STORE | SUPERSET}
            out = torch.full((34,), GARBAGE, dtype=torch.int64, device="cuda")
            a["OUT"], a["SEL"], a["HIGH"] = out.data_ptr(), out.data_ptr() + 256, out.data_ptr() + 264
            name = entry_name(unit, "device")
            assert getattr(hip, name)(*arguments(unit, a, True)) == 0, (name, hip.FLAGSTATS_hip_last_error())
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint64)
            assert np.array_equal(got[:32], want.rows[0]) and got[32] == want.selected[0], (name, k, got.tolist(), want.rows[0].tolist())
            # every selected element is read, so both rules give the same mask: the union's own is that of all its elements
            assert W == 2 or got[33] == want.high_read[0], (name, k, hex(int(got[33])), hex(int(want.high_read[0])))
        Shared.set_bit(bitmap, k, False)
    # the units without a selection: -q 60 passes exactly the needles
    call = dict(case="needles-q60", layout="whole", offsets=whole, pred=(0, 0, 60), form="bytes", sel_offset=0, local=False)
    unit = (W > 2, False, True, False)
    assert int(slab.want(call, True, False).selected[0]) == len(col.needles)
    assert run_unit(hip, shared, slab, unit, "device", True, call) is None
    del bitmap


# ------------------------------------------------------------------ 4: segmented units on three layouts
@pytest.mark.parametrize("layout", ["blocks", "one", "around"])
def test_segmented_units_on_layouts(hip, shared, slab, layout):
    call = [c for c in po.slab_calls(slab.W) if c["case"] == layout][0]
    o = call["offsets"]
    if layout == "around":
        mark = po.MARK[slab.W]
        assert o.size > 3000 and (np.diff(o[1:-1]) <= 2000).all() and o[1] < mark < o[-2] and slab.n - 1 in slab.col.needles
    for unit in units_of(slab, SEGMENTED):
        for form in ("device", "sync"):
            for store in (True, False):
                assert run_unit(hip, shared, slab, unit, form, store, call) is None


# ------------------------------------------------------------------ 7: the Python layer, one call per module
def test_python_layer_on_the_resident_slab(hip, shared, slab):
    import torch
    from libflagstats_amd import (filter, filter_where, segments, segments_filter, segments_filter_where, segments_where,  # noqa: F401
                                  segments_wide, segments_wide_filter, segments_wide_filter_where, segments_wide_where, where, wide,
                                  wide_filter, wide_filter_where, wide_where)
    from libflagstats_amd import filter_rf, wide_filter_rf
    W, t, n = slab.W, slab.body, slab.n
    calls = {c["case"]: c for c in po.slab_calls(W)}
    flat, seg = calls["whole-bitmap-big-p1"], calls["one"]
    assert flat["sel_offset"] == seg["sel_offset"] == po.BIG_OFFSET
    bitmap = shared.bitmaps[po.BIG_OFFSET][PAD:]
    mapq = shared.mapq[PAD:PAD + n]
    offsets = torch.from_numpy(seg["offsets"]).cuda()
    sel = dict(packed=True, bit_offset=po.BIG_OFFSET)
    fp = dict(require=flat["pred"][0], exclude=flat["pred"][1], mapq=mapq, min_mapq=flat["pred"][2])
    assert fp["min_mapq"] == 30
    sp = dict(require=seg["pred"][0], exclude=seg["pred"][1], mapq=mapq, min_mapq=seg["pred"][2])
    common = dict(store=True, superset=True)
    if W == 2:
        runs = [((False, False, False, True), flat, lambda: where.count_torch_where(t, bitmap, **sel, **common)),
                ((False, False, True, False), flat, lambda: filter.count_torch_filter(t, **fp, **common)),
                ((False, False, True, True), flat, lambda: filter_where.count_torch_filter_where(t, bitmap, **fp, **sel, **common)),
                ((False, True, False, False), seg, lambda: (segments.count_segments_torch(t, offsets, **common),)),
                ((False, True, False, True), seg, lambda: segments_where.count_segments_torch_where(t, offsets, bitmap, **sel, **common)),
                ((False, True, True, False), seg, lambda: segments_filter.count_segments_torch_filter(t, offsets, **sp, **common)),
                ((False, True, True, True), seg,
                 lambda: segments_filter_where.count_segments_torch_filter_where(t, offsets, bitmap, **sp, **sel, **common))]
    else:
        runs = [((True, False, False, False), flat, lambda: wide.count_torch_ints(t, **common)),
                ((True, False, False, True), flat, lambda: wide_where.count_torch_ints_where(t, bitmap, **sel, **common)),
                ((True, False, True, False), flat, lambda: wide_filter.count_torch_ints_filter(t, **fp, **common)),
                ((True, False, True, True), flat, lambda: wide_filter_where.count_torch_ints_filter_where(t, bitmap, **fp, **sel, **common)),
                ((True, True, False, False), seg, lambda: segments_wide.count_segments_torch_ints(t, offsets, **common)),
                ((True, True, False, True), seg, lambda: segments_wide_where.count_segments_torch_ints_where(t, offsets, bitmap, **sel, **common)),
                ((True, True, True, False), seg, lambda: segments_wide_filter.count_segments_torch_ints_filter(t, offsets, **sp, **common)),
                ((True, True, True, True), seg,
                 lambda: segments_wide_filter_where.count_segments_torch_ints_filter_where(t, offsets, bitmap, **sp, **sel, **common))]
    rf_call = po.rf_slab_calls(W)[1]                 # the whole slab under -F 0x904 --rf 0x60 -G 0x3 -q 30
    rp = dict(require=rf_call["pred"][0], exclude=rf_call["pred"][1], include_any=rf_call["rf"][0], exclude_all=rf_call["rf"][1], mapq=mapq,
              min_mapq=rf_call["pred"][2])
    assert rp["min_mapq"] == 30 and rf_call["layout"] == "whole"
    if W == 2:
        runs.append((RF[0], rf_call, lambda: filter_rf.count_torch_filter_rf(t, **rp, **common)))
        from libflagstats_amd import segments_filter_rf
        rs_call = [c for c in po.rf_segments_slab_calls() if c["case"] == "rf-one-b1"][0]      # [7, n - 3) under -F 0x4 --rf 0x60 -G 0x11 -q 30
        rsp = dict(require=rs_call["pred"][0], exclude=rs_call["pred"][1], include_any=rs_call["rf"][0], exclude_all=rs_call["rf"][1],
                   mapq=mapq, min_mapq=rs_call["pred"][2])
        rs_offsets = torch.from_numpy(rs_call["offsets"]).cuda()
        assert rsp["min_mapq"] == 30 and rs_call["layout"] == "one"
        runs.append((RF[2], rs_call, lambda: segments_filter_rf.count_segments_torch_filter_rf(t, rs_offsets, **rsp, **common)))
    else:
        runs.append((RF[1], rf_call, lambda: wide_filter_rf.count_torch_ints_filter_rf(t, **rp, **common)))
    for unit, call, run in runs:
        wide_, _, filt, mask = unit[:4]
        want = slab.want(call, filt, mask)
        got = [x.cpu().numpy().view(np.uint64) for x in run()]
        torch.cuda.synchronize()
        wants = [want.rows] + ([want.selected] if filt or mask else []) + ([want.high(mask)] if wide_ else [])
        assert len(got) == len(wants), (stem(unit), len(got))
        for g, w in zip(got, wants):
            assert np.array_equal(g.ravel(), w.ravel()), (stem(unit), g.ravel()[:40].tolist(), w.ravel()[:40].tolist())


# ------------------------------------------------------------------ 5: one workgroup past 2^32
def launch(hip, name, *argv):
    """one direct launch, synchronized on both sides; its wall time is printed (``pytest -s`` shows it), never asserted"""
    import time
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = getattr(hip, name)(*argv, None)
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    print("%s at grid %d: %.1f ms" % (name, argv[-1], 1e3 * (time.perf_counter() - t0)))


@pytest.mark.parametrize("slab", [2, 4], indirect=True)
def test_one_workgroup_past_2_pow_32(hip, shared, slab):
    """grid 1 through the launchers themselves, under a selection and a predicate so dense that ``selected`` and slot 9 of the
    one workgroup pass 2^32 (the oracle says so): the epilogues' 64-bit sums.  Among the needles every other one is deselected
    and the rest have MAPQ 0, so none counts under -q 1 -- unless an element reads another's bit or byte."""
    import torch
    W, n = slab.W, slab.n
    col = po.column(W, dense=True)
    needles = po.needle_positions(n)
    whole = np.array([0, n], dtype=np.int64)
    dense = shared.bitmap(0, [], n=n, pattern=np.ones(po.LEN_S, dtype=bool))
    quiet = torch.tensor([p for p, i in needles.items() if i % 2 == 1], dtype=torch.int64, device="cuda") + PAD
    for p, i in needles.items():
        if i % 2 == 0:
            Shared.set_bit(dense, p, False)
    A, Q, S = slab.base, shared.mapq.data_ptr() + PAD, dense.data_ptr() + PAD
    mode = STORE | SUPERSET
    try:
        shared.mapq[quiet] = 0
        kinds = ((False, True), (True, False), (True, True)) if W == 2 else ((True, True),)
        for filt, mask in kinds:
            want = col.expect(whole, superset=True, **po.reduced(po.DENSE_CALL, filt, mask))
            assert int(want.selected[0]) > 1 << 32 and int(want.rows[0, 9]) > 1 << 32
            out = torch.full((34,), GARBAGE, dtype=torch.int64, device="cuda")
            OUT, SEL, HIGH = out.data_ptr(), out.data_ptr() + 256, out.data_ptr() + 264
            if W == 4:
                launch(hip, "fsk_launch_wide_filter_where", A, n, 4, 0, 0, Q, 1, S, 0, 1, OUT, SEL, HIGH, mode, 1)
            elif filt and mask:
                launch(hip, "fsk_launch_filter_where", A, n, 0, 0, Q, 1, S, 0, 1, OUT, SEL, mode, 1)
            elif filt:
                launch(hip, "fsk_launch_filter", A, n, 0, 0, Q, 1, OUT, SEL, mode, 1)
            else:
                launch(hip, "fsk_launch_where", A, n, S, 0, 1, OUT, SEL, mode, 1)
            got = out.cpu().numpy().view(np.uint64)
            assert np.array_equal(got[:32], want.rows[0]) and got[32] == want.selected[0], (W, filt, mask, got.tolist(), want.rows[0].tolist())
            assert W == 2 or got[33] == want.high_selected[0], (hex(int(got[33])), hex(int(want.high_selected[0])))
        if W == 2:
            want = col.expect(whole, superset=True, **po.reduced(po.DENSE_CALL, True, True))
            offsets = torch.from_numpy(whole).cuda()
            rows = torch.full((1, 32), GARBAGE, dtype=torch.int64, device="cuda")
            selected = torch.full((1,), GARBAGE, dtype=torch.int64, device="cuda")
            launch(hip, "fsk_launch_segments_filter_where", A, Q, S, 0, 1, 0, n, offsets.data_ptr(), 1, 0, 0, 1, rows.data_ptr(),
                   selected.data_ptr(), mode, 1)
            assert np.array_equal(rows.cpu().numpy().view(np.uint64), want.rows) and int(selected.item()) == int(want.selected[0])
    finally:
        shared.mapq[quiet] = po.NEEDLE_MAPQ
        torch.cuda.synchronize()
    del dense


@pytest.mark.parametrize("slab", [2, 4], indirect=True)
def test_rf_units_one_workgroup_past_2_pow_32(hip, shared, slab):
    """grid 1 through fsk_launch_filter_rf (uint16) and fsk_launch_wide_filter_rf (int32) under po.RF_DENSE, a residue predicate
    that all but a few background flags pass, and -q 1 with the MAPQ of every other needle 0: ``selected`` and slot 9 of the one
    workgroup pass 2^32 (the oracle says so).  Launch-only times beside the positional-popcount yardstick:
    tests/perf/grid1_rf_vs_pospopcnt.py -- int32 491 ms, inside the yardstick scaled by bytes plus 15 % (516 ms); uint16 403 ms
    against 310 ms, over it (DESIGN.md section 7 says why)"""
    import torch
    W, n = slab.W, slab.n
    col = po.column(W, dense=True)
    quiet = torch.tensor([p for p, i in po.needle_positions(n).items() if i % 2 == 1], dtype=torch.int64, device="cuda") + PAD
    require, exclude, include_any, exclude_all, min_mapq = po.RF_DENSE
    want = col.expect(np.array([0, n], dtype=np.int64), require, exclude, min_mapq, superset=True, include_any=include_any, exclude_all=exclude_all)
    assert int(want.selected[0]) > 1 << 32 and int(want.rows[0, 9]) > 1 << 32 and int(want.selected[0]) < n
    A, Q = slab.base, shared.mapq.data_ptr() + PAD
    out = torch.full((34,), GARBAGE, dtype=torch.int64, device="cuda")
    OUT, SEL, HIGH = out.data_ptr(), out.data_ptr() + 256, out.data_ptr() + 264
    try:
        shared.mapq[quiet] = 0
        if W == 2:
            launch(hip, "fsk_launch_filter_rf", A, n, require, exclude, include_any, exclude_all, Q, min_mapq, OUT, SEL, STORE | SUPERSET, 1)
        else:
            launch(hip, "fsk_launch_wide_filter_rf", A, n, 4, require, exclude, include_any, exclude_all, Q, min_mapq, OUT, SEL, HIGH,
                   STORE | SUPERSET, 1)
        got = out.cpu().numpy().view(np.uint64)
    finally:
        shared.mapq[quiet] = po.NEEDLE_MAPQ
        torch.cuda.synchronize()
    assert np.array_equal(got[:32], want.rows[0]) and got[32] == want.selected[0], (W, got.tolist(), want.rows[0].tolist())
    assert W == 2 or got[33] == want.high_read[0], (hex(int(got[33])), hex(int(want.high_read[0])))


# ------------------------------------------------------------------ 8: the segmented unit of the whole predicate (uint16 only)
@pytest.mark.parametrize("slab", [2], indirect=True)
@pytest.mark.parametrize("layout", ["blocks", "one", "around"])
def test_rf_segmented_unit_on_layouts(hip, shared, slab, layout):
    """u16_segments_filter_rf on the three layouts, without and with -q 30, in the device form (store and +=) and the _sync form:
    `blocks` under po.RF_PREDICATES; `one` and `around` under po.RF_BOUNDS_PREDICATES, which an element in front of the first
    segment and one behind the last pass (tests/test_periodic_oracle_host.py), so that offsets[0] and offsets[nseg] are tested"""
    calls = [c for c in po.rf_segments_slab_calls() if c["layout"] == layout]
    assert [c["pred"][2] for c in calls] == [0, 30] and all(np.array_equal(c["offsets"], po.layouts(2, slab.n)[layout]) for c in calls)
    for call in calls:
        want = slab.want(call, True, False)
        length = np.diff(call["offsets"]).astype(np.uint64)
        assert (want.selected > 0).sum() > length.size // 2 and (want.selected <= length).all() and want.selected.sum() < length.sum() // 2
        for form in ("device", "sync"):
            for store in (True, False):
                assert run_unit(hip, shared, slab, RF[2], form, store, call) is None


@pytest.mark.parametrize("slab", [2], indirect=True)
def test_rf_segmented_unit_window_past_the_mark(hip, shared, slab):
    """the window that begins past the mark, 2 bytes past a 16-byte boundary, as the whole array of both segmented forms"""
    calls = [c for c in po.rf_segments_slab_calls() if c["local"]]
    assert len(calls) == 2
    for call in calls:
        first = int(call["offsets"][0])
        assert first > po.MARK[2] and (slab.base + first * 2) % 16 == 2
        assert 0 < int(slab.want(call, True, False).selected[0]) < int(call["offsets"][1]) - first
        for form in ("device", "sync"):
            assert run_unit(hip, shared, slab, RF[2], form, True, call, first=first) is None


@pytest.mark.parametrize("slab", [2], indirect=True)
def test_rf_segmented_unit_needles_one_at_a_time(hip, shared, slab):
    """the `around` layout under the residue predicate with -q 60 that one needle alone passes, for every needle inside it:
    exactly one of the 3,002 segments has selected == 1 and the rows of that element, every other row is zero"""
    col = slab.col
    around = po.layouts(2, slab.n)["around"]
    calls = po.rf_needle_calls(col, around)
    assert len(calls) == len(col.needles) - 1 and po.MARK[2] + 1 in dict(calls)
    for k, call in calls:
        want = slab.want(call, True, False)
        seg = int(np.searchsorted(around, k, side="right")) - 1
        assert int(want.selected[seg]) == 1 and int(want.selected.sum()) == 1 and not np.delete(want.rows, seg, axis=0).any()
        assert np.array_equal(want.rows[seg], col.expect([k, k + 1], superset=True).rows[0])
        assert run_unit(hip, shared, slab, RF[2], "device", True, call) is None


@pytest.mark.parametrize("slab", [2], indirect=True)
def test_rf_segmented_unit_one_workgroup_past_2_pow_32(hip, shared, slab):
    """grid 1 through fsk_launch_segments_filter_rf: one segment over the whole slab under po.RF_DENSE and -q 1, the MAPQ of every
    other needle 0 -- ``selected[0]`` and slot 9 of the one workgroup pass 2^32"""
    import torch
    n = slab.n
    col = po.column(2, dense=True)
    quiet = torch.tensor([p for p, i in po.needle_positions(n).items() if i % 2 == 1], dtype=torch.int64, device="cuda") + PAD
    require, exclude, include_any, exclude_all, min_mapq = po.RF_DENSE
    whole = np.array([0, n], dtype=np.int64)
    want = col.expect(whole, require, exclude, min_mapq, superset=True, include_any=include_any, exclude_all=exclude_all)
    assert int(want.selected[0]) == 4_298_113_024 > 1 << 32 and int(want.rows[0, 9]) > 1 << 32 and int(want.selected[0]) < n
    offsets = torch.from_numpy(whole).cuda()
    rows = torch.full((1, 32), GARBAGE, dtype=torch.int64, device="cuda")
    selected = torch.full((1,), GARBAGE, dtype=torch.int64, device="cuda")
    try:
        shared.mapq[quiet] = 0
        launch(hip, "fsk_launch_segments_filter_rf", slab.base, shared.mapq.data_ptr() + PAD, 0, n, offsets.data_ptr(), 1, require, exclude,
               include_any, exclude_all, min_mapq, rows.data_ptr(), selected.data_ptr(), STORE | SUPERSET, 1)
        got, got_selected = rows.cpu().numpy().view(np.uint64), int(selected.item())
    finally:
        shared.mapq[quiet] = po.NEEDLE_MAPQ
        torch.cuda.synchronize()
    assert np.array_equal(got, want.rows) and got_selected == int(want.selected[0]), (got.tolist(), want.rows.tolist(), got_selected)


# ------------------------------------------------------------------ 6: host forms, default chunk_flags
def host_bitmap(col, so):
    """the packed selection of a host column whose element j is bit so + j (so < 8): ones in the unused bits at either end"""
    nbytes = (so + col.n + 7) // 8
    packed = np.resize(np.packbits(col.S[np.arange(8 * po.LEN_S) % po.LEN_S], bitorder="little"), nbytes)
    packed[0] |= (1 << so) - 1
    packed[-1] |= 0xFF & ~((1 << ((so + col.n - 1) & 7) + 1) - 1)
    for p, (_, _, s, _) in col.needles.items():
        at, bit = (so + p) >> 3, 1 << ((so + p) & 7)
        packed[at] = (int(packed[at]) | bit) if s else (int(packed[at]) & ~bit)
    return packed


def host_periodic(period, n):
    """period repeated to n elements, written in place (np.resize would hold a second copy of the 8 GiB while it builds)"""
    out = np.empty(n, dtype=period.dtype)
    k = n // period.size
    out[:k * period.size].reshape(k, period.size)[:] = period
    out[k * period.size:] = period[:n - k * period.size]
    return out


def host_column(col):
    """(values, mapq) of a column on the host, needles included"""
    j = np.arange(po.LEN_F * po.LEN_H, dtype=np.int64)
    flag, hb, _, _ = col.background(j, j, j)
    values = host_periodic((flag.astype(np.uint64) | hb).astype(po.UNSIGNED[col.W]), col.n)
    mapq = host_periodic(col.Q, col.n)
    for p, (f, h, _, q) in col.needles.items():
        values[p], mapq[p] = f | h, q
    return values, mapq


@pytest.fixture(scope="module")
def host_flags():
    """2^32 + 3 * 65536 + 5 flags, their MAPQ column and a bitmap at an odd offset, in host memory; -q 30"""
    col = po.column(2, n=po.HOST_N)
    so = po.HOST_CALL["sel_offset"]
    assert so % 2 == 1 and po.HOST_CALL["pred"] == (0, 0, 30)
    values, mapq = host_column(col)
    yield col, so, values, mapq, host_bitmap(col, so)
    del values, mapq


def test_host_form_past_2_pow_32_flags(hip, host_flags):
    col, so, values, mapq, bitmap = host_flags
    whole = np.array([0, col.n], dtype=np.int64)
    want = col.expect(whole, superset=True, **po.reduced(po.HOST_CALL, True, True))
    out, selected = np.full(32, BIAS, dtype=np.uint64), np.full(1, SEL_BIAS, dtype=np.uint64)
    rc = hip.FLAGSTATS_hip_u16_x64_filter_where(values.ctypes.data, col.n, 0, 0, mapq.ctypes.data, 30, bitmap.ctypes.data, so, 1,
                                                out.ctypes.data, selected.ctypes.data, SUPERSET)
    assert rc == 0, hip.FLAGSTATS_hip_last_error()
    assert np.array_equal(out, want.rows[0] + np.uint64(BIAS)) and selected[0] == want.selected[0] + np.uint64(SEL_BIAS)


def test_host_form_segments_past_2_pow_32_flags(hip, host_flags):
    col, so, values, mapq, bitmap = host_flags
    offsets = np.array(po.HOST_OFFSETS[2], dtype=np.uint64)
    want = col.expect(offsets.astype(np.int64), superset=True, **po.reduced(po.HOST_CALL, True, True))
    nseg = offsets.size - 1
    rows, selected = np.full((nseg, 32), GARBAGE, dtype=np.uint64), np.full(nseg, GARBAGE, dtype=np.uint64)
    rc = hip.FLAGSTATS_hip_u16_x64_segments_filter_where(values.ctypes.data, col.n, offsets.ctypes.data, nseg, 0, 0, mapq.ctypes.data, 30,
                                                         bitmap.ctypes.data, so, 1, rows.ctypes.data, selected.ctypes.data, STORE | SUPERSET)
    assert rc == 0, hip.FLAGSTATS_hip_last_error()
    assert np.array_equal(rows, want.rows) and np.array_equal(selected, want.selected)


def test_host_form_rf_segments_past_2_pow_32_flags(hip, host_flags):
    """FLAGSTATS_hip_u16_x64_segments_filter_rf on the host column: -F 0x4 --rf 0x60 -G 0x11 -q 30 over po.HOST_OFFSETS[2], which
    leave elements that pass in front of the first segment and behind the last; a chunk's MAPQ slice rides behind its flags and
    the launcher's `base` passes 2^32"""
    col, _, values, mapq, _ = host_flags
    offsets = np.array(po.HOST_OFFSETS[2], dtype=np.uint64)
    require, exclude, include_any, exclude_all, min_mapq = po.RF_BOUNDS_PREDICATES[1]
    want = col.expect(offsets.astype(np.int64), require, exclude, min_mapq, superset=True, include_any=include_any, exclude_all=exclude_all)
    nseg = offsets.size - 1
    assert min_mapq == 30 and (want.selected > 0).all() and (want.selected < np.diff(offsets)).all()
    rows, selected = np.full((nseg, 32), GARBAGE, dtype=np.uint64), np.full(nseg, GARBAGE, dtype=np.uint64)
    rc = hip.FLAGSTATS_hip_u16_x64_segments_filter_rf(values.ctypes.data, col.n, offsets.ctypes.data, nseg, require, exclude, include_any,
                                                      exclude_all, mapq.ctypes.data, min_mapq, rows.ctypes.data, selected.ctypes.data,
                                                      STORE | SUPERSET)
    assert rc == 0, hip.FLAGSTATS_hip_last_error()
    assert np.array_equal(rows, want.rows) and np.array_equal(selected, want.selected)


def test_host_form_wide_past_2_pow_32_bytes(hip):
    """W = 8 and 2^29 + 65541 elements: the byte offset ``pos * W`` of a chunk passes 2^32"""
    col = po.column(8, n=po.HOST_WIDE_N)
    so = po.HOST_CALL["sel_offset"]
    values, _ = host_column(col)
    bitmap = host_bitmap(col, so)
    want = col.expect(np.array(po.HOST_OFFSETS[8], dtype=np.int64), superset=True, **po.reduced(po.HOST_CALL, False, True))
    out = np.full(34, GARBAGE, dtype=np.uint64)
    rc = hip.FLAGSTATS_hip_wide_x64_where(values.ctypes.data, col.n, 8, bitmap.ctypes.data, so, 1, out.ctypes.data, out.ctypes.data + 256,
                                          out.ctypes.data + 264, STORE | SUPERSET)
    assert rc == 0, hip.FLAGSTATS_hip_last_error()
    assert np.array_equal(out[:32], want.rows[0]) and out[32] == want.selected[0] and out[33] == want.high_selected[0]


def test_host_form_rf_past_2_pow_32_flags(hip, host_flags):
    """FLAGSTATS_hip_u16_x64_filter_rf on the host column: -F 0x904 --rf 0x60 -G 0x3 -q 30"""
    col, _, values, mapq, _ = host_flags
    require, exclude, include_any, exclude_all, min_mapq = po.RF_PREDICATES[1]
    want = col.expect(np.array([0, col.n], dtype=np.int64), require, exclude, min_mapq, superset=True, include_any=include_any,
                      exclude_all=exclude_all)
    assert min_mapq == 30 and 0 < int(want.selected[0]) < col.n
    out, selected = np.full(32, BIAS, dtype=np.uint64), np.full(1, SEL_BIAS, dtype=np.uint64)
    rc = hip.FLAGSTATS_hip_u16_x64_filter_rf(values.ctypes.data, col.n, require, exclude, include_any, exclude_all, mapq.ctypes.data, min_mapq,
                                             out.ctypes.data, selected.ctypes.data, SUPERSET)
    assert rc == 0, hip.FLAGSTATS_hip_last_error()
    assert np.array_equal(out, want.rows[0] + np.uint64(BIAS)) and selected[0] == want.selected[0] + np.uint64(SEL_BIAS)
