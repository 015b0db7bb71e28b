"""CPU: tests/periodic_oracle.py, the exact reference of the GPU tests past 2^32 (tests/test_gpu_derived_limits.py).
(a) The oracle against every brute-force oracle of the family, on columns of a few million elements with random phases,
    selection offsets, segment offsets and needles.
(b) For every call of the GPU module, the wrapped models: a kernel that held the array's byte offset, the selection index, the
    MAPQ index or a segment offset in 32 bits (modulo 2^31, modulo 2^32, or sign-extended) would report something else than the
    truth in the very quantities the GPU test compares -- so a subtly wrong kernel fails there, and no GPU run of broken code is
    needed to know it.
(c) The same two for the units of the whole predicate (--rf / -G): the oracle with include_any / exclude_all against
    filter_rf_oracle and wide_filter_rf_oracle, what the chosen predicates do to the needles and to the library's dispatch, and
    the wrapped models against every rf call of the GPU module.
(d) And for the segmented unit of the whole predicate: the oracle against segments_filter_rf_oracle, that the predicates of the
    `one` and `around` layouts test the segment bounds, what the one-needle calls of `around` must report, and the wrapped
    models -- the segment offsets among them -- against every call of that unit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_oracle  # noqa: E402
import filter_rf_oracle  # noqa: E402
import filter_where_oracle  # noqa: E402
import periodic_oracle as po  # noqa: E402
import segments_filter_oracle  # noqa: E402
import segments_filter_rf_oracle  # noqa: E402
import segments_filter_where_oracle  # noqa: E402
import segments_oracle  # noqa: E402
import segments_where_oracle  # noqa: E402
import segments_wide_filter_oracle  # noqa: E402
import segments_wide_filter_where_oracle  # noqa: E402
import segments_wide_oracle  # noqa: E402
import segments_wide_where_oracle  # noqa: E402
import where_oracle  # noqa: E402
import wide_filter_oracle  # noqa: E402
import wide_filter_rf_oracle  # noqa: E402
import wide_filter_where_oracle  # noqa: E402
import wide_where_oracle  # noqa: E402


def random_column(W, rng, n):
    F, H, S, Q = po.patterns(W)
    needles = {}
    for i, k in enumerate([0, n - 1] + [int(x) for x in rng.randint(1, n - 1, 4)]):
        needles[k] = (po.NEEDLE_FLAGS[i], 0 if W == 2 else 1 << po.NEEDLE_BITS[W][i], bool(rng.randint(0, 2)), int(rng.randint(0, 256)))
    return po.Column(W, n, rng.permutation(F), rng.permutation(H), rng.permutation(S), rng.permutation(Q), phase=int(rng.randint(0, 5000)),
                     needles=needles)


def random_offsets(col, rng):
    n = col.n
    cuts = np.sort(rng.randint(0, n + 1, 40))
    near = [k + d for k in col.needles for d in (0, 1) if 0 <= k + d <= n]      # segments that begin and end at a needle
    return np.unique(np.concatenate([cuts, near])).astype(np.int64)


@pytest.mark.parametrize("W", [2, 4, 8])
def test_oracle_matches_every_brute_force_oracle(W, oracle_mod):
    rng = np.random.RandomState(100 + W)
    n = 2_000_003 + W
    col = random_column(W, rng, n)
    assert col.n > 2 * po.JOINT
    for trial, (require, exclude, min_mapq) in enumerate(po.PREDICATES + ((2, 2, 0), (0, 0x100, 60))):
        sel_offset = int((0, 5, po.BIG_OFFSET, rng.randint(0, 1 << 40), rng.randint(0, 100))[trial])
        superset = bool(trial % 2)
        o = random_offsets(col, rng)
        flat = np.array([o[1], o[-2]], dtype=np.int64)
        v, m, q = col.materialize(0, n, sel_offset)
        low = wide_where_oracle.low16(v) if W > 2 else v
        mq = q if min_mapq else None
        pred = dict(require=require, exclude=exclude, min_mapq=min_mapq)
        same = lambda got, want: all(np.array_equal(np.asarray(g, dtype=np.uint64).ravel(), np.asarray(w, dtype=np.uint64).ravel())  # noqa: E731
                                     for g, w in zip(got, want))
        # segmented, the four kinds on the low 16 bits and the four wide ones
        r = col.expect(o, superset=superset)
        assert np.array_equal(r.rows, segments_oracle.segmented_counters(low, o, superset))
        rf = col.expect(o, superset=superset, **pred)
        assert same((rf.rows, rf.selected), segments_filter_oracle.want(low, o, require, exclude, mq, min_mapq, superset))
        rw = col.expect(o, superset=superset, masked=True, sel_offset=sel_offset)
        assert same((rw.rows, rw.selected), segments_where_oracle.want(low, o, m, superset))
        rfw = col.expect(o, superset=superset, masked=True, sel_offset=sel_offset, **pred)
        assert same((rfw.rows, rfw.selected), segments_filter_where_oracle.want(low, o, m, require, exclude, mq, min_mapq, superset))
        if W > 2:
            assert same((r.rows, r.high_read), segments_wide_oracle.want(v, o, superset))
            assert same((rf.rows, rf.selected, rf.high_read), segments_wide_filter_oracle.want(v, o, require, exclude, mq, min_mapq, superset))
            assert same((rw.rows, rw.selected, rw.high_selected), segments_wide_where_oracle.want(v, o, m, superset))
            assert same((rfw.rows, rfw.selected, rfw.high_selected),
                        segments_wide_filter_where_oracle.want(v, o, m, require, exclude, mq, min_mapq, superset))
        # flat: one segment, compacted and handed to the C reference
        a, b = int(flat[0]), int(flat[1])
        va, ma, qa, la = v[a:b], m[a:b], (None if mq is None else mq[a:b]), low[a:b]
        f = col.expect(flat, superset=superset, **pred)
        assert same((f.rows, f.selected), filter_oracle.want_counters(oracle_mod, la, require, exclude, qa, min_mapq, superset))
        w = col.expect(flat, superset=superset, masked=True, sel_offset=sel_offset)
        assert same((w.rows,), (where_oracle.want_counters(oracle_mod, la, ma, superset),)) and int(w.selected[0]) == int(ma.sum())
        fw = col.expect(flat, superset=superset, masked=True, sel_offset=sel_offset, **pred)
        assert same((fw.rows, fw.selected), filter_where_oracle.want_counters(oracle_mod, la, ma, require, exclude, qa, min_mapq, superset))
        if W > 2:
            c, k, h = wide_filter_oracle.want(oracle_mod, va, require, exclude, qa, min_mapq, superset)
            h = 0 if require & exclude else h         # (that oracle leaves the pair that reads nothing to its caller)
            assert same((f.rows, f.selected, f.high_read), (c, k, h))
            assert same((w.rows, w.selected, w.high_selected), wide_where_oracle.want(oracle_mod, va, ma, superset))
            assert same((fw.rows, fw.selected, fw.high_selected),
                        wide_filter_where_oracle.want(oracle_mod, va, ma, require, exclude, qa, min_mapq, superset))


def test_index_maps_against_a_gather():
    """the maps themselves: ``expect`` under a map equals the brute-force count of the gathered column (small marks stand in for
    2^31 and 2^32, so that the column can be materialized)"""
    rng = np.random.RandomState(7)
    n = 1_700_000
    col = random_column(4, rng, n)
    o = random_offsets(col, rng)
    maps = (((0, 900_000, 0), (900_000, po.INF, -900_000)), ((0, 500_000, 0), (500_000, 1_000_000, -1_000_000), (1_000_000, po.INF, 0)))
    j = np.arange(n, dtype=np.int64)
    for pieces in maps:
        for what in ("array_map", "sel_map", "mapq_map"):
            sel_offset = 11
            ja = po.map_indices(pieces, j) if what == "array_map" else j
            je = po.map_indices(pieces, j + sel_offset) - sel_offset if what == "sel_map" else j
            jq = po.map_indices(pieces, j) if what == "mapq_map" else j
            flag, hb, sel, q = col.read(ja, je, jq, sel_offset)
            v = (flag.astype(np.uint64) | hb).astype(np.uint32)
            got = col.expect(o, 0, 0x904, 30, masked=True, sel_offset=sel_offset, superset=True, **{what: pieces})
            rows, selected, high = segments_wide_filter_where_oracle.want(v, o, sel, 0, 0x904, q, 30, True)
            assert np.array_equal(got.rows, rows) and np.array_equal(got.selected, selected) and np.array_equal(got.high_selected, high), what


def assert_detected(found: dict, whats, label):
    """every model that moves an index of the call is told, and each of ``whats`` that the call reads by one model at least"""
    missed = [k for k, hit in found.items() if k[0] in whats and hit is False]
    assert not missed, "%s: a kernel with these wrapped indices would pass: %r" % (label, missed)
    for what in {k[0] for k in found if k[0] in whats}:
        assert any(hit for k, hit in found.items() if k[0] == what), (label, what)
    assert any(k[0] in whats for k in found), label


@pytest.mark.parametrize("W", [2, 4, 8])
def test_wrapped_models_fail_every_slab_call(W):
    col = po.column(W)
    found = {}                                    # calls that differ only in what a kernel does not take are one call to it
    for call in po.slab_calls(W):
        segmented = len(call["offsets"]) > 2
        for filt in (False, True):
            for mask in (False, True):
                if call["local"] and not mask:
                    continue                      # a window without a selection holds no index past the mark
                whats = ("selection",) if call["local"] else ("array", "offsets", "selection", "mapq") if segmented else ("array", "selection", "mapq")
                key = po.call_key(call, filt, mask)
                if key not in found:
                    found[key] = col.detects(call["offsets"], superset=True, **po.reduced(call, filt, mask))
                assert_detected(found[key], whats, (W, call["case"], filt, mask))


@pytest.mark.parametrize("W", [2, 4, 8])
def test_wrapped_models_fail_the_one_needle_calls(W):
    """every model is told by the call of at least one needle (a needle below 2^31 bytes cannot tell any)"""
    col = po.column(W)
    for filt in (False, True):
        pred = dict(min_mapq=60) if filt else {}
        found = {}
        for k in col.needles:
            truth = po.union_expect(col, po.one_needle_ranges(k), **pred)
            if filt:                                  # counters and selected are those of exactly that element
                alone = col.expect([k, k + 1])
                assert int(truth.selected[0]) == 1 and np.array_equal(truth.rows, alone.rows) and alone.rows[0, [10, 25]].any()
            for model in po.MODELS:
                tries = {"array": po.union_expect(col, po.one_needle_ranges(k), array_map=po.wrapped(model, W), **pred),
                         "selection": po.union_expect(col, po.one_needle_ranges(k, po.wrapped(model)), **pred)}
                if filt:
                    tries["mapq"] = po.union_expect(col, po.one_needle_ranges(k), mapq_map=po.wrapped(model), **pred)
                for what, got in tries.items():
                    moved = po.delta_at(po.wrapped(model, W if what == "array" else 1), k) != 0
                    hit = (not truth.same(got, True, W > 2)) if moved else None
                    found[(what, model)] = found.get((what, model)) or hit
        assert_detected(found, ("array", "selection", "mapq"), (W, filt))


def test_wrapped_models_fail_the_one_workgroup_calls():
    for W, kinds in ((2, ((False, True), (True, False), (True, True))), (4, ((True, True),))):
        col = po.column(W, dense=True)
        whole = np.array([0, col.n], dtype=np.int64)
        for filt, mask in kinds:
            kw = po.reduced(po.DENSE_CALL, filt, mask)
            truth = col.expect(whole, superset=True, **kw)
            assert int(truth.selected[0]) > 1 << 32 and int(truth.rows[0, 9]) > 1 << 32       # one workgroup's total passes 2^32
            assert_detected(col.detects(whole, superset=True, **kw), ("array", "selection", "mapq"), (W, filt, mask))


def test_wrapped_models_fail_the_host_calls():
    col = po.column(2, n=po.HOST_N)
    kw = po.reduced(po.HOST_CALL, True, True)
    assert_detected(col.detects(np.array([0, col.n]), **kw), ("array", "selection", "mapq"), "flat")
    assert_detected(col.detects(np.array(po.HOST_OFFSETS[2]), **kw), ("array", "selection", "mapq", "offsets"), "segments")
    wide = po.column(8, n=po.HOST_WIDE_N)
    found = wide.detects(np.array(po.HOST_OFFSETS[8]), **po.reduced(po.HOST_CALL, False, True))
    # 2^29 + 65541 elements: only the byte offset pos * W passes 2^32 -- no selection index does
    assert_detected(found, ("array",), "wide")


# ------------------------------------------------------------------ the two units of the whole predicate (--rf / -G)
def rf_kw(pred):
    require, exclude, include_any, exclude_all, min_mapq = pred
    return dict(require=require, exclude=exclude, include_any=include_any, exclude_all=exclude_all, min_mapq=min_mapq)


def all_rf_predicates():
    return po.RF_PREDICATES + (po.RF_DENSE,) + tuple(po.needle_rf_predicate(f) for f in po.NEEDLE_FLAGS)


@pytest.mark.parametrize("W", [2, 4, 8])
def test_oracle_matches_the_rf_brute_force_oracles(W, oracle_mod):
    """``expect`` with include_any / exclude_all against filter_rf_oracle and wide_filter_rf_oracle on a materialized window:
    the predicates of the GPU tests, two of the one-needle predicates, and masks that no FLAG value satisfies"""
    rng = np.random.RandomState(200 + W)
    n = 2_000_003 + W
    col = random_column(W, rng, n)
    o = random_offsets(col, rng)
    a, b = int(o[1]), int(o[-2])
    v, _, q = col.materialize(0, n)
    preds = po.RF_PREDICATES + (po.RF_DENSE, po.needle_rf_predicate(po.NEEDLE_FLAGS[0]), po.needle_rf_predicate(po.NEEDLE_FLAGS[3]),
                                (0, 0x30, 0x30, 0, 0), (0x3, 0, 0, 0x3, 20), (0, 0, 0x8100, 0xC001, 0))
    for trial, pred in enumerate(preds):
        superset = bool(trial % 2)
        kw = rf_kw(pred)
        got = col.expect(np.array([a, b]), superset=superset, **kw)
        args = (kw["require"], kw["exclude"], kw["include_any"], kw["exclude_all"], q[a:b] if kw["min_mapq"] else None, kw["min_mapq"], superset)
        if W == 2:
            rows, selected = filter_rf_oracle.want_counters(oracle_mod, v[a:b], *args)
            high = 0
        else:
            rows, selected, high = wide_filter_rf_oracle.want(oracle_mod, v[a:b], *args)
        assert np.array_equal(got.rows[0], rows) and int(got.selected[0]) == selected and int(got.high_read[0]) == high, (W, pred)
        assert selected == 0 if trial in (5, 6) else selected > 0 or trial in (3, 4), (pred, selected)     # (the random needles' MAPQ)
    assert not po.satisfiable(0, 0x30, 0x30, 0) and not po.satisfiable(0x3, 0, 0, 0x3) and po.satisfiable(*po.RF_DENSE[:4])


def test_rf_predicates_are_what_the_gpu_tests_need():
    """among the eleven needle flags at least three pass and three fail each of the two tests of RF_PREDICATES; every predicate of
    the GPU tests leaves a residue, so that the rf kernel and not the parent's runs (the dispatch kind of the library's own host
    reduction -- a classification, no expected value); every one-needle predicate passes exactly its needle"""
    import ctypes
    from libflagstats_amd import _lib
    reduce_ = _lib.lib().fsk_filter_rf_reduce
    flags = np.array(po.NEEDLE_FLAGS, dtype=np.uint16)
    for require, exclude, include_any, exclude_all, _ in po.RF_PREDICATES:
        assert po.flag_pass(flags, require, exclude).all()
        any_of, all_of = po.flag_pass(flags, 0, 0, include_any, 0), po.flag_pass(flags, 0, 0, 0, exclude_all)
        assert 3 <= any_of.sum() <= flags.size - 3 and 3 <= all_of.sum() <= flags.size - 3
    assert po.RF_PREDICATES[0][4] == 0 and po.RF_PREDICATES[1] == po.RF_PREDICATES[0][:4] + (30,)
    out = (ctypes.c_uint32 * 4)()
    for pred in all_rf_predicates():
        assert reduce_(*pred[:4], out) == 2 and (out[2] or out[3]), pred
    for require, exclude, include_any, exclude_all, _ in po.RF_PREDICATES + (po.RF_DENSE,):
        assert reduce_(require, exclude, include_any, exclude_all, out) == 2 and out[2] and out[3]       # both tests are left
    for f in po.NEEDLE_FLAGS:
        pred = po.needle_rf_predicate(f)
        assert pred[4] == po.NEEDLE_MAPQ and po.flag_pass(flags, *pred[:4]).tolist() == [g == f for g in po.NEEDLE_FLAGS], hex(f)


@pytest.mark.parametrize("W", [2, 4, 8])
def test_wrapped_models_fail_the_rf_calls(W):
    """the new GPU calls of the rf units: the whole slab under both predicates, the needles one at a time, one workgroup and the
    host form -- each of the three index models, in the array's byte offset and in the MAPQ index, would miss the asserted values
    (a window is handed pointers to its first element: no index of it passes the mark)"""
    col = po.column(W)
    whole = np.array([0, col.n], dtype=np.int64)
    for call in po.rf_slab_calls(W):
        if call["layout"] == "window":
            continue
        kw = po.reduced(call, True, False)
        whats = ("array", "mapq") if kw["min_mapq"] else ("array",)
        assert_detected(col.detects(call["offsets"], superset=True, **kw), whats, (W, call["case"]))
    found = {}
    for k, (flag, _, _, _) in col.needles.items():
        kw = rf_kw(po.needle_rf_predicate(flag))
        truth = col.expect(whole, superset=True, **kw)
        assert int(truth.selected[0]) == 1 and np.array_equal(truth.rows, col.expect([k, k + 1], superset=True).rows)
        for key, hit in col.detects(whole, superset=True, **kw).items():
            found[key] = found.get(key) or hit
    assert_detected(found, ("array", "mapq"), (W, "needles"))
    if W in (2, 4):
        dense = po.column(W, dense=True)
        kw = rf_kw(po.RF_DENSE)
        truth = dense.expect(whole, superset=True, **kw)
        assert int(truth.selected[0]) > 1 << 32 and int(truth.rows[0, 9]) > 1 << 32
        assert_detected(dense.detects(whole, superset=True, **kw), ("array", "mapq"), (W, "one workgroup"))
    if W == 2:
        host = po.column(2, n=po.HOST_N)
        assert_detected(host.detects(np.array([0, host.n]), superset=True, **rf_kw(po.RF_PREDICATES[1])), ("array", "mapq"), "host")


# ------------------------------------------------------------------ the segmented unit of the whole predicate
def rf_segmented_want(v, o, q, pred, superset):
    kw = rf_kw(pred)
    return segments_filter_rf_oracle.want(v, o, kw["require"], kw["exclude"], kw["include_any"], kw["exclude_all"],
                                          q if kw["min_mapq"] else None, kw["min_mapq"], superset)


def test_oracle_matches_the_rf_segmented_brute_force_oracle():
    """``expect`` with include_any / exclude_all over segments against segments_filter_rf_oracle: a random column of two million
    elements under every kind of predicate of the GPU tests, then materialized windows of the slab's own column -- its first and
    last elements and those around 2^32 -- under the `around` layout"""
    rng = np.random.RandomState(302)
    n = 2_000_005
    col = random_column(2, rng, n)
    v, _, q = col.materialize(0, n)
    preds = po.RF_PREDICATES + po.RF_BOUNDS_PREDICATES + (po.RF_DENSE, po.needle_rf_predicate(po.NEEDLE_FLAGS[0]),
                                                          po.needle_rf_predicate(po.NEEDLE_FLAGS[3]), (0, 0x30, 0x30, 0, 0), (0x3, 0, 0, 0x3, 20))
    for trial, pred in enumerate(preds):
        o, superset = random_offsets(col, rng), bool(trial % 2)
        got = col.expect(o, superset=superset, **rf_kw(pred))
        rows, selected = rf_segmented_want(v, o, q, pred, superset)
        assert np.array_equal(got.rows, rows) and np.array_equal(got.selected, selected), pred
        # the one-needle predicates pass what the random needles' MAPQ lets them; the last two pass nothing
        assert selected.any() if trial < 5 else not selected.any() or trial < 7, (pred, selected)
    slab = po.column(2)
    around = po.layouts(2, slab.n)["around"]
    mark = po.MARK[2]
    preds = po.RF_PREDICATES + po.RF_BOUNDS_PREDICATES + (po.needle_rf_predicate(slab.needles[mark + 1][0]),)
    for b, e in ((0, 6000), (mark - 5000, mark + 5000), (slab.n - 6000, slab.n)):
        o = np.unique(np.clip(around, b, e))
        assert o.size >= 2 and (o.size > 5 or not b < mark < e)       # several short segments cross the mark
        v, _, q = slab.materialize(b, e)
        for pred in preds:
            got = slab.expect(o, superset=True, **rf_kw(pred))
            rows, selected = rf_segmented_want(v, o - b, q, pred, True)
            assert np.array_equal(got.rows, rows) and np.array_equal(got.selected, selected), (b, e, pred)


def test_rf_bounds_predicates_test_the_segment_bounds():
    """the condition that a call tests offsets[0] and offsets[nseg]: an element in front of the first segment and one behind the
    last would count.  RF_BOUNDS_PREDICATES meet it on `one` and `around` (but for the three elements in front of `around` under
    -q 30, whose MAPQ is below 30), RF_PREDICATES meet it nowhere; every one of them leaves both tests to the kernel."""
    import ctypes
    from libflagstats_amd import _lib
    reduce_ = _lib.lib().fsk_filter_rf_reduce
    out = (ctypes.c_uint32 * 4)()
    for pred in po.RF_BOUNDS_PREDICATES + po.RF_PREDICATES + (po.RF_DENSE,):
        assert reduce_(*pred[:4], out) == 2 and out[2] and out[3], pred
    assert po.RF_BOUNDS_PREDICATES[0][4] == 0 and po.RF_BOUNDS_PREDICATES[1] == po.RF_BOUNDS_PREDICATES[0][:4] + (30,)
    col = po.column(2)
    lay = po.layouts(2, col.n)

    def outside(column, o, pred):
        head = column.expect([0, int(o[0])], **rf_kw(pred)).selected[0]
        tail = column.expect([int(o[-1]), column.n], **rf_kw(pred)).selected[0]
        return int(head), int(tail)

    for name in ("one", "around"):
        o = lay[name]
        assert 0 < o[0] and o[-1] < col.n
        for pred in po.RF_BOUNDS_PREDICATES:
            head, tail = outside(col, o, pred)
            assert tail >= 1, (name, pred)
            if name == "around" and pred[4] == 30:
                assert head == 0 and (col.materialize(0, int(o[0]))[2] < 30).all()
            else:
                assert head >= 1, (name, pred)
        for pred in po.RF_PREDICATES:
            assert outside(col, o, pred) == (0, 0), (name, pred)
    host = po.column(2, n=po.HOST_N)
    head, tail = outside(host, np.array(po.HOST_OFFSETS[2]), po.RF_BOUNDS_PREDICATES[1])
    assert head >= 1 and tail >= 1


def test_rf_needle_calls_name_one_segment_of_the_around_layout():
    """every needle inside the `around` layout under its own predicate: one segment with selected == 1 and the rows of that
    element alone, every other row zero -- the needle at 2^32 + 1 among them, in one of the short segments that cross the mark"""
    col = po.column(2)
    around = po.layouts(2, col.n)["around"]
    calls = po.rf_needle_calls(col, around)
    assert [k for k, _ in calls] == sorted(k for k in col.needles if k != col.n - 1) and po.MARK[2] + 1 in dict(calls)
    for k, call in calls:
        want = col.expect(around, superset=True, **po.reduced(call, True, False))
        seg = int(np.searchsorted(around, k, side="right")) - 1
        assert want.selected[seg] == 1 and want.selected.sum() == 1
        assert np.array_equal(want.rows[seg], col.expect([k, k + 1], superset=True).rows[0]) and want.rows[seg].any()
        assert not np.delete(want.rows, seg, axis=0).any()
    seg = int(np.searchsorted(around, po.MARK[2] + 1, side="right")) - 1
    assert 0 < seg < around.size - 2 and around[seg + 1] - around[seg] <= 2000


def detects_over_segments(col, offsets, **kw):
    """``col.detects`` of a segmented call, with the models that move none of the call's own offsets taken out (``detects`` asks
    whether a model moves an index between the first and the last offset; [7, n - 3) has no offset for "sext" to move)"""
    found = col.detects(offsets, superset=True, **kw)
    for model in po.MODELS:
        if np.array_equal(po.map_indices(po.wrapped(model), offsets), np.asarray(offsets, dtype=np.int64)):
            found[("offsets", model)] = None
    return found


def test_wrapped_models_fail_the_rf_segmented_calls():
    """the GPU calls of u16_segments_filter_rf: the three layouts, the needles one at a time, one workgroup and the host form --
    each of the three index models, in the array's byte offset, the MAPQ index and the segment offsets, would miss the asserted
    values (a window is handed pointers to its first element and offsets relative to it: no index of it passes the mark)"""
    col = po.column(2)
    calls = po.rf_segments_slab_calls()
    assert sorted(c["layout"] for c in calls) == sorted(2 * ["blocks", "one", "around", "window"])
    for call in calls:
        if call["local"]:
            continue
        kw = po.reduced(call, True, False)
        whats = ("array", "offsets", "mapq") if kw["min_mapq"] else ("array", "offsets")
        assert_detected(detects_over_segments(col, call["offsets"], **kw), whats, call["case"])
    found = {}
    for k, call in po.rf_needle_calls(col, po.layouts(2, col.n)["around"]):
        for key, hit in detects_over_segments(col, call["offsets"], **po.reduced(call, True, False)).items():
            found[key] = found.get(key) or hit
    assert_detected(found, ("array", "offsets", "mapq"), "needles")
    dense = po.column(2, dense=True)
    whole = np.array([0, dense.n], dtype=np.int64)
    truth = dense.expect(whole, superset=True, **rf_kw(po.RF_DENSE))
    assert int(truth.selected[0]) == 4_298_113_024 and int(truth.rows[0, 9]) > 1 << 32
    assert_detected(detects_over_segments(dense, whole, **rf_kw(po.RF_DENSE)), ("array", "offsets", "mapq"), "one workgroup")
    host = po.column(2, n=po.HOST_N)
    assert_detected(detects_over_segments(host, np.array(po.HOST_OFFSETS[2]), **rf_kw(po.RF_BOUNDS_PREDICATES[1])),
                    ("array", "offsets", "mapq"), "host")
