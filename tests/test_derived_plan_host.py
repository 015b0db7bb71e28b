"""CPU: the case plan and the reference of the randomized sweep over the derived kernels (tests/derived_plan.py) -- the reference
against the per-kernel oracles, the plan's determinism, what the default plan covers, and that it skips nothing.  No GPU."""
import ctypes
import hashlib
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import derived_plan as dp  # noqa: E402
import filter_oracle  # noqa: E402
import filter_rf_oracle  # noqa: E402
import filter_where_oracle  # noqa: E402
import segments_filter_where_oracle  # noqa: E402
import segments_filter_oracle  # noqa: E402
import segments_filter_rf_oracle  # noqa: E402
import segments_oracle  # noqa: E402
import segments_wide_filter_oracle  # noqa: E402
import segments_where_oracle  # noqa: E402
import segments_wide_filter_where_oracle  # noqa: E402
import segments_wide_oracle  # noqa: E402
import segments_wide_where_oracle  # noqa: E402
import where_oracle  # noqa: E402
import wide_filter_oracle  # noqa: E402
import wide_filter_rf_oracle  # noqa: E402
import wide_filter_where_oracle  # noqa: E402
import wide_where_oracle  # noqa: E402

SEED = 20261019
DEFAULT_ITERS = 240


@pytest.fixture(scope="module")
def planned(oracle_mod):
    """(plan(SEED, 300), its references, seconds the references of the first DEFAULT_ITERS took): computed once, never changed"""
    cases = dp.plan(SEED, 300)
    refs, spent = [], 0.0
    for c in cases:
        t0 = time.perf_counter()
        refs.append(dp.reference(c))
        if c["index"] < DEFAULT_ITERS:
            spent += time.perf_counter() - t0
    return cases, refs, spent


def low16(case):
    return (case["array"].view(dp.UNSIGNED[case["W"]]) & dp.UNSIGNED[case["W"]](0xFFFF)).astype(np.uint16)


def oracle_of(oracle_mod, c):
    """(rows[nseg, 32], selected[nseg] or None, high[nseg] or None) by the kernel's own oracle, superset form"""
    kind, pred = c["kind"], (c["require"], c["exclude"], c["mapq"], c["min_mapq"])
    one = lambda v: np.array([v], dtype=np.uint64)  # noqa: E731
    if c["family"] == "where":
        return where_oracle.want_counters(oracle_mod, low16(c), c["mask"], True)[None, :], one(int(c["mask"].sum())), None
    if kind == "filter":
        rows, sel = filter_oracle.want_counters(oracle_mod, low16(c), *pred, True)
        return rows[None, :], one(sel), None
    if kind == "segments":
        return segments_oracle.segmented_counters(low16(c), c["offsets"], True), None, None
    if kind == "segments_filter":
        rows, sel = segments_filter_oracle.want(low16(c), c["offsets"], *pred, True)
        return rows, sel, None
    if kind == "wide":
        rows, sel, high = wide_filter_oracle.want(oracle_mod, c["array"], 0, 0, None, 0, True)
        assert sel == c["n"]
        return rows[None, :], None, one(high)
    if kind == "wide_filter":
        rows, sel, high = wide_filter_oracle.want(oracle_mod, c["array"], *pred, True)
        # that oracle reports the column's mask whatever the predicate; an overlapping pair reads no element (the header's contract)
        return rows[None, :], one(sel), one(0 if c["require"] & c["exclude"] else high)
    if kind == "wide_segments":
        rows, high = segments_wide_oracle.want(c["array"], c["offsets"], True)
        return rows, None, high
    assert kind == "wide_segments_filter"
    return segments_wide_filter_oracle.want(c["array"], c["offsets"], *pred, True)


def test_reference_agrees_with_the_per_kernel_oracles(oracle_mod, planned):
    cases, refs, _ = planned
    assert len(cases) == 300
    for c, r in zip(cases, refs):
        rows, sel, high = oracle_of(oracle_mod, c)
        what = dp.describe(c)
        assert rows.shape == r["rows"].shape and np.array_equal(rows, r["rows"]), what
        if sel is not None:
            assert np.array_equal(np.asarray(sel, dtype=np.uint64), r["selected"]), what
        else:
            assert np.array_equal(r["selected"], r["length"]), what
        if high is not None:
            assert np.array_equal(np.asarray(high, dtype=np.uint64), r["high"]), what
        else:
            assert not r["high"].any(), what
        if c["require"] & c["exclude"]:
            assert not r["rows"].any() and not r["selected"].any() and not r["high"].any(), what


def test_expected_applies_the_mode(planned):
    cases, refs, _ = planned
    for c, r in zip(cases[:60], refs):
        rows, sel, high = dp.expected(c, r)
        base = np.uint64(0 if c["mode"] & dp.STORE else dp.BIAS)
        if not c["mode"] & dp.SUPERSET:
            assert (rows[:, [0, 9, 16]] == base).all()
        live = [s for s in range(32) if s not in (0, 9, 16)]
        assert np.array_equal(rows[:, live], r["rows"][:, live] + base)
        assert (sel is None) == (c["selected_at"] not in ("together", "apart"))
        assert (high is None) == (c["high_at"] not in ("together", "apart"))
        if high is not None and not c["mode"] & dp.STORE:
            assert ((high & np.uint64(dp.MASK_BIAS)) == np.uint64(dp.MASK_BIAS)).all()
        images = dp.expected_images(c, r)
        allocs, where = dp.output_layout(c)
        assert len(images) == len(allocs) == 1 + (c["selected_at"] == "apart") + (c["high_at"] == "apart")
        for img, a in zip(images, allocs):
            assert (img[:32] == dp.GARBAGE).all() and (img[-32:] == dp.GARBAGE).all() and img.size == a.size
        if c["selected_at"] == "together":
            assert where["selected"][:2] == (0, 32 + c["nseg"] * 32)


def same_case(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert isinstance(b[k], np.ndarray) and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k] and type(a[k]) is type(b[k]), k


def test_plan_is_deterministic_and_prefix_closed(planned):
    cases = planned[0]
    for k in (0, 1, 35, 36, 37, 80):
        shorter, longer = dp.plan(SEED, k), dp.plan(SEED, k + 1)
        assert len(shorter) == k and len(longer) == k + 1
        for a, b in zip(shorter, longer):
            same_case(a, b)
        for a, b in zip(longer, cases):
            same_case(a, b)
    assert any(a["n"] != b["n"] for a, b in zip(dp.plan(SEED + 1, 10), cases))


def test_default_plan_covers_what_it_is_for(planned):
    cases, refs, _ = planned
    cases, refs = cases[:DEFAULT_ITERS], refs[:DEFAULT_ITERS]
    count = lambda pred: sum(1 for c in cases if pred(c))  # noqa: E731
    for kind in dp.KINDS:
        for form in dp.FORMS:
            assert count(lambda c: c["kind"] == kind and c["form"] == form) >= 3, (kind, form)
    for W in (2, 4, 8):
        assert count(lambda c: c["W"] == W) >= 5, W
    for mode in range(4):
        assert count(lambda c: c["mode"] == mode) >= 5, mode
    for grid in dp.GRIDS:
        assert count(lambda c: c["grid"] == grid) >= 5, grid
    for chunk in dp.CHUNKS:
        assert count(lambda c: c["chunk_flags"] == chunk) >= 5, chunk
    for mu in dp.MIN_UNITS:
        assert count(lambda c: c["policy"] is not None and c["policy"][0] == mu) >= 1, mu
    for name in ("int16", "uint16", "int32", "uint32", "int64", "uint64"):
        assert count(lambda c: c["dtype"] == name) >= 5, name
    assert count(lambda c: c["big_offset"]) >= 1 and count(lambda c: c["kind"] == "where_bitmap" and c["sel_offset"] & 7) >= 5
    assert {c["n_cluster"] for c in cases} == {0, 1, 2, 3} and max(c["n"] for c in cases) <= dp.CAP
    assert sum(c["n"] for c in cases) < 40_000_000
    # a selection that is partly taken in some segment: all but 15 % of the cases of the kinds that select (a kind without a
    # predicate selects every element by definition)
    selecting = [(c, r) for c, r in zip(cases, refs) if c["kind"] in dp.SELECTING]
    partial = [bool(((r["selected"] > 0) & (r["selected"] < r["length"])).any()) for c, r in selecting]
    assert len(selecting) >= 100 and sum(partial) >= 0.85 * len(selecting), (sum(partial), len(selecting))
    overlapping = count(lambda c: bool(c["require"] & c["exclude"]))
    assert 1 <= overlapping <= DEFAULT_ITERS // 12
    for kind in dp.WIDE:
        mine = [(c, r) for c, r in zip(cases, refs) if c["kind"] == kind and not c["require"] & c["exclude"]]
        if kind in dp.SEGMENTED:    # masks in some but not all segments of one call
            assert sum(1 for c, r in mine if r["high"].any() and (r["high"][r["length"] > 0] == 0).any()) >= 3, kind
        assert any(r["high"].any() for c, r in mine) and any(not r["high"].any() and c["n"] for c, r in mine), kind
        assert any(int(r["high"].max()) >> (8 * c["W"] - 1) for c, r in mine), (kind, "the sign bit")
    for kind in dp.SEGMENTED:
        mine = [c for c in cases if c["kind"] == kind]
        assert any((np.diff(c["offsets"]) == 0).any() and (np.diff(c["offsets"]) > 0).any() for c in mine), kind
        assert any(c["offsets"][0] > 0 for c in mine) and any(c["offsets"][-1] < c["n"] for c in mine), kind
        assert {c["nseg"] for c in mine} == set(dp.NSEGS), kind
        assert {c["layout"] for c in mine} == {"random", "units", "runs"}, kind
        assert any((np.diff(c["offsets"]) >= 2 * 8192 // c["W"]).any() for c in mine), (kind, "a segment of chain length")
    for at in dp.PLACEMENTS:
        assert count(lambda c: c["selected_at"] == at) >= 5 and count(lambda c: c["high_at"] == at) >= 5, at


def test_no_case_is_skipped(planned):
    cases = planned[0]
    assert dp.skip_reasons(cases[:DEFAULT_ITERS]) == []
    assert all(c["skip"] is None for c in cases)
    # what the plan narrows instead of skipping: the host forms' chunk count, and where a 2^33 bit offset is applied
    for c in cases:
        if c["form"] == "host":
            assert c["n"] <= dp.MAX_CHUNKS * max(2, c["chunk_flags"] * 2 // c["W"])
        assert not c["big_offset"] or (c["kind"] == "where_bitmap" and c["form"] in ("launcher", "host") and c["sel_offset"] >> 33 == 1)


def test_reference_of_the_default_plan_is_quick(planned):
    assert planned[2] < 20.0, planned[2]


def test_input_images_hold_the_inputs_between_poison(planned):
    for c in planned[0][:80]:
        img, at = dp.array_image(c)
        W, n = c["W"], c["n"]
        assert at % 16 == c["phase"] and img[at:at + n * W].tobytes() == c["array"].tobytes()
        assert (img[:at] == 0xFF).all() and (img[at + n * W:] == 0xFF).all() and at >= 64 * W and img.size - at - n * W >= 64 * W
        if c["mapq"] is not None:
            q, qa = dp.bytes_image(c["mapq"], c["mapq_align"])
            assert qa % 16 == c["mapq_align"] and np.array_equal(q[qa:qa + n], c["mapq"]) and (q[:qa] == 0xFF).all() and (q[qa + n:] == 0xFF).all()
        if c["kind"] == "where_bitmap":
            b, ba, back = dp.bitmap_image(c)
            bits = np.unpackbits(b[ba:], bitorder="little")
            local = c["sel_offset"] - 8 * back
            assert 0 <= local < 64 and np.array_equal(bits[local:local + n].astype(bool), c["mask"])
            assert bits[:local].all() and bits[local + n:].all() and (b[:ba] == 0xFF).all()
            assert np.array_equal(where_oracle.pack(c["mask"], local), b[ba:ba + (local + n + 7) // 8])


# ------------------------------------------------------------------ the old plan is what it was
PLAN_DIGEST = "7f53b51ff32d1c7c94ca21df9c5291ea9ad9ee631bca4d1057d8d9868f1743f3"   # taken before plan_later was written


def plan_digest(cases):
    h = hashlib.sha256()
    for c in cases:
        h.update(repr(dp.describe(c)).encode())
        for k in ("array", "mapq", "mask", "offsets"):
            if c[k] is not None:
                h.update(np.ascontiguousarray(c[k]).tobytes())
    return h.hexdigest()


def test_plan_is_byte_for_byte_what_it_was(planned):
    """sha256 over every case's describe() and the bytes of its array, mapq, mask and offsets: sharing _draw's pieces with
    plan_later has not moved one draw of plan()"""
    assert plan_digest(planned[0]) == PLAN_DIGEST


# ------------------------------------------------------------------ the later plan: the nine units derived afterwards
LATER_SEED = 20261021
MASKED_WIDE = tuple(k for k in dp.MASKED if k in dp.LATER_WIDE)
MASKED_SEGMENTED = tuple(k for k in dp.MASKED if k in dp.LATER_SEGMENTED)
MASKED_FLAT = tuple(k for k in dp.MASKED if k not in dp.LATER_SEGMENTED)
MASKED_FILTERED = tuple(k for k in dp.MASKED if k in dp.LATER_FILTERED)


@pytest.fixture(scope="module")
def planned_later(oracle_mod):
    """planned, of plan_later(LATER_SEED, 300)"""
    cases = dp.plan_later(LATER_SEED, 300)
    refs, spent = [], 0.0
    for c in cases:
        t0 = time.perf_counter()
        refs.append(dp.reference(c))
        if c["index"] < DEFAULT_ITERS:
            spent += time.perf_counter() - t0
    return cases, refs, spent


def later_oracle_of(oracle_mod, c):
    """oracle_of for LATER_KINDS: (rows[nseg, 32], selected[nseg], high[nseg] or None) by the kernel's own oracle, superset form"""
    kind, m, o = c["kind"], c["mask"], c["offsets"]
    pred = (c["require"], c["exclude"], c["mapq"], c["min_mapq"])
    rf = (c["require"], c["exclude"], c["include_any"], c["exclude_all"], c["mapq"], c["min_mapq"])
    one = lambda v: np.array([v], dtype=np.uint64)  # noqa: E731
    if kind == "segments_where":
        return segments_where_oracle.want(low16(c), o, m, True) + (None,)
    if kind == "wide_where":
        rows, sel, high = wide_where_oracle.want(oracle_mod, c["array"], m, True)
        return rows[None, :], one(sel), one(high)
    if kind == "wide_segments_where":
        return segments_wide_where_oracle.want(c["array"], o, m, True)
    if kind == "filter_where":
        rows, sel = filter_where_oracle.want_counters(oracle_mod, low16(c), m, *pred, True)
        return rows[None, :], one(sel), None
    if kind == "segments_filter_where":
        return segments_filter_where_oracle.want(low16(c), o, m, *pred, True) + (None,)
    if kind == "wide_filter_where":
        rows, sel, high = wide_filter_where_oracle.want(oracle_mod, c["array"], m, *pred, True)
        return rows[None, :], one(sel), one(high)
    if kind == "wide_segments_filter_where":
        return segments_wide_filter_where_oracle.want(c["array"], o, m, *pred, True)
    if kind == "filter_rf":
        rows, sel = filter_rf_oracle.want_counters(oracle_mod, low16(c), *rf, True)
        return rows[None, :], one(sel), None
    assert kind == "wide_filter_rf"
    rows, sel, high = wide_filter_rf_oracle.want(oracle_mod, c["array"], *rf, True)
    return rows[None, :], one(sel), one(high)


def test_later_reference_agrees_with_the_per_kernel_oracles(oracle_mod, planned_later):
    cases, refs, _ = planned_later
    assert len(cases) == 300 and {c["kind"] for c in cases} == set(dp.LATER_KINDS)
    for c, r in zip(cases, refs):
        rows, sel, high = later_oracle_of(oracle_mod, c)
        what = dp.describe(c)
        assert rows.shape == r["rows"].shape and np.array_equal(rows, r["rows"]), what
        assert np.array_equal(np.asarray(sel, dtype=np.uint64), r["selected"]), what
        if high is not None:
            assert np.array_equal(np.asarray(high, dtype=np.uint64), r["high"]), what
        else:
            assert not r["high"].any(), what
        if c["require"] & c["exclude"] or c["rf_outcome"] == "empty":
            assert not r["rows"].any() and not r["selected"].any() and not r["high"].any(), what


def test_later_plan_is_deterministic_and_prefix_closed(planned_later):
    cases = planned_later[0]
    for k in (0, 1, 35, 36, 37, 80):
        shorter, longer = dp.plan_later(LATER_SEED, k), dp.plan_later(LATER_SEED, k + 1)
        assert len(shorter) == k and len(longer) == k + 1
        for a, b in zip(shorter, longer):
            same_case(a, b)
        for a, b in zip(longer, cases):
            same_case(a, b)
    assert any(a["n"] != b["n"] for a, b in zip(dp.plan_later(LATER_SEED + 1, 10), cases))


def rf_outcome(reduce_, c):
    """which of dp.RF_OUTCOMES the library's host reduction makes of the case's four masks: a classification of the case for the
    coverage floors below, never an expected value"""
    out = (ctypes.c_uint32 * 4)()
    rc = reduce_(c["require"], c["exclude"], c["include_any"], c["exclude_all"], out)
    return ("empty", "pair", ("any" if out[2] else "all") if not (out[2] and out[3]) else "both")[rc]


def high_over(c, which):
    """OR of the bits above bit 15 over the whole array (which is None) or over the elements `which` marks"""
    above = c["array"].view(dp.UNSIGNED[c["W"]]).astype(np.uint64) & ~np.uint64(0xFFFF)
    return int(np.bitwise_or.reduce(above if which is None else above[which])) if above.size else 0


def test_later_plan_covers_what_it_is_for(planned_later):
    from libflagstats_amd import _lib
    reduce_ = _lib.lib().fsk_filter_rf_reduce
    cases, refs, _ = planned_later
    cases, refs = cases[:DEFAULT_ITERS], refs[:DEFAULT_ITERS]
    count = lambda pred: sum(1 for c in cases if pred(c))  # noqa: E731
    for kind in dp.LATER_KINDS:
        for form in dp.FORMS:
            assert count(lambda c: c["kind"] == kind and c["form"] == form) >= 3, (kind, form)
    for kind in dp.MASKED:
        for bits in (1, 8):
            assert count(lambda c: c["kind"] == kind and c["sel_bits"] == bits) >= 3, (kind, bits)
            for form in dp.FORMS:
                assert count(lambda c: c["kind"] == kind and c["sel_bits"] == bits and c["form"] == form) >= 1, (kind, bits, form)
    for kind in dp.RF:
        seen = [rf_outcome(reduce_, c) for c in cases if c["kind"] == kind]
        assert seen == [c["rf_outcome"] for c in cases if c["kind"] == kind], kind      # the plan dealt what the reduction finds
        for outcome in dp.RF_OUTCOMES:
            assert seen.count(outcome) >= 3, (kind, outcome)
        assert any((c["include_any"] | c["exclude_all"]) & 0xFF00 for c in cases if c["kind"] == kind), kind
    for kind in MASKED_FLAT:
        assert count(lambda c: c["kind"] == kind and c["big_offset"]) >= 1, kind
    for kind in MASKED_WIDE:
        mine = [c for c in cases if c["kind"] == kind and not c["require"] & c["exclude"]]
        assert sum(1 for c in mine if high_over(c, None) != high_over(c, c["mask"])) >= 3, kind
        ones = [c for c in mine if c["high_style"] == "one" and c["n"] >= 3]
        assert any(high_over(c, c["mask"]) == 0 for c in ones) and any(high_over(c, c["mask"]) != 0 for c in ones), kind
    for kind in MASKED_SEGMENTED:
        assert count(lambda c: c["kind"] == kind and c["offsets"][0] > 0) >= 3, kind
    # what test_default_plan_covers_what_it_is_for asserts of the old plan, where it applies
    for W in (2, 4, 8):
        assert count(lambda c: c["W"] == W) >= 5, W
    for mode in range(4):
        assert count(lambda c: c["mode"] == mode) >= 5, mode
    for grid in dp.GRIDS:
        assert count(lambda c: c["grid"] == grid) >= 5, grid
    for chunk in dp.CHUNKS:
        assert count(lambda c: c["chunk_flags"] == chunk) >= 5, chunk
    for mu in dp.MIN_UNITS:
        assert count(lambda c: c["policy"] is not None and c["policy"][0] == mu) >= 1, mu
    for name in ("int16", "uint16", "int32", "uint32", "int64", "uint64"):
        assert count(lambda c: c["dtype"] == name) >= 5, name
    assert count(lambda c: c["sel_bits"] == 1 and c["sel_offset"] & 7) >= 5 and count(lambda c: c["sel_bits"] == 8 and c["sel_offset"] & 1) >= 5
    assert {c["n_cluster"] for c in cases} == {0, 1, 2, 3} and max(c["n"] for c in cases) <= dp.CAP
    assert sum(c["n"] for c in cases) < 40_000_000
    # every later kind selects: a selection partly taken in some segment in all but 15 % of the cases
    partial = [bool(((r["selected"] > 0) & (r["selected"] < r["length"])).any()) for r in refs]
    assert sum(partial) >= 0.85 * len(cases), (sum(partial), len(cases))
    overlapping = count(lambda c: bool(c["require"] & c["exclude"]) and c["kind"] not in dp.RF)
    assert 1 <= overlapping <= DEFAULT_ITERS // 12
    for kind in dp.LATER_WIDE:
        mine = [(c, r) for c, r in zip(cases, refs) if c["kind"] == kind and not c["require"] & c["exclude"]]
        if kind in dp.LATER_SEGMENTED:    # masks in some but not all segments of one call
            assert sum(1 for c, r in mine if r["high"].any() and (r["high"][r["length"] > 0] == 0).any()) >= 3, kind
        assert any(r["high"].any() for c, r in mine) and any(not r["high"].any() and c["n"] for c, r in mine), kind
        assert any(int(r["high"].max()) >> (8 * c["W"] - 1) for c, r in mine), (kind, "the sign bit")
    for kind in dp.LATER_SEGMENTED:
        mine = [c for c in cases if c["kind"] == kind]
        assert any((np.diff(c["offsets"]) == 0).any() and (np.diff(c["offsets"]) > 0).any() for c in mine), kind
        assert any(c["offsets"][0] > 0 for c in mine) and any(c["offsets"][-1] < c["n"] for c in mine), kind
        assert {c["nseg"] for c in mine} == set(dp.NSEGS), kind
        assert {c["layout"] for c in mine} == {"random", "units", "runs"}, kind
        assert any((np.diff(c["offsets"]) >= 2 * 8192 // c["W"]).any() for c in mine), (kind, "a segment of chain length")
    for at in dp.PLACEMENTS:
        assert count(lambda c: c["selected_at"] == at) >= 5 and count(lambda c: c["high_at"] == at) >= 5, at


def test_no_later_case_is_skipped(planned_later):
    cases = planned_later[0]
    assert dp.skip_reasons(cases[:DEFAULT_ITERS]) == []
    assert all(c["skip"] is None for c in cases)
    for c in cases:
        if c["form"] == "host":
            assert c["n"] <= dp.MAX_CHUNKS * max(2, c["chunk_flags"] * 2 // c["W"])
        assert not c["big_offset"] or (c["sel_bits"] == 1 and c["form"] in ("launcher", "host") and c["sel_offset"] >> 33 == 1)


def test_reference_of_the_later_plan_is_quick(planned_later):
    assert planned_later[2] < 20.0, planned_later[2]


# ------------------------------------------------------------------ what the later plan would notice: a table of wrong models
class HighOverAll(dp.Definition):
    high = lambda self, case, above, sel, counted: np.bitwise_or.reduce(above)  # noqa: E731


class HighOverCounted(dp.Definition):
    high = lambda self, case, above, sel, counted: np.bitwise_or.reduce(above[counted]) if counted.any() else np.uint64(0)  # noqa: E731


class SelectionBySegment(dp.Definition):
    def sel(self, case):
        m, o = case["mask"].copy(), case["offsets"]
        for a, b in zip(o[:-1], o[1:]):
            m[a:b] = case["mask"][:b - a]       # bit sel_offset + (j - offsets[i])
        return m


class SelectionFromItsByte(dp.Definition):
    sel = lambda self, case: np.concatenate([np.ones(case["sel_offset"] & 7, dtype=bool), case["mask"]])[:case["n"]]  # noqa: E731


class SelectionOneOn(dp.Definition):
    sel = lambda self, case: np.append(case["mask"][1:], True)[:case["n"]]  # noqa: E731


class SelectionByteAndOne(dp.Definition):
    sel = lambda self, case: case["mask"] & bool(case["sel_bits"] == 1 or (1 + case["n"] % 255) & 1)  # noqa: E731


class MapqOneOn(dp.Definition):
    mapq = lambda self, case: np.append(case["mapq"][1:], np.uint8(255))[:case["n"]]  # noqa: E731


class SelectedIsTheSelection(dp.Definition):
    selected = lambda self, sel, counted: int(sel.sum())  # noqa: E731


class SegmentOneLate(dp.Definition):
    segment = lambda self, offsets, i: (int(offsets[i]) + 1, int(offsets[i + 1]))  # noqa: E731


class AnyOfAsAllOf(dp.Definition):
    any_of = lambda self, f, include_any: (f & include_any) == include_any  # noqa: E731


class AllOfAsExclude(dp.Definition):
    all_of = lambda self, f, exclude_all: (f & exclude_all) == 0  # noqa: E731


class AnyOfLowByte(dp.Definition):
    masks = lambda self, c: (c["require"], c["exclude"], c["include_any"] & 0xFF, c["exclude_all"])  # noqa: E731


class AllOfLowByte(dp.Definition):
    masks = lambda self, c: (c["require"], c["exclude"], c["include_any"], c["exclude_all"] & 0xFF)  # noqa: E731


class UnreadColumnReported(dp.Definition):
    unread_high = lambda self, case, above: np.bitwise_or.reduce(above) if above.size else np.uint64(0)  # noqa: E731


WRONG_MODELS = (
    ("high over all elements", HighOverAll, MASKED_WIDE),
    ("high over the counted elements only", HighOverCounted, ("wide_filter_where", "wide_segments_filter_where", "wide_filter_rf")),
    ("selection read at sel_offset + (j - offsets[i])", SelectionBySegment, MASKED_SEGMENTED),
    ("selection bit (sel_offset & ~7) + j", SelectionFromItsByte, dp.MASKED),
    ("selection bit sel_offset + j + 1", SelectionOneOn, dp.MASKED),
    ("a selection byte tested as byte & 1", SelectionByteAndOne, dp.MASKED),
    ("MAPQ of element j taken from j + 1", MapqOneOn, dp.LATER_FILTERED),
    ("selected as the number of selected elements", SelectedIsTheSelection, MASKED_FILTERED),
    ("a segment starting one element late", SegmentOneLate, dp.LATER_SEGMENTED),
    ("any-of evaluated as all-of", AnyOfAsAllOf, dp.RF),
    ("all-of evaluated as an exclude", AllOfAsExclude, dp.RF),
    ("include_any & 0xFF", AnyOfLowByte, dp.RF),
    ("exclude_all & 0xFF", AllOfLowByte, dp.RF),
    ("an unsatisfiable rf predicate that still reports the column's high", UnreadColumnReported, ("wide_filter_rf",)),
)


@pytest.mark.parametrize("name,model,kinds", WRONG_MODELS, ids=[w[0] for w in WRONG_MODELS])
def test_later_plan_notices_a_wrong_model(planned_later, name, model, kinds):
    """the expected images of at least 5 cases of the default plan differ under each one-line variation of the reference"""
    cases, refs, _ = planned_later
    changed = []
    for c, r in zip(cases[:DEFAULT_ITERS], refs):
        if c["kind"] not in kinds:
            continue
        wrong = dp.expected_images(c, dp.reference(c, model()))
        if any(not np.array_equal(a, b) for a, b in zip(dp.expected_images(c, r), wrong)):
            changed.append(c["index"])
    assert len(changed) >= 5, (name, changed)


LATER_PLAN_DIGEST = "345770c44eb04cf10be5f1282b8e0bed1239f5afc9af9e036b680b17647315b5"   # taken before plan_rf_segmented was written


def test_later_plan_is_byte_for_byte_what_it_was(planned_later):
    """test_plan_is_byte_for_byte_what_it_was, of plan_later: a block size taken from the kinds has not moved one draw of it"""
    assert plan_digest(planned_later[0]) == LATER_PLAN_DIGEST


def test_later_input_images_hold_the_inputs_between_poison(planned_later):
    seen = set()
    for c in planned_later[0][:120]:
        img, at = dp.array_image(c)
        W, n = c["W"], c["n"]
        assert at % 16 == c["phase"] and img[at:at + n * W].tobytes() == c["array"].tobytes()
        assert (img[:at] == 0xFF).all() and (img[at + n * W:] == 0xFF).all() and at >= 64 * W and img.size - at - n * W >= 64 * W
        if c["mapq"] is not None:
            q, qa = dp.bytes_image(c["mapq"], c["mapq_align"])
            assert qa % 16 == c["mapq_align"] and np.array_equal(q[qa:qa + n], c["mapq"]) and (q[:qa] == 0xFF).all() and (q[qa + n:] == 0xFF).all()
        if c["mask"] is None:
            assert dp.sel_bits_of(c) is None
            continue
        seen.add((c["sel_bits"], c["mapq"] is not None))
        s, (b, ptr) = c["sel_offset"], dp.selection_image(c)
        first = ptr + (s // 8 if c["sel_bits"] == 1 else s)        # the byte that holds element 0
        packed = ptr if c["sel_bits"] == 1 and not c["big_offset"] else first     # a small bit offset lies within the packed bytes
        assert packed % 16 == c["sel_align"] and 64 <= packed and (b[:packed] == 0xFF).all()
        if c["sel_bits"] == 8:
            assert ((b[first:first + n] != 0) == c["mask"]).all() and (b[first + n:] == 0xFF).all() and b.size - first - n >= 64
            assert not (b[first:first + n] == 1).any() or n % 255 == 0
        else:
            bits = np.unpackbits(b[first:], bitorder="little")
            assert np.array_equal(bits[s & 7:(s & 7) + n].astype(bool), c["mask"]) and bits[:s & 7].all() and bits[(s & 7) + n:].all()
            assert (ptr < 0) == c["big_offset"]
    assert seen == {(1, False), (1, True), (8, False), (8, True)}     # a case with a MAPQ column and a selection has both images


# ------------------------------------------------------------------ the third plan: the segmented units of the whole predicate
# chosen on the CPU, before any GPU run, by the coverage test below alone: the share of partly taken selections is 82 to 90 % over
# the seeds 20261021 .. 20261027 (tiny arrays and single-valued columns take all or nothing), and this is the first of them to
# meet the 85 % that the other two plans meet
RF_SEGMENTED_SEED = 20261024


@pytest.fixture(scope="module")
def planned_rf_segmented(oracle_mod):
    """planned, of plan_rf_segmented(RF_SEGMENTED_SEED, 300)"""
    cases = dp.plan_rf_segmented(RF_SEGMENTED_SEED, 300)
    refs, spent = [], 0.0
    for c in cases:
        t0 = time.perf_counter()
        refs.append(dp.reference(c))
        if c["index"] < DEFAULT_ITERS:
            spent += time.perf_counter() - t0
    return cases, refs, spent


def test_rf_segmented_reference_agrees_with_the_per_kernel_oracle(planned_rf_segmented):
    cases, refs, _ = planned_rf_segmented
    assert len(cases) == 300 and {c["kind"] for c in cases} == set(dp.RF_SEGMENTED_KINDS)
    for c, r in zip(cases, refs):
        rows, sel = segments_filter_rf_oracle.want(low16(c), c["offsets"], c["require"], c["exclude"], c["include_any"], c["exclude_all"],
                                                   c["mapq"], c["min_mapq"], True)
        what = dp.describe(c)
        assert rows.shape == r["rows"].shape and np.array_equal(rows, r["rows"]), what
        assert np.array_equal(np.asarray(sel, dtype=np.uint64), r["selected"]) and not r["high"].any(), what
        if c["rf_outcome"] == "empty":
            assert not r["rows"].any() and not r["selected"].any(), what


def test_rf_segmented_plan_is_deterministic_and_prefix_closed(planned_rf_segmented):
    cases = planned_rf_segmented[0]
    for k in (0, 1, 3, 4, 5, 80):
        shorter, longer = dp.plan_rf_segmented(RF_SEGMENTED_SEED, k), dp.plan_rf_segmented(RF_SEGMENTED_SEED, k + 1)
        assert len(shorter) == k and len(longer) == k + 1
        for a, b in zip(shorter, longer):
            same_case(a, b)
        for a, b in zip(longer, cases):
            same_case(a, b)
    assert any(a["n"] != b["n"] for a, b in zip(dp.plan_rf_segmented(RF_SEGMENTED_SEED + 1, 10), cases))
    for block in range(0, 300 - 3, 4):                  # a block is the four forms
        assert sorted(c["form"] for c in cases[block:block + 4]) == sorted(dp.FORMS)


def whole_units(c, a, b):
    """whole units of the kernel that the segment [a, b) holds: units lie at multiples of UNIT_FLAGS from the 16-byte boundary in
    front of the array (a staged chunk of the host form starts on one)"""
    lo = 0 if c["form"] == "host" else c["phase"] // 2
    return max(0, (b + lo) // dp.UNIT_FLAGS - -(-(a + lo) // dp.UNIT_FLAGS))


def hazard_segment(c):
    """(a, b) of the segment that the dealt zero-fill case is about"""
    o = c["offsets"]
    return (int(o[0]), int(o[1])) if c["hazard"] == "front" else (int(o[-2]), int(o[-1]))


def test_rf_segmented_plan_covers_what_it_is_for(planned_rf_segmented):
    from libflagstats_amd import _lib
    reduce_ = _lib.lib().fsk_filter_rf_reduce
    cases, refs, _ = planned_rf_segmented
    cases, refs = cases[:DEFAULT_ITERS], refs[:DEFAULT_ITERS]
    count = lambda pred: sum(1 for c in cases if pred(c))  # noqa: E731
    truth = dp.Definition()
    for kind in dp.RF_SEGMENTED_KINDS:
        mine = [c for c in cases if c["kind"] == kind]
        # ... of an rf kind: the plan dealt what the reduction finds, every outcome in every form, a bit in the high byte plane
        assert [rf_outcome(reduce_, c) for c in mine] == [c["rf_outcome"] for c in mine], kind
        for form in dp.FORMS:
            for outcome in dp.RF_OUTCOMES:
                assert sum(1 for c in mine if c["form"] == form and c["rf_outcome"] == outcome) >= 3, (kind, form, outcome)
        assert any((c["include_any"] | c["exclude_all"]) & 0xFF00 for c in mine), kind
        # ... of a segmented kind
        assert any((np.diff(c["offsets"]) == 0).any() and (np.diff(c["offsets"]) > 0).any() for c in mine), kind
        assert any(c["offsets"][0] > 0 for c in mine) and any(c["offsets"][-1] < c["n"] for c in mine), kind
        assert {c["nseg"] for c in mine} == set(dp.NSEGS), kind
        assert {c["layout"] for c in mine} == {"random", "units", "runs"}, kind
        assert any((np.diff(c["offsets"]) >= 2 * 8192 // c["W"]).any() for c in mine), (kind, "a segment of chain length")
        assert all(c["W"] == 2 and c["mask"] is None and c["mapq"] is not None for c in mine), kind
    for mode in range(4):
        assert count(lambda c: c["mode"] == mode) >= 5, mode
    for grid in dp.GRIDS:
        assert count(lambda c: c["grid"] == grid) >= 5, grid
    for chunk in dp.CHUNKS:
        assert count(lambda c: c["chunk_flags"] == chunk) >= 5, chunk
    for mu in dp.MIN_UNITS:
        assert count(lambda c: c["policy"][0] == mu) >= 5, mu
    for nseg in dp.NSEGS:
        assert count(lambda c: c["nseg"] == nseg) >= 5, nseg
    for at in dp.PLACEMENTS:
        assert count(lambda c: c["selected_at"] == at) >= 5, at
    for name in ("int16", "uint16"):
        assert count(lambda c: c["dtype"] == name) >= 5, name
    assert count(lambda c: c["min_mapq"] > 0) >= 20 and count(lambda c: c["min_mapq"] == 0) >= 20
    assert count(lambda c: c["min_mapq"] == 0 and not c["mapq_null"]) >= 5 and count(lambda c: c["mapq_align"] & 1) >= 5
    assert {c["n_cluster"] for c in cases} == {0, 1, 2, 3} and max(c["n"] for c in cases) <= dp.CAP
    assert sum(c["n"] for c in cases) < 40_000_000
    # the dealt zero-fill cases: in every form at least twice, each with all of what makes a position outside the array pass
    dealt = [c for c in cases if c["hazard"] is not None]
    out = (ctypes.c_uint32 * 4)()
    for c in dealt:
        what = dp.describe(c)
        assert reduce_(c["require"], c["exclude"], c["include_any"], c["exclude_all"], out) == 2 and out[0] == 0 and out[2] == 0 and out[3], what
        assert c["require"] == 0 and c["include_any"] == 0 and c["min_mapq"] == 0 and c["rf_outcome"] == "all", what
        assert bool(truth.flag_pass(np.zeros(1, dtype=np.uint64), *truth.masks(c))[0]), what     # flag 0 passes
        a, b = hazard_segment(c)
        assert b > a, what
        if c["hazard"] == "front":
            assert a == 0 and c["phase"] != 0 and c["form"] != "host", what
        else:
            assert b == c["n"] and (c["phase"] // 2 + c["n"]) % 8 != 0 and c["n"] % 8 != 0, what
    per_flag = [whole_units(c, *hazard_segment(c)) < max(1, c["policy"][0]) for c in dealt]
    assert 2 * sum(per_flag) == len(dealt), per_flag
    assert any(whole_units(c, *hazard_segment(c)) >= max(1, c["policy"][0]) and c["form"] == "launcher" for c in dealt)
    for form in dp.FORMS:
        mine = [c for c in dealt if c["form"] == form]
        assert len(mine) >= 2 and {c["mapq_null"] for c in mine} == {False, True}, form
    assert {c["hazard"] for c in dealt} == {"front", "back"}
    assert any(c["form"] == "host" and c["chunk_flags"] == 8 for c in dealt)
    # a selection partly taken in some segment: all but 15 % of the cases that can pass anything (a fifth is dealt `empty`)
    can = [(c, r) for c, r in zip(cases, refs) if truth.reads(c)]
    assert len(can) == count(lambda c: c["rf_outcome"] != "empty") >= 180
    partial = [bool(((r["selected"] > 0) & (r["selected"] < r["length"])).any()) for c, r in can]
    assert sum(partial) >= 0.85 * len(can), (sum(partial), len(can))


def test_no_rf_segmented_case_is_skipped(planned_rf_segmented):
    cases = planned_rf_segmented[0]
    assert dp.skip_reasons(cases[:DEFAULT_ITERS]) == []
    assert all(c["skip"] is None for c in cases)
    for c in cases:
        if c["form"] == "host":
            assert c["n"] <= dp.MAX_CHUNKS * max(2, c["chunk_flags"])
        assert not c["big_offset"] and c["sel_offset"] == 0


def test_reference_of_the_rf_segmented_plan_is_quick(planned_rf_segmented):
    assert planned_rf_segmented[2] < 20.0, planned_rf_segmented[2]


class RfIgnoredBesideAPair(dp.Definition):
    """--rf / -G dropped where the reduction leaves a plain pair: the parent's kernel called with the caller's pair, not the
    reduced one"""
    def masks(self, c):
        return (c["require"], c["exclude"]) + ((0, 0) if c["rf_outcome"] == "pair" else (c["include_any"], c["exclude_all"]))


class ValidBitsDropped(dp.Definition):
    """the per-flag count without its valid-bits mask: a non-empty segment also counts the positions of its first and last vector
    of 8 flags that lie outside it.  Vectors are aligned to 16 bytes in memory: element index = -phase / 2 modulo 8.  A position
    inside [0, n) carries its own flag and MAPQ; one outside carries flag 0 and MAPQ 0."""
    inside, outside = True, True

    def stray(self, case, ok, a, b):
        lo, n = case["phase"] // case["W"], case["n"]
        first, last = (a + lo) // 8 * 8 - lo, (b - 1 + lo) // 8 * 8 - lo           # element index of position 0 of either vector
        j = np.array([k for k in sorted(set(range(first, first + 8)) | set(range(last, last + 8))) if not a <= k < b], dtype=np.int64)
        real = (j >= 0) & (j < n)
        zero_passes = bool(self.flag_pass(np.zeros(1, dtype=np.uint64), *self.masks(case))[0]) and case["min_mapq"] == 0
        kept = j[real][ok[j[real]]] if self.inside else j[:0]
        flags = (case["array"].view(dp.UNSIGNED[case["W"]])[kept] & dp.UNSIGNED[case["W"]](0xFFFF)).astype(np.uint16)
        zeros = int((~real).sum()) if self.outside and zero_passes else 0
        return np.concatenate([flags, np.zeros(zeros, dtype=np.uint16)])


class ValidBitsDroppedOutsideTheArray(ValidBitsDropped):
    """... of the positions outside [0, n) alone: what no neighbouring element shows"""
    inside = False


RF_SEGMENTED_WRONG_MODELS = (
    ("any-of evaluated as all-of", AnyOfAsAllOf),
    ("all-of evaluated as an exclude", AllOfAsExclude),
    ("include_any & 0xFF", AnyOfLowByte),
    ("exclude_all & 0xFF", AllOfLowByte),
    ("MAPQ of element j taken from j + 1", MapqOneOn),
    ("a segment starting one element late", SegmentOneLate),
    ("--rf / -G ignored where the reduction leaves a pair", RfIgnoredBesideAPair),
    ("the per-flag count without its valid-bits mask", ValidBitsDropped),
)


def changed_by(cases, refs, model):
    """indices of the cases whose expected images differ under the model"""
    changed = []
    for c, r in zip(cases, refs):
        wrong = dp.expected_images(c, dp.reference(c, model()))
        if any(not np.array_equal(a, b) for a, b in zip(dp.expected_images(c, r), wrong)):
            changed.append(c["index"])
    return changed


@pytest.mark.parametrize("name,model", RF_SEGMENTED_WRONG_MODELS, ids=[w[0] for w in RF_SEGMENTED_WRONG_MODELS])
def test_rf_segmented_plan_notices_a_wrong_model(planned_rf_segmented, name, model):
    """the expected images of at least 5 cases of the default plan differ under each one-line variation of the reference"""
    cases, refs, _ = planned_rf_segmented
    changed = changed_by(cases[:DEFAULT_ITERS], refs, model)
    assert len(changed) >= 5, (name, changed)


def test_rf_segmented_plan_notices_a_zero_filled_position_that_counts(planned_rf_segmented):
    """the valid-bits mask dropped for the positions outside [0, n) alone: only the dealt cases can tell, and at least 5 do"""
    cases, refs, _ = planned_rf_segmented
    cases = cases[:DEFAULT_ITERS]
    changed = changed_by(cases, refs, ValidBitsDroppedOutsideTheArray)
    assert len(changed) >= 5, changed
    assert all(cases[i]["hazard"] is not None for i in changed), changed
    for form in dp.FORMS:
        assert any(cases[i]["form"] == form for i in changed), (form, changed)
