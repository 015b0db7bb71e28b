"""CPU: the case plan and the reference of the randomized sweep over the derived kernels (tests/derived_plan.py) -- the reference
against the per-kernel oracles, the plan's determinism, what the default plan covers, and that it skips nothing.  No GPU."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import derived_plan as dp  # noqa: E402
import filter_oracle  # noqa: E402
import segments_filter_oracle  # noqa: E402
import segments_oracle  # noqa: E402
import segments_wide_filter_oracle  # noqa: E402
import segments_wide_oracle  # noqa: E402
import where_oracle  # noqa: E402
import wide_filter_oracle  # noqa: E402

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
