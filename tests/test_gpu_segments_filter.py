"""The filtered segmented flagstat on the MI355X: fsk::flagstat_segments_filter with and without a MAPQ column, the three C entries
and libflagstats_amd/segments_filter.py.  Every comparison is exact.

Expected rows never come from the code under test: segments_filter_oracle.want is segments_oracle.segmented_counters of the array
with the failing flags zeroed (filter_oracle.filter_mask), slot 9 from the definition; the expected `selected` is the per-segment
sum of the mask.  Large inputs are periodic (one prime period for flags and MAPQ) and use the oracle's periodic form.  Layouts
are placed with segments_oracle.WriterSplit, the launcher's work split mirrored, and checked to contain the runs they are for."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_filter_oracle as sfo  # noqa: E402
from filter_oracle import filter_mask  # noqa: E402
from segments_oracle import SEG_EPOCH, SEG_UNIT, segmented_counters, writer_ranges  # noqa: E402

pytestmark = pytest.mark.gpu

U = SEG_UNIT
P = 65_521                                    # prime: no unit, row or writer seam is a multiple of the period
STORE, SUPERSET = 1, 2
MODES = (1, 0, 3, 2)                          # store, +=, store + superset, += + superset
GARBAGE, BIAS, SEL_BIAS = 0x5EED_0000_0BAD, 3, 1_000_003
BYTE_ALIGNMENTS = (0, 1, 3, 8, 15)
EVERY_MIN_UNITS = (0, 1, 2, 3, 255, 256, 0xFFFFFFFF)   # tests/test_gpu_segments_regimes.py's list
SINGLE_BITS = tuple(1 << b for b in range(16))
PREDICATES = ([(bit, 0) for bit in SINGLE_BITS] + [(0, bit) for bit in SINGLE_BITS]
              + [(0, 0x904), (0x2, 0x900), (0x1, 0xF04), (0x0101, 0x8080), (0xFFFF, 0), (0, 0xFFFF), (0x0040, 0x0040), (0, 0)])


def dev16(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint16).view(np.int16)).cuda()


def dev8(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint8)).cuda()


def dev64(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.int64)).cuda()


def err(hip):
    return hip.FLAGSTATS_hip_last_error().decode(errors="replace")


def expect(want_sup, want_sel, mode):
    """what a launch in `mode` must leave in rows prefilled with GARBAGE (store) or BIAS (+=) and counts prefilled with GARBAGE
    or SEL_BIAS"""
    w = want_sup.copy()
    if not mode & SUPERSET:
        w[:, [0, 9, 16]] = 0
    if mode & STORE:
        return w, want_sel.copy()
    return w + np.uint64(BIAS), want_sel + np.uint64(SEL_BIAS)


class Batch:
    """device words for many launches -- per launch nseg rows of 32, then nseg counts -- prefilled in one copy and read back in
    one copy after every launch has been queued"""

    def __init__(self):
        self.items, self.words, self.t = [], 0, None

    def add(self, mode, want_sup, want_sel, note, with_selected=True):
        nseg = want_sup.shape[0]
        self.items.append((self.words, nseg, mode, want_sup, want_sel, note, with_selected))
        self.words += nseg * 33
        return len(self.items) - 1

    def upload(self):
        import torch
        host = np.empty(max(self.words, 1), dtype=np.uint64)
        for at, nseg, mode, _, _, _, _ in self.items:
            host[at:at + nseg * 32] = GARBAGE if mode & STORE else BIAS
            host[at + nseg * 32:at + nseg * 33] = GARBAGE if mode & STORE else SEL_BIAS
        self.host = host
        self.t = torch.from_numpy(host.view(np.int64)).cuda()
        torch.cuda.synchronize()

    def out(self, k):
        return self.t.data_ptr() + 8 * self.items[k][0]

    def selected(self, k):
        at, nseg = self.items[k][:2]
        return self.t.data_ptr() + 8 * (at + nseg * 32) if self.items[k][6] else None

    def check(self):
        import torch
        torch.cuda.synchronize()
        got = self.t.cpu().numpy().view(np.uint64)
        for at, nseg, mode, want_sup, want_sel, note, with_selected in self.items:
            rows, sel = expect(want_sup, want_sel, mode)
            g = got[at:at + nseg * 32].reshape(nseg, 32)
            bad = np.nonzero((g != rows).any(axis=1))[0]
            assert bad.size == 0, (note, "mode", mode, "rows", bad[:8], g[bad[:2]], rows[bad[:2]])
            gs = got[at + nseg * 32:at + nseg * 33]
            if not with_selected:
                sel = self.host[at + nseg * 32:at + nseg * 33]      # NULL d_selected: the words behind the rows stay
            bad = np.nonzero(gs != sel)[0]
            assert bad.size == 0, (note, "mode", mode, "selected", bad[:8], gs[bad[:8]], sel[bad[:8]])


def get_policy(hip):
    mu, bpc = ctypes.c_uint32(), ctypes.c_uint32()
    hip.fsk_segments_policy(ctypes.byref(mu), ctypes.byref(bpc))
    return mu.value, bpc.value


@pytest.fixture(scope="module")
def launcher(hip):
    hip.fsk_segments_policy.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    hip.fsk_segments_policy.restype = None
    hip.fsk_set_segments_policy.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    hip.fsk_set_segments_policy.restype = None
    return hip.fsk_launch_segments_filter


@contextlib.contextmanager
def policy(hip, min_units, blocks_per_cu=1):
    saved = get_policy(hip)
    try:
        hip.fsk_set_segments_policy(min_units, blocks_per_cu)
        yield
    finally:
        hip.fsk_set_segments_policy(*saved)
    assert get_policy(hip) == saved


def coprime_offsets(n, start=0, lengths=(7, 11, 13, 0, 4099, 1, 509, 8191, 17, 0, 0, 3, 1021, 64, 4096, 19)):
    """segments of lengths without a common factor with the vector, the row or the unit (and some empty ones), end to end"""
    o = [start]
    i = 0
    while o[-1] < n:
        o.append(min(o[-1] + lengths[i % len(lengths)], n))
        i += 1
    return np.array(o, dtype=np.int64)


# ------------------------------------------------------------------ 1. every value under every kind of predicate
def test_every_value_under_every_kind_of_predicate(hip, launcher):
    """0..65535 once each, shuffled (16 units), cut into segments of coprime lengths, under every single required bit, every
    single excluded bit, the samtools filters, predicates on both byte planes, everything required, everything excluded, an
    overlapping pair and the empty predicate -- store + superset form and += form, through the device entry, the _sync form and
    the host form, and through the Python layer"""
    import torch
    from libflagstats_amd import segments_filter as sf
    n = 65536
    values = np.random.RandomState(2026).permutation(n).astype(np.uint16)
    o = coprime_offsets(n - 5, start=2)
    nseg = o.size - 1
    t, d_off = dev16(values), dev64(o)
    wants = {p: sfo.want(values, o, p[0], p[1], superset=True) for p in PREDICATES}
    inside = values[o[0]:o[-1]]
    assert int(wants[0, 0xFFFF][1].sum()) == int((inside == 0).sum()) <= 1 and not wants[0, 0xFFFF][0][:, 10:].any()
    assert int(wants[0xFFFF, 0][1].sum()) == int((inside == 0xFFFF).sum()) <= 1
    assert not wants[0x0040, 0x0040][1].any() and not wants[0x0040, 0x0040][0].any()
    assert np.array_equal(wants[0, 0][1], np.diff(o).astype(np.uint64))
    batch = Batch()
    plan = [(p, mode, batch.add(mode, wants[p][0], wants[p][1], ("device", p, mode))) for p in PREDICATES for mode in (STORE | SUPERSET, 0)]
    batch.upload()
    for (require, exclude), mode, k in plan:
        rc = hip.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), n, d_off.data_ptr(), nseg, require, exclude, None, 0,
                                                          batch.out(k), batch.selected(k), mode, None)
        assert rc == 0, (require, exclude, mode, err(hip))
    batch.check()
    for name, entry, src in (("sync", hip.FLAGSTATS_hip_device_u16_segments_filter_sync, t.data_ptr()),
                             ("host", hip.FLAGSTATS_hip_u16_x64_segments_filter, values.ctypes.data)):
        for p in PREDICATES:
            for mode in (STORE | SUPERSET, 0):
                rows = np.full((nseg, 32), GARBAGE if mode & STORE else BIAS, dtype=np.uint64)
                sel = np.full(nseg, GARBAGE if mode & STORE else SEL_BIAS, dtype=np.uint64)
                rc = entry(src, n, o.ctypes.data, nseg, p[0], p[1], None, 0, rows.ctypes.data, sel.ctypes.data, mode)
                assert rc == 0, (name, p, mode, err(hip))
                want_rows, want_sel = expect(wants[p][0], wants[p][1], mode)
                assert np.array_equal(rows, want_rows) and np.array_equal(sel, want_sel), (name, p, mode)
    # the Python layer under samtools' usual filter
    want_rows, want_sel = sfo.want(values, o, 0x2, 0x904)
    for got_rows, got_sel in (sf.flagstats_segments_filter(values, o, require=0x2, exclude=0x904),
                              sf.count_segments_device_ptr_filter(t.data_ptr(), n, o, require=0x2, exclude=0x904)):
        assert got_rows.dtype == np.uint64 and got_sel.dtype == np.uint64
        assert np.array_equal(got_rows, want_rows) and np.array_equal(got_sel, want_sel)
    rows_t, sel_t = sf.count_segments_torch_filter(t, d_off, require=0x2, exclude=0x904)
    torch.cuda.synchronize()
    assert rows_t.dtype == torch.int64 and tuple(rows_t.shape) == (nseg, 32) and tuple(sel_t.shape) == (nseg,) and rows_t.device == t.device
    assert np.array_equal(rows_t.cpu().numpy().view(np.uint64), want_rows) and np.array_equal(sel_t.cpu().numpy().view(np.uint64), want_sel)
    dicts = sf.segment_filter_dicts(got_rows, got_sel)
    assert [d["n_values"] for d in dicts] == [int(x) for x in want_sel]
    i = int(np.argmax(want_sel))
    assert int(dicts[i]["passed"]["mapped"]) == int(want_sel[i]) - int(want_rows[i, 2]) - int(want_rows[i, 18])


# ------------------------------------------------------------------ 2. geometry
LENGTHS = (1, 7, 8, 9, 511, 513, U - 1, U, U + 1, 2 * U + 1, 5 * U - 1, 9 * U + 5)
PRED_NO_REQUIRE, PRED_BOTH_PLANES = (0, 0x0904), (0x0041, 0x0900)


def geometry_offsets(w, n, variant):
    """boundaries at a flag inside a vector, at a 512-flag row, at a unit seam +-1 and at every writer seam +-1 (all as grid
    positions, i.e. shifted by the array's phase), with empty segments; variant 0 covers [0, n), variant 1 leaves a gap in front
    and behind, variant 2 starts inside the first vector and ends at n"""
    cuts = {3, 512 - w.lo0, 1024 - w.lo0 + 5, U - w.lo0 - 1, U - w.lo0, U - w.lo0 + 1, 2 * U - w.lo0, 3 * U - w.lo0 - 1}
    for k, s in enumerate(w.seams()):
        cuts.add(int(s) + (-1, 0, 1)[k % 3])
    cuts = sorted(c for c in cuts if 0 < c < n)
    first, last = ((0, n), (min(5, n - 1), max(n - 9, min(5, n - 1))), (min(2, n - 1), n))[variant]
    inner = [c for c in cuts if first < c < last]
    o = [first] + inner[:2] + inner[1:2] * 2 + inner[2:] + [last, last]     # a doubled boundary: empty segments
    return np.array(o, dtype=np.int64)


def test_geometry_direct_launches(hip, launcher):
    """fsk_launch_segments_filter on grids 1, 2, 3: array phases 0-7, MAPQ byte alignments 0, 1, 3, 8, 15 (and no column), lengths
    from one flag to nine units, boundaries inside a vector, at a row, at unit and writer seams +-1, empty segments, gaps in
    front of and behind the segments.  One predicate has no `require` bits: the flags around the array pass it (0xFFFF & ~exclude,
    MAPQ 0xFF), as would the zero-filled positions of a partial first or last unit, so `selected` shows any position counted
    outside its segment.  Also one chunk of a longer array (base != 0): segments before and behind it clamp to empty."""
    rng = np.random.RandomState(47)
    nmax = LENGTHS[-1]
    body = rng.randint(0, 65536, nmax).astype(np.uint16)
    forced = rng.randint(0, 100, nmax) < 55       # these pass both predicates
    body[forced] = (body[forced] & np.uint16(~0x0904 & 0xFFFF)) | np.uint16(0x0041)
    mapq = rng.randint(15, 60, nmax).astype(np.uint8)   # two thirds reach 30
    slabs, at = [], {}
    pos = 0
    for n in LENGTHS:
        for phase in range(8):
            region = np.full((64 + 8 + n + 64 + 7) // 8 * 8, 0xFFFF & ~0x0904, dtype=np.uint16)
            region[64 + phase:64 + phase + n] = body[:n]
            at[n, phase] = pos + 64 + phase
            slabs.append(region)
            pos += region.size
    cols, q_at = [], {}
    pos = 0
    for n in LENGTHS:
        for align in BYTE_ALIGNMENTS:
            region = np.full((16 + 16 + n + 16 + 15) // 16 * 16, 0xFF, dtype=np.uint8)
            region[16 + align:16 + align + n] = mapq[:n]
            q_at[n, align] = pos + 16 + align
            cols.append(region)
            pos += region.size
    d_arrays, d_cols = dev16(np.concatenate(slabs)), dev8(np.concatenate(cols))
    assert d_arrays.data_ptr() % 16 == 0 and d_cols.data_ptr() % 16 == 0
    batch, calls, offs = Batch(), [], []
    i = 0
    seen = set()
    for n in LENGTHS:
        for phase in range(8):
            ptr = d_arrays.data_ptr() + 2 * at[n, phase]
            assert ptr % 16 == 2 * phase
            for grid in (1, 2, 3):
                w = writer_ranges(ptr % 16, n, grid)
                for p in (PRED_NO_REQUIRE, PRED_BOTH_PLANES):
                    align = (None,) + BYTE_ALIGNMENTS
                    align = align[(i + phase) % 6]
                    mode = MODES[i % 4]
                    o = geometry_offsets(w, n, i % 3)
                    i += 1
                    seen.add((phase, align))
                    mn = 0 if align is None else 30
                    qptr = None if align is None else d_cols.data_ptr() + q_at[n, align]
                    want_rows, want_sel = sfo.want(body[:n], o, p[0], p[1], mapq[:n], mn, superset=True)
                    k = batch.add(mode, want_rows, want_sel, (n, phase, grid, p, align, mode, o.tolist()))
                    offs.append(o)
                    calls.append((k, ptr, qptr, 0, n, len(offs) - 1, p, mn, mode, grid))
    assert len({a for _, a in seen}) == 6 and len({ph for ph, _ in seen}) == 8 and len(seen) >= 40
    # one chunk [c0, c0 + m) of the longest array, global offsets over the whole of it
    n = LENGTHS[-1]
    o_all = np.array([0, 3, U + 1, 2 * U, 2 * U, 4 * U - 3, 6 * U + 9, 8 * U, n - 2], dtype=np.int64)
    for phase, c0, m in ((0, U + 3, 3 * U), (3, 2 * U - 5, 4 * U + 11), (6, 7, U)):
        for align in (None, 3):
            mn = 0 if align is None else 30
            clipped = np.clip(o_all, c0, c0 + m)
            want_rows, want_sel = sfo.want(body[:n], clipped, 0, 0x0904, mapq[:n], mn, superset=True)
            assert (o_all < c0).any() and (o_all > c0 + m).any() and want_sel.any() and not want_sel.all()
            ptr = d_arrays.data_ptr() + 2 * (at[n, phase] + c0)
            qptr = None if align is None else d_cols.data_ptr() + q_at[n, align] + c0
            for mode in (3, 0):
                k = batch.add(mode, want_rows, want_sel, ("chunk", phase, c0, m, align, mode))
                offs.append(o_all)
                calls.append((k, ptr, qptr, c0, m, len(offs) - 1, (0, 0x0904), mn, mode, 2))
    lens = np.array([0] + [x.size for x in offs], dtype=np.int64)
    starts = np.cumsum(lens)
    d_off = dev64(np.concatenate(offs))
    batch.upload()
    for k, ptr, qptr, base, m, oi, p, mn, mode, grid in calls:
        rc = launcher(ptr, qptr, base, m, d_off.data_ptr() + 8 * int(starts[oi]), offs[oi].size - 1, p[0], p[1], mn, batch.out(k),
                      batch.selected(k), mode, grid, None)
        assert rc == 0, (batch.items[k][5], rc)
    batch.check()


# ------------------------------------------------------------------ 3. which MAPQ byte belongs to which flag
@pytest.mark.parametrize("phase,align", [(0, 0), (5, 3)])
def test_which_mapq_byte_belongs_to_which_flag(hip, launcher, phase, align):
    """16 units at grid 1 (four units per writer); every flag passes the FLAG test and the values differ from their neighbours
    (read1 / read2 / neither in turn).  MAPQ 60 at one position p and 0 elsewhere: `selected` is 1 in p's segment and 0 in the
    others, and the row is that of array[p] alone; then 0 at p and 60 elsewhere.  p sweeps lanes, rows and units of a per-flag
    unit, of a chain run, and of the joints between them."""
    import torch
    n = 16 * U
    require, exclude = 0x0001, 0x0900
    values = np.array([0x0041, 0x0081, 0x0001], dtype=np.uint16)[np.arange(n) % 3]
    slab = torch.full((64 + 8 + n + 64,), 0x00C1, dtype=torch.int16, device="cuda")
    slab[64 + phase:64 + phase + n] = dev16(values)
    arr = slab[64 + phase:64 + phase + n]
    assert arr.data_ptr() % 16 == 2 * phase
    col = torch.full((16 + 16 + n + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    q = col[16 + align:16 + align + n]
    assert q.data_ptr() % 16 == align
    w = writer_ranges(arr.data_ptr() % 16, n, 1)
    g = lambda k: k * U - w.lo0                                  # array index of unit boundary k  # noqa: E731
    # per-flag pieces in units 0 and 1, a chain of units 5-7 with a ragged head in unit 4 and a tail in unit 8 (writers 1, 2),
    # a one-unit segment (per-flag: below min_units), a chain across the seam of writers 2 | 3
    o = np.array([0, 100, g(1) + 9, g(2) - 1, g(4) + 300, g(8) + 5, g(9) + 5, g(10), g(15) - 3, n], dtype=np.int64)
    pieces = w.pieces(o)
    assert {2, 3}.issubset(set(pieces["chain"].tolist())) and (pieces["chain"] == 0).any() and (pieces["head"] > 0).any()
    positions = sorted({min(max(g(k) + d, 0), n - 1) for k in (0, 1, 4, 5, 6, 8, 9, 10, 12, 15)
                        for d in (-1, 0, 1, 7, 8, 9, 299, 300, 511, 512, 513, 2048 + 77, U - 9)} | {0, n - 1})
    d_off = dev64(o)
    nseg = o.size - 1
    batch, plan = Batch(), []
    mq = np.zeros(n, dtype=np.uint8)
    for p in positions:
        mq[:] = 0
        mq[p] = 60
        alone = sfo.want(values, o, require, exclude, mq, 30, superset=True)
        assert int(alone[1].sum()) == 1
        rest = sfo.want(values, o, require, exclude, 60 - mq, 30, superset=True)
        assert int(rest[1].sum()) == n - 1
        plan.append((p, batch.add(STORE | SUPERSET, alone[0], alone[1], ("alone", phase, align, p)),
                     batch.add(SUPERSET, rest[0], rest[1], ("all but", phase, align, p))))
    batch.upload()
    for p, k_alone, k_rest in plan:
        for k, everywhere, at_p in ((k_alone, 0, 60), (k_rest, 60, 0)):
            q.fill_(everywhere)
            q[p] = at_p
            rc = launcher(arr.data_ptr(), q.data_ptr(), 0, n, d_off.data_ptr(), nseg, require, exclude, 30, batch.out(k),
                          batch.selected(k), batch.items[k][2], 1, None)
            assert rc == 0, rc
    batch.check()


# ------------------------------------------------------------------ 4. chain and epochs
def periodic_tensors(pattern, mq_pattern, n):
    import torch
    reps = -(-(n + 16) // pattern.size)
    t = torch.from_numpy(pattern.view(np.int16)).cuda().repeat(reps)
    q = torch.from_numpy(mq_pattern).cuda().repeat(reps)
    torch.cuda.synchronize()
    return t, q


def epochs_layout(w, n):
    """chain runs of 2 and 511 units (writer 0), 254 and 255 (writer 1), 256 (writer 2), and a segment across the seam of writers
    2 | 3 whose two pieces run 100 and 300 units; every run with a ragged head and tail"""
    g = lambda wr, k: int(-(-(w.begin[wr] + w.lo0) // U) * U - w.lo0) + k * U   # unit boundary k of writer wr  # noqa: E731
    o = [3, g(0, 1) - 5, g(0, 3) + 9, g(0, 5) - 1, g(0, 5 + 511) + 8,
         g(1, 1) - 7, g(1, 255) + 1, g(1, 511) + 3,
         g(2, 1) - 8, g(2, 257) + 8, g(3, 0) - 100 * U - 3, g(3, 300) + 5, n - 1]
    o = np.array(o, dtype=np.int64)
    assert (np.diff(o) >= 0).all() and o[-1] <= n
    return o


N_EPOCHS = 2100 * U + 77          # grid 1: four writers of 525 units each (a run of 511 units needs one writer to hold it)


@pytest.mark.parametrize("min_mapq", [0, 30])
def test_chain_and_epochs(hip, launcher, min_mapq):
    """grid 1 over 2100 units (17 MB of flags) of periodic input: chain runs of 2, 254, 255, 256 and 511 whole units -- below, at
    and past the epoch of 255, and two epochs and one unit -- with ragged heads and tails, rows stored plainly and rows added by
    two writers; all four modes over garbage / bias in rows and counts"""
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
    want_rows, want_sel = sfo.periodic_want(pattern, o, 0x0001, 0x0804, mq_pattern, min_mapq, superset=True, phase=3)
    assert (want_sel[np.diff(o) > 0] > 0).all() and (want_sel < np.diff(o).astype(np.uint64)).any()
    d_off = dev64(o)
    batch = Batch()
    ks = [batch.add(mode, want_rows, want_sel, (min_mapq, mode)) for mode in MODES]
    batch.upload()
    for k in ks:
        rc = launcher(ptr, qptr if min_mapq else None, 0, n, d_off.data_ptr(), o.size - 1, 0x0001, 0x0804, min_mapq, batch.out(k),
                      batch.selected(k), batch.items[k][2], 1, None)
        assert rc == 0, rc
    batch.check()
    del t, q


def test_every_min_units_through_the_public_entries(hip, launcher):
    """the segments policy's chain threshold 0, 1, 2, 3, 255, 256 and 0xFFFFFFFF (per flag everywhere) under the device entry, the
    _sync form and the host form: the same rows and counts under every one"""
    import torch
    from libflagstats_amd import segments_filter as sf
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
    for i, mu in enumerate(EVERY_MIN_UNITS):
        sup = bool(i % 2)
        mn = 30 if i % 3 else 0
        want_rows, want_sel = sfo.periodic_want(pattern, o, 0x0001, 0x0804, mq_pattern, mn, superset=sup)
        chain = writer_ranges(t.data_ptr() % 16, n, cus).pieces(o, mu)["chain"]
        assert (chain.max() > 0) == (mu <= 3), (mu, chain.max())
        with policy(hip, mu):
            for store in (True, False):
                rows = torch.full((o.size - 1, 32), GARBAGE if store else BIAS, dtype=torch.int64, device="cuda")
                sel = torch.full((o.size - 1,), GARBAGE if store else SEL_BIAS, dtype=torch.int64, device="cuda")
                sf.count_segments_torch_filter(t, d_off, require=0x0001, exclude=0x0804, mapq=q if mn else None, min_mapq=mn, out=rows,
                                               selected=sel, store=store, superset=sup)
                torch.cuda.synchronize()
                w_rows, w_sel = expect(want_rows, want_sel, (STORE if store else 0) | SUPERSET)   # (want_rows has no superset slots unless sup)
                assert np.array_equal(rows.cpu().numpy().view(np.uint64), w_rows), ("device", mu, store)
                assert np.array_equal(sel.cpu().numpy().view(np.uint64), w_sel), ("device", mu, store)
            got = sf.count_segments_device_ptr_filter(t.data_ptr(), n, o, 0x0001, 0x0804, q.data_ptr() if mn else 0, mn, superset=sup)
            assert np.array_equal(got[0], want_rows) and np.array_equal(got[1], want_sel), ("sync", mu)
            got = sf.flagstats_segments_filter(x, o, 0x0001, 0x0804, xq if mn else None, mn, superset=sup)
            assert np.array_equal(got[0], want_rows) and np.array_equal(got[1], want_sel), ("host", mu)


# ------------------------------------------------------------------ 5. every MAPQ value against the thresholds
THRESHOLDS = (1, 30, 127, 128, 129, 255)


def test_every_mapq_value_against_the_thresholds(hip, launcher):
    """all 256 MAPQ values in a per-flag piece, in a chain run and in a ragged last unit, against thresholds on both sides of every
    carry the byte-wise compare could get wrong; array one flag into a 16-byte line, column at alignment 5"""
    import torch
    n = 7 * U + 100
    rng = np.random.RandomState(31)
    values = rng.randint(0, 65536, n).astype(np.uint16)
    mapq = rng.randint(0, 256, n).astype(np.uint8)
    mapq[:512] = np.tile(np.arange(256, dtype=np.uint8), 2)
    mapq[-256:] = np.arange(256, dtype=np.uint8)
    slab = torch.full((8 + n + 8,), -1, dtype=torch.int16, device="cuda")
    slab[1:1 + n] = dev16(values)
    ptr = slab.data_ptr() + 2
    col = torch.full((16 + n + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    col[16 + 5:16 + 5 + n] = dev8(mapq)
    qptr = col.data_ptr() + 16 + 5
    assert ptr % 16 == 2 and qptr % 16 == 5
    w = writer_ranges(ptr % 16, n, 1)
    o = np.array([0, 600, 2 * U - 1 + 5, 6 * U, n - 256, n], dtype=np.int64)
    pieces = w.pieces(o)
    for k in np.nonzero(pieces["chain"] > 0)[0]:                 # every chain run sees every MAPQ value
        b = int(pieces["b"][k] + pieces["head"][k])
        assert set(mapq[b:b + int(pieces["chain"][k]) * U].tolist()) == set(range(256))
    assert (pieces["chain"] > 0).any() and set(mapq[:600].tolist()) == set(range(256))
    d_off = dev64(o)
    batch, calls = Batch(), []
    for require, exclude in ((0, 0), (0, 0x904)):
        for mn in THRESHOLDS:
            want_rows, want_sel = sfo.want(values, o, require, exclude, mapq, mn, superset=True)
            assert int(want_sel.sum()) == int((filter_mask(values, require, exclude) & (mapq.astype(np.int64) >= mn)).sum())
            for mode in (STORE | SUPERSET, 0):
                for grid in (1, None):
                    calls.append((batch.add(mode, want_rows, want_sel, (require, exclude, mn, mode, grid)), require, exclude, mn, mode, grid))
    batch.upload()
    for k, require, exclude, mn, mode, grid in calls:
        if grid is None:
            rc = hip.FLAGSTATS_hip_device_u16_segments_filter(ptr, n, d_off.data_ptr(), o.size - 1, require, exclude, qptr, mn, batch.out(k),
                                                              batch.selected(k), mode, None)
            assert rc == 0, err(hip)
        else:
            assert launcher(ptr, qptr, 0, n, d_off.data_ptr(), o.size - 1, require, exclude, mn, batch.out(k), batch.selected(k), mode, grid, None) == 0
    batch.check()


# ------------------------------------------------------------------ 6. equivalences
def test_equivalences(hip, launcher):
    """the empty predicate is FLAGSTATS_hip_device_u16_segments with the clamped lengths as `selected` (device offsets that run
    past the array are clamped); one segment [0, n) is FLAGSTATS_hip_device_u16_filter; a NULL d_selected is legal; an
    overlapping pair launches nothing and the store form zeroes"""
    import torch
    n = 5 * U + 77
    rng = np.random.RandomState(53)
    values = rng.randint(0, 65536, n).astype(np.uint16)
    mapq = rng.randint(0, 60, n).astype(np.uint8)
    t, q = dev16(values), dev8(mapq)
    o = np.array([5, 5, 300, U + 1, 4 * U, n + 1000, n + 5000], dtype=np.int64)     # the last two run past the array
    d_off = dev64(o)
    nseg = o.size - 1
    for mode in MODES:
        plain = torch.full((nseg, 32), BIAS, dtype=torch.int64, device="cuda")
        rows = torch.full((nseg, 32), BIAS, dtype=torch.int64, device="cuda")
        sel = torch.full((nseg,), SEL_BIAS, dtype=torch.int64, device="cuda")
        assert hip.FLAGSTATS_hip_device_u16_segments(t.data_ptr(), n, d_off.data_ptr(), nseg, plain.data_ptr(), mode, None) == 0, err(hip)
        rc = hip.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), n, d_off.data_ptr(), nseg, 0, 0, None, 0, rows.data_ptr(),
                                                          sel.data_ptr(), mode, None)
        assert rc == 0, err(hip)
        torch.cuda.synchronize()
        assert torch.equal(rows, plain), mode
        lengths = np.diff(np.clip(o, 0, n)).astype(np.uint64)
        assert np.array_equal(sel.cpu().numpy().view(np.uint64), lengths + np.uint64(0 if mode & 1 else SEL_BIAS)), mode
    # the plain rows themselves against the oracle (both kernels could be wrong alike)
    assert np.array_equal(plain.cpu().numpy().view(np.uint64)[:, 2], segmented_counters(values, np.clip(o, 0, n))[:, 2] + np.uint64(BIAS))
    # one segment [0, n) is the filter entry
    whole = dev64(np.array([0, n]))
    for require, exclude, mn in ((0, 0x904, 0), (0x2, 0x900, 30)):
        for mode in (STORE | SUPERSET, 0):
            a = torch.full((33,), BIAS, dtype=torch.int64, device="cuda")
            b = torch.full((33,), BIAS, dtype=torch.int64, device="cuda")
            assert hip.FLAGSTATS_hip_device_u16_filter(t.data_ptr(), n, require, exclude, q.data_ptr(), mn, a.data_ptr(), a.data_ptr() + 256,
                                                       mode, None) == 0, err(hip)
            assert hip.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), n, whole.data_ptr(), 1, require, exclude, q.data_ptr(), mn,
                                                                b.data_ptr(), b.data_ptr() + 256, mode, None) == 0, err(hip)
            torch.cuda.synchronize()
            assert torch.equal(a, b) and int(b[32]) not in (0, BIAS), (require, exclude, mn, mode)
    # NULL d_selected; an overlapping pair
    o2 = np.array([0, 100, 2 * U + 3, n], dtype=np.int64)
    d_off2 = dev64(o2)
    want_rows, want_sel = sfo.want(values, o2, 0, 0x904, mapq, 30, superset=True)
    nothing = (np.zeros((3, 32), dtype=np.uint64), np.zeros(3, dtype=np.uint64))
    batch = Batch()
    null_sel = [batch.add(mode, want_rows, want_sel, ("NULL d_selected", mode), with_selected=False) for mode in MODES]
    overlap = [batch.add(mode, *nothing, ("overlapping pair", mode)) for mode in MODES]
    batch.upload()
    for k in null_sel:
        for call in ("launcher", "entry"):
            if call == "entry" and batch.items[k][2] & STORE == 0:
                continue                                                        # (+= twice would add twice)
            if call == "launcher":
                rc = launcher(t.data_ptr(), q.data_ptr(), 0, n, d_off2.data_ptr(), 3, 0, 0x904, 30, batch.out(k), None, batch.items[k][2], 2, None)
            else:
                rc = hip.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), n, d_off2.data_ptr(), 3, 0, 0x904, q.data_ptr(), 30, batch.out(k),
                                                                  None, batch.items[k][2], None)
            assert rc == 0, (call, err(hip))
    for k in overlap:
        rc = hip.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), n, d_off2.data_ptr(), 3, 0x0044, 0x0140, q.data_ptr(), 30, batch.out(k),
                                                          batch.selected(k), batch.items[k][2], None)
        assert rc == 0, err(hip)
    batch.check()
    for entry, src, qsrc in ((hip.FLAGSTATS_hip_device_u16_segments_filter_sync, t.data_ptr(), q.data_ptr()),
                             (hip.FLAGSTATS_hip_u16_x64_segments_filter, values.ctypes.data, mapq.ctypes.data)):
        for mode in MODES:
            rows = np.full((3, 32), GARBAGE if mode & 1 else BIAS, dtype=np.uint64)
            sel = np.full(3, GARBAGE if mode & 1 else SEL_BIAS, dtype=np.uint64)
            assert entry(src, n, o2.ctypes.data, 3, 0x0044, 0x0140, qsrc, 30, rows.ctypes.data, sel.ctypes.data, mode) == 0, err(hip)
            want = expect(*nothing, mode)
            assert np.array_equal(rows, want[0]) and np.array_equal(sel, want[1]), mode
            rows[:] = GARBAGE if mode & 1 else BIAS                             # NULL selected in the synchronous forms
            assert entry(src, n, o2.ctypes.data, 3, 0, 0x904, qsrc, 30, rows.ctypes.data, None, mode) == 0, err(hip)
            assert np.array_equal(rows, expect(want_rows, want_sel, mode)[0]), mode
    # nseg == 0 touches nothing
    assert hip.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), n, None, 0, 0, 0, None, 0, None, None, STORE, None) == 0
    assert hip.FLAGSTATS_hip_u16_x64_segments_filter(values.ctypes.data, n, None, 0, 0, 0, None, 0, None, None, STORE) == 0


# ------------------------------------------------------------------ 7. atomics
def test_three_streams_add_into_one_set_of_rows(hip):
    import torch
    from libflagstats_amd import segments_filter as sf
    rng = np.random.RandomState(73)
    o = np.array([0, 50, 3 * U + 1, 3 * U + 1, 20 * U - 7, 36 * U], dtype=np.int64)
    nseg = o.size - 1
    d_off = dev64(o)
    rows = torch.zeros((nseg, 32), dtype=torch.int64, device="cuda")
    sel = torch.zeros(nseg, dtype=torch.int64, device="cuda")
    total_rows, total_sel = np.zeros((nseg, 32), dtype=np.uint64), np.zeros(nseg, dtype=np.uint64)
    inputs = []
    for n, require, exclude, mn in ((36 * U + 11, 0, 0x904, 30), (30 * U + 5, 0x2, 0x900, 0), (40 * U - 3, 0x0101, 0x8080, 200)):
        values = rng.randint(0, 65536, n).astype(np.uint16)
        mapq = rng.randint(0, 256, n).astype(np.uint8)
        w_rows, w_sel = sfo.want(values, np.clip(o, 0, n), require, exclude, mapq, mn, superset=True)
        assert w_sel.any()
        total_rows += w_rows
        total_sel += w_sel
        inputs.append((dev16(values), require, exclude, dev8(mapq) if mn else None, mn))
    streams = [torch.cuda.Stream() for _ in inputs]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    for st, (t, require, exclude, q, mn) in zip(streams, inputs):
        with torch.cuda.stream(st):
            sf.count_segments_torch_filter(t, d_off, require=require, exclude=exclude, mapq=q, min_mapq=mn, out=rows, selected=sel,
                                           store=False, superset=True)
    for st in streams:
        st.synchronize()
    assert np.array_equal(rows.cpu().numpy().view(np.uint64), total_rows) and np.array_equal(sel.cpu().numpy().view(np.uint64), total_sel)


# ------------------------------------------------------------------ 8. host form across chunks
def test_host_form_across_chunks(hip):
    """chunks of 8,193 flags from offsets[0] = 3 on: segments span several chunks, chunks start at odd and even elements of array
    and column (the host arrays themselves start one element into their buffers), and the column's slice sits 16,386 bytes into
    the staging buffer; flags before offsets[0] and behind offsets[nseg] never cross the bus"""
    from libflagstats_amd import _lib
    from libflagstats_amd import segments_filter as sf
    n = 6 * 8193 + 77
    rng = np.random.RandomState(89)
    values = rng.randint(0, 65536, n + 1).astype(np.uint16)[1:]
    mapq = rng.randint(0, 60, n + 1).astype(np.uint8)[1:]
    o = np.array([3, 10, 10, 8193 + 2, 3 * 8193 + 500, 3 * 8193 + 501, 5 * 8193 + 3, n - 20], dtype=np.int64)
    require, exclude = 0x0001, 0x0804
    old = hip.FLAGSTATS_hip_get(b"chunk_flags")
    try:
        _lib.check(hip.FLAGSTATS_hip_set(b"chunk_flags", 8193), "chunk_flags")
        for q, mn in ((None, 0), (mapq, 30)):
            for sup in (False, True):
                want_rows, want_sel = sfo.want(values, o, require, exclude, q, mn, superset=sup)
                assert want_sel.any() and (want_sel < np.diff(o).astype(np.uint64)).any()
                got = sf.flagstats_segments_filter(values, o, require, exclude, mapq=q, min_mapq=mn, superset=sup)
                assert np.array_equal(got[0], want_rows) and np.array_equal(got[1], want_sel), (mn, sup)
            want_rows, want_sel = sfo.want(values, o, require, exclude, q, mn, superset=True)
            for flags in (0, SUPERSET):                  # += over bias words
                rows = np.full((o.size - 1, 32), BIAS, dtype=np.uint64)
                sel = np.full(o.size - 1, SEL_BIAS, dtype=np.uint64)
                rc = hip.FLAGSTATS_hip_u16_x64_segments_filter(values.ctypes.data, n, o.ctypes.data, o.size - 1, require, exclude,
                                                               q.ctypes.data if mn else None, mn, rows.ctypes.data, sel.ctypes.data, flags)
                assert rc == 0, err(hip)
                w = expect(want_rows, want_sel, flags)
                assert np.array_equal(rows, w[0]) and np.array_equal(sel, w[1]), (mn, flags)
            # one chunk only (a single staging slot), and segments that cover nothing
            for oo in (np.array([1, 50, 99]), np.array([7, 7, 7]), np.array([n, n])):
                got = sf.flagstats_segments_filter(values, oo, require, exclude, mapq=q, min_mapq=mn)
                want = sfo.want(values, oo, require, exclude, q, mn)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), oo
    finally:
        hip.FLAGSTATS_hip_set(b"chunk_flags", old)
    assert hip.FLAGSTATS_hip_get(b"chunk_flags") == old
    got = sf.flagstats_segments_filter(values[:0], [0, 0], 1, 4, mapq=mapq[:0], min_mapq=30)
    assert got[0].shape == (1, 32) and not got[0].any() and not got[1].any()
    got = sf.count_segments_device_ptr_filter(0, 0, [0, 0, 0], 1, 4)
    assert got[0].shape == (2, 32) and not got[0].any() and not got[1].any()


# ------------------------------------------------------------------ 9. refusals
def test_refusals(hip, launcher):
    """every refusal of the C entries, the launcher and what the Python layer can refuse only with a device at hand: each is an
    argument check that returns before anything is launched, and rows and counts stay as they were"""
    import torch
    from libflagstats_amd import segments_filter as sf
    n, nseg = 4096, 3
    t = torch.zeros(n + 8, dtype=torch.int16, device="cuda")
    q = torch.full((n + 8,), 60, dtype=torch.uint8, device="cuda")
    o = np.array([0, 10, 2000, n], dtype=np.uint64)
    d_off = dev64(o)
    out = torch.full((nseg, 32), BIAS, dtype=torch.int64, device="cuda")
    sel = torch.full((nseg,), SEL_BIAS, dtype=torch.int64, device="cuda")
    h_out = np.full((nseg, 32), BIAS, dtype=np.uint64)
    h_sel = np.full(nseg, SEL_BIAS, dtype=np.uint64)
    host16 = np.zeros(n + 8, dtype=np.uint16)
    host8 = np.full(n + 8, 60, dtype=np.uint8)

    def untouched(what):
        torch.cuda.synchronize()
        assert (out == BIAS).all() and (sel == SEL_BIAS).all(), what
        assert (h_out == BIAS).all() and (h_sel == SEL_BIAS).all(), what

    def refused(what, text, d_array=t.data_ptr(), n_=n, offsets=o, nseg_=nseg, require=0, exclude=0x904, d_mapq=q.data_ptr(), mn=30, flags=0,
                rows=True, forms=("device", "sync", "host")):
        d_o = None if offsets is None else dev64(offsets.astype(np.int64))
        for form in forms:
            if form == "device":
                rc = hip.FLAGSTATS_hip_device_u16_segments_filter(d_array, n_, None if d_o is None else d_o.data_ptr(), nseg_, require, exclude,
                                                                  d_mapq, mn, out.data_ptr() if rows else None, sel.data_ptr(), flags, None)
            elif form == "sync":
                rc = hip.FLAGSTATS_hip_device_u16_segments_filter_sync(d_array, n_, None if offsets is None else offsets.ctypes.data, nseg_,
                                                                       require, exclude, d_mapq, mn, h_out.ctypes.data if rows else None,
                                                                       h_sel.ctypes.data, flags)
            else:
                src = host16.ctypes.data + (d_array - t.data_ptr()) if d_array else None
                rc = hip.FLAGSTATS_hip_u16_x64_segments_filter(src, n_, None if offsets is None else offsets.ctypes.data, nseg_, require, exclude,
                                                               host8.ctypes.data if d_mapq else None, mn, h_out.ctypes.data if rows else None,
                                                               h_sel.ctypes.data, flags)
            assert rc != 0, (what, form)
            assert text in err(hip), (what, form, err(hip))
        untouched(what)

    refused("require above 16 bits", "require must be a 16-bit FLAG mask", require=0x10000)
    refused("exclude above 16 bits", "exclude must be a 16-bit FLAG mask", exclude=0x10000)
    refused("min_mapq above a byte", "min_mapq must be at most 255", mn=256)
    refused("NULL mapq", "NULL mapq with min_mapq > 0 and n > 0", d_mapq=None)
    refused("NULL array", "NULL array with n > 0", d_array=None)
    refused("an odd array address", "2-byte aligned", d_array=t.data_ptr() + 1)
    refused("an extra flag bit", "no other bits", flags=4)
    refused("NULL rows", "with nseg > 0", rows=False)
    refused("NULL offsets", "with nseg > 0", offsets=None)
    refused("n * 2 is no size", "n * 2 is not a size", n_=1 << 63)
    refused("too many segments", "nseg is too large", nseg_=1 << 60)
    refused("decreasing offsets", "offsets must be non-decreasing", offsets=np.array([0, 20, 10, n], dtype=np.uint64), forms=("sync", "host"))
    refused("offsets past the array", "exceeds the array's", offsets=np.array([0, 10, 20, n + 1], dtype=np.uint64), forms=("sync", "host"))
    # the column somewhere else than the array: in host memory, a CPU tensor in Python
    rc = hip.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), n, d_off.data_ptr(), nseg, 0, 0x904, host8.ctypes.data, 30, out.data_ptr(),
                                                      sel.data_ptr(), 0, None)
    assert rc != 0 and "d_mapq" in err(hip), err(hip)
    rc = hip.FLAGSTATS_hip_device_u16_segments_filter_sync(t.data_ptr(), n, o.ctypes.data, nseg, 0, 0x904, host8.ctypes.data, 30,
                                                           h_out.ctypes.data, h_sel.ctypes.data, 0)
    assert rc != 0 and "d_mapq" in err(hip), err(hip)
    cpu = {"offsets": torch.zeros(4, dtype=torch.int64), "mapq": torch.zeros(n + 8, dtype=torch.uint8),
           "out": torch.zeros((3, 32), dtype=torch.int64), "selected": torch.zeros(3, dtype=torch.int64)}
    for name, x in cpu.items():
        kw = {"mapq": q, "min_mapq": 30}
        args = [t, d_off]
        if name == "offsets":
            args[1] = x
        else:
            kw[name] = x
        with pytest.raises(ValueError, match=r"%s must live on t's device \(cuda:0\), not on cpu" % name):
            sf.count_segments_torch_filter(*args, **kw)
    untouched("column elsewhere")
    # host pointers (pageable, then page-locked) as d_out, d_selected, d_offsets
    rc = hip.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), n, d_off.data_ptr(), nseg, 0, 0x904, q.data_ptr(), 30, h_out.ctypes.data,
                                                      sel.data_ptr(), 0, None)
    assert rc != 0 and "d_out" in err(hip), err(hip)
    rc = hip.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), n, d_off.data_ptr(), nseg, 0, 0x904, q.data_ptr(), 30, out.data_ptr(),
                                                      h_sel.ctypes.data, 0, None)
    assert rc != 0 and "d_selected" in err(hip), err(hip)
    rc = hip.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), n, o.ctypes.data, nseg, 0, 0x904, q.data_ptr(), 30, out.data_ptr(),
                                                      sel.data_ptr(), 0, None)
    assert rc != 0 and "d_offsets" in err(hip), err(hip)
    pinned = hip.FLAGSTATS_hip_host_alloc(1024)
    assert pinned
    try:
        ctypes.memset(pinned, 0, 1024)
        rc = hip.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), n, d_off.data_ptr(), nseg, 0, 0x904, q.data_ptr(), 30, pinned,
                                                          sel.data_ptr(), STORE, None)
        assert rc != 0 and "d_out must be device memory" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), n, d_off.data_ptr(), nseg, 0, 0x904, q.data_ptr(), 30, out.data_ptr(),
                                                          pinned, STORE, None)
        assert rc != 0 and "d_selected must be device memory" in err(hip), err(hip)
        assert not any(ctypes.string_at(pinned, 1024))
    finally:
        hip.FLAGSTATS_hip_host_free(pinned)
    untouched("host pointers")
    # a stream of another device cannot be made on a one-GPU box; extents: column one byte short, array one flag short, rows,
    # counts and offsets 8 bytes short
    nbytes = 2 << 20
    raw = hip.FLAGSTATS_hip_device_alloc(nbytes)
    big = torch.zeros(nbytes + 8, dtype=torch.int16, device="cuda")
    assert raw
    try:
        assert hip.FLAGSTATS_hip_memcpy_h2d(raw, np.zeros(nbytes, dtype=np.uint8).ctypes.data, nbytes) == 0
        big_off = dev64(np.array([0, 5, 100, nbytes]))
        rc = hip.FLAGSTATS_hip_device_u16_segments_filter(big.data_ptr(), nbytes + 1, big_off.data_ptr(), nseg, 0, 0x904, raw, 30,
                                                          out.data_ptr(), sel.data_ptr(), STORE, None)
        assert rc != 0 and "d_mapq" in err(hip) and "1 bytes short" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_u16_segments_filter_sync(big.data_ptr(), nbytes + 1, np.array([0, 5, 100, nbytes], dtype=np.uint64).ctypes.data,
                                                               nseg, 0, 0x904, raw, 30, h_out.ctypes.data, h_sel.ctypes.data, STORE)
        assert rc != 0 and "d_mapq" in err(hip) and "1 bytes short" in err(hip), err(hip)
        rc = hip.FLAGSTATS_hip_device_u16_segments_filter(raw, nbytes // 2 + 1, big_off.data_ptr(), nseg, 0, 0x904, None, 0, out.data_ptr(),
                                                          sel.data_ptr(), STORE, None)
        assert rc != 0 and "d_array" in err(hip) and "2 bytes short" in err(hip), err(hip)
        end = raw + nbytes
        for name, kw in (("d_out", {"rows": end - nseg * 256 + 8}), ("d_selected", {"counts": end - nseg * 8 + 8}),
                         ("d_offsets", {"offsets": end - (nseg + 1) * 8 + 8})):
            rc = hip.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr(), n, kw.get("offsets", d_off.data_ptr()), nseg, 0, 0x904, q.data_ptr(),
                                                              30, kw.get("rows", out.data_ptr()), kw.get("counts", sel.data_ptr()), 0, None)
            assert rc != 0 and name in err(hip) and "8 bytes short" in err(hip), (name, err(hip))
        back = np.ones(nbytes, dtype=np.uint8)
        assert hip.FLAGSTATS_hip_memcpy_d2h(back.ctypes.data, raw, nbytes) == 0 and not back.any()
    finally:
        hip.FLAGSTATS_hip_device_free(raw)
    untouched("extents")
    # the launcher itself: other mode bits, no workgroups, a wave's uint32 totals, predicates out of range, NULLs -- nothing queued
    words = torch.full((nseg * 33,), BIAS, dtype=torch.int64, device="cuda")
    p, ps = words.data_ptr(), words.data_ptr() + nseg * 256
    a, c, f = t.data_ptr(), q.data_ptr(), d_off.data_ptr()
    assert launcher(a, c, 0, 8, f, nseg, 0, 0x904, 30, p, ps, 4, 1, None) != 0
    assert launcher(a, c, 0, 8, f, nseg, 0, 0x904, 30, p, ps, STORE, 0, None) != 0
    assert launcher(a, None, 0, 1 << 35, f, nseg, 0, 0x904, 0, p, ps, STORE, 1, None) != 0       # 2^33 flags per wave
    assert launcher(a, None, 0, 8, f, nseg, 0x10000, 0, 0, p, ps, STORE, 1, None) != 0
    assert launcher(a, None, 0, 8, f, nseg, 0, 0x10000, 0, p, ps, STORE, 1, None) != 0
    assert launcher(a, c, 0, 8, f, nseg, 0, 0, 256, p, ps, STORE, 1, None) != 0
    assert launcher(a, None, 0, 8, f, nseg, 0, 0, 30, p, ps, STORE, 1, None) != 0
    assert launcher(None, c, 0, 8, f, nseg, 0, 0, 30, p, ps, STORE, 1, None) != 0
    assert launcher(a + 1, c, 0, 8, f, nseg, 0, 0, 30, p, ps, STORE, 1, None) != 0
    assert launcher(a, c, 0, 8, None, nseg, 0, 0, 30, p, ps, STORE, 1, None) != 0
    assert launcher(a, c, 0, 8, f, nseg, 0, 0, 30, None, ps, STORE, 1, None) != 0
    torch.cuda.synchronize()
    assert (words == BIAS).all()
