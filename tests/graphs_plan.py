"""Inputs and expected values of tests/test_gpu_graphs.py (every stream-taking device entry captured into a HIP graph, replayed,
its buffers rewritten, replayed again), built without a GPU: test_graphs_plan_host.py checks on any machine what the GPU tests
rely on.

Every input comes twice, as data set "A" and data set "B": the same sizes, addresses and alignments, different contents.  A graph
is captured over A, replayed, then B is copied into the same device buffers and the graph replayed again: a launch that froze
anything but its pointers and its geometry at capture time gives A's values once more.

Expected values never come from the code under test: oracle.flagstat_hist, where_oracle / filter_oracle.want_counters,
wide_filter_oracle.want, segments_oracle.segmented_counters, segments_filter_oracle.want and steps_oracle.periodic_pospopcnt.

Layout of every input (``Slab``): the elements a launch may read sit inside a larger host array whose other elements would
change the result if they were read -- flags and wide elements that pass every predicate and count in several slots (the wide
ones with every high bit set), MAPQ and selection bytes of 0xFF (they reach every threshold, select, and are all ones as bitmap
bits)."""
import numpy as np

import filter_oracle
import segments_filter_oracle
import where_oracle
import wide_filter_oracle as wfo
from segments_oracle import SEG_UNIT, WriterSplit, segmented_counters
from steps_oracle import STEP_WORDS, StepSplit, periodic_pospopcnt

S = STEP_WORDS
DATA_SETS = ("A", "B")
# name -> (flags, array phase: the first flag lies 2 * phase bytes past a 16-byte line)
SHAPES = {
    "edge": (2 * S + 100, 1),        # a head edge step, one fast step, a tail edge step
    "grouped": (100 * S + 77, 0),    # 101 workgroups of one step each: K1's direct epilogue takes the two-level form
}
REQUIRE, EXCLUDE, MIN_MAPQ = 0x0041, 0x0900, 30       # a predicate on both byte planes
BACKGROUND = 0xFFFF & ~EXCLUDE                        # passes the predicate; QC-fail, paired, read1 + read2, DUP, ...
PAD = 64                                              # elements of background on either side (a multiple of a 16-byte line)
MAPQ_ALIGN, SEL_ALIGN, BIT_OFFSET = 3, 3, 5
NSEG = 40
LONG_SEGMENT = 3 * SEG_UNIT + 123                     # three whole 4,096-flag units and a ragged end
PERIOD = 8191                                         # prime: no step, unit or line is a multiple of it
GRID_BLOCKS = 256                                     # workgroups a launch may use on the MI355X (one per CU)
WIDTHS = (4, 8)
SIGNED = {4: np.int32, 8: np.int64}
# (element index, high bits) of the wide columns, per data set: in the head edge step, the fast step and the tail edge step; the
# last one is the negative element
HIGH_BITS = {
    (4, "A"): ((5, 1 << 17), (S + 3, 1 << 20), (2 * S + 90, 1 << 31)),
    (4, "B"): ((9, 1 << 18), (S + 11, 1 << 29), (2 * S + 70, 1 << 31)),
    (8, "A"): ((5, 1 << 17), (S + 3, 1 << 40), (2 * S + 90, 1 << 63)),
    (8, "B"): ((9, 1 << 18), (S + 11, 1 << 45), (2 * S + 70, (1 << 63) | (1 << 33))),
}


class Slab:
    """one input in both data sets: host arrays ``a`` and ``b`` of one size and dtype; the launch reads ``n`` elements from element
    ``at`` on (``at`` * itemsize bytes past the 16-byte aligned start of the device copy)"""

    def __init__(self, a, b, at, n):
        assert a.shape == b.shape and a.dtype == b.dtype and a.ndim == 1 and 0 <= at and at + n <= a.size
        self.a, self.b, self.at, self.n = a, b, at, n

    def host(self, ds):
        return self.a if ds == "A" else self.b

    def body(self, ds):
        return self.host(ds)[self.at:self.at + self.n]

    def phase_bytes(self):
        return self.at * self.a.dtype.itemsize % 16


def _slab(bodies, background, lead, dtype):
    """the bodies (A, B) behind ``PAD + lead`` elements of background and in front of at least PAD more, a whole number of
    16-byte lines in all"""
    n = bodies[0].size
    per_line = 16 // np.dtype(dtype).itemsize
    size = -(-(PAD + per_line + n + PAD) // per_line) * per_line
    hosts = []
    for body in bodies:
        h = np.full(size, background, dtype=dtype)
        h[PAD + lead:PAD + lead + n] = body
        hosts.append(h)
    return Slab(hosts[0], hosts[1], PAD + lead, n)


def _flags(seed, n):
    """random flags of which 55 % are forced through the predicate (a random 16-bit value passes it one time in 16)"""
    rng = np.random.RandomState(seed)
    v = rng.randint(0, 65536, n).astype(np.uint16)
    forced = rng.randint(0, 100, n) < 55
    v[forced] = (v[forced] & np.uint16(~EXCLUDE & 0xFFFF)) | np.uint16(REQUIRE)
    return v


def _offsets(seed, n, long_at, front):
    """NSEG + 1 CSR offsets: two empty segments, short ones of 1, 2, 7, 63 and 65 flags, one of LONG_SEGMENT flags as segment
    ``long_at``, the others random; ``front`` flags in front of the first segment and 50 - ``front`` behind the last belong to none"""
    rng = np.random.RandomState(seed)
    lengths = np.full(NSEG, -1, dtype=np.int64)
    lengths[long_at] = LONG_SEGMENT
    free = [i for i in range(NSEG) if i != long_at]
    rng.shuffle(free)
    for i, length in zip(free, (0, 0, 1, 2, 7, 63, 65)):
        lengths[i] = length
    rest = np.nonzero(lengths < 0)[0]
    room = n - 50 - int(lengths[lengths >= 0].sum())          # 50 flags stay outside every segment
    cuts = np.sort(rng.choice(np.arange(1, room), rest.size - 1, replace=False))
    lengths[rest] = np.diff(np.concatenate([[0], cuts, [room]]))
    o = np.concatenate([[0], np.cumsum(lengths)]) + front
    assert o.size == NSEG + 1 and (np.diff(o) >= 0).all() and o[-1] == n - (50 - front)
    return o.astype(np.uint64)


def cut(want, superset):
    """the superset counters ``want`` ([..., 32]) as a launch without the superset flag reports them"""
    w = np.array(want, dtype=np.uint64)
    if not superset:
        w[..., [0, 9, 16]] = 0
    return w


class Plan:
    """``slabs``: name -> Slab.  ``want``: key -> {data set: {result name: uint64 array}}, counters always in the superset form
    (``cut`` gives the plain form).  ``masks``: key -> {data set: bool[n]}, which elements each predicate or selection passes."""

    def __init__(self):
        self.slabs, self.want, self.masks = {}, {}, {}


_PLAN = None


def plan(oracle_mod):
    """the plan, built once per process"""
    global _PLAN
    if _PLAN is None:
        _PLAN = _build(oracle_mod)
    return _PLAN


def _build(oracle_mod):
    p = Plan()
    for k, (shape, (n, phase)) in enumerate(SHAPES.items()):
        bodies = [_flags(1000 + 10 * k + i, n) for i in range(2)]
        p.slabs["flags", shape] = _slab(bodies, BACKGROUND, phase, np.uint16)
        p.want["k1", shape] = {ds: {"out": where_oracle.want_counters(oracle_mod, body, np.ones(n, dtype=bool), superset=True)}
                               for ds, body in zip(DATA_SETS, bodies)}
        p.want["hist", shape] = {ds: {"out": oracle_mod.flagstat_hist(body).astype(np.uint64)} for ds, body in zip(DATA_SETS, bodies)}
        # the positional popcount's input is periodic: x[i] = pattern[i % PERIOD]
        patterns = [np.random.RandomState(2000 + 10 * k + i).randint(0, 65536, PERIOD).astype(np.uint16) for i in range(2)]
        p.slabs["periodic", shape] = _slab([np.resize(q, n) for q in patterns], 0xFFFF, phase, np.uint16)
        p.want["pospopcnt", shape] = {ds: {"out": periodic_pospopcnt(q, 0, n)} for ds, q in zip(DATA_SETS, patterns)}
    n, _ = SHAPES["edge"]
    flags = p.slabs["flags", "edge"]
    values = {ds: flags.body(ds) for ds in DATA_SETS}
    # MAPQ: 15 .. 59, two thirds reach the threshold
    mapq = {ds: np.random.RandomState(3000 + i).randint(15, 60, n).astype(np.uint8) for i, ds in enumerate(DATA_SETS)}
    p.slabs["mapq"] = _slab([mapq[ds] for ds in DATA_SETS], 0xFF, MAPQ_ALIGN, np.uint8)
    # selections: one boolean mask per data set, as bytes (any non-zero byte selects) and as an LSB-first bitmap from bit 5 on
    sel = {}
    for i, ds in enumerate(DATA_SETS):
        rng = np.random.RandomState(4000 + i)
        sel[ds] = rng.randint(0, 2, n).astype(bool)
        sel[ds, "bytes"] = np.where(sel[ds], np.array([0x01, 0x02, 0x80, 0xFF], dtype=np.uint8)[rng.randint(0, 4, n)], 0).astype(np.uint8)
        sel[ds, "bitmap"] = where_oracle.pack(sel[ds], BIT_OFFSET, fill=1)
    p.slabs["sel", "bytes"] = _slab([sel[ds, "bytes"] for ds in DATA_SETS], 0xFF, SEL_ALIGN, np.uint8)
    p.slabs["sel", "bitmap"] = _slab([sel[ds, "bitmap"] for ds in DATA_SETS], 0xFF, SEL_ALIGN, np.uint8)
    p.masks["where"] = {ds: sel[ds] for ds in DATA_SETS}
    p.want["where"] = {ds: {"out": where_oracle.want_counters(oracle_mod, values[ds], sel[ds], superset=True),
                            "selected": np.array([sel[ds].sum()], dtype=np.uint64)} for ds in DATA_SETS}
    # the predicate without and with the MAPQ column
    for key, mn in (("filter", 0), ("filter_mapq", MIN_MAPQ)):
        p.masks[key] = {ds: filter_oracle.filter_mask(values[ds], REQUIRE, EXCLUDE, mapq[ds], mn) for ds in DATA_SETS}
        p.want[key] = {}
        for ds in DATA_SETS:
            w, nsel = filter_oracle.want_counters(oracle_mod, values[ds], REQUIRE, EXCLUDE, mapq[ds], mn, superset=True)
            p.want[key][ds] = {"out": w, "selected": np.array([nsel], dtype=np.uint64)}
    # segments: the long one is segment 11 in A and segment 29 in B
    offsets = {"A": _offsets(5000, n, 11, 17), "B": _offsets(5001, n, 29, 29)}
    p.slabs["offsets"] = Slab(offsets["A"], offsets["B"], 0, NSEG + 1)
    p.want["segments"] = {ds: {"out": segmented_counters(values[ds], offsets[ds], superset=True)} for ds in DATA_SETS}
    p.want["segments_filter"] = {}
    for ds in DATA_SETS:
        rows, nsel = segments_filter_oracle.want(values[ds], offsets[ds], REQUIRE, EXCLUDE, mapq[ds], MIN_MAPQ, superset=True)
        p.want["segments_filter"][ds] = {"out": rows, "selected": nsel}
    # wide columns: the edge shape's flags in the low 16 bits, one element (4 or 8 bytes) past a 16-byte line
    for W in WIDTHS:
        cols = []
        for ds in DATA_SETS:
            col = values[ds].astype(np.uint64)
            for at, bits in HIGH_BITS[W, ds]:
                col[at] |= np.uint64(bits)
            cols.append(col.astype(wfo.UNSIGNED[W]).view(SIGNED[W]))
        background = np.array([wfo.ALL_HIGH[W] | BACKGROUND], dtype=wfo.UNSIGNED[W]).view(SIGNED[W])[0]
        p.slabs["wide", W] = _slab(cols, background, 1, SIGNED[W])
        p.want["wide", W], p.want["wide_filter", W] = {}, {}
        for ds, col in zip(DATA_SETS, cols):
            w, nsel, high = wfo.want(oracle_mod, col, 0, 0, superset=True)
            assert nsel == n
            p.want["wide", W][ds] = {"out": w, "high": np.array([high], dtype=np.uint64)}
            w, nsel, high = wfo.want(oracle_mod, col, REQUIRE, EXCLUDE, mapq[ds], MIN_MAPQ, superset=True)
            p.want["wide_filter", W][ds] = {"out": w, "selected": np.array([nsel], dtype=np.uint64), "high": np.array([high], dtype=np.uint64)}
    return p


def step_split(shape):
    """K1's step geometry of a shape on the device's grid"""
    n, phase = SHAPES[shape]
    return StepSplit(2 * phase, n, GRID_BLOCKS)


def chain_units(offsets, min_units):
    """whole units the segmented kernels' carry-save chain counts, summed over the writers of a launch over the edge shape"""
    n, phase = SHAPES["edge"]
    return int(WriterSplit(2 * phase, n, GRID_BLOCKS).pieces(np.asarray(offsets, dtype=np.int64), min_units)["chain"].sum())
