"""Case plan and reference of the randomized sweep over the eight kernels derived from K1's step tree (where, filter, segments,
segments_filter, wide, wide_filter, wide_segments, wide_segments_filter): tests/test_gpu_derived_fuzz.py runs the plan on the
device, tests/test_derived_plan_host.py checks plan and reference on the CPU.  No GPU is touched here.

``plan(seed, iters)`` draws every parameter of every case from one ``np.random.RandomState(seed)``, the same quantities in the same
order whatever the build, so the GPU test and the CPU test see one sequence and ``plan(seed, k)`` is a prefix of
``plan(seed, k + 1)``.  What must occur a minimum number of times in a plan of a few hundred cases is dealt, not diced: the
(kind, form) pair of a case comes from a permutation drawn once per block of 36 cases, and the grid / ``chunk_flags`` of a case
rotate with its kind and block.

``reference(case)`` is the definition read aloud: per segment, compact the passing elements with boolean indexing, take their low
16 bits, hand that subsequence to oracle.flagstat_c; it shares no code with the library or with the per-kernel oracles
(where_oracle, filter_oracle, segments*_oracle, wide_filter_oracle), which test_derived_plan_host.py compares it with.
``expected(case, ref)`` applies the call's mode to it.

Two deliberate limits, both recorded in the case itself:
  * a host-form case crosses the bus in at most MAX_CHUNKS chunks (``chunk_flags`` 8 is one vector a chunk: 300,000 elements
    would be 150,000 launches), so its n is reduced modulo MAX_CHUNKS chunks;
  * a bitmap ``sel_offset`` of 2^33 + k needs the selection pointer moved 2^30 bytes back, which names no allocation: the public
    device and _sync entries check the allocation from the pointer itself on and refuse it as documented, so such an offset is
    applied in the direct-launcher and host forms only (``big_offset`` says whether it was); the others get the drawn small one.
No case is skipped: ``case["skip"]`` is None throughout, and test_derived_plan_host.py asserts so."""
import numpy as np

KINDS = ("where_bitmap", "where_bytes", "filter", "segments", "segments_filter", "wide", "wide_filter", "wide_segments",
         "wide_segments_filter")
FAMILY = {"where_bitmap": "where", "where_bytes": "where"}          # kind -> kernel; every other kind is its own
FORMS = ("launcher", "device", "sync", "host")
GRIDS = (1, 2, 3, 5, 8, 61)
CHUNKS = (8, 1000, 8192, 65544)
MIN_UNITS = (0, 1, 2, 3, 255, 256, 0xFFFFFFFF)
NSEGS = (1, 2, 3, 17, 1000)
CAP = 300_000
MAX_CHUNKS = 2000
STEP_BYTES = 32768
PAIRS = len(KINDS) * len(FORMS)

STORE, SUPERSET = 1, 2
GARBAGE, BIAS, SEL_BIAS, MASK_BIAS = 0x5EED_0000_0BAD, 3, 5, (1 << 48) | (1 << 17)
POISON_ELEMS = 64
SIGNED = {2: np.int16, 4: np.int32, 8: np.int64}
UNSIGNED = {2: np.uint16, 4: np.uint32, 8: np.uint64}

SEGMENTED = ("segments", "segments_filter", "wide_segments", "wide_segments_filter")
FILTERED = ("filter", "segments_filter", "wide_filter", "wide_segments_filter")
WIDE = ("wide", "wide_filter", "wide_segments", "wide_segments_filter")
SELECTING = ("where_bitmap", "where_bytes") + FILTERED            # kinds that report `selected`
PLACEMENTS = ("together", "apart", "null")


def family(kind):
    return FAMILY.get(kind, kind)


def _bits(rs, pool=0x0FFF):
    """one to three random bits of `pool`"""
    out = 0
    positions = [b for b in range(16) if pool >> b & 1]
    for _ in range(int(rs.randint(1, 4))):
        out |= 1 << positions[int(rs.randint(0, len(positions)))]
    return out


def _mask_side(rs, pool):
    """require or exclude: 0 (one in five), one to three random bits of 0x0FFF -- of `pool` where it has any: the bits that let one
    drawn element of the array pass, so that a predicate of three bits over an array of twenty elements still selects something --
    or 0xFFFF (one in forty)"""
    r = int(rs.randint(0, 40))
    bits = _bits(rs, pool & 0x0FFF or 0x0FFF)
    return 0 if r < 8 else 0xFFFF if r == 39 else bits


def _values(rs, n):
    """uint16[n]: uniform, NA12878-like, one value repeated, or a 0..65535 ramp"""
    import oracle
    r = int(rs.randint(0, 20))
    seed, first, single = int(rs.randint(0, 2 ** 31)), int(rs.randint(0, 2 ** 40)), int(rs.randint(0, 65536))
    if r < 9:
        return "uniform", rs.randint(0, 65536, n).astype(np.uint16)
    if r < 15:
        return "na12878", oracle.generate(oracle.GEN_NA12878, seed, int(rs.randint(0, 2)), first, n)
    if r < 19:
        return "ramp", ((np.arange(n, dtype=np.uint64) + np.uint64(first)) & np.uint64(0xFFFF)).astype(np.uint16)
    return "single", np.full(n, single, dtype=np.uint16)


def _layout(rs, n, W, nseg):
    """int64[nseg + 1] CSR offsets within [0, n]: cut points with repeats (empty segments), offsets[0] > 0 and offsets[nseg] < n in
    half the cases each, one layout in four on whole units, one in four with runs of 1..9 elements between long ones"""
    front, behind, style = int(rs.randint(0, 2)), int(rs.randint(0, 2)), int(rs.randint(0, 4))
    a, b = int(rs.randint(0, 1 << 30)), int(rs.randint(0, 1 << 30))
    lo = 1 + a % max(1, min(n // 3, 5000)) if front and n > 1 else 0
    hi = n - 1 - b % max(1, min(n // 3, 5000)) if behind and n > 1 else n
    lo, hi = min(lo, hi), max(lo, hi)
    inner = nseg - 1
    raw = rs.randint(0, 1 << 30, inner)
    small = rs.randint(1, 10, inner)
    span = hi - lo
    if style == 2:                                            # whole units of 8192 bytes
        unit = 8192 // W
        cuts = lo + (raw % (span // unit + 1)) * unit
    elif style == 3:                                          # pairs of cuts 1..9 elements apart
        anchors = lo + raw % (span + 1)
        cuts = np.where(np.arange(inner) % 2 == 0, anchors, np.roll(anchors, 1) + small)
    else:
        cuts = lo + raw % (span + 1)
    cuts = np.clip(np.sort(cuts), lo, hi)
    return np.concatenate([[lo], cuts, [hi]]).astype(np.int64), ("random", "random", "units", "runs")[style]


def _draw(rs, index, kind, form, block):
    case = {"index": index, "kind": kind, "family": family(kind), "form": form, "skip": None}
    wide = kind in WIDE
    W = (4, 8)[int(rs.randint(0, 2))] if wide else 2
    signed = bool(rs.randint(0, 2))
    case["W"], case["dtype"] = W, np.dtype(SIGNED[W] if signed else UNSIGNED[W]).name
    rot = KINDS.index(kind) + block
    case["grid"] = GRIDS[rot % len(GRIDS)] if form == "launcher" else None
    case["chunk_flags"] = CHUNKS[rot % len(CHUNKS)] if form == "host" else None
    mu, bpc = int(rs.randint(0, len(MIN_UNITS))), int(rs.randint(1, 3))
    case["policy"] = (MIN_UNITS[mu], bpc) if kind in SEGMENTED else None
    # n: four clusters under the cap
    pick, step = int(rs.randint(0, 4)), STEP_BYTES // W
    draws = (int(rs.randint(0, 64)), int(step * rs.randint(0, 13) + rs.randint(-9, 10)),
             int((16 // W) * rs.randint(0, CAP * W // 16 + 1) + rs.randint(-1, 2)), int(rs.randint(0, CAP + 1)))
    n = max(0, min(draws[pick], CAP))
    if form == "host":
        limit = MAX_CHUNKS * max(2, case["chunk_flags"] * 2 // W)
        if n > limit:
            n %= limit
    case["n"], case["n_cluster"] = n, pick
    case["phase"] = int(rs.randint(0, 16 // W)) * W           # bytes past a 16-byte boundary
    case["mapq_align"], case["sel_align"] = int(rs.randint(0, 16)), int(rs.randint(0, 16))
    small_off, big, k = int(rs.randint(0, 64)), int(rs.randint(0, 8)) == 0, int(rs.randint(0, 8))
    case["big_offset"] = bool(big and kind == "where_bitmap" and form in ("launcher", "host"))
    case["sel_offset"] = ((1 << 33) + k if case["big_offset"] else small_off) if kind == "where_bitmap" else 0
    case["values"], low = _values(rs, n)
    # wide extras: bits above bit 15 on one element in 37, on exactly one element, nowhere
    style, pos = int(rs.randint(0, 3)), int(rs.randint(0, 1 << 30))
    hot = rs.randint(0, 37, n) == 0
    hi = rs.randint(0, 1 << 16, n).astype(np.uint64) << np.uint64(16)
    hi |= rs.randint(0, 1 << 32, n).astype(np.uint64) << np.uint64(32)
    x = low.astype(np.uint64)
    case["high_style"] = ("many", "one", "none")[style] if wide else None
    if wide and n:
        if style == 0:
            x |= np.where(hot, hi, np.uint64(0))
        elif style == 1:
            x[pos % n] |= np.uint64(1) << np.uint64(16 + pos % (8 * W - 16))
    case["array"] = x.astype(UNSIGNED[W]).view(case["dtype"])
    # predicate and MAPQ bytes
    witness = int(rs.randint(0, 1 << 30)) % max(n, 1)         # one element that the drawn bits let pass
    v = int(low[witness]) if n else 0
    require, exclude = _mask_side(rs, v), _mask_side(rs, ~v)
    overlap = int(rs.randint(0, 24)) == 0
    shared = _bits(rs)
    if overlap:
        require, exclude = (require | shared) & 0xFFFF, (exclude | shared) & 0xFFFF
    else:
        exclude &= ~require
    mq = (0, 1, 30, 255, int(rs.randint(0, 256)))[int(rs.randint(0, 5))]
    q = rs.randint(0, 256, n)
    near = rs.randint(0, 3, n) == 0
    q = np.where(near, np.clip(mq + rs.randint(-1, 2, n), 0, 255), q).astype(np.uint8)
    if n:
        q[witness] = max(int(q[witness]), mq)
    mapq_null = bool(rs.randint(0, 2))
    if kind in FILTERED:
        case.update(require=require, exclude=exclude, min_mapq=mq, mapq=q, mapq_null=mapq_null and mq == 0)
    else:
        case.update(require=0, exclude=0, min_mapq=0, mapq=None, mapq_null=True)
    # selection of the `where` kinds: half, sparse, dense, everything (1 in 40), nothing (1 in 40)
    density = (0.5,) * 24 + (0.1,) * 7 + (0.9,) * 7 + (1.0, 0.0)
    d = density[int(rs.randint(0, 40))]
    m = rs.random_sample(n) < d
    case["mask"] = m if kind in ("where_bitmap", "where_bytes") else None
    # segments
    nseg = NSEGS[int(rs.randint(0, len(NSEGS)))]
    offsets, style = _layout(rs, n, W, nseg)
    case["offsets"], case["layout"] = (offsets, style) if kind in SEGMENTED else (None, None)
    case["nseg"] = nseg if kind in SEGMENTED else 1
    case["mode"] = int(rs.randint(0, 4))
    sel_place, high_place = PLACEMENTS[int(rs.randint(0, 3))], PLACEMENTS[int(rs.randint(0, 3))]
    case["selected_at"] = sel_place if kind in SELECTING else None
    case["high_at"] = high_place if wide else None
    return case


def plan(seed, iters):
    """the first `iters` cases of the sequence that `seed` names"""
    rs = np.random.RandomState(seed)
    cases = []
    perm = None
    for it in range(iters):
        block, j = divmod(it, PAIRS)
        if j == 0:
            perm = rs.permutation(PAIRS)
        kind, form = KINDS[perm[j] // len(FORMS)], FORMS[perm[j] % len(FORMS)]
        cases.append(_draw(rs, it, kind, form, block))
    return cases


def describe(case):
    """the drawn parameters of a case, without its arrays: what a failure message carries"""
    keep = ("index", "kind", "form", "W", "dtype", "n", "phase", "grid", "chunk_flags", "policy", "mode", "sel_offset", "sel_align",
            "mapq_align", "require", "exclude", "min_mapq", "mapq_null", "values", "high_style", "nseg", "layout", "selected_at", "high_at")
    d = {k: case[k] for k in keep}
    if case["offsets"] is not None:
        d["offsets"] = (int(case["offsets"][0]), int(case["offsets"][-1]))
    return d


def skip_reasons(cases):
    """[(index, reason)] of the cases the GPU test would not run"""
    return [(c["index"], c["skip"]) for c in cases if c["skip"] is not None]


# ------------------------------------------------------------------ the reference
def segments_of(case):
    """int64[nseg + 1]: the case's segments; the whole array is one segment"""
    return case["offsets"] if case["offsets"] is not None else np.array([0, case["n"]], dtype=np.int64)


def passing(case):
    """bool[n]: which elements the call selects"""
    n, W = case["n"], case["W"]
    if case["mask"] is not None:
        return case["mask"].astype(bool)
    low = case["array"].view(UNSIGNED[W]).astype(np.uint64) & np.uint64(0xFFFF)
    ok = ((low & np.uint64(case["require"])) == np.uint64(case["require"])) & ((low & np.uint64(case["exclude"])) == 0)
    if case["min_mapq"] > 0:
        ok &= case["mapq"] >= case["min_mapq"]
    assert ok.shape == (n,)
    return ok


def reference(case):
    """{"rows": uint64[nseg, 32] with the superset slots, "selected": uint64[nseg], "high": uint64[nseg], "length": uint64[nseg]}"""
    import oracle
    W = case["W"]
    u = case["array"].view(UNSIGNED[W])
    o = segments_of(case)
    nseg = o.size - 1
    rows, selected, high = np.zeros((nseg, 32), dtype=np.uint64), np.zeros(nseg, dtype=np.uint64), np.zeros(nseg, dtype=np.uint64)
    length = np.diff(o).astype(np.uint64)
    if case["require"] & case["exclude"]:
        return {"rows": rows, "selected": selected, "high": high, "length": length}     # no element is read
    ok = passing(case)
    above = u.astype(np.uint64) & ~np.uint64(0xFFFF)
    for i in range(nseg):
        a, b = int(o[i]), int(o[i + 1])
        if b <= a:
            continue
        seg = u[a:b]
        kept = seg[ok[a:b]]
        low = np.ascontiguousarray((kept & UNSIGNED[W](0xFFFF)).astype(np.uint16))
        if low.size:
            rows[i] = oracle.flagstat_c(low)
            pair_all = oracle.samtools_counts(low)["n_pair_all"]
            rows[i, 0], rows[i, 16] = pair_all[0], pair_all[1]
        selected[i] = low.size
        rows[i, 9] = np.uint64(low.size) - rows[i, 25]
        high[i] = np.bitwise_or.reduce(above[a:b])
    return {"rows": rows, "selected": selected, "high": high, "length": length}


def expected(case, ref):
    """(rows, selected or None, high or None) a call in the case's mode must leave in words prefilled with GARBAGE (store) or BIAS /
    SEL_BIAS / MASK_BIAS (+=); None where the kind reports no such value or the case passes NULL for it"""
    mode = case["mode"]
    rows = ref["rows"].copy()
    if not mode & SUPERSET:
        rows[:, [0, 9, 16]] = 0
    selected = ref["selected"].copy() if case["selected_at"] in ("together", "apart") else None
    high = ref["high"].copy() if case["high_at"] in ("together", "apart") else None
    if not mode & STORE:
        rows = rows + np.uint64(BIAS)
        selected = None if selected is None else selected + np.uint64(SEL_BIAS)
        high = None if high is None else high | np.uint64(MASK_BIAS)
    return rows, selected, high


# ------------------------------------------------------------------ inputs as the device sees them: poisoned slabs
def array_image(case):
    """(uint8 image, byte offset of element 0): POISON_ELEMS all-ones elements, `phase` bytes of ones, the array, ones again.  Laid
    at a 16-byte boundary the array starts `phase` bytes past one."""
    W = case["W"]
    body = np.ascontiguousarray(case["array"]).view(np.uint8)
    front = POISON_ELEMS * W + case["phase"]
    img = np.full(front + body.size + POISON_ELEMS * W + 16, 0xFF, dtype=np.uint8)
    img[front:front + body.size] = body
    return img, front


def bytes_image(column, align):
    """(uint8 image, offset of byte 0) of a MAPQ or byte-selection column: 0xFF around it, byte 0 `align` bytes past a 16-byte
    boundary"""
    front = 64 + align
    img = np.full(front + column.size + 64, 0xFF, dtype=np.uint8)
    img[front:front + column.size] = column
    return img, front


def bitmap_image(case):
    """(uint8 image, offset in it of the packed selection's first byte, bytes the selection pointer is moved BACK from there): element
    i is bit sel_offset + i from the moved pointer on; LSB-first, ones in the unused bits of the first and last byte, 0xFF bytes
    around"""
    s = case["sel_offset"]
    local = s & 7 if case["big_offset"] else s
    nbits = local + case["n"]
    bits = np.ones((nbits + 7) // 8 * 8, dtype=bool)
    bits[local:nbits] = case["mask"]
    packed = np.packbits(bits, bitorder="little")
    front = 64 + case["sel_align"]
    img = np.full(front + packed.size + 64, 0xFF, dtype=np.uint8)
    img[front:front + packed.size] = packed
    return img, front, (s - local) // 8


def output_layout(case):
    """the output allocations of a case as numpy images: ([uint64 prefilled allocation, ...], {"rows" / "selected" / "high":
    (allocation, first word, words)}).  Every allocation has one spare row (32 words) of GARBAGE in front of and behind its
    payload; a value placed "together" follows the rows (selected first, then high), one placed "apart" has its own allocation."""
    nseg, store = case["nseg"], bool(case["mode"] & STORE)
    fill = {"rows": GARBAGE if store else BIAS, "selected": GARBAGE if store else SEL_BIAS, "high": GARBAGE if store else MASK_BIAS}
    main = [("rows", nseg * 32)]
    apart = []
    for name, at in (("selected", case["selected_at"]), ("high", case["high_at"])):
        if at == "together":
            main.append((name, nseg))
        elif at == "apart":
            apart.append([(name, nseg)])
    allocs, where = [], {}
    for parts in [main] + apart:
        words = np.full(32 + sum(c for _, c in parts) + 32, GARBAGE, dtype=np.uint64)
        at = 32
        for name, count in parts:
            words[at:at + count] = fill[name]
            where[name] = (len(allocs), at, count)
            at += count
        allocs.append(words)
    return allocs, where


def expected_images(case, ref):
    """the allocations of output_layout as they must read after the call: the payloads replaced, every spare word as it was"""
    allocs, where = output_layout(case)
    rows, selected, high = expected(case, ref)
    for name, value in (("rows", rows), ("selected", selected), ("high", high)):
        if name in where:
            k, at, count = where[name]
            allocs[k][at:at + count] = value.ravel()
    return allocs


def fixed_case(kind, form, array, mode, mask=None, sel_offset=0, require=0, exclude=0, mapq=None, min_mapq=0, offsets=None, phase=0,
               mapq_align=0, sel_align=0, selected_at="together", high_at="together", index=-1):
    """a case that is stated, not drawn: the dict that reference / expected / the images above take, for the tests with a fixed
    sequence of calls"""
    array = np.ascontiguousarray(array)
    W = array.dtype.itemsize
    assert kind in KINDS and form in FORMS and (W == 2) == (kind not in WIDE) and phase % W == 0
    assert (mask is not None) == (kind in ("where_bitmap", "where_bytes")) and (offsets is not None) == (kind in SEGMENTED)
    assert kind in FILTERED or (require == exclude == min_mapq == 0 and mapq is None)
    return {"index": index, "kind": kind, "family": family(kind), "form": form, "skip": None, "W": W, "dtype": array.dtype.name, "grid": None,
            "chunk_flags": None, "policy": None, "n": array.size, "n_cluster": None, "phase": phase, "mapq_align": mapq_align,
            "sel_align": sel_align, "big_offset": False, "sel_offset": sel_offset, "values": "fixed", "high_style": None, "array": array,
            "require": require, "exclude": exclude, "min_mapq": min_mapq, "mapq": mapq, "mapq_null": mapq is None,
            "mask": None if mask is None else np.asarray(mask, dtype=bool),
            "offsets": None if offsets is None else np.asarray(offsets, dtype=np.int64), "layout": "fixed" if offsets is not None else None,
            "nseg": 1 if offsets is None else len(offsets) - 1, "mode": mode,
            "selected_at": selected_at if kind in SELECTING else None, "high_at": high_at if kind in WIDE else None}
