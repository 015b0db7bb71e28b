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
No case is skipped: ``case["skip"]`` is None throughout, and test_derived_plan_host.py asserts so.

``plan_later(seed, iters)`` is the same for the nine units derived afterwards (LATER_KINDS: the masked kinds, which take a
selection and, where they filter, a predicate as well, and the two kinds of the whole predicate, --rf / -G).  It is a sequence of
its own, drawn with the pieces that ``_draw`` is made of, so ``plan`` is byte for byte what it was (test_derived_plan_host.py pins
its digest).  Beyond an existing case a later one carries ``sel_bits`` (dealt: it alternates with block and form), the --rf / -G
masks with the outcome of the host reduction that they were built for (``rf_outcome``, dealt from RF_OUTCOMES), and, in the
masked wide kinds, decoys: an unselected element with every bit above bit 15 set, and in the ``one`` style the column's single
high bit in an unselected slot about half the time.  The big bitmap offset is dealt to half of the launcher- and host-form
bitmap cases.

``plan_rf_segmented(seed, iters)`` is a third sequence, for the segmented units of the whole predicate (RF_SEGMENTED_KINDS: so far
``segments_filter_rf``), dealt in blocks of one case a form -- ``_deal`` takes its block size from the kinds it is given, which
leaves the two sequences above byte for byte what they were (both digests are pinned).  Its cases are drawn with _draw_later's
pieces.  What the dice do not produce in a few hundred cases is dealt: a position of the array's first or last vector that lies
outside the array is zero-filled by the kernel, and flag 0 with MAPQ 0 passes an all-of test that stands alone (nothing required,
no -q); only the per-flag count's valid-bits mask keeps it out.  ``hazard_dealt`` says which cases get such a predicate and a
segment that touches such a vector (``case["hazard"]``: "front" or "back"), half of them short enough for the per-flag regime
under any policy.

``Definition`` states what the headers define, one method each: counted(j) = pass(j) && sel(j), ``selected`` the number counted,
``high`` over the selected elements, passing or not (every element where the kind takes no selection), nothing read where no FLAG
value can pass.  ``reference`` evaluates it; the wrong models of test_derived_plan_host.py override one method each."""
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

# the nine units derived afterwards: plan_later deals them as plan deals KINDS.  A masked kind takes a selection (sel_bits 1 or 8
# is part of the case, not of the kind) and, where it also filters, a predicate; an rf kind takes samtools' --rf / -G masks.
LATER_KINDS = ("segments_where", "wide_where", "wide_segments_where", "filter_where", "segments_filter_where", "wide_filter_where",
               "wide_segments_filter_where", "filter_rf", "wide_filter_rf")
RF = ("filter_rf", "wide_filter_rf")
MASKED = tuple(k for k in LATER_KINDS if k.endswith("where"))
LATER_SEGMENTED = tuple(k for k in LATER_KINDS if "segments" in k)
LATER_FILTERED = tuple(k for k in LATER_KINDS if "filter" in k)
LATER_WIDE = tuple(k for k in LATER_KINDS if k.startswith("wide"))
RF_OUTCOMES = ("empty", "pair", "any", "all", "both")       # what the host reduction can leave of the four FLAG masks
assert len(LATER_KINDS) * len(FORMS) == PAIRS

# the segmented units of the whole predicate: plan_rf_segmented deals them, in blocks of their own size.  The wide and the masked
# ones join this tuple when they are built.
RF_SEGMENTED_KINDS = ("segments_filter_rf",)
UNIT_FLAGS = 4096                                           # flags of one unit of the segmented uint16 kernels (8192 bytes)
HAZARD_EVERY = 3                                            # of the all-of cases of a form, every third is dealt the hazard


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


def _geometry(rs, case, rot, wide, segmented):
    """element width and type, grid / chunk_flags (rotating with `rot`), segment policy, n in its four clusters, the three
    alignments; returns the drawn small selection offset, whether a big one was drawn, and its k"""
    form = case["form"]
    W = (4, 8)[int(rs.randint(0, 2))] if wide else 2
    signed = bool(rs.randint(0, 2))
    case["W"], case["dtype"] = W, np.dtype(SIGNED[W] if signed else UNSIGNED[W]).name
    case["grid"] = GRIDS[rot % len(GRIDS)] if form == "launcher" else None
    case["chunk_flags"] = CHUNKS[rot % len(CHUNKS)] if form == "host" else None
    mu, bpc = int(rs.randint(0, len(MIN_UNITS))), int(rs.randint(1, 3))
    case["policy"] = (MIN_UNITS[mu], bpc) if segmented else None
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
    return int(rs.randint(0, 64)), int(rs.randint(0, 8)) == 0, int(rs.randint(0, 8))


def _column(rs, case, wide):
    """the array: its low 16 bits by _values; wide extras: bits above bit 15 on one element in 37, on exactly one element, nowhere.
    Returns (the low 16 bits, the high style drawn, the draw that places the single high bit)"""
    n, W = case["n"], case["W"]
    case["values"], low = _values(rs, n)
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
    return low, style, pos


def _predicate(rs, low):
    """require / exclude / min_mapq and the MAPQ bytes: {"witness": an element that the drawn bits let pass, "require", "exclude",
    "overlap": the pair was made to share bits, "min_mapq", "mapq", "mapq_null"}"""
    n = low.size
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
    return {"witness": witness, "value": v, "require": require, "exclude": exclude, "overlap": overlap, "min_mapq": mq, "mapq": q,
            "mapq_null": mapq_null and mq == 0}


def _selection(rs, n):
    """(bool[n], its density): half, sparse, dense, everything (1 in 40), nothing (1 in 40)"""
    density = (0.5,) * 24 + (0.1,) * 7 + (0.9,) * 7 + (1.0, 0.0)
    d = density[int(rs.randint(0, 40))]
    return rs.random_sample(n) < d, d


def _segments(rs, case, segmented):
    nseg = NSEGS[int(rs.randint(0, len(NSEGS)))]
    offsets, style = _layout(rs, case["n"], case["W"], nseg)
    case["offsets"], case["layout"] = (offsets, style) if segmented else (None, None)
    case["nseg"] = nseg if segmented else 1


def _outputs(rs, case, selecting, wide):
    case["mode"] = int(rs.randint(0, 4))
    sel_place, high_place = PLACEMENTS[int(rs.randint(0, 3))], PLACEMENTS[int(rs.randint(0, 3))]
    case["selected_at"] = sel_place if selecting else None
    case["high_at"] = high_place if wide else None


def _draw(rs, index, kind, form, block):
    case = {"index": index, "kind": kind, "family": family(kind), "form": form, "skip": None}
    wide = kind in WIDE
    small_off, big, k = _geometry(rs, case, KINDS.index(kind) + block, wide, kind in SEGMENTED)
    case["big_offset"] = bool(big and kind == "where_bitmap" and form in ("launcher", "host"))
    case["sel_offset"] = ((1 << 33) + k if case["big_offset"] else small_off) if kind == "where_bitmap" else 0
    low, _, _ = _column(rs, case, wide)
    p = _predicate(rs, low)
    if kind in FILTERED:
        case.update(require=p["require"], exclude=p["exclude"], min_mapq=p["min_mapq"], mapq=p["mapq"], mapq_null=p["mapq_null"])
    else:
        case.update(require=0, exclude=0, min_mapq=0, mapq=None, mapq_null=True)
    m, _ = _selection(rs, case["n"])
    case["mask"] = m if kind in ("where_bitmap", "where_bytes") else None
    _segments(rs, case, kind in SEGMENTED)
    _outputs(rs, case, kind in SELECTING, wide)
    return case


def _deal(seed, iters, kinds, draw):
    rs = np.random.RandomState(seed)
    cases = []
    perm = None
    pairs = len(kinds) * len(FORMS)                           # a block holds every (kind, form) once
    for it in range(iters):
        block, j = divmod(it, pairs)
        if j == 0:
            perm = rs.permutation(pairs)
        kind, form = kinds[perm[j] // len(FORMS)], FORMS[perm[j] % len(FORMS)]
        cases.append(draw(rs, it, kind, form, block))
    return cases


def plan(seed, iters):
    """the first `iters` cases of the sequence that `seed` names"""
    return _deal(seed, iters, KINDS, _draw)


def _positions(mask):
    return [b for b in range(16) if mask >> b & 1]


def _several(rs, pool, prefer):
    """two to four distinct bits of `pool` (which has two or more): the first from `prefer` where the pool has any of it"""
    draws, k = rs.randint(0, 1 << 30, 4), 2 + int(rs.randint(0, 3))
    firsts = _positions(pool & prefer) or _positions(pool)
    first = firsts[int(draws[0]) % len(firsts)]
    rest = [b for b in _positions(pool) if b != first]
    out = 1 << first
    for d in draws[1:k]:
        out |= 1 << rest[int(d) % len(rest)]
    return out


def _rf_masks(rs, outcome, require, exclude, v):
    """(require, exclude, include_any, exclude_all) that the host reduction must turn into `outcome` (RF_OUTCOMES), dealt by the
    caller: bits are drawn over all of 0xFFFF, the any-of test around a bit the witness value `v` has, the all-of test around one
    it lacks.  The pair loses bits 12-15 and its overlap, so that eight bits or more are free and `empty` occurs only as dealt."""
    r = require & 0x0FFF
    e = exclude & 0x0FFF & ~r
    free = 0xFFFF & ~(r | e)
    any2, all2 = _several(rs, free, v), _several(rs, free, ~v)
    s, variant = rs.randint(0, 1 << 30, 2), int(rs.randint(0, 3))
    spots = _positions(free & v) or _positions(free)
    bit_a = 1 << spots[int(s[0]) % len(spots)]                # alone in --rf it is a required bit
    spots = _positions(free & ~v & ~bit_a) or _positions(free & ~bit_a)
    bit_g = 1 << spots[int(s[1]) % len(spots)]                # alone in -G it is an excluded bit
    low_r, low_e = r & -r, e & -e
    if outcome == "empty":     # every --rf bit excluded; every -G bit required; an overlapping pair
        return ((r, e | any2, any2, 0), (r | all2, e, 0, all2), (r | bit_a, e | bit_a, any2, all2))[variant]
    if outcome == "pair":      # single bits; tests that -f / -F already decide; a single --rf bit alone
        return ((r, e, bit_a, bit_g), (r, e, any2 | low_r if r else 0, all2 | low_e if e else 0), (r, e, bit_a, 0))[variant]
    if outcome == "any":
        return r, e, any2, (0, 0 if bit_g & any2 else bit_g, all2 | low_e if e else 0)[variant]
    if outcome == "all":
        return r, e, (0, 0 if bit_a & all2 else bit_a, any2 | low_r if r else 0)[variant], all2
    assert outcome == "both"
    return r, e, any2 | (low_e if variant == 1 else 0), all2 | (low_r if variant == 2 else 0)


def _draw_later(rs, index, kind, form, block):
    """_draw for LATER_KINDS: the same pieces in the same order, then what only these kinds have"""
    case = {"index": index, "kind": kind, "family": kind, "form": form, "skip": None}
    wide, segmented, masked, rf = kind in LATER_WIDE, kind in LATER_SEGMENTED, kind in MASKED, kind in RF
    ki, fi = LATER_KINDS.index(kind), FORMS.index(form)
    small_off, big, k = _geometry(rs, case, ki + block, wide, segmented)
    # dealt: sel_bits alternates with block and form; half the bitmap cases of the launcher and host forms take the big offset
    case["sel_bits"] = (1, 8)[(block + fi) % 2] if masked else None
    dealt = (block // 2 + ki) % 2 == 0
    case["big_offset"] = bool((big or dealt) and case["sel_bits"] == 1 and form in ("launcher", "host"))
    case["sel_offset"] = ((1 << 33) + k if case["big_offset"] else small_off) if masked else 0
    low, style, pos = _column(rs, case, wide)
    p = _predicate(rs, low)
    if kind in LATER_FILTERED:
        case.update(require=p["require"], exclude=p["exclude"], min_mapq=p["min_mapq"], mapq=p["mapq"], mapq_null=p["mapq_null"])
    else:
        case.update(require=0, exclude=0, min_mapq=0, mapq=None, mapq_null=True)
    m, density = _selection(rs, case["n"])
    _segments(rs, case, segmented)
    _outputs(rs, case, True, wide)
    # --rf / -G
    case["rf_outcome"] = RF_OUTCOMES[(block * len(FORMS) + fi + ki) % len(RF_OUTCOMES)] if rf else None
    masks = _rf_masks(rs, case["rf_outcome"] or "both", p["require"], p["exclude"], p["value"])
    case["include_any"], case["exclude_all"] = masks[2:] if rf else (0, 0)
    if rf:
        case["require"], case["exclude"] = masks[:2]
    # the selection: the witness is selected as well as passing; decoys in the masked wide kinds
    n, W = case["n"], case["W"]
    e = rs.randint(0, 1 << 30, 2)
    case["mask"] = m if masked else None
    if masked and n and density > 0:
        m[p["witness"]] = True
    if masked and wide and n >= 3 and style in (0, 1):
        u = case["array"].view(UNSIGNED[W]).copy()
        single = pos % n
        if style == 1 and e[1] & 1 and single != p["witness"]:
            m[single] = False                                 # the one high bit of the column lies in a slot that is not selected
        else:
            if style == 1 and density > 0:
                m[single] = True
            decoy = int(e[0]) % n
            while decoy == p["witness"] or (style == 1 and decoy == single):
                decoy = (decoy + 1) % n
            m[decoy] = False
            u[decoy] |= UNSIGNED[W](np.iinfo(UNSIGNED[W]).max - 0xFFFF)     # every bit above bit 15, the low 16 as drawn
        case["array"] = u.view(case["dtype"])
    if wide and n and case["rf_outcome"] == "empty":
        # a call that reads nothing says nothing about the column: let the column have something to say, and the call a place for it
        u = case["array"].view(UNSIGNED[W]).copy()
        u[int(e[0]) % n] |= UNSIGNED[W](np.iinfo(UNSIGNED[W]).max - 0xFFFF)
        case["array"] = u.view(case["dtype"])
        case["high_at"] = "together" if case["high_at"] == "null" else case["high_at"]
    return case


def plan_later(seed, iters):
    """plan() for LATER_KINDS: the first `iters` cases of the sequence that `seed` names, under plan()'s contract"""
    return _deal(seed, iters, LATER_KINDS, _draw_later)


def hazard_dealt(outcome, block):
    """None, or the number 0, 1, 2, ... of the dealt zero-fill case that the rf-segmented plan makes of a case of `block` with the
    dealt `outcome`: a (kind, form) pair is dealt `all` once in five blocks, and every HAZARD_EVERY-th of those is taken"""
    turn = block // len(RF_OUTCOMES)
    return turn // HAZARD_EVERY if outcome == "all" and turn % HAZARD_EVERY == 0 else None


def _hazard_shape(case, h):
    """Before the column is drawn: n, phase and policy of dealt zero-fill case number `h`.  The array starts off a 16-byte boundary
    and ends off one, so its first vector holds positions before element 0 and its last one positions past element n - 1; an even
    `h` keeps the drawn n under two thirds of a unit, so that no segment has a whole unit and every policy counts flag by flag,
    an odd one makes room for a segment of five units (six or more in the array) and takes one of the four smallest MIN_UNITS."""
    index, lanes = case["index"], 8
    case["phase"] = case["phase"] or 2 * (1 + index % 7)
    n = case["n"]
    if h % 2 == 0:
        n = 9 + n % (2 * UNIT_FLAGS // 3)
    else:
        n = max(n, 6 * UNIT_FLAGS + index % 1000)
        case["policy"] = (MIN_UNITS[index % 4], case["policy"][1])
        if case["form"] == "host":
            n = min(n, MAX_CHUNKS * max(2, case["chunk_flags"]))
    while n % lanes == 0 or (case["phase"] // 2 + n) % lanes == 0:    # a ragged end in memory, and in a staged chunk as well
        n += 1
    case["n"] = n


def _hazard_layout(case, h):
    """After the layout is drawn: its first segment becomes [0, L) (`h // 2` even; the device forms only, a staged chunk starts on
    a boundary) or its last one [n - L, n), L under a unit for an even `h` and five units and a bit for an odd one, and nothing
    else moves but to stay in order."""
    n, o = case["n"], case["offsets"].copy()
    L = min(n, 1 + case["index"] % 1000 if h % 2 == 0 else 5 * UNIT_FLAGS + case["index"] % 1000)
    front = (h // 2) % 2 == 0 and case["form"] != "host"
    if front:
        o[0], o[1] = 0, L
        o[2:] = np.maximum(o[2:], L)
    else:
        o[-1], o[-2] = n, n - L
        o[:-2] = np.minimum(o[:-2], n - L)
    case["offsets"], case["hazard"] = o, "front" if front else "back"


def _draw_rf_segmented(rs, index, kind, form, block):
    """_draw_later for RF_SEGMENTED_KINDS: the pieces of _draw_later that a segmented uint16 kind of the whole predicate has, in
    that order.  Dealt on top of the dice: the zero-fill hazard (hazard_dealt says where) -- an all-of test alone, nothing
    required, no -q, the MAPQ column NULL or given in turn, and a segment that touches the ragged first or last vector of the
    array; a position there holds flag 0 and MAPQ 0, which such a predicate passes."""
    case = {"index": index, "kind": kind, "family": kind, "form": form, "skip": None, "hazard": None}
    ki, fi = RF_SEGMENTED_KINDS.index(kind), FORMS.index(form)
    case["rf_outcome"] = RF_OUTCOMES[(block * len(FORMS) + fi + ki) % len(RF_OUTCOMES)]      # _draw_later's rotation
    h = hazard_dealt(case["rf_outcome"], block)
    _geometry(rs, case, ki + block, False, True)
    if h is not None:
        _hazard_shape(case, h)
    case["sel_bits"], case["big_offset"], case["sel_offset"] = None, False, 0
    low, _, _ = _column(rs, case, False)
    p = _predicate(rs, low)
    case.update(require=p["require"], exclude=p["exclude"], min_mapq=p["min_mapq"], mapq=p["mapq"], mapq_null=p["mapq_null"])
    _selection(rs, case["n"])                                 # drawn as _draw_later draws it; the kind takes none
    case["mask"] = None
    _segments(rs, case, True)
    _outputs(rs, case, True, False)
    masks = _rf_masks(rs, case["rf_outcome"], 0 if h is not None else p["require"], p["exclude"], p["value"])
    case["require"], case["exclude"], case["include_any"], case["exclude_all"] = masks
    if h is not None:
        assert case["require"] == 0
        case["include_any"], case["min_mapq"] = 0, 0
        case["mapq_null"] = (h // 2 % 2 == 1) if form == "host" else (h % 4 in (1, 2))       # both ways beside either segment
        _hazard_layout(case, h)
    return case


def plan_rf_segmented(seed, iters):
    """plan() for RF_SEGMENTED_KINDS, in blocks of one case a form: the first `iters` cases of the sequence that `seed` names,
    under plan()'s contract"""
    return _deal(seed, iters, RF_SEGMENTED_KINDS, _draw_rf_segmented)


def describe(case):
    """the drawn parameters of a case, without its arrays: what a failure message carries"""
    keep = ("index", "kind", "form", "W", "dtype", "n", "phase", "grid", "chunk_flags", "policy", "mode", "sel_offset", "sel_align",
            "mapq_align", "require", "exclude", "min_mapq", "mapq_null", "values", "high_style", "nseg", "layout", "selected_at", "high_at")
    d = {k: case[k] for k in keep}
    d.update({k: case[k] for k in ("sel_bits", "include_any", "exclude_all", "rf_outcome", "hazard") if k in case})   # later kinds
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


_EVERY_FLAG = np.arange(65536, dtype=np.uint64)


class Definition:
    """The headers' definitions, one method each, in the plain way.  reference() evaluates them; the wrong models of
    tests/test_derived_plan_host.py override one method each, which is how the plan shows what it would notice."""

    def any_of(self, f, include_any):
        return (f & include_any) != 0

    def all_of(self, f, exclude_all):
        return (f & exclude_all) != exclude_all

    def flag_pass(self, f, require, exclude, include_any, exclude_all):
        """-f / -F / --rf / -G on FLAG values f (uint64): the last two are off at 0"""
        ok = ((f & np.uint64(require)) == np.uint64(require)) & ((f & np.uint64(exclude)) == 0)
        if include_any:
            ok &= self.any_of(f, np.uint64(include_any))
        if exclude_all:
            ok &= self.all_of(f, np.uint64(exclude_all))
        return ok

    def masks(self, case):
        return case["require"], case["exclude"], case.get("include_any", 0), case.get("exclude_all", 0)

    def reads(self, case):
        """False where no FLAG value at all passes the call's FLAG masks: such a call launches nothing and reads nothing.  Decided
        by trying all 65,536 values, never by the library's reduction of the masks."""
        return bool(self.flag_pass(_EVERY_FLAG, *self.masks(case)).any())

    def mapq(self, case):
        return case["mapq"]

    def sel(self, case):
        """bool[n], element j of the ARRAY at index j: the selection; every element where the kind takes none"""
        return np.ones(case["n"], dtype=bool) if case["mask"] is None else case["mask"].astype(bool)

    def passes(self, case):
        """bool[n]: pass(j), the predicate alone"""
        low = case["array"].view(UNSIGNED[case["W"]]).astype(np.uint64) & np.uint64(0xFFFF)
        ok = self.flag_pass(low, *self.masks(case))
        if case["min_mapq"] > 0:
            ok &= self.mapq(case) >= case["min_mapq"]
        return ok

    def segment(self, offsets, i):
        return int(offsets[i]), int(offsets[i + 1])

    def selected(self, sel, counted):
        """the number counted -- not the number selected"""
        return int(counted.sum())

    def high(self, case, above, sel, counted):
        """OR over the selected elements, passing or not; a kind without a selection selects every element"""
        return np.bitwise_or.reduce(above[sel]) if sel.any() else np.uint64(0)

    def unread_high(self, case, above):
        return np.uint64(0)

    def stray(self, case, ok, a, b):
        """uint16[k]: flags that the non-empty segment [a, b) counts beside those of its own elements that pass -- none"""
        return np.zeros(0, dtype=np.uint16)


def passing(case, d=None):
    """bool[n]: counted(j) = pass(j) && sel(j)"""
    d = d or Definition()
    ok = d.passes(case) & d.sel(case)
    assert ok.shape == (case["n"],)
    return ok


def reference(case, d=None):
    """{"rows": uint64[nseg, 32] with the superset slots, "selected": uint64[nseg], "high": uint64[nseg], "length": uint64[nseg]}"""
    import oracle
    d = d or Definition()
    W = case["W"]
    u = case["array"].view(UNSIGNED[W])
    o = segments_of(case)
    nseg = o.size - 1
    rows, selected, high = np.zeros((nseg, 32), dtype=np.uint64), np.zeros(nseg, dtype=np.uint64), np.zeros(nseg, dtype=np.uint64)
    length = np.diff(o).astype(np.uint64)
    above = u.astype(np.uint64) & ~np.uint64(0xFFFF)
    if not d.reads(case):
        high[:] = d.unread_high(case, above)
        return {"rows": rows, "selected": selected, "high": high, "length": length}     # no element is read
    ok, sel = passing(case, d), d.sel(case)
    for i in range(nseg):
        a, b = d.segment(o, i)
        if b <= a:
            continue
        seg = u[a:b]
        kept = seg[ok[a:b]]
        extra = d.stray(case, ok, a, b)
        low = np.ascontiguousarray(np.concatenate([(kept & UNSIGNED[W](0xFFFF)).astype(np.uint16), extra]))
        if low.size:
            rows[i] = oracle.flagstat_c(low)
            pair_all = oracle.samtools_counts(low)["n_pair_all"]
            rows[i, 0], rows[i, 16] = pair_all[0], pair_all[1]
        selected[i] = d.selected(sel[a:b], ok[a:b]) + extra.size
        rows[i, 9] = np.uint64(low.size) - rows[i, 25]
        high[i] = d.high(case, above[a:b], sel[a:b], ok[a:b])
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
               mapq_align=0, sel_align=0, selected_at="together", high_at="together", index=-1, sel_bits=None, include_any=0,
               exclude_all=0):
    """a case that is stated, not drawn: the dict that reference / expected / the images above take, for the tests with a fixed
    sequence of calls.  A later kind (LATER_KINDS, RF_SEGMENTED_KINDS) with a selection states its `sel_bits`; an rf kind its
    --rf / -G masks."""
    array = np.ascontiguousarray(array)
    W = array.dtype.itemsize
    later_kinds = LATER_KINDS + RF_SEGMENTED_KINDS
    assert kind in KINDS + later_kinds and form in FORMS and (W == 2) == (kind not in WIDE + LATER_WIDE) and phase % W == 0
    if kind in later_kinds:
        assert (mask is not None) == (kind in MASKED) == (sel_bits in (1, 8))
        assert (offsets is not None) == (kind in LATER_SEGMENTED + RF_SEGMENTED_KINDS)
        assert kind in LATER_FILTERED + RF_SEGMENTED_KINDS or (require == exclude == min_mapq == 0 and mapq is None)
        assert kind in RF + RF_SEGMENTED_KINDS or include_any == exclude_all == 0
        later = {"sel_bits": sel_bits, "include_any": include_any, "exclude_all": exclude_all, "rf_outcome": None}
    else:
        assert (mask is not None) == (kind in ("where_bitmap", "where_bytes")) and (offsets is not None) == (kind in SEGMENTED)
        assert kind in FILTERED or (require == exclude == min_mapq == 0 and mapq is None)
        assert sel_bits is None and include_any == exclude_all == 0
        later = {}
    return {**later,
            "index": index, "kind": kind, "family": family(kind), "form": form, "skip": None, "W": W, "dtype": array.dtype.name, "grid": None,
            "chunk_flags": None, "policy": None, "n": array.size, "n_cluster": None, "phase": phase, "mapq_align": mapq_align,
            "sel_align": sel_align, "big_offset": False, "sel_offset": sel_offset, "values": "fixed", "high_style": None, "array": array,
            "require": require, "exclude": exclude, "min_mapq": min_mapq, "mapq": mapq, "mapq_null": mapq is None,
            "mask": None if mask is None else np.asarray(mask, dtype=bool),
            "offsets": None if offsets is None else np.asarray(offsets, dtype=np.int64), "layout": "fixed" if offsets is not None else None,
            "nseg": 1 if offsets is None else len(offsets) - 1, "mode": mode,
            "selected_at": selected_at if kind in SELECTING + later_kinds else None,
            "high_at": high_at if kind in WIDE + LATER_WIDE else None}


def sel_bits_of(case):
    """1, 8 or None: the encoding of the case's selection"""
    if case["mask"] is None:
        return None
    return case["sel_bits"] if "sel_bits" in case else 1 if case["kind"] == "where_bitmap" else 8


def selection_image(case):
    """(uint8 image, offset in it of the byte the selection pointer names) of the case's selection in its encoding, between poison:
    bitmap_image for a bitmap; for a byte mask bytes_image of non-zero values other than 1 (1 + n % 255), element 0 at byte
    sel_offset from the pointer on.  The offset may be negative: a bitmap offset of 2^33 + k moves the pointer 2^30 bytes back."""
    if sel_bits_of(case) == 1:
        img, at, back = bitmap_image(case)
        return img, at - back
    img, at = bytes_image(case["mask"].astype(np.uint8) * np.uint8(1 + case["n"] % 255), case["sel_align"])
    assert case["sel_offset"] <= at
    return img, at - case["sel_offset"]
