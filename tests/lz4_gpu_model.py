"""CPU: a sequential model of what lz4_decode_wg does BEHIND the walker (flagstat_lz4_kernels.hip lz4wg_emit, flagstat_wgpipe.h
wgpipe_scan / wgpipe_copy), on top of the walker's restatement in tests/test_lz4_walker_model.py.  Per window record it decides
plain or batch form by the kernel's three conditions; the emitters leave markers and literal bytes; per 256-byte chunk the scanner
turns the markers into one source per byte -- the last marker at or before it, the carry through the 8 slots, roots against in-chunk
pointers, doubling rounds until nothing changes (at most 8) -- and the copier gathers from the 67,584-byte ring (the d + kNR wrap).
Its output must be the block's decoded bytes; beside them it yields a census of which paths a block went through.  The pieces run
in the one order the hand-over words allow a test to rely on: everything that starts below a chunk's end is emitted, then the chunk
is scanned and copied.  Deliberate errors (tests/test_lz4_writer_host.py) are parameters of decode(), never wrong code."""
import collections

import numpy as np

import test_lz4_walker_model as wm

LIT = 0x10000
DEFAULT = dict(span=384, plain_lit=4, rounds=8, emit_ring=67584)
RING, CHUNK, MARKS, CARRIES, PIECE = 67584, 256, 1024, 8, 64
_REL = np.arange(CHUNK, dtype=np.int64)


def parse(comp, p):
    """the sequence at token position p: (literals, where they start, offset, match length or 0, next token, literal-length bytes,
    match-length bytes)"""
    n = len(comp)
    tok = comp[p]
    ll, q, nl, nm = tok >> 4, p + 1, 0, 0
    if ll == 15:
        while True:
            e = comp[q]
            q, ll, nl = q + 1, ll + e, nl + 1
            if e != 255:
                break
    lit_at = q
    q += ll
    if q >= n:
        return ll, lit_at, 0, 0, n, nl, 0
    off = comp[q] | (comp[q + 1] << 8)
    q += 2
    ml = tok & 15
    if ml == 15:
        while True:
            e = comp[q]
            q, ml, nm = q + 1, ml + e, nm + 1
            if e != 255:
                break
    return ll, lit_at, off, ml + 4, q, nl, nm


def units(comp, tiles, census, span, plain_lit, emit_ring, detail):
    """what the emitters do, in order, as (first output position, marks [(position, value)], literal writes [(ring index, bytes)])"""
    op = 0
    iend = len(comp)

    def ring_put(writes, at, data):
        ri = at % emit_ring
        first = min(len(data), emit_ring - ri)      # (byte by byte in the kernel, the index wrapping at the ring's end)
        if first:
            writes.append((ri, bytes(data[:first])))
        if first < len(data):
            writes.append((0, bytes(data[first:])))

    def slow(p):
        nonlocal op
        ll, lit_at, off, ml, nxt, nl, nm = parse(comp, p)
        census["scalar sequences"] += 1
        if nl:
            census["stop: literal length bytes"] += 1
        if nl >= 8 or nm >= 8:
            census["stop: 8 or more length bytes (the walker drains the queue)"] += 1
        if nm and not nl and comp[nxt - nm] == 255:
            census["stop: match length byte 255"] += 1
        while ll > PIECE:
            w = []
            ring_put(w, op, comp[lit_at:lit_at + PIECE])
            census["literal pieces of 64"] += 1
            census["scalar records"] += 1
            yield op, [(op, LIT)], w
            op, lit_at, ll = op + PIECE, lit_at + PIECE, ll - PIECE
        if ml and nm and ll:            # (the literals go first: the length bytes may be many)
            w = []
            ring_put(w, op, comp[lit_at:lit_at + ll])
            census["scalar records"] += 1
            yield op, [(op, LIT)], w
            op, ll = op + ll, 0
        w, marks = [], []
        ring_put(w, op, comp[lit_at:lit_at + ll])
        if ll:
            marks.append((op, LIT))
        if ml:
            marks.append((op + ll, off))
        census["scalar records"] += 1
        yield op, marks, w
        op += ll + ml
        return nxt

    ip = 0
    for tip, members, adv, stopped in tiles:
        nvalid = adv // wm.SEG + (1 if stopped else 0)
        nseg = min(wm.SEGS, (iend - tip - wm.TAIL) // wm.SEG + 1)
        if not stopped and nvalid < nseg:
            census["tiles ended by an exit of 12 or more"] += 1
        if stopped and adv == 0:
            census["tiles that advance nothing"] += 1
        census["tiles"] += 1
        by_window = collections.defaultdict(list)
        for p in members:
            by_window[(p - tip) // 64].append(p)
        for wn in range((nvalid + 1) // 2):
            w0 = tip + 64 * wn
            seqs, rel = [], 0
            for p in by_window.get(wn, ()):
                ll, lit_at, off, ml, _, _, _ = parse(comp, p)
                seqs.append((p, ll, off, ml, rel))
                rel += ll + ml
            total = rel
            ri = lambda r: (op % emit_ring + r) - (emit_ring if op % emit_ring + r >= emit_ring else 0)  # noqa: E731
            long_lit = any(ll > plain_lit for _, ll, _, _, _ in seqs)
            ring_end = any(ll > 0 and ri(r) + 4 > emit_ring for _, ll, _, _, r in seqs)
            if ring_end:
                census["windows with a literal run at the ring's end"] += 1
            if detail is not None:
                detail[w0] = ("plain" if total <= span and not long_lit and not ring_end else "batch", total, op, ring_end)
            if total <= span and not long_lit and not ring_end:
                census["windows plain"] += 1
                marks, writes = [], []
                for p, ll, off, ml, r in seqs:
                    marks.append((op + r + ll, off))
                    if ll:
                        marks.append((op + r, LIT))
                        writes.append((ri(r), bytes(comp[p + 1:p + 5])))      # four bytes, whatever the run's length
                yield op, marks, writes
            else:
                census["windows batch"] += 1
                if total > span:
                    census["windows of more than one batch"] += 1
                done = 0
                while done < total:
                    now = [s for s in seqs if s[4] >= done and s[4] + s[1] + s[3] <= done + span]
                    assert now, "a batch with no sequence"
                    marks, writes = [], []
                    for p, ll, off, ml, r in now:
                        marks.append((op + r + ll, off))
                        if ll:
                            marks.append((op + r, LIT))
                            ring_put(writes, op + r, comp[p + 1:p + 1 + ll])
                    yield op + done, marks, writes
                    done = now[-1][4] + now[-1][1] + now[-1][3]
                    census["batches"] += 1
            op += total
        ip = tip + adv
        if stopped:
            ip = yield from slow(ip)
    while ip < iend:
        ip = yield from slow(ip)


def decode(comp, usize, tiles=None, span=384, plain_lit=4, rounds=8, emit_ring=RING, detail=None):
    """(decoded bytes, census) of one valid block as the pipeline's stages compute them"""
    comp = bytes(comp)
    if tiles is None:
        tiles = wm.check_stream(comp)
    census = collections.Counter()
    ring = np.zeros(RING + 8, dtype=np.uint8)
    mark = np.zeros(MARKS, dtype=np.int64)
    carry = [0] * CARRIES
    out = np.zeros(usize + CHUNK, dtype=np.uint8)
    gen = units(comp, tiles, census, span, plain_lit, emit_ring, detail)
    pending = next(gen, None)
    for kc in range((usize + CHUNK - 1) // CHUNK):
        c = kc * CHUNK
        need = min(c + CHUNK, usize)
        while pending is not None and pending[0] < need:
            start, marks, writes = pending
            for pos, val in marks:
                assert c <= pos < c + MARKS, ("a marker outside the slots the scanners have cleared", pos, c)
                assert mark[pos & (MARKS - 1)] == 0, ("two markers in one slot", pos)
                mark[pos & (MARKS - 1)] = val
            for ri, data in writes:
                ring[ri:ri + len(data)] = np.frombuffer(data, dtype=np.uint8)
            pending = next(gen, None)
        cidx = c % RING
        slot = c & (MARKS - 1)
        mk = mark[slot:slot + CHUNK].copy()
        mark[slot:slot + CHUNK] = 0
        has = mk != 0
        cin = carry[kc & (CARRIES - 1)] if kc else 0
        if has.any():
            last = np.maximum.accumulate(np.where(has, _REL, -1))
            offv = np.where(last >= 0, mk[np.maximum(last, 0)], cin) & 0xFFFF
            carry[(kc + 1) & (CARRIES - 1)] = int(mk[last[-1]])
            if cin & 0xFFFF and not has[0]:
                census["carries taken"] += 1
        else:
            offv = np.full(CHUNK, cin & 0xFFFF, dtype=np.int64)
            carry[(kc + 1) & (CARRIES - 1)] = cin
            if cin & 0xFFFF:
                census["carries taken"] += 1
                census["chunks that are all carry"] += 1
        t = _REL - offv
        ptr = np.where(t >= 0, t, _REL)
        d = t + cidx
        ext = np.where(d < 0, d + RING, d)
        if (ptr != _REL).any():
            r = 0
            for r in range(1, rounds + 1):
                n = ptr[ptr]
                changed = (n != ptr).any()
                ptr = n
                if not changed:
                    break
            census["chunks with in-chunk pointers, %d round%s" % (r, "" if r == 1 else "s")] += 1
            ext = ext[ptr]
        if (d < 0).any():
            census["chunks that read across the ring's end"] += 1
        ring[cidx:cidx + CHUNK] = ring[ext]
        out[c:c + CHUNK] = ring[cidx:cidx + CHUNK]
        census["chunks"] += 1
    while pending is not None and pending[0] >= usize and not any(data for _, data in pending[2]):
        pending = next(gen, None)           # (an empty literals-only sequence at the very end writes nothing)
    assert pending is None, "records left over"
    return out[:usize].tobytes(), census
