"""Test-only writer of LZ4 BLOCKS from a description (the LZ4 counterpart of tests/zstd_frame_writer.py): seq(literals, offset,
match_length) ... end(literals) gives (compressed, decoded, layout), layout = one Seq(ip, op, ll, off, ml) per sequence -- where its
token sits in the input, where its first output byte goes, its literal count, offset and match length (0, 0: the literals-only end).
Padding helpers put the next token at an exact input position and / or the next output byte at an exact output position with
window-form filler sequences of 3..18 input bytes; raw() appends bytes the writer does not interpret, for blocks that are invalid
on purpose.  Nothing loops per byte over a long match (a self-overlapping match is its period repeated), a 1 MB block is cheap.

FAMILIES places sequences on the boundaries of the GPU decoder's workgroup kernel (lz4_decode_wg: flagstat_lz4_kernels.hip,
flagstat_wgpipe.h) -- the numbers below, pinned against the source text by tests/test_lz4_writer_host.py -- and on those of the wave
kernel; REJECTED holds blocks with one defect each; random_block(rng) draws from the same vocabulary with the boundary numbers
over-weighted.  A case is (name, compressed, decoded, layout, claims); claims say what the case is named for and are proved from
the layout and the walker model by the host test: ("token_at", k, segment, position), ("match_at", k, r) / ("match_end", k, r): first
byte / end of sequence k's match = r mod 256, ("lit_covers", k, p): its literals cover output byte p, ("window_out", k, n): the
64-byte window that holds token k writes n bytes, ("stop", k): the tile hands token k to the scalar code."""
import collections
import random

# ---- the workgroup kernel's constants, mirrored once
SEG, TILE_SEGS, EXIT_TAB = 32, 64, 12         # walker: bytes per segment, segments per tile, entries of a segment's exit table
TAIL = 50                                     # a tile's last position leaves this many input bytes less 31 behind it
IN_PAD, IN_RING = 96, 6144                    # input ring and the mirror of its first bytes behind its end
LIT_PIECE, SPAN, CHUNK = 64, 384, 256         # scalar literal pieces; most output of a plain window; output bytes per scan step
MARK_SLOTS, FSRC_SLOTS = 1024, 512
OUT_RING, QUEUE = 67584, 16
PLAIN_LIT, ROUNDS, CARRIES, FLUSH = 4, 8, 8, 1024
WINDOW = 2 * SEG
TILE = SEG * TILE_SEGS
BLOCK_MAX = 1024000

Seq = collections.namedtuple("Seq", "ip op ll off ml")


def _lenbytes(v):
    out = bytearray()
    while v >= 255:
        out.append(255)
        v -= 255
    out.append(v)
    return bytes(out)


class Block:
    def __init__(self, seed=0):
        self.rng = random.Random(seed)
        self.comp, self.out, self.layout = bytearray(), bytearray(), []

    # ---- the description
    def _lits(self, literals):
        return self.rng.randbytes(literals) if isinstance(literals, int) else bytes(literals)

    def seq(self, literals, offset, match_length, ll_bytes=None, ml_bytes=None):
        """literals: bytes or a count; ll_bytes / ml_bytes: the length bytes behind nibble 15, when they shall not be the shortest form"""
        lits = self._lits(literals)
        ll, ml = len(lits), match_length
        assert ml >= 4 and 1 <= offset <= min(65535, len(self.out) + ll), (offset, len(self.out) + ll, ml)
        self.layout.append(Seq(len(self.comp), len(self.out), ll, offset, ml))
        self.comp.append((min(ll, 15) << 4) | min(ml - 4, 15))
        if ll >= 15:
            self.comp += _lenbytes(ll - 15) if ll_bytes is None else ll_bytes
        self.comp += lits
        self.out += lits
        self.comp += bytes((offset & 255, offset >> 8))
        if ml - 4 >= 15:
            self.comp += _lenbytes(ml - 19) if ml_bytes is None else ml_bytes
        self._copy(offset, ml)
        return len(self.layout) - 1

    def _copy(self, offset, ml):
        at = len(self.out) - offset
        if offset >= ml:
            self.out += self.out[at:at + ml]
        else:                                   # an overlapping match repeats with period `offset`
            pat = bytes(self.out[at:])
            self.out += (pat * (ml // offset + 1))[:ml]

    def end(self, literals):
        lits = self._lits(literals)
        self.layout.append(Seq(len(self.comp), len(self.out), len(lits), 0, 0))
        self.comp.append(min(len(lits), 15) << 4)
        if len(lits) >= 15:
            self.comp += _lenbytes(len(lits) - 15)
        self.comp += lits
        self.out += lits
        return self.finish()

    def raw(self, data):
        self.comp += bytes(data)
        return self

    def finish(self):
        return bytes(self.comp), bytes(self.out), list(self.layout)

    @property
    def ip(self):
        return len(self.comp)

    @property
    def op(self):
        return len(self.out)

    # ---- fillers: window-form sequences (all lengths in the token, or one match-length byte below 255), 3..18 input bytes
    def _off(self, near=False):
        have = len(self.out)
        assert have > 0, "a filler needs output to copy from: begin the block with literals"
        r = self.rng.random()
        if near or r < 0.3:
            return self.rng.randint(1, min(have, 40))
        return self.rng.randint(1, min(have, 65535 if r < 0.6 else 3000))

    def filler(self, n_in, n_out):
        """one filler of n_in input bytes (3..18) that writes n_out bytes"""
        assert 3 <= n_in <= 18 and _piece_min(n_in) <= n_out <= _piece_max(n_in), (n_in, n_out)
        if n_out <= n_in + 15 and n_in < 18:                    # no match-length byte: ll = n_in - 3 (at most 14), ml = n_out - ll
            ll = n_in - 3
            # (n_out = n_in + 15 is ml 18 here, or ml 19 with a length byte 0 and one literal less: take the former)
        else:
            ll = n_in - 4
        return self.seq(ll, self._off(), n_out - ll)

    def pad(self, ip=None, op=None, maxlen=18, fat=False):
        """fillers until the next token sits at input position ip and / or the next output byte at output position op (fat: as few
        fillers as maxlen allows, where only the distance matters)"""
        rng = self.rng
        if ip is None and op is None:
            return self
        if ip is None:
            ro = op - self.op
            assert ro == 0 or ro >= 4, ("cannot pad the output by", ro)
            while ro:
                ml = rng.randint(4, 18)
                if ro - ml in (1, 2, 3) or ml > ro:
                    ml = ro if ro <= 18 else 4 + (ro - 4) % 4
                    if ro - ml in (1, 2, 3):
                        ml = 4
                self.seq(0, self._off(), ml)
                ro -= ml
            return self
        ri = ip - self.ip
        assert ri == 0 or ri >= 3, ("cannot pad the input by", ri)
        if op is None:
            while ri:
                n = min(maxlen if fat and rng.random() < 0.9 else rng.choice([3, 3, 3, 3, 4, 5, 6, 8, 11, 14, 18]), maxlen, ri)
                if ri - n in (1, 2):
                    n = ri if ri <= maxlen else 3
                    if ri - n in (1, 2):
                        n = 4
                lo, hi = _piece_min(n), min(_piece_max(n), n + 5 if fat else n + 15 if rng.random() < 0.9 else n + 60)
                self.filler(n, rng.randint(lo, hi))
                ri -= n
            return self
        ro = op - self.op
        assert _min_out(ri) <= ro <= _max_out(ri), ("cannot pad", ri, "input bytes to", ro, "output bytes")
        while ri:
            cand = [n for n in range(3, min(maxlen, 18, ri) + 1) if ri - n not in (1, 2)]
            rng.shuffle(cand)
            cand.sort(key=lambda n: n != 3 and rng.random() < 0.7)  # mostly bare fillers first
            for n in cand:
                lo = max(_piece_min(n), ro - _max_out(ri - n))
                hi = min(_piece_max(n), ro - _min_out(ri - n))
                if lo <= hi:
                    want = rng.randint(n + 1, n + 15)           # what a filler writes when nothing forces it
                    # (spread what is missing over the fillers to come, so that the last ones need no 270-byte matches)
                    left = max(1, (ri + 3) // 4)
                    want = max(want, min(hi, (ro + left - 1) // left)) if ro > 18 * left else want
                    o = min(max(want, lo), hi)
                    self.filler(n, o)
                    ri, ro = ri - n, ro - o
                    break
            else:
                raise AssertionError(("pad: no filler fits", ri, ro))
        assert ro == 0
        return self


def reach(b, op, extra_in=0):
    """fillers until the next output byte is `op` (any number of input bytes, `extra_in` more than needed at least)"""
    ro = op - b.op
    if ro:
        assert ro >= 4, ("cannot pad the output by", ro)
        b.pad(ip=b.ip + 3 * max(1, -(-ro // 14)) + extra_in, op=op)
    return b


def sync(b, at):
    """a sequence for the scalar code (20 literals or a few more: 24 input bytes) that ends at input position `at`: whatever the tiles before did,
    the next tile starts at `at`"""
    n = next(n for n in range(24, 60) if at - n - b.ip == 0 or at - n - b.ip >= 3)
    b.pad(ip=at - n, maxlen=11)
    k = b.seq(n - 4, b._off(), 4)
    assert b.ip == at
    return k


def _piece_min(n):
    return n + 1 if n < 18 else 33   # ll = n - 3, ml = 4; 18 input bytes: 14 literals and a match-length byte, ml 19


def _piece_max(n):
    return 18 if n == 3 else n - 4 + 273


def _min_out(n):
    return 0 if n == 0 else (1 << 40 if n < 3 else n + (n + 16) // 17)


def _max_out(n):
    if n < 3:
        return 0 if n == 0 else -1
    q, r = divmod(n, 4)
    return 273 * q + (0, 1, 2, 18)[r]


def start(seed, lits=8, ml=8):
    """a block that begins with a window-form sequence: `lits` literals and a match into them"""
    b = Block(seed)
    b.seq(lits, b.rng.randint(1, lits), ml)
    return b


def case(name, b, tail, claims=()):
    comp, dec, layout = b.end(tail)
    assert len(dec) <= BLOCK_MAX, (name, len(dec))
    return (name, comp, dec, layout, list(claims))


# ------------------------------------------------------------------------------------------------------------- families
def _sized(n_in, rng):
    """(literals, match length) of a window-form sequence of n_in input bytes: with a match-length byte where it fits, now and then"""
    if n_in == 18 or (n_in >= 4 and rng.random() < 0.4):      # (18: 14 literals and the byte, there is no other way)
        return n_in - 4, 19 + rng.choice([0, 1, 100, 254])
    return n_in - 3, rng.randint(4, 18)


def fam_segments():
    out = []
    # every input length 3..18 at every position 0..31 of segments 62 and 63 of a full tile (and of segments 0 and 1 of the same
    # tile, where the sequence does not enter the next segment at 12 or more, which ends the tile): one block per length, tile
    # behind tile.  The fillers are short enough that no entry reaches 12, so a tile ends where its 64th segment does -- the next
    # one starts on the first token from there -- or behind a placed sequence that enters the next segment at 12 or more.
    for n in range(3, 19):
        b = start(1000 + n)
        claims = []
        t0 = b.ip + 64
        sync(b, t0)
        for pos in range(32):
            for segs in [(0, 1, 62, 63)] if pos + n < SEG + EXIT_TAB else [(62,), (63,)]:
                for seg in segs:
                    if seg == 0 and pos in (1, 2):        # (a tile starts on a token: none can sit 1 or 2 bytes behind it)
                        continue
                    b.pad(ip=t0 + SEG * seg + pos, maxlen=11, fat=True)
                    ll, ml = _sized(n, b.rng)
                    claims.append(("token_at", b.seq(ll, b._off(), ml), seg, pos))
                if pos + n < SEG + EXIT_TAB and b.ip != t0 + TILE:
                    if b.ip <= t0 + TILE - 3:
                        b.pad(ip=t0 + TILE, maxlen=11, fat=True)
                    elif b.ip < t0 + TILE:
                        b.seq(0, b._off(), 5)
                t0 = b.ip
        b.pad(ip=b.ip + 60, maxlen=11, fat=True)
        out.append(case("segments: %d input bytes at every position of segments 62 and 63 (0 and 1) of full tiles" % n, b, 70, claims))
    # ... and at every position of segments 0 and 1 of a short last tile: the block ends 3 segments into it
    for n in range(3, 19):
        for pos in range(32):
            for segs in [(0, 1)] if pos + n < SEG + EXIT_TAB else [(0,), (1,)]:
                if segs == (0,) and pos in (1, 2):
                    continue
                b = start(5000 + 100 * n + pos + segs[0])
                t0 = 64
                sync(b, t0)
                claims = []
                for seg in segs:
                    if seg == 0 and pos in (1, 2):
                        continue
                    b.pad(ip=t0 + SEG * seg + pos, maxlen=11)
                    ll, ml = _sized(n, b.rng)
                    k = b.seq(ll, b._off(), ml)
                    claims += [("token_at", k, seg, pos), ("short_tile", k)]
                b.pad(ip=max(t0 + 3 * SEG + 3, b.ip + 3), maxlen=11)
                out.append(case("segments: %d input bytes at position %d of segment%s of a short last tile" % (n, pos, " %d" % segs[0] if len(segs) == 1 else "s 0 and 1"),
                                b, 40, claims))
    # entries into the next segment of 0..17: 12..17 end the tile with the segment before
    for seg in (0, 30, 62):
        for entry in range(18):
            for n in sorted({max(3, entry + 1), 18}):
                if entry > n - 1:
                    continue
                b = start(7000 + 100 * seg + entry + n)
                at = SEG * (seg + 1) + entry - n      # the sequence ends `entry` bytes into the next segment
                b.pad(ip=at, maxlen=11)
                ll, ml = _sized(n, b.rng)
                b.seq(ll, b._off(), ml)
                k2 = b.seq(0, b._off(), 9)
                b.pad(ip=b.ip + 120, maxlen=11)
                claim = ("token_at", k2, seg + 1, entry) if entry < EXIT_TAB else ("tile_ended_by_exit", k2, seg, entry)
                out.append(case("segments: entry %d into segment %d behind %d input bytes" % (entry, seg + 1, n), b, 30, [claim]))
    # tiles at input-ring phases so that a window straddles byte 6,144 (the mirror, the emitters' wi >= kWgInw wrap)
    for phase in (IN_RING - 1, IN_RING - 3, IN_RING - 17, IN_RING - 31, IN_RING - 63, IN_RING - 64, IN_RING - 95, IN_RING - 96):
        for lap in (1, 2):
            b = start(9000 + phase + lap)
            at = IN_RING * lap - (IN_RING - phase)
            sync(b, at - at % SEG - 5 * SEG)       # (a tile from a few segments before: the windows go over the ring's end)
            b.pad(ip=at, maxlen=18)
            ks = [b.seq(ll, b._off(), ml) for ll, ml in ((14, 18), (0, 4), (14, 19 + 254), (3, 7), (13, 5), (14, 4), (0, 18), (5, 30))]
            b.pad(ip=b.ip + 300)
            out.append(case("segments: sequences from input byte %d (ring byte %d, lap %d)" % (at, phase % IN_RING, lap), b, 20,
                            [("in_near", ks[0], IN_RING * lap, 96)]))
    return out


def fam_stops():
    out = []
    lit_forms = [("ext 0", 15, None), ("ext 1", 16, None), ("ext 254", 269, None), ("ext 255+0", 270, None),
                 ("255 x 7", 15 + 255 * 7 + 3, None), ("255 x 8", 15 + 255 * 8 + 3, None)]
    ml_forms = [("first byte 0", 19, False), ("first byte 254", 19 + 254, False), ("255+0", 19 + 255, True),
                ("255 x 7", 19 + 255 * 7 + 9, True), ("255 x 8", 19 + 255 * 8 + 9, True)]
    places = [("at position 0 of segment 0", TILE), ("mid-tile", TILE + SEG * 20 + 7), ("in the last segment", TILE + SEG * 63 + 9)]
    seed = 0
    for pname, at in places:
        for fname, ll, _ in lit_forms:
            seed += 1
            b = start(20000 + seed)
            sync(b, TILE)
            b.pad(ip=at, maxlen=11)
            k = b.seq(ll, b._off(), 6)
            b.pad(ip=b.ip + 400)
            out.append(case("stops: literal length %s, %s" % (fname, pname), b, 33, [("stop_at", k, (at - TILE) // SEG, at % SEG)]))
        for fname, ml, stops in ml_forms:
            seed += 1
            b = start(21000 + seed)
            sync(b, TILE)
            b.pad(ip=at, maxlen=11)
            k = b.seq(2, b._off(), ml)
            b.pad(ip=b.ip + 400)
            out.append(case("stops: match length %s, %s" % (fname, pname), b, 33,
                            [("stop_at" if stops else "token_at", k, (at - TILE) // SEG, at % SEG)]))
    for gap in (3, 9, 20):      # two in one segment
        b = start(22000 + gap)
        at = TILE + SEG * 5
        sync(b, TILE)
        b.pad(ip=at, maxlen=11)
        k1 = b.seq(0, b._off(), 19 + 255 + 30)        # 5 input bytes
        if gap > 5:
            b.pad(ip=at + gap)
        k2 = b.seq(15, b._off(), 4)
        b.pad(ip=b.ip + 400)
        out.append(case("stops: two in one segment, %d apart" % (b.layout[k2].ip - at), b, 12, [("stop", k1), ("stop", k2)]))
    return out


def fam_literals():
    out = []
    b = start(30000)
    ks = []
    for ll in range(15):            # window form: 0..4 plain, 5..14 batch
        b.pad(op=b.op + 900)        # (bare fillers, about 250 input bytes: the run is the only one of its window)
        ks.append(b.seq(ll, b._off(), 5 + ll))
    b.pad(op=b.op + 900)
    out.append(case("literals: window-form runs of 0..14", b, 15, [("window_lit", k, ll) for ll, k in enumerate(ks)]))
    # runs that end on, straddle and begin at ring byte 67,583, in the first lap and one lap later
    edge = OUT_RING - 1
    for lap in (0, 1):
        for ll in (1, 2, 4, 5, 9, 14):
            for first in sorted({edge - ll + 1, edge - ll // 2, edge}):      # first literal byte, as a ring byte
                b = start(31000 + 100 * ll + lap + first % 97)
                tgt = lap * OUT_RING + first
                if lap:
                    b.seq(0, 1, OUT_RING - 20000)                           # (a lap of output is cheap: long matches)
                    b.pad(ip=b.ip + 200)
                b.seq(3, 2, tgt - 700 - b.op)
                b.pad(ip=b.ip + 64, maxlen=11)
                reach(b, tgt)
                k = b.seq(ll, b._off(), 7)
                b.pad(ip=b.ip + 200)
                out.append(case("literals: run of %d from ring byte %d, lap %d" % (ll, first, lap), b, 19, [("lit_covers", k, lap * OUT_RING + edge)]))
    b = start(32000)
    ks = []
    for ll in (15, 16, 63, 64, 65, 127, 128, 129, 270, 6143, 6144, 6145, 12289):
        b.pad(ip=b.ip + 90)
        ks.append(b.seq(ll, b._off(), 11))
    out.append(case("literals: scalar-path runs of 15 .. 12,289", b, 64, [("stop", k) for k in ks]))
    out.append(case("literals: one run of 1,024,000 bytes", Block(32001), BLOCK_MAX, [("literal_only", 0)]))
    return out


def _window_of(b, seqs, at):
    """sequences (ll, off, ml) from input position `at` on (a multiple of 64 in tile 0)"""
    b.pad(ip=at, maxlen=11)
    return [b.seq(ll, off or b._off(), ml) for ll, off, ml in seqs]


def fam_span():
    out = []
    for total in (383, 384, 385):
        for lit in (0, 4):
            b = start(40000 + total + lit)
            # sixteen 4-byte sequences fill a window exactly; their output adds up to `total`
            mls = [19 + 4] * 16
            mls[15] = total - sum(mls[:15]) - (lit and 4)
            seqs = [(0, 0, m) for m in mls]
            if lit:                                   # ... with one run of 4 literals (still the plain form): 8 + 14 x 4 = 64 input bytes
                seqs = [(4, 0, mls[15] + 23)] + [(0, 0, 23)] * 14
            ks = _window_of(b, seqs, 10 * WINDOW)
            b.pad(ip=b.ip + 300)
            out.append(case("span: a window of %d output bytes, %d literals" % (total, lit), b, 25, [("window_out", ks[0], total)]))
    big = [(0, 0, 19 + 254)] * 16
    b = start(41000)
    ks = _window_of(b, big, 4 * WINDOW)
    b.pad(ip=b.ip + 300)
    out.append(case("span: the most output a window can have", b, 25, [("window_out", ks[0], 16 * 273)]))
    for offs in (1, 7, 300, 5000):
        b = start(41001 + offs)
        b.seq(0, 1, 6000)
        sync(b, 2 * TILE)
        ks = []
        for w in range(32):
            ks.append(_window_of(b, [(0, offs, 19 + 254)] * 16, 2 * TILE + w * WINDOW)[0])
        b.pad(ip=b.ip + 300)
        out.append(case("span: 32 full windows back to back, offset %d" % offs, b, 25, [("window_out", k, 16 * 273) for k in ks]))
    return out


def fam_chunks():
    out = []
    seed = 50000
    for k256 in (3, 9, 263, 264, 265):              # (264 chunks are one lap of the ring)
        for d in (-1, 0, 1):
            for ends in (False, True):
                seed += 1
                b = start(seed)
                if k256 > 100:
                    b.seq(0, 2, 66000)
                tgt = CHUNK * k256 + d
                ml = b.rng.choice([4, 9, 18, 100])
                st = tgt - ml if ends else tgt
                b.pad(ip=b.ip + 60)
                reach(b, st, 30)
                k = b.seq(0, b._off(), ml)
                b.pad(ip=b.ip + 200)
                out.append(case("chunks: a match that %s at output byte %d" % ("ends" if ends else "starts", tgt), b, 14,
                                [("match_end" if ends else "match_at", k, d % CHUNK)]))
    for off in (1, 2, 3, 4, 5, 7):
        b = start(51000 + off, lits=8)
        ks = []
        for ml in (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 70000):
            b.pad(ip=b.ip + 40)
            ks.append(b.seq(b.rng.choice([0, 1, 3]), off, ml))
        out.append(case("chunks: offset %d, lengths 255 .. 70,000" % off, b, 14, [("period", k, off) for k in ks]))
    for depth in (2, 3, 8, 17, 60):                 # match i copies from the output of match i - 1, all in one chunk
        for base in (0, 1):
            b = start(52000 + depth + base)
            b.pad(ip=b.ip + 100)
            reach(b, CHUNK * 9 + base, 9)
            ks = [b.seq(0, b.rng.randint(300, 2000), 4)]
            for i in range(1, depth):
                ks.append(b.seq(0, 4, 4) if i % 3 else b.seq(0, 3, 4))
            b.pad(ip=b.ip + 200)
            out.append(case("chunks: a chain of depth %d from byte %d of a chunk" % (depth, base), b, 16, [("chain", ks[0], ks[-1], depth)]))
    for dist in (5, 100, 255):                      # offsets = the distance to the chunk's first byte - 1, + 0, + 1: pointer against root
        for d in (-1, 0, 1):
            b = start(53000 + dist + d)
            b.pad(ip=b.ip + 100)
            tgt = CHUNK * 7 + dist
            reach(b, tgt, 9)
            k = b.seq(0, dist + d, 12)
            b.pad(ip=b.ip + 200)
            out.append(case("chunks: offset %d at byte %d of a chunk" % (dist + d, dist), b, 16, [("match_at", k, dist)]))
    for off in (65535, 65534, 65280):
        for around in (OUT_RING, 2 * OUT_RING, 1000000):
            for d in (-3, 0, 2, 300) if around < 1000000 else (off % 7 - 3,):
                b = start(54000 + off % 100 + around % 1000 + d)
                b.seq(5, 7, 30000)
                b.pad(ip=b.ip + 500)
                b.seq(0, 1, around - 1200 - b.op)
                b.pad(ip=b.ip + 100)
                reach(b, around + d, 9)
                k = b.seq(0, off, b.rng.choice([4, 40, 700]))
                b.pad(ip=b.ip + 200)
                out.append(case("chunks: offset %d at output byte %d" % (off, around + d), b, 16, [("match_pos", k, around + d)]))
    return out


def fam_tails():
    out = []
    for size in list(range(1, 14)) + [255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 67583, 67584, 67585, 135167, 135168, 135169]:
        b = Block(60000 + size)
        if size <= 13:
            out.append(case("tails: %d decoded bytes, literals only" % size, b, size, [("size", size)]))
            if size == 13:
                b = Block(60100)
                b.seq(1, 1, 4)                        # the smallest block with a match: 1 + 4, then 8 literals... 13 bytes
                out.append(case("tails: 13 decoded bytes with a match", b, 8, [("size", 13)]))
            continue
        b.seq(6, 3, 8)
        if size > 60000:
            b.seq(2, 11, size - 3000)
        tail = 5 + size % 9
        reach(b, size - tail)
        out.append(case("tails: %d decoded bytes" % size, b, tail, [("size", size)]))
    for csize in (49, 50, 51, 61, 62, 63, 81, 82, 83, 93, 94, 95, 1024, 2048, 6144, 12288):
        b = start(61000 + csize)
        tail = 7
        b.pad(ip=csize - 1 - tail, maxlen=11)
        out.append(case("tails: %d compressed bytes" % csize, b, tail, [("csize", csize)]))
    return out


def fam_ends():
    out = []
    for ml in (4, 5, 6, 7):            # last match exactly 12 bytes before the end: final run 12 - ml ... but never below 5
        b = start(70000 + ml)
        b.pad(ip=b.ip + 100)
        b.seq(0, b._off(), ml)
        out.append(case("ends: last match of %d exactly 12 bytes before the end" % ml, b, 12 - ml, [("last_match_from_end", 12)]))
    for tail in (5, 6, 11, 12, 13):
        for ll in (0, 3):
            b = start(70100 + tail + ll)
            b.pad(ip=b.ip + 100)
            b.seq(ll, b._off(), 18)
            out.append(case("ends: last literals exactly %d, behind a match with %d literals" % (tail, ll), b, tail, [("last_literals", tail)]))
    # the last match as a tile's last member, and behind it.  A tile from input byte 0 reaches position iend - 19 when
    # iend = 50 mod 32: the tile then notes where its last member's match starts, for the scalar code that sees the block's end.
    at = SEG * 12 + 31
    for n, tail in ((18, 5), (18, 6), (18, 11), (18, 12), (17, 5), (3, 14), (3, 15), (3, 5), (3, 8)):
        b = start(70200 + tail + n)
        b.pad(ip=at, maxlen=11)
        ll, ml = (n - 3, 9) if n < 18 else (14, 19 + 7)
        k = b.seq(ll, b._off(), ml)
        iend = b.ip + 1 + tail + (tail >= 15)
        member = at <= SEG * ((iend - TAIL) // SEG) + SEG - 1
        out.append(case("ends: a last match of %d input bytes at %d before %d literals" % (n, at, tail), b, tail,
                        [("last_literals", tail), ("token_at", k, 12, 31) if member else ("scalar", k)]))
    for n in range(0, 51):
        out.append(case("ends: %d literals and nothing else" % n, Block(70300 + n), n, [("literal_only", 0)]))
    return out


def fam_wave():
    out = []
    for off in (8127, 8128, 8129, 8191, 8192, 8193, 16319, 16320, 16321):
        for phase in (0, 8190, 4095):
            b = start(80000 + off + phase)
            b.seq(3, 5, 17000)
            b.pad(ip=b.ip + 100)
            tgt = 8192 * 3 + phase
            b.seq(0, 7, tgt - 900 - b.op)
            reach(b, tgt, 9)
            ks = [b.seq(0, off, ml) for ml in (4, 16, 17, 18)] + [b.seq(2, off, 70)]
            b.pad(ip=b.ip + 200)
            out.append(case("wave: offset %d at ring phase %d" % (off, phase), b, 12, [("match_pos", ks[0], tgt)]))
    for n in (15, 16, 17, 33):
        b = start(81000 + n)
        b.seq(4, 2, 300)
        b.seq(1, 9, 5)
        for i in range(n):
            b.seq(0, b.rng.randint(20, 300), b.rng.randint(4, 18))
        b.seq(1, 3, 5)
        out.append(case("wave: %d bare sequences in a row" % n, b, 12, [("bare_run", n)]))
    for ml in (4, 16):              # four sequences of one pass that read each other's output
        b = start(82000 + ml)
        b.seq(4, 2, 300)
        for rep in range(6):
            b.seq(1, 9, 5)
            b.seq(0, 100, ml)
            for i in range(3):
                b.seq(0, ml - rep % 3 if ml - rep % 3 > 0 else 1, ml)
        out.append(case("wave: sequences of one pass that read each other's output, %d bytes" % ml, b, 12, [("bare_run", 4)]))
    for q in (2048, 4096, 6144, 8192, 10240):
        for d in (-1, 0, 1):
            b = start(83000 + q + d)
            b.pad(ip=b.ip + 100)
            reach(b, q + d - 9, 9)
            k = b.seq(0, b._off(), 9)
            k2 = b.seq(3, b._off(), 18)
            b.pad(ip=b.ip + 100)
            out.append(case("wave: output crosses flush quarter %d by %d" % (q, d), b, 12, [("match_end", k, (q + d) % CHUNK)]))
    return out


FAMILIES = collections.OrderedDict([("segments", fam_segments), ("stops", fam_stops), ("literals", fam_literals), ("span", fam_span),
                                    ("chunks", fam_chunks), ("tails", fam_tails), ("ends", fam_ends), ("wave", fam_wave)])


# ------------------------------------------------------------------------------------------------------------- rejected
END_DEFECTS = ("ends in a match", "last literals below 5", "last match within 12 of the end")


def rejected():
    """(name, compressed, declared size): one defect each; liblz4's LZ4_decompress_safe refuses every one"""
    out = []

    def good(seed, n=600):
        b = start(seed)
        b.pad(ip=n)
        return b

    b = good(1)
    b.raw(bytes([0x02, 0, 0]))
    b.out += b"\0" * 6
    out.append(("offset 0 in a window", b, 20))
    b = good(2)
    b.raw(bytes([0xF0, 5]) + bytes(20) + bytes([0, 0]))
    b.out += bytes(24)
    out.append(("offset 0 in the scalar path", b, 20))
    for where, n in (("in a window", 600), ("in a window of the second tile", 2600)):
        b = good(3, n)
        o = b.op + 1
        if o <= 65535:
            b.raw(bytes([0x03, o & 255, o >> 8]))
            b.out += bytes(7)
            out.append(("an offset one beyond the output, " + where, b, 20))
    b = good(4)
    o = b.op + 20 + 1
    b.raw(bytes([0xF0, 5]) + bytes(20) + bytes([o & 255, o >> 8]))
    b.out += bytes(24)
    out.append(("an offset one beyond the output, in the scalar path", b, 20))
    b = Block(5)
    b.raw(bytes([0x40, 1, 2, 3, 4, 5, 0]))
    b.out += bytes(8)
    out.append(("an offset one beyond the output, as the block's first match", b, 30))
    res = [(name, *_finish_bad(b, tail)) for name, b, tail in out]
    # length bytes that run past the input
    b = good(6)
    res.append(("literal-length bytes run past the input", bytes(b.comp) + bytes([0xF0, 255, 255, 255]), b.op + 900))
    b = good(7)
    res.append(("match-length bytes run past the input", bytes(b.comp) + bytes([0x0F, 1, 0, 255, 255]), b.op + 900))
    # a literal run / a match that passes the declared size by one; a declared size one more and one less
    b = good(8)
    comp, dec, _ = b.end(20)
    res.append(("a literal run passes the declared size by one", comp, len(dec) - 1))
    res.append(("a declared size one more than the block decodes to", comp, len(dec) + 1))
    b = good(9)
    b.seq(0, 5, 100)
    at = b.op
    comp, dec, _ = b.end(6)
    res.append(("a match passes the declared size by one", comp, at - 1))
    res.append(("a declared size one less than the block decodes to", comp, len(dec) - 1))
    b = good(10, 300)
    b.seq(20, 9, 30)
    b.pad(ip=b.ip + 30)
    comp, dec, _ = b.end(9)
    for cut in range(1, 21):
        res.append(("cut %d bytes before the end" % cut, comp[:-cut], len(dec)))
    res += end_defects()
    return res


def _finish_bad(b, tail):
    comp, dec, _ = b.end(tail)
    return comp, len(dec)


def end_defects():
    """the three end-of-block shapes liblz4 refuses, in short and in long blocks (the last tile's tail rule)"""
    res = []
    at = SEG * 12 + 31          # (the last match as a tile's last member: fam_ends has the valid neighbours)
    for what, n_in, ml, tail in ((1, 18, 26, 4), (1, 18, 26, 0), (1, 3, 9, 4), (2, 17, 4, 7), (2, 17, 6, 5), (2, 3, 4, 7), (2, 3, 5, 6)):
        b = start(80 + n_in + ml + tail)
        b.pad(ip=at, maxlen=11)
        b.seq(n_in - (3 if ml < 19 else 4), b._off(), ml)
        comp, dec, _ = b.end(tail)
        res.append(("%s (match %d + tail %d, the last member of a tile, %d input bytes)" % (END_DEFECTS[what], ml, tail, n_in), comp, len(dec)))
    for n in (0, 300, 3000):
        for ml in (4, 18, 300):
            b = start(90 + n + ml)
            if n:
                b.pad(ip=n)
            b.seq(2, b._off(), ml)
            res.append(("%s (match of %d, %d input bytes)" % (END_DEFECTS[0], ml, b.ip), bytes(b.comp), b.op))
        for tail in (0, 1, 4):
            for n_in in (3, 18):
                b = start(95 + n + tail + n_in)
                if n:
                    b.pad(ip=n)
                b.seq(n_in - 3, b._off(), 18)
                comp, dec, _ = b.end(tail)
                res.append(("%s (%d, behind %d input bytes, %d in all)" % (END_DEFECTS[1], tail, n_in, len(comp)), comp, len(dec)))
        for ml, tail in ((4, 7), (6, 5), (5, 6), (4, 5)):
            for n_in in (3, 17):
                b = start(99 + n + ml + tail + n_in)
                if n:
                    b.pad(ip=n)
                b.seq(n_in - 3, b._off(), ml)
                comp, dec, _ = b.end(tail)
                res.append(("%s (match %d + tail %d, behind %d input bytes, %d in all)" % (END_DEFECTS[2], ml, tail, n_in, len(comp)), comp, len(dec)))
    return res


# ---------------------------------------------------------------------------------------------------------- random_block
_LL = [0] * 8 + [1, 2, 3, 4, 5, 6, 13, 14, 15, 16, 63, 64, 65, 127, 128, 129, 269, 270, 271]
_ML = [4, 5, 7, 17, 18, 19, 20, 19 + 254, 19 + 255, 255, 256, 257, 383, 384, 385, 511, 512, 513, 1023, 1024, 1025]
_OFF = [1, 2, 3, 4, 5, 7, 8, 16, 63, 64, 65, 255, 256, 257, 8127, 8128, 8129, 8191, 8192, 8193, 16320, 65280, 65534, 65535]


def random_block(rng, big=True):
    """a valid block from the families' vocabulary: (compressed, decoded, layout); big=False: at most some 30 KB of output"""
    b = start(rng.getrandbits(32), lits=rng.choice([1, 4, 8, 14]), ml=rng.choice([4, 8, 40]))
    target = rng.choice([60, 300, 2100, 7000, 70000, 140000, 300000])
    if not big and target > 7000:
        target = 20000
    if target >= 20000:
        ll = rng.choice([0, 3])
        b.seq(ll, min(rng.choice([1, 2, 3, 5, 7]), b.op + ll), target - rng.choice([100, 3000, 9000]))
    steps = 0
    while b.op < target and steps < 60:
        steps += 1
        r = rng.random()
        if r < 0.35:        # a token at a boundary position of the input
            at = b.ip + rng.choice([3, 30, 64, 200])
            at += rng.choice([0, -1, 1, 31, 32]) - at % rng.choice([SEG, WINDOW, TILE, 1024, IN_RING])
            if at >= b.ip + 3:
                b.pad(ip=at, maxlen=rng.choice([11, 18]))
        elif r < 0.6:       # the next match at a boundary position of the output
            at = b.op + rng.choice([40, 300, 1500])
            at += rng.choice([0, -1, 1]) - at % rng.choice([CHUNK, FLUSH, 2048, SPAN])
            if at >= b.op + 4:
                b.pad(op=at)
        ll = rng.choice(_LL) if rng.random() < 0.5 else rng.randint(0, 14)
        ml = rng.choice(_ML) if rng.random() < 0.4 else rng.randint(4, 30)
        off = rng.choice(_OFF) if rng.random() < 0.6 else rng.randint(1, 65535)
        b.seq(ll, max(1, min(off, b.op + ll, 65535)), ml)
    return b.end(max(rng.choice([5, 6, 12, 13, 15, 40, 300]), 12 - b.layout[-1].ml))
