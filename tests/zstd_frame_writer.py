"""A Zstandard frame WRITER for tests (RFC 8878), test infrastructure only: an encoder of a given shape, not a compressor.

The caller says what every block looks like -- its kind, the form of its literals section, the Huffman tree and how it is
described, the mode and the normalised counts of each of the three sequence tables, the (literal length, match length,
offset) triples themselves -- and the writer serialises exactly that, with the codes, extra bits, FSE states and backward
bit streams the format prescribes.  It also returns the bytes the frame must decode to, computed from the same description
(as test_gpu_blockfile._synthetic_lz4_block returns (comp, dec)).  Every frame the GPU decoder's tests had before came out
of libzstd's compressor; this one writes valid Zstandard no compressor would: chosen lengths and distances, every size
format, every table mode at every accuracy log, Huffman trees of every depth.

Written from RFC 8878 and from tests/zstd_model.py, whose tables and table builders it imports; the inverse of that model's
readers.  tests/test_zstd_writer_host.py holds it against libzstd's ZSTD_decompress: every frame it can make must decode
there to the bytes it says."""
import bisect
import functools
import random
import struct

import zstd_model as zm

SKIPPABLE_MAGIC = 0x184D2A50
BLOCK_MAX = zm.BLOCK_MAX
_M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------------------- XXH64
def xxh64(data, seed=0):
    """XXH64 (the frame's content checksum is its low four bytes); plain Python, from the published algorithm"""
    p1, p2, p3, p4, p5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261

    def rotl(x, r):
        return ((x << r) | (x >> (64 - r))) & _M64

    def rnd(acc, inp):
        return (rotl((acc + inp * p2) & _M64, 31) * p1) & _M64

    def merge(acc, val):
        return ((acc ^ rnd(0, val)) * p1 + p4) & _M64

    data = bytes(data)
    n, p = len(data), 0
    if n >= 32:
        v1, v2, v3, v4 = (seed + p1 + p2) & _M64, (seed + p2) & _M64, seed, (seed - p1) & _M64
        while p + 32 <= n:
            a, b, c, d = struct.unpack_from("<QQQQ", data, p)
            v1, v2, v3, v4 = rnd(v1, a), rnd(v2, b), rnd(v3, c), rnd(v4, d)
            p += 32
        h = (rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18)) & _M64
        for v in (v1, v2, v3, v4):
            h = merge(h, v)
    else:
        h = (seed + p5) & _M64
    h = (h + n) & _M64
    while p + 8 <= n:
        h ^= rnd(0, struct.unpack_from("<Q", data, p)[0])
        h = (rotl(h, 27) * p1 + p4) & _M64
        p += 8
    if p + 4 <= n:
        h ^= (struct.unpack_from("<I", data, p)[0] * p1) & _M64
        h = (rotl(h, 23) * p2 + p3) & _M64
        p += 4
    while p < n:
        h ^= (data[p] * p5) & _M64
        h = (rotl(h, 11) * p1) & _M64
        p += 1
    h ^= h >> 33
    h = (h * p2) & _M64
    h ^= h >> 29
    h = (h * p3) & _M64
    h ^= h >> 32
    return h


# ------------------------------------------------------------------------------------------------------- bit streams
def back_stream(fields):
    """fields: (value, nbits) in the order the DECODER reads them -> the backward bit stream with its closing 1 bit"""
    parts = []
    for v, n in fields:
        assert 0 <= v < (1 << n) or (n == 0 and v == 0), (v, n)
        if n:
            parts.append(format(v, "0%db" % n))
    s = "".join(parts)
    return int("1" + s, 2).to_bytes((len(s) + 8) // 8, "little")


def write_fse_counts(counts, log):
    """the inverse of zstd_model.read_fse_counts: normalised counts (-1: "less than one") -> table description bytes"""
    counts = list(counts)
    while counts and counts[-1] == 0:
        counts.pop()
    assert 5 <= log <= 9 and sum(abs(c) for c in counts) == 1 << log, (log, counts)
    acc, at = log - 5, 4
    remaining, threshold, nbits = (1 << log) + 1, 1 << log, log + 1
    i = 0
    while i < len(counts):
        assert remaining > 1
        mx = (2 * threshold - 1) - remaining
        v = counts[i] + 1
        i += 1
        if v < mx:
            acc |= v << at
            at += nbits - 1
        else:
            acc |= (v if v < threshold else v + mx) << at
            at += nbits
        remaining -= abs(v - 1)
        if v == 1:              # a zero probability: how many more zeros follow, in 2-bit flags (3 = "and more")
            z = 0
            while i < len(counts) and counts[i] == 0:
                z += 1
                i += 1
            while z >= 3:
                acc |= 3 << at
                at += 2
                z -= 3
            acc |= z << at
            at += 2
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
    assert remaining == 1
    return acc.to_bytes((at + 7) >> 3, "little")


def make_counts(used, log, low=(), rng=None, cap=None):
    """normalised counts of accuracy log `log` in which every symbol of `used` has a probability: "less than one" for those in
    `low`, the rest shared out evenly (rng: at random) among the others, none above `cap`"""
    used = sorted(set(used))
    size = 1 << log
    counts = [0] * (used[-1] + 1)
    for s in used:
        counts[s] = -1 if s in low else 1
    share = [s for s in used if s not in low]
    assert share and len(used) <= size
    cap = cap or size
    rest = size - len(used)
    k = 0
    while rest:
        open_ = [s for s in share if counts[s] < cap]
        assert open_, "no symbol left to take the rest of the probability"
        s = rng.choice(open_) if rng else open_[k % len(open_)]
        take = 1 if not rng else min(rest, cap - counts[s], rng.choice([1, 1, 2, 5, max(1, rest // 2)]))
        counts[s] += take
        rest -= take
        k += 1
    return counts


class FseEncoder:
    """table-driven FSE encoder over zstd_model.build_fse_table's decoding table: for a symbol, the state whose
    [base, base + 2^nb) holds the next state"""

    def __init__(self, counts=None, log=0, rle=None):
        self.counts, self.log, self.rle = counts, log, rle
        self.table = zm.rle_table(rle) if rle is not None else zm.build_fse_table(counts, log)
        self.by_sym = {}
        for state, (sym, nb, base) in enumerate(self.table):
            self.by_sym.setdefault(sym, []).append((base, nb, state))
        for v in self.by_sym.values():
            v.sort()
        self.bases = {s: [e[0] for e in v] for s, v in self.by_sym.items()}

    def final_state(self, sym, pick=0, need_bits=False):
        cands = [e for e in self.by_sym[sym] if e[1] > 0 or not need_bits]
        return cands[pick % len(cands)][2]

    def state_before(self, sym, nxt):
        """-> (state, nb, bits): the state with `sym` from which reading `bits` in nb bits leads to state `nxt`"""
        k = bisect.bisect_right(self.bases[sym], nxt) - 1
        base, nb, state = self.by_sym[sym][k]
        assert base <= nxt < base + (1 << nb)
        return state, nb, nxt - base

    def chain(self, syms, pick=0, need_bits=False):
        """states for `syms` in decoding order -> (first state, [(bits, nb) read after symbol i, for i < n - 1])"""
        state = self.final_state(syms[-1], pick, need_bits)
        steps = [None] * (len(syms) - 1)
        for i in range(len(syms) - 2, -1, -1):
            state, nb, bits = self.state_before(syms[i], state)
            steps[i] = (bits, nb)
        return state, steps


PREDEFINED = None


def predefined():
    global PREDEFINED
    if PREDEFINED is None:
        PREDEFINED = (FseEncoder(zm.LL_DEFAULT, 6), FseEncoder(zm.OF_DEFAULT, 5), FseEncoder(zm.ML_DEFAULT, 6))
    return PREDEFINED


# ----------------------------------------------------------------------------------------------------------- Huffman
class Tree:
    """a Huffman tree given by the weights of symbols 0..last (0: absent; the last one is implied in the description)"""

    def __init__(self, weights):
        weights = list(weights)
        while weights and weights[-1] == 0:
            weights.pop()
        self.weights = weights
        self.depth, table, allw = zm.huffman_table_from_weights(weights[:-1])
        assert allw == weights, "the last weight is not the one the others imply"
        assert sum(1 for w in weights if w == 1) >= 2
        self.codes = {}
        for idx, (s, nb) in enumerate(table):
            if s not in self.codes:
                self.codes[s] = (idx >> (self.depth - nb), nb)

    def stream(self, lits):
        return back_stream([self.codes[b] for b in lits])

    def describe(self, how="direct", log=6):
        w = self.weights[:-1]
        if how == "direct":
            assert 1 <= len(w) <= 128
            w2 = w + [0]
            return bytes([127 + len(w)]) + bytes((w2[i] << 4) | w2[i + 1] for i in range(0, len(w), 2))
        assert 2 <= len(w) <= 255
        # FSE-compressed weights: two interleaved states; no probability above half the table, so that every state
        # reads at least one bit and the end of the stream is where the decoder looks for it
        size = 1 << log
        freq = [w.count(v) for v in range(13)]
        used = [v for v in range(13) if freq[v]]
        counts = [1 if freq[v] else 0 for v in range(13)]
        rest = size - len(used)
        while rest:
            open_ = [v for v in used if counts[v] < size // 2]
            if open_:
                v = max(open_, key=lambda v: freq[v] / counts[v])
            else:       # one weight value only: the other half of the table goes to values that do not occur
                v = next(v for v in range(13) if counts[v] < size // 2)
            counts[v] += 1
            rest -= 1
        enc = FseEncoder(counts, log)
        a, b = w[0::2], w[1::2]             # state 1 decodes the even positions, state 2 the odd ones
        last_is_a = len(w) % 2 == 1         # the stream ends with a failed read after w[n - 2]: that state must read bits
        sa, steps_a = enc.chain(a, need_bits=not last_is_a)
        sb, steps_b = enc.chain(b, need_bits=last_is_a)
        fields = [(sa, log), (sb, log)]
        for k in range(len(w) - 2):
            fields.append((steps_a if k % 2 == 0 else steps_b)[k // 2])
        body = write_fse_counts(counts, log) + back_stream(fields)
        assert len(body) < 128, "FSE-compressed weights of %d bytes do not fit the one-byte size" % len(body)
        return bytes([len(body)]) + body


def tree_for(symbols, depth, rng=None):
    """a complete tree of exactly `depth` bits over `symbols` (depth + 1 <= len(symbols) <= 2^depth): a comb 1, 2, .., depth,
    depth whose leaves are split further until every symbol has one"""
    symbols = sorted(set(symbols))
    assert depth + 1 <= len(symbols) <= (1 << depth) and 1 <= depth <= 11, (depth, len(symbols))
    lengths = list(range(1, depth)) + [depth, depth]
    while len(lengths) < len(symbols):
        short = [i for i, n in enumerate(lengths) if n < depth]
        i = rng.choice(short) if rng else min(short, key=lambda i: lengths[i])
        lengths[i] += 1
        lengths.append(lengths[i])
    if rng:
        rng.shuffle(lengths)
    weights = [0] * (symbols[-1] + 1)
    for s, n in zip(symbols, lengths):
        weights[s] = depth + 1 - n
    return Tree(weights)


# ------------------------------------------------------------------------------------------------------------ blocks
def ll_code(v):
    c = bisect.bisect_right(zm.LL_BASE, v) - 1
    return c, v - zm.LL_BASE[c], zm.LL_BITS[c]


def ml_code(v):
    assert v >= 3
    c = bisect.bisect_right(zm.ML_BASE, v) - 1
    return c, v - zm.ML_BASE[c], zm.ML_BITS[c]


MODES = {"predef": 0, "rle": 1, "fse": 2, "repeat": 3}
MAX_SYMBOL = (35, 31, 52)
MAX_LOG = (9, 8, 9)


class FrameWriter:
    """blocks are added one by one (raw, rle, compressed); finish() puts the header in front.  `out` is what the frame decodes
    to so far and `rep` the three repeat offsets after the last block: a generator may look at both."""

    def __init__(self):
        self.body = []          # (type, block size field, payload)
        self.out = bytearray()
        self.rep = [1, 4, 8]
        self.tables = [None, None, None]
        self.tree = None
        self.max_offset = 0
        self.max_block = 0

    # -------------------------------------------------------------------------------------------- raw and RLE blocks
    def raw(self, data):
        data = bytes(data)
        assert len(data) <= BLOCK_MAX
        self.body.append((0, len(data), data))
        self.out += data
        self.max_block = max(self.max_block, len(data))
        return self

    def rle(self, byte, count):
        assert count <= BLOCK_MAX
        self.body.append((1, count, bytes([byte])))
        self.out += bytes([byte]) * count
        self.max_block = max(self.max_block, count)
        return self

    # ----------------------------------------------------------------------------------------------- literals section
    def _literals(self, lits, lit, hdr, streams, tree, describe, fse_log):
        n = len(lits)
        if lit in ("raw", "rle"):
            if lit == "rle":
                assert n >= 1 and lits == lits[:1] * n
            hdr = hdr or (1 if n < 32 else 2 if n < 4096 else 3)
            kind = 0 if lit == "raw" else 1
            if hdr == 1:
                assert n < 32
                head = bytes([kind | (n << 3)])
            elif hdr == 2:
                assert n < 4096
                head = struct.pack("<H", kind | (1 << 2) | (n << 4))
            else:
                assert n < (1 << 20)
                head = (kind | (3 << 2) | (n << 4)).to_bytes(3, "little")
            return head + (lits if lit == "raw" else lits[:1])
        assert lit in ("huf", "treeless") and n >= 2
        if lit == "huf":
            assert tree is not None
            self.tree = tree
            desc = tree.describe(describe, fse_log)
        else:
            assert self.tree is not None, "treeless literals without an earlier tree"
            desc = b""
        tree = self.tree
        if streams == 1:
            payload = tree.stream(lits)
        else:
            assert streams == 4 and n >= 8
            per = (n + 3) // 4
            parts = [tree.stream(lits[k * per:(k + 1) * per]) for k in range(4)]
            assert all(len(p) < 65536 for p in parts)
            payload = struct.pack("<HHH", len(parts[0]), len(parts[1]), len(parts[2])) + b"".join(parts)
        comp = len(desc) + len(payload)
        kind = 2 if lit == "huf" else 3
        big = max(n, comp)
        if streams == 1:
            assert big < 1024 and hdr in (None, 3)
            head = (kind | (n << 4) | (comp << 14)).to_bytes(3, "little")
        else:
            hdr = hdr or (3 if big < 1024 else 4 if big < 16384 else 5)
            if hdr == 3:
                assert big < 1024
                head = (kind | (1 << 2) | (n << 4) | (comp << 14)).to_bytes(3, "little")
            elif hdr == 4:
                assert big < 16384
                head = (kind | (2 << 2) | (n << 4) | (comp << 18)).to_bytes(4, "little")
            else:
                assert big < 262144
                head = (kind | (3 << 2) | (n << 4) | (comp << 22)).to_bytes(5, "little")
        return head + desc + payload

    # ---------------------------------------------------------------------------------------------- sequences section
    def _offset_value(self, ll, off, rep_auto):
        """the offset value to write (1..3: a repeat code) for actual offset `off`, or for a repeat code given as -1..-3"""
        r = self.rep
        cands = {1: r[0], 2: r[1], 3: r[2]} if ll else {1: r[1], 2: r[2], 3: r[0] - 1}
        if off < 0:
            ofv = -off
            assert 1 <= ofv <= 3 and cands[ofv] >= 1, "repeat offset of zero"
            return ofv
        if rep_auto:
            for ofv in (1, 2, 3):
                if cands[ofv] == off:
                    return ofv
        return off + 3

    def _sequences(self, seqs, at, modes, counts, logs, low, rep_auto, count_bytes, pick, rng):
        """-> (section bytes, resolved triples)"""
        n = len(seqs)
        if n == 0:
            return b"\0", []
        natural = 1 if n < 128 else 2 if n < 0x7F00 else 3
        count_bytes = count_bytes or natural
        assert count_bytes >= natural and (count_bytes < 3 or n >= 0x7F00)
        if count_bytes == 1:
            head = bytes([n])
        elif count_bytes == 2:
            head = bytes([128 + (n >> 8), n & 255])
        else:
            head = b"\xff" + struct.pack("<H", n - 0x7F00)
        resolved, coded = [], []
        for ll, ml, off in seqs:
            ofv = self._offset_value(ll, off, rep_auto)
            (_, _, actual), = zm.resolve_offsets([(ll, ml, ofv)], self.rep)
            assert off < 0 or actual == off
            resolved.append((ll, ml, actual))
            oc = ofv.bit_length() - 1
            coded.append((ll_code(ll), (oc, ofv - (1 << oc), oc), ml_code(ml)))
        encs, descs = [], b""
        for t in range(3):
            used = sorted(set(c[t][0] for c in coded))
            mode = modes[t]
            if mode == "predef":
                enc = predefined()[t]
            elif mode == "rle":
                assert len(used) == 1, "RLE mode needs one code for every sequence"
                enc = FseEncoder(rle=used[0])
                descs += bytes([used[0]])
            elif mode == "fse":
                c = counts[t]
                if c is None:
                    log = logs[t] or 6
                    lows = set(low[t] or ())
                    syms = set(used) | lows
                    if len(syms) < 2:                   # (one symbol with the whole table is what RLE mode is for)
                        lows.add(used[0] + 1 if used[0] < MAX_SYMBOL[t] else 0)
                        syms |= lows
                    if not syms - lows:
                        lows.discard(used[0])           # somebody has to take the rest of the probability
                    c = make_counts(syms, log, low=lows, rng=rng)
                else:
                    log = (sum(abs(x) for x in c)).bit_length() - 1
                assert 5 <= log <= MAX_LOG[t] and len(c) <= MAX_SYMBOL[t] + 1
                enc = FseEncoder(c, log)
                descs += write_fse_counts(c, log)
            else:
                enc = self.tables[t]
                assert enc is not None, "repeat mode without an earlier table"
            assert all(s in enc.by_sym for s in used), ("table %d lacks a code of this block" % t, used)
            encs.append(enc)
            self.tables[t] = enc
        mode_byte = (MODES[modes[0]] << 6) | (MODES[modes[1]] << 4) | (MODES[modes[2]] << 2)
        first, steps = [], []
        for t in range(3):
            s0, st = encs[t].chain([c[t][0] for c in coded], pick)
            first.append(s0)
            steps.append(st)
        fields = [(first[0], encs[0].log), (first[1], encs[1].log), (first[2], encs[2].log)]
        for i, (lc, oc, mc) in enumerate(coded):
            fields += [oc[1:], mc[1:], lc[1:]]
            if i + 1 < n:
                fields += [steps[0][i], steps[2][i], steps[1][i]]
        return head + bytes([mode_byte]) + descs + back_stream(fields), resolved

    # ------------------------------------------------------------------------------------------------ compressed block
    def compressed(self, literals, seqs=(), lit="raw", lit_hdr=None, streams=1, tree=None, describe="direct", fse_log=6,
                   modes=("predef", "predef", "predef"), counts=(None, None, None), logs=(None, None, None), low=(None, None, None),
                   rep="never", count_bytes=None, pick=0, rng=None):
        """literals: all of the block's literal bytes; seqs: (literal length, match length, offset) with the offset either the
        actual distance (written as a repeat code only with rep="auto" and where one fits) or -1 / -2 / -3 for that repeat code"""
        literals = bytes(literals)
        seqs = [tuple(s) for s in seqs]
        assert sum(s[0] for s in seqs) <= len(literals)
        section, resolved = self._sequences(seqs, len(self.out), modes, counts, logs, low, rep == "auto", count_bytes, pick, rng)
        payload = self._literals(literals, lit, lit_hdr, streams, tree, describe, fse_log) + section
        assert len(payload) <= BLOCK_MAX, "compressed block of %d bytes" % len(payload)
        # (no literals in the one-byte form and no sequences: valid, but libzstd before 1.5.5 refuses a compressed block of two bytes)
        assert len(payload) >= 3, "a compressed block of two bytes: give the empty literals a wider header (lit_hdr=2)"
        before = len(self.out)
        out, lp = self.out, 0
        for ll, ml, off in resolved:
            out += literals[lp:lp + ll]
            lp += ll
            assert 1 <= off <= len(out), "offset %d with %d bytes decoded" % (off, len(out))
            self.max_offset = max(self.max_offset, off)
            start = len(out) - off
            if off >= ml:
                out += out[start:start + ml]
            else:
                pat = bytes(out[start:])
                out += (pat * (ml // off + 1))[:ml]
        out += literals[lp:]
        assert len(out) - before <= BLOCK_MAX, "block decodes to %d bytes" % (len(out) - before)
        self.body.append((2, len(payload), payload))
        self.max_block = max(self.max_block, len(payload), len(out) - before)
        return self

    # ---------------------------------------------------------------------------------------------------------- frame
    def need_window(self):
        return max(self.max_offset, self.max_block)

    def finish(self, single=None, window=None, fcs_bytes=None, checksum=False, dict_id_bytes=0, dict_id=0):
        """single: single-segment frame (no window descriptor; the content size is the window, so every block and offset must
        fit it); window: (exponent, mantissa), default the smallest that holds every offset and block; fcs_bytes: width of the
        content size field (0: none; any width that holds the value); -> (frame, decoded bytes)"""
        assert self.body, "a frame has at least one block"
        n = len(self.out)
        if single is None:
            single = window is None and self.need_window() <= n and fcs_bytes != 0
        if fcs_bytes is None:
            fcs_bytes = (1 if n < 256 else 2 if n < 65536 + 256 else 4) if single else 0
        fits = {0: not single, 1: single and n < 256, 2: 256 <= n < 65536 + 256, 4: n < (1 << 32), 8: True}
        assert fits[fcs_bytes], "a content size of %d does not go into %d bytes here" % (n, fcs_bytes)
        flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
        did_flag = {0: 0, 1: 1, 2: 2, 4: 3}[dict_id_bytes]
        head = struct.pack("<IB", zm.MAGIC, (flag << 6) | (int(single) << 5) | (int(checksum) << 2) | did_flag)
        if single:
            assert self.need_window() <= n, "single segment: a block or an offset larger than the content"
        else:
            if window is None:
                need = self.need_window()
                window = next((e, m) for e in range(22) for m in range(8) if (1 << (10 + e)) + ((1 << (10 + e)) >> 3) * m >= need)
            e, m = window
            assert (1 << (10 + e)) + ((1 << (10 + e)) >> 3) * m >= self.need_window(), "window smaller than an offset or a block"
            head += bytes([(e << 3) | m])
        head += dict_id.to_bytes(dict_id_bytes, "little")
        if fcs_bytes:
            head += (n - 256 if fcs_bytes == 2 else n).to_bytes(fcs_bytes, "little")
        parts = [head]
        for i, (btype, size, payload) in enumerate(self.body):
            parts.append(((1 if i + 1 == len(self.body) else 0) | (btype << 1) | (size << 3)).to_bytes(3, "little"))
            parts.append(payload)
        if checksum:
            parts.append(struct.pack("<I", xxh64(self.out) & 0xFFFFFFFF))
        return b"".join(parts), bytes(self.out)


def skippable_frame(data, nibble=0):
    return struct.pack("<II", SKIPPABLE_MAGIC + nibble, len(data)) + bytes(data)


# ------------------------------------------------------------------------------------------------ what a frame is made of
def forms_of(frame, det=None):
    """the names of the format forms a frame uses, from zstd_model.decode_frame's detail (`det`, if the caller has it already)
    and the header byte; the census of tests/test_zstd_writer_host.py counts frames per name"""
    frame = bytes(frame)
    fhd = frame[4]
    single = (fhd >> 5) & 1
    fcs = (1 if single else 0, 2, 4, 8)[fhd >> 6]
    forms = {"hdr %s fcs%d" % ("single" if single else "window", fcs)}
    if det is None:
        det = []
        zm.decode_frame(frame, det)
    prev = None
    for d in det:
        forms.add("block " + d["type"])
        if d["type"] != "compressed":
            prev = d["type"] + " block"
            continue
        li, si = d["literals"], d["sequences"]
        b0 = frame[d["at"] + 3]
        fmt = (b0 >> 2) & 3
        back = set()
        if li["type"] in ("raw", "rle"):
            forms.add("lit %s %dB" % (li["type"], (1, 2, 1, 3)[fmt]))
        else:
            name = "huf" if li["type"] == "compressed" else "treeless"
            forms.add("lit %s 1 stream" % name if li["streams"] == 1 else "lit %s 4 streams %dB" % (name, fmt + 2))
            if li["type"] == "treeless":
                back.add("treeless literals")
        if "tree" in li:
            forms.add("tree " + li["tree"]["kind"])
            forms.add("tree depth %d" % li["max_bits"])
            if len(li["tree"]["weights"]) > 129:
                forms.add("tree above 128 weights")
        n = si["nseq"]
        forms.add("nseq 0" if n == 0 else "nseq 1B" if frame[d["at"] + 3 + _lit_section_bytes(frame, d["at"] + 3)] < 128 else
                  "nseq 2B" if n < 0x7F00 else "nseq 3B")
        if 127 <= n <= 129:
            forms.add("nseq 127..129")
        if n:
            for nm, m, lg in zip(("ll", "of", "ml"), si["modes"], si["logs"]):
                forms.add("mode %s %s" % (nm, ("predef", "rle", "fse", "repeat")[m]))
                if m == 2:
                    forms.add("log %s %d" % (nm, lg))
                if m == 3:
                    back.add("repeat-mode table")
        for ll, ml, ofv in d["seqs"]:
            if ofv <= 3:
                forms.add("rep code %d ll%s" % (ofv, "=0" if ll == 0 else ">0"))
                back.add("repeat offset")
        if prev:
            forms.update("%s after %s" % (b, prev) for b in back)
        prev = "zero-sequence block" if n == 0 else None
    return forms


def _lit_section_bytes(frame, pos):
    b0 = frame[pos]
    kind, fmt = b0 & 3, (b0 >> 2) & 3
    if kind < 2:
        hdr = (1, 2, 1, 3)[fmt]
        size = b0 >> 3 if hdr == 1 else int.from_bytes(frame[pos:pos + hdr], "little") >> 4
        return hdr + (size if kind == 0 else 1)
    if fmt < 2:
        return 3 + ((int.from_bytes(frame[pos:pos + 3], "little") >> 14) & 1023)
    if fmt == 2:
        return 4 + ((int.from_bytes(frame[pos:pos + 4], "little") >> 18) & 16383)
    return 5 + ((int.from_bytes(frame[pos:pos + 5], "little") >> 22) & 262143)


# ------------------------------------------------------------------------------------------------ the hand-written corpus
# Families of small frames that isolate one form each, in three variants (other data, other lengths, other neighbours), and
# frames that mix forms over several blocks.  Each entry is (name, frame, decoded bytes).  A frame here has at most 12 blocks:
# what the GPU decoder's first pass takes for a frame below 128 KiB (4 per 128 KiB + 8; more is its declared limit 67).
VARIANTS = 3


def _bytes(rng, n, alphabet=None):
    if alphabet is None:
        return rng.randbytes(n)
    return bytes(rng.choices(list(alphabet), k=n))


def _small_block(w, rng, nlit=40, **kw):
    """a compressed block of three short sequences over raw literals (needs at least 16 bytes decoded before it)"""
    lits = _bytes(rng, nlit)
    return w.compressed(lits, [(rng.randrange(1, 9), rng.randrange(3, 12), rng.randrange(1, 17)), (0, 5, 3), (4, 3, 9)], **kw)


@functools.lru_cache(maxsize=None)
def header_frames():
    out = []
    for v in range(VARIANTS):
        rng = random.Random(100 + v)
        for single, fcs, n in ((True, 1, 60 + v), (True, 2, 300 + 900 * v), (True, 4, 80 + 4000 * v), (True, 8, 200 + v), (True, 2, 65536 + 255 - v),
                               (True, 4, 65536 + 256 + v), (False, 0, 500 + v), (False, 2, 256 + v), (False, 4, 100 + v), (False, 8, 70000 + v),
                               (False, 2, 40000 + v), (True, 8, 65536 * (v + 1))):
            w = FrameWriter()
            w.raw(_bytes(rng, 30))
            _small_block(w, rng, nlit=12)
            left = n - len(w.out)
            while left > 0:
                k = min(left, 50000)
                (w.rle(rng.randrange(256), k) if rng.randrange(2) else w.raw(_bytes(rng, k, b"\x00\x01\x40\x41")))
                left -= k
            window = None if single else ((v, 0) if w.need_window() <= 1024 << v else (6, v), None, (v + 7, 7 - v))[rng.randrange(3)]
            out.append(("header %s fcs%d n%d v%d" % ("single" if single else "window", fcs, len(w.out), v),) + w.finish(single=single, window=window, fcs_bytes=fcs))
        w = FrameWriter().raw(b"")
        out.append(("header empty frame v%d" % v,) + w.finish(single=True, fcs_bytes=(1, 4, 8)[v]))
        w = FrameWriter().compressed(b"", [], lit_hdr=2 + v % 2)
        out.append(("header empty compressed block v%d" % v,) + w.finish(fcs_bytes=(0, 4, 8)[v]))
    return out


@functools.lru_cache(maxsize=None)
def literal_frames():
    out = []
    for v in range(VARIANTS):
        rng = random.Random(200 + v)
        abc = bytes(rng.sample(range(129), 9 + v))
        for lit, hdr, n in (("raw", 1, 0), ("raw", 1, 31 - v), ("raw", 2, 20 + v), ("raw", 2, 4095 - v), ("raw", 3, 17 + v), ("raw", 3, 4096 + 9000 * v),
                            ("rle", 1, 1 + v), ("rle", 1, 31), ("rle", 2, 20 + v), ("rle", 2, 4095 - v), ("rle", 3, 31 - v), ("rle", 3, (100000, 5000, 1 << 17)[v] - 20)):
            w = FrameWriter().raw(_bytes(rng, 40))
            lits = _bytes(rng, n) if lit == "raw" else bytes([rng.randrange(256)]) * n
            seqs = [(min(n, 3), 7, 20), (0, 3, 1)] if v != 1 else ([(n, 4, 40)] if n else [(0, 4, 40)])
            w.compressed(lits, seqs, lit=lit, lit_hdr=hdr)
            out.append(("literals %s %dB n%d v%d" % (lit, hdr, n, v),) + w.finish())
        for streams, hdr, n in ((1, 3, 2 + v), (1, 3, 700 + v), (4, 3, 8 + v), (4, 3, 900 + v), (4, 4, 40 + v), (4, 4, 16000 + v), (4, 5, 99 + v), (4, 5, (131000, 17000, 40000)[v])):
            w = FrameWriter().raw(_bytes(rng, 40))
            tree = tree_for(abc, 4 + v, rng)
            w.compressed(_bytes(rng, n, abc), [(2, 9, 33)], lit="huf", lit_hdr=hdr, streams=streams, tree=tree, describe=("direct", "fse")[(v + n) % 2])
            # ... and the same tree once more without its description, in every header form it fits
            w.compressed(_bytes(rng, n, abc), [(1, 4, 2)], lit="treeless", lit_hdr=hdr, streams=streams)
            out.append(("literals huf %d streams %dB n%d v%d" % (streams, hdr, n, v),) + w.finish())
        # treeless literals after blocks of every other kind: the tree survives them all
        for between in ("raw literals", "rle literals", "raw block", "rle block", "zero sequences", "empty block"):
            w = FrameWriter().raw(_bytes(rng, 40))
            w.compressed(_bytes(rng, 300, abc), [(2, 9, 33)], lit="huf", streams=(1, 4)[v % 2], tree=tree_for(abc, 5, rng), describe=("fse", "direct")[v % 2])
            for _ in range(1 + v):
                if between == "raw literals":
                    _small_block(w, rng)
                elif between == "rle literals":
                    w.compressed(b"z" * 50, [(10, 4, 5)], lit="rle")
                elif between == "raw block":
                    w.raw(_bytes(rng, 77))
                elif between == "rle block":
                    w.rle(3, 1000)
                elif between == "zero sequences":
                    w.compressed(_bytes(rng, 60), [])
                else:
                    w.compressed(b"", [], lit_hdr=2)
            w.compressed(_bytes(rng, 500, abc), [(9, 30, 60), (0, 3, 1)], lit="treeless", streams=(4, 1)[v % 2])
            w.compressed(_bytes(rng, 90, abc), [], lit="treeless")
            out.append(("literals treeless after %s v%d" % (between, v),) + w.finish())
    return out


@functools.lru_cache(maxsize=None)
def huffman_frames():
    out = []
    for v in range(VARIANTS):
        rng = random.Random(300 + v)
        for depth in range(1, 12):
            for describe in ("direct", "fse"):
                k = min(1 << depth, depth + 1 + (0, 3, 40)[v])
                top = 129 if describe == "direct" else 256
                symbols = sorted(rng.sample(range(top), k))
                if v == 2 and describe == "direct" and k > 1:
                    symbols[-1] = 128                   # 128 weights written out, the 129th implied
                tree = tree_for(symbols, depth, rng)
                w = FrameWriter().raw(_bytes(rng, 20))
                n = (300, 1000, 5000)[v]
                w.compressed(_bytes(rng, n, symbols), [(5, 6, 7), (0, 3, 3)], lit="huf", streams=1 if n < 500 else 4, tree=tree, describe=describe,
                             fse_log=(6, 5, 6)[v])
                out.append(("huffman depth %d %s %d symbols v%d" % (depth, describe, k, v),) + w.finish())
        for k, depth in ((256, 8), (256, 11), (255, 9), (200, 8)):
            symbols = sorted(rng.sample(range(256), k - 1)) + [255] if k < 256 else list(range(256))
            symbols = sorted(set(symbols))
            w = FrameWriter().raw(_bytes(rng, 20))
            w.compressed(_bytes(rng, 4000, symbols), [(5, 6, 7)], lit="huf", streams=4, tree=tree_for(symbols, depth, rng), describe="fse")
            out.append(("huffman %d symbols depth %d fse v%d" % (len(symbols), depth, v),) + w.finish())
    return out


def _counted_block(w, rng, n, style):
    """a compressed block of exactly n sequences that decodes to less than 128 KiB"""
    if style == 0:          # three RLE tables: two bits a sequence (nothing but the offsets' extra bits)
        w.compressed(b"", [(0, 3, 2)] * n, modes=("rle", "rle", "rle"))
    elif style == 1:
        seqs = [(rng.randrange(2) if i % 8 == 0 else 0, 3, rng.randrange(1, 13)) for i in range(n)]
        w.compressed(_bytes(rng, sum(s[0] for s in seqs) + 3), seqs)
    else:
        seqs = [(rng.randrange(2) if i % 8 == 0 else 0, 3 + (i % 16 == 0), rng.choice([1, 2, 3, 5, 9, 13, -1, -2])) for i in range(n)]
        w.compressed(_bytes(rng, sum(s[0] for s in seqs)), seqs, modes=("fse", "fse", "fse"), logs=(5, 5, 5), rep="auto", rng=rng)


@functools.lru_cache(maxsize=None)
def seqcount_frames():
    out = []
    for v in range(VARIANTS):
        rng = random.Random(400 + v)
        for n in (0, 1, 2, 63, 64, 65, 126, 127, 128, 129, 255, 256, 257) + ((0x7EFF, 0x7F00), (0x7F01,), (0x7F00,))[v]:
            w = FrameWriter().raw(_bytes(rng, 50))
            _counted_block(w, rng, n, (v + n) % 3 if n else 1)
            w.compressed(_bytes(rng, 9), [(3, 4, 40)])
            out.append(("sequences %d v%d" % (n, v),) + w.finish())
        for n, cb in ((1, 2), (100 + v, 2), (127, 2)):      # a count below 128 in the two-byte form
            w = FrameWriter().raw(_bytes(rng, 50))
            seqs = [(1, 3, rng.randrange(1, 40)) for _ in range(n)]
            w.compressed(_bytes(rng, n), seqs, count_bytes=cb)
            out.append(("sequences %d in %d bytes v%d" % (n, cb, v),) + w.finish())
    return out


def _spread_block(w, rng, nseq, modes, logs=(None, None, None), low=(None, None, None), codes=None, **kw):
    """sequences whose three codes are drawn from `codes` = (LL codes, OF codes, ML codes) -- in repeat mode, from those of them
    the table being repeated has; every offset is a new one (code 2 and up) inside what has been decoded, the block stays
    below 128 KiB"""
    codes = codes or (list(range(0, 26)), list(range(2, 6)), list(range(0, 40)))
    codes = [[c for c in cs if m != "repeat" or c in w.tables[t].by_sym] for t, (cs, m) in enumerate(zip(codes, modes))]
    seqs, pos, room = [], len(w.out), BLOCK_MAX - 64
    for i in range(nseq):
        lc, mc = rng.choice(codes[0]), rng.choice(codes[2])
        ll = zm.LL_BASE[lc] + rng.getrandbits(zm.LL_BITS[lc])
        ml = zm.ML_BASE[mc] + rng.getrandbits(zm.ML_BITS[mc])
        if ll + ml > room:
            continue
        fits = [oc for oc in codes[1] if oc >= 2 and (1 << oc) - 3 <= pos + ll]
        assert fits, "no offset code of this table reaches back so little"
        oc = rng.choice(fits)
        ofv = min((1 << oc) + rng.getrandbits(oc), pos + ll + 3)
        seqs.append((ll, ml, ofv - 3))
        pos += ll + ml
        room -= ll + ml
    lits = _bytes(rng, sum(s[0] for s in seqs) + rng.randrange(0, 9))
    return w.compressed(lits, seqs, modes=modes, logs=logs, low=low, rng=rng, **kw)


@functools.lru_cache(maxsize=None)
def table_frames():
    out = []
    one = ([3], [4], [7])           # one code per table: what RLE mode needs
    for v in range(VARIANTS):
        rng = random.Random(500 + v)
        for log in (5, 6, 7, 8, 9):
            logs = (log, min(log, 8), log)
            w = FrameWriter().raw(_bytes(rng, 3000))
            many = tuple(c[:(1 << lg) - 4] for c, lg in zip((list(range(0, 24 + v)), list(range(2, 12)), list(range(0, 40 + v))), logs))
            _spread_block(w, rng, 200 + 50 * v, ("fse", "fse", "fse"), logs, codes=many)
            _spread_block(w, rng, 40, ("repeat", "repeat", "repeat"), codes=many)
            out.append(("tables fse log %d v%d" % (log, v),) + w.finish())
            # few codes far apart, some "less than one": long runs of zero probabilities in the description
            w = FrameWriter().raw(_bytes(rng, 3000))
            sparse = ([0, 1, 30 - v], [2, 11 - v], [0, 44 + v])
            _spread_block(w, rng, 30, ("fse", "fse", "fse"), logs, low=([35, 30 - v], [31 - 9 * v], [52 - v, 20]), codes=sparse)
            out.append(("tables fse sparse log %d v%d" % (log, v),) + w.finish())
        for t, name in enumerate(("ll", "of", "ml")):
            for other in ("predef", "fse"):
                modes = [other] * 3
                modes[t] = "rle"
                codes = [list(range(0, 20)), list(range(2, 9)), list(range(0, 36))]
                codes[t] = [(16 + v, 5 + v, 33 + v)[t]]
                w = FrameWriter().raw(_bytes(rng, 3000))
                _spread_block(w, rng, 60, tuple(modes), codes=tuple(codes))
                modes[t] = "repeat"
                _spread_block(w, rng, 20, tuple(modes), codes=tuple(codes))
                out.append(("tables rle %s with %s v%d" % (name, other, v),) + w.finish())
        # repeat mode after RLE, FSE and predefined tables, directly and across blocks that leave the tables alone
        for first in ("rle", "fse", "predef"):
            for between in ("nothing", "raw block", "rle block", "zero sequences"):
                w = FrameWriter().raw(_bytes(rng, 3000))
                codes = one if first == "rle" else None
                _spread_block(w, rng, 50, (first,) * 3, codes=codes, logs=(7, 6, 8))
                for k in range(3):
                    if between == "raw block":
                        w.raw(_bytes(rng, 10 + k))
                    elif between == "rle block":
                        w.rle(k, 5000)
                    elif between == "zero sequences":
                        w.compressed(_bytes(rng, 33), [])
                    modes = ("repeat", "repeat", "repeat") if k != 1 else ("repeat", "predef", "repeat")
                    _spread_block(w, rng, 30 + k, modes, codes=codes if k != 1 or codes is None else (one[0], list(range(2, 7)), one[2]))
                out.append(("tables repeat after %s, %s between v%d" % (first, between, v),) + w.finish())
    return out


@functools.lru_cache(maxsize=None)
def repeat_frames():
    """the six repeat-offset cases (codes 1..3 with and without literals; code 3 without literals is `first offset - 1`), at the
    start of a frame (history 1, 4, 8), inside a block, and at the start of a block after blocks of every kind"""
    out = []
    for v in range(VARIANTS):
        rng = random.Random(600 + v)
        w = FrameWriter()
        w.compressed(_bytes(rng, 60), [(8 + v, 5, -3), (2, 4, -2), (1, 3, -3), (0, 3, -1), (0, 6, -2), (3, 9, -1), (2, 7, 13 + v), (0, 4, -3), (0, 3, -3)])
        out.append(("repeats from the initial history v%d" % v,) + w.finish())
        for between in ("nothing", "raw block", "rle block", "zero sequences", "empty block"):
            for start in ((1, -1), (1, -2), (1, -3), (0, -1), (0, -2), (0, -3)):
                w = FrameWriter().raw(_bytes(rng, 200))
                w.compressed(_bytes(rng, 50), [(3, 5, 100 + v), (2, 4, 37), (1, 3, 66 - v), (4, 4, -2)], modes=("fse", "predef", "fse"))
                if between == "raw block":
                    w.raw(_bytes(rng, 30 + v))
                elif between == "rle block":
                    w.rle(9, 300 + v)
                elif between == "zero sequences":
                    w.compressed(_bytes(rng, 20 + v), [])
                elif between == "empty block":
                    w.compressed(b"", [], lit_hdr=3)
                # the block begins with a repeat code: its history is the previous blocks'
                seqs = [(start[0] * (1 + v), 6, start[1]), (0, 3, -3), (2, 5, -2), (0, 4, -1), (5, 3, -1), (1, 3, -3), (0, 5, 150), (0, 3, -2), (7, 3, -1)]
                w.compressed(_bytes(rng, 40), seqs)
                w.compressed(_bytes(rng, 120), [(2, 3, -1), (0, 3, -1)] + [(i % 3, 3 + i, -(1 + (i * 7 + v) % 3)) for i in range(70)], rep="auto")
                out.append(("repeats code %d ll %d after %s v%d" % (-start[1], start[0], between, v),) + w.finish())
        # offsets given as distances, written as repeat codes wherever one fits
        w = FrameWriter().raw(_bytes(rng, 500))
        offs = [9, 33, 120]
        seqs = [(rng.randrange(3), rng.randrange(3, 20), rng.choice(offs + [rng.randrange(1, 400)])) for _ in range(300)]
        w.compressed(_bytes(rng, sum(s[0] for s in seqs)), seqs, rep="auto", modes=("predef", "fse", "predef"))
        w.compressed(_bytes(rng, sum(s[0] for s in seqs)), seqs, rep="auto", modes=("predef", "repeat", "predef"))
        out.append(("repeats chosen by distance v%d" % v,) + w.finish())
    return out


EVERY_CODE = (range(36), range(32), range(53))      # as "less than one" probabilities: a later block may repeat the table with any code


@functools.lru_cache(maxsize=None)
def mixed_frames():
    """twelve blocks a frame (the decoder prepares eight side by side: trees, tables and offset history cross that seam)"""
    out = []
    for v in range(VARIANTS * 2):
        rng = random.Random(700 + v)
        abc = bytes(rng.sample(range(129), 20))
        w = FrameWriter().raw(_bytes(rng, 2000))
        w.compressed(_bytes(rng, 800, abc), [(4, 9, 1000), (0, 3, 5)], lit="huf", streams=4, tree=tree_for(abc, 6 + v % 5, rng), describe=("fse", "direct")[v % 2],
                     modes=("fse", "fse", "fse"), logs=(9, 8, 9), low=EVERY_CODE)
        kinds = ["raw", "rle", "zero", "treeless", "treeless4", "rawlit", "rlelit", "treeless", "rawlit", "treeless4"]
        rng.shuffle(kinds)
        for kind in kinds[:rng.randrange(6, 11)]:
            if kind == "raw":
                w.raw(_bytes(rng, rng.randrange(0, 300)))
            elif kind == "rle":
                w.rle(rng.randrange(256), rng.randrange(1, 20000))
            elif kind == "zero":
                w.compressed(_bytes(rng, 50, abc), [], lit=rng.choice(["raw", "treeless"]))
            else:
                lit = {"treeless": "treeless", "treeless4": "treeless", "rawlit": "raw", "rlelit": "rle"}[kind]
                seqs = [(rng.randrange(4), rng.randrange(3, 40), rng.choice([-1, -2, -3, -1, rng.randrange(1, 2000)])) for _ in range(rng.randrange(1, 80))]
                seqs = [(ll + (1 if off == -3 else 0), ml, off) for ll, ml, off in seqs]     # (code 3 without literals may reach zero)
                n = sum(s[0] for s in seqs) + rng.randrange(10)
                lits = bytes([abc[0]]) * max(n, 1) if lit == "rle" else _bytes(rng, max(n, 8), abc)
                modes = tuple(rng.choice(["repeat", "repeat", "predef", "fse"]) for _ in range(3))
                w.compressed(lits, seqs, lit=lit, streams=4 if kind == "treeless4" else 1, modes=modes, low=EVERY_CODE, rep="auto", rng=rng)
        out.append(("mixed %d blocks v%d" % (len(w.body), v),) + w.finish(single=bool(v % 2), fcs_bytes=(None, 8, 4)[v % 3] if v % 2 else None))
    return out


FAMILIES = {"header": header_frames, "literals": literal_frames, "huffman": huffman_frames, "sequences": seqcount_frames, "tables": table_frames,
            "repeats": repeat_frames, "mixed": mixed_frames}


def form_corpus():
    return [e for f in FAMILIES.values() for e in f()]


# --------------------------------------------------------------------------------------- geometry: the kernels' own boundaries
# The execution kernel splits runs above 16,383 into several records, keeps a checkpoint per 64 records and the last 32 KiB (+ 4 KiB)
# of output in a ring, reads matches from farther back out of the flushed output, and resolves repeat offsets per block before it
# knows the history the block starts with.  These frames put exact numbers on each of those.
RUN_LENGTHS = sorted({k * 16383 + d for k in (1, 2, 3, 4, 8) for d in (-1, 0, 1)} | {65535, 65536})
FOUR = b"\x00\x01\x40\x41"


def _long_literals(w, rng, n, seqs, **kw):
    """a block with n literals: raw while that fits a block, else four Huffman streams of two bits a literal"""
    if n < 8 or (n <= 60000 and rng.randrange(2)):
        return w.compressed(_bytes(rng, n), seqs, **kw)
    return w.compressed(_bytes(rng, n, FOUR), seqs, lit="huf", streams=4, tree=tree_for(FOUR, 2), **kw)


@functools.lru_cache(maxsize=None)
def run_frames():
    out = []
    rng = random.Random(800)
    for n in RUN_LENGTHS + [BLOCK_MAX - 3]:
        w = FrameWriter().raw(_bytes(rng, 300))
        _long_literals(w, rng, n + (4 if n + 7 <= BLOCK_MAX else 0), [(n, 3, rng.choice([1, 250, 300]))])
        out.append(("literal run of %d" % n,) + w.finish())
    for n in RUN_LENGTHS + [BLOCK_MAX - 2, BLOCK_MAX]:
        w = FrameWriter().raw(_bytes(rng, 300))
        ll = 2 if n + 2 <= BLOCK_MAX else 0
        w.compressed(_bytes(rng, ll), [(ll, n, rng.choice([1, 3, 299, 300 + ll]))])
        out.append(("match of %d" % n,) + w.finish())
    for n in [x for x in RUN_LENGTHS if x <= 65536]:
        w = FrameWriter().raw(_bytes(rng, 300))
        _long_literals(w, rng, n, [(n, n, rng.choice([2, n, n + 300]))])
        out.append(("literal run and match of %d" % n,) + w.finish())
    # several in a row, in one block and in consecutive blocks; with offsets that are repeat codes of a history the block does
    # not know yet (a split match then continues "what the record before resolved to")
    for v in range(3):
        w = FrameWriter().raw(_bytes(rng, 300))
        _long_literals(w, rng, 16383 + 16382 + 16384 + 1 + v, [(16383, 16383, 77), (16382, 16384, 16382), (16384, 16382, 1 + v), (1, 3, 1)])
        _long_literals(w, rng, 32766 + 5, [(32766, 49149, 32766 + 49149), (0, 3, 1), (5, 32768, 2 + v)])
        w.compressed(_bytes(rng, 9), [(0, 16384 + v, 5), (0, 32766 + v, 9), (0, 49149, 16383 + v), (9, 16383, 16382 + v)])
        _long_literals(w, rng, 40000 + 16384, [(40000, 36000, -2), (0, 20000, -3), (16384, 16384, -1)])
        _long_literals(w, rng, 16384, [(0, 65536, -3), (16384, 32768, -2)])
        out.append(("long runs in a row v%d" % v,) + w.finish())
    return out


@functools.lru_cache(maxsize=None)
def near_frames():
    """offsets 1..8 with matches that go round the ring several times, the second one from a block's first byte"""
    out = []
    rng = random.Random(810)
    for off in range(1, 9):
        w = FrameWriter().raw(_bytes(rng, 8))
        w.compressed(_bytes(rng, 5), [(5, 100000 + off, off)])
        w.compressed(b"", [(0, BLOCK_MAX, off)])
        w.compressed(_bytes(rng, 3), [(3, 40000, off), (0, 40000, -1), (0, 40000 + off, 9 - off)], rep="auto")
        out.append(("offset %d round the ring" % off,) + w.finish())
    return out


FAR_OFFSETS = [32766, 32767, 32768, 32769, 36862, 36863, 36864, 36865, 65535, 65536, 65537, 131071, 131072, 131073, 262143, 262145]


def _raw_bytes(w, rng, n):
    while n > 0:
        k = min(n, BLOCK_MAX)
        w.raw(_bytes(rng, k))
        n -= k
    return w


@functools.lru_cache(maxsize=None)
def far_frames():
    out = []
    rng = random.Random(820)
    for off in FAR_OFFSETS:
        # the match's source begins at the frame's first byte / a few bytes in; then the same distance once more as a repeat
        for extra in (0, 11):
            w = _raw_bytes(FrameWriter(), rng, off - 7 + extra)
            w.compressed(_bytes(rng, 20), [(7, 5000, off), (0, 40, 3), (4, 3000, -2), (9, 20000, off + 1 if extra else off - 1)])
            out.append(("offset %d, %d bytes before its source" % (off, extra),) + w.finish())
    w = _raw_bytes(FrameWriter(), rng, 262145 + 10)
    seqs = []
    for off in FAR_OFFSETS:
        seqs += [(1, 700, off), (0, 5, 1)]
    w.compressed(_bytes(rng, len(FAR_OFFSETS)), seqs)
    out.append(("every far offset in one block",) + w.finish())
    return out


@functools.lru_cache(maxsize=None)
def huge_frame():
    """3 MiB, whose last blocks copy from its first bytes"""
    rng = random.Random(830)
    w = _raw_bytes(FrameWriter(), rng, 23 * BLOCK_MAX + 12345)
    for k in range(4):
        n = len(w.out)
        seqs = [(10, 30000, n + 10), (0, 20000, (1 << 20) + 1 + k), (5, 40000, (2 << 20) - k), (0, 3, 1), (3, 30000, n + 10 + 90008 - 100 * k), (1, 9000, 3)]
        w.compressed(_bytes(rng, 19 + k), seqs)
    return [("3 MiB reaching back to the first bytes",) + w.finish()]


@functools.lru_cache(maxsize=None)
def seam_frames():
    """A match whose source ends exactly at, one byte before and one byte after the start of the record that copies it (the
    record begins with the sequence's literals; a sequence of more than 16,383 literals or match bytes is several records),
    and the same around the start of the match itself."""
    out = []
    rng = random.Random(840)
    for ll, ml in ((16383, 16383), (5, 3000), (0, 16383), (20000, 20000), (16384, 16384), (100, 40000), (16383, 3)):
        starts = {"record": ml + (ll if ll <= 16383 else ll % 16383), "sequence": ml + ll, "match": ml}
        for what, base in starts.items():
            for d in (-1, 0, 1):
                if base + d < 1:
                    continue
                w = _raw_bytes(FrameWriter(), rng, 50000)
                _long_literals(w, rng, ll + 2, [(ll, ml, base + d), (1, 4, 9)])
                out.append(("ll %d ml %d: source ends %+d from the %s's start" % (ll, ml, d, what),) + w.finish())
    return out


@functools.lru_cache(maxsize=None)
def boundary_frames():
    """matches and literal runs across block boundaries"""
    out = []
    rng = random.Random(850)
    for v in range(3):
        w = FrameWriter()
        w.compressed(_bytes(rng, 6000 + v), [(500, 700, 100 + v)])              # ends with 5,500 literals behind its last sequence ...
        w.compressed(_bytes(rng, 5000), [(5000 - v, 30, 1)])                     # ... and the next block goes on with literals
        w.compressed(b"", [(0, 20000 + v, 1)])                                   # begins with the previous block's last byte, many times
        w.compressed(_bytes(rng, 3), [(0, 100, 50), (3, 3, -1)])                 # a source that runs on into the block that copies it
        w.raw(_bytes(rng, 1000 + v))
        w.compressed(b"", [(0, 3000, 1), (0, 3000, 1000 + v)])                   # after a raw block
        w.rle(200 + v, 70000)
        w.compressed(b"", [(0, 40000, 1), (0, 3, 70001), (0, 20000, 70000 + v)])  # after an RLE block, and back across it
        w.compressed(_bytes(rng, 10), [])
        w.compressed(_bytes(rng, 1), [(0, 9, 10), (1, 3, 20)])                   # from a block that was nothing but literals
        w.compressed(b"", [(0, 3, 3)])
        out.append(("across block boundaries v%d" % v,) + w.finish())
    return out


@functools.lru_cache(maxsize=None)
def dense_frames():
    """Sequences that take as many bits each as the format has: offsets of a megabyte (20 extra bits), every code in use a "less
    than one" probability of tables at their highest accuracy logs (9 + 8 + 9 state bits a sequence), thousands in a row"""
    out = []
    rng = random.Random(860)
    for v, (lcs, mcs, ocs) in enumerate((([16, 17], [32, 33, 34], [20]), ([25, 24], [43, 42], [20, 19]), ([16, 26], [32, 44], [20, 18, 2]))):
        w = _raw_bytes(FrameWriter(), rng, (2 << 20) + 100)
        for blk in range(2):
            seqs, room, pos = [], BLOCK_MAX - 16, len(w.out)
            while True:
                lc, mc, oc = rng.choice(lcs), rng.choice(mcs), rng.choice(ocs)
                ll = zm.LL_BASE[lc] + rng.getrandbits(zm.LL_BITS[lc])
                ml = zm.ML_BASE[mc] + rng.getrandbits(zm.ML_BITS[mc])
                if ll + ml > room:
                    break
                seqs.append((ll, ml, min((1 << oc) + rng.getrandbits(oc), pos + ll + 3) - 3))
                pos += ll + ml
                room -= ll + ml
            low = tuple([s for s in r if s != 0] for r in EVERY_CODE)           # code 0 takes what probability is left
            w.compressed(_bytes(rng, sum(s[0] for s in seqs)), seqs, modes=("fse", "fse", "fse") if blk == 0 else ("repeat",) * 3, logs=(9, 8, 9), low=low)
        out.append(("dense bit stream v%d, %d sequences in the last block" % (v, len(seqs)),) + w.finish())
    return out


@functools.lru_cache(maxsize=None)
def literal_use_frames():
    out = []
    rng = random.Random(870)
    for v in range(3):
        w = FrameWriter().raw(_bytes(rng, 100))
        w.compressed(_bytes(rng, 5000 + v), [(0, 10 + v, 7)] * 50)                          # every literal behind the last sequence
        w.compressed(_bytes(rng, 50 * (3 + v)), [(3 + v, 4, 100)] * 50)                     # every literal used up by the sequences
        w.compressed(b"", [(0, 5, 100 + v)] * 70)                                           # no literals at all
        w.compressed(_bytes(rng, 20000 + v, FOUR), [(0, 3, 1), (0, 3, 2)], lit="huf", streams=4, tree=tree_for(FOUR, 2))
        w.compressed(_bytes(rng, 1), [(1, 3, 1)])
        out.append(("literals all behind, all used, none v%d" % v,) + w.finish())
    return out


GEOMETRY = {"runs": run_frames, "near": near_frames, "far": far_frames, "huge": huge_frame, "seams": seam_frames, "boundaries": boundary_frames,
            "dense": dense_frames, "literal_use": literal_use_frames}


def geometry_corpus():
    return [e for f in GEOMETRY.values() for e in f()]


# ------------------------------------------------------------------------------- valid frames the GPU decoder declares it does not take
def limit_frames():
    """(name, payload, decoded bytes, the status codes flagstat_zstd_kernels.h allows for it); libzstd decodes every one.
    (A dictionary ID other than zero makes libzstd ask for that dictionary, so the ID field written here, one, two or four bytes
    wide, holds zero: "no dictionary", which libzstd accepts and the GPU decoder declines by the flag alone.)"""
    rng = random.Random(900)

    def small():
        w = FrameWriter().raw(_bytes(rng, 3000))
        _spread_block(w, rng, 100, ("fse", "predef", "fse"))
        return w

    out = [("content checksum",) + small().finish(checksum=True) + ((66,),),
           ("content checksum, single segment",) + small().finish(checksum=True, single=True, fcs_bytes=4) + ((66,),)]
    for nb in (1, 2, 4):
        out.append(("dictionary ID field of %d bytes" % nb,) + small().finish(dict_id_bytes=nb) + ((65,),))
    f, e = small().finish()
    out.append(("skippable frame in front", skippable_frame(_bytes(rng, 33), 3) + f, e, (64,)))
    out.append(("empty skippable frame in front", skippable_frame(b"") + f, e, (64,)))
    f2, e2 = small().finish(single=True)
    out.append(("second frame behind", f + f2, e + e2, (68,)))
    out.append(("skippable frame behind", f + skippable_frame(b"abc"), e, (68,)))
    w = FrameWriter()
    for k in range(512):
        w.rle(k & 255, BLOCK_MAX)
    w.rle(7, 2)
    # 64 MiB + 2 bytes in 513 RLE blocks: above kZstdMaxFrameBytes AND above kZstdMaxBlocks, whichever the decoder meets first
    out.append(("content above 64 MiB",) + w.finish(fcs_bytes=8) + ((69, 67),))
    return out


# ------------------------------------------------------------------------------------------------------ the seeded shape fuzzer
_LENGTHS = [0, 1, 2, 3, 4, 7, 15, 16, 17, 35, 63, 64, 65, 130, 131, 259, 1000, 16382, 16383, 16384, 16385, 32765, 32766, 32767, 49149, 65535, 65536, 65537]
_OFFSETS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 100, 32766, 32767, 32768, 32769, 36862, 36863, 36864, 36865, 65535, 65536, 65537, 131071, 131072, 131073]


def random_frame(rng):
    """a random valid frame -> (frame, decoded bytes): a random header form, 1..12 blocks of random kinds, random legal tables and
    modes, sequences drawn with a bias towards the lengths and distances where the execution kernel changes path"""
    w = FrameWriter()
    abc = bytes(rng.sample(range(256 if rng.randrange(3) else 129), rng.choice([2, 3, 4, 9, 17, 40, 100])))
    for _ in range(rng.randrange(1, 13)):
        if len(w.out) > 70000:          # (the tests that run this decode every frame in Python as well)
            break
        kind = rng.choice(["raw", "rle", "compressed", "compressed", "compressed", "compressed"])
        if kind == "raw":
            w.raw(_bytes(rng, rng.choice([0, 1, 17, 300, 300, 5000, 5000, 5000, 40000, BLOCK_MAX])))
            continue
        if kind == "rle":
            w.rle(rng.randrange(256), rng.choice([1, 2, 31, 31, 1000, 1000, 16383, 16384, 16385, BLOCK_MAX]))
            continue
        # ---- sequences: repeat codes wherever the history allows them, else the lengths and distances of the lists above
        r, pos, room, seqs = list(w.rep), len(w.out), BLOCK_MAX - rng.randrange(0, 40), []
        nseq = rng.choice([0, 1, 2, 5, 5, 20, 63, 64, 65, 127, 128, 129, 300, 2000])
        small = nseq > 129
        for _ in range(nseq):
            ll = rng.choice(_LENGTHS[:9] if small or rng.randrange(8) else _LENGTHS)
            ml = max(3, rng.choice(_LENGTHS[:12] if small or rng.randrange(8) else _LENGTHS))
            if ll + ml > room:
                ll, ml = min(ll, 2), 3
                if ll + ml > room:
                    break
            code = rng.choice([1, 2, 3])
            cand = ({1: r[0], 2: r[1], 3: r[2]} if ll else {1: r[1], 2: r[2], 3: r[0] - 1})[code]
            if rng.randrange(3) == 0 and 1 <= cand <= pos + ll:
                off = -code
            else:
                near = [o for o in _OFFSETS if o <= pos + ll]
                if not near:
                    ll += 1
                    if ll + ml > room:
                        break
                    near = [1]
                off = rng.choice(near + [pos + ll, rng.randrange(1, pos + ll + 1)])
            ofv = -off if off < 0 else off + 3
            zm.resolve_offsets([(ll, ml, ofv)], r)
            seqs.append((ll, ml, off))
            pos += ll + ml
            room -= ll + ml
        used = sum(s[0] for s in seqs)
        nlit = used + (rng.choice([0, 0, 1, 5, 5, 200, 200, 200, 20000]) if room > 20000 else min(room, rng.randrange(3)))
        # ---- literals
        lit = rng.choice(["raw", "rle", "huf", "huf", "treeless", "treeless"])
        if lit == "treeless" and w.tree is None:
            lit = "huf"
        if lit in ("huf", "treeless") and nlit < 8:
            lit = "raw"
        if lit == "raw" and nlit > 60000:
            lit = "huf"
        kw = {}
        if lit == "raw":
            lits = _bytes(rng, nlit)
            kw["lit_hdr"] = rng.choice([h for h in (1, 2, 3) if nlit < (32, 4096, 1 << 20)[h - 1] and (h > 1 or nlit or seqs)])
        elif lit == "rle":
            lits = bytes([rng.randrange(256)]) * max(nlit, 1)
            kw["lit_hdr"] = rng.choice([h for h in (1, 2, 3) if len(lits) < (32, 4096, 1 << 20)[h - 1]])
        else:
            if lit == "huf":
                depth = rng.choice([d for d in range(1, 12) if d + 1 <= len(abc) <= 1 << d])
                kw["tree"] = tree_for(abc, depth, rng)
                kw["describe"] = "direct" if max(abc) <= 128 and rng.randrange(2) else "fse"
                kw["fse_log"] = rng.choice([5, 6])
                symbols = abc
            else:
                symbols = bytes(s for s, x in enumerate(w.tree.weights) if x)
            lits = _bytes(rng, nlit, symbols)
            # (the worst code here has 11 bits: below 700 literals the section fits the 10-bit sizes of one stream)
            kw["streams"] = 1 if nlit < 700 and rng.randrange(2) else 4
            if kw["streams"] == 4:
                kw["lit_hdr"] = rng.choice([h for h in (3, 4, 5) if nlit < (700, 11000, 1 << 18)[h - 3]])
        # ---- tables
        modes = []
        for t in range(3):
            pick = rng.choice(["predef", "fse", "fse", "repeat", "repeat", "rle"])
            if pick == "repeat" and (w.tables[t] is None or not seqs):
                pick = "fse"
            modes.append(pick)
        logs = (rng.randrange(5, 10), rng.randrange(5, 9), rng.randrange(5, 10))
        logs = tuple(max(lg, 6) for lg in logs)          # (every code gets a probability below: 53 of them need 64 cells)
        w.compressed(lits, _fit_codes(w, seqs, modes), lit=lit, modes=tuple(modes), logs=logs, low=EVERY_CODE, rng=rng, **kw)
    n = len(w.out)
    single = w.need_window() <= n and rng.randrange(2) == 0
    widths = [b for b in ((1, 2, 4, 8) if single else (0, 2, 4, 8)) if b in (0, 4, 8) or (b == 1 and n < 256) or (b == 2 and 256 <= n < 65792)]
    return w.finish(single=single, fcs_bytes=rng.choice(widths))


def _fit_codes(w, seqs, modes):
    """RLE mode wants one code in every sequence of the block, the predefined offset table has no code above 28 and a repeated
    table only the codes it was written with: `modes` is changed in place to a mode that can carry the sequences drawn"""
    r = list(w.rep)
    coded = []
    for ll, ml, off in seqs:
        ofv = -off if off < 0 else off + 3
        zm.resolve_offsets([(ll, ml, ofv)], r)
        coded.append((ll_code(ll)[0], ofv.bit_length() - 1, ml_code(ml)[0]))
    for t in range(3):
        used = set(c[t] for c in coded)
        if modes[t] == "rle" and len(used) != 1:
            modes[t] = "fse"
        if modes[t] == "repeat" and not used <= set(w.tables[t].by_sym):
            modes[t] = "fse"
        if modes[t] == "predef" and not used <= set(predefined()[t].by_sym):
            modes[t] = "fse"
    return seqs
