"""The test-only LZ4 block writer (tests/lz4_block_writer.py) held against liblz4 and the product's host decoder, and the two Python
restatements of the GPU decoder's workgroup kernel -- the walker (tests/test_lz4_walker_model.py) and what comes behind it
(tests/lz4_gpu_model.py) -- held against the writer's blocks: valid LZ4 that no compressor writes, with tokens, matches and literal
runs placed on the kernel's own boundaries.  No GPU: what these tests prove is that the blocks the GPU tests feed the decoders
(tests/test_gpu_decode_bytes.py) are what they are named for (every case proves its placement from its layout and the model's
tiles), that the census below reaches every path, and that the model the kernel was written against decodes them -- and stops
doing so, or stops agreeing with the placement, when one of its constants is off by one.
The reference decodes every payload with LZ4_decompress_safe (benchmark/flagstats.cpp:316): that call is the yardstick here."""
import bisect
import collections
import functools
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import blockfile_tool as bt  # noqa: E402
import lz4_block_writer as bw  # noqa: E402
import lz4_gpu_model as gm  # noqa: E402
import test_lz4_walker_model as wm  # noqa: E402

CSRC = os.path.join(os.path.dirname(HERE), "libflagstats_amd", "csrc")
FUZZ_SEEDS = range(0, 200)

# Every path of the workgroup kernel the model tells apart.  The hand-placed families must reach each in at least three blocks.
CENSUS = ["windows plain", "windows batch", "windows of more than one batch", "windows with a literal run at the ring's end",
          "scalar records", "literal pieces of 64", "carries taken", "chunks that are all carry", "chunks that read across the ring's end",
          "tiles ended by an exit of 12 or more", "tiles that advance nothing",
          "stop: literal length bytes", "stop: match length byte 255", "stop: 8 or more length bytes (the walker drains the queue)"] + \
         ["chunks with in-chunk pointers, %d round%s" % (r, "" if r == 1 else "s") for r in range(1, 9)]


def ref(comp, usize):
    r = bt.decompress_block_ref(bytes(comp), usize)
    return r if r is not None and len(r) == usize else None


def host(comp, usize):
    from libflagstats_amd import blockfile
    r = blockfile.lz4_block_decode(bytes(comp), usize)
    return r if r is not None and len(r) == usize else None


def test_the_writers_constants_are_the_kernels():
    src = open(os.path.join(CSRC, "flagstat_lz4_kernels.hip")).read()
    pipe = open(os.path.join(CSRC, "flagstat_wgpipe.h")).read()
    for text in ("kWgSeg = %d, kWgTileSegs = %d;" % (bw.SEG, bw.TILE_SEGS), "if (i < %d) {" % bw.EXIT_TAB, "e2 >= %du" % bw.EXIT_TAB,
                 "(iend - ip - %du) / kWgSeg + 1u" % bw.TAIL, "kWgInw = %d, kWgInPad = %d;" % (bw.IN_RING, bw.IN_PAD),
                 "while (ll > %du) {" % bw.LIT_PIECE, "kWgSpan = %d;" % bw.SPAN, "kWgChunk = %d;" % bw.CHUNK, "kWgMR = %d;" % bw.MARK_SLOTS,
                 "kWgK = %d;" % bw.FSRC_SLOTS, "kWgNR = %d;" % bw.OUT_RING, "kWgQ = %d;" % bw.QUEUE, "kWgFlush = %d;" % bw.FLUSH,
                 "(ll > %du) | (ri + 4u > kWgNR)" % bw.PLAIN_LIT, "s_carry[%d]" % bw.CARRIES):
        assert text in src, text
    assert "for (int round = 0; round < %d; ++round)" % bw.ROUNDS in pipe and "s_carry[kc & %du]" % (bw.CARRIES - 1) in pipe
    assert (wm.SEG, wm.SEGS, wm.TAB, wm.TAIL) == (bw.SEG, bw.TILE_SEGS, bw.EXIT_TAB, bw.TAIL)
    assert (gm.RING, gm.CHUNK, gm.MARKS, gm.CARRIES, gm.PIECE) == (bw.OUT_RING, bw.CHUNK, bw.MARK_SLOTS, bw.CARRIES, bw.LIT_PIECE)
    assert gm.DEFAULT == dict(span=bw.SPAN, plain_lit=bw.PLAIN_LIT, rounds=bw.ROUNDS, emit_ring=bw.OUT_RING)


def test_padding_lands_where_it_is_told():
    rng = random.Random(1)
    for _ in range(300):
        b = bw.start(rng.getrandbits(30))
        di = rng.choice([0, 3, 4, 5, 7, 18, 19, 64, 500])
        if rng.random() < 0.5:
            b.pad(ip=b.ip + di, maxlen=rng.choice([11, 18]))
            assert b.ip == 11 + di
        elif di:
            do = rng.randint(bw._min_out(di), min(bw._max_out(di), 40 * di))
            b.pad(ip=b.ip + di, op=b.op + do)
            assert (b.ip, b.op) == (11 + di, 16 + do)
        else:
            do = rng.choice([0, 4, 5, 7, 19, 300])
            b.pad(op=b.op + do)
            assert b.op == 16 + do
        comp, dec, layout = b.end(12)
        assert ref(comp, len(dec)) == dec
        assert all(4 <= s.ml and s.ll <= 14 and (s.ml <= 18 + 255) for s in layout[1:-1])      # fillers are window-form


# ------------------------------------------------------------------------------------------------------ placement proofs
def expected_form(seqs):
    """what the emitter's three conditions give for a window of these sequences, from the writer's layout and constants alone"""
    total = sum(s.ll + s.ml for s in seqs)
    plain = total <= bw.SPAN and all(s.ll <= bw.PLAIN_LIT for s in seqs) and all(s.op % bw.OUT_RING + 4 <= bw.OUT_RING for s in seqs if s.ll)
    return "plain" if plain else "batch", total


def prove(name, comp, dec, layout, claims, tiles, detail):
    by_ip = {s.ip: s for s in layout}
    where = {}
    for t, (tip, members, adv, stopped) in enumerate(tiles):
        for p in members:
            where[p] = (t, (p - tip) // bw.SEG, (p - tip) % bw.SEG)
    stops = {tip + adv: (t, adv // bw.SEG, adv % bw.SEG) for t, (tip, members, adv, stopped) in enumerate(tiles) if stopped}
    # every window of every tile: the model's form and output against the layout's
    starts = [tl[0] for tl in tiles]
    for w0, (form, total, op, ring_end) in detail.items():
        t = bisect.bisect_right(starts, w0) - 1
        mem = tiles[t][1]
        seqs = [by_ip[p] for p in mem[bisect.bisect_left(mem, w0):bisect.bisect_left(mem, w0 + bw.WINDOW)]]
        assert (form, total) == expected_form(seqs), (name, "window at", w0, form, total, expected_form(seqs))
        assert not seqs or seqs[0].op == op, (name, "window at", w0, "output position")
    window = lambda p: detail[tiles[where[p][0]][0] + (p - tiles[where[p][0]][0]) // bw.WINDOW * bw.WINDOW]  # noqa: E731
    for claim in claims:
        kind, a = claim[0], claim[1:]
        s = layout[a[0]] if kind not in ("size", "csize", "last_match_from_end", "last_literals", "bare_run") else None
        if kind == "token_at":
            assert where.get(s.ip, (None,))[1:] == (a[1], a[2]), (name, claim, where.get(s.ip), stops.get(s.ip))
        elif kind == "stop_at":
            assert stops.get(s.ip, (None,))[1:] == (a[1], a[2]), (name, claim, stops.get(s.ip), where.get(s.ip))
        elif kind == "scalar":
            assert s.ip not in where, (name, claim, where.get(s.ip))
        elif kind == "stop":
            assert s.ip in stops, (name, claim)
        elif kind == "tile_ended_by_exit":
            ended = [tl for tl in tiles if tl[0] + tl[2] == s.ip and not tl[3]]
            assert ended and ended[0][2] == bw.SEG * (a[1] + 1) + a[2] and where[s.ip][1:] == (0, 0), (name, claim, ended[:1], where.get(s.ip))
        elif kind == "short_tile":
            tip = tiles[where[s.ip][0]][0]
            assert (len(comp) - tip - bw.TAIL) // bw.SEG + 1 < bw.TILE_SEGS, (name, claim)
        elif kind == "in_near":
            assert 0 < a[1] - s.ip <= a[2] and a[1] % bw.IN_RING == 0 and s.ip in where, (name, claim, s.ip)
        elif kind == "match_at":
            assert (s.op + s.ll) % bw.CHUNK == a[1], (name, claim, s)
        elif kind == "match_end":
            assert (s.op + s.ll + s.ml) % bw.CHUNK == a[1], (name, claim, s)
        elif kind == "match_pos":
            assert s.op + s.ll == a[1], (name, claim, s)
        elif kind == "lit_covers":
            assert s.op <= a[1] < s.op + s.ll and a[1] % bw.OUT_RING == bw.OUT_RING - 1, (name, claim, s)
            if s.op % bw.OUT_RING + 4 > bw.OUT_RING:
                assert window(s.ip)[3], (name, claim, "the window is not a ring-end one")
        elif kind == "window_out":
            assert window(s.ip)[1] == a[1] and window(s.ip)[0] == ("plain" if a[1] <= bw.SPAN else "batch"), (name, claim, window(s.ip))
        elif kind == "window_lit":
            assert s.ll == a[1] and s.ip in where and window(s.ip)[0] == ("plain" if s.ll <= bw.PLAIN_LIT else "batch"), (name, claim)
        elif kind == "period":
            assert s.off == a[1] and s.ml > s.off, (name, claim)
        elif kind == "chain":
            ch = layout[a[0]:a[1] + 1]
            assert len(ch) == a[2] and ch[0].op // bw.CHUNK == (ch[-1].op + ch[-1].ml - 1) // bw.CHUNK, (name, claim)
            assert all(c.ll == 0 and c.op - c.off >= prev.op for prev, c in zip(ch, ch[1:])), (name, claim)
        elif kind == "size":
            assert len(dec) == a[0], (name, claim)
        elif kind == "csize":
            assert len(comp) == a[0], (name, claim)
        elif kind == "last_match_from_end":
            assert len(dec) - layout[-2].op - layout[-2].ll == a[0], (name, claim)
        elif kind == "last_literals":
            assert layout[-1].ll == a[0] and layout[-1].ml == 0, (name, claim)
        elif kind == "literal_only":
            assert len(layout) == 1, (name, claim)
        elif kind == "bare_run":
            run = best = 0
            for q in layout:
                run = run + 1 if q.ll == 0 and 4 <= q.ml <= 18 else 0
                best = max(best, run)
            assert best >= a[0], (name, claim, best)
        else:
            raise AssertionError(("unknown claim", claim))


def check_case(case, **model):
    """liblz4, the host decoder, the walker model with its assertions, the back-end model, the placement: the case's census"""
    name, comp, dec, layout, claims = case
    assert ref(comp, len(dec)) == dec, (name, "liblz4")
    assert host(comp, len(dec)) == dec, (name, "the host decoder")
    at = 0
    for s in layout:       # the layout is the block's: positions, lengths and offsets as a parse of the bytes finds them
        ll, _, off, ml, nxt, _, _ = gm.parse(comp, s.ip)
        assert (s.ip, s.ll, s.off, s.ml) == (at, ll, off, ml), (name, "layout", s)
        at = nxt
    assert at == len(comp)
    tiles = wm.check_stream(comp, name)
    detail = {}
    got, census = gm.decode(comp, len(dec), tiles, detail=detail, **model)
    assert got == dec, (name, "the back-end model's bytes")
    prove(name, comp, dec, layout, claims, tiles, detail)
    return census


@functools.lru_cache(maxsize=None)
def family(name):
    return bw.FAMILIES[name]()


@functools.lru_cache(maxsize=None)
def family_census(name):
    return [check_case(c) for c in family(name)]


@pytest.mark.parametrize("name", list(bw.FAMILIES))
def test_hand_placed_blocks_decode_and_sit_where_they_are_named_for(name):
    assert list(bw.FAMILIES) == ["segments", "stops", "literals", "span", "chunks", "tails", "ends", "wave"]
    cases = family(name)
    assert len({c[0] for c in cases}) == len(cases), "two cases of one name"
    assert all(len(c[2]) <= bw.BLOCK_MAX for c in cases)
    family_census(name)


def test_the_families_reach_every_path_of_the_model_in_three_blocks():
    blocks = collections.Counter()
    total = collections.Counter()
    for name in bw.FAMILIES:
        for census in family_census(name):
            total.update(census)
            blocks.update(k for k, v in census.items() if v)
    for k in sorted(total):
        print("%-66s %8d in %4d blocks" % (k, total[k], blocks[k]))
    for k in CENSUS:
        assert blocks[k] >= 3, (k, blocks[k])


def test_rejected_blocks_are_refused_by_liblz4_and_by_the_host_decoder():
    """one defect each.  (offset 0: liblz4 1.9.3's LZ4_decompress_safe does not check it and copies from the match's own first
    byte, so only the product's decoders are held to it)"""
    cases = bw.rejected()
    names = [n for n, _, _ in cases]
    assert len(set(names)) == len(names) and all(any(n.startswith(d) for n in names) for d in bw.END_DEFECTS)
    for name, comp, usize in cases:
        if not name.startswith("offset 0"):
            assert ref(comp, usize) is None, (name, "liblz4 decodes it")
        assert host(comp, usize) is None, (name, "the host decoder decodes it")
    # what stays valid: literals only, of any length, and the empty block
    for n in (0, 1, 4, 5, 11, 12, 13, 300):
        comp, dec, _ = bw.Block(n).end(n)
        assert ref(comp, n) == dec and host(comp, n) == dec, n
    assert ref(b"\0", 0) == b"" and host(b"\0", 0) == b""


def test_random_blocks_from_the_same_vocabulary():
    total = collections.Counter()
    for seed in FUZZ_SEEDS:
        comp, dec, layout = bw.random_block(random.Random(seed), big=False)      # (the GPU tests take the seeds at full size)
        total.update(check_case(("random_block seed %d" % seed, comp, dec, layout, [])))
    print(dict(total))
    assert total["windows plain"] and total["windows batch"] and total["scalar records"] and total["carries taken"]


# ---------------------------------------------------------------------------------------------------- deliberate model errors
# Each is a constant of the model moved by one, applied by parameter.  The named family must notice: wrong bytes, a failed
# assertion of the walker model, or a placement proof that no longer holds.  Whether the liblz4-written corpus of
# test_walker_tiles_follow_the_token_chain notices is printed beside it (it has no layout: wrong bytes or a failed assertion).
ERRORS = [("span threshold 385", "span", dict(span=385), {}),
          ("literal bound 5", "literals", dict(plain_lit=5), {}),
          ("7 doubling rounds", "chunks", dict(rounds=7), {}),
          ("ring size 67,583", "literals", dict(emit_ring=67583), {}),
          ("exit-table size 11", "segments", {}, dict(TAB=11)),
          ("tail rule 49", "tails", {}, dict(TAIL=49))]


def notices(cases, model):
    n = 0
    for case in cases:
        try:
            check_case(case, **model)
        except AssertionError:
            n += 1
    return n


@functools.lru_cache(maxsize=None)
def liblz4_corpus(sizes=((2, 9_000),)):
    """the blocks of test_walker_tiles_follow_the_token_chain; in the suite, for the time it takes, only its 9,000-flag size under LZ4-HC (5 blocks
    of 18 KB: none reaches the output ring's end).  `python tests/test_lz4_writer_host.py` prints the record over all 30."""
    import numpy as np
    out = []
    for kind in ("na12878", "uniform", "zeros", "runs", "repeats"):
        for mode, level in (("fast", 2), ("hc", 9)) if len(sizes) > 1 else (("hc", 9),):
            for seed, n in sizes:
                raw = np.ascontiguousarray(wm.flags_like(kind, n, seed)).tobytes()
                comp = bt.compress_block(raw, mode, level)
                out.append(("%s %s %d" % (kind, mode, n), comp, raw))
    return out


def corpus_notices(model, sizes=((2, 9_000),)):
    n = 0
    for name, comp, raw in liblz4_corpus(sizes):
        try:
            got, _ = gm.decode(comp, len(raw), wm.check_stream(comp, name), **model)
            assert got == raw
        except AssertionError:
            n += 1
    return n


@pytest.mark.parametrize("what,fam,model,walker", ERRORS, ids=[e[0] for e in ERRORS])
def test_a_model_constant_off_by_one_is_noticed(monkeypatch, what, fam, model, walker):
    cases = family(fam)
    if fam == "segments":
        cases = [c for c in cases if "entry" in c[0]]
    elif fam == "chunks":
        cases = [c for c in cases if "lengths" in c[0] or "chain" in c[0]]
    elif fam == "literals":       # (a slice, for the time it takes: the window-form runs, and some of the runs at the ring's end)
        cases = [c for c in cases if "window-form" in c[0]] + [c for c in cases if "ring byte" in c[0]][::5]
    for k, v in walker.items():
        monkeypatch.setattr(wm, k, v)
    caught = notices(cases, model)
    old = corpus_notices(model)
    print("%s: %d of %d blocks of family '%s' notice it; the 9,000-flag LZ4-HC blocks of the liblz4-written corpus: %d of %d" % (what, caught, len(cases), fam, old, len(liblz4_corpus())))
    assert caught >= 1, what



if __name__ == "__main__":      # the record over the whole corpus of test_walker_tiles_follow_the_token_chain (a minute or two)
    ALL = ((1, 60_000), (2, 9_000), (3, 150_000))
    for what, fam, model, walker in ERRORS:
        saved = {k: getattr(wm, k) for k in walker}
        for k, v in walker.items():
            setattr(wm, k, v)
        try:
            print("%s: the liblz4-written corpus notices it in %d of %d blocks" % (what, corpus_notices(model, ALL), len(liblz4_corpus(ALL))), flush=True)
        finally:
            for k, v in saved.items():
                setattr(wm, k, v)
