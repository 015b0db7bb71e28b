"""CPU: the ALGORITHM of the GPU LZ4 decoder's walker wave (flagstat_lz4_kernels.hip, lz4wg_walk), restated in Python and
checked against the true token chain of liblz4-written blocks.  The kernel finds which input bytes are tokens with one
lane per 32-byte segment of a 2 KiB tile: (1) backward over a segment's positions, the "exit" of every position -- where
a chain through it lands in the next segment, from the token alone (a sequence whose lengths sit in its token is
3 + literals (+ 1 match-length byte) long); (2) the chain through the tile, segment by segment, from a 12-entry exit table
per segment; (3) forward again, the positions reachable from each segment's entry.  Tokens whose literal length continues
in further bytes (or whose match-length byte is 255) stop the tile.  This file pins that restatement -- the tables' sizes,
the stop rules, the tile-end arithmetic, and (r05) that the prefix SCAN over the exit tables gives what the serial walk gives -- on LZ4-fast and LZ4-HC streams of flag data and on streams full of long matches
and literal runs; the HIP code itself is checked on the GPU (tests/test_gpu_blockfile.py)."""
import bisect
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import blockfile_tool as bt  # noqa: E402

SEG, SEGS, TAB = 32, 64, 12
TAIL = 50     # a tile's last position, were it the token of a sequence of 19 input bytes, has that sequence inside the block


def true_chain(comp):
    """token positions and, per token, whether the window form covers it (all lengths in the token, one length byte < 255)"""
    pos, simple, ip, n = [], {}, 0, len(comp)
    while ip < n:
        tok = comp[ip]
        ll, p, ok = tok >> 4, ip + 1, (tok >> 4) < 15
        if ll == 15:
            while True:
                e = comp[p]
                p += 1
                ll += e
                if e != 255:
                    break
        p += ll
        pos.append(ip)
        if p >= n:
            simple[ip] = False          # the last sequence: literals only
            break
        p += 2
        if (tok & 15) == 15:
            first = True
            while True:
                e = comp[p]
                p += 1
                if first and e == 255:
                    ok = False
                first = False
                if e != 255:
                    break
        simple[ip] = ok
        ip = p
    return pos, simple


def _exit_tables(buf, lanes):
    """pass (1) of walk_tile for all lanes at once (what its loop does per segment, on numpy columns): the tables as integers"""
    B = np.frombuffer(buf, dtype=np.uint8)[:SEG * lanes].reshape(lanes, SEG).astype(np.int64)
    win = np.zeros((lanes, 19), dtype=np.int64)          # (column 18 stays zero: d - 1 = 18 only under ll = 15, which is overridden)
    tab = [0] * lanes
    rows = np.arange(lanes)
    for i in range(SEG - 1, -1, -1):
        tok = B[:, i]
        ll = tok >> 4
        d = 3 + ll + ((tok & 15) == 15)
        ex = win[rows, d - 1]
        ex = np.where(d >= SEG - i, i + d - SEG, ex)
        ex = np.where(ll == 15, 31, ex)
        win[:, 1:18] = win[:, 0:17].copy()
        win[:, 0] = ex
        if i < TAB:
            for s, e in enumerate(ex.tolist()):
                tab[s] |= e << (5 * i)
    return tab


def _members(buf, ip, ent, nvalid, e_next):
    """pass (3) of walk_tile for all lanes at once (what its loop does per segment, on numpy columns), and its result"""
    W = np.lib.stride_tricks.as_strided(np.frombuffer(buf, dtype=np.uint8), shape=(nvalid, 2 * SEG), strides=(SEG, 1)).astype(np.int64)
    rows = np.arange(nvalid)
    reach = np.left_shift(1, np.array(ent[:nvalid], dtype=np.int64))
    stop = np.full(nvalid, SEG, dtype=np.int64)
    for i in range(SEG):
        tok = W[:, i]
        ll, mlc = tok >> 4, tok & 15
        on = ((reach >> i) & 1) == 1
        halt = on & ((ll == 15) | ((mlc == 15) & (W[rows, np.minimum(i + 3 + ll, 2 * SEG - 1)] == 255)))
        stop = np.where(halt, np.minimum(stop, i), stop)
        reach |= np.where(on & ~halt, np.left_shift(1, i + 3 + ll + (mlc == 15)), 0)
    members = []
    for s, (r, st) in enumerate(zip(reach.tolist(), stop.tolist())):
        members += [ip + SEG * s + i for i in range(min(st, SEG)) if (r >> i) & 1]
        if st < SEG:
            return members, SEG * s + st, True
    assert e_next < 18, "the chain saw a token for the scalar code that the members pass did not"
    return members, SEG * nvalid + e_next, False


def walk_tile(comp, ip):
    """one tile at input position ip, as the kernel does it: (members found, positions advanced, stopped at a token for the scalar code)"""
    iend = len(comp)
    nseg = min(SEGS, (iend - ip - TAIL) // SEG + 1) if iend >= ip + TAIL else 0
    if nseg == 0:
        return None
    # (the kernel computes all 64 lanes; what lanes behind the tile's last segment hold reaches nothing: the chain runs left to
    # right and is read eight segments at a time, so the model stops at the next multiple of eight)
    lanes = min(SEGS, (nseg + 7) // 8 * 8)
    buf = bytes(comp[ip:ip + SEG * lanes + 64])
    buf += bytes(SEG * lanes + 64 - len(buf))        # (what lies behind the block reads as zero)
    byte = lambda x: buf[x - ip]  # noqa: E731
    tabs = _exit_tables(buf, lanes) if lanes > 16 else []
    for s in range(0 if tabs else lanes):
        win, tab = [0] * 18, 0
        for i in range(SEG - 1, -1, -1):
            tok = byte(ip + SEG * s + i)
            ll = tok >> 4
            d = 3 + ll + (1 if (tok & 15) == 15 else 0)
            ex = win[d - 1] if d - 1 < 18 else 0
            if d >= SEG - i:
                ex = i + d - SEG
            if ll == 15:
                ex = 31
            win = [ex] + win[:17]
            if i < TAB:
                tab |= ex << (5 * i)
        tabs.append(tab)
    ent, e, nvalid, e_next = [0] * SEGS, 0, nseg, 0
    for sg in range(lanes):
        if sg % 8 == 0 and sg >= nvalid:
            break
        ent[sg] = e
        e2 = (tabs[sg] >> (5 * e)) & 31
        last = (sg + 1 == nvalid) or e2 >= TAB
        if last and sg < nvalid:
            e_next = e2
        if last:
            nvalid = min(nvalid, sg + 1)
        e = 0 if e2 >= TAB else e2
    # r05: the kernel does not walk that chain any more, it SCANS it -- lane s ends up with F(s) = T(s) o ... o T(0) after six
    # doubling rounds (a lane composes its table with the one 1, 2, 4 ... lanes to its left; an exit of 12 or more stays what it
    # is), F(s)(0) is segment s's exit, the first exit of 12 or more (or the last segment) ends the tile.  Same entries, same end.
    ident = sum(e << (5 * e) for e in range(TAB))
    F = np.array(tabs, dtype=np.uint64)              # (the lanes at once, as the kernel has them)
    u = np.uint64
    d = 1
    while d < SEGS and d < lanes:                    # (a round whose left neighbours are all the identity changes nothing)
        G = np.concatenate([np.full(min(d, lanes), ident, dtype=np.uint64), F[:max(lanes - d, 0)]])
        n = np.zeros(lanes, dtype=np.uint64)
        for en in range(TAB):
            v = (G >> u(5 * en)) & u(31)
            t = (F >> ((u(5) * v) & u(63))) & u(31)
            n |= np.where(v >= u(TAB), v, t) << u(5 * en)
        F, d = n, d * 2
    exits = [int(f) & 31 for f in F]
    last_seg = min(s for s in range(lanes) if exits[s] >= TAB or s + 1 >= nseg)
    assert last_seg + 1 == nvalid and exits[last_seg] == e_next, ("scan", ip, last_seg, nvalid, exits[last_seg], e_next)
    assert [0] + exits[:last_seg] == ent[:nvalid], ("scan entries", ip)
    members = []
    if lanes > 16:
        return _members(buf, ip, ent, nvalid, e_next)
    for s in range(nvalid):
        reach, stop = 1 << ent[s], SEG
        for i in range(SEG):
            tok = byte(ip + SEG * s + i)
            ll, mlc = tok >> 4, tok & 15
            if not (reach >> i) & 1:
                continue
            if ll == 15 or (mlc == 15 and byte(ip + SEG * s + i + 3 + ll) == 255):
                stop = min(stop, i)
                continue
            reach |= 1 << (i + 3 + ll + (1 if mlc == 15 else 0))
        got = [ip + SEG * s + i for i in range(min(stop, SEG)) if (reach >> i) & 1]
        members += got
        if stop < SEG:
            return members, SEG * s + stop, True
    assert e_next < 18, "the chain saw a token for the scalar code that the members pass did not"
    return members, SEG * nvalid + e_next, False


def check_block(raw, mode, level):
    comp = bt.compress_block(raw, mode, level)
    assert bt.decompress_block_ref(comp, len(raw)) == raw
    return len(check_stream(comp, mode, level))


def check_stream(comp, mode="written", level=0):
    """the walker's tiles over one valid block, whoever wrote it: [(tile's input position, members, positions advanced, stopped)]"""
    pos, simple = true_chain(comp)
    nxt = {p: (pos[k + 1] if k + 1 < len(pos) else len(comp)) for k, p in enumerate(pos)}
    chain = set(pos)
    ip, tiles = 0, []
    while True:
        t = walk_tile(comp, ip)
        if t is None:
            break
        members, adv, stopped = t
        end = ip + adv
        assert end in chain, (mode, level, "tile ends off the chain", ip, end)
        assert members == pos[bisect.bisect_left(pos, ip):bisect.bisect_left(pos, end)], (mode, level, "members", ip)
        assert all(simple[p] for p in members), (mode, level, "a member the window form does not cover", ip)
        if stopped:
            assert not simple[end], (mode, level, "stopped at a token the window form covers", end)
            end = nxt[end]                 # the scalar code takes that sequence
        else:
            assert adv > 0
        # what the tail rule is for: a sequence of 19 input bytes from the tile's last position would still lie inside the block
        nseg = min(SEGS, (len(comp) - ip - TAIL) // SEG + 1)
        assert ip + SEG * nseg - 1 + 19 <= len(comp), (mode, level, "the tile's last position is too close to the block's end", ip)
        tiles.append((ip, members, adv, stopped))
        ip = end
        if ip >= len(comp):
            break
    return tiles


def flags_like(kind, n, seed):
    import oracle
    rs = np.random.RandomState(seed)
    if kind == "na12878":
        return oracle.generate(oracle.GEN_NA12878, seed, 1, 0, n)
    if kind == "uniform":
        return oracle.generate(oracle.GEN_UNIFORM, seed, 0x0FFF, 0, n)
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint16)
    if kind == "runs":
        parts, left = [], n
        while left > 0:
            m = int(min(left, rs.choice([1, 3, 17, 40, 300, 5000])))
            parts.append(np.full(m, rs.randint(0, 4096), dtype=np.uint16) if rs.rand() < 0.7 else rs.randint(0, 65536, size=m).astype(np.uint16))
            left -= m
        return np.concatenate(parts)
    base = rs.randint(0, 4096, size=3000).astype(np.uint16)
    parts, left = [], n
    while left > 0:
        o, m = int(rs.randint(0, 2900)), int(min(left, rs.randint(2, 100)))
        parts.append(base[o:o + m])
        left -= len(parts[-1])
    return np.concatenate(parts)[:n]


@pytest.mark.parametrize("kind", ["na12878", "uniform", "zeros", "runs", "repeats"])
@pytest.mark.parametrize("mode,level", [("fast", 2), ("hc", 9)])
def test_walker_tiles_follow_the_token_chain(kind, mode, level):
    for seed, n in ((1, 60_000), (2, 9_000), (3, 150_000)):
        raw = np.ascontiguousarray(flags_like(kind, n, seed)).tobytes()
        check_block(raw, mode, level)


def test_kernel_constants_match_the_model():
    src = open(os.path.join(ROOT, "libflagstats_amd", "csrc", "flagstat_lz4_kernels.hip")).read()
    assert "kWgSeg = 32, kWgTileSegs = 64" in src and "if (i < 12) {" in src and "e2 >= 12u" in src and "(iend - ip - 50u) / kWgSeg + 1u" in src
