"""The step-geometry mirror and the periodic positional-popcount oracle of the epoch-regime tests (steps_oracle.py), on the CPU:
the mirror covers every step once and restates the launchers' and kernels' arithmetic, the oracle agrees with oracle.pospopcnt."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from steps_oracle import EPOCH, STAGGER, STEP_WORDS, WAVES, StepSplit, k1_starts, periodic_pospopcnt  # noqa: E402


def _source(*parts):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, *parts)) as f:
        return re.sub(r"\s+", " ", f.read())


def test_step_mirror_covers_every_step_once():
    rng = np.random.RandomState(41)
    cases = [(a, n, g) for a in range(0, 16, 2) for n, g in ((1, 1), (7, 3), (16384, 1), (16384 - 3, 2), (16385, 2),
                                                             (2 * 16384 - 5, 1), (2 * 16384 - 5, 7), (255 * 16384, 7))]
    cases += [(2 * int(rng.randint(8)), int(rng.randint(1, 40 * 16384)), int(rng.randint(1, 12))) for _ in range(300)]
    for addr, n, grid in cases:
        for plain in (False, True):
            s = StepSplit(addr, n, grid, plain)
            assert s.grid == min(grid, s.nsteps) and s.hi == s.lo + n
            assert s.nsteps * STEP_WORDS >= s.hi > (s.nsteps - 1) * STEP_WORDS
            every = [st for b in range(s.grid) for st in s.pushes(b)]
            assert sorted(every) == list(range(s.nsteps)), (addr, n, grid, plain)
            assert s.counts().sum() == s.nsteps
            # every workgroup gets floor or ceil of nsteps / grid steps
            assert s.counts().max() - s.counts().min() <= 1 + (0 if plain else 1), (addr, n, grid)
            if not plain:
                # steps outside [fast_begin, fast_end) are exactly the edge steps, and they come first
                for b in range(s.grid):
                    p = s.pushes(b)
                    edges = [st for st in p if not s.fast_begin <= st < s.fast_end]
                    assert p[:len(edges)] == edges and len(edges) <= 2
                    assert p[len(edges):] == sorted(p[len(edges):])


def test_step_mirror_flush_points():
    assert StepSplit.flush_points(254) == [] and StepSplit.flush_points(255) == [255]
    assert StepSplit.flush_points(510) == [255, 510] and StepSplit.flush_points(509) == [255]
    assert [StepSplit.flush_points(63, s) for s in k1_starts(True)] == [[], [], [], [63]]
    assert [StepSplit.flush_points(300, s) for s in k1_starts(True)] == [[255], [191], [127], [63]]
    assert k1_starts(False) == [0] * WAVES
    s = StepSplit(0, 64 * STEP_WORDS, 1)
    assert s.counts().tolist() == [64] and s.seam_offsets(k1_starts(True)) == {-191, -127, -63, 1}
    assert s.flushes(0, 192) == [63] and s.flushes(0, 0) == []


def test_periodic_pospopcnt_matches_the_oracle(oracle_mod):
    rng = np.random.RandomState(43)
    for _ in range(60):
        period = int(rng.randint(1, 300))
        pat = rng.randint(0, 65536, period).astype(np.uint16)
        phase = int(rng.randint(0, 2 * period))
        a = int(rng.randint(0, 3000))
        b = a + int(rng.randint(0, 3000))
        x = np.resize(np.roll(pat, -phase), b + 1)
        assert np.array_equal(periodic_pospopcnt(pat, a, b, phase), oracle_mod.pospopcnt(x[a:b])), (period, phase, a, b)
    # all-ones: every bit counts every word
    assert (periodic_pospopcnt(np.array([0xFFFF], dtype=np.uint16), 3, (1 << 33) + 3) == 1 << 33).all()


def test_step_mirror_matches_the_sources():
    """The mirror restates the launchers' and the kernels' arithmetic: if either changes, this test names what to update."""
    k1h = _source("libflagstats_amd", "csrc", "flagstat_kernels.h")
    k1 = _source("libflagstats_amd", "csrc", "flagstat_kernels.hip")
    core = _source("libflagstats_amd", "csrc", "flagstat_count_core.h")
    pos = _source("libflagstats_amd", "csrc", "flagstat_pospopcnt.hip")
    threads = int(re.search(r"constexpr int kThreads = (\d+);", k1h).group(1))
    unroll = int(re.search(r"constexpr int kUnroll = (\d+);", k1h).group(1))
    assert threads == 64 * WAVES
    assert "constexpr int kVecPerStep = kThreads * kUnroll;" in k1h and threads * unroll * 8 == STEP_WORDS
    assert (1 << int(re.search(r"constexpr int kPosDepth = (\d+);", pos).group(1))) - 1 == EPOCH
    assert "if (blk == (1u << kPosDepth) - 1u) { pos_flush(s); blk = 0; }" in pos
    # K1: DEPTH 8 on every shipped schedule, the flush test, the stagger start
    for case in ("case 9: e = launch_count_t<8, true, false, true>(a, stream);",
                 "case 25: e = launch_count_t<8, true, false, true, 1>(a, stream);",
                 "case 71: e = launch_count_t<8, true, false, false, 9>(a, stream);"):
        assert case in k1, case
    # (the flush test and the stagger start live once in flagstat_count_core.h: end_step, stagger_start; K1 calls them)
    assert core.count("if (blk == (1u << DEPTH) - 1u) { flush(s, (1u << DEPTH) - 1u); blk = 0; }") == 1
    assert "blk = __builtin_amdgcn_readfirstlane(blk); step<DEPTH, STAGE, NT, USTRIDE, HAS_NEXT>(s, v, blk, next, cur); end_step(s, blk);" in k1
    assert "tree_step<DEPTH>(s, blk, [&]" in k1 and core.count("uint32_t t8a = 0") == 1 and "t8a" not in k1
    assert core.count("return (wave & 3u) * %du;" % STAGGER) == 1
    assert "uint32_t blk = (mode & 16) ? stagger_start(wave) : 0u;" in k1
    assert "if (g_epoch_stagger.load()) a.mode |= 16;" in k1
    # the launchers' geometry (K1 keeps it in CountArgs a.*)
    for src, p in ((pos, ""), (k1, "a.")):
        for rule in ("const uint64_t nvec = (%shi + 7) / 8;" % p,
                     "%sfast_begin = (%slo == 0) ? 0 : 1;" % (p, p),
                     "%sfast_end = (%shi / 8) / " % (p, p),
                     "if (%sfast_end < %sfast_begin) %sfast_end = %sfast_begin;" % (p, p, p, p),
                     "if (static_cast<uint64_t>(grid) > %snsteps) grid = static_cast<uint32_t>(%snsteps);" % (p, p)):
            assert rule in src, rule
    assert "const uint64_t lo = (addr - base) / 2, hi = lo + n;" in pos
    assert "a.lo = (addr - base) / 2; a.hi = a.lo + n;" in k1
    # the kernels' push order: head edge, tail edge, fast steps from b (+G below fast_begin); schedule 9 one loop
    for src in (pos, k1):
        assert "if (nsteps > fast_end && nsteps - 1 >= fast_begin && (nsteps - 1) % G == blockIdx.x" in src
        assert "uint64_t st = blockIdx.x; if (st < fast_begin) st += G;" in src
    assert "if (fast_begin != 0 && blockIdx.x == 0) edge_step(0);" in pos
    assert "if (fast_begin != 0 && blockIdx.x == 0 && wave < T / 64) {" in k1
    assert "for (uint64_t st = blockIdx.x; st < nsteps; st += G) {" in k1
    assert pos.index("edge_step(0);") < pos.index("edge_step(nsteps - 1);") < pos.index("if (st < fast_end) {")
