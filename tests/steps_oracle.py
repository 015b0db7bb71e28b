"""The step geometry of K1 (fsk_launch, flagstat_kernels.hip) and of the positional popcount (fsk_launch_pospopcnt,
flagstat_pospopcnt.hip), mirrored for the epoch-regime tests, and a periodic positional-popcount oracle.

Both launchers derive the same values from (pointer, n, grid): the caller's words occupy [lo, hi) of the 16-byte aligned grid,
``nsteps`` steps of 16,384 words cover it, steps in [fast_begin, fast_end) lie fully inside it, and the grid is clamped to
``nsteps``.  A workgroup b then pushes, in this order: the head edge step 0 (b == 0, when lo != 0), the tail edge step
nsteps - 1 (b == (nsteps - 1) % G), then its fast steps b (+G if b < fast_begin), b + G, ... below fast_end.  K1's plain
schedule 9 pushes st = b, b + G, ... below nsteps instead.  Every wave of a workgroup pushes every step of it; wave w starts its
epoch count at ``start`` (0; 64 * w under K1's epoch stagger) and flushes when the count reaches 255.
test_steps_host.py::test_step_mirror_matches_the_sources reads these values and rules back out of the sources."""
import numpy as np

STEP_WORDS = 16384       # kVecPerStep * 8: kThreads (256) lanes x kUnroll (8) vectors x 8 words
WAVES = 4                # kThreads / 64
EPOCH = 255              # (1 << kPosDepth) - 1 == (1 << DEPTH) - 1 for DEPTH 8: pushes between in-loop flushes
STAGGER = 64             # K1 mode bit 4: wave w starts its first epoch at (w & 3) * 64


def k1_starts(stagger: bool):
    """the epoch count each wave of a K1 workgroup starts at"""
    return [(w & 3) * STAGGER if stagger else 0 for w in range(WAVES)]


class StepSplit:
    """The steps of one launch over ``n`` words whose first word lies ``addr_mod_16`` bytes past a 16-byte boundary, on a
    requested grid of ``grid`` workgroups.  ``plain``: K1's schedule 9 (one loop over every step, no separate edge steps)."""

    def __init__(self, addr_mod_16: int, n: int, grid: int, plain: bool = False):
        assert addr_mod_16 % 2 == 0 and n > 0 and grid > 0
        self.lo = (addr_mod_16 % 16) // 2
        self.hi = self.lo + n
        self.n = n
        nvec = (self.hi + 7) // 8
        self.nsteps = (nvec + STEP_WORDS // 8 - 1) // (STEP_WORDS // 8)
        self.fast_begin = 0 if self.lo == 0 else 1
        self.fast_end = max((self.hi // 8) // (STEP_WORDS // 8), self.fast_begin)
        self.grid = min(grid, self.nsteps)
        self.plain = plain
        G = self.grid
        self.head_edge = self.fast_begin != 0
        self.tail_edge = self.nsteps > self.fast_end and self.nsteps - 1 >= self.fast_begin
        self.tail_block = (self.nsteps - 1) % G if self.tail_edge else None
        self._pushes = []
        for b in range(G):
            if plain:
                steps = list(range(b, self.nsteps, G))
            else:
                steps = []
                if self.head_edge and b == 0:
                    steps.append(0)
                if self.tail_edge and b == self.tail_block:
                    steps.append(self.nsteps - 1)
                st = b + G if b < self.fast_begin else b
                steps += list(range(st, self.fast_end, G))
            self._pushes.append(steps)

    def pushes(self, b: int) -> list:
        """workgroup b's steps, in the order it pushes them"""
        return self._pushes[b]

    def counts(self) -> np.ndarray:
        """pushes per workgroup"""
        return np.array([len(p) for p in self._pushes], dtype=np.int64)

    @staticmethod
    def flush_points(pushes: int, start: int = 0) -> list:
        """after which pushes (1-based) a wave that starts its count at ``start`` flushes in the loop"""
        assert 0 <= start < EPOCH
        return list(range(EPOCH - start, pushes + 1, EPOCH))

    def flushes(self, b: int, start: int = 0) -> list:
        return self.flush_points(len(self._pushes[b]), start)

    def seam_offsets(self, starts) -> set:
        """{last push - first in-loop flush point} over every (workgroup, wave with this start): -1 = the flush would have come
        one push later, 0 = the last push flushes, +1 = one push after the flush"""
        out = set()
        for c in self.counts():
            for s in starts:
                out.add(int(c) - (EPOCH - s))
        return out


def periodic_pospopcnt(pattern, a: int, b: int, phase: int = 0) -> np.ndarray:
    """uint64[16]: exact positional popcount of x[a:b] for x[i] = pattern[(i + phase) % P], in O(P): per bit, the count over
    [0, t) is (t // P) * (count over one period) + (count over the period's first t % P)."""
    p = np.roll(np.ascontiguousarray(pattern, dtype=np.uint16).ravel(), -int(phase))
    period = p.size
    out = np.zeros(16, dtype=np.uint64)
    if b <= a:
        return out
    for j in range(16):
        pre = np.concatenate([[0], np.cumsum((p >> np.uint16(j)) & np.uint16(1), dtype=np.int64)])
        upto = lambda t: (t // period) * int(pre[-1]) + int(pre[t % period])  # noqa: E731
        out[j] = upto(int(b)) - upto(int(a))
    return out
