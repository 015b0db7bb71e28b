"""The selected-elements flagstat (fsk_launch_where, csrc/flagstat_where.hip) mirrored in pure Python: the launcher's geometry,
the selection bytes a launch may read, and the two encodings of a boolean mask as the tests lay them out.

Expected counters never come from the code under test: ``want_counters`` is oracle.flagstat_c of ``values[mask]`` (superset
slots from oracle.samtools_counts and the definition), ``selected`` is ``int(mask.sum())``."""
import numpy as np

from steps_oracle import StepSplit

BITMAP, BYTES = 1, 8


def where_geometry(address: int, n: int, sel_offset: int, sel_bits: int, grid: int) -> list:
    """what fsk_where_geometry returns in geo[0..8) for n > 0: K1's step split of (address, n, grid), then the first selection
    byte that holds an element's bit or byte and one past the last, as offsets from the selection pointer"""
    assert sel_bits in (BITMAP, BYTES) and n > 0
    s = StepSplit(address % 16, n, grid)
    if sel_bits == BITMAP:
        first, end = sel_offset // 8, (sel_offset + n - 1) // 8 + 1
    else:
        first, end = sel_offset, sel_offset + n
    return [s.lo, s.hi, s.nsteps, s.fast_begin, s.fast_end, s.grid, first, end]


def selection_bytes(n: int, sel_offset: int, sel_bits: int) -> np.ndarray:
    """sorted offsets of the selection bytes that hold the bit (bitmap) or byte of an element 0 <= i < n, element by element"""
    i = np.arange(n, dtype=np.uint64) + np.uint64(sel_offset)
    return np.unique(i >> np.uint64(3) if sel_bits == BITMAP else i)


def pack(mask: np.ndarray, bit_offset: int = 0, fill: int = 1) -> np.ndarray:
    """the mask as an LSB-first bitmap whose bit ``bit_offset + i`` is mask[i]; the unused bits of its first and last byte are
    ``fill``"""
    m = np.asarray(mask, dtype=bool)
    nbits = bit_offset + m.size
    bits = np.full((nbits + 7) // 8 * 8, bool(fill))
    bits[bit_offset:nbits] = m
    return np.packbits(bits, bitorder="little")


def want_counters(oracle_mod, values: np.ndarray, mask: np.ndarray, superset: bool = False) -> np.ndarray:
    """uint64[32] of values[mask]"""
    x = np.ascontiguousarray(np.asarray(values, dtype=np.uint16)[np.asarray(mask, dtype=bool)])
    if x.size == 0:
        return np.zeros(32, dtype=np.uint64)
    c = oracle_mod.flagstat_c(x).astype(np.uint64)
    if superset:
        pa = oracle_mod.samtools_counts(x)["n_pair_all"]
        c[0], c[16] = pa[0], pa[1]
        c[9] = x.size - int(c[25])
    return c
