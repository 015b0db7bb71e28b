"""The selected-elements flagstat of int32 / int64 columns (fsk_launch_wide_where, csrc/flagstat_wide_where.hip) mirrored in pure
Python: the launcher's geometry, the selection bytes a launch may read, the addresses its fast path forms, and the expected
results.

Expected values never come from the code under test: the counters are oracle.flagstat_c of ``(values[mask] & 0xFFFF)`` (superset
slots as where_oracle.want_counters derives them), ``selected`` is ``int(mask.sum())``, ``high`` the OR of ``values[mask]`` with
the low 16 bits cleared -- of the SELECTED elements only."""
import numpy as np

import where_oracle
from steps_oracle import StepSplit
from where_oracle import BITMAP, BYTES, pack, selection_bytes  # noqa: F401  (re-exported)

UNSIGNED = {4: np.uint32, 8: np.uint64}
VPS, WAVE_VECS, US, UNROLL, LANES, WAVES = 2048, 512, 64, 8, 64, 4   # vectors per step / per wave, a lane's stride, its vectors


def step_elems(W: int) -> int:
    """S: elements of a 32 KiB step"""
    return VPS * 16 // W


def row_elems(W: int) -> int:
    """R: elements of one wave's row of 64 vectors"""
    return LANES * 16 // W


def wide_where_geometry(address: int, n: int, W: int, sel_offset: int, sel_bits: int, grid: int) -> list:
    """what fsk_wide_where_geometry returns in geo[0..8) for n > 0: the step split of (address, n * W bytes, grid) in elements,
    then the first selection byte that holds an element's bit or byte and one past the last, as offsets from the selection"""
    assert W in (4, 8) and sel_bits in (BITMAP, BYTES) and n > 0
    s = StepSplit(address % 16, n * W // 2, grid)
    if sel_bits == BITMAP:
        first, end = sel_offset // 8, (sel_offset + n - 1) // 8 + 1
    else:
        first, end = sel_offset, sel_offset + n
    return [s.lo * 2 // W, s.hi * 2 // W, s.nsteps, s.fast_begin, s.fast_end, s.grid, first, end]


def fast_vectors(geo, first_step=None) -> np.ndarray:
    """grid vector indices of every fast step (from step `first_step` on, where given): all of their positions are elements"""
    begin = geo[3] if first_step is None else max(geo[3], first_step)
    return np.arange(begin * VPS, max(geo[4], begin) * VPS, dtype=np.int64)


def fast_path_bitmap_model(geo, W: int, sel_offset: int):
    """The bitmap form's fast-path addresses, derived as the kernel derives them (the header of flagstat_wide_where.hip): for every
    vector j of a fast step the byte offset (from the selection pointer) of the first byte its lane loads, whether its bits
    straddle two bytes, and the shift at which its bits lie in what it loaded.  Returns (j, first, d, sh, funnel): arrays over the
    fast vectors.  Not funnelled: the lane loads the one byte ``first`` = k.  Funnelled: it loads the two bytes ``first`` and
    ``first + 1``, where ``first`` = k + d - 1, and the launch runs step 0 through the guarded path whatever the step split says."""
    EPV = 16 // W
    lo = geo[0]
    bit0 = sel_offset + 8 - lo
    base = (bit0 >> 3) - 1                  # the kernel's `sel` as an offset from the selection pointer
    shift = bit0 & 7
    funnel = shift != 0
    j = fast_vectors(geo, 1 if funnel else None)
    in_step = j % VPS
    lane_vec = (in_step // WAVE_VECS) * WAVE_VECS + in_step % LANES      # wave * 512 + lane
    u = (in_step % WAVE_VECS) // US
    step = j // VPS
    lane_bit = lane_vec * EPV + shift
    d = (((lane_bit & 7) + EPV > 8) & funnel).astype(np.int64)
    k = base + step * (VPS * EPV // 8) + u * (US * EPV // 8) + (lane_bit >> 3)
    if funnel:
        return j, k + d - 1, d, (lane_bit & 7) + 8 * (1 - d), funnel
    return j, k, d, lane_bit & 7, funnel


def fast_path_bytes_model(geo, W: int, sel_offset: int):
    """The byte form's fast-path addresses: (j, first, count) -- vector j loads `count` = 16 / W bytes from offset first[j]"""
    EPV = 16 // W
    j = fast_vectors(geo)
    return j, sel_offset - geo[0] + j * EPV, EPV


def low16(values: np.ndarray) -> np.ndarray:
    v = np.ascontiguousarray(values)
    return (v.view(UNSIGNED[v.dtype.itemsize]) & 0xFFFF).astype(np.uint16)


def want(oracle_mod, values: np.ndarray, mask: np.ndarray, superset: bool = False):
    """(uint64[32] counters, selected, high) of ``values`` (a 4-byte or 8-byte integer array) under the boolean ``mask``"""
    m = np.asarray(mask, dtype=bool)
    v = np.ascontiguousarray(values)
    u = v.view(UNSIGNED[v.dtype.itemsize])
    c = where_oracle.want_counters(oracle_mod, low16(v), m, superset=superset)
    picked = u[m]
    high = int(np.bitwise_or.reduce(picked & ~u.dtype.type(0xFFFF))) if picked.size else 0
    return c, int(m.sum()), high


def poison(W: int):
    """an element that must never be counted: low 16 bits 0xFFFF and every bit above bit 15 set"""
    return UNSIGNED[W](np.iinfo(UNSIGNED[W]).max)
