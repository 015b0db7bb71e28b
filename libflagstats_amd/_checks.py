"""What the entries of the fifteen derived modules (``wide``, ``where``, ``filter`` and their combinations, flat and
``segments_*``) share besides the value checks they take from one another: the C entries' ``flags`` bits, raw-pointer integers,
the tensor checks that belong to no one module (a 16-bit tensor, device offsets), the result tensors of the torch entries -- the
flat ``(out, second)`` pair and the per-segment rows with their trailing words -- the numpy results of the host entries, and the
strict / ``"high_bits"`` shaping of the ``flagstats_*ints*`` functions.  Every check raises ``ValueError``."""
from __future__ import annotations

import numpy as np

STORE, SUPERSET = 1, 2   # the C entry points' `flags` bits


def c_flags(store, superset) -> int:
    return (STORE if store else 0) | (SUPERSET if superset else 0)


def check_int(name: str, x) -> None:
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        raise ValueError("%s must be an int, not %s" % (name, type(x).__name__))


def check_raw_ints(named, non_negative=("n",)) -> None:
    """``named``: ``(name, value)`` pairs that go to the C entries as unsigned 64-bit integers.  All must be ints; those listed in
    ``non_negative`` get a message of their own when negative; all must fit."""
    for name, x in named:
        check_int(name, x)
    for name, x in named:
        if name in non_negative and x < 0:
            raise ValueError("%s must not be negative" % name)
    for name, x in named:
        if not 0 <= x < 1 << 64:
            raise ValueError("%s must fit an unsigned 64-bit integer, not %d" % (name, x))


def check_elem_bytes(elem_bytes, u16_function: str) -> None:
    """the element width of a raw device pointer to wide elements; ``u16_function`` takes a pointer to 16-bit ones"""
    if elem_bytes not in (4, 8):
        raise ValueError("elem_bytes must be 4 or 8 (16-bit arrays: %s), not %r" % (u16_function, elem_bytes))


def check_u16_tensor(t) -> None:
    """``t`` is a 1-D contiguous ``int16`` / ``uint16`` tensor (where it lives is the placement's business)"""
    import torch

    if not isinstance(t, torch.Tensor):
        raise ValueError("t must be a torch.Tensor, not %s" % type(t).__name__)
    if t.dtype not in (torch.int16, torch.uint16):
        raise ValueError("t must have dtype int16 or uint16, not %s" % t.dtype)
    if t.dim() != 1 or not t.is_contiguous():
        raise ValueError("t must be 1-D and contiguous")


def check_offsets_tensor(offsets) -> int:
    """``offsets`` is a 1-D contiguous ``int64`` tensor of nseg + 1 >= 1 values (its order is the kernel's business: checking it
    would synchronise); returns nseg"""
    import torch

    if not (isinstance(offsets, torch.Tensor) and offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.is_contiguous()
            and offsets.numel() >= 1):
        raise ValueError("offsets must be a 1-D contiguous int64 tensor (nseg + 1 values)")
    return offsets.numel() - 1


def check_result_pair(out, second_name: str, second) -> None:
    """a given ``out`` is a contiguous int64 tensor of 32 elements, a given second tensor one of 1 element"""
    import torch

    for name, x, numel in (("out", out, 32), (second_name, second, 1)):
        if x is not None and not (isinstance(x, torch.Tensor) and x.dtype == torch.int64 and x.numel() == numel and x.is_contiguous()):
            raise ValueError("%s must be a contiguous int64 tensor of %d element%s" % (name, numel, "s" if numel > 1 else ""))


def place_result_pair(t, out, second_name: str, second, others=()):
    """``t`` is a CUDA tensor; ``others`` (``(name, tensor or None)`` pairs), ``out`` and the second tensor live on its device
    where given; the pair, made zeroed there where not given."""
    import torch

    if not t.is_cuda:
        raise ValueError("t must be a CUDA tensor")
    for name, x in tuple(others) + (("out", out), (second_name, second)):
        if x is not None and x.device != t.device:
            raise ValueError("%s must live on t's device (%s), not on %s" % (name, t.device, x.device))
    if out is None:
        out = torch.zeros(32, dtype=torch.int64, device=t.device)
    if second is None:
        second = torch.zeros(1, dtype=torch.int64, device=t.device)
    return out, second


def place_result_triple(t, out, selected, high, others=()):
    """the pair ``(out, selected)`` with the mask ``high`` as a third result of 1 element: checked, on ``t``'s device, made zeroed
    where not given"""
    import torch

    check_result_pair(out, "selected", selected)
    check_result_pair(None, "high", high)
    out, selected = place_result_pair(t, out, "selected", selected, others=tuple(others) + (("high", high),))
    if high is None:
        high = torch.zeros(1, dtype=torch.int64, device=t.device)
    return out, selected, high


def place_result_rows(t, nseg: int, store, results, others=()):
    """The per-segment counterpart of the pair: ``results`` are ``(name, tensor or None)`` pairs, the rows first (``(nseg, 32)``),
    then one to two tensors of one word per segment (``(nseg,)``).  The given ones are contiguous int64 tensors of their shape;
    ``t`` is a CUDA tensor; ``others`` (``(name, tensor or None)`` pairs) and the given results live on its device.  Returns the
    results, those not given made there: uninitialised with ``store`` (the entry overwrites them), zeroed without."""
    import torch

    shaped = [(name, x, (nseg, 32) if i == 0 else (nseg,)) for i, (name, x) in enumerate(results)]
    for name, x, shape in shaped:
        if x is not None and not (isinstance(x, torch.Tensor) and x.dtype == torch.int64 and tuple(x.shape) == shape and x.is_contiguous()):
            raise ValueError("%s must be a contiguous int64 tensor of shape %s" % (name, shape))
    if not t.is_cuda:
        raise ValueError("t must be a CUDA tensor")
    for name, x in tuple(others) + tuple(results):
        if x is not None and x.device != t.device:
            raise ValueError("%s must live on t's device (%s), not on %s" % (name, t.device, x.device))
    make = torch.empty if store else torch.zeros
    return [make(shape, dtype=torch.int64, device=t.device) if x is None else x for _, x, shape in shaped]


def segment_results(nseg: int, words: int):
    """the zeroed numpy results of a host entry over ``nseg`` segments: ``uint64[nseg, 32]`` rows and ``words`` ``uint64[nseg]``"""
    return [np.zeros((nseg, 32), dtype=np.uint64)] + [np.zeros(nseg, dtype=np.uint64) for _ in range(words)]


def with_high_bits(strict, high, message, make):
    """The strict / ``"high_bits"`` shaping of the ``flagstats_*ints*`` functions.  ``high``: the mask (an int) or the masks per
    segment (an array).  ``strict`` and a bit set: ``ValueError(message())``.  Else ``make()`` -- a dict, or a list of one dict per
    segment -- and, with ``strict=False``, every dict gets its mask as ``"high_bits"``."""
    if strict and np.any(high):
        raise ValueError(message())
    ret = make()
    if not strict:
        if isinstance(ret, dict):
            ret["high_bits"] = high
        else:
            for d, h in zip(ret, high.tolist()):
                d["high_bits"] = int(h)
    return ret
