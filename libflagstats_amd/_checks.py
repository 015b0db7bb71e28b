"""Argument checks that wide.py, where.py and filter.py share: raw-pointer integers, and the ``(out, second)`` pair of result
tensors of the torch entries (``second``: the high-bit mask or the selected count).  Every check raises ``ValueError``."""
from __future__ import annotations

import numpy as np


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
