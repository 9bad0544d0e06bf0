"""Operand checks the volume modules share (metrics.py, components.py): a tensor is refused here, with the caller's name in the
message, before its address reaches a kernel."""
from __future__ import annotations

import torch

from . import _lib as L


def volume_u8(t: torch.Tensor, who: str) -> torch.Tensor:
    """uint8 D x H x W, dense: a view such as the last channel of a uint8 C x D x H x W volume is read where it lies; another layout
    is copied once."""
    L.require_gpu(t, who)
    if t.dim() != 3:
        raise ValueError(f"{who}: a D x H x W volume expected, got shape {tuple(t.shape)}")
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if t.dtype != torch.uint8:
        raise ValueError(f"{who}: a uint8 volume expected, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def like_volume(t, ref: torch.Tensor, dtype, who: str, what: str, same_device: bool = True) -> torch.Tensor:
    """`t` (an out= tensor or a second operand) must be a contiguous `dtype` volume of `ref`'s shape, on its device where
    same_device; `what` is the sentence that says so in the caller's words.  None (no out= given) -> a new such volume."""
    if t is None:
        return torch.empty(tuple(ref.shape), dtype=dtype, device=ref.device)
    if t.dtype != dtype or t.shape != ref.shape or not t.is_contiguous() or (same_device and t.device != ref.device):
        raise ValueError(f"{who}: {what}")
    return t
