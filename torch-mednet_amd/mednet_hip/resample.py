"""Resampling of device-resident volumes between voxel grids (csrc/resample.hip): a case comes from its native
spacing to the spacing the network was trained at, and the prediction goes back.

    net_vol = resample(volume, spacing=(2.5, 0.8, 0.8), target_spacing=(1, 1, 1))        # anti-aliased where it shrinks
    labels  = resample_argmax(probabilities, size=volume.shape[1:])                       # uint8 D x H x W at the native grid
    seg     = resample_labels(seg_u8, size=..., num_classes=4)                            # one-hot linear, without the one-hot tensor

Resampling is separable and table-driven: `axis_table` states the arithmetic of one axis once, on the host, in fp64, and the
kernels only execute it.

Conventions.  Output index i sits at source coordinate s = (i + 0.5) * (n_in / n_out) - 0.5: pixel centres are aligned, the
align_corners=False rule of torch / skimage / PIL; the scale is n_in / n_out, never the spacing ratio.  Kinds: "nearest" (one tap
floor(s + 0.5), clamped), "linear" (triangle filter), "cubic" (Keys kernel, a = -0.5).  antialias=True stretches the filter by the
scale where n_in > n_out (support x scale, argument / scale) and changes nothing elsewhere.  Border: a tap outside [0, n_in) is
folded onto the edge voxel (edge replication) -- its weight is added to the edge tap, nothing is renormalised away; the row is
then normalised by its sum in fp64 and rounded to fp32 once."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from . import _volume as V

KINDS = ("nearest", "linear", "cubic")
MAX_TAPS = 64
MAX_CLASSES = 256
_DTYPES = {torch.float32: L.F32, torch.float16: L.F16, torch.uint8: L.U8}


# ---------------------------------------------------------------------------------------------- host side: sizes and tables
def output_size(shape, spacing, target_spacing):
    """max(1, floor(n * sp / tsp + 0.5)) per axis."""
    shape, spacing, target_spacing = tuple(shape), tuple(spacing), tuple(target_spacing)
    if not (len(shape) == len(spacing) == len(target_spacing) == 3):
        raise ValueError(f"output_size: three extents and two spacings of three expected, got {shape}, {spacing}, {target_spacing}")
    for sp in spacing + target_spacing:
        if not (math.isfinite(float(sp)) and float(sp) > 0):
            raise ValueError(f"output_size: spacing {sp!r} is not finite and positive")
    return tuple(max(1, int(math.floor(int(n) * float(sp) / float(tsp) + 0.5))) for n, sp, tsp in zip(shape, spacing, target_spacing))


def _filter(kind, x):
    x = np.abs(x)
    if kind == "linear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x <= 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))


def axis_table(n_in, n_out, kind="linear", antialias=True):
    """-> (start int32[n_out], count int32[n_out], weight fp32[n_out][taps], taps): output i reads the source indices
    [start[i], start[i] + count[i]) with the weights weight[i, :count[i]]; unused slots are 0 and are never read by the kernels."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"axis_table: extents {n_in} -> {n_out} (both at least 1)")
    if kind not in KINDS:
        raise ValueError(f"axis_table: kind {kind!r} (supported: {', '.join(KINDS)})")
    scale = n_in / n_out
    rows = []
    for i in range(n_out):
        s = (i + 0.5) * scale - 0.5
        if kind == "nearest":
            rows.append((min(max(int(math.floor(s + 0.5)), 0), n_in - 1), np.ones(1)))
            continue
        stretch = scale if (antialias and n_in > n_out) else 1.0
        radius = (1.0 if kind == "linear" else 2.0) * stretch
        lo, hi = int(math.floor(s - radius)), int(math.ceil(s + radius))
        j = np.arange(lo, hi + 1)
        wj = _filter(kind, (j - s) / stretch)
        first, last = min(max(lo, 0), n_in - 1), min(max(hi, 0), n_in - 1)
        w = np.zeros(last - first + 1)
        np.add.at(w, np.clip(j, first, last) - first, wj)           # the fold: an outside tap's weight goes to the edge tap
        nz = np.flatnonzero(w)
        first, w = first + int(nz[0]), w[nz[0]:nz[-1] + 1]            # (zero weights at either end are no taps)
        rows.append((first, w / w.sum()))
    taps = max(len(w) for _, w in rows)
    if taps > MAX_TAPS:
        raise ValueError(f"axis_table: {n_in} -> {n_out} {kind} needs {taps} taps (at most {MAX_TAPS})")
    start = np.array([r[0] for r in rows], dtype=np.int32)
    count = np.array([len(r[1]) for r in rows], dtype=np.int32)
    weight = np.zeros((n_out, taps), dtype=np.float32)
    for i, (_, w) in enumerate(rows):
        weight[i, :len(w)] = w.astype(np.float32)
    return start, count, weight, taps


def is_identity(table):
    start, count, weight, _ = table
    return bool((count == 1).all() and (start == np.arange(len(start))).all() and (weight[:, 0] == 1.0).all())


_tables = {}


def device_table(n_in, n_out, kind, antialias, device):
    """The table of an axis on `device`, cached per (n_in, n_out, kind, antialias, device): (start, count, weight, taps, identity)."""
    key = (int(n_in), int(n_out), kind, bool(antialias), torch.device(device))
    hit = _tables.get(key)
    if hit is None:
        t = axis_table(n_in, n_out, kind, antialias)
        hit = tuple(torch.from_numpy(a).to(device) for a in t[:3]) + (t[3], is_identity(t))
        _tables[key] = hit
    return hit


# ---------------------------------------------------------------------------------------------- the entries
def resample_axis(src, axis, table, dtype=None):
    """One pass: src C x D x H x W (f32 / f16 / u8, contiguous, device) -> the same with extent `axis` (0, 1, 2 within D x H x W)
    replaced by the table's length, as `dtype` (src's by default)."""
    start, count, weight, taps = table[:4]
    c, d, h, w = src.shape
    shape = [c, d, h, w]
    shape[1 + axis] = int(start.numel())
    out = torch.empty(tuple(shape), dtype=dtype or src.dtype, device=src.device)
    L.check(L.lib().mednet_resample_axis(src.data_ptr(), _DTYPES[src.dtype], out.data_ptr(), _DTYPES[out.dtype], c, d, h, w, int(axis),
                                         shape[1 + axis], start.data_ptr(), count.data_ptr(), weight.data_ptr(), int(taps), L.stream()),
            "resample_axis")
    return out


def _size_of(shape, size, spacing, target_spacing, who):
    if (size is None) == (spacing is None and target_spacing is None):
        raise ValueError(f"{who}: give either size= or spacing= with target_spacing=")
    if size is None:
        if spacing is None or target_spacing is None:
            raise ValueError(f"{who}: spacing= and target_spacing= go together")
        return output_size(shape, spacing, target_spacing)
    size = tuple(int(v) for v in size)
    if len(size) != 3 or min(size) < 1:
        raise ValueError(f"{who}: size {size} (three extents, each at least 1)")
    return size


def _volume(vol, who):
    """-> (C x D x H x W contiguous, whether a channel axis was added)"""
    L.require_gpu(vol, who)
    if vol.dim() not in (3, 4):
        raise ValueError(f"{who}: a C x D x H x W or D x H x W volume expected, got shape {tuple(vol.shape)}")
    if vol.dtype not in _DTYPES:
        raise ValueError(f"{who}: a float32, float16 or uint8 volume expected, got {vol.dtype}")
    added = vol.dim() == 3
    vol = vol[None] if added else vol
    return (vol if vol.is_contiguous() else vol.contiguous()), added


def resample(vol, size=None, spacing=None, target_spacing=None, kind="linear", antialias=True, dtype=None):
    """vol C x D x H x W or D x H x W (f16 / f32 / u8, device) -> the same at `size` (or at output_size(shape, spacing,
    target_spacing)), as `dtype` (vol's by default).  Passes over axes 2, 1, 0 with fp32 between them; an axis whose table is the
    identity is skipped; if every axis is, the result is a copy (bit-equal for equal dtypes)."""
    v, added = _volume(vol, "resample")
    dtype = dtype or v.dtype
    if dtype not in _DTYPES:
        raise ValueError(f"resample: dtype {dtype} (supported: float32, float16, uint8)")
    size = _size_of(v.shape[1:], size, spacing, target_spacing, "resample")
    todo = []
    for axis in (2, 1, 0):
        t = device_table(v.shape[1 + axis], size[axis], kind, antialias, v.device)
        if not t[4]:
            todo.append((axis, t))
    if not todo:
        if dtype == v.dtype:
            out = v.clone()
        else:   # the kernel's store converts: one pass with an identity table
            out = resample_axis(v, 2, device_table(v.shape[3], v.shape[3], kind, antialias, v.device), dtype)
    else:
        out = v
        for k, (axis, t) in enumerate(todo):
            out = resample_axis(out, axis, t, dtype if k == len(todo) - 1 else torch.float32)
    return out[0] if added else out


def _argmax(src, ncls, size, kind, antialias, return_max, who):
    d, h, w = src.shape[-3:]
    tz, ty, tx = (device_table(n, m, kind, antialias, src.device) for n, m in zip((d, h, w), size))
    out = torch.empty(size, dtype=torch.uint8, device=src.device)
    best = torch.empty(size, dtype=torch.float32, device=src.device) if return_max else None
    L.check(L.lib().mednet_resample_argmax(src.data_ptr(), _DTYPES[src.dtype], int(ncls), d, h, w, out.data_ptr(), L.ptr(best), *size,
                                           *(a for t in (tz, ty, tx) for a in (t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3])),
                                           L.stream()), who)
    return (out, best) if return_max else out


def resample_argmax(scores, size=None, spacing=None, target_spacing=None, kind="linear", antialias=True, return_max=False):
    """scores classes x D x H x W (f32 / f16, device: probabilities, logits, any score) -> uint8 D' x H' x W': the arg-max class of the
    resampled scores (the first maximum, the lowest class on ties), in ONE pass over the output -- no class volume at the output
    size.  return_max=True: also the winning scores (fp32).  Equal, bit for bit, to torch.argmax over resample(scores, dtype=float32)
    of fp32 passes (every axis run, the identity ones too)."""
    L.require_gpu(scores, "resample_argmax")
    if scores.dim() != 4 or scores.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"resample_argmax: float32 / float16 scores classes x D x H x W expected, got {tuple(scores.shape)} {scores.dtype}")
    if not 1 <= scores.shape[0] <= MAX_CLASSES:
        raise ValueError(f"resample_argmax: {scores.shape[0]} classes (1 .. {MAX_CLASSES})")
    if kind not in ("linear", "cubic"):
        raise ValueError(f"resample_argmax: kind {kind!r} (supported: linear, cubic)")
    size = _size_of(scores.shape[1:], size, spacing, target_spacing, "resample_argmax")
    src = scores if scores.is_contiguous() else scores.contiguous()
    return _argmax(src, src.shape[0], size, kind, antialias, return_max, "resample_argmax")


def resample_labels(vol, size=None, spacing=None, target_spacing=None, num_classes=None, kind="linear", antialias=True):
    """vol uint8 D x H x W (device) -> uint8 D' x H' x W'.  "linear": the arg-max of the linearly resampled one-hot planes of the
    classes 0 .. num_classes - 1, computed from the label volume itself (a label >= num_classes scores for nobody); "nearest": one
    tap per axis, exact."""
    vol = V.volume_u8(vol, "resample_labels")
    if kind not in ("linear", "nearest"):
        raise ValueError(f"resample_labels: kind {kind!r} (supported: linear, nearest)")
    size = _size_of(vol.shape, size, spacing, target_spacing, "resample_labels")
    if kind == "nearest":
        return resample(vol, size=size, kind="nearest")
    if num_classes is None or not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"resample_labels: num_classes {num_classes!r} (1 .. {MAX_CLASSES})")
    return _argmax(vol, int(num_classes), size, "linear", antialias, False, "resample_labels")
