"""Intensity normalisation of device-resident volumes (csrc/intensity.hip): the step between a volume as stored
and the volume a network was trained on, next to resampling.

    stats = intensity_stats(train_volumes, masks=[label > 0 for label in labels])     # a CT data-set fingerprint, pooled exactly
    ct    = CTWindow.from_stats(stats)                                                 # clip to (p0.5, p99.5), (x - mean) / std
    x     = ZScore(mask="nonzero")(mri)                                                # per channel, over the non-zero mask
    pred  = GridPredictor(model, ..., normalize=ct, target_spacing=...).predict(volume_i16, spacing=...)

Volumes are C x D x H x W or D x H x W, float32, float16, int16 or uint8, on the device.  A voxel of channel c is a MEMBER of the
statistics iff the mask (uint8 / bool D x H x W, shared by the channels; None: every voxel) is non-zero there and the value is not
NaN.  Order statistics are exact (a radix select over integer histograms: bit-equal to np.sort(members)[rank], repeatable); mean
and std are two-pass fp64 (np.std's population form); the apply pass is pinned in fp32:
    y = (min(max(x, lo), hi) - sub) * mul, each operation rounded on its own; outside the mask and at a NaN: fill.
Nothing here waits for the device except IntensityStats.to_host() and the box of crop_to_nonzero."""
from __future__ import annotations

import math

import torch

from . import _lib as L
from . import _volume as V

MAX_RANKS = L.INTENSITY_MAX_RANKS
_DTYPES = {torch.float32: L.F32, torch.float16: L.F16, torch.int16: L.I16, torch.uint8: L.U8}
_OUT = {torch.float32: L.F32, torch.float16: L.F16}


# ---------------------------------------------------------------------------------------------- operands
def _volume(vol, who):
    """-> (C x D x H x W contiguous, whether a channel axis was added)"""
    if not torch.is_tensor(vol):
        raise TypeError(f"{who}: a tensor expected, got {type(vol).__name__}")
    L.require_gpu(vol, who)
    if vol.dim() not in (3, 4):
        raise ValueError(f"{who}: a C x D x H x W or D x H x W volume expected, got shape {tuple(vol.shape)}")
    if vol.dtype not in _DTYPES:
        raise ValueError(f"{who}: a float32, float16, int16 or uint8 volume expected, got {vol.dtype}")
    added = vol.dim() == 3
    vol = vol[None] if added else vol
    if vol.numel() == 0:
        raise ValueError(f"{who}: an empty volume, shape {tuple(vol.shape)}")
    return (vol if vol.is_contiguous() else vol.contiguous()), added


def _mask(mask, vol, who):
    """None, "nonzero" or a uint8 / bool D x H x W tensor -> None or a dense uint8 mask of vol's grid"""
    if mask is None:
        return None
    if isinstance(mask, str):
        if mask != "nonzero":
            raise ValueError(f"{who}: mask {mask!r} (supported: None, \"nonzero\", a D x H x W tensor)")
        return nonzero_mask(vol)
    m = V.volume_u8(mask, who)
    if tuple(m.shape) != tuple(vol.shape[1:]) or m.device != vol.device:
        raise ValueError(f"{who}: mask {tuple(m.shape)} on {m.device} does not match the volume's grid {tuple(vol.shape[1:])} on {vol.device}")
    return m


def _percentiles(percentiles, who):
    ps = tuple(float(p) for p in percentiles)
    if not 1 <= len(ps) <= MAX_RANKS // 2:
        raise ValueError(f"{who}: {len(ps)} percentiles (1 .. {MAX_RANKS // 2}: two ranks each, at most {MAX_RANKS} ranks)")
    for p in ps:
        if not (0.0 <= p <= 100.0):       # (a NaN fails both)
            raise ValueError(f"{who}: percentile {p!r} outside [0, 100]")
    return ps


# ---------------------------------------------------------------------------------------------- the entries
def nonzero_mask(vol, return_box=False):
    """vol C x D x H x W or D x H x W -> uint8 D x H x W: 1 where any channel is non-zero (a NaN counts as non-zero).
    return_box=True: also the inclusive box as int32[6] = (z0, y0, x0, z1, y1, x1) ON THE DEVICE; an all-zero volume gives
    (0, 0, 0, -1, -1, -1)."""
    v, _ = _volume(vol, "nonzero_mask")
    c, d, h, w = v.shape
    mask = torch.empty((d, h, w), dtype=torch.uint8, device=v.device)
    box = torch.empty((6,), dtype=torch.int32, device=v.device)
    L.check(L.lib().mednet_nonzero_mask(v.data_ptr(), _DTYPES[v.dtype], c, d, h, w, mask.data_ptr(), box.data_ptr(), L.stream()),
            "nonzero_mask")
    return (mask, box) if return_box else mask


def crop_to_nonzero(vol, *others, margin=0):
    """-> (vol cropped to the box of its non-zero mask, every tensor of `others` cropped alike, box).  The results are VIEWS; box is
    the tuple (z0, y0, x0, z1, y1, x1), inclusive, widened by `margin` voxels and clamped at the border.  An all-zero volume is
    returned whole.  Reading the box synchronises with the device: it decides shapes on the host."""
    margin = int(margin)
    if margin < 0:
        raise ValueError(f"crop_to_nonzero: margin {margin} (at least 0)")
    _volume(vol, "crop_to_nonzero")
    for o in others:
        if not torch.is_tensor(o) or tuple(o.shape[-3:]) != tuple(vol.shape[-3:]):
            raise ValueError(f"crop_to_nonzero: every other tensor must end in the volume's grid {tuple(vol.shape[-3:])}")
    _, box = nonzero_mask(vol, return_box=True)
    z0, y0, x0, z1, y1, x1 = (int(v) for v in box.tolist())     # the one synchronisation
    d, h, w = vol.shape[-3:]
    if z1 < 0:
        z0, y0, x0, z1, y1, x1 = 0, 0, 0, d - 1, h - 1, w - 1
    z0, y0, x0 = max(z0 - margin, 0), max(y0 - margin, 0), max(x0 - margin, 0)
    z1, y1, x1 = min(z1 + margin, d - 1), min(y1 + margin, h - 1), min(x1 + margin, w - 1)
    cut = lambda t: t[..., z0:z1 + 1, y0:y1 + 1, x0:x1 + 1]
    return (cut(vol),) + tuple(cut(o) for o in others) + ((z0, y0, x0, z1, y1, x1),)


def _cases(vols, masks, who):
    """-> [(volume C x D x H x W, mask or None)], equal channel counts"""
    one = torch.is_tensor(vols)
    vols = [vols] if one else list(vols)
    if not vols:
        raise ValueError(f"{who}: no volume")
    if masks is None or isinstance(masks, str):
        masks = [masks] * len(vols)
    elif one and torch.is_tensor(masks):
        masks = [masks]
    else:
        masks = list(masks)
    if len(masks) != len(vols):
        raise ValueError(f"{who}: {len(masks)} masks for {len(vols)} volumes")
    out = []
    for v, m in zip(vols, masks):
        v, _ = _volume(v, who)
        if out and (v.shape[0] != out[0][0].shape[0] or v.device != out[0][0].device):
            raise ValueError(f"{who}: volumes with {out[0][0].shape[0]} and {v.shape[0]} channels (or on two devices) cannot be pooled")
        out.append((v, _mask(m, v, who)))
    return out


def _flags(i, n):
    return (L.INTENSITY_FIRST if i == 0 else 0) | (L.INTENSITY_LAST if i == n - 1 else 0)


def _moments(cases, passes=(0, 1)):
    """The statistics table (int64 C x 5 holding MEDNET_INTENSITY_TABLE_BYTES per row) of the pooled members."""
    lib, dev, c = L.lib(), cases[0][0].device, cases[0][0].shape[0]
    table = torch.empty((c, L.INTENSITY_TABLE_BYTES // 8), dtype=torch.int64, device=dev)
    ws = L.workspace(max(lib.mednet_intensity_moments_ws_bytes(*v.shape) for v, _ in cases), dev)
    for p in passes:
        for i, (v, m) in enumerate(cases):
            L.check(lib.mednet_intensity_moments(v.data_ptr(), _DTYPES[v.dtype], L.ptr(m), *v.shape, p, _flags(i, len(cases)),
                                                 table.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()), "intensity_moments")
    return table


def _select(cases, ranks, who="order_statistics"):
    """ranks int64 C x R (device) -> (fp32 C x R, counts int64 C x 2 = (n, n_nan)) over the pooled members"""
    lib, dev = L.lib(), cases[0][0].device
    c, r = ranks.shape
    out = torch.empty((c, r), dtype=torch.float32, device=dev)
    counts = torch.empty((c, 2), dtype=torch.int64, device=dev)
    ws = L.workspace(lib.mednet_intensity_select_ws_bytes(c, r), dev)
    for level in range(3):
        for i, (v, m) in enumerate(cases):
            L.check(lib.mednet_intensity_select(v.data_ptr(), _DTYPES[v.dtype], L.ptr(m), *v.shape, ranks.data_ptr(), r, out.data_ptr(),
                                                counts.data_ptr(), level, _flags(i, len(cases)), ws.data_ptr(), ws.numel(), L.stream()),
                    who)
    return out, counts


def order_statistics(vol, ranks, mask=None):
    """-> fp32 C x len(ranks) on the device: for every channel the values with exactly these zero-based ranks among its members,
    bit-equal to np.sort(members)[rank].  vol: a volume, or a list of volumes pooled exactly (mask: a list alike).  ranks: up to 8
    integers (the same for every channel), or an int64 C x R tensor on the device.  A rank outside [0, n) gives NaN."""
    cases = _cases(vol, mask, "order_statistics")
    c, dev = cases[0][0].shape[0], cases[0][0].device
    if torch.is_tensor(ranks):
        L.require_gpu(ranks, "order_statistics")
        if ranks.dtype != torch.int64 or ranks.dim() != 2 or ranks.shape[0] != c:
            raise ValueError(f"order_statistics: ranks as a tensor are int64 {c} x R, got {tuple(ranks.shape)} {ranks.dtype}")
        rk = ranks.contiguous()
    else:
        rk = [int(r) for r in ranks]
        if rk:
            rk = torch.tensor([rk] * c, dtype=torch.int64).to(dev, non_blocking=True)
    n = rk.shape[1] if torch.is_tensor(rk) else 0
    if not 1 <= n <= MAX_RANKS:
        raise ValueError(f"order_statistics: {n} ranks (1 .. {MAX_RANKS})")
    return _select(cases, rk)[0]


class IntensityStats:
    """Per-channel statistics of the members, as device tensors: n, n_nan (int64 C), min, max (fp32 C), mean, std (fp64 C),
    percentiles (fp64 C x P: the values at `q`), order (fp32 C x P x 2: the two order statistics behind each) and frac (fp64 C x P:
    the interpolation weight between them).  to_host() is the only transfer."""
    FIELDS = ("n", "n_nan", "min", "max", "mean", "std", "percentiles", "order", "frac")

    def __init__(self, q, **fields):
        self.q = tuple(float(v) for v in q)
        for k in self.FIELDS:
            setattr(self, k, fields[k])

    def to_host(self):
        """The same with every tensor on the host (one synchronisation)."""
        return IntensityStats(self.q, **{k: getattr(self, k).cpu() for k in self.FIELDS})

    def __repr__(self):
        return f"IntensityStats(q={self.q}, channels={self.n.shape[0]}, device={self.n.device})"


def _table_fields(table):
    return dict(n=table[:, 0], n_nan=table[:, 1], min=table[:, 2:3].view(torch.float32)[:, 0], max=table[:, 2:3].view(torch.float32)[:, 1],
                mean=table[:, 3].view(torch.float64), std=table[:, 4].view(torch.float64))


def _ranks(table, ps):
    lib, c = L.lib(), table.shape[0]
    ranks = torch.empty((c, 2 * len(ps)), dtype=torch.int64, device=table.device)
    frac = torch.empty((c, len(ps)), dtype=torch.float64, device=table.device)
    q4 = ps + (0.0,) * (4 - len(ps))
    L.check(lib.mednet_intensity_ranks(table.data_ptr(), c, *q4, len(ps), ranks.data_ptr(), frac.data_ptr(), L.stream()), "intensity_ranks")
    return ranks, frac


def _params(scheme, table, order, frac, nq, c, eps, dev, want_pct=False):
    lib = L.lib()
    out = torch.empty((c, 4), dtype=torch.float32, device=dev) if scheme != L.INTENSITY_PERCENTILES else None
    pct = torch.empty((c, nq), dtype=torch.float64, device=dev) if want_pct else None
    L.check(lib.mednet_intensity_params(scheme, L.ptr(table), L.ptr(order), L.ptr(frac), nq, c, float(eps), L.ptr(pct), L.ptr(out),
                                        L.stream()), "intensity_params")
    return out, pct


def intensity_stats(vols, masks=None, percentiles=(0.5, 99.5)):
    """vols: a volume or a list of volumes with equal channel counts, pooled exactly (no concatenated tensor); masks: None,
    "nonzero" (each case's own non-zero mask), a mask, or a list alike -> IntensityStats of the members, on the device."""
    ps = _percentiles(percentiles, "intensity_stats")
    cases = _cases(vols, masks, "intensity_stats")
    c, dev = cases[0][0].shape[0], cases[0][0].device
    table = _moments(cases)
    ranks, frac = _ranks(table, ps)
    order, _ = _select(cases, ranks, "intensity_stats")
    _, pct = _params(L.INTENSITY_PERCENTILES, None, order, frac, len(ps), c, 0.0, dev, want_pct=True)
    return IntensityStats(ps, percentiles=pct, order=order.view(c, len(ps), 2), frac=frac, **_table_fields(table))


def apply_table(vol, table, mask=None, fill=0.0, dtype=torch.float16, out=None, who="intensity_apply"):
    """One pass: y = (min(max(x, lo), hi) - sub) * mul with the rows (lo, hi, sub, mul) of table (fp32 C x 4, device); voxels
    outside the mask and NaN voxels get `fill`.  out: a contiguous tensor of vol's shape (vol itself for equal dtypes)."""
    v, added = _volume(vol, who)
    c, d, h, w = v.shape
    if out is not None:
        dtype = out.dtype
    if dtype not in _OUT:
        raise ValueError(f"{who}: dtype {dtype} (supported: float32, float16)")
    if table.dtype != torch.float32 or tuple(table.shape) != (c, 4) or table.device != v.device or not table.is_contiguous():
        raise ValueError(f"{who}: table must be contiguous fp32 {c} x 4 on {v.device}, got {tuple(table.shape)} {table.dtype}")
    m = _mask(mask, v, who)
    if out is None:
        res = torch.empty(tuple(v.shape), dtype=dtype, device=v.device)
    else:
        res = V.like_volume(out[None] if (added and out.dim() == 3) else out, v, dtype, who,
                            f"out must be a contiguous {dtype} tensor of shape {tuple(vol.shape)} on {v.device}")
    L.check(L.lib().mednet_intensity_apply(v.data_ptr(), _DTYPES[v.dtype], res.data_ptr(), _OUT[dtype], L.ptr(m), c, d, h, w,
                                           table.data_ptr(), float(fill), L.stream()), who)
    return res[0] if added else res


# ---------------------------------------------------------------------------------------------- schemes
class _Scheme:
    """Common to the three schemes: fill and dtype, the mask argument, pickling as plain attributes."""

    def __init__(self, fill, dtype, who):
        if dtype not in _OUT:
            raise ValueError(f"{who}: dtype {dtype} (supported: float32, float16)")
        self.fill, self.dtype = float(fill), dtype

    @staticmethod
    def _check_mask(mask, who, tensors=True):
        if mask is None or (isinstance(mask, str) and mask == "nonzero") or (tensors and torch.is_tensor(mask)):
            return mask
        raise ValueError(f"{who}: mask {mask!r} (supported: None, \"nonzero\"" + (", a D x H x W tensor)" if tensors else ")"))

    def __call__(self, vol, out=None):
        raise NotImplementedError


class ZScore(_Scheme):
    """(x - mean) / max(std, eps) per channel, the statistics taken over the mask's members of THIS volume; outside the mask: fill."""

    def __init__(self, mask=None, eps=1e-8, fill=0.0, dtype=torch.float16):
        super().__init__(fill, dtype, "ZScore")
        self.mask, self.eps = self._check_mask(mask, "ZScore"), float(eps)

    def __call__(self, vol, out=None):
        v, _ = _volume(vol, "ZScore")
        m = _mask(self.mask, v, "ZScore")
        table = _moments([(v, m)])
        params, _ = _params(L.INTENSITY_ZSCORE, table, None, None, 0, v.shape[0], self.eps, v.device)
        return apply_table(vol, params, m, self.fill, self.dtype, out, "ZScore")


class Rescale(_Scheme):
    """Clip to the two percentiles of the mask's members of THIS volume, then (x - lo) / max(hi - lo, eps): [0, 1]."""

    def __init__(self, percentiles=(0.5, 99.5), mask=None, eps=1e-8, fill=0.0, dtype=torch.float16):
        super().__init__(fill, dtype, "Rescale")
        self.percentiles = _percentiles(percentiles, "Rescale")
        if len(self.percentiles) != 2 or self.percentiles[0] > self.percentiles[1]:
            raise ValueError(f"Rescale: percentiles {self.percentiles} (a lower and an upper one)")
        self.mask, self.eps = self._check_mask(mask, "Rescale", tensors=False), float(eps)

    def __call__(self, vol, out=None):
        v, _ = _volume(vol, "Rescale")
        m = _mask(self.mask, v, "Rescale")
        table = _moments([(v, m)], passes=(0,))       # n for the ranks
        ranks, frac = _ranks(table, self.percentiles)
        order, _ = _select([(v, m)], ranks, "Rescale")
        params, _ = _params(L.INTENSITY_RESCALE, None, order, frac, 2, v.shape[0], self.eps, v.device)
        return apply_table(vol, params, m, self.fill, self.dtype, out, "Rescale")


class CTWindow(_Scheme):
    """nnU-Net's CT scheme from data-set numbers: clip to (lower, upper), then (x - mean) / max(std, eps), the same for every case.
    Numbers or per-channel sequences; the apply table is computed in fp64 and rounded to fp32 once, on the host, at construction."""

    def __init__(self, lower, upper, mean, std, eps=1e-8, fill=0.0, dtype=torch.float16):
        super().__init__(fill, dtype, "CTWindow")
        cols = [list(v) if isinstance(v, (list, tuple)) else [v] for v in (lower, upper, mean, std)]
        if len({len(col) for col in cols}) != 1:
            raise ValueError("CTWindow: lower, upper, mean and std need the same number of channels")
        self.lower, self.upper, self.mean, self.std = (tuple(float(v) for v in col) for col in cols)
        self.eps = float(eps)
        for lo, hi in zip(self.lower, self.upper):
            if not lo <= hi:
                raise ValueError(f"CTWindow: window ({lo}, {hi}) is empty or NaN")
        self._tables = {}

    @classmethod
    def from_stats(cls, stats, channel=None, **kw):
        """The window (first percentile, second percentile) with mean and std of an IntensityStats (one synchronisation unless it is
        on the host already); channel: one channel's numbers for a one-channel scheme, None: every channel."""
        s = stats.to_host()
        if s.percentiles.shape[1] < 2:
            raise ValueError("CTWindow.from_stats: the statistics need two percentiles (lower, upper)")
        pick = range(s.n.shape[0]) if channel is None else [int(channel)]
        return cls([float(s.percentiles[k, 0]) for k in pick], [float(s.percentiles[k, 1]) for k in pick],
                   [float(s.mean[k]) for k in pick], [float(s.std[k]) for k in pick], **kw)

    def table(self):
        """fp32 C x 4 (lo, hi, sub, mul) on the host"""
        rows = [[lo, hi, mu, 1.0 / max(sd, self.eps)] for lo, hi, mu, sd in zip(self.lower, self.upper, self.mean, self.std)]
        return torch.tensor(rows, dtype=torch.float64).to(torch.float32)

    def __getstate__(self):
        return {k: v for k, v in self.__dict__.items() if k != "_tables"}

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._tables = {}

    def __call__(self, vol, out=None):
        v, _ = _volume(vol, "CTWindow")
        if v.shape[0] != len(self.lower):
            raise ValueError(f"CTWindow: a scheme for {len(self.lower)} channels on a volume with {v.shape[0]}")
        t = self._tables.get(v.device)
        if t is None:         # (uploaded once per device)
            t = self._tables[v.device] = self.table().to(v.device)
        return apply_table(vol, t, None, self.fill, self.dtype, out, "CTWindow")


def normalize(vol, scheme, out=None):
    """scheme(vol): the normalised volume as the scheme's dtype (out: written there)."""
    if not isinstance(scheme, _Scheme):
        raise TypeError(f"normalize: a ZScore, CTWindow or Rescale expected, got {type(scheme).__name__}")
    return scheme(vol, out=out)
