"""Patch-based inference on the device: what examples/predict.py:83-97 does around `model(inputs)`
with GridPatchSampler (midasmednet/dataset.py:349-474), without leaving HBM.

    predictor = GridPredictor(model, patch_size, patch_overlap, num_heatmaps, pad_mode="constant", batch_size=4)
    result = predictor(volume)        # volume: C x D x H x W (numpy / torch, float16 or float32) -> uint8 (H + 1) x D x H x W

The volume is uploaded once; the overlapping grid patches are gathered on the device (np.pad semantics: constant or
symmetric), run through the network in batches (forward kernels only, `torch.no_grad`), and the logits are turned into
the uint8 result -- arg-max class, heat maps clipped to 0..255 -- and stitched into the result volume by ONE kernel that
applies the reference's crop rule (including its asymmetric first-axis window, dataset.py:453).  Bit-identical to the
reference's procedure for identical logits (tests/test_gpu_predict.py).

Beyond the reference (csrc/blend.hip): GridPredictor(..., blend="gaussian", mirror_axes=(0, 1, 2)) blends
overlapping windows with an importance map instead of cropping them, averages over flips, and `predict(volume)` returns a
BlendedPrediction with .result() (the uint8 layout above), .probabilities(), .heatmaps() and .peaks()."""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from . import _lib as L

_PAD = {"constant": L.PAD_CONSTANT, "symmetric": L.PAD_SYMMETRIC}


def grid_positions(img_size, patch_size, patch_overlap):
    """Grid of dataset.py:372-389: positions (in the padded volume) of every patch, in the reference's order."""
    patch_size, img_size, ov = np.array(patch_size), np.array(img_size), np.array(patch_overlap)
    cropped = patch_size - 2 * ov
    if np.any(cropped <= 0):
        raise ValueError(f"patch_size {patch_size.tolist()} leaves nothing after removing the overlap {ov.tolist()} twice")
    n_patches = np.ceil(img_size / cropped).astype(int)
    axes = [np.arange(0, n_patches[k]) * cropped[k] for k in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32)


def crop_window(patch_size, patch_overlap):
    """(start[3], shape[3]) of the reference's `data[:, o0:-o1, o1:-o1, o2:-o2]` (dataset.py:452-455)."""
    o = [int(v) for v in patch_overlap]
    sl = [slice(o[0], -o[1]), slice(o[1], -o[1]), slice(o[2], -o[2])]
    idx = [range(int(p))[s] for p, s in zip(patch_size, sl)]
    return [r.start if len(r) else 0 for r in idx], [len(r) for r in idx]


def gather_patches(volume: torch.Tensor, pos: torch.Tensor, patch_size, patch_overlap, pad_mode="symmetric", mirror=0):
    """volume C x D x H x W fp32 (device), pos B x 3 int32 (device) -> B x C x pD x pH x pW fp32.  Bit k of `mirror` reverses
    patch axis k (test-time mirroring; 0: the reference's patches)."""
    L.require_gpu(volume, "grid_gather")
    if pad_mode not in _PAD:
        raise NotImplementedError(f"pad mode {pad_mode!r} (supported: constant, symmetric)")
    c, d, h, w = volume.shape
    pd, ph, pw = (int(v) for v in patch_size)
    out = torch.empty((pos.shape[0], c, pd, ph, pw), dtype=torch.float32, device=volume.device)
    o = [int(v) for v in patch_overlap]
    if mirror:
        L.check(L.lib().mednet_grid_gather_mirror(volume.data_ptr(), pos.data_ptr(), out.data_ptr(), pos.shape[0], c, d, h, w, pd, ph,
                                                  pw, o[0], o[1], o[2], _PAD[pad_mode], int(mirror), L.stream()), "grid_gather_mirror")
        return out
    L.check(L.lib().mednet_grid_gather(volume.data_ptr(), pos.data_ptr(), out.data_ptr(), pos.shape[0], c, d, h, w, pd, ph, pw,
                                       o[0], o[1], o[2], _PAD[pad_mode], L.stream()), "grid_gather")
    return out


def assemble(logits: torch.Tensor, pos: torch.Tensor, result: torch.Tensor, num_heatmaps, patch_overlap):
    """logits B x (H + classes) x pD x pH x pW fp32 planar -> writes uint8 result (H + 1) x D x H x W in place."""
    L.require_gpu(logits, "predict_assemble")
    lg = logits.float().contiguous()
    b, ch, pd, ph, pw = lg.shape
    _, d, h, w = result.shape
    start, shape = crop_window((pd, ph, pw), patch_overlap)
    L.check(L.lib().mednet_predict_assemble(lg.data_ptr(), pos.data_ptr(), result.data_ptr(), b, num_heatmaps, ch - num_heatmaps,
                                            d, h, w, pd, ph, pw, start[0], start[1], start[2], shape[0], shape[1], shape[2],
                                            L.stream()), "predict_assemble")
    return result


# ---------------------------------------------------------------------------------------------- blended inference
_BLEND_OF = {"probabilities": L.BLEND_PROBABILITIES, "logits": L.BLEND_LOGITS}


def blend_window(patch_size, kind="gaussian", sigma_scale=0.125):
    """Three fp32 vectors (one per patch axis) whose outer product is the patch's importance map.  "gaussian":
    exp(-0.5 * ((i - (p - 1) / 2) / (sigma_scale * p)) ** 2), computed in fp64 (nnU-Net's map up to its normalisation, which the
    division by the weight sum removes; the smallest product at p = 128 is about 5.5e-11: no clamp needed in fp32); "constant": ones."""
    if kind not in ("gaussian", "constant"):
        raise ValueError(f"blend window {kind!r} (supported: gaussian, constant)")
    out = []
    for p in (int(v) for v in patch_size):
        i = np.arange(p, dtype=np.float64)
        v = np.exp(-0.5 * ((i - (p - 1) / 2.0) / (sigma_scale * p)) ** 2) if kind == "gaussian" else np.ones(p)
        out.append(v.astype(np.float32))
    return tuple(out)


def mirror_mask(axes):
    """Patch axes (0, 1, 2) -> the kernels' mask (bit k reverses axis k)."""
    mask = 0
    for a in axes:
        if int(a) not in (0, 1, 2):
            raise ValueError(f"mirror axis {a!r} (patch axes are 0, 1, 2)")
        mask |= 1 << int(a)
    return mask


def _acc_check(acc: torch.Tensor, wsum: torch.Tensor, who: str, expected: str, channels=None):
    """acc C x D x H x W and wsum D x H x W, both contiguous fp32 (C = channels where given); `expected` ends the message."""
    if (channels is not None and acc.shape[0] != channels) or tuple(wsum.shape) != tuple(acc.shape[1:]) \
            or acc.dtype != torch.float32 or wsum.dtype != torch.float32 or not (acc.is_contiguous() and wsum.is_contiguous()):
        raise ValueError(f"{who}: acc {tuple(acc.shape)} {acc.dtype} / wsum {tuple(wsum.shape)} {wsum.dtype}{expected}")


def accumulate(logits: torch.Tensor, pos: torch.Tensor, acc: torch.Tensor, wsum: torch.Tensor, windows, num_heatmaps, patch_overlap,
               mirror=0, blend_of="probabilities"):
    """logits B x (H + classes) x pD x pH x pW -> adds the window-weighted heat maps and class probabilities (or logits) of every
    patch to acc ((H + classes) x D x H x W fp32) and the weights to wsum (D x H x W fp32), in place.  windows: three fp32 device
    vectors (blend_window); mirror: the mask the patches were gathered with (the logits are flipped back).  Bit-reproducible and
    independent of how the rows are split into calls."""
    L.require_gpu(logits, "blend_accumulate")
    lg = logits.float().contiguous()
    b, ch, pd, ph, pw = lg.shape
    _, d, h, w = acc.shape
    _acc_check(acc, wsum, "blend_accumulate", f" do not fit {ch} channels (contiguous fp32)", ch)
    if [int(t.numel()) for t in windows] != [pd, ph, pw] or any(t.dtype != torch.float32 or not t.is_contiguous() for t in windows):
        raise ValueError(f"blend_accumulate: windows must be three contiguous fp32 vectors of {pd}, {ph}, {pw} entries")
    o = [int(v) for v in patch_overlap]
    L.check(L.lib().mednet_blend_accumulate(lg.data_ptr(), pos.data_ptr(), acc.data_ptr(), wsum.data_ptr(), windows[0].data_ptr(),
                                            windows[1].data_ptr(), windows[2].data_ptr(), b, num_heatmaps, ch - num_heatmaps, d, h, w,
                                            pd, ph, pw, o[0], o[1], o[2], int(mirror), _BLEND_OF[blend_of], L.stream()),
            "blend_accumulate")
    return acc, wsum


def finalize(acc: torch.Tensor, wsum: torch.Tensor, num_heatmaps, blend_of="probabilities", result=False, probabilities=None,
             heatmaps=False):
    """One pass over the accumulators -> (result, probabilities, heatmaps), None for what was not asked for.  result=True: uint8
    (H + 1) x D x H x W in `assemble`'s layout; probabilities=torch.float32 / torch.float16: classes x D x H x W; heatmaps=True:
    H x D x H x W fp32."""
    L.require_gpu(acc, "blend_finalize")
    ch, d, h, w = acc.shape
    ncls = ch - num_heatmaps
    _acc_check(acc, wsum, "blend_finalize", ": contiguous fp32 expected")
    res = torch.empty((num_heatmaps + 1, d, h, w), dtype=torch.uint8, device=acc.device) if result else None
    prob = torch.empty((ncls, d, h, w), dtype=probabilities, device=acc.device) if probabilities is not None else None
    heat = torch.empty((num_heatmaps, d, h, w), dtype=torch.float32, device=acc.device) if heatmaps else None
    if prob is not None and prob.dtype not in (torch.float32, torch.float16):
        raise RuntimeError(f"blend_finalize: probabilities as {prob.dtype} (supported: float32, float16)")
    if res is None and prob is None and heat is not None and num_heatmaps == 0:
        return res, prob, heat  # (the heat maps of a network without any: nothing to compute)
    L.check(L.lib().mednet_blend_finalize(acc.data_ptr(), wsum.data_ptr(), L.ptr(res), L.ptr(prob), L.dt(prob) if prob is not None else L.F32,
                                          L.ptr(heat) if num_heatmaps else None, num_heatmaps, ncls, d, h, w, _BLEND_OF[blend_of],
                                          L.stream()), "blend_finalize")
    return res, prob, heat


def heatmap_peaks(heat: torch.Tensor):
    """heat H x D x H x W fp32 (device) -> (positions H x 3 int64 as (z, y, x), values H fp32): every channel's maximum, the lowest
    flat index on ties; a NaN never wins."""
    L.require_gpu(heat, "heatmap_peaks")
    ht = heat.float().contiguous()
    nh, d, h, w = ht.shape
    vox = d * h * w
    index = torch.empty((nh,), dtype=torch.int64, device=ht.device)
    value = torch.empty((nh,), dtype=torch.float32, device=ht.device)
    if nh == 0:
        return index.reshape(0, 3), value
    ws = L.workspace(L.lib().mednet_heatmap_peaks_ws_bytes(nh, vox), ht.device)
    L.check(L.lib().mednet_heatmap_peaks(ht.data_ptr(), nh, vox, index.data_ptr(), value.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()),
            "heatmap_peaks")
    zyx = torch.stack((torch.div(index, h * w, rounding_mode="floor"), torch.div(index, w, rounding_mode="floor") % h, index % w), dim=1)
    return zyx, value


class BlendedPrediction:
    """What GridPredictor.predict leaves on the device: the accumulators, the weight sum and how to read them."""

    def __init__(self, acc, wsum, num_heatmaps, blend_of):
        self.acc, self.wsum, self.num_heatmaps, self.blend_of = acc, wsum, num_heatmaps, blend_of

    def result(self, postprocess=None):
        """uint8 (H + 1) x D x H x W: the crop-stitch predictor's layout (heat maps clipped to 0..255, then the arg-max class).
        postprocess: a callable on the uint8 D x H x W class volume (mednet_hip.components.Postprocess) whose result replaces the
        class channel [-1]; None runs exactly the launches of a call without it."""
        res = finalize(self.acc, self.wsum, self.num_heatmaps, self.blend_of, result=True)[0]
        if postprocess is not None:
            res[-1].copy_(postprocess(res[-1]))
        return res

    def probabilities(self, dtype=torch.float32):
        return finalize(self.acc, self.wsum, self.num_heatmaps, self.blend_of, probabilities=dtype)[1]

    def heatmaps(self):
        return finalize(self.acc, self.wsum, self.num_heatmaps, self.blend_of, heatmaps=True)[2]

    def peaks(self):
        """(positions H x 3 int64 as (z, y, x), values H fp32) of the blended heat maps."""
        return heatmap_peaks(self.heatmaps())

    def evaluate(self, label, spacing=(1, 1, 1), **kw):
        """mednet_hip.metrics.evaluate_case on the class channel of result() against `label` (D x H x W on the device): overlap and
        surface distances per class as a CaseMetrics; num_classes defaults to the number of class channels."""
        from .metrics import evaluate_case
        num_classes = kw.pop("num_classes", self.acc.shape[0] - self.num_heatmaps)
        return evaluate_case(self.result()[-1], label, num_classes, spacing=spacing, **kw)


class ResampledPrediction(BlendedPrediction):
    """A BlendedPrediction whose network ran on a resampled grid (GridPredictor(target_spacing=...).predict(volume, spacing=...)):
    the accumulators lie at the network's grid, everything read from them is brought back to the native grid `native_shape`
    (mednet_hip.resample)."""

    def __init__(self, acc, wsum, num_heatmaps, blend_of, native_shape, kind="linear"):
        super().__init__(acc, wsum, num_heatmaps, blend_of)
        self.native_shape, self.kind = tuple(int(v) for v in native_shape), kind

    def result(self, postprocess=None):
        """uint8 (H + 1) x D x H x W at the native grid: the class channel is resample_argmax of the class probabilities (no class
        volume at the native size), the heat maps are resampled linearly, then clipped to 0..255 and truncated as at the network's
        grid; then `postprocess` on the class channel."""
        from .resample import resample_argmax
        res = torch.empty((self.num_heatmaps + 1,) + self.native_shape, dtype=torch.uint8, device=self.acc.device)
        res[-1].copy_(resample_argmax(super().probabilities(), size=self.native_shape, kind=self.kind, antialias=True))
        if self.num_heatmaps:
            res[:-1].copy_(self.heatmaps().clamp_(0, 255).to(torch.uint8))
        if postprocess is not None:
            res[-1].copy_(postprocess(res[-1]))
        return res

    def probabilities(self, dtype=torch.float32):
        from .resample import resample
        return resample(super().probabilities(), size=self.native_shape, kind=self.kind, antialias=True, dtype=dtype)

    def heatmaps(self):
        from .resample import resample
        heat = super().heatmaps()
        if not self.num_heatmaps:
            return torch.empty((0,) + self.native_shape, dtype=torch.float32, device=self.acc.device)
        return resample(heat, size=self.native_shape, kind="linear", antialias=True)

    def peaks(self):
        """(positions H x 3 float64 as (z, y, x) in native voxel coordinates, values H fp32): the peaks of the blended heat maps at
        the network's grid, mapped by p = (q + 0.5) * n_native / n_net - 0.5."""
        zyx, value = heatmap_peaks(super().heatmaps())
        net = torch.tensor(tuple(self.acc.shape[1:]), dtype=torch.float64, device=zyx.device)
        native = torch.tensor(self.native_shape, dtype=torch.float64, device=zyx.device)
        return (zyx.double() + 0.5) * native / net - 0.5, value


class GridPredictor:
    def __init__(self, model, patch_size, patch_overlap, num_heatmaps=0, pad_mode="constant", batch_size=4,
                 channel_selection=None, blend=None, sigma_scale=0.125, mirror_axes=(), blend_of="probabilities", postprocess=None,
                 target_spacing=None, resample_kind="linear", normalize=None):
        """normalize: an intensity scheme (mednet_hip.intensity.ZScore / CTWindow / Rescale) applied to the uploaded volume at its
        native grid, before any resampling (nnU-Net v2's order); int16 volumes are accepted then.  None (the default): exactly the
        calls of a predictor without the argument.  target_spacing: the voxel spacing the network was trained at; `predict(volume, spacing=...)` then resamples the volume to
        it (anti-aliased, resample_kind) and returns a ResampledPrediction at the native grid.  None (the default): no resampling,
        exactly the calls of a predictor without the argument.  postprocess: a callable on the uint8 D x H x W class volume (mednet_hip.components.Postprocess), applied to the class
        channel [-1] of what __call__ returns; `predict` is unchanged.  blend=None: the reference's crop-stitch (the default).  blend="gaussian" / "constant" / three per-axis weight vectors:
        overlapping windows are blended (`predict`); mirror_axes: patch axes averaged over their flips (2^k passes per patch);
        blend_of: what the class channels accumulate, "probabilities" (softmax per patch) or "logits" (softmax once, at the end)."""
        self.model, self.patch_size, self.patch_overlap = model, list(patch_size), list(patch_overlap)
        self.num_heatmaps, self.pad_mode, self.batch_size, self.channel_selection = num_heatmaps, pad_mode, batch_size, channel_selection
        self.blend, self.blend_of, self.postprocess = blend, blend_of, postprocess
        self.target_spacing, self.resample_kind, self.normalize = target_spacing, resample_kind, normalize
        self.mirror_bits = mirror_mask(mirror_axes)
        if blend is None:
            if self.mirror_bits:
                raise ValueError("mirror_axes needs blend: averaging over flips is an accumulate-style stitch")
            return
        if blend_of not in _BLEND_OF:
            raise ValueError(f"blend_of {blend_of!r} (supported: probabilities, logits)")
        if isinstance(blend, str):
            self.windows = blend_window(self.patch_size, blend, sigma_scale)
        else:
            self.windows = tuple(np.ascontiguousarray(np.asarray(v, dtype=np.float32)) for v in blend)
            if [v.shape for v in self.windows] != [(int(p),) for p in self.patch_size]:
                raise ValueError(f"blend: three weight vectors of {self.patch_size} entries expected")
        # the passes of a patch: every subset of the mirror axes, ascending mask
        self.mirror_passes = [m for m in range(8) if m & ~self.mirror_bits == 0]

    def _upload(self, volume):
        """-> (the selected channels of the volume as fp32 on the model's device (the reference's `.float()`), uploaded once; the
        grid of patch positions there)."""
        dev = next(self.model.parameters()).device
        vol = torch.as_tensor(np.asarray(volume) if not torch.is_tensor(volume) else volume)
        if self.channel_selection is not None:
            vol = vol[self.channel_selection]
        vol = vol.to(dev, non_blocking=True)
        if self.normalize is not None:
            vol = self.normalize(vol)
        vol = vol.float().contiguous()
        return vol, torch.from_numpy(grid_positions(vol.shape[1:], self.patch_size, self.patch_overlap)).to(dev)

    def _batches(self, vol: torch.Tensor, pos_all: torch.Tensor, mirror=0):
        """(pos, logits) of every batch of grid positions, in order, the model in eval mode until the generator is closed: callers
        iterate under contextlib.closing, so an exception in their loop restores the mode while it unwinds."""
        was_training = self.model.training
        self.model.eval()
        try:
            for b0 in range(0, pos_all.shape[0], self.batch_size):
                pos = pos_all[b0:b0 + self.batch_size].contiguous()
                yield pos, self.model(gather_patches(vol, pos, self.patch_size, self.patch_overlap, self.pad_mode, mirror=mirror))
        finally:
            self.model.train(was_training)

    @torch.no_grad()
    def predict(self, volume, spacing=None) -> BlendedPrediction:
        """spacing (with the predictor's target_spacing): the volume's voxel spacing; the network runs at target_spacing and the
        prediction is a ResampledPrediction at the volume's own grid.  Blended sliding-window inference.  For every mirror pass (ascending mask) and every batch of grid positions:
        gather(mirror) -> model -> accumulate(mirror).  A voxel's sums are taken pass by pass in patch order, so the result does not
        depend on batch_size.  An overlap of 0 is legal here (nothing is cropped)."""
        if self.blend is None:
            raise ValueError("predict() needs blend (the crop-stitch path is __call__)")
        vol, pos_all = self._upload(volume)
        native_shape = None
        if spacing is not None and self.target_spacing is not None:
            from .resample import resample
            native_shape = tuple(vol.shape[1:])
            vol = resample(vol, spacing=spacing, target_spacing=self.target_spacing, kind=self.resample_kind, antialias=True)
            pos_all = torch.from_numpy(grid_positions(vol.shape[1:], self.patch_size, self.patch_overlap)).to(vol.device)
        windows = tuple(torch.from_numpy(v).to(vol.device) for v in self.windows)
        acc = wsum = None
        for m in self.mirror_passes:
            with contextlib.closing(self._batches(vol, pos_all, m)) as batches:
                for pos, logits in batches:
                    if acc is None:
                        acc = torch.zeros((logits.shape[1],) + tuple(vol.shape[1:]), dtype=torch.float32, device=vol.device)
                        wsum = torch.zeros(tuple(vol.shape[1:]), dtype=torch.float32, device=vol.device)
                    accumulate(logits, pos, acc, wsum, windows, self.num_heatmaps, self.patch_overlap, m, self.blend_of)
        if native_shape is not None:
            return ResampledPrediction(acc, wsum, self.num_heatmaps, self.blend_of, native_shape, self.resample_kind)
        return BlendedPrediction(acc, wsum, self.num_heatmaps, self.blend_of)

    @torch.no_grad()
    def __call__(self, volume):
        if self.blend is not None:
            return self.predict(volume).result(self.postprocess)
        vol, pos_all = self._upload(volume)
        result = torch.zeros((self.num_heatmaps + 1,) + tuple(vol.shape[1:]), dtype=torch.uint8, device=vol.device)
        with contextlib.closing(self._batches(vol, pos_all)) as batches:
            for pos, logits in batches:
                assemble(logits, pos, result, self.num_heatmaps, self.patch_overlap)
        if self.postprocess is not None:
            result[-1].copy_(self.postprocess(result[-1]))
        return result
