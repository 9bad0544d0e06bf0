"""Validation sample logging on the device: the arrays `log_samples` (segmentation.py:67-92,
landmarks.py:85-123) feeds to imshow through vis_logimages / vis_loglabels / vis_logheatmaps (utils/plots.py:21-127), computed
from ONE sample of the batch where its tensors lie.

    panels = sample_panels(outputs, batch["label"], inputs, num_heatmaps=nh, projection_type="mean")
    host = panels.to_host()                       # the feature's only host transfer: one copy, one event wait
    ax.imshow(host["label_grid"], ...)            # drawing (matplotlib, PNG files, the logger) stays with the caller

The reference moves the whole batch to the host (data, int64 labels, the int64 arg-max of the soft-maxed logits and, for
landmarks, the float heat maps and raw outputs) and reduces 3-D numpy arrays there although it draws sample 0 only.  Here one
fused HIP pass per source tensor (csrc/vis.hip, mednet_sample_panels) produces the projected panels: the class planes are read
once for arg-max and projection together (the soft-max is dropped: it does not change the arg-max), and no arg-max volume or
slice copy is stored.  The reference's int64 panels (`pred_class`, `labels`) are uint8 here, with the same values."""
from __future__ import annotations

import math

import torch

from . import _lib as L

_MODES = {"mean": L.MIP_MEAN, "max": L.MIP_MAX}
_ALIGN = 16  # bytes between the panels inside the one buffer they share


def slice_indices(num_slices: int, steps: int = 5):
    """vis_logimages' slice rule (plots.py:33-35), literally: range(0, num_slices, num_slices // steps) -- 6 slices for 128 and
    steps=5, not 5.  num_slices < steps raises ValueError, as the range with a zero step does."""
    return list(range(0, num_slices, num_slices // steps))


def grid_shape(n: int, cell_h: int, cell_w: int, nrow: int = 8, padding: int = 2):
    """(rows, columns, xmaps, ymaps) of torchvision.utils.make_grid's canvas for n cells."""
    xmaps = min(nrow, n)
    ymaps = int(math.ceil(n / xmaps))
    return ymaps * (cell_h + padding) + padding, xmaps * (cell_w + padding) + padding, xmaps, ymaps


def make_grid2d(cells: torch.Tensor, nrow: int = 8, padding: int = 2, pad_value=0) -> torch.Tensor:
    """Channel 0 of torchvision.utils.make_grid(cells[:, None], nrow, padding, pad_value=pad_value) for n single-channel cells
    [n, A, B] (the reference draws `grid[0, ...]` only; make_grid repeats a single channel three times).  Cell k starts at row
    (k // xmaps) * (A + padding) + padding and column (k % xmaps) * (B + padding) + padding of a canvas of
    (ymaps * (A + padding) + padding) x (xmaps * (B + padding) + padding) filled with pad_value, xmaps = min(nrow, n),
    ymaps = ceil(n / xmaps).  torchvision is not a dependency of this package: the rule is restated from its source and has NOT
    been run against it.  (torchvision returns a lone image, n == 1, unpadded; no caller of the reference builds such a grid and
    the rule above is applied to it too.)  Works on any device; a few small copies."""
    n, a, b = cells.shape
    if n == 0:
        raise ValueError("make_grid2d: no cells")
    rows, cols, xmaps, _ = grid_shape(n, a, b, nrow, padding)
    grid = cells.new_full((rows, cols), pad_value)
    for k in range(n):
        r0, c0 = (k // xmaps) * (a + padding) + padding, (k % xmaps) * (b + padding) + padding
        grid[r0:r0 + a, c0:c0 + b] = cells[k]
    return grid


class SamplePanels:
    """The panels of one sample, as views of ONE device buffer (`buffer`, uint8):
        pred_mip            uint8 [P0, P1]      max over mip_axis of the arg-max class
        label_mip           uint8 [P0, P1]      max over mip_axis of the class map
        input_mip           fp32  [P0, P1]      mean | max over mip_axis of inputs[sample, 0]
        heatmap_mip         fp32  [nh, P0, P1]  max over mip_axis of the target heat maps      (None without heat maps)
        output_heatmap_mip  fp32  [nh, P0, P1]  max over mip_axis of the raw heat-map outputs  (None without heat maps)
        images              fp32  [C * k, D, W] vis_logimages' slices inputs[sample][c, :, idx, :], channel-major
    (P0, P1) = D x H x W without mip_axis."""

    _FIELDS = ("pred_mip", "label_mip", "input_mip", "heatmap_mip", "output_heatmap_mip", "images")

    def __init__(self, buffer, views, num_heatmaps, steps):
        self.buffer, self._views, self.num_heatmaps, self.steps = buffer, views, num_heatmaps, steps
        for name in self._FIELDS:
            v = views.get(name)
            setattr(self, name, None if v is None else self._view(buffer, v))

    @staticmethod
    def _view(buf, spec):
        off, dtype, shape = spec
        nbytes = int(math.prod(shape)) * (1 if dtype == torch.uint8 else 4)
        return buf[off:off + nbytes].view(dtype).view(shape)

    # ---- the 2-D arrays the reference hands to imshow (grid[0, ...] of make_grid) ----------------------------------------
    def label_grid(self) -> torch.Tensor:
        """grid_mask[0] of vis_loglabels (plots.py:65-68): [pred_mip, label_mip] side by side (make_grid's default nrow=8)."""
        return make_grid2d(torch.stack([self.pred_mip, self.label_mip]))

    def background_grid(self, n: int = 2, nrow: int = 8) -> torch.Tensor:
        """grid_bg[0]: n copies of input_mip.  vis_loglabels (plots.py:76-78) takes n=2 and the default nrow;
        vis_logheatmaps (plots.py:114-116) n = 2 * num_heatmaps, nrow = num_heatmaps."""
        return make_grid2d(self.input_mip.unsqueeze(0).expand(n, -1, -1), nrow=nrow)

    def heatmap_grid(self) -> torch.Tensor:
        """grid_fg[0] of vis_logheatmaps (plots.py:117-121): the target heat-map projections in the first row, the raw output
        projections in the second (nrow = num_heatmaps)."""
        if self.heatmap_mip is None:
            raise ValueError("heatmap_grid: the panels were computed without heat maps (num_heatmaps=0)")
        return make_grid2d(torch.cat([self.heatmap_mip, self.output_heatmap_mip]), nrow=self.num_heatmaps)

    def to_host(self):
        """{name: numpy array} of every panel: ONE non-blocking copy of the shared buffer into pinned memory, one event wait.
        The arrays are views of that pinned buffer."""
        host = torch.empty(self.buffer.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(self.buffer, non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self.buffer.device))
        done.synchronize()
        return {name: self._view(host, self._views[name]).numpy() for name in self._FIELDS if self._views.get(name) is not None}


def _dense_volume(t: torch.Tensor, what: str):
    """The trailing D x H x W of `t` must be dense: the kernels read the tensor where it lies."""
    d, h, w = t.shape[-3:]
    if tuple(t.stride()[-3:]) != (h * w, w, 1):
        raise ValueError(f"sample_panels: {what} must be dense in its last three dimensions (strides {tuple(t.stride())})")


def sample_panels(outputs, label, inputs, num_heatmaps=0, mip_axis=1, projection_type="mean", steps=5, sample=0, heatmaps=None):
    """Everything `log_samples` draws, for sample `sample` of the batch (the reference draws sample 0).

    outputs   N x (num_heatmaps + classes) x D x H x W fp32 planar network output (raw heat-map outputs, then class logits)
    label     `batch['label']`, N x (num_heatmaps + 1) x D x H x W: channels [:num_heatmaps] are the target heat maps, channel -1
              is the class map -- both read in place -- or the class map alone, N x D x H x W.  Class map: uint8 or int64 (values
              above 255 are a caller error: the uint8 panel wraps them).
    heatmaps  optional N x num_heatmaps x D x H x W targets (uint8 or fp32) when `label` is the class map alone or holds them in
              another type
    inputs    N x C x D x H x W fp32
    mip_axis  0, 1 or 2, counted within D x H x W (the reference's default 1 projects over H and gives D x W panels)
    projection_type  "mean" | "max" for the input panel;  steps: vis_logimages' slice count (slice_indices)

    Returns SamplePanels (device tensors).  Launches on the current stream and does not synchronise; raises on CPU tensors (no
    CPU fallback)."""
    for t, what in ((outputs, "outputs"), (label, "label"), (inputs, "inputs")) + (((heatmaps, "heatmaps"),) if heatmaps is not None else ()):
        L.require_gpu(t, f"vis.sample_panels({what})")
    if mip_axis not in (0, 1, 2):
        raise ValueError(f"sample_panels: mip_axis {mip_axis!r} (0, 1 or 2, counted within D x H x W)")
    if projection_type not in _MODES:
        raise ValueError(f"sample_panels: projection_type {projection_type!r} ('mean' or 'max')")
    nh = int(num_heatmaps)
    if outputs.dim() != 5 or inputs.dim() != 5 or outputs.dtype != torch.float32 or inputs.dtype != torch.float32:
        raise ValueError("sample_panels: outputs and inputs must be 5-D float32 tensors (N x C x D x H x W)")
    n, ch, d, h, w = outputs.shape
    ncls = ch - nh
    if nh < 0 or not 1 <= ncls <= 256:
        raise ValueError(f"sample_panels: {ch} output channels with num_heatmaps={nh} (1 to 256 class channels needed)")
    if tuple(inputs.shape[-3:]) != (d, h, w) or tuple(label.shape[-3:]) != (d, h, w):
        raise ValueError(f"sample_panels: volumes differ: outputs {tuple(outputs.shape)}, inputs {tuple(inputs.shape)}, label {tuple(label.shape)}")
    if not 0 <= sample < n:
        raise IndexError(f"sample_panels: sample {sample} of a batch of {n}")
    index = slice_indices(h, steps)  # (ValueError when H < steps, before anything is launched)

    cls_map = label[:, -1] if label.dim() == 5 else label
    if heatmaps is None and nh:
        if label.dim() != 5 or label.shape[1] < nh + 1:
            raise ValueError(f"sample_panels: num_heatmaps={nh} needs label N x {nh + 1} x D x H x W or heatmaps=")
        heatmaps = label[:, :nh]
    if cls_map.dtype not in (torch.uint8, torch.int64):
        raise ValueError(f"sample_panels: class map of type {cls_map.dtype} (uint8 or int64)")
    for t, what in ((outputs, "outputs"), (inputs, "inputs"), (cls_map, "the class map")):
        _dense_volume(t, what)
    hm = None
    if nh:
        if heatmaps.dtype not in (torch.uint8, torch.float32) or tuple(heatmaps.shape[1:]) != (nh, d, h, w):
            raise ValueError(f"sample_panels: heat maps {tuple(heatmaps.shape)} of type {heatmaps.dtype} (N x {nh} x D x H x W, uint8 or float32)")
        _dense_volume(heatmaps, "the heat maps")
        if nh > 1 and heatmaps.stride(1) != d * h * w:
            raise ValueError("sample_panels: the heat-map channels of one sample must be adjacent")
        hm = heatmaps[sample]

    panel = tuple(v for k, v in enumerate((d, h, w)) if k != mip_axis)
    c_in = inputs.shape[1]
    specs, off = {}, 0
    for name, dtype, shape in (("pred_mip", torch.uint8, panel), ("label_mip", torch.uint8, panel), ("input_mip", torch.float32, panel),
                               ("heatmap_mip", torch.float32, (nh,) + panel), ("output_heatmap_mip", torch.float32, (nh,) + panel),
                               ("images", torch.float32, (c_in * len(index), d, w))):
        if nh == 0 and name.endswith("heatmap_mip"):
            continue
        specs[name] = (off, dtype, shape)
        off += -(-int(math.prod(shape)) * (1 if dtype == torch.uint8 else 4) // _ALIGN) * _ALIGN
    dev = outputs.device
    out = SamplePanels(torch.empty(off, dtype=torch.uint8, device=dev), specs, nh, steps)

    lib = L.lib()
    ws_bytes = lib.mednet_sample_panels_ws_bytes(d, h, w, nh, mip_axis)
    ws = L.workspace(ws_bytes, dev) if ws_bytes else None
    lg, lab, x0 = outputs[sample], cls_map[sample], inputs[sample, 0]
    L.check(lib.mednet_sample_panels(lg.data_ptr(), outputs.stride(1), nh, ncls, lab.data_ptr(),
                                     L.U8 if lab.dtype == torch.uint8 else L.I64, L.ptr(hm),
                                     L.U8 if hm is not None and hm.dtype == torch.uint8 else L.F32, x0.data_ptr(),
                                     out.pred_mip.data_ptr(), out.label_mip.data_ptr(), out.input_mip.data_ptr(),
                                     L.ptr(out.heatmap_mip), L.ptr(out.output_heatmap_mip), d, h, w, mip_axis,
                                     _MODES[projection_type], L.ptr(ws), ws_bytes, L.stream()), "sample_panels")
    # vis_logimages (plots.py:32-36): a strided gather of a few slices -- plain indexing, channel-major
    step = h // steps
    out.images.view(c_in, len(index), d, w).copy_(inputs[sample][:, :, ::step, :].permute(0, 2, 1, 3))
    return out
