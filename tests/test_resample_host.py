"""Host logic of mednet_hip.resample and of the predictor's optional resampling, without a GPU: output sizes, argument errors, and
a GridPredictor without target_spacing (or a predict() without spacing) makes exactly the calls it made before the module existed."""
import numpy as np
import pytest
import torch

from mednet_hip import predict as P
from mednet_hip import resample as M


def test_output_size():
    assert M.output_size((40, 36, 44), (2, 1, 1), (1, 1, 1)) == (80, 36, 44)
    assert M.output_size((400, 512, 512), (2.5, 0.8, 0.8), (1.0, 1.0, 1.0)) == (1000, 410, 410)
    assert M.output_size((3, 3, 3), (1, 1, 1), (2, 2, 2)) == (2, 2, 2)              # floor(1.5 + 0.5)
    assert M.output_size((5, 5, 5), (1, 1, 1), (4, 4, 4)) == (1, 1, 1)              # floor(1.25 + 0.5)
    assert M.output_size((1, 2, 3), (0.1, 0.1, 0.1), (100, 100, 100)) == (1, 1, 1)  # never below 1
    for n in range(1, 40):
        assert M.output_size((n, n, n), (1, 1, 1), (1, 1, 1)) == (n, n, n)
    for bad in ((0, 1, 1), (1, -1, 1), (1, 1, float("nan")), (float("inf"), 1, 1)):
        with pytest.raises(ValueError, match="spacing"):
            M.output_size((4, 4, 4), bad, (1, 1, 1))
        with pytest.raises(ValueError, match="spacing"):
            M.output_size((4, 4, 4), (1, 1, 1), bad)
    with pytest.raises(ValueError, match="three"):
        M.output_size((4, 4), (1, 1), (1, 1))


def test_size_arguments():
    with pytest.raises(ValueError, match="either size= or spacing="):
        M._size_of((4, 4, 4), None, None, None, "resample")
    with pytest.raises(ValueError, match="either size= or spacing="):
        M._size_of((4, 4, 4), (4, 4, 4), (1, 1, 1), (1, 1, 1), "resample")
    with pytest.raises(ValueError, match="go together"):
        M._size_of((4, 4, 4), None, (1, 1, 1), None, "resample")
    with pytest.raises(ValueError, match="three extents"):
        M._size_of((4, 4, 4), (4, 4), None, None, "resample")
    with pytest.raises(ValueError, match="three extents"):
        M._size_of((4, 4, 4), (4, 0, 4), None, None, "resample")
    assert M._size_of((4, 6, 8), None, (2, 1, 1), (1, 1, 1), "resample") == (8, 6, 8)


def test_operands_are_refused_before_any_kernel():
    """No CPU fallback: a host tensor is an error, and so are a wrong rank, dtype, kind or class count."""
    with pytest.raises(RuntimeError, match="HIP"):
        M.resample(torch.zeros(2, 4, 4, 4), size=(4, 4, 4))
    with pytest.raises(RuntimeError, match="HIP"):
        M.resample_argmax(torch.zeros(2, 4, 4, 4), size=(4, 4, 4))
    with pytest.raises(RuntimeError, match="HIP"):
        M.resample_labels(torch.zeros(4, 4, 4, dtype=torch.uint8), size=(4, 4, 4), num_classes=2)
    meta = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")
    orig = M.L.require_gpu
    M.L.require_gpu = lambda t, who: None
    try:
        with pytest.raises(ValueError, match="volume expected"):
            M.resample(meta(4, 4), size=(4, 4, 4))
        with pytest.raises(ValueError, match="float32, float16 or uint8"):
            M.resample(meta(4, 4, 4, dtype=torch.int64), size=(4, 4, 4))
        with pytest.raises(ValueError, match="scores classes"):
            M.resample_argmax(meta(4, 4, 4), size=(4, 4, 4))
        with pytest.raises(ValueError, match="scores classes"):
            M.resample_argmax(meta(2, 4, 4, 4, dtype=torch.uint8), size=(4, 4, 4))
        with pytest.raises(ValueError, match="classes"):
            M.resample_argmax(meta(257, 2, 2, 2), size=(4, 4, 4))
        with pytest.raises(ValueError, match="kind"):
            M.resample_argmax(meta(2, 4, 4, 4), size=(4, 4, 4), kind="nearest")
    finally:
        M.L.require_gpu = orig


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv3d(1, 3, 1)

    def forward(self, x):
        return self.conv(x)


def _predict_calls(monkeypatch, ctor_kw, predict_kw):
    """The calls a predict() makes into the predictor's kernels wrappers, with CPU stand-ins for them and every entry point of the
    resampling module patched to raise."""
    calls = []

    def gather(vol, pos, patch_size, patch_overlap, pad_mode="symmetric", mirror=0):
        calls.append(("gather", tuple(vol.shape), pos.tolist(), mirror))
        return torch.zeros((pos.shape[0], vol.shape[0]) + tuple(patch_size))

    def accumulate(logits, pos, acc, wsum, windows, num_heatmaps, patch_overlap, mirror=0, blend_of="probabilities"):
        calls.append(("accumulate", tuple(logits.shape), tuple(acc.shape), mirror, blend_of))

    def refuse(*a, **k):
        raise AssertionError("the resampling module was touched")

    monkeypatch.setattr(P, "gather_patches", gather)
    monkeypatch.setattr(P, "accumulate", accumulate)
    for name in ("resample", "resample_argmax", "resample_labels", "resample_axis", "device_table", "axis_table", "output_size"):
        monkeypatch.setattr(M, name, refuse)
    pred = P.GridPredictor(_Net(), (8, 8, 8), (2, 2, 2), blend="gaussian", batch_size=2, **ctor_kw)
    out = pred.predict(np.zeros((1, 8, 10, 12), dtype=np.float32), **predict_kw)
    return calls, out


def test_predictor_without_spacings_never_touches_the_module(monkeypatch):
    base, out = _predict_calls(monkeypatch, {}, {})
    assert type(out) is P.BlendedPrediction and base and tuple(out.acc.shape) == (3, 8, 10, 12)
    for ctor_kw, predict_kw in (({"target_spacing": None}, {"spacing": (2, 1, 1)}), ({"target_spacing": (1, 1, 1)}, {}),
                                ({"target_spacing": (1, 1, 1)}, {"spacing": None}), ({"resample_kind": "cubic"}, {})):
        calls, out = _predict_calls(monkeypatch, ctor_kw, predict_kw)
        assert calls == base and type(out) is P.BlendedPrediction, (ctor_kw, predict_kw)
    # with both given the volume goes through the module (here: the stand-in that raises)
    with pytest.raises(AssertionError, match="resampling module was touched"):
        _predict_calls(monkeypatch, {"target_spacing": (1, 1, 1)}, {"spacing": (2, 1, 1)})


def test_resampled_prediction_maps_peaks_to_native_coordinates(monkeypatch):
    """p = (q + 0.5) * n_native / n_net - 0.5 per axis, as floats."""
    acc, wsum = torch.zeros(3, 80, 36, 44), torch.ones(80, 36, 44)
    pred = P.ResampledPrediction(acc, wsum, 2, "probabilities", (40, 36, 44))
    monkeypatch.setattr(P.BlendedPrediction, "heatmaps", lambda self: "net-grid heat maps")
    monkeypatch.setattr(P, "heatmap_peaks", lambda heat: (torch.tensor([[0, 0, 0], [79, 35, 43], [10, 7, 3]]), torch.tensor([1.0, 2.0, 3.0])))
    pos, val = pred.peaks()
    assert pos.dtype == torch.float64 and val.tolist() == [1.0, 2.0, 3.0]
    assert pos.tolist() == [[-0.25, 0.0, 0.0], [39.25, 35.0, 43.0], [4.75, 7.0, 3.0]]
    assert pred.native_shape == (40, 36, 44) and isinstance(pred, P.BlendedPrediction)
