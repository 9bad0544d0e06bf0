"""Validation sample logging on the MI355X (-m gpu): the fused class / MIP panels of mednet_hip.vis (csrc/vis.hip) against torch on
the CPU over the same tensors, and the log_interval / on_samples arguments of the two validation steps.

Max and arg-max involve no rounding, so every panel except the mean projection is compared for equality.  The batch has two
samples and the one that is NOT drawn is poisoned (logits + 1000 on another class, labels and heat maps 255, inputs 1e6): a read
of the wrong sample shows in every panel."""
import numpy as np
import pytest
import torch

import mednet_hip
from mednet_hip import ops, vis
from mednet_hip.unet import model as HM
from oracle import ref_cpu as O

from gpu_util import DEV, assert_exact, lattice, rnd

pytestmark = pytest.mark.gpu

# odd extents (5, 7, 9); a reduced axis longer than a wave (W = 130 for axis 2) and longer than the segment count (70 > 64, so a
# segment holds more than one element; 16 / 8 / 6 take one element per segment); the contiguous axis longer than 128 (130) and very
# short (9); extents that are and are not multiples of 4 (the 16-byte and the scalar loads)
SHAPES = [(5, 7, 9), (16, 8, 64), (70, 6, 40), (6, 70, 40), (8, 6, 130)]
CHANNELS = [(2, 0), (4, 0), (5, 2)]  # (classes, heat maps)


def make_case(shape, ncls, nh, c_in, drawn=0, logits="lattice"):
    """CPU tensors of a two-sample batch whose sample `drawn` is clean and whose other sample is poisoned."""
    d, h, w = shape
    tag = f"vis{d}x{h}x{w}c{ncls}h{nh}i{c_in}"
    if logits == "lattice":  # many exact ties between the class planes
        out = lattice(tag + "lg", 2, nh + ncls, d, h, w, values=(-2, -1, 1, 2), density=0.5)
    else:
        out = rnd(tag + "lg", 2, nh + ncls, d, h, w)
    g = O._rng("in:" + tag + "lab")
    label = torch.from_numpy(np.concatenate([g.integers(0, 256, size=(2, nh, d, h, w), dtype=np.uint8),
                                             g.integers(0, ncls, size=(2, 1, d, h, w), dtype=np.uint8)], axis=1))
    inputs = rnd(tag + "in", 2, c_in, d, h, w)
    other = 1 - drawn
    out[other] += 1000.0 * (torch.arange(nh + ncls).view(-1, 1, 1, 1) == nh + ncls - 1)  # another class wins everywhere
    out[other, :nh] += 1000.0
    label[other] = 255
    inputs[other] = 1e6
    return out, label, inputs


def reference(out, label, inputs, nh, axis, projection, s=0, steps=5):
    """What log_samples computes on the host for sample s (torch on the CPU), uint8 where the reference has int64."""
    cls = label[s, -1].long()
    ref = {"pred_mip": out[s, nh:].argmax(dim=0).amax(dim=axis).to(torch.uint8),
           "label_mip": cls.amax(dim=axis).to(torch.uint8),
           "input_mip": inputs[s, 0].amax(dim=axis) if projection == "max" else inputs[s, 0].double().mean(dim=axis)}
    if nh:
        ref["heatmap_mip"] = label[s, :nh].float().amax(dim=axis + 1)
        ref["output_heatmap_mip"] = out[s, :nh].amax(dim=axis + 1)
    h = inputs.shape[3]
    ref["images"] = torch.cat([torch.stack([inputs[s, c, :, i, :] for i in range(0, h, h // steps)]) for c in range(inputs.shape[1])])
    return ref


def check_exact(panels, ref, what):
    for name, want in ref.items():
        got = getattr(panels, name)
        assert got.dtype == want.dtype or name == "input_mip", (what, name, got.dtype, want.dtype)
        assert_exact(got, want, f"{what} {name}")
    if "heatmap_mip" not in ref:
        assert panels.heatmap_mip is None and panels.output_heatmap_mip is None


def both_label_forms(out, label, inputs, nh, **kw):
    """(a) batch['label'] as it lies: uint8, the class map a strided view of the N x (nh + 1) x ... volume, uint8 heat maps;
    (b) a contiguous int64 class map with fp32 heat maps."""
    o, l, x = out.to(DEV), label.to(DEV), inputs.to(DEV)
    yield "u8 in place", vis.sample_panels(o, l, x, nh, **kw)
    yield "i64 + fp32", vis.sample_panels(o, l[:, -1].long().contiguous(), x, nh, heatmaps=l[:, :nh].float() if nh else None, **kw)


@pytest.mark.parametrize("ncls,nh", CHANNELS)
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_panels_equal_torch_on_the_cpu(shape, axis, ncls, nh):
    """pred_mip (logits with many exact ties: the first maximum must win, as torch.argmax on the CPU), label_mip, both heat-map
    panels, the max projection of the input and the image slices, element for element."""
    c_in = 1 + (axis + ncls) % 2
    out, label, inputs = make_case(shape, ncls, nh, c_in)
    planes = out[0, nh:]
    assert int((planes == planes.amax(dim=0, keepdim=True)).sum(dim=0).gt(1).sum()) > 0, "the lattice logits hold no tie"
    ref = reference(out, label, inputs, nh, axis, "max")
    for form, panels in both_label_forms(out, label, inputs, nh, mip_axis=axis, projection_type="max"):
        check_exact(panels, ref, f"{shape} axis {axis} {form}")


@pytest.mark.parametrize("shape,axis", [((4, 5, 258), 2), ((2, 5, 1040), 2), ((16, 128, 512), 0), ((16, 127, 515), 0)])
def test_reductions_of_four_and_more_elements_per_lane(shape, axis):
    """The arg-max loop takes four positions per trip and a one-position tail: a lane meets four or more positions only in lines
    longer than 256 (axis 2; 1040 for the 16-byte loads) or where the panel alone fills the chip and the segments grow
    (axes 0 and 1: a 65536-pixel panel, with 16-byte and with scalar loads)."""
    out, label, inputs = make_case(shape, 3, 1, 1)
    ref = reference(out, label, inputs, 1, axis, "max")
    check_exact(vis.sample_panels(out.to(DEV), label.to(DEV), inputs.to(DEV), 1, mip_axis=axis, projection_type="max"), ref,
                f"{shape} axis {axis}")


def test_sample_one_is_drawn_when_asked():
    out, label, inputs = make_case((16, 8, 64), 5, 2, 2, drawn=1)
    ref = reference(out, label, inputs, 2, 1, "max", s=1)
    for form, panels in both_label_forms(out, label, inputs, 2, mip_axis=1, projection_type="max", sample=1):
        check_exact(panels, ref, f"sample 1 {form}")


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_tie_free_logits(axis):
    """4 * integer + class index: two class planes never agree, and every class wins somewhere."""
    ncls, shape = 4, (8, 16, 24)
    g = O._rng("in:vis-tiefree")
    out = torch.from_numpy((4 * g.integers(-3, 4, size=(2, ncls) + shape) + np.arange(ncls).reshape(1, ncls, 1, 1, 1)).astype(np.float32))
    top2 = out[0].topk(2, dim=0).values
    assert bool((top2[0] > top2[1]).all()), "tie between the two largest class logits"
    assert sorted(out[0].argmax(dim=0).unique().tolist()) == list(range(ncls))
    _, label, inputs = make_case(shape, ncls, 0, 1)
    out[1, 0] += 1000.0
    ref = reference(out, label, inputs, 0, axis, "max")
    panels = vis.sample_panels(out.to(DEV), label.to(DEV), inputs.to(DEV), 0, mip_axis=axis, projection_type="max")
    assert_exact(panels.pred_mip, ref["pred_mip"], f"tie-free axis {axis}")


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_mean_projection_exact_for_small_integers(axis):
    """Small integers and reduced lengths that are powers of two (16, 8, 64): every fp32 partial sum and the division are exact in
    any order, so the panel equals the fp64 mean."""
    shape = (16, 8, 64)
    out, label, inputs = make_case(shape, 2, 0, 1)
    inputs[0] = lattice("vis-mean-int", 1, *shape, values=(-3, -2, -1, 1, 2, 3), density=0.9)
    want = inputs[0, 0].double().mean(dim=axis)
    assert bool((want.float().double() == want).all())
    panels = vis.sample_panels(out.to(DEV), label.to(DEV), inputs.to(DEV), 0, mip_axis=axis, projection_type="mean")
    assert_exact(panels.input_mip, want, f"exact mean axis {axis}")


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_mean_projection_within_the_fp32_summation_bound(shape, axis):
    """|got - fp64 mean| <= (L + 1) * 2^-24 * mean|x| along the reduced line of length L: the bound of an fp32 sum of L terms in any
    order, plus the division."""
    out, label, inputs = make_case(shape, 2, 0, 1)
    x = inputs[0, 0].double()
    length = shape[axis]
    bound = (length + 1) * 2.0 ** -24 * x.abs().mean(dim=axis)
    panels = vis.sample_panels(out.to(DEV), label.to(DEV), inputs.to(DEV), 0, mip_axis=axis, projection_type="mean")
    err = (panels.input_mip.double().cpu() - x.mean(dim=axis)).abs()
    worst = float((err / bound).max())
    print(f"[vis mean {shape} axis {axis}] worst error / bound = {worst:.3f}")
    assert bool((err <= bound).all()), (shape, axis, worst)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_two_calls_give_the_same_bits(axis):
    out, label, inputs = make_case((70, 6, 40), 5, 2, 2, logits="rnd")
    o, l, x = out.to(DEV), label.to(DEV), inputs.to(DEV)
    a = vis.sample_panels(o, l, x, 2, mip_axis=axis)
    b = vis.sample_panels(o, l, x, 2, mip_axis=axis)
    for name in vis.SamplePanels._FIELDS:
        ta, tb = getattr(a, name), getattr(b, name)
        assert torch.equal(ta.reshape(-1).view(torch.uint8), tb.reshape(-1).view(torch.uint8)), name


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_misaligned_views_take_the_scalar_form(axis):
    """Extents that are multiples of 4 but tensors that start one element off a 16-byte boundary."""
    shape = (16, 8, 64)
    out, label, inputs = make_case(shape, 4, 0, 1)
    ref = reference(out, label, inputs, 0, axis, "max")

    def shifted(t):
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        flat[1:] = t.to(DEV).flatten()
        return flat[1:].view(t.shape)
    o, l, x = shifted(out), shifted(label), shifted(inputs)
    assert o.data_ptr() % 16 and x.data_ptr() % 16 and l.data_ptr() % 4
    check_exact(vis.sample_panels(o, l, x, 0, mip_axis=axis, projection_type="max"), ref, f"misaligned axis {axis}")


def test_to_host_returns_the_device_panels():
    out, label, inputs = make_case((5, 7, 9), 5, 2, 2)
    panels = vis.sample_panels(out.to(DEV), label.to(DEV), inputs.to(DEV), 2)
    host = panels.to_host()
    assert sorted(host) == sorted(vis.SamplePanels._FIELDS)
    for name, arr in host.items():
        assert isinstance(arr, np.ndarray)
        np.testing.assert_array_equal(arr, getattr(panels, name).cpu().numpy())
    # the grids the reference hands to imshow, from the device panels
    lg = panels.label_grid()
    assert lg.dtype == torch.uint8 and tuple(lg.shape) == (5 + 4, 2 * (9 + 2) + 2)
    assert torch.equal(lg[2:7, 2:11], panels.pred_mip) and torch.equal(lg[2:7, 13:22], panels.label_mip)
    hg = panels.heatmap_grid()
    assert tuple(hg.shape) == (2 * 7 + 2, 2 * 11 + 2) and torch.equal(hg[9:14, 13:22], panels.output_heatmap_mip[1])
    bg = panels.background_grid(4, nrow=2)
    assert tuple(bg.shape) == tuple(hg.shape) and torch.equal(bg[9:14, 2:11], panels.input_mip)


def test_bad_arguments_raise():
    out, label, inputs = make_case((5, 7, 9), 2, 0, 1)
    o, l, x = out.to(DEV), label.to(DEV), inputs.to(DEV)
    with pytest.raises(ValueError):
        vis.sample_panels(o, l, x, mip_axis=3)
    with pytest.raises(ValueError):
        vis.sample_panels(o, l, x, projection_type="median")
    with pytest.raises(ValueError, match="must not be zero"):
        vis.sample_panels(*(t.to(DEV) for t in make_case((5, 4, 9), 2, 0, 1)))  # H = 4 < steps = 5
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vis.sample_panels(out, label, inputs)


# ---- the validation steps ---------------------------------------------------------------------------------------------------
def _panels_equal(a, b, what):
    for name in vis.SamplePanels._FIELDS:
        ta, tb = getattr(a, name), getattr(b, name)
        assert (ta is None) == (tb is None), (what, name)
        if ta is not None:
            assert_exact(ta, tb, f"{what} {name}")


def _host_equals_device(panels):
    for name, arr in panels.to_host().items():
        np.testing.assert_array_equal(arr, getattr(panels, name).cpu().numpy())


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_segmentation_validation_logs_samples(mode):
    from mednet_hip.train import SegmentationValidation
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(2, 1, (16, 16, 16), 3, 0, seed=810).items()}
    seen = []
    with mednet_hip.precision(mode):
        net = O.keyed_init_(HM.ResidualUNet3D(1, 3, False, f_maps=[32, 64])).to(DEV)
        net.train()
        plain = SegmentationValidation(net, loss_weight=[0.05, 1.0, 1.0])
        logged = SegmentationValidation(net, loss_weight=[0.05, 1.0, 1.0], log_interval=2, log_vis_mip="max",
                                        on_samples=lambda panels, nb: seen.append((nb, panels)))
        for nb in range(3):
            got, want = logged.validation_step(batch, nb), plain.validation_step(batch, nb)
            assert list(got) == list(want)
            for k in want:
                assert torch.equal(got[k], want[k]), (nb, k)
            assert net.training
        assert [nb for nb, _ in seen] == [0, 2]
        net.eval()
        with torch.no_grad():
            mine = vis.sample_panels(net(batch["data"].float()), batch["label"], batch["data"].float(), 0, projection_type="max")
    for nb, panels in seen:
        _panels_equal(panels, mine, f"segmentation {mode} batch {nb}")
    _host_equals_device(seen[0][1])


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_landmark_validation_logs_samples(mode):
    from mednet_hip.train import LandmarkValidation
    nh = 2
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(2, 1, (16, 16, 16), 3, nh, seed=811).items()}
    assert batch["label"].dtype == torch.uint8
    seen, fused_calls = [], []
    real = ops.head_landmark_eval

    def counted(*a, **k):
        fused_calls.append(1)
        return real(*a, **k)
    ops.head_landmark_eval = counted
    try:
        with mednet_hip.precision(mode):
            net = O.keyed_init_(HM.ResidualUNet3D(1, nh + 3, False, f_maps=[32, 64])).to(DEV)
            net.train()
            kw = dict(class_weight=[0.05, 1.0, 1.0], regression_weight=[0.015, 0.02])
            plain = LandmarkValidation(net, **kw)
            logged = LandmarkValidation(net, log_interval=2, on_samples=lambda panels, nb: seen.append((nb, panels)), **kw)
            for nb in range(3):
                got, want = logged.validation_step(batch, nb), plain.validation_step(batch, nb)
                assert list(got) == list(want)
                for k in want:
                    assert torch.equal(got[k], want[k]), (nb, k)
                assert net.training
            assert [nb for nb, _ in seen] == [0, 2]
            fused = bool(fused_calls)
            assert fused == (mode != "fp32")  # the single-pass head serves the 16-bit modes: no logit tensor there
            inputs = batch["data"].float()
            net.eval()
            with torch.no_grad():
                logits = net.final_conv(net.forward_features(inputs)[0:1]) if fused else net(inputs)
                mine = vis.sample_panels(logits, batch["label"][0:1] if fused else batch["label"], inputs[0:1] if fused else inputs, nh)
    finally:
        ops.head_landmark_eval = real
    assert mine.heatmap_mip is not None and tuple(mine.output_heatmap_mip.shape) == (nh, 16, 16)
    for nb, panels in seen:
        _panels_equal(panels, mine, f"landmark {mode} batch {nb}")
    _host_equals_device(seen[1][1])
