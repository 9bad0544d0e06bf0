"""Multi-channel network input (2-4 fp32 channels: PET/CT, multi-sequence MRI) in the 16-bit storage modes, from the first layer's
kernels up to the trainer, the patch sampler and the grid predictor.  The exact-arithmetic side is in
tests/test_gpu_multichannel_exact.py; here: the GroupNorm form of the weight gradient against the two-kernel form (bit for bit),
random-input parity against ATen fp64, whole networks against the CPU oracle, and the callers on in_channels = 2."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import block, config, ops
from mednet_hip import nn as hnn
from mednet_hip import predict as HP
from mednet_hip.unet import components as HC
from mednet_hip.unet import loss as HL
from mednet_hip.unet import model as HM
from oracle import ref_cpu as O
from oracle import ref_predict as P

from gpu_util import DEV, DT, TOL, rel, rnd
from test_gpu_network import NET_TOL

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- GroupNorm form
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("cin,n,c,shape", [(2, 2, 32, (9, 11, 21)), (4, 2, 32, (9, 11, 21)), (4, 1, 64, (8, 8, 16)), (3, 1, 32, (16, 16, 16))])
def test_first_layer_groupnorm_backward_inside_the_multichannel_weight_gradient(mode, cin, n, c, shape):
    """mednet_gn_bwd_coefficients + mednet_conv3d_wgrad_cm_gn (the apply pass inside the weight-gradient kernel's staging) against
    mednet_gn_act_bwd_fused + mednet_conv3d_wgrad on the same tensors: every parameter gradient bit-identical -- the kernel restates
    the apply pass expression for expression."""
    x = torch.from_numpy(O._rng(f"cmgn{cin}{n}{c}{shape}").standard_normal((n, cin) + shape).astype(np.float32))
    g = torch.from_numpy(O._rng("cmgncot").standard_normal((n, c) + shape).astype(np.float32))
    res = {}
    for fused in (True, False):
        old = block.FUSE_C1GN
        block.FUSE_C1GN = fused
        before = block.C1GN_COUNT["fused"]
        try:
            with mednet_hip.precision(mode):
                net = O.keyed_init_(HC.ExtResNetBlock(cin, c, order="cge", num_groups=8)).to(DEV)
                yg = net(x.to(DEV))
                (yg.float() * g.to(DEV)).sum().backward()
                torch.cuda.synchronize()
                res[fused] = [p.grad.clone() for p in net.parameters()]
                assert L.lib().mednet_conv3d_dgrad_gn_rows_dt(n, *shape, c, c, config.conv_algo(), L.dt(yg)) > 0
        finally:
            block.FUSE_C1GN = old
        assert block.C1GN_COUNT["fused"] - before == (1 if fused else 0)
    for (k, _), a, b in zip(net.named_parameters(), res[True], res[False]):
        assert torch.isfinite(a).all(), k
        assert torch.equal(a, b), f"{k}: fused differs from the two-kernel form by {(a - b).abs().max().item():.3e}"


# ---------------------------------------------------------------------------------------------- random inputs
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("cin", [2, 3, 4])
def test_multichannel_first_layer_parity_on_random_inputs(mode, cin):
    """y, dw and the fused partial sums for fp32 inputs that are NOT numbers of the storage type, against F.conv3d in fp64 within
    the bounds the project holds its kernels of this kind to (gpu_util.TOL)."""
    n, cout, shape = 2, 32, (9, 11, 21)
    x = rnd(f"mcx{cin}", n, cin, *shape)
    w = rnd(f"mcw{cin}", cout, cin, 3, 3, 3, scale=1.0 / (27 * cin) ** 0.5)
    g = rnd(f"mcg{cin}", n, cout, *shape)
    dt = DT[mode]
    g = g.to(dt).float()
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = F.conv3d(x64, w64, padding=1)
    y64.backward(g.double())
    with mednet_hip.precision(mode):
        conv = hnn.Conv3d(cin, cout, 3, bias=False).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(w)
        y, partial = conv.forward_with_stats(x.to(DEV))
        assert partial is not None, "no fused statistics"
        y.backward(g.to(DEV).to(dt))
        torch.cuda.synchronize()
    ry, rw = rel(y, y64.detach()), rel(conv.weight.grad, w64.grad)
    print(f"[multichannel] cin={cin} {mode}: y rel-L2 {ry:.2e} dw rel-L2 {rw:.2e} (bound {TOL[mode]:.1e})")
    assert ry <= TOL[mode] and rw <= TOL[mode]
    # the sums are those of the STORED y: fp32 accumulation of K terms is off by at most K * 2^-24 of the sum of the terms' magnitudes
    ys = y.detach().double().cpu()
    tot = partial.double().cpu().sum(1)                      # [n][cout][2], entry 2j = the channel pair 2j, 2j + 1
    assert float(tot[:, 1::2].abs().max()) == 0.0
    pair = lambda t: t.sum((2, 3, 4)).reshape(n, cout // 2, 2).sum(2)
    k = 2 * ys[0, 0].numel()
    assert bool(((tot[:, 0::2, 0] - pair(ys)).abs() <= k * 2.0 ** -24 * pair(ys.abs())).all())
    assert bool(((tot[:, 0::2, 1] - pair(ys * ys)).abs() <= k * 2.0 ** -24 * pair(ys * ys)).all())


# ---------------------------------------------------------------------------------------------- networks
def _oracle_run(ctor, batch, dtype):
    ora = O.keyed_init_(O.ResidualUNet3D(**ctor)).to(dtype)
    lo = ora(batch["data"].to(dtype))
    O.DiceLoss()(lo, batch["label"][:, -1].long()).backward()
    return ora, lo


def _hip_run(ctor, batch, mode):
    with mednet_hip.precision(mode):
        net = O.keyed_init_(HM.ResidualUNet3D(**ctor)).to(DEV)
        lg = net(batch["data"].to(DEV))
        HL.DiceLoss().to(DEV)(lg, batch["label"][:, -1].long().to(DEV)).backward()
        torch.cuda.synchronize()
    return net, lg


_ORACLE = {}


def _oracle(c, dtype):
    """The oracle's run per channel count and precision, computed once."""
    if (c, dtype) not in _ORACLE:
        ctor = dict(in_channels=c, out_channels=3, final_sigmoid=False, f_maps=[32, 64])
        batch = O.synthetic_batch(2, c, (16, 16, 16), 3, 0, seed=77 + c)
        _ORACLE[(c, dtype)] = (ctor, batch) + _oracle_run(ctor, batch, dtype)
    return _ORACLE[(c, dtype)]


@pytest.mark.parametrize("c", [2, 4])
def test_multichannel_network_fp32_mode_against_the_oracle(c):
    """fp32 storage does not use the new path (the fp32 matrix instruction takes such layers): this guards the plumbing around it."""
    ctor, batch, ora, lo = _oracle(c, torch.float32)
    _, _, ora64, _ = _oracle(c, torch.float64)
    cond = {k: max(1.0, rel(p.grad, q.grad) / 1e-6) for (k, p), (_, q) in zip(ora.named_parameters(), ora64.named_parameters())}
    net, lg = _hip_run(ctor, batch, "fp32")
    tl, tg = NET_TOL["fp32"]
    assert rel(lg, lo) <= tl
    for (k, p), (_, q) in zip(net.named_parameters(), ora.named_parameters()):
        r = rel(p.grad, q.grad)
        assert r <= tg * cond[k], f"grad {k}: rel-L2 {r:.3e} (cond {cond[k]:.1f})"


@pytest.mark.parametrize("c", [2, 4])
def test_multichannel_network_bf16_within_the_references_own_drift(c, monkeypatch):
    """bf16 storage against the fp64 oracle, held to max(NET_TOL, 1.5 x the reference's own bf16 drift computed here); the first
    layer made no layout copy of the input and its statistics were fused."""
    ctor, batch, ora64, l64 = _oracle(c, torch.float64)
    _, _, ora16, l16 = _oracle(c, torch.bfloat16)
    drift_l = rel(l16, l64)
    drift_g = max(rel(p.grad, q.grad) for p, q in zip(ora16.parameters(), ora64.parameters()))
    copies, firsts = [], []
    real_to_cl, real_fwd = ops.to_cl, block._conv_fwd

    def spy_to_cl(x):
        if x.dim() == 5 and x.shape[1] == c and x.dtype == torch.float32 and not x.is_contiguous(memory_format=ops.CL):
            copies.append(tuple(x.shape))
        return real_to_cl(x)

    def spy_fwd(x, packed, cout, want_stats, *a, **kw):
        y, partial = real_fwd(x, packed, cout, want_stats, *a, **kw)
        if x.shape[1] == c:
            firsts.append((x.data_ptr(), x.dtype, partial is not None))
        return y, partial

    monkeypatch.setattr(ops, "to_cl", spy_to_cl)
    monkeypatch.setattr(block, "_conv_fwd", spy_fwd)
    data = batch["data"].to(DEV)
    with mednet_hip.precision("bf16"):
        net = O.keyed_init_(HM.ResidualUNet3D(**ctor)).to(DEV)
        lg = net(data)
        HL.DiceLoss().to(DEV)(lg, batch["label"][:, -1].long().to(DEV)).backward()
        torch.cuda.synchronize()
        assert L.lib().mednet_conv3d_fused_stats_chunks(2, 16, 16, 16, c, 32, 3, L.F32, L.BF16, config.conv_algo()) > 0
    assert copies == [], f"layout copies of the input: {copies}"
    assert firsts == [(data.data_ptr(), torch.float32, True)], firsts
    rl = rel(lg, l64)
    worst = max((rel(p.grad, q.grad), k) for (k, p), (_, q) in zip(net.named_parameters(), ora64.named_parameters()))
    tl, tg = max(NET_TOL["bf16"][0], 1.5 * drift_l), max(NET_TOL["bf16"][1], 1.5 * drift_g)
    print(f"[multichannel] c={c} bf16: logits {rl:.2e} (drift {drift_l:.2e}, bound {tl:.2e}) worst gradient {worst[0]:.2e} "
          f"({worst[1]}; drift {drift_g:.2e}, bound {tg:.2e})")
    assert rl <= tl and worst[0] <= tg, (rl, tl, worst, tg)


# ---------------------------------------------------------------------------------------------- trainer
CTOR2 = dict(in_channels=2, out_channels=4, final_sigmoid=False, f_maps=[32, 64])


def _train(graph, batches):
    from mednet_hip.train import SegmentationStep
    with mednet_hip.precision("bf16"):
        net = O.keyed_init_(HM.ResidualUNet3D(**CTOR2)).to(DEV)
        step = SegmentationStep(net, loss_weight=[0.05, 1, 1, 1.0], lr=1e-3, graph=graph)
        losses = [float(step({k: v.to(DEV) for k, v in b.items()})) for b in batches]
        torch.cuda.synchronize()
        flat = step.flat.flat.clone()
        step.flat.release()
    return losses, flat


def test_multichannel_training_steps_graph_equals_eager_and_repeat():
    """Three SegmentationSteps at in_channels = 2 (bf16: side-stream weight gradients, the GroupNorm form on the caller's stream):
    the captured graph against the eager step and two eager runs against each other, losses and parameters bit-identical."""
    batches = [O.synthetic_batch(2, 2, (16, 16, 16), 4, 0, seed=300 + i) for i in range(3)]
    before = block.C1GN_COUNT["fused"]
    e1, e2, gr = _train(False, batches), _train(False, batches), _train(True, batches)
    assert block.C1GN_COUNT["fused"] > before, "the GroupNorm form of the first layer's weight gradient did not run"
    assert all(np.isfinite(e1[0]))
    assert e1[0] == e2[0] and torch.equal(e1[1], e2[1]), "two eager runs differ"
    assert gr[0] == e1[0] and torch.equal(gr[1], e1[1]), (gr[0], e1[0])


def test_multichannel_landmark_step_and_validation_run():
    """LandmarkStep and both validation classes on in_channels = 2: finite losses."""
    from mednet_hip.train import LandmarkStep, LandmarkValidation, SegmentationValidation
    with mednet_hip.precision("bf16"):
        batch = {k: v.to(DEV) for k, v in O.synthetic_batch(2, 2, (16, 16, 16), 2, 3, seed=41).items()}
        net = O.keyed_init_(HM.ResidualUNet3D(in_channels=2, out_channels=5, final_sigmoid=False, f_maps=[32, 64])).to(DEV)
        step = LandmarkStep(net, class_weight=[0.05, 1.0], regression_weight=[0.015] * 3, regression="L2", lr=1e-3)
        tot, cl, rg = step(batch)
        assert all(np.isfinite(float(v)) for v in (tot, cl, rg))
        step.flat.release()
        val = LandmarkValidation(net, class_weight=[0.05, 1.0], regression_weight=[0.015] * 3, regression="L2")
        end = val.validation_epoch_end([val.validation_step(batch, 0)])
        assert all(np.isfinite(float(v)) for v in end["log"].values())
        sbatch = {k: v.to(DEV) for k, v in O.synthetic_batch(2, 2, (16, 16, 16), 4, 0, seed=42).items()}
        snet = O.keyed_init_(HM.ResidualUNet3D(**CTOR2)).to(DEV)
        sval = SegmentationValidation(snet, loss_weight=[0.05, 1, 1, 1.0])
        send = sval.validation_epoch_end([sval.validation_step(sbatch, 0)])
        assert all(np.isfinite(float(v)) for v in send["log"].values())


# ---------------------------------------------------------------------------------------------- end to end
def test_patch_sampler_batch_reaches_the_first_layer_without_a_copy(monkeypatch):
    """DevicePatchSampler on two synthetic 2-channel subjects of 24^3, one training step at 16^3 patches: the planar fp32 `data`
    tensor of the batch is the very memory the first layer's kernel reads."""
    from mednet_hip.sampler import DevicePatchSampler
    from mednet_hip.train import SegmentationStep
    rng = O._rng("mc:sampler")
    images = [(rng.standard_normal((2, 24, 24, 24)) * 2).astype(np.float32) for _ in range(2)]
    labels = [rng.integers(0, 4, size=(1, 24, 24, 24)).astype(np.uint8) for _ in range(2)]
    dev = DevicePatchSampler(images, labels, [16, 16, 16], samples_per_subject=2, device=DEV)
    np.random.seed(3)
    batch = dev.batch([0, 1, 2, 3])
    assert tuple(batch["data"].shape) == (4, 2, 16, 16, 16) and batch["data"].dtype == torch.float32
    seen = []
    real_fwd = block._conv_fwd

    def spy_fwd(x, packed, cout, want_stats, *a, **kw):
        if x.shape[1] == 2:
            seen.append((x.data_ptr(), a, kw))
        return real_fwd(x, packed, cout, want_stats, *a, **kw)

    monkeypatch.setattr(block, "_conv_fwd", spy_fwd)
    with mednet_hip.precision("bf16"):
        net = O.keyed_init_(HM.ResidualUNet3D(**CTOR2)).to(DEV)
        step = SegmentationStep(net, loss_weight=[0.05, 1, 1, 1.0], lr=1e-3)
        loss = float(step(batch))
        step.flat.release()
    assert np.isfinite(loss)
    assert len(seen) == 1 and seen[0][0] == batch["data"].data_ptr(), "the first layer read a copy of the batch"
    assert seen[0][1] == (L.NCDHW,) or seen[0][2].get("x_layout") == L.NCDHW


def test_grid_predictor_on_a_two_channel_volume_matches_the_oracle_loop():
    """GridPredictor on a 2-channel 24^3 volume against the oracle's loop (the agreement rule of tests/test_gpu_predict.py: the
    uint8 volumes agree except where a logit sits within float noise of a decision boundary), fp32 mode; in bf16 mode, where the
    first layer is the multi-channel kernel's, the predictor runs and returns a volume of that shape."""
    ctor = dict(in_channels=2, out_channels=5, final_sigmoid=False, f_maps=[8, 16])
    nh, patch, ov = 2, [16, 16, 16], [2, 3, 4]
    img = (O._rng("predict:mc").standard_normal((2, 24, 24, 24)) * 2).astype(np.float16)
    ora = O.keyed_init_(O.ResidualUNet3D(**ctor)).eval()

    def fwd(x):
        with torch.no_grad():
            return (ora(torch.from_numpy(x)) * 40.0).numpy()

    want = P.predict_volume(fwd, img, patch, ov, nh, batch_size=3, pad_kwargs={"mode": "symmetric"})

    class Scaled(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.m = m

        def forward(self, x):
            return self.m(x) * 40.0

    with mednet_hip.precision("fp32"):
        net = O.keyed_init_(HM.ResidualUNet3D(**ctor)).to(DEV)
        got = HP.GridPredictor(Scaled(net), patch, ov, num_heatmaps=nh, pad_mode="symmetric", batch_size=3)(img).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8
    assert (got[nh] != want[nh]).mean() < 2e-3                      # labels
    d = np.abs(got[:nh].astype(int) - want[:nh].astype(int))
    assert d.max() <= 1 and (d != 0).mean() < 2e-3                 # heat maps: truncation flips only
    ctor16 = dict(ctor, f_maps=[16, 32])   # (Cout % 16 == 0: the multi-channel kernel takes the first layer)
    with mednet_hip.precision("bf16"):
        assert L.lib().mednet_conv3d_cm_supported(2, 16, 3, L.F32, L.BF16, config.conv_algo()) == 1
        net16 = O.keyed_init_(HM.ResidualUNet3D(**ctor16)).to(DEV)
        out16 = HP.GridPredictor(net16, patch, ov, num_heatmaps=nh, pad_mode="symmetric", batch_size=3)(img)
        torch.cuda.synchronize()
    assert tuple(out16.shape) == want.shape and out16.dtype == torch.uint8
