"""Dice + cross-entropy through the matrix-core heads (class kind 2 of ops.head_seg for 5 .. 16 classes and of ops.head_landmark /
head_landmark_eval) and through the training and validation steps, on the MI355X (-m gpu).  Shapes and bounds are those of
tests/test_gpu_seg_heads.py (SHAPES, _compare) and of the CE heads' step tests (tests/test_gpu_ce_heads.py)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import nn as hnn
from mednet_hip import ops
from mednet_hip.unet import loss as HL
from mednet_hip.unet import model as HM
from oracle import ref_cpu as O

from fence import Fence
from gpu_util import DEV, TOL, assert_close, half_round, rel, rnd
from test_gpu_seg_heads import SHAPES, _compare, _count_calls, _inputs, _weights

pytestmark = pytest.mark.gpu
MODES = ["bf16", "fp16"]


def _gscale(mode):
    return 3.0 * 16384.0 if mode == "fp16" else 3.0  # (fp16 stores the feature gradient: scaled as train.LossScaler does)


def _dice_ce_cpu(z, y, w):
    return O.DiceLoss(weight=w)(z, y) + F.cross_entropy(z, y, weight=w)


# ------------------------------------------------------------------------------------------------ ops.head_seg, class kind 2
def _seg_pair(mode, x, w, b, lab_u8, wt, want_logits=False):
    c = w.shape[0]
    res, logits = {}, None
    with mednet_hip.precision(mode):
        for fused in (False, True):
            conv = hnn.Conv3d(32, c, 1, planar_output=True).to(DEV)
            with torch.no_grad():
                conv.weight.copy_(w)
                conv.bias.copy_(b)
            xg = ops.to_cl(x.to(DEV).to(mednet_hip.config.act_dtype())).requires_grad_(True)
            wd = None if wt is None else wt.to(DEV)
            if fused:
                assert ops.head_seg_supported(xg, 32, c, lab_u8)
                lg, loss = ops.head_seg(xg, conv.weight, conv.bias, conv._packed(), lab_u8, wd, 1e-5, class_loss="DICE_CE",
                                        want_logits=want_logits)
                assert (lg is not None) == want_logits
                logits = lg
            else:
                lg = conv(xg)
                loss = ops.dice_ce_loss(lg, lab_u8, wd, 1e-5)
                unfused_logits = lg.detach()
            (loss * _gscale(mode)).backward()
            res[fused] = (loss.detach(), xg.grad, conv.weight.grad, conv.bias.grad)
    return res, logits, unfused_logits


def _seg_case(mode, c, n, shape, weighted, classes=None, want_logits=False, tag=""):
    x, w, b, lab_vol = _inputs(mode, c, n, shape, classes)
    wt = _weights(c) if weighted else None
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    loss_r = _dice_ce_cpu(F.conv3d(xr, wr, br), lab_vol[:, -1].long(), wt)
    loss_r.backward()
    res, lg, lg0 = _seg_pair(mode, x, w, b, lab_vol.to(DEV)[:, -1], wt, want_logits)
    _compare(mode, f"{tag}{mode} C={c} n={n} {shape} DICE_CE w={int(weighted)}", res, (loss_r.detach(), xr.grad, wr.grad, br.grad), _gscale(mode))
    if want_logits:
        assert tuple(lg.shape) == (n, c) + shape and lg.dtype == torch.float32
        assert_close(lg, lg0, 1e-5, "logits written on request vs the VALU head's")
    return res


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", [5, 8, 9, 14, 16])
def test_seg_head_with_dice_ce_against_the_unfused_launches(mode, c):
    """ops.head_seg(class_loss="DICE_CE") against hnn.Conv3d(32, C, 1, planar_output=True) + ops.dice_ce_loss and against ATen on the CPU
    (O.DiceLoss + F.cross_entropy) from the same rounded features: loss 2e-6 (relative above 1), gradients 3e-3 rel-L2 against the
    unfused path, TOL[mode] / max(tol, 1e-4) against ATen -- test_gpu_seg_heads._compare, its SHAPES; weights on and off, the logits
    on request on one shape."""
    for k, (n, shape) in enumerate(SHAPES):
        _seg_case(mode, c, n, shape, weighted=bool((k + c) % 2), want_logits=(k == 2))
        if k == 2:
            _seg_case(mode, c, n, shape, weighted=not bool((k + c) % 2))


@pytest.mark.parametrize("mode", MODES)
def test_seg_head_with_dice_ce_and_three_of_fourteen_classes_present(mode):
    _seg_case(mode, 14, 3, (12, 10, 6), True, classes=(0, 6, 13), tag="three classes ")


def test_seg_head_with_dice_ce_out_of_range_label_and_refusals():
    """A uint8 label >= ncls: NaN loss, the backward still runs; sigmoid or an ignore_index with "DICE_CE" is refused."""
    with mednet_hip.precision("bf16"):
        conv = hnn.Conv3d(32, 14, 1, planar_output=True).to(DEV)
        x = ops.to_cl(rnd("sgdc-bad", 2, 32, 8, 8, 8).to(DEV).bfloat16()).requires_grad_(True)
        lab = torch.zeros((2, 8, 8, 8), dtype=torch.uint8, device=DEV)
        lab[1, 3, 4, 5] = 14
        _, loss = ops.head_seg(x, conv.weight, conv.bias, conv._packed(), lab, None, class_loss="DICE_CE")
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isnan(loss) and x.grad.shape == x.shape and tuple(conv.weight.grad.shape) == (14, 32, 1, 1, 1)
        lab[1, 3, 4, 5] = 13
        _, loss = ops.head_seg(x, conv.weight, conv.bias, conv._packed(), lab, None, class_loss="DICE_CE")
        assert torch.isfinite(loss)
        for kw in (dict(sigmoid=True), dict(ignore_index=3), dict(ignore_index=-100)):
            with pytest.raises(ValueError, match="DICE_CE"):
                ops.head_seg(x, conv.weight, conv.bias, conv._packed(), lab, None, class_loss="DICE_CE", **kw)


# ------------------------------------------------------------------------------------------------ ops.head_landmark, class kind 2
def _landmark_case(mode, n, shape, nh, ncls, kind):
    tag = f"lmdc{nh}{ncls}{n}{shape}"
    m = nh + ncls
    x = half_round(rnd(tag + "x", n, 32, *shape), mode)
    w, b = rnd(tag + "w", m, 32, 1, 1, 1, scale=0.3), rnd(tag + "b", m)
    g = np.random.Generator(np.random.PCG64(85 + nh))
    hm = torch.from_numpy(g.integers(0, 256, size=(n, nh) + shape).astype(np.uint8))
    lab = torch.from_numpy(g.integers(0, ncls, size=(n, 1) + shape).astype(np.uint8))
    vol = torch.cat([hm, lab], dim=1)
    cw = _weights(ncls)
    rw = [0.015 + 0.003 * i for i in range(nh)]
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out_r = F.conv3d(xr, wr, br)
    cl_r = _dice_ce_cpu(out_r[:, nh:], lab[:, 0].long(), cw)
    reg = F.mse_loss if kind == "L2" else F.l1_loss
    rg_r = sum(rw[c] * reg(out_r[:, c], hm[:, c].float()) for c in range(nh))
    (cl_r + rg_r).backward()
    gs = _gscale(mode)
    res, extra = {}, {}
    with mednet_hip.precision(mode):
        vd = vol.to(DEV)
        hmd, labd = vd[:, :nh], vd[:, nh]
        for fused in (False, True):
            conv = hnn.Conv3d(32, m, 1, planar_output=True).to(DEV)
            with torch.no_grad():
                conv.weight.copy_(w)
                conv.bias.copy_(b)
            xg = ops.to_cl(x.to(DEV).to(mednet_hip.config.act_dtype())).requires_grad_(True)
            if fused:
                assert ops.head_landmark_supported(xg, 32, nh, ncls, hmd, labd)
                cl, rg = ops.head_landmark(xg, conv.weight, conv.bias, conv._packed(), hmd, labd, cw.to(DEV), rw, kind, 1e-5,
                                           class_loss="DICE_CE")
                with torch.no_grad():
                    extra["eval"] = ops.head_landmark_eval(xg.detach(), conv.weight, conv.bias, conv._packed(), hmd, labd, cw.to(DEV), rw, kind,
                                                           1e-5, None, "DICE_CE")
            else:
                out = conv(xg)
                cl = ops.dice_ce_loss(out[:, nh:], labd, cw.to(DEV), 1e-5)
                rg = HL.HeatmapRegressionLoss(rw, kind).to(DEV)(out[:, :nh], hmd)
                extra["metric"] = ops.per_channel_dice(out[:, nh:].detach(), labd)
            ((cl + rg) * gs).backward()
            res[fused] = (cl.detach(), xg.grad, conv.weight.grad, conv.bias.grad)
            extra[fused] = rg.detach()
    what = f"landmark {mode} nh={nh} ncls={ncls} {kind} n={n} {shape} DICE_CE"
    _compare(mode, what, res, (cl_r.detach(), xr.grad, wr.grad, br.grad), gs)
    r1, r0 = float(extra[True]), float(extra[False])
    assert abs(r1 - r0) <= 2e-6 * max(1.0, abs(r0)), (what, r1, r0)
    rr = float(rg_r.detach())
    assert abs(r1 - rr) <= TOL[mode] * max(1.0, abs(rr)), (what, r1, rr)
    # the forward-only form: the same two losses bit for bit, and dice_metric of the class channels at the landmark validation test's bound
    ecl, erg, edice = extra["eval"]
    assert torch.equal(ecl, res[True][0]) and torch.equal(erg, extra[True]), what
    for k in range(ncls):
        a, b_ = float(edice[k]), float(extra["metric"][k])
        assert abs(a - b_) <= 1e-5 * max(1.0, abs(b_)), (what, k, a, b_)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nh,ncls,kind", [(5, 3, "L1"), (16, 2, "L2")])
def test_landmark_head_with_dice_ce_against_the_unfused_launches(mode, nh, ncls, kind):
    """ops.head_landmark(class_loss="DICE_CE") against the 1x1x1 head + ops.dice_ce_loss + the heat-map regression as separate launches
    and against ATen on the CPU, on SHAPES at _compare's bounds; ops.head_landmark_eval gives the same losses and dice_metric."""
    for n, shape in SHAPES:
        _landmark_case(mode, n, shape, nh, ncls, kind)


def test_landmark_head_with_dice_ce_out_of_range_label():
    with mednet_hip.precision("bf16"):
        conv = hnn.Conv3d(32, 5, 1, planar_output=True).to(DEV)
        x = ops.to_cl(rnd("lmdc-bad", 2, 32, 8, 8, 8).to(DEV).bfloat16())
        vol = torch.zeros((2, 4, 8, 8, 8), dtype=torch.uint8, device=DEV)
        ok, _ = ops.head_landmark(x, conv.weight, conv.bias, conv._packed(), vol[:, :3], vol[:, 3], class_loss="DICE_CE")
        vol[1, 3, 3, 4, 5] = 2
        bad, _ = ops.head_landmark(x, conv.weight, conv.bias, conv._packed(), vol[:, :3], vol[:, 3], class_loss="DICE_CE")
        assert torch.isfinite(ok) and torch.isnan(bad)
        with pytest.raises(RuntimeError, match="softmax form without ignore_index"):
            ops.head_landmark(x, conv.weight, conv.bias, conv._packed(), vol[:, :3], vol[:, 3], ignore_index=1, class_loss="DICE_CE")


# ------------------------------------------------------------------------------------------------ the training steps
SEG_SHAPE = (32, 32, 32)


def _ctor(c):
    return dict(in_channels=1, out_channels=c, final_sigmoid=False, f_maps=[32, 64])


def _w(c):
    return [0.05] + [1.0] * (c - 1)


def _seg_step(mode, c, fused, batch, graph=None, steps=0):
    """One _fwd_bwd (steps = 0) -> (loss, flat gradient / scale, per-parameter names, calls of the fused nodes); or `steps` whole
    steps -> (losses, parameters, calls)."""
    from mednet_hip.train import SegmentationStep
    old = ops.FUSE_HEAD_LOSS
    ops.FUSE_HEAD_LOSS = fused
    valu, real_valu = _count_calls(ops.HeadDiceCEFn)
    seg, real_seg = _count_calls(ops.HeadSegFn)
    try:
        with mednet_hip.precision(mode):
            net = O.keyed_init_(HM.ResidualUNet3D(**_ctor(c))).to(DEV)
            step = SegmentationStep(net, loss_weight=_w(c), lr=1e-3, loss="DICE_CE", graph=graph)
            assert type(step.loss) is HL.DiceCELoss
            scale = step.scaler.snapshot()[0] if step.scaler is not None else 1.0
            if steps:
                losses = [float(step(batch)) for _ in range(steps)]
                torch.cuda.synchronize()
                out = (losses, step.flat.flat.clone(), step.scaler.skipped_steps() if step.scaler is not None else 0)
            else:
                (loss,) = step._fwd_bwd(batch)
                torch.cuda.synchronize()
                names = [(nm, off, p.numel()) for (nm, p), off in zip(net.named_parameters(), step.flat.offsets)]
                out = (float(loss), (step.flat.grad / scale).clone(), names)
            step.flat.release()
    finally:
        ops.HeadDiceCEFn.apply, ops.HeadSegFn.apply = real_valu, real_seg
        ops.FUSE_HEAD_LOSS = old
    return out + ((valu["n"], seg["n"]),)


@functools.lru_cache(maxsize=None)
def _seg_batch(c):
    return O.synthetic_batch(2, 1, SEG_SHAPE, c, 0, seed=61 + c)


@functools.lru_cache(maxsize=None)
def _seg_oracle(c):
    batch = _seg_batch(c)
    ora = O.keyed_init_(O.ResidualUNet3D(**_ctor(c)))
    loss = O.seg_training_step(ora, lambda z, y: _dice_ce_cpu(z, y, torch.tensor(_w(c))), batch)
    loss.backward()
    return float(loss.detach()), [q.grad.clone() for q in ora.parameters()]


@pytest.mark.parametrize("mode,tol_l,tol_g", [("fp32", 2e-4, 2e-3), ("bf16", 2e-2, 5e-2), ("fp16", 1e-2, 3e-2)])
def test_segmentation_step_with_4_classes_takes_the_fused_head(mode, tol_l, tol_g):
    """SegmentationStep(loss="DICE_CE") on ResidualUNet3D(1, 4, f_maps [32, 64]) at 32^3: head + loss as ops.HeadDiceCEFn (once) against
    the two-node step (final_conv + DiceCELoss) -- loss and every gradient in front of the head bit for bit, the head's own to 1e-5,
    the fused CE head's step bounds -- and against the live CPU oracle at the CE-head oracle tests' tolerances."""
    batch = {k: v.to(DEV) for k, v in _seg_batch(4).items()}
    l1, f1, names, (nv1, ns1) = _seg_step(mode, 4, True, batch)
    l0, f0, _, (nv0, ns0) = _seg_step(mode, 4, False, batch)
    assert (nv1, ns1, nv0, ns0) == (1, 0, 0, 0)
    assert l1 == l0, (l1, l0)
    for name, off, cnt in names:
        a, b = f1[off:off + cnt], f0[off:off + cnt]
        if name.startswith("final_conv."):
            assert_close(a, b, 1e-5, name)
        else:
            assert torch.equal(a, b), f"{name}: gradient differs between the fused and the two-node step"
    lo, go = _seg_oracle(4)
    worst = max(rel(f1[off:off + cnt].view_as(q), q) for (_, off, cnt), q in zip(names, go))
    print(f"[seg step DICE_CE 4 classes {mode}] loss {l1:.8f} / oracle {lo:.8f}; worst grad vs oracle {worst:.2e}")
    assert abs(l1 - lo) <= tol_l * max(1.0, abs(lo)), (l1, lo)
    assert worst <= tol_g, worst


@pytest.mark.parametrize("mode,tol_l,tol_g", [("bf16", 2e-2, 5e-2), ("fp16", 1e-2, 3e-2)])
def test_segmentation_step_with_14_classes_takes_the_wide_node(mode, tol_l, tol_g):
    """The same with 14 classes: ops.HeadSegFn with class kind 2 (once) against the two-node step -- loss 2e-6, flat gradient 3e-3
    rel-L2 -- and against the live CPU oracle; the bounds of test_gpu_seg_heads' 14-class step test."""
    batch = {k: v.to(DEV) for k, v in _seg_batch(14).items()}
    l1, f1, names, (nv1, ns1) = _seg_step(mode, 14, True, batch)
    l0, f0, _, (nv0, ns0) = _seg_step(mode, 14, False, batch)
    assert (nv1, ns1, nv0, ns0) == (0, 1, 0, 0)
    e = float((f1 - f0).norm() / f0.norm())
    lo, go = _seg_oracle(14)
    worst = max(rel(f1[off:off + cnt].view_as(q), q) for (_, off, cnt), q in zip(names, go))
    print(f"[seg step DICE_CE 14 classes {mode}] loss {l1:.8f} / two-node {l0:.8f} / oracle {lo:.8f}; flat grad vs two-node {e:.2e}; "
          f"worst grad vs oracle {worst:.2e}")
    assert torch.isfinite(f1).all()
    assert abs(l1 - l0) <= 2e-6 * max(1.0, abs(l0)), (l1, l0)
    assert e <= 3e-3, e
    assert abs(l1 - lo) <= tol_l * max(1.0, abs(lo)), (l1, lo)
    assert worst <= tol_g, worst


def test_17_classes_take_the_two_node_path_with_the_one_pass_loss():
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(2, 1, (16, 16, 16), 17, 0, seed=7).items()}
    calls, real = _count_calls(ops.DiceCELossFn)
    try:
        loss, flat, _, (nv, ns) = _seg_step("bf16", 17, True, batch)
    finally:
        ops.DiceCELossFn.apply = real
    assert (nv, ns, calls["n"]) == (0, 0, 1) and np.isfinite(loss) and torch.isfinite(flat).all()


@pytest.mark.parametrize("c", [4, 14])
def test_segmentation_steps_repeat_and_graph_equals_eager(c):
    """Three whole steps (bf16): two eager runs and the captured graph give the same losses and parameters bit for bit."""
    batch = {k: v.to(DEV) for k, v in _seg_batch(c).items()}
    e1, e2, gr = (_seg_step("bf16", c, True, batch, graph=g, steps=3) for g in (False, False, True))
    assert all(np.isfinite(e1[0])) and sum(e1[3]) == 3 and sum(gr[3]) >= 1
    assert e1[0] == e2[0] and torch.equal(e1[1], e2[1]), "two eager runs differ"
    assert gr[0] == e1[0] and torch.equal(gr[1], e1[1]), (gr[0], e1[0])


@pytest.mark.parametrize("c", [4, 14])
def test_fp16_segmentation_step_takes_its_step_behind_the_loss_scaler(c):
    batch = {k: v.to(DEV) for k, v in _seg_batch(c).items()}
    before = None
    with mednet_hip.precision("fp16"):
        before = O.keyed_init_(HM.ResidualUNet3D(**_ctor(c))).to(DEV)
        before = torch.cat([p.detach().flatten() for p in before.parameters()])
    losses, params, skipped, calls = _seg_step("fp16", c, True, batch, steps=2)
    assert skipped == 0 and all(np.isfinite(losses)) and sum(calls) == 2
    assert torch.isfinite(params).all() and losses[1] != losses[0]
    assert float(params.abs().sum()) != float(before.abs().sum()), "the parameters did not move"


def test_segmentation_validation_with_dice_ce():
    """SegmentationValidation(loss="DICE_CE"): val_loss is the compound loss of the eval-mode outputs (against the CPU oracle), the Dice
    metrics are there as for the other kinds."""
    from mednet_hip.train import SegmentationValidation
    batch = _seg_batch(4)
    ora = O.keyed_init_(O.ResidualUNet3D(**_ctor(4))).eval()
    with torch.no_grad():
        out = ora(batch["data"])
        want = float(_dice_ce_cpu(out, batch["label"][:, -1].long(), torch.tensor(_w(4))))
    with mednet_hip.precision("fp32"):
        net = O.keyed_init_(HM.ResidualUNet3D(**_ctor(4))).to(DEV)
        val = SegmentationValidation(net, loss_weight=_w(4), loss="DICE_CE")
        res = val.validation_step({k: v.to(DEV) for k, v in batch.items()}, 1)
    assert sorted(res) == ["val_dice0", "val_dice1", "val_dice2", "val_dice3", "val_loss"]
    assert abs(float(res["val_loss"]) - want) <= 2e-5 * max(1.0, abs(want)), (float(res["val_loss"]), want)


# ---- LandmarkStep / LandmarkValidation
NH, NCLS = 16, 2
LM_CTOR = dict(in_channels=1, out_channels=NH + NCLS, final_sigmoid=False, f_maps=[32, 64])
LM_REGW = [0.015 + 0.003 * i for i in range(NH)]
LM_CW = [0.05, 1.0]


@functools.lru_cache(maxsize=None)
def _lm_batch():
    return O.synthetic_batch(2, 1, SEG_SHAPE, NCLS, NH, seed=4444)


def _lm_step(mode, fused, batch, graph=None, steps=0):
    from mednet_hip.train import LandmarkStep
    old = ops.FUSE_HEAD_LOSS
    ops.FUSE_HEAD_LOSS = fused
    calls, real = _count_calls(ops.HeadLandmarkFn)
    try:
        with mednet_hip.precision(mode):
            net = O.keyed_init_(HM.ResidualUNet3D(**LM_CTOR)).to(DEV)
            step = LandmarkStep(net, class_weight=LM_CW, regression_weight=LM_REGW, regression="L2", lr=1e-3, class_loss="DICE_CE", graph=graph)
            scale = step.scaler.snapshot()[0] if step.scaler is not None else 1.0
            if steps:
                losses = [tuple(float(v) for v in step(batch)) for _ in range(steps)]
                torch.cuda.synchronize()
                out = (losses, step.flat.flat.clone(), step.scaler.skipped_steps() if step.scaler is not None else 0)
            else:
                tot, cl, rg = step._fwd_bwd(batch)
                torch.cuda.synchronize()
                names = [(nm, off, p.numel()) for (nm, p), off in zip(net.named_parameters(), step.flat.offsets)]
                out = ((float(tot), float(cl), float(rg)), (step.flat.grad / scale).clone(), names)
            step.flat.release()
    finally:
        ops.HeadLandmarkFn.apply = real
        ops.FUSE_HEAD_LOSS = old
    return out + (calls["n"],)


@functools.lru_cache(maxsize=None)
def _lm_oracle():
    ora = O.keyed_init_(O.ResidualUNet3D(**LM_CTOR))
    tot, cl, rg = O.ldmk_training_step(ora, lambda z, y: _dice_ce_cpu(z, y, torch.tensor(LM_CW)), nn.MSELoss(), LM_REGW, _lm_batch())
    tot.backward()
    return (float(tot), float(cl), float(rg)), [q.grad.clone() for q in ora.parameters()]


@pytest.mark.parametrize("mode,tol_l,tol_g", [("bf16", 2e-2, 5e-2), ("fp16", 1e-2, 3e-2)])
def test_landmark_step_with_dice_ce(mode, tol_l, tol_g):
    """LandmarkStep(class_loss="DICE_CE") at 32^3 (16 heat maps + 2 classes, f_maps [32, 64]): the one matrix-core node against the
    stock launches -- losses 2e-6 (relative above 1), gradients 3e-3 rel-L2, the CE landmark head's bounds -- and against the live
    CPU oracle at the tolerances of the CE landmark step's oracle test."""
    batch = {k: v.to(DEV) for k, v in _lm_batch().items()}
    (t1, c1, r1), f1, names, n1 = _lm_step(mode, True, batch)
    (t0, c0, r0), f0, _, n0 = _lm_step(mode, False, batch)
    assert (n1, n0) == (1, 0)
    e = float((f1 - f0).norm() / f0.norm())
    (to, co, ro), go = _lm_oracle()
    worst = max(rel(f1[off:off + cnt].view_as(q), q) for (_, off, cnt), q in zip(names, go))
    print(f"[landmark step DICE_CE {mode}] class {c1:.8f} / stock {c0:.8f} / oracle {co:.8f}; reg {r1:.5f} / {r0:.5f} / {ro:.5f}; "
          f"grads vs stock {e:.2e}; worst grad vs oracle {worst:.2e}")
    assert torch.isfinite(f1).all()
    assert abs(c1 - c0) <= 2e-6 * max(1.0, abs(c0)), (c1, c0)
    assert abs(r1 - r0) <= 2e-6 * max(1.0, abs(r0)), (r1, r0)
    assert e <= 3e-3, e
    for a, b in ((c1, co), (r1, ro), (t1, to)):
        assert abs(a - b) <= tol_l * max(1.0, abs(b)), (mode, a, b)
    assert worst <= tol_g, (mode, worst)


def test_landmark_steps_repeat_graph_equals_eager_and_fp16_takes_its_step():
    batch = {k: v.to(DEV) for k, v in _lm_batch().items()}
    e1, e2, gr = (_lm_step("bf16", True, batch, graph=g, steps=3) for g in (False, False, True))
    assert e1[3] == 3 and gr[3] >= 1
    assert e1[0] == e2[0] and torch.equal(e1[1], e2[1]), "two eager runs differ"
    assert gr[0] == e1[0] and torch.equal(gr[1], e1[1]), (gr[0], e1[0])
    losses, params, skipped, n = _lm_step("fp16", True, batch, steps=2)
    assert skipped == 0 and n == 2 and all(np.isfinite(v) for t in losses for v in t) and losses[0] != losses[1]
    assert torch.isfinite(params).all()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_landmark_validation_with_dice_ce(mode):
    """LandmarkValidation(class_loss="DICE_CE") against the composition on the CPU oracle; the single fused pass (bf16) and the unfused
    form agree to fp32 summation order -- the structure and bounds of the CE landmark validation test."""
    from mednet_hip.train import LandmarkValidation
    ctor = dict(in_channels=1, out_channels=5, final_sigmoid=False, f_maps=[32, 64])
    batch = O.synthetic_batch(2, 1, (16, 16, 16), 2, 3, seed=700)
    regw, cw = [0.015, 0.02, 0.001], torch.tensor([0.05, 1.0])
    ora = O.keyed_init_(O.ResidualUNet3D(**ctor)).eval()
    with torch.no_grad():
        out = ora(batch["data"].float())
        hm, lab = batch["label"][:, :-1].float(), batch["label"][:, -1].long()
        cl = _dice_ce_cpu(out[:, 3:], lab, cw)
        rg = sum(regw[c] * F.mse_loss(out[:, c], hm[:, c]) for c in range(3))
        dice = O.dice_metric(out[:, 3:], lab)
        want = {"val_loss": rg + cl, "val_class_loss": cl, "val_regression_loss": rg, "val_dice0": dice[0], "val_dice1": dice[1]}
    tol = {"fp32": 2e-5, "bf16": 3e-2}[mode]
    res, calls = {}, {True: 0, False: 0}
    old, real = ops.FUSE_HEAD_LOSS, ops.head_landmark_eval
    try:
        for fused in (True, False):
            ops.FUSE_HEAD_LOSS = fused

            def counted(*a, **k):
                calls[fused] += 1
                return real(*a, **k)
            ops.head_landmark_eval = counted
            with mednet_hip.precision(mode):
                net = O.keyed_init_(HM.ResidualUNet3D(**ctor)).to(DEV)
                val = LandmarkValidation(net, class_weight=[0.05, 1.0], regression_weight=regw, class_loss="DICE_CE")
                o = val.validation_step({k: v.to(DEV) for k, v in batch.items()}, 1)
            assert list(o.keys()) == list(want.keys())
            res[fused] = {k: float(v) for k, v in o.items()}
    finally:
        ops.FUSE_HEAD_LOSS, ops.head_landmark_eval = old, real
    assert calls == {True: 1 if mode != "fp32" else 0, False: 0}, calls
    for fused in (True, False):
        for k, v in want.items():
            assert abs(res[fused][k] - float(v)) <= tol * max(1.0, abs(float(v))), (fused, k, res[fused][k], float(v))
    for k in want:
        assert abs(res[True][k] - res[False][k]) <= 1e-5 * max(1.0, abs(res[False][k])), (k, res[True][k], res[False][k])


# ------------------------------------------------------------------------------------------------ footprint
def _same(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        assert not bool(torch.isnan(a.float()).any()), f"{what}: result {k} holds a NaN"
        assert torch.equal(a, b), f"{what}: result {k} differs from the unfenced call"


def _finish(fence, what, outputs, ws_sites, ws_bytes):
    for t in outputs:
        assert fence.owns(t), f"{what}: an output of shape {tuple(t.shape)} was not allocated inside the fence"
    asked = [r for r in fence.ws_requests if r[2] in ws_sites]
    assert len(asked) == len(ws_sites) and all(r[0] == ws_bytes and r[1] == ws_bytes for r in asked), (what, fence.ws_requests)
    fence.check()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("head", ["seg", "landmark"])
def test_matrix_core_heads_with_kind_two_inside_guard_bands(mode, head):
    """ops.head_seg (9 classes) and ops.head_landmark (5 heat maps + 3 classes) with "DICE_CE", forward and backward inside the fence:
    the uint8 volume ENDS with the class map's last byte, the workspace is exactly the head's query, the results equal the unfenced
    run bit for bit, every guard byte is intact."""
    n, shape = 3, (12, 10, 6)
    sp = int(np.prod(shape))
    nh, ncls = (0, 9) if head == "seg" else (5, 3)
    m = nh + ncls
    g = np.random.Generator(np.random.PCG64(89))
    vol = torch.cat([torch.from_numpy(g.integers(0, 256, size=(n, max(nh, 1)) + shape).astype(np.uint8)),
                     torch.from_numpy(g.integers(0, ncls, size=(n, 1) + shape).astype(np.uint8))], dim=1).to(DEV)
    off = max(nh, 1)
    cw = _weights(ncls).to(DEV)

    def run(put):
        with mednet_hip.precision(mode):
            conv = hnn.Conv3d(32, m, 1, planar_output=True).to(DEV)
            with torch.no_grad():
                conv.weight.copy_(rnd(f"fdw{m}", m, 32, 1, 1, 1, scale=0.3))
                conv.bias.copy_(rnd(f"fdb{m}", m))
            w, b = put(conv.weight.detach()).requires_grad_(True), put(conv.bias.detach()).requires_grad_(True)
            pk = ops.pack_conv_weight(w.detach(), 1, False)
            x = put(ops.to_cl(rnd(f"fdx{n}{shape}", n, 32, *shape).to(DEV).to(mednet_hip.config.act_dtype()))).requires_grad_(True)
            v = put(vol)
            if head == "seg":
                _, loss = ops.head_seg(x, w, b, pk, v[:, off], put(cw), class_loss="DICE_CE")
                outs = (loss,)
            else:
                cl, rg = ops.head_landmark(x, w, b, pk, v[:, :nh], v[:, off], put(cw), None, "L1", class_loss="DICE_CE")
                loss, outs = cl + rg, (cl, rg)
            loss.backward(put(torch.tensor(_gscale(mode), device=DEV)))
            torch.cuda.synchronize()
        return tuple(t.detach() for t in outs) + (x.grad, w.grad, b.grad)
    want = run(lambda t: t)
    lib = L.lib()
    need = lib.mednet_head_seg_ws_bytes(n, sp, ncls) if head == "seg" else lib.mednet_head_landmark_ws_bytes(n, sp, nh, ncls)
    with Fence() as fence:
        got = run(fence.put)
        what = f"head_{head} DICE_CE {mode}"
        _same(got, want, what)
        _finish(fence, what, got[:1 if head == "seg" else 2], ("forward" if head == "seg" else "_landmark_fwd", "__init__"), need)
