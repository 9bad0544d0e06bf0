"""The cross-entropy forms of the two fused heads (segmentation: head_loss.hip, landmark: head_mfma.hip), the trainer's CE branches
and train.LandmarkValidation, on the MI355X (-m gpu)."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mednet_hip
from mednet_hip import nn as hnn
from mednet_hip import ops
from mednet_hip.unet import model as HM
from oracle import ref_cpu as O

from gpu_util import DEV, TOL, assert_close, rel, rnd

pytestmark = pytest.mark.gpu
MODES = ["fp32", "bf16", "fp16"]


def _prep(mode, x):
    return x.bfloat16().float() if mode == "bf16" else (x.half().float() if mode == "fp16" else x)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin,cout,shape,n,labels_u8,weighted,ignore", [
    (32, 4, (9, 11, 21), 2, True, True, -100), (32, 2, (16, 16, 32), 3, False, True, -100), (64, 4, (8, 12, 10), 2, True, False, 3),
    (16, 2, (5, 7, 33), 1, True, True, 255), (16, 3, (12, 8, 8), 2, False, False, 1), (64, 1, (4, 6, 7), 2, False, True, -100),
    (32, 3, (6, 10, 12), 2, True, True, 0)])
def test_fused_head_ce_against_the_unfused_launches(mode, cin, cout, shape, n, labels_u8, weighted, ignore):
    """ops.head_ce (mednet_head_ce_fwd / _bwd) against final_conv + ops.cross_entropy as two nodes: logits, loss, feature gradient
    BIT-identical, dW / db to 1e-5, all within the mode's tolerance of ATen F.cross_entropy on the CPU.  Label forms: int64, and the
    last channel of a uint8 volume where it lies; ignore_index values that occur in the labels."""
    tag = f"hce{cin}{cout}{shape}{n}"
    x, w, b = _prep(mode, rnd(tag + "x", n, cin, *shape)), rnd(tag + "w", cout, cin, 1, 1, 1, scale=0.3), rnd(tag + "b", cout)
    g = np.random.Generator(np.random.PCG64(78))
    lab_vol = torch.from_numpy(g.integers(0, cout, size=(n, 2) + shape).astype(np.uint8))
    if ignore == 255:
        lab_vol[:, -1, ::3] = 255  # (voxels the loss ignores)
    wt = torch.tensor([0.05, 1.0, 0.7, 1.3][:cout]) if weighted else None
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    lr = F.conv3d(xr, wr, br)
    loss_r = F.cross_entropy(lr, lab_vol[:, -1].long(), weight=wt, ignore_index=ignore)
    loss_r.backward()
    gscale = 3.0 * 16384.0 if mode == "fp16" else 3.0  # (fp16 stores the feature gradient: scaled as train.LossScaler does)
    res = {}
    with mednet_hip.precision(mode):
        for fused in (False, True):
            conv = hnn.Conv3d(cin, cout, 1, planar_output=True).to(DEV)
            with torch.no_grad():
                conv.weight.copy_(w)
                conv.bias.copy_(b)
            xg = ops.to_cl(x.to(DEV).to(mednet_hip.config.act_dtype())).requires_grad_(True)
            lab_dev = lab_vol.to(DEV)
            lab = lab_dev[:, -1] if labels_u8 else lab_dev[:, -1].long()
            wd = None if wt is None else wt.to(DEV)
            if fused:
                assert ops.head_ce_supported(xg, cin, cout, lab)
                lg, loss = ops.head_ce(xg, conv.weight, conv.bias, conv._packed(), lab, wd, ignore)
            else:
                lg = conv(xg)
                loss = ops.cross_entropy(lg, lab.long(), wd, ignore)
            (loss * gscale).backward()
            res[fused] = (lg.detach(), loss.detach(), xg.grad, conv.weight.grad, conv.bias.grad)
    (l0, s0, dx0, dw0, db0), (l1, s1, dx1, dw1, db1) = res[False], res[True]
    assert torch.equal(l0, l1), "logits differ between the fused and the unfused head"
    assert torch.equal(s0, s1), (float(s0), float(s1))
    assert torch.equal(dx0, dx1), "feature gradient differs between the fused and the unfused path"
    assert_close(dw1, dw0, 1e-5, "dW fused vs unfused")
    assert_close(db1, db0, 1e-5, "db fused vs unfused")
    tol = TOL[mode]
    assert_close(l1, lr, tol, "logits vs ATen")
    assert abs(float(s1) - float(loss_r)) <= tol * max(1.0, abs(float(loss_r)))
    assert_close(dx1.float() / gscale, xr.grad, max(tol, 1e-4), "dx vs ATen")
    assert_close(dw1 / gscale, wr.grad, max(tol, 1e-4), "dW vs ATen")
    assert_close(db1 / gscale, br.grad, max(tol, 1e-4), "db vs ATen")


def test_fused_head_ce_out_of_range_label_poisons_the_loss():
    """A label outside [0, C) that is not ignore_index: NaN loss (class_loss_fwd_kernel<CE>'s rule), an ignored one changes nothing."""
    with mednet_hip.precision("bf16"):
        conv = hnn.Conv3d(32, 2, 1, planar_output=True).to(DEV)
        x = ops.to_cl(rnd("hce-bad", 2, 32, 8, 8, 8).to(DEV).bfloat16())
        lab = torch.zeros((2, 8, 8, 8), dtype=torch.uint8, device=DEV)
        lab[1, 3, 4, 5] = 7
        _, loss = ops.head_ce(x, conv.weight, conv.bias, conv._packed(), lab, None, -100)
        assert torch.isnan(loss)
        _, loss = ops.head_ce(x, conv.weight, conv.bias, conv._packed(), lab, None, 7)
        assert torch.isfinite(loss)


@pytest.mark.parametrize("mode,net_cls", [("bf16", "ResidualUNet3D"), ("fp32", "ResidualUNet3D"), ("fp16", "ResidualUNet3D"),
                                          ("bf16", "UNet3D"), ("fp16", "UNet3D")])
def test_fused_head_ce_step_equals_the_two_node_step(mode, net_cls):
    """train.SegmentationStep(loss="CE") with head + cross-entropy as one node (ops.head_ce) against the same step with
    MEDNET_FUSE_HEAD_LOSS off: loss and every gradient in front of the head BIT-identical, the head's own gradients to 1e-5.
    UNet3D ('gcr') ends in conv -> ReLU: its activation derivative is folded into the stored feature gradient (the FOLD form of
    head_dice_bwd_kernel<..., CE = true>) and that layer skips its own activation pass."""
    from mednet_hip.train import SegmentationStep
    ctor = dict(in_channels=1, out_channels=4, final_sigmoid=False, f_maps=[32, 64])
    make = getattr(HM, net_cls)
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(2, 1, (24, 40, 32), 4, 0, seed=31).items()}
    res = {}
    old = ops.FUSE_HEAD_LOSS
    try:
        for fused in (False, True):
            ops.FUSE_HEAD_LOSS = fused
            with mednet_hip.precision(mode):
                net = O.keyed_init_(make(**ctor)).to(DEV)
                step = SegmentationStep(net, loss_weight=[0.05, 1.0, 1.0, 1.0], lr=1e-3, loss="CE")
                calls = {"n": 0, "folded": 0}
                real = ops.HeadCEFn.apply

                def counted(*a):
                    calls["n"] += 1
                    calls["folded"] += int(getattr(a[0], "_mednet_actmask", None) is not None and ops._gn3_hook_of(a[0], a[0].dtype) is None)
                    return real(*a)
                ops.HeadCEFn.apply = counted
                try:
                    (loss,) = step._fwd_bwd(batch)
                finally:
                    ops.HeadCEFn.apply = real
                torch.cuda.synchronize()
                names = [(nm, off, p.numel()) for (nm, p), off in zip(net.named_parameters(), step.flat.offsets)]
                res[fused] = (float(loss), step.flat.grad.clone(), calls["n"], calls["folded"])
                step.flat.release()
    finally:
        ops.FUSE_HEAD_LOSS = old
    assert res[True][2] == 1 and res[False][2] == 0, "the fused CE node was not (or wrongly) taken"
    assert res[True][3] == int(net_cls == "UNet3D"), "the activation fold was not (or wrongly) taken"
    assert res[True][0] == res[False][0], (res[True][0], res[False][0])
    for name, off, cnt in names:
        a, b = res[True][1][off:off + cnt], res[False][1][off:off + cnt]
        if name.startswith("final_conv."):
            assert_close(a, b, 1e-5, name)
        else:
            assert torch.equal(a, b), f"{name}: gradient differs between the fused and the two-node step"


def _landmark_grads(mode, shape, nh, ncls, kind, n, fused, seed=99, ctor_f=(32, 64)):
    from mednet_hip.train import LandmarkStep
    ctor = dict(in_channels=1, out_channels=nh + ncls, final_sigmoid=False, f_maps=list(ctor_f))
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(n, 1, shape, ncls, nh, seed=seed).items()}
    regw = [0.015 + 0.003 * i for i in range(nh)]
    old = ops.FUSE_HEAD_LOSS
    ops.FUSE_HEAD_LOSS = fused
    try:
        with mednet_hip.precision(mode):
            net = O.keyed_init_(HM.ResidualUNet3D(**ctor)).to(DEV)
            step = LandmarkStep(net, class_weight=[0.05, 1.0, 0.7, 1.2][:ncls], regression_weight=regw, regression=kind, lr=1e-3,
                                class_loss="CE")
            scale = step.scaler.snapshot()[0] if step.scaler is not None else 1.0
            tot, cl, rg = step._fwd_bwd(batch)
            torch.cuda.synchronize()
            out = (float(tot), float(cl), float(rg), (step.flat.grad / scale).clone())
            with torch.no_grad():
                took = ops.head_landmark_supported(net.forward_features(batch["data"].float()), ctor_f[0], nh, ncls,
                                                   batch["label"][:, :-1], batch["label"][:, -1])
            step.flat.release()
    finally:
        ops.FUSE_HEAD_LOSS = old
    return out, took


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("shape,nh,ncls,kind,n", [((32, 32, 32), 16, 2, "L2", 2), ((12, 10, 6), 5, 3, "L1", 3),
                                                 ((8, 8, 20), 16, 4, "L2", 1), ((64, 48, 32), 16, 2, "L2", 1),
                                                 ((4, 4, 4), 1, 2, "L2", 2)])
def test_landmark_ce_head_on_the_matrix_cores_against_the_unfused_launches(mode, shape, nh, ncls, kind, n):
    """LandmarkStep(class_loss="CE"): head, heat-map regression and cross-entropy as one matrix-core node against the stock launches
    (1x1x1 head, heat-map and CE kernels, head data / weight gradient): losses to 2e-6 (relative above 1), every gradient to 3e-3
    rel-L2 -- the bounds of the Dice form's test (the matrix-core logits differ from the VALU head's in their last bits)."""
    (t1, c1, r1, g1), took1 = _landmark_grads(mode, shape, nh, ncls, kind, n, True)
    (t0, c0, r0, g0), took0 = _landmark_grads(mode, shape, nh, ncls, kind, n, False)
    assert took1 and not took0
    assert abs(c1 - c0) <= 2e-6 * max(1.0, abs(c0)), (c1, c0)
    assert abs(r1 - r0) <= 2e-6 * max(1.0, abs(r0)), (r1, r0)
    assert torch.isfinite(g1).all()
    e = float((g1 - g0).norm() / g0.norm())
    print(f"[landmark CE head fused vs stock, {mode} {shape} nh={nh} ncls={ncls}] CE {c1:.8f}/{c0:.8f} reg {r1:.5f}/{r0:.5f} grads {e:.2e}")
    assert e <= 3e-3, e


# tol_delta: fraction of parameters whose first-step delta may disagree.  fp32: the caller-fixture test's bound (4 of 3 738); the 16-bit
# modes' gradients carry their storage noise (rel-L2 1.4e-2 bf16, 1.8e-3 fp16 here), and every parameter whose gradient is within it
# of zero can take the other sign (measured: 5.7e-4 fp32, 2.0e-2 bf16, 6.7e-3 fp16 of 8.77 M)
@pytest.mark.parametrize("mode,tol_l,tol_g,tol_delta", [("fp32", 2e-4, 2e-3, 1.1e-3), ("bf16", 2e-2, 5e-2, 3e-2), ("fp16", 1e-2, 3e-2, 1.5e-2)])
def test_landmark_step_ce_against_the_live_oracle(mode, tol_l, tol_g, tol_delta):
    """LandmarkNet(loss_class='CE').training_step + .loss (landmarks.py:43-49, 66-83, 125-134) -- config 4's network (f_maps 32 .. 256,
    16 heat maps + 2 classes) at 32^3 -- through train.LandmarkStep(class_loss="CE") against O.ldmk_training_step with
    torch.nn.CrossEntropyLoss(weight) on the CPU: the three losses, every gradient, and one Adam step's parameter delta."""
    from mednet_hip.train import LandmarkStep
    ctor = dict(in_channels=1, out_channels=18, final_sigmoid=False, f_maps=[32, 64, 128, 256])
    batch = O.synthetic_batch(2, 1, (32, 32, 32), 2, 16, seed=4444)
    regw = [0.015] * 16
    ora = O.keyed_init_(O.ResidualUNet3D(**ctor))
    ora_before = {k: p.detach().clone() for k, p in ora.named_parameters()}
    opt = torch.optim.Adam(ora.parameters(), lr=1e-3)  # (configure_optimizers, landmarks.py:176-177)
    tot_o, cl_o, rg_o = O.ldmk_training_step(ora, nn.CrossEntropyLoss(weight=torch.tensor([0.05, 1.0])), nn.MSELoss(), regw, batch)
    tot_o.backward()
    grads_o = [q.grad.clone() for q in ora.parameters()]
    opt.step()
    with mednet_hip.precision(mode):
        net = O.keyed_init_(HM.ResidualUNet3D(**ctor)).to(DEV)
        before = {k: p.detach().clone() for k, p in net.named_parameters()}
        step = LandmarkStep(net, class_weight=[0.05, 1.0], regression_weight=regw, regression="L2", lr=1e-3, class_loss="CE")
        scale = step.scaler.snapshot()[0] if step.scaler is not None else 1.0
        gb = {k: v.to(DEV) for k, v in batch.items()}
        tot, cl, rg = step(gb)  # forward, backward and the fused Adam update (behind the loss scaler in fp16)
        torch.cuda.synchronize()
        if step.scaler is not None:
            assert step.scaler.skipped_steps() == 0
        grads = [p._mednet_grad / scale for p in step.flat.params]
        worst = max(rel(g, q) for g, q in zip(grads, grads_o))
        bad = total = 0
        for k, p in net.named_parameters():
            want = ora.state_dict()[k] - ora_before[k]
            got = (p.detach() - before[k]).cpu()
            bad += int(((got - want).abs() > 2e-6 + 1e-3 * want.abs()).sum())
            total += want.numel()
        step.flat.release()
    for a, b in ((cl, cl_o), (rg, rg_o), (tot, tot_o)):
        assert abs(float(a) - float(b)) <= tol_l * max(1.0, abs(float(b))), (mode, float(a), float(b))
    assert worst <= tol_g, (mode, worst)
    # the first Adam step moves a parameter by lr * g / (|g| + eps): +-lr wherever |g| >> eps, so an element disagrees only where the
    # gradient is within the mode's noise of zero and takes the other sign
    print(f"[cfg4 CE 32^3 {mode}] losses {float(cl):.6f}/{float(cl_o):.6f} {float(rg):.5f}/{float(rg_o):.5f}; worst grad rel-L2 {worst:.2e}; "
          f"Adam delta: {bad} of {total} elements outside rtol 1e-3")
    assert bad <= tol_delta * total, (mode, bad, total)


@pytest.mark.parametrize("class_loss", ["DICE", "CE"])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_landmark_validation_matches_the_reference_composition(mode, class_loss):
    """train.LandmarkValidation against LandmarkNet.validation_step / validation_epoch_end (landmarks.py:136-174) recomposed on the
    CPU oracle: the reference's keys, values within the mode's tolerance, device tensors; the fused single-pass form (16-bit modes)
    agrees with the unfused form to fp32 summation order."""
    from mednet_hip.train import LandmarkValidation
    ctor = dict(in_channels=1, out_channels=5, final_sigmoid=False, f_maps=[32, 64])
    batches = [O.synthetic_batch(2, 1, (16, 16, 16), 2, 3, seed=700 + i) for i in range(2)]
    regw = [0.015, 0.02, 0.001]
    cw = torch.tensor([0.05, 1.0])
    crit = O.DiceLoss(weight=cw) if class_loss == "DICE" else nn.CrossEntropyLoss(weight=cw)
    ora = O.keyed_init_(O.ResidualUNet3D(**ctor)).eval()
    want = []
    with torch.no_grad():
        for b in batches:
            out = ora(b["data"].float())
            hm, lab = b["label"][:, :-1].float(), b["label"][:, -1].long()
            cl = crit(out[:, 3:], lab)
            rg = sum(regw[c] * F.mse_loss(out[:, c], hm[:, c]) for c in range(3))
            dice = O.dice_metric(out[:, 3:], lab)
            want.append({"val_loss": rg + cl, "val_class_loss": cl, "val_regression_loss": rg, "val_dice0": dice[0], "val_dice1": dice[1]})
    want_end = {k: float(torch.stack([o[k] for o in want]).mean()) for k in want[0]}
    tol = {"fp32": 2e-5, "bf16": 3e-2}[mode]
    res = {}
    old, real = ops.FUSE_HEAD_LOSS, ops.head_landmark_eval
    calls = {True: 0, False: 0}
    try:
        for fused in (True, False):
            ops.FUSE_HEAD_LOSS = fused

            def counted(*a, **k):
                calls[fused] += 1
                return real(*a, **k)
            ops.head_landmark_eval = counted
            with mednet_hip.precision(mode):
                net = O.keyed_init_(HM.ResidualUNet3D(**ctor)).to(DEV)
                net.train()
                val = LandmarkValidation(net, class_weight=[0.05, 1.0], regression_weight=regw, class_loss=class_loss)
                outs = [val.validation_step({k: v.to(DEV) for k, v in b.items()}, i + 1) for i, b in enumerate(batches)]
                end = val.validation_epoch_end(outs)
                assert net.training
            assert list(outs[0].keys()) == ["val_loss", "val_class_loss", "val_regression_loss", "val_dice0", "val_dice1"]
            assert all(v.is_cuda and v.dim() == 0 for o in outs for v in o.values())
            assert sorted(end.keys()) == ["log", "progress_bar", "val_loss"] and end["log"] is end["progress_bar"]
            res[fused] = {k: float(v) for k, v in end["log"].items()}
    finally:
        ops.FUSE_HEAD_LOSS, ops.head_landmark_eval = old, real
    # the single fused pass serves the 16-bit modes (one call per batch); fp32 storage and the knob off take the unfused calls
    assert calls == {True: 2 if mode != "fp32" else 0, False: 0}, calls
    for fused in (True, False):
        for k, v in want_end.items():
            assert abs(res[fused][k] - v) <= tol * max(1.0, abs(v)), (fused, k, res[fused][k], v)
    for k in want_end:
        assert abs(res[True][k] - res[False][k]) <= 1e-5 * max(1.0, abs(res[False][k])), (k, res[True][k], res[False][k])


def test_landmark_ce_step_repeats_bit_for_bit_at_the_timed_shape():
    """LandmarkStep(class_loss="CE") at config 4's timed shape (128^3, N=4, bf16): two runs of two steps from the same initialisation
    give bitwise-identical losses and parameters (fixed-order sums in the fused CE head, as in its Dice twin)."""
    from mednet_hip.train import LandmarkStep
    ctor = dict(in_channels=1, out_channels=18, final_sigmoid=False, f_maps=[32, 64, 128, 256])
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(4, 1, (128, 128, 128), 2, 16, seed=9).items()}
    runs = []
    with mednet_hip.precision("bf16"):
        for _ in range(2):
            net = O.keyed_init_(HM.ResidualUNet3D(**ctor)).to(DEV)
            step = LandmarkStep(net, class_weight=[0.05, 1.0], regression_weight=[0.015] * 16, regression="L2", lr=1e-3, class_loss="CE")
            losses = [tuple(float(v) for v in step(batch)) for _ in range(2)]
            torch.cuda.synchronize()
            runs.append((losses, step.flat.flat.clone()))
            step.flat.release()
            del step, net
    assert runs[0][0] == runs[1][0], runs
    assert torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_landmark_ce_head_honours_ignore_index_and_poisons_bad_labels(mode):
    """ops.head_landmark(class_loss="CE") with an ignore_index that occurs (class 1 of the uint8 labels) against the unfused launches
    (ops.cross_entropy with the same ignore_index): the same loss, ignored voxels contribute no gradient; a label outside [0, ncls)
    that is not ignore_index makes the class loss NaN (class_loss_fwd_kernel<CE>'s rule)."""
    from mednet_hip.unet import loss as HL
    nh, ncls = 3, 2
    net_kw = dict(in_channels=1, out_channels=nh + ncls, final_sigmoid=False, f_maps=[32, 64])
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(2, 1, (16, 16, 16), ncls, nh, seed=55).items()}
    regw = torch.tensor([0.015, 0.02, 0.001], device=DEV)
    cw = torch.tensor([0.05, 1.0], device=DEV)
    res = {}
    with mednet_hip.precision(mode):
        net = O.keyed_init_(HM.ResidualUNet3D(**net_kw)).to(DEV)
        fc = net.final_conv
        feats = net.forward_features(batch["data"].float()).detach()
        hm, lab = batch["label"][:, :-1], batch["label"][:, -1]
        assert ops.head_landmark_supported(feats, 32, nh, ncls, hm, lab)
        for fused in (True, False):
            x = feats.clone().requires_grad_(True)
            fc.weight.grad = fc.bias.grad = None
            if fused:
                cl, rg = ops.head_landmark(x, fc.weight, fc.bias, fc._packed(), hm, lab, cw, regw, "L2", ignore_index=1, class_loss="CE")
            else:
                out = fc(x)
                cl = ops.cross_entropy(out[:, nh:], lab.long(), cw, 1)
                rg = HL.HeatmapRegressionLoss(regw, "L2").to(DEV)(out[:, :nh], hm)
            (cl + rg).backward()
            res[fused] = (float(cl), float(rg), x.grad.float().clone(), fc.weight.grad.clone())
        bad = lab.clone()
        bad[1, 2, 3, 4] = 9
        cl_bad, _ = ops.head_landmark(feats, fc.weight, fc.bias, fc._packed(), hm, bad, cw, regw, "L2", class_loss="CE")
        cl_ign, _ = ops.head_landmark(feats, fc.weight, fc.bias, fc._packed(), hm, bad, cw, regw, "L2", ignore_index=9, class_loss="CE")
    (c1, r1, dx1, dw1), (c0, r0, dx0, dw0) = res[True], res[False]
    assert abs(c1 - c0) <= 2e-6 * max(1.0, abs(c0)), (c1, c0)
    assert abs(r1 - r0) <= 2e-6 * max(1.0, abs(r0)), (r1, r0)
    assert rel(dx1, dx0) <= 1e-2 and rel(dw1, dw0) <= 3e-3, (rel(dx1, dx0), rel(dw1, dw0))
    assert torch.isnan(cl_bad) and torch.isfinite(cl_ign)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("shape,n,nh,ncls,kind", [((12, 10, 6), 3, 5, 3, "L1"), ((24, 20, 21), 2, 16, 2, "L2")])
def test_landmark_cls_entries_with_dice_equal_the_plain_entries_bit_for_bit(mode, shape, n, nh, ncls, kind):
    """mednet_head_landmark_cls_fwd / _cls_bwd with MEDNET_CLASS_DICE and no metric against mednet_head_landmark_fwd / _bwd on the same
    inputs, through the C ABI: both losses, `saved`, dz, the GroupNorm partial rows, dW and db bit for bit, with and without gn_y.
    (12, 10, 6): one workgroup per sample with a ragged last run; (24, 20, 21): two workgroups, the second short."""
    from mednet_hip import _lib as L
    lib, dt = L.lib(), {"bf16": torch.bfloat16, "fp16": torch.float16}[mode]
    tag, sp, m = f"lmcls{shape}{nh}", int(np.prod(shape)), nh + ncls
    z = ops.to_cl(rnd(tag + "z", n, 32, *shape).to(DEV).to(dt))
    gy = ops.to_cl(rnd(tag + "y", n, 32, *shape).to(DEV).to(dt))
    w, b = rnd(tag + "w", m, 32, 1, 1, 1, scale=0.3).to(DEV), rnd(tag + "b", m).to(DEV)
    with mednet_hip.precision(mode):
        pk = ops.pack_conv_weight(w, 1, False)
    g = np.random.Generator(np.random.PCG64(81))
    hm = torch.from_numpy(g.integers(0, 256, size=(n, nh) + shape).astype(np.uint8)).to(DEV)
    lab = torch.from_numpy(g.integers(0, ncls, size=(n,) + shape).astype(np.uint8)).to(DEV)
    cw = torch.tensor([0.05, 1.0, 0.7][:ncls], device=DEV)
    rw = torch.tensor([0.015 + 0.003 * i for i in range(nh)], device=DEV)
    dc, dr = torch.tensor(3.0, device=DEV), torch.tensor(1.5, device=DEV)
    rk, code = (L.REG_L2 if kind == "L2" else L.REG_L1), L.dt_of(dt)
    assert lib.mednet_head_landmark_supported(32, nh, ncls, code, sp) == 1
    ws = L.workspace(lib.mednet_head_landmark_ws_bytes(n, sp, nh, ncls), z.device)
    rows = lib.mednet_head_landmark_gn_rows(sp)
    front = (z.data_ptr(), pk.data_ptr(), b.data_ptr(), hm.data_ptr(), nh * sp, lab.data_ptr(), sp, cw.data_ptr(), rw.data_ptr())
    tail = (1e-5, 0, L.NO_IGNORE, code, ws.data_ptr(), ws.numel(), L.stream())
    out = {}
    for cls in (False, True):
        closs, rloss = (torch.full((), float("nan"), device=DEV) for _ in range(2))
        saved = torch.full((ncls, 2), float("nan"), device=DEV)
        if cls:
            L.check(lib.mednet_head_landmark_cls_fwd(*front, None, closs.data_ptr(), rloss.data_ptr(), saved.data_ptr(), None, n, sp, 32, nh,
                                                     ncls, rk, L.CLASS_DICE, *tail), "head_landmark_cls_fwd")
        else:
            L.check(lib.mednet_head_landmark_fwd(*front, None, closs.data_ptr(), rloss.data_ptr(), saved.data_ptr(), n, sp, 32, nh, ncls, rk,
                                                 *tail), "head_landmark_fwd")
        res = [closs, rloss, saved]
        for with_gy in (True, False):
            dz = torch.full_like(z, float("nan"))
            part = torch.full((n, rows, 32, 2), float("nan"), device=DEV) if with_gy else None
            dw, db = torch.full((m, 32), float("nan"), device=DEV), torch.full((m,), float("nan"), device=DEV)
            mid = (saved.data_ptr(), dc.data_ptr(), dr.data_ptr(), dz.data_ptr(), gy.data_ptr() if with_gy else None, L.ACT_ELU,
                   L.ptr(part), dw.data_ptr(), db.data_ptr(), n, sp, 32, nh, ncls, rk)
            if cls:
                L.check(lib.mednet_head_landmark_cls_bwd(*front, *mid, L.CLASS_DICE, *tail), "head_landmark_cls_bwd")
            else:
                L.check(lib.mednet_head_landmark_bwd(*front, *mid, *tail), "head_landmark_bwd")
            res += [dz, dw, db] + ([part] if with_gy else [])
        torch.cuda.synchronize()
        out[cls] = res
    names = ["class loss", "regression loss", "saved", "dz", "dW", "db", "GroupNorm rows", "dz (no gn_y)", "dW (no gn_y)", "db (no gn_y)"]
    for name, a, c in zip(names, out[False], out[True]):
        assert torch.isfinite(a.float()).all() and torch.equal(a, c), f"{name}: the _cls_ entry differs from the plain entry"


def test_ce_caller_fixtures_meet_the_hip_path(golden_dir):
    """tests/golden/callers_ce.npz -- the reference's own callers (tools/make_golden.py) -- through the HIP path: SegmentationStep /
    SegmentationValidation with loss="CE", LandmarkStep(class_loss="CE") with L2 and L1, LandmarkValidation with DICE and CE.  The
    tolerances of test_reference_caller_fixtures_meet_the_hip_path in the fp32 mode (where the segmentation head is the fused CE
    node), and the bf16 mode's for the landmark callers, whose fused head serves the 16-bit modes."""
    import os
    from mednet_hip.train import LandmarkStep, LandmarkValidation, SegmentationStep, SegmentationValidation
    from test_callers_ce_golden import CE_LDMK, CE_SEG
    rec = np.load(os.path.join(golden_dir, "callers_ce.npz"))
    cin, cout, fm = CE_SEG["ctor"]
    taken = {"seg": 0, "ldmk": 0, "val": 0}
    real_ce, real_lm, real_eval = ops.HeadCEFn.apply, ops.HeadLandmarkFn.apply, ops.head_landmark_eval

    def count(key, fn):
        def wrapped(*a, **k):
            taken[key] += 1
            return fn(*a, **k)
        return wrapped
    ops.HeadCEFn.apply, ops.HeadLandmarkFn.apply = count("seg", real_ce), count("ldmk", real_lm)
    ops.head_landmark_eval = count("val", real_eval)
    try:
        with mednet_hip.precision("fp32"):
            net = O.keyed_init_(HM.ResidualUNet3D(cin, cout, False, f_maps=fm)).to(DEV)
            step = SegmentationStep(net, loss_weight=CE_SEG["weight"], lr=1e-3, loss="CE")
            batch = {k: v.to(DEV) for k, v in O.synthetic_batch(2, 1, CE_SEG["shape"], cout, 0, seed=CE_SEG["seed"]).items()}
            loss = step(batch)
            assert abs(float(loss) - float(rec["seg.loss"])) <= 1e-4, (float(loss), float(rec["seg.loss"]))
            step.flat.release()
            net = O.keyed_init_(HM.ResidualUNet3D(cin, cout, False, f_maps=fm)).to(DEV)
            val = SegmentationValidation(net, loss_weight=CE_SEG["weight"], loss="CE")
            outs = [val.validation_step({k: v.to(DEV) for k, v in O.synthetic_batch(2, 1, CE_SEG["shape"], cout, 0, seed=s).items()}, 1 + i)
                    for i, s in enumerate(CE_SEG["val_seeds"])]
            end = val.validation_epoch_end(outs)
            for i, o in enumerate(outs):
                for k, v in o.items():
                    assert abs(float(v) - float(rec[f"seg.val{i}.{k}"])) <= 2e-5 * max(1.0, abs(float(v))), (i, k)
            for k, v in end["log"].items():
                assert abs(float(v) - float(rec["seg.val_end." + k])) <= 2e-5 * max(1.0, abs(float(v))), k
        assert taken["seg"] == 1
        cin, cout, fm = CE_LDMK["ctor"]
        regw = CE_LDMK["regw"]
        nh = len(regw)
        batch = {k: v.to(DEV) for k, v in O.synthetic_batch(2, 1, CE_LDMK["shape"], cout - nh, nh, seed=CE_LDMK["seed"]).items()}
        vbs = [{k: v.to(DEV) for k, v in O.synthetic_batch(2, 1, CE_LDMK["shape"], cout - nh, nh, seed=s).items()} for s in CE_LDMK["val_seeds"]]
        for mode, rtol in (("fp32", 1e-4), ("bf16", 3e-2)):
            with mednet_hip.precision(mode):
                for kind in ("L2", "L1"):
                    net = O.keyed_init_(HM.ResidualUNet3D(cin, cout, False, f_maps=fm)).to(DEV)
                    step = LandmarkStep(net, class_weight=CE_LDMK["weight"], regression_weight=regw, regression=kind, lr=1e-3, class_loss="CE")
                    for name, v in zip(("loss", "class_loss", "regression_loss"), step(batch)):
                        want = float(rec[f"ldmk.{kind}.{name}"])
                        assert abs(float(v) - want) <= rtol * max(1e-2, abs(want)), (mode, kind, name, float(v), want)
                    step.flat.release()
                for lc in ("DICE", "CE"):
                    net = O.keyed_init_(HM.ResidualUNet3D(cin, cout, False, f_maps=fm)).to(DEV)
                    val = LandmarkValidation(net, class_weight=CE_LDMK["weight"], regression_weight=regw, class_loss=lc)
                    outs = [val.validation_step(b, 1 + i) for i, b in enumerate(vbs)]
                    end = val.validation_epoch_end(outs)
                    for i, o in enumerate(outs):
                        assert list(o.keys()) == ["val_loss", "val_class_loss", "val_regression_loss", "val_dice0", "val_dice1"]
                        for k, v in o.items():
                            want = float(rec[f"ldmk_val.{lc}.{i}.{k}"])
                            assert abs(float(v) - want) <= rtol * max(1e-2, abs(want)), (mode, lc, i, k, float(v), want)
                    for k, v in end["log"].items():
                        want = float(rec[f"ldmk_val_end.{lc}.{k}"])
                        assert abs(float(v) - want) <= rtol * max(1e-2, abs(want)), (mode, lc, k, float(v), want)
    finally:
        ops.HeadCEFn.apply, ops.HeadLandmarkFn.apply, ops.head_landmark_eval = real_ce, real_lm, real_eval
    # the fused landmark node serves the bf16 runs: two training steps, and one validation pass per batch and class loss
    assert taken["ldmk"] == 2 and taken["val"] == 4, taken
