"""The matrix-core segmentation head for 5 .. 16 classes (head_mfma.hip: head_seg_kernel; ops.head_seg; the wide branch of
train.SegmentationStep._head_loss) on the MI355X (-m gpu): against the unfused launches and ATen, exact logits on lattice inputs,
out-of-range labels, the training step against the two-node step and the live CPU oracle, the dispatch rules, graph capture."""
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
from mednet_hip.unet import model as HM
from oracle import ref_cpu as O

from gpu_util import DEV, DT, TOL, assert_exact, assert_representable, assert_sums_exact, half_round, lattice, rel, report, rnd

pytestmark = pytest.mark.gpu
MODES = ["bf16", "fp16"]
# (n, shape): half a run; two runs and two idle waves; a ragged last run; two workgroups per sample
SHAPES = [(2, (4, 4, 4)), (1, (4, 6, 10)), (3, (12, 10, 6)), (2, (16, 16, 36))]
# (class loss, weighted, sigmoid, ignore_index)
VARIANTS = [("DICE", False, False, None), ("DICE", True, False, None), ("DICE", True, False, 2), ("DICE", False, True, None),
            ("CE", True, False, -100), ("CE", False, False, -100), ("CE", True, False, 3)]


def _weights(c):
    return torch.tensor([0.05] + [0.6 + 0.1 * (k % 7) for k in range(1, c)])


def _reference(kind, lr, lab, wt, sigmoid, ignore):
    if kind == "DICE":
        return O.DiceLoss(weight=wt, sigmoid_normalization=sigmoid, ignore_index=ignore)(lr, lab)
    return F.cross_entropy(lr, lab, weight=wt, ignore_index=ignore)


def _head_pair(mode, x, w, b, lab_u8, kind, wt, sigmoid, ignore, gscale):
    """-> {fused: (loss, dx, dW, db)} of ops.head_seg and of final_conv + ops.dice_loss / ops.cross_entropy on the same tensors."""
    c = w.shape[0]
    res = {}
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
                lg, loss = ops.head_seg(xg, conv.weight, conv.bias, conv._packed(), lab_u8, wd, 1e-5, sigmoid, ignore, kind)
                assert lg is None
            else:
                lg = conv(xg)
                loss = (ops.dice_loss(lg, lab_u8.long(), wd, 1e-5, sigmoid, ignore) if kind == "DICE"
                        else ops.cross_entropy(lg, lab_u8.long(), wd, ignore))
            (loss * gscale).backward()
            res[fused] = (loss.detach(), xg.grad, conv.weight.grad, conv.bias.grad)
    return res


def _compare(mode, tag, res, ref, gscale):
    """The bounds of the landmark form's comparison: loss 2e-6 (relative above 1) and gradients 3e-3 rel-L2 against the unfused
    launches; everything within the mode's tolerance (gradients max(tol, 1e-4)) of ATen on the CPU."""
    (s0, dx0, dw0, db0), (s1, dx1, dw1, db1) = res[False], res[True]
    loss_r, dxr, dwr, dbr = ref
    tol = TOL[mode]
    vals = dict(loss=abs(float(s1) - float(s0)), dx=rel(dx1, dx0), dW=rel(dw1, dw0), db=rel(db1, db0),
                loss_aten=abs(float(s1) - float(loss_r)), dx_aten=rel(dx1.float() / gscale, dxr), dW_aten=rel(dw1 / gscale, dwr),
                db_aten=rel(db1 / gscale, dbr))
    print(f"[seg head {tag}] " + " ".join(f"{k} {v:.2e}" for k, v in vals.items()))
    assert torch.isfinite(s1) and torch.isfinite(dx1).all() and torch.isfinite(dw1).all() and torch.isfinite(db1).all(), tag
    assert vals["loss"] <= 2e-6 * max(1.0, abs(float(s0))), (tag, float(s1), float(s0))
    for k in ("dx", "dW", "db"):
        assert vals[k] <= 3e-3, (tag, k, vals[k])
    assert vals["loss_aten"] <= tol * max(1.0, abs(float(loss_r))), (tag, float(s1), float(loss_r))
    for k in ("dx_aten", "dW_aten", "db_aten"):
        assert vals[k] <= max(tol, 1e-4), (tag, k, vals[k])


def _inputs(mode, c, n, shape, classes=None):
    tag = f"sg{c}{n}{shape}"
    x = half_round(rnd(tag + "x", n, 32, *shape), mode)
    w, b = rnd(tag + "w", c, 32, 1, 1, 1, scale=0.3), rnd(tag + "b", c)
    g = np.random.Generator(np.random.PCG64(79 + c))
    pool = np.arange(c) if classes is None else np.asarray(classes)
    lab_vol = torch.from_numpy(pool[g.integers(0, len(pool), size=(n, 2) + shape)].astype(np.uint8))
    return x, w, b, lab_vol


def _run_variants(mode, c, n, shape, variants, lab_vol=None, classes=None, tag=""):
    x, w, b, lv = _inputs(mode, c, n, shape, classes)
    lab_vol = lv if lab_vol is None else lab_vol
    gscale = 3.0 * 16384.0 if mode == "fp16" else 3.0  # (fp16 stores the feature gradient: scaled as train.LossScaler does)
    lab_dev = lab_vol.to(DEV)[:, -1]  # the last channel of a uint8 volume, where it lies
    for kind, weighted, sigmoid, ignore in variants:
        wt = _weights(c) if weighted else None
        xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        loss_r = _reference(kind, F.conv3d(xr, wr, br), lab_vol[:, -1].long(), wt, sigmoid, ignore)
        loss_r.backward()
        res = _head_pair(mode, x, w, b, lab_dev, kind, wt, sigmoid, ignore, gscale)
        _compare(mode, f"{tag}{mode} C={c} n={n} {shape} {kind} w={int(weighted)} sig={int(sigmoid)} ign={ignore}", res,
                 (loss_r.detach(), xr.grad, wr.grad, br.grad), gscale)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", [5, 8, 9, 14, 16])
@pytest.mark.parametrize("n,shape", SHAPES)
def test_seg_head_on_the_matrix_cores_against_the_unfused_launches(mode, c, n, shape):
    """ops.head_seg (mednet_head_seg_fwd / _bwd) against hnn.Conv3d(32, C, 1, planar_output=True) + ops.dice_loss / ops.cross_entropy
    and against ATen on the CPU from the same rounded features, every variant of both losses."""
    _run_variants(mode, c, n, shape, VARIANTS)


@pytest.mark.parametrize("mode", MODES)
def test_seg_head_with_labels_from_three_of_the_classes(mode):
    """Eleven of the fourteen classes never occur: their Dice terms have I = 0 and D = sum p only."""
    _run_variants(mode, 14, 3, (12, 10, 6), [VARIANTS[1], VARIANTS[4]], classes=(0, 6, 13), tag="three classes ")


@pytest.mark.parametrize("mode", MODES)
def test_seg_head_label_volume_at_an_odd_byte_offset(mode):
    """A label view whose base address is odd is copied once on the Python side (the kernel reads four labels at a time): the same
    numbers as from the aligned volume, bit for bit."""
    c, n, shape = 9, 3, (12, 10, 6)
    x, w, b, lab_vol = _inputs(mode, c, n, shape)
    lab = lab_vol[:, -1].contiguous()
    buf = torch.zeros(lab.numel() + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = lab.flatten().to(DEV)
    odd = buf[1:].view(n, *shape)
    assert odd.data_ptr() % 2 == 1
    out = {}
    with mednet_hip.precision(mode):
        conv = hnn.Conv3d(32, c, 1, planar_output=True).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(b)
        for key, lv in (("odd", odd), ("even", lab.to(DEV))):
            for kind in ("DICE", "CE"):
                xg = ops.to_cl(x.to(DEV).to(mednet_hip.config.act_dtype())).requires_grad_(True)
                conv.weight.grad = conv.bias.grad = None
                assert ops.head_seg_supported(xg, 32, c, lv)
                _, loss = ops.head_seg(xg, conv.weight, conv.bias, conv._packed(), lv, None, class_loss=kind)
                (loss * 1024.0).backward()
                out[key, kind] = (loss.detach().clone(), xg.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone())
    for kind in ("DICE", "CE"):
        for a, b_ in zip(out["odd", kind], out["even", kind]):
            assert torch.isfinite(a).all() and torch.equal(a, b_), kind


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", [5, 9, 16])
def test_seg_head_logits_are_exact_on_lattice_inputs(mode, c):
    """Lattice features and weights (numbers of the storage type: the low half of the weight split is zero), integer bias: the logits
    the forward writes on request equal ATen's fp64 conv3d in every element."""
    n, shape = 3, (12, 10, 6)
    x = lattice(f"sgx{c}", n, 32, *shape)
    w = lattice(f"sgw{c}", c, 32, 1, 1, 1, density=0.5, scale=0.5)
    b = lattice(f"sgb{c}", c, values=(-3, -1, 2, 5), density=0.8)
    assert_representable(x, DT[mode], "features")
    assert_representable(w, DT[mode], "weights")
    ref = F.conv3d(x.double(), w.double(), b.double())
    assert_representable(ref, torch.float32, "logits")
    assert_sums_exact(F.conv3d(x.double().abs(), w.double().abs(), b.double().abs()), "logits", unit=0.5)
    lab = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).integers(0, c, size=(n,) + shape).astype(np.uint8)).to(DEV)
    with mednet_hip.precision(mode):
        conv = hnn.Conv3d(32, c, 1, planar_output=True).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(b)
        xg = ops.to_cl(x.to(DEV).to(mednet_hip.config.act_dtype()))
        for kind in ("DICE", "CE"):
            lg, loss = ops.head_seg(xg, conv.weight, conv.bias, conv._packed(), lab, None, class_loss=kind, want_logits=True)
            assert tuple(lg.shape) == (n, c) + shape and lg.dtype == torch.float32 and lg.is_contiguous()
            report("seg_head", f"logits {mode} C={c} {kind}", "head_seg_kernel<false>", assert_exact(lg, ref, f"logits {kind}"))
            assert torch.isfinite(loss)


@pytest.mark.parametrize("kind", ["DICE", "CE"])
def test_seg_head_out_of_range_label_poisons_the_loss(kind):
    """A uint8 label of 200 with 14 classes: NaN loss (class_loss_fwd_kernel<DICE>'s / class_loss_fwd_kernel<CE>'s rule), nothing indexed out of range, the
    backward still runs and fills gradients of the right shapes."""
    with mednet_hip.precision("bf16"):
        conv = hnn.Conv3d(32, 14, 1, planar_output=True).to(DEV)
        x = ops.to_cl(rnd("sg-bad", 2, 32, 8, 8, 8).to(DEV).bfloat16()).requires_grad_(True)
        lab = torch.zeros((2, 8, 8, 8), dtype=torch.uint8, device=DEV)
        lab[1, 3, 4, 5] = 200
        _, loss = ops.head_seg(x, conv.weight, conv.bias, conv._packed(), lab, None, class_loss=kind)
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isnan(loss)
        assert tuple(conv.weight.grad.shape) == (14, 32, 1, 1, 1) and tuple(conv.bias.grad.shape) == (14,) and x.grad.shape == x.shape
        lab[1, 3, 4, 5] = 13
        _, loss = ops.head_seg(x, conv.weight, conv.bias, conv._packed(), lab, None, class_loss=kind)
        assert torch.isfinite(loss)


# ---------------------------------------------------------------------------------------------- the training step
CTOR14 = dict(in_channels=1, out_channels=14, final_sigmoid=False, f_maps=[32, 64])
W14 = [0.05] + [1.0] * 13


def _count_calls(fn_cls):
    calls = {"n": 0}
    real = fn_cls.apply

    def counted(*a):
        calls["n"] += 1
        return real(*a)
    fn_cls.apply = counted
    return calls, real


def _step_grads(mode, kind, fused, batch, ctor=CTOR14, weight=W14, make=HM.ResidualUNet3D):
    from mednet_hip.train import SegmentationStep
    old = ops.FUSE_HEAD_LOSS
    ops.FUSE_HEAD_LOSS = fused
    calls, real = _count_calls(ops.HeadSegFn)
    try:
        with mednet_hip.precision(mode):
            net = O.keyed_init_(make(**ctor)).to(DEV)
            step = SegmentationStep(net, loss_weight=weight, lr=1e-3, loss=kind)
            scale = step.scaler.snapshot()[0] if step.scaler is not None else 1.0
            (loss,) = step._fwd_bwd(batch)
            torch.cuda.synchronize()
            step.flat.grads_as_attr()
            grads = [(p.grad / scale).clone() for p in net.parameters()]
            flat = (step.flat.grad / scale).clone()
            step.flat.release()
    finally:
        ops.HeadSegFn.apply = real
        ops.FUSE_HEAD_LOSS = old
    return float(loss), flat, grads, calls["n"]


@functools.lru_cache(maxsize=None)
def _oracle14(kind):
    batch = O.synthetic_batch(2, 1, (24, 40, 32), 14, 0, seed=61)
    ora = O.keyed_init_(O.ResidualUNet3D(**CTOR14))
    crit = O.DiceLoss(weight=torch.tensor(W14)) if kind == "DICE" else nn.CrossEntropyLoss(weight=torch.tensor(W14))
    loss = crit(ora(batch["data"]), batch["label"][:, -1].long())
    loss.backward()
    return float(loss.detach()), [q.grad.clone() for q in ora.parameters()]


@pytest.mark.parametrize("mode,tol_l,tol_g", [("bf16", 2e-2, 5e-2), ("fp16", 1e-2, 3e-2)])
@pytest.mark.parametrize("kind", ["DICE", "CE"])
def test_segmentation_step_with_14_classes_takes_the_wide_node(mode, tol_l, tol_g, kind):
    """train.SegmentationStep on ResidualUNet3D(1, 14, f_maps [32, 64]): head + loss as the one matrix-core node (ops.HeadSegFn, called
    exactly once) against the same step with ops.FUSE_HEAD_LOSS off -- loss to 2e-6, the flat gradient to 3e-3 rel-L2 --, and against
    the live CPU oracle (O.ResidualUNet3D + O.DiceLoss / nn.CrossEntropyLoss) with the tolerances of the landmark step's oracle test."""
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(2, 1, (24, 40, 32), 14, 0, seed=61).items()}
    l1, f1, g1, n1 = _step_grads(mode, kind, True, batch)
    l0, f0, _, n0 = _step_grads(mode, kind, False, batch)
    assert n1 == 1 and n0 == 0, (n1, n0)
    e = float((f1 - f0).norm() / f0.norm())
    lo, go = _oracle14(kind)
    worst = max(rel(g, q) for g, q in zip(g1, go))
    print(f"[seg step 14 classes {mode} {kind}] loss {l1:.8f} / two-node {l0:.8f} / oracle {lo:.8f}; flat grad vs two-node {e:.2e}; "
          f"worst grad vs oracle {worst:.2e}")
    assert torch.isfinite(f1).all()
    assert abs(l1 - l0) <= 2e-6 * max(1.0, abs(l0)), (l1, l0)
    assert e <= 3e-3, e
    assert abs(l1 - lo) <= tol_l * max(1.0, abs(lo)), (l1, lo)
    assert worst <= tol_g, worst


def _dispatch_loss(mode, ctor, shape, make=HM.ResidualUNet3D, hook=False, kind="DICE"):
    from mednet_hip.train import SegmentationStep
    c = ctor["out_channels"]
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(2, 1, shape, c, 0, seed=17).items()}
    seg, real_seg = _count_calls(ops.HeadSegFn)
    dice, real_dice = _count_calls(ops.HeadDiceFn)
    try:
        with mednet_hip.precision(mode):
            net = O.keyed_init_(make(**ctor)).to(DEV)
            handle = net.final_conv.register_forward_hook(lambda m, i, o: None) if hook else None
            step = SegmentationStep(net, loss_weight=[0.05] + [1.0] * (c - 1), lr=1e-3, loss=kind)
            (loss,) = step._fwd_bwd(batch)
            torch.cuda.synchronize()
            finite = bool(torch.isfinite(loss)) and bool(torch.isfinite(step.flat.grad).all())
            step.flat.release()
            if handle is not None:
                handle.remove()
    finally:
        ops.HeadSegFn.apply, ops.HeadDiceFn.apply = real_seg, real_dice
    return finite, seg["n"], dice["n"]


@pytest.mark.parametrize("case", ["control", "fp16x2", "4 classes", "17 classes", "64 features", "fp32", "UNet3D", "hooked", "option off"])
def test_the_wide_node_is_taken_only_where_it_applies(case):
    """Everything but 5 .. 16 classes on a 32-feature ResidualUNet3D head in a 16-bit mode (bf16, fp16, fp16x2) keeps its path, with a
    finite loss."""
    shape = (16, 16, 16)
    kw = dict(mode="bf16", ctor=dict(CTOR14), shape=shape)
    if case == "4 classes":
        kw["ctor"]["out_channels"] = 4
    elif case == "17 classes":
        kw["ctor"]["out_channels"] = 17
    elif case == "64 features":
        kw["ctor"]["f_maps"] = [64, 128]
    elif case in ("fp32", "fp16x2"):
        kw["mode"] = case
    elif case == "UNet3D":
        kw["make"] = HM.UNet3D
    elif case == "hooked":
        kw["hook"] = True
    lib = L.lib()
    try:
        if case == "option off":
            assert lib.mednet_set_option(b"head_seg_mfma", 0) == 0
        finite, nseg, ndice = _dispatch_loss(**kw)
    finally:
        lib.mednet_set_option(b"head_seg_mfma", 1)
    assert finite
    assert nseg == (1 if case in ("control", "fp16x2") else 0), (case, nseg)
    assert ndice == (1 if case == "4 classes" else 0), (case, ndice)


def test_a_volume_whose_size_is_no_multiple_of_4_keeps_the_two_node_path():
    """spatial % 4 != 0 (3 x 3 x 3): ops.head_seg_supported refuses, final_conv + ops.dice_loss give a finite loss."""
    with mednet_hip.precision("bf16"):
        conv = hnn.Conv3d(32, 14, 1, planar_output=True).to(DEV)
        x = ops.to_cl(rnd("sg-333", 2, 32, 3, 3, 3).to(DEV).bfloat16()).requires_grad_(True)
        lab = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).integers(0, 14, size=(2, 3, 3, 3)).astype(np.uint8)).to(DEV)
        assert not ops.head_seg_supported(x, 32, 14, lab)
        assert ops.head_seg_supported(ops.to_cl(rnd("sg-334", 2, 32, 3, 3, 4).to(DEV).bfloat16()), 32, 14, lab)  # (3 x 3 x 4 is taken)
        loss = ops.dice_loss(conv(x), lab.long(), None, 1e-5, False, None)
        loss.backward()
        assert torch.isfinite(loss) and torch.isfinite(x.grad).all()


def _train14(graph, batches):
    from mednet_hip.train import SegmentationStep
    calls, real = _count_calls(ops.HeadSegFn)
    try:
        with mednet_hip.precision("bf16"):
            net = O.keyed_init_(HM.ResidualUNet3D(**CTOR14)).to(DEV)
            step = SegmentationStep(net, loss_weight=W14, lr=1e-3, graph=graph)
            losses = [float(step({k: v.to(DEV) for k, v in b.items()})) for b in batches]
            torch.cuda.synchronize()
            flat = step.flat.flat.clone()
            step.flat.release()
    finally:
        ops.HeadSegFn.apply = real
    return losses, flat, calls["n"]


def test_14_class_training_steps_graph_equals_eager_and_repeat():
    """Three SegmentationSteps at 14 classes (bf16): the captured graph against the eager step and two eager runs against each other,
    losses and parameters bit-identical (every sum of the wide node is made in a fixed order; nothing in it synchronises)."""
    batches = [O.synthetic_batch(2, 1, (16, 16, 16), 14, 0, seed=500 + i) for i in range(3)]
    e1, e2, gr = _train14(False, batches), _train14(False, batches), _train14(True, batches)
    assert e1[2] == 3 and gr[2] >= 1, (e1[2], gr[2])
    assert all(np.isfinite(e1[0]))
    assert e1[0] == e2[0] and torch.equal(e1[1], e2[1]), "two eager runs differ"
    assert gr[0] == e1[0] and torch.equal(gr[1], e1[1]), (gr[0], e1[0])
