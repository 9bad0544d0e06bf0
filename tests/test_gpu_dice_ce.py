"""Dice + cross-entropy, the compound class loss, on the MI355X (-m gpu): the one-pass kernel pair of loss.hip (ops.dice_ce_loss) and
the fused head for up to 4 classes (ops.head_dice_ce) against the launches they replace, BIT FOR BIT; the reference pin
tests/golden/dice_ce.npz; out-of-range labels; and both operator families inside guard bands (tests/fence.py)."""
import os

import numpy as np
import pytest
import torch

import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import nn as hnn
from mednet_hip import ops
from mednet_hip.unet import components as HC
from mednet_hip.unet import loss as HL
from mednet_hip.unet import model as HM
from oracle import ref_cpu as O

from fence import Fence
from gpu_util import DEV, assert_close, rnd

pytestmark = pytest.mark.gpu
GSCALE = 3.0  # the gradient scale of every comparison (a power of two would hide a dropped factor)


def _weights(c):
    return torch.tensor([0.05] + [0.6 + 0.1 * (k % 7) for k in range(1, c)])


@pytest.fixture(scope="module")
def volumes():
    """Logits (wide enough for every class count, as a channel slice of it) and a uint8 label volume per shape, made once."""
    out = {}
    for key, n, shape in (("ragged", 2, (13, 13, 13)), ("trips", 3, (65, 64, 63))):
        width = 34 if key == "ragged" else 7
        g = np.random.Generator(np.random.PCG64(17 + n))
        out[key] = (n, shape, (rnd("dce" + key, n, width, *shape, scale=2.0)).to(DEV),
                    torch.from_numpy(g.integers(0, 256, size=(n, 2) + shape).astype(np.uint8)).to(DEV))
    return out


def _labels(vol, c, form):
    """u8: the last channel of a uint8 volume, where it lies (a sample stride of two channels); i64s: every second sample of a
    twice-as-long int64 tensor (a sample stride); i64: contiguous."""
    lab = (vol[:, -1] % c)
    if form == "u8":
        v = vol.clone()
        v[:, -1] = lab
        assert not v[:, -1].is_contiguous()
        return v[:, -1]
    if form == "i64s":
        wide = torch.zeros((2 * lab.shape[0],) + tuple(lab.shape[1:]), dtype=torch.int64, device=DEV)
        wide[::2] = lab.long()
        return wide[::2]
    return lab.long()


def _pair(logits, lab, wt):
    """-> ((loss, grad) of ops.dice_ce_loss, (loss, grad) of ops.dice_loss + ops.cross_entropy) on the same tensors."""
    res = []
    for fused in (True, False):
        z = logits.detach().clone().requires_grad_(True)
        if fused:
            loss = ops.dice_ce_loss(z, lab, wt, 1e-5)
        else:
            loss = ops.dice_loss(z, lab, wt, 1e-5, False, None) + ops.cross_entropy(z, lab.long(), wt)
        (loss * GSCALE).backward()
        res.append((loss.detach(), z.grad))
    return res


CASES = [("ragged", c, form, weighted, sliced) for c in (1, 2, 4, 5, 16, 32) for form, weighted, sliced in
         (("u8", True, False), ("i64s", False, True), ("i64", True, True))]
CASES += [("trips", 4, "u8", True, False), ("trips", 5, "i64s", False, True)]


@pytest.mark.parametrize("key,c,form,weighted,sliced", CASES)
def test_one_pass_loss_equals_the_two_kernel_composition_bit_for_bit(volumes, key, c, form, weighted, sliced):
    """ops.dice_ce_loss against ops.dice_loss + ops.cross_entropy: the loss and every element of the logit gradient are equal (the
    one fp32 add autograd makes of the two gradients is the kernel's).  13^3 = 2 197 voxels: a second workgroup with a ragged last
    block; n = 3, 65 x 64 x 63: 128 workgroups per sample, 384 partial rows, the finalize loop's second trip.  `sliced`: the logits
    are a channel slice of a wider tensor (the landmark layout), so sample and channel strides differ from the dense ones."""
    n, shape, wide, vol = volumes[key]
    lab = _labels(vol, c, form)
    wt = _weights(c).to(DEV) if weighted else None
    if sliced:
        res = []
        for fused in (True, False):
            z = wide.detach().clone().requires_grad_(True)
            view = z[:, wide.shape[1] - c:]
            loss = (ops.dice_ce_loss(view, lab, wt) if fused
                    else ops.dice_loss(view, lab, wt, 1e-5, False, None) + ops.cross_entropy(view, lab.long(), wt))
            (loss * GSCALE).backward()
            res.append((loss.detach(), z.grad))
        (l1, g1), (l0, g0) = res
        assert not g1[:, :wide.shape[1] - c].any(), "the gradient of the channels in front of the slice is not zero"
    else:
        (l1, g1), (l0, g0) = _pair(wide[:, :c].contiguous(), lab, wt)
    assert torch.isfinite(l1) and torch.isfinite(g1).all()
    assert torch.equal(l1, l0), (float(l1), float(l0))
    assert torch.equal(g1, g0), f"{int((g1 != g0).sum())} of {g1.numel()} gradient elements differ, max {float((g1 - g0).abs().max()):.3e}"


def test_loss_is_the_rounded_sum_of_the_two_terms_and_saved_holds_both(volumes):
    """Through the C ABI: saved = [c][2] {I, D} of mednet_dice_fwd_lt followed by sum w_y of mednet_ce_fwd, dice_out the per-channel
    dice, loss = fl(dice + ce); the workspace is exactly mednet_dice_ce_ws_bytes, filled with NaN."""
    n, shape, wide, vol = volumes["ragged"]
    c, sp = 5, int(np.prod(shape))
    z = wide[:, :c].contiguous()
    lab = _labels(vol, c, "i64")
    wt = _weights(c).to(DEV)
    lib = L.lib()
    ws = torch.full((lib.mednet_dice_ce_ws_bytes(n, c, sp),), 255, dtype=torch.uint8, device=DEV)
    loss, saved, dice = (torch.full(s, float("nan"), device=DEV) for s in ((), (2 * c + 1,), (c,)))
    L.check(lib.mednet_dice_ce_fwd_lt(z.data_ptr(), lab.data_ptr(), L.I64, sp, wt.data_ptr(), loss.data_ptr(), saved.data_ptr(),
                                      dice.data_ptr(), n, c, sp, c * sp, sp, 1e-5, ws.data_ptr(), ws.numel(), L.stream()), "dice_ce_fwd")
    ws2 = torch.full((lib.mednet_loss_ws_bytes(n, c, sp),), 255, dtype=torch.uint8, device=DEV)
    ld, sd, dd, lc, sc = (torch.full(s, float("nan"), device=DEV) for s in ((), (c, 2), (c,), (), (2,)))
    L.check(lib.mednet_dice_fwd_lt(z.data_ptr(), lab.data_ptr(), L.I64, sp, wt.data_ptr(), ld.data_ptr(), sd.data_ptr(), dd.data_ptr(), n,
                                   c, sp, c * sp, sp, 1e-5, 0, L.NO_IGNORE, ws2.data_ptr(), ws2.numel(), L.stream()), "dice_fwd")
    L.check(lib.mednet_ce_fwd(z.data_ptr(), lab.data_ptr(), wt.data_ptr(), lc.data_ptr(), sc.data_ptr(), n, c, sp, c * sp, sp, -100,
                              ws2.data_ptr(), ws2.numel(), L.stream()), "ce_fwd")
    torch.cuda.synchronize()
    assert torch.equal(saved[:2 * c], sd.flatten()) and torch.equal(saved[2 * c], sc[0]) and torch.equal(dice, dd)
    assert torch.equal(loss, ld + lc) and torch.isfinite(loss)


@pytest.mark.parametrize("bad,form", [(4, "u8"), (255, "u8"), (4, "i64"), (2 ** 32 + 1, "i64"), (-1, "i64")])
def test_out_of_range_label_poisons_loss_and_gradients(volumes, bad, form):
    """A label outside [0, C) -- C itself, 255, and an int64 that would narrow to class 1 -- gives a NaN loss and NaN gradients."""
    n, shape, wide, vol = volumes["ragged"]
    c = 4
    lab = _labels(vol, c, form).clone()
    lab[1, 2, 3, 4] = bad
    z = wide[:, :c].contiguous().requires_grad_(True)
    loss = ops.dice_ce_loss(z, lab, _weights(c).to(DEV))
    loss.backward()
    assert torch.isnan(loss) and torch.isnan(z.grad).all()


@pytest.mark.parametrize("c", [2, 4, 14])
@pytest.mark.parametrize("wtag", ["plain", "weight"])
def test_reference_pin(golden_dir, c, wtag):
    """tests/golden/dice_ce.npz (the reference's DiceLoss + torch.nn.CrossEntropyLoss) through HL.DiceCELoss: the bounds
    tests/test_gpu_ops.py holds the two single losses to against losses.npz (2e-6 on the loss, 1e-5 on dlogits); uint8 labels."""
    rec = np.load(os.path.join(golden_dir, "dice_ce.npz"))
    z = torch.from_numpy(rec[f"c{c}.logits"]).to(DEV).requires_grad_(True)
    y = torch.from_numpy(rec[f"c{c}.labels"]).to(DEV)
    w = torch.from_numpy(rec[f"c{c}.weight"]).to(DEV) if wtag == "weight" else None
    loss = HL.DiceCELoss(weight=w).to(DEV)(z, y)
    loss.backward()
    print(f"[dice_ce golden c{c}.{wtag}] loss {float(loss.detach()):.8f} / {float(rec[f'c{c}.{wtag}.loss']):.8f}")
    assert abs(float(loss.detach()) - float(rec[f"c{c}.{wtag}.loss"])) <= 2e-6
    assert_close(z.grad, torch.from_numpy(rec[f"c{c}.{wtag}.dlogits"]), 1e-5, "dlogits vs golden")


def test_sigmoid_and_shape_errors():
    with pytest.raises(ValueError):
        HL.DiceCELoss(sigmoid_normalization=True)
    z = rnd("dce-shape", 2, 3, 4, 4, 4).to(DEV)
    with pytest.raises(AssertionError, match="same shape"):
        ops.dice_ce_loss(z, torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="dice_ce_fwd"):
        ops.dice_ce_loss(rnd("dce-33", 1, 33, 2, 2, 2).to(DEV), torch.zeros((1, 2, 2, 2), dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------------------ the head for <= 4 classes
MODES = ["bf16", "fp16", "fp32"]
HEAD_SHAPES = [(3, (12, 10, 6)), (2, (24, 20, 21))]  # the digest tool's shapes


def _gscale(mode):
    return 3.0 * 16384.0 if mode == "fp16" else 3.0  # (fp16 stores the feature gradient: scaled as train.LossScaler does)


def _block_head(mode, cin, c, n, shape, lab, wt, fused):
    """ExtResNetBlock(cin, cin, 'cge') -> 1x1x1 head -> Dice + CE, fused or as final_conv + ops.dice_ce_loss."""
    with mednet_hip.precision(mode):
        blk = O.keyed_init_(HC.ExtResNetBlock(cin, cin, order="cge", num_groups=8)).to(DEV)
        conv = hnn.Conv3d(cin, c, 1, planar_output=True).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(rnd(f"hdw{cin}{c}", c, cin, 1, 1, 1, scale=0.3))
            conv.bias.copy_(rnd(f"hdb{c}", c))
        x = rnd(f"hdx{cin}{n}{shape}", n, cin, *shape).to(DEV).requires_grad_(True)
        feats = blk(x)
        if fused:
            assert ops.head_dice_ce_supported(feats, cin, c, lab)
            assert ops._gn3_hook_of(feats, feats.dtype) is not None, "the GroupNorm-3 hook is not live"
            lg, loss = ops.head_dice_ce(feats, conv.weight, conv.bias, conv._packed(), lab, wt, 1e-5)
        else:
            lg = conv(feats)
            loss = ops.dice_ce_loss(lg, lab, wt, 1e-5)
        (loss * _gscale(mode)).backward()
        torch.cuda.synchronize()
    return (lg.detach(), loss.detach(), x.grad, [p.grad for p in blk.parameters()], conv.weight.grad, conv.bias.grad)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin", [16, 32, 64])
@pytest.mark.parametrize("c", [1, 2, 4])
def test_fused_head_equals_the_unfused_launches_bit_for_bit(mode, cin, c):
    """ops.head_dice_ce against hnn.Conv3d(cin, C, 1, planar_output=True) + ops.dice_ce_loss behind an ExtResNetBlock('cge'), whose
    GroupNorm-3 backward takes its first pass from the head: logits, loss, the gradient of the block's input and every block
    parameter gradient are equal; dW / db are held to 1e-5 (their summation order differs by contract, the bound of the head_dice /
    head_ce tests).  Both shapes, each with uint8 labels as the last channel of a volume and with an int64 map."""
    for (n, shape), form in [(ns, f) for ns in HEAD_SHAPES for f in ("u8", "i64")]:
        g = np.random.Generator(np.random.PCG64(83 + c))
        vol = torch.from_numpy(g.integers(0, c, size=(n, 2) + shape).astype(np.uint8)).to(DEV)
        lab = vol[:, -1] if form == "u8" else vol[:, -1].long()
        wt = _weights(c).to(DEV)
        l1, s1, dx1, dp1, dw1, db1 = _block_head(mode, cin, c, n, shape, lab, wt, True)
        l0, s0, dx0, dp0, dw0, db0 = _block_head(mode, cin, c, n, shape, lab, wt, False)
        tag = f"{mode} cin={cin} C={c} {shape} {form}"
        assert torch.isfinite(s1) and torch.isfinite(dx1).all(), tag
        assert torch.equal(l1, l0), f"{tag}: logits differ"
        assert torch.equal(s1, s0), (tag, float(s1), float(s0))
        assert torch.equal(dx1, dx0), f"{tag}: the gradient of the block's input differs"
        for k, (a, b) in enumerate(zip(dp1, dp0)):
            assert torch.equal(a, b), f"{tag}: block parameter {k} gradient differs"
        assert_close(dw1, dw0, 1e-5, f"{tag}: dW fused vs unfused")
        assert_close(db1, db0, 1e-5, f"{tag}: db fused vs unfused")


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_fused_head_folds_the_activation_of_a_unet3d_last_block(mode):
    """SegmentationStep(loss='DICE_CE') on UNet3D ('gcr': the last block ends in conv -> ReLU, no GroupNorm-3 behind it): the FOLD
    form of the head's backward against the two-node step, every gradient in front of the head bit for bit."""
    from mednet_hip.train import SegmentationStep
    ctor = dict(in_channels=1, out_channels=4, final_sigmoid=False, f_maps=[32, 64])
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(2, 1, (24, 40, 32), 4, 0, seed=31).items()}
    res, old = {}, ops.FUSE_HEAD_LOSS
    try:
        for fused in (False, True):
            ops.FUSE_HEAD_LOSS = fused
            with mednet_hip.precision(mode):
                net = O.keyed_init_(HM.UNet3D(**ctor)).to(DEV)
                step = SegmentationStep(net, loss_weight=[0.05, 1.0, 1.0, 1.0], lr=1e-3, loss="DICE_CE")
                calls = {"n": 0, "folded": 0}
                real = ops.HeadDiceCEFn.apply

                def counted(*a):
                    calls["n"] += 1
                    calls["folded"] += int(getattr(a[0], "_mednet_actmask", None) is not None and ops._gn3_hook_of(a[0], a[0].dtype) is None)
                    return real(*a)
                ops.HeadDiceCEFn.apply = counted
                try:
                    (loss,) = step._fwd_bwd(batch)
                finally:
                    ops.HeadDiceCEFn.apply = real
                torch.cuda.synchronize()
                names = [(nm, off, p.numel()) for (nm, p), off in zip(net.named_parameters(), step.flat.offsets)]
                res[fused] = (float(loss), step.flat.grad.clone(), calls["n"], calls["folded"])
                step.flat.release()
    finally:
        ops.FUSE_HEAD_LOSS = old
    assert (res[True][2], res[True][3], res[False][2]) == (1, 1, 0), "the fused node / the activation fold was not (or wrongly) taken"
    assert res[True][0] == res[False][0], (res[True][0], res[False][0])
    for name, off, cnt in names:
        a, b = res[True][1][off:off + cnt], res[False][1][off:off + cnt]
        if name.startswith("final_conv."):
            assert_close(a, b, 1e-5, name)
        else:
            assert torch.equal(a, b), f"{name}: gradient differs between the fused and the two-node step"


def test_fused_head_out_of_range_label_and_refusals():
    with mednet_hip.precision("bf16"):
        conv = hnn.Conv3d(32, 2, 1, planar_output=True).to(DEV)
        x = ops.to_cl(rnd("hdce-bad", 2, 32, 8, 8, 8).to(DEV).bfloat16()).requires_grad_(True)
        lab = torch.zeros((2, 8, 8, 8), dtype=torch.uint8, device=DEV)
        _, ok = ops.head_dice_ce(x, conv.weight, conv.bias, conv._packed(), lab)
        lab[1, 3, 4, 5] = 2
        _, loss = ops.head_dice_ce(x, conv.weight, conv.bias, conv._packed(), lab)
        loss.backward()
        assert torch.isfinite(ok) and torch.isnan(loss) and torch.isnan(x.grad.float()).all()
        wide = hnn.Conv3d(32, 5, 1, planar_output=True).to(DEV)
        assert not ops.head_dice_ce_supported(x, 32, 5, lab)
        with pytest.raises(RuntimeError, match="head_dice_ce_fwd"):
            ops.head_dice_ce(x, wide.weight, wide.bias, wide._packed(), lab)


# ------------------------------------------------------------------------------------------------ footprint
def _same(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        assert not bool(torch.isnan(a.float()).any()), f"{what}: result {k} holds a NaN"
        assert torch.equal(a, b), f"{what}: result {k} differs from the unfenced call"


def _finish(fence, what, outputs, sites, ws_sites, ws_bytes):
    """Forward outputs live in slabs (a gradient may have been moved by autograd: its kernel's buffer is the slab from `sites`); every
    workspace request of the operator asked for exactly the query's bytes; every guard byte is intact."""
    for t in outputs:
        assert fence.owns(t), f"{what}: an output of shape {tuple(t.shape)} was not allocated inside the fence"
    seen = {s.site for s in fence.slabs}
    assert set(sites) <= seen, f"{what}: no fenced allocation from {sorted(set(sites) - seen)} (sites seen: {sorted(seen)})"
    asked = [r for r in fence.ws_requests if r[2] in ws_sites]
    assert len(asked) == len(ws_sites) and all(r[0] == ws_bytes and r[1] == ws_bytes for r in asked), (what, fence.ws_requests)
    fence.check()


@pytest.mark.parametrize("c,form", [(4, "u8"), (17, "i64")])
def test_one_pass_loss_inside_guard_bands(volumes, c, form):
    """ops.dice_ce_loss forward and backward with logits, labels, weight, every output and a workspace of exactly
    mednet_dice_ce_ws_bytes in slabs of their own: the uint8 label volume ENDS with the class map's last byte; equal to the unfenced
    run bit for bit, every guard byte intact."""
    n, shape, wide, vol = volumes["ragged"]
    sp = int(np.prod(shape))
    v = vol.clone()
    v[:, -1] %= c
    wt = _weights(c).to(DEV)

    def run(put):
        z = put(wide[:, :c].contiguous()).requires_grad_(True)
        lab = put(v)[:, -1] if form == "u8" else put(v[:, -1].long().contiguous())
        loss = ops.dice_ce_loss(z, lab, put(wt))
        loss.backward(put(torch.tensor(GSCALE, device=DEV)))
        torch.cuda.synchronize()
        return loss.detach(), z.grad
    want = run(lambda t: t)
    with Fence() as fence:
        got = run(fence.put)
        _same(got, want, f"dice_ce C={c} {form}")
        _finish(fence, f"dice_ce C={c} {form}", got[:1], ("_loss_grad_like",), ("forward",), L.lib().mednet_dice_ce_ws_bytes(n, c, sp))


@pytest.mark.parametrize("mode,cin,form", [("bf16", 32, "u8"), ("fp16", 16, "i64"), ("fp32", 64, "u8")])
def test_fused_head_inside_guard_bands(mode, cin, form):
    """ops.head_dice_ce forward and backward inside the fence: features, packed weights, bias, labels (the volume ends with them),
    logits, loss, saved, dz, dW, db and the workspace of exactly mednet_head_dice_ce_ws_bytes."""
    n, shape, c = 3, (12, 10, 6), 4
    sp = int(np.prod(shape))
    g = np.random.Generator(np.random.PCG64(87))
    vol = torch.from_numpy(g.integers(0, c, size=(n, 2) + shape).astype(np.uint8)).to(DEV)
    wt = _weights(c).to(DEV)

    def run(put):
        with mednet_hip.precision(mode):
            conv = hnn.Conv3d(cin, c, 1, planar_output=True).to(DEV)
            with torch.no_grad():
                conv.weight.copy_(rnd(f"hdw{cin}{c}", c, cin, 1, 1, 1, scale=0.3))
                conv.bias.copy_(rnd(f"hdb{c}", c))
            w, b = put(conv.weight.detach()).requires_grad_(True), put(conv.bias.detach()).requires_grad_(True)
            pk = ops.pack_conv_weight(w.detach(), 1, False)
            x = put(ops.to_cl(rnd(f"hdx{cin}{n}{shape}", n, cin, *shape).to(DEV).to(mednet_hip.config.act_dtype()))).requires_grad_(True)
            lab = put(vol)[:, -1] if form == "u8" else put(vol[:, -1].long().contiguous())
            lg, loss = ops.head_dice_ce(x, w, b, pk, lab, put(wt))
            loss.backward(put(torch.tensor(_gscale(mode), device=DEV)))
            torch.cuda.synchronize()
        return lg.detach(), loss.detach(), x.grad, w.grad, b.grad
    want = run(lambda t: t)
    with Fence() as fence:
        got = run(fence.put)
        what = f"head_dice_ce {mode} cin={cin} {form}"
        _same(got, want, what)
        _finish(fence, what, got[:2], ("_grad_target", "__init__"), ("_valu_head_fwd", "__init__"),
                L.lib().mednet_head_dice_ce_ws_bytes(n, sp, cin, c))
