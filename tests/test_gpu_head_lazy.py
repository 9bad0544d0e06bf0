"""The head junction without the head's feature gradient in memory (-m gpu): mednet_head_{dice,ce,dice_ce}_bwd_sums take the sums
of the small fused head's backward and store no dz; mednet_gn_act_bwd_fused_res_head, the GroupNorm-3 apply pass of the block in
front, rebuilds each row of dz from the voxel's logits, its label and the head weights.  Everything here is an EQUALITY of bits:

1. sums       gn_partial, dW and db of the sums-only entry == those of the storing entry on the same inputs;
2. rebuild    dy3, dres, dgamma, dbeta of mednet_gn_act_bwd_fused_res_head == mednet_gn_act_bwd_fused_res fed with the dz the storing
              entry wrote;
3. one logit gradient per voxel (the quad of lanes that owns a voxel shares it): the storing entry's dz == the unfused launches'
              (the stand-alone loss backward of loss.hip, one evaluation per voxel and lane, + mednet_head_dgrad_gn);
4. footprint  the new entry points run inside guard bands (tests/fence.py: outputs and exact-size workspaces), and through ops the
              placeholder gradient tensor still holds the fence's pattern after the lazy backward;
5. end to end a small ResidualUNet3D through SegmentationStep: loss, every gradient and the parameters after one Adam step with
              ops.LAZY_HEAD (MEDNET_LAZY_HEAD) on == off; ops.GN3_COUNT["lazy_head"] says which path ran;
6. fallbacks  a tensor hook / retain_grad() on the block output, a second consumer of it (a forward hook on the last decoder), fp32
              storage and a hand-made ops.GN3Hook() all take the stored path.

Shapes (32 features; a head workgroup takes 2048 voxels, an apply chunk 512, both two voxels per lane and trip): 8 x 8 x 16 (whole
trips), 5 x 7 x 9 (315 voxels: a last trip with one voxel, a ragged workgroup) and 9 x 11 x 43 (three head workgroups and nine apply
chunks per sample, the last ones ragged)."""
import numpy as np
import pytest
import torch

import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import ops
from mednet_hip.unet import model as HM
from mednet_hip.unet.components import ExtResNetBlock
from mednet_hip import nn as hnn
from oracle import ref_cpu as O

from fence import Fence
from gpu_util import DEV, DT, half_round, rnd
import test_gpu_head_backward as HB

pytestmark = pytest.mark.gpu
CL = torch.channels_last_3d
CIN, GROUPS, N = 32, 8, 2
SHAPES = [(8, 8, 16), (5, 7, 9), (9, 11, 43)]
# (loss, ignore_index): where the kind allows one, set (a class that occurs) and unset
LOSSES = [("DICE", None), ("DICE", 1), ("CE", None), ("CE", 1), ("DICE_CE", None)]
NAME = {"DICE": "head_dice", "CE": "head_ce", "DICE_CE": "head_dice_ce"}
KIND = {"DICE": L.CLASS_DICE, "CE": L.CLASS_CE, "DICE_CE": L.CLASS_DICE_CE}
WEIGHT = [0.05, 1.0, 0.7, 1.3]
EPS = 1e-5


def _scalars(kind, ii):
    """The arguments between cout and the dtype of mednet_<name>_fwd / _bwd / _bwd_sums."""
    return (ii,) if kind == "CE" else (EPS, 0, ii)


def _ignore_code(kind, ignore):
    if kind == "DICE_CE":
        return L.NO_IGNORE
    return (L.NO_IGNORE if kind == "DICE" else -100) if ignore is None else ignore


def _forward(lib, kind, zg, pk, bias, lab, lab_dt, lab_sn, wt, spatial, cout, ii, dcode):
    name = NAME[kind]
    logits = HB.nan_like((N, cout) + tuple(zg.shape[2:]), torch.float32)
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    saved = torch.zeros(2 * cout + 1, dtype=torch.float32, device=DEV)
    ws = L.workspace(getattr(lib, f"mednet_{name}_ws_bytes")(N, spatial, CIN, cout), zg.device)
    L.check(getattr(lib, f"mednet_{name}_fwd")(zg.data_ptr(), pk.data_ptr(), bias.data_ptr(), lab.data_ptr(), lab_dt, lab_sn, wt.data_ptr(),
                                               logits.data_ptr(), loss.data_ptr(), saved.data_ptr(), N, spatial, CIN, cout,
                                               *_scalars(kind, ii), dcode, ws.data_ptr(), ws.numel(), L.stream()), name + "_fwd")
    return logits, saved


def _backward(lib, kind, store, alloc, workspace, logits, saved, zg, gyg, pk, lab, lab_dt, lab_sn, wt, dl, act, spatial, cout, ii, dt, dcode):
    """mednet_<name>_bwd (store) or mednet_<name>_bwd_sums -> (dz or None, gn_partial, dW, db); outputs from alloc(shape, dtype, cl)."""
    name = NAME[kind]
    rows = getattr(lib, f"mednet_{name}_gn_rows")(N, spatial, CIN)
    ws = workspace(getattr(lib, f"mednet_{name}_ws_bytes")(N, spatial, CIN, cout))
    part, dw, db = alloc((N, rows, CIN, 2), torch.float32), alloc((cout, CIN), torch.float32), alloc((cout,), torch.float32)
    head = (logits.data_ptr(), lab.data_ptr(), lab_dt, lab_sn, pk.data_ptr(), wt.data_ptr(), saved.data_ptr(), dl.data_ptr())
    tail = (gyg.data_ptr(), zg.data_ptr(), act, part.data_ptr(), dw.data_ptr(), db.data_ptr(), N, spatial, CIN, cout, *_scalars(kind, ii),
            dcode, ws.data_ptr(), ws.numel(), L.stream())
    if store:
        dz = alloc(tuple(zg.shape), dt, True)
        L.check(getattr(lib, f"mednet_{name}_bwd")(*head, dz.data_ptr(), *tail), name + "_bwd")
        return dz, part, dw, db
    L.check(getattr(lib, f"mednet_{name}_bwd_sums")(*head, *tail), name + "_bwd_sums")
    return None, part, dw, db


def _plain_alloc(shape, dtype, cl=False):
    return HB.nan_like(shape, dtype, cl=cl)


def _unfused_dz(lib, kind, zg, pk, bias, lab, lab_dt, lab_sn, lab64, wt, gyg, act, shape, cout, dcode, dl, ii, dt):
    """dz and the GroupNorm rows of the unfused launches: the head, the stand-alone loss backward, mednet_head_dgrad_gn."""
    if kind != "DICE_CE":
        out = HB._unfused(lib, kind, zg, pk, bias, lab, lab_dt, lab_sn, lab64, wt, gyg, act, N, shape, CIN, cout, dcode, dl, EPS, False, ii, dt)
        return out[4], out[5]
    d, h, w = shape
    spatial = d * h * w
    logits = HB.nan_like((N, cout, d, h, w), torch.float32)
    L.check(lib.mednet_conv3d_fwd(zg.data_ptr(), pk.data_ptr(), bias.data_ptr(), logits.data_ptr(), N, d, h, w, CIN, cout, 1, dcode,
                                  L.NDHWC, L.F32, L.NCDHW, 0, mednet_hip.config.conv_algo(), None, L.stream()), "conv3d_fwd")
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    saved = torch.zeros(2 * cout + 1, dtype=torch.float32, device=DEV)
    ws = L.workspace(lib.mednet_dice_ce_ws_bytes(N, cout, spatial), zg.device)
    dlg = HB.nan_like((N, cout, d, h, w), torch.float32)
    sn, sc = cout * spatial, spatial
    L.check(lib.mednet_dice_ce_fwd_lt(logits.data_ptr(), lab.data_ptr(), lab_dt, lab_sn, wt.data_ptr(), loss.data_ptr(), saved.data_ptr(),
                                      None, N, cout, spatial, sn, sc, EPS, ws.data_ptr(), ws.numel(), L.stream()), "dice_ce_fwd_lt")
    L.check(lib.mednet_dice_ce_bwd_lt(logits.data_ptr(), lab.data_ptr(), lab_dt, lab_sn, wt.data_ptr(), saved.data_ptr(), dl.data_ptr(),
                                      dlg.data_ptr(), N, cout, spatial, sn, sc, EPS, L.stream()), "dice_ce_bwd_lt")
    rows = lib.mednet_head_dgrad_gn_rows(N, d, h, w, CIN, dcode)
    dz = HB.nan_like((N, CIN, d, h, w), dt, cl=True)
    part = HB.nan_like((N, rows, CIN, 2), torch.float32)
    L.check(lib.mednet_head_dgrad_gn(dlg.data_ptr(), pk.data_ptr(), dz.data_ptr(), gyg.data_ptr(), zg.data_ptr(), act, part.data_ptr(),
                                     N, d, h, w, CIN, cout, dcode, L.stream()), "head_dgrad_gn")
    return dz, part


def _gn_operands(lib, tag, gyg, spatial, dcode):
    """GroupNorm-3's forward results on gy (its input y3) and an affine: stats [n][g][2], coef [n][c][2], gamma."""
    gamma, beta = (1.0 + 0.25 * rnd(tag + "ga", CIN)).to(DEV), rnd(tag + "be", CIN).to(DEV)
    stats = torch.empty((N, GROUPS, 2), dtype=torch.float32, device=DEV)
    coef = torch.empty((N, CIN, 2), dtype=torch.float32, device=DEV)
    ws = L.workspace(lib.mednet_gn_ws_bytes(N, CIN, spatial), gyg.device)
    L.check(lib.mednet_gn_stats(gyg.data_ptr(), gamma.data_ptr(), beta.data_ptr(), stats.data_ptr(), coef.data_ptr(), N, spatial, CIN,
                                GROUPS, 1e-5, dcode, ws.data_ptr(), ws.numel(), L.stream()), "gn_stats")
    return gamma, stats, coef


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_sums_only_backward_and_rebuilding_apply_pass_equal_the_stored_path(mode, shape):
    """Items 1 - 4 of the module docstring at kernel level; classes, losses, ignore_index, label forms and activations looped inside."""
    lib = L.lib()
    dt, dcode = DT[mode], L.dt_of(DT[mode])
    d, h, w = shape
    spatial = d * h * w
    tag = f"hlz{shape}"
    u = rnd(tag + "u", N, CIN, *shape)
    gy = half_round(rnd(tag + "y", N, CIN, *shape), mode)
    gyg = HB.to_dev_cl(gy, dt)
    dl = torch.tensor(HB.gscale_of(mode), dtype=torch.float32, device=DEV)
    compared = 0
    with mednet_hip.precision(mode):
        gamma, stats, coef = _gn_operands(lib, tag, gyg, spatial, dcode)
        gn_bytes = lib.mednet_gn_ws_bytes(N, CIN, spatial)
        for act in (L.ACT_ELU, L.ACT_RELU):
            zg = HB.to_dev_cl(HB.act_output(u, act, mode), dt)
            for cout in (2, 3, 4):
                assert lib.mednet_gn_act_bwd_fused_res_head_supported(CIN, cout, dcode, L.U8) == 1
                assert lib.mednet_gn_act_bwd_fused_res_head_supported(CIN, cout, dcode, L.I64) == 1
                wgt, bias = rnd(tag + f"w{cout}", cout, CIN, 1, 1, 1, scale=0.3), rnd(tag + f"b{cout}", cout).to(DEV)
                pk = ops.pack_conv_weight(wgt.to(DEV), 1, False)
                wt = torch.tensor(WEIGHT[:cout], device=DEV)
                g = np.random.Generator(np.random.PCG64(17 + cout))
                vol = torch.from_numpy(g.integers(0, cout, size=(N, 2) + shape).astype(np.uint8)).to(DEV)
                lab_u8, lab64 = vol[:, -1], vol[:, -1].long().contiguous()
                for kind, ignore in LOSSES:
                    ii = _ignore_code(kind, ignore)
                    for lab, lab_dt, lab_sn in ((lab_u8, L.U8, 2 * spatial), (lab64, L.I64, spatial)):
                        what = f"{kind} C={cout} ignore={ignore} {mode} {shape} labels={lab_dt} act={HB.ACT_NAME[act]}"
                        logits, saved = _forward(lib, kind, zg, pk, bias, lab, lab_dt, lab_sn, wt, spatial, cout, ii, dcode)
                        common = (logits, saved, zg, gyg, pk, lab, lab_dt, lab_sn, wt, dl, act, spatial, cout, ii, dt, dcode)
                        dz, part, dw, db = _backward(lib, kind, True, _plain_alloc, lambda nb: L.workspace(nb, zg.device), *common)
                        # 3. the storing kernel's dz (one logit gradient per voxel, shared by its quad) against the unfused launches
                        dz0, part0 = _unfused_dz(lib, kind, zg, pk, bias, lab, lab_dt, lab_sn, lab64, wt, gyg, act, shape, cout, dcode, dl, ii, dt)
                        torch.cuda.synchronize()
                        assert not bool(torch.isnan(dz0).any()) and torch.equal(dz, dz0), what + ": dz differs from the unfused dz"
                        assert torch.equal(part, part0), what + ": gn_partial differs from mednet_head_dgrad_gn's rows"
                        # the stored path's apply pass on that dz
                        dx0, dres0 = HB.nan_like(tuple(zg.shape), dt, cl=True), HB.nan_like(tuple(zg.shape), dt, cl=True)
                        dg0, dbe0 = HB.nan_like((CIN,), torch.float32), HB.nan_like((CIN,), torch.float32)
                        ws0 = L.workspace(gn_bytes, zg.device)
                        L.check(lib.mednet_gn_act_bwd_fused_res(dz.data_ptr(), gyg.data_ptr(), zg.data_ptr(), coef.data_ptr(), stats.data_ptr(),
                                                                gamma.data_ptr(), part.data_ptr(), part.shape[1], dx0.data_ptr(), dres0.data_ptr(),
                                                                dg0.data_ptr(), dbe0.data_ptr(), N, spatial, CIN, GROUPS, act, dcode,
                                                                ws0.data_ptr(), ws0.numel(), L.stream()), "gn_act_bwd_fused_res")
                        with Fence() as fence:
                            def alloc(shp, dtype, cl=False):
                                return fence.alloc(shp, dtype, memory_format=CL if cl else None)
                            # 1. the sums-only entry
                            _, part1, dw1, db1 = _backward(lib, kind, False, alloc, fence.workspace, *common)
                            # 2. the apply pass that rebuilds dz
                            dx1, dres1 = alloc(tuple(zg.shape), dt, True), alloc(tuple(zg.shape), dt, True)
                            dg1, dbe1 = alloc((CIN,), torch.float32), alloc((CIN,), torch.float32)
                            ws1 = fence.workspace(gn_bytes)
                            eps, sigmoid = (0.0, 0) if kind == "CE" else (EPS, 0)
                            L.check(lib.mednet_gn_act_bwd_fused_res_head(logits.data_ptr(), lab.data_ptr(), lab_dt, lab_sn, pk.data_ptr(),
                                                                         wt.data_ptr(), saved.data_ptr(), dl.data_ptr(), eps, sigmoid, ii,
                                                                         KIND[kind], cout, gyg.data_ptr(), zg.data_ptr(), stats.data_ptr(),
                                                                         gamma.data_ptr(), part1.data_ptr(), part1.shape[1], dx1.data_ptr(),
                                                                         dres1.data_ptr(), dg1.data_ptr(), dbe1.data_ptr(), N, spatial, CIN,
                                                                         GROUPS, act, dcode, ws1.data_ptr(), ws1.numel(), L.stream()),
                                    "gn_act_bwd_fused_res_head")
                            fence.check()   # 4. nothing outside the outputs and the exact-size workspaces was written
                        for name, a, b in (("gn_partial", part1, part), ("dW", dw1, dw), ("db", db1, db)):
                            assert not bool(torch.isnan(a).any()) and torch.equal(a, b), f"{what}: {name} of the sums-only entry differs"
                        for name, a, b in (("dy3", dx1, dx0), ("dres", dres1, dres0), ("dgamma", dg1, dg0), ("dbeta", dbe1, dbe0)):
                            assert not bool(torch.isnan(b).any()), f"{what}: {name} of the stored path has NaN"
                            assert torch.equal(a, b), f"{what}: {name} of the rebuilding apply pass differs from the stored path"
                        compared += 2 * dz.numel() + part.numel()
    print(f"[exact] item=head_lazy {shape} {mode} kernel=gn_bwd_apply_head_kernel elements={compared}")


# ---------------------------------------------------------------------------------------------- through ops: block + head
def _block_and_head(mode, kind, lazy, mark=True, after=None, fence=None):
    """ExtResNetBlock(32, 32) -> ops.head_<kind> on (2, 32, 8, 8, 16); `mark`: the block is told that the head is the sole consumer
    (head_next).  `after(out)`: called on the block output before the head (-> extra loss term or None).  -> (loss, gradients of the
    block's and the head's parameters and of the input, GN3_COUNT deltas, the gradient tensor the head offered to the hook)."""
    old, old_offer = ops.LAZY_HEAD, ops.GN3Hook.offer
    seen = {}

    def spy(self, dx, partial, lazy=None):
        seen["dx"], seen["lazy"] = dx, lazy
        return old_offer(self, dx, partial, lazy)
    try:
        ops.LAZY_HEAD = lazy
        ops.GN3Hook.offer = spy
        with mednet_hip.precision(mode):
            torch.manual_seed(3)
            blk = O.keyed_init_(ExtResNetBlock(32, 32)).to(DEV)
            conv = hnn.Conv3d(32, 3, 1, planar_output=True).to(DEV)
            x = rnd("hlz-x", N, 32, 8, 8, 16).to(DEV).requires_grad_(True)
            g = np.random.Generator(np.random.PCG64(5))
            lab = torch.from_numpy(g.integers(0, 3, size=(N, 8, 8, 16)).astype(np.uint8)).to(DEV)
            wt = torch.tensor(WEIGHT[:3], device=DEV)
            before = dict(ops.GN3_COUNT)
            out = blk(x, head_next=True) if mark else blk(x)
            extra = after(out) if after is not None else None
            call = {"DICE": ops.head_dice, "CE": ops.head_ce, "DICE_CE": ops.head_dice_ce}[kind]
            _, loss = call(out, conv.weight, conv.bias, conv._packed(), lab, wt)
            total = loss * HB.gscale_of(mode) + (extra if extra is not None else 0.0)
            if fence is not None:
                with fence:
                    total.backward()
                    fence.check()
            else:
                total.backward()
            torch.cuda.synchronize()
            grads = [p.grad.clone() for p in list(blk.parameters()) + list(conv.parameters())] + [x.grad.clone()]
            delta = {k: ops.GN3_COUNT[k] - before[k] for k in before}
    finally:
        ops.LAZY_HEAD, ops.GN3Hook.offer = old, old_offer
    return float(loss.detach()), grads, delta, seen


def _same(a, b, what):
    assert a[0] == b[0], f"{what}: loss {a[0]} against {b[0]}"
    for i, (p, q) in enumerate(zip(a[1], b[1])):
        assert not bool(torch.isnan(p).any()) and torch.equal(p, q), f"{what}: gradient {i} differs"


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["DICE", "CE", "DICE_CE"])
def test_the_placeholder_gradient_stays_unwritten_and_nothing_changes(mode, kind):
    """Item 4 through ops: the backward runs inside a fence, so the placeholder comes from the fenced torch.empty_like and holds the
    pattern (0x7FC0 in every 16-bit element) -- after the backward it still does, no guard band changed, and every gradient equals
    the stored path's."""
    stored = _block_and_head(mode, kind, lazy=False)
    fence = Fence()
    lazy = _block_and_head(mode, kind, lazy=True, fence=fence)
    assert stored[2]["lazy_head"] == 0 and stored[2]["taken"] == 1 and stored[3]["lazy"] is None
    assert lazy[2]["lazy_head"] == 1 and lazy[2]["taken"] == 1 and lazy[2]["declined"] == 0 and lazy[3]["lazy"][0] == "head"
    dx = lazy[3]["dx"]
    assert fence.owns(dx) and dx.shape == (N, 32, 8, 8, 16)
    words = dx.permute(0, 2, 3, 4, 1).contiguous().view(torch.int16)
    assert bool((words == 0x7FC0).all()), "the lazy backward wrote into the placeholder gradient"
    assert not bool(torch.isnan(stored[3]["dx"]).any())
    _same(lazy, stored, f"{kind} {mode} lazy against stored")


@pytest.mark.parametrize("how", ["tensor_hook", "retain_grad", "unmarked", "fp32"])
def test_fallbacks_of_the_block_and_head_pair_take_the_stored_path(how):
    """Item 6 at the junction: what reads the gradient of the block output (a tensor hook, retain_grad()), a hook nobody marked (what a
    hand-made ops.GN3Hook() is: lazy_head_ok is False) and fp32 storage keep the gradient materialised, with the gradients of the
    run with the knob off."""
    mode = "fp32" if how == "fp32" else "bf16"
    box = {}

    def keep(g):
        box["grad"] = g.clone()

    def after(out):
        if how == "tensor_hook":
            out.register_hook(keep)
        elif how == "retain_grad":
            out.retain_grad()
            box["out"] = out
        return None
    runs = {lazy: _block_and_head(mode, "DICE", lazy=lazy, mark=how != "unmarked", after=after) for lazy in (False, True)}
    assert runs[True][2]["lazy_head"] == 0 and runs[True][3]["lazy"] is None, runs[True][2]
    assert runs[True][2] == runs[False][2]   # (the hook is asked, and answers, as with the knob off)
    _same(runs[True], runs[False], how)
    if how == "tensor_hook":
        assert torch.equal(box["grad"], runs[True][3]["dx"])
    if how == "retain_grad":
        assert torch.equal(box["out"].grad, runs[True][3]["dx"])


def test_a_second_consumer_of_a_marked_block_output_is_an_error():
    """head_next=True is a contract of the caller (the U-Net's own forward checks for forward hooks before it gives it); breaking it
    must not yield a silently wrong gradient."""
    with pytest.raises(RuntimeError, match="MEDNET_LAZY_HEAD"):
        _block_and_head("bf16", "DICE", lazy=True, after=lambda out: 1e-3 * out.float().square().mean())


# ---------------------------------------------------------------------------------------------- end to end
def _step_once(mode, lazy, loss="DICE", hooked=False):
    from mednet_hip.train import SegmentationStep
    ctor = dict(in_channels=1, out_channels=3, final_sigmoid=False, f_maps=[32, 64])
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(2, 1, (16, 16, 16), 3, 0, seed=7).items()}
    old = ops.LAZY_HEAD
    try:
        ops.LAZY_HEAD = lazy
        before = dict(ops.GN3_COUNT)
        with mednet_hip.precision(mode):
            net = O.keyed_init_(HM.ResidualUNet3D(**ctor)).to(DEV)
            seen = []
            if hooked:   # a second consumer of the last block's output may exist: a forward hook on the last decoder saw it
                net.decoders[-1].register_forward_hook(lambda m, i, o: seen.append(o))
            step = SegmentationStep(net, loss_weight=[0.05, 1.0, 1.0], lr=1e-3, loss=loss)
            out = step(batch)
            torch.cuda.synchronize()
            res = (float(out), step.flat.grad.clone(), step.flat.flat.clone(), {k: ops.GN3_COUNT[k] - before[k] for k in before})
            step.flat.release()
    finally:
        ops.LAZY_HEAD = old
    return res


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("loss", ["DICE", "CE", "DICE_CE"])
def test_a_training_step_is_the_same_with_and_without_the_stored_gradient(mode, loss):
    """Item 5: ResidualUNet3D(f_maps=[32, 64]) on 2 x 16^3 through SegmentationStep, one Adam step."""
    stored, lazy = _step_once(mode, False, loss), _step_once(mode, True, loss)
    assert stored[3]["lazy_head"] == 0 and lazy[3]["lazy_head"] == 1, (stored[3], lazy[3])
    assert lazy[3]["taken"] == stored[3]["taken"] and lazy[3]["declined"] == stored[3]["declined"] == 0
    assert lazy[0] == stored[0] and not np.isnan(lazy[0])
    assert torch.equal(lazy[1], stored[1]), "a gradient differs"
    assert torch.equal(lazy[2], stored[2]), "a parameter differs after the Adam step"


@pytest.mark.parametrize("how", ["forward_hook", "fp32"])
def test_a_training_step_falls_back_to_the_stored_gradient(how):
    """Item 6 in the network: a forward hook on the last decoder (a possible second consumer) and fp32 storage."""
    mode = "fp32" if how == "fp32" else "bf16"
    stored, lazy = _step_once(mode, False, hooked=how == "forward_hook"), _step_once(mode, True, hooked=how == "forward_hook")
    assert lazy[3]["lazy_head"] == 0 and lazy[3] == stored[3], lazy[3]
    assert lazy[0] == stored[0] and torch.equal(lazy[1], stored[1]) and torch.equal(lazy[2], stored[2])
